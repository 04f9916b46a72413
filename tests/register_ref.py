"""numpy / scipy restatement of detection_3d_amd/csrc/register.hip's semantics, in the style of
tests/clean_ref.py.

nearest_ref: the candidates of a query come from a k-d tree at 1.001 r; d2 is recomputed IN FP32 IN THE KERNEL'S
OPERATION ORDER, (dx dx + dy dy) + dz dz with dx = C.x - Q.x, and compared as unsigned integers, so every output bit
is reproduced and no point is excused.  step_ref: one Gauss-Newton step in fp64 with the header's formulas, operation
by operation (numpy does not contract a product and a sum); only the order of the 29 sums differs from the kernels',
and the sums of the terms' magnitudes are returned so that a test can bound that difference.  icp_ref: the loop."""
import itertools
import math

import numpy as np
from scipy.spatial import cKDTree

U = 2.0 ** -53
PIVOT_REL = 1e-12


def r2_bits(radius):
    r = np.float32(radius)
    return int(np.float32(r * r).view(np.uint32))


def d2_f32(c, q):
    """fp32 [K, 3] cloud rows, fp32 [K, 3] (or [3]) queries -> fp32 [K]: the kernel's distance"""
    c, q = np.asarray(c, np.float32), np.asarray(q, np.float32)
    with np.errstate(all="ignore"):
        dx, dy, dz = c[..., 0] - q[..., 0], c[..., 1] - q[..., 1], c[..., 2] - q[..., 2]
        return (dx * dx + dy * dy) + dz * dz


def nearest_ref(query, cloud, radius):
    """query fp32 [M, >= 3], cloud fp32 [N, >= 3] -> (index int32 [M], dist2 fp32 [M]): the cloud row with the smallest
    (bits of d2, row) among those with bits(d2) <= bits(r r); -1 / +inf for none, for a query that is not finite; a
    cloud row that is not finite is never a neighbour."""
    q = np.ascontiguousarray(np.asarray(query, np.float32)[:, :3])
    c = np.ascontiguousarray(np.asarray(cloud, np.float32)[:, :3])
    m = q.shape[0]
    index = np.full(m, -1, np.int32)
    dist2 = np.full(m, np.inf, np.float32)
    rows = np.flatnonzero(np.isfinite(c).all(1))
    live = np.flatnonzero(np.isfinite(q).all(1))
    if rows.size == 0 or live.size == 0:
        return index, dist2
    r = float(np.float32(radius))
    balls = cKDTree(c[rows].astype(np.float64)).query_ball_point(q[live].astype(np.float64), 1.001 * r, workers=-1)
    lens = np.fromiter((len(b) for b in balls), np.int64, live.size)
    total = int(lens.sum())
    if total == 0:
        return index, dist2
    cand = rows[np.fromiter(itertools.chain.from_iterable(balls), np.int64, total)]
    owner = np.repeat(live, lens)                     # the pairs of a query are consecutive
    bits = d2_f32(c[cand], q[owner]).view(np.uint32)
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    key = (bits.astype(np.uint64) << np.uint64(32)) | cand.astype(np.uint64)      # the minimum of (bits, row)
    key[bits > np.uint32(r2_bits(radius))] = none
    some = lens > 0
    best = np.minimum.reduceat(key, (np.cumsum(lens) - lens)[some])
    found = best != none
    who = live[some][found]
    index[who] = (best[found] & np.uint64(0xFFFFFFFF)).astype(np.int32)
    dist2[who] = (best[found] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return index, dist2


def transform_ref(pose, source):
    """-> (p' fp64 [M, 3] = ((R_k0 x + R_k1 y) + R_k2 z) + t_k, the queries fp32(p'))"""
    T = np.asarray(pose, np.float64).reshape(4, 4)
    s = np.asarray(source, np.float32)[:, :3].astype(np.float64)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    with np.errstate(all="ignore"):
        p = np.stack([((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3] for k in range(3)], 1)
        return p, p.astype(np.float32)


def _rows(p, q, nrm, method):
    """the Jacobian rows [K, 6] and residuals [K] of the pairs, and the number of contributing pairs"""
    d = p - q
    if method == "plane":
        ok = np.isfinite(nrm).all(1) & (nrm != 0).any(1)
        p, d, n = p[ok], d[ok], nrm[ok]
        r = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
        J = np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2],
                      p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]], 1)
        return J, r, p.shape[0]
    k = p.shape[0]
    zero, one = np.zeros(k), np.ones(k)
    J0 = np.stack([zero, p[:, 2], -p[:, 1], one, zero, zero], 1)
    J1 = np.stack([-p[:, 2], zero, p[:, 0], zero, one, zero], 1)
    J2 = np.stack([p[:, 1], -p[:, 0], zero, zero, zero, one], 1)
    return np.concatenate([J0, J1, J2]), np.concatenate([d[:, 0], d[:, 1], d[:, 2]]), k


def system_matrix(system):
    """the 29 sums -> (A [6, 6] symmetric, b [6], e, c)"""
    A = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = system[k]
            k += 1
    return A, np.asarray(system[21:27], np.float64), float(system[27]), float(system[28])


def solve_ref(system, pose, tol):
    """the kernel's solve and update -> (new pose [4, 4], status, |w|, |v|)"""
    A, g, e, c = system_matrix(system)
    T = np.array(pose, np.float64).reshape(4, 4)
    top = max(A[a, a] for a in range(6))
    L = np.zeros((6, 6))
    degenerate = not c >= 6.0
    for a in range(6):
        if degenerate:
            break
        d = A[a, a]
        for j in range(a):
            d -= L[a, j] * L[a, j]
        if not d > PIVOT_REL * top:
            degenerate = True
            break
        L[a, a] = math.sqrt(d)
        for i in range(a + 1, 6):
            s = A[i, a]
            for j in range(a):
                s -= L[i, j] * L[a, j]
            L[i, a] = s / L[a, a]
    if degenerate:
        return T, 2, 0.0, 0.0
    y, x = np.zeros(6), np.zeros(6)
    for i in range(6):
        s = -g[i]
        for j in range(i):
            s -= L[i, j] * y[j]
        y[i] = s / L[i, i]
    for i in range(5, -1, -1):
        s = y[i]
        for j in range(i + 1, 6):
            s -= L[j, i] * x[j]
        x[i] = s / L[i, i]
    th2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]
    wn = math.sqrt(th2)
    vn = math.sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5])
    if not (math.isfinite(wn) and math.isfinite(vn)):
        return T, 2, 0.0, 0.0
    if th2 < 1e-16:
        ca, cb = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        sh = math.sin(0.5 * wn)
        ca, cb = math.sin(wn) / wn, 2.0 * sh * sh / th2
    K = np.array([[0.0, -x[2], x[1]], [x[2], 0.0, -x[0]], [-x[1], x[0], 0.0]])
    dR = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            dR[i, j] = ((1.0 if i == j else 0.0) + ca * K[i, j]) + cb * (x[i] * x[j] - (th2 if i == j else 0.0))
    out = T.copy()
    for i in range(3):
        for j in range(4):
            out[i, j] = ((dR[i, 0] * T[0, j] + dR[i, 1] * T[1, j]) + dR[i, 2] * T[2, j]) + (x[3 + i] if j == 3 else 0.0)
    return out, (1 if wn <= tol and vn <= tol else 0), wn, vn


def step_ref(pose, source, target, normals, max_dist, method="plane", tol=1e-6):
    """One step from `pose` -> dict: index int32 [M] (the pairs), system fp64 [29], magnitude fp64 [29] (the sums of the
    terms' absolute values), pose [4, 4] after the step, status, c, e, wn, vn."""
    p, q32 = transform_ref(pose, source)
    index, _ = nearest_ref(q32, target, max_dist)
    sel = np.flatnonzero(index >= 0)
    t = index[sel]
    tq = np.asarray(target, np.float32)[t, :3].astype(np.float64)
    nrm = np.asarray(normals, np.float32)[t, :3].astype(np.float64) if method == "plane" else None
    J, r, c = _rows(p[sel], tq, nrm, method)
    terms = [J[:, a] * J[:, b] for a in range(6) for b in range(a, 6)] + [J[:, a] * r for a in range(6)] + [r * r]
    system = np.array([v.sum() for v in terms] + [float(c)])
    magnitude = np.array([np.abs(v).sum() for v in terms] + [float(c)])
    new_pose, status, wn, vn = solve_ref(system, pose, tol)
    return dict(index=index, system=system, magnitude=magnitude, pose=new_pose, status=status, c=c, e=system[27], wn=wn,
                vn=vn)


def icp_ref(source, target, normals, init=None, max_dist=0.1, iterations=30, tol=1e-6, method="plane"):
    """-> (pose [4, 4], steps, status, history: the dicts of step_ref per executed step)"""
    pose = np.eye(4) if init is None else np.array(init, np.float64).reshape(4, 4)
    history, status = [], 0
    for _ in range(iterations):
        s = step_ref(pose, source, target, normals, max_dist, method, tol)
        history.append(s)
        pose, status = s["pose"], s["status"]
        if status != 0:
            break
    return pose, len(history), status, history


# ---- motions and their errors ----
def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def motion_about(centre, axis, angle, shift):
    """the pose that rotates by `angle` about `axis` through `centre` and then shifts by `shift`"""
    R = rodrigues(axis, angle)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = np.asarray(centre) - R @ np.asarray(centre) + np.asarray(shift, np.float64)
    return T


def move(pose, xyz):
    """fp32 [N, 3] moved in fp64 and rounded once"""
    T = np.asarray(pose, np.float64)
    return (np.asarray(xyz, np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


def pose_errors(pose, truth, centre):
    """-> (the angle of the rotation between the two poses in radians, the distance between the two images of centre)"""
    P, Q = np.asarray(pose, np.float64), np.asarray(truth, np.float64)
    dR = P[:3, :3] @ Q[:3, :3].T
    s = 0.5 * np.linalg.norm([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    c = np.asarray(centre, np.float64)
    return math.atan2(s, 0.5 * (np.trace(dR) - 1.0)), float(np.linalg.norm((P[:3, :3] @ c + P[:3, 3]) - (Q[:3, :3] @ c + Q[:3, 3])))
