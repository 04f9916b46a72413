"""numpy restatement of d3d_manhattan_frame (include/d3d_hip.h) and the scenes its tests use.  Imports nothing from the
package; written from the definition, not from the kernel.

Definition.  A row (n0, n1, n2) of fp32 normals has m = (n0 n0 + n1 n1) + n2 n2 and votes iff 0.5 <= m <= 2.  Its vote
for a unit direction u with tolerance s2 (fp32): d = (n0 u0 + n1 u1) + n2 u2, a2 = d d, r = min(a2, max(m - a2, 0)),
v = max(s2 - r, 0), the integer trunc(v 2^30); every product and sum an fp32 operation of its own.  Scores are int64 sums.

rot(v), the smallest rotation that takes (0, 0, 1) to the unit vector v, with a = 1 + v2, every entry + 0.0:
    [[1 - (v0 v0) / a, -(v0 v1) / a, v0], [-(v0 v1) / a, 1 - (v1 v1) / a, v1], [-v0, -v1, v2]]
(v2 = -1 exactly: diag(1, -1, -1)).  unit(w) = w / sqrt((w0 w0 + w1 w1) + w2 w2).

Tilt: step_1 = max_tilt / 8 degrees, step_{k+1} = step_k / 8; t_k = tan(step_k); M_k[16 i + j] = rot(unit(((j - 8) t_k,
(i - 8) t_k, 1))); B_0 = rot(unit(up)); candidate frame B_{k-1} M_k[c] with element (r, c) = (B[r,0] M[0,c] + B[r,1]
M[1,c]) + B[r,2] M[2,c] in fp64; its third column rounded to fp32 is the candidate; s2_k = fp32(sin^2(max(tol, step_k)));
the highest score wins, the lowest index among equals, index 136 when the highest score is 0.  Heading: with u the fp32
third column of B_3 and s2 = fp32(sin^2 tol) the wall rows are the voting rows with a2 <= s2; p, q their fp32 dot
products (same order as d) with the fp32 first and second column of B_3; candidate (c, s): d1 = c p + s q, d2 = c q - s p,
r = min(d1 d1, d2 d2), v = max(s2 - r, 0); coarse candidates the fp32 (cos, sin) of a 128 Q, fine ones (ia, i) fp32(Ca Fc -
Sa Fs), fp32(Sa Fc + Ca Fs) (Q = pi / 65536, F of (i - 128) Q); score 0: coarse 0, fine 128.  t = 128 ia + ib - 128, (C, S) the
fp64 composition; t >= 16384: t -= 32768, (C, S) <- (S, -C).  pose = [(B_3 Rz(C, S))^T 0; 0 1]."""
import math

import numpy as np

Q = math.pi / 65536
_A = np.arange(256, dtype=np.float64)
COARSE = np.stack([np.cos(_A * 128 * Q), np.sin(_A * 128 * Q)], 1)
FINE = np.stack([np.cos((_A - 128) * Q), np.sin((_A - 128) * Q)], 1)
SCALE = np.float32(2.0 ** 30)


def unit(w):
    w = np.asarray(w, np.float64)
    return w / np.sqrt((w[..., 0:1] * w[..., 0:1] + w[..., 1:2] * w[..., 1:2]) + w[..., 2:3] * w[..., 2:3])


def rot(v):
    """v fp64 [..., 3] unit -> [..., 3, 3], the smallest rotation taking z to v"""
    v = np.asarray(v, np.float64)
    v0, v1, v2 = v[..., 0], v[..., 1], v[..., 2]
    if v.ndim == 1 and v2 == -1.0:
        return np.diag([1.0, -1.0, -1.0])
    a = 1.0 + v2
    x = -(v0 * v1) / a
    R = np.stack([np.stack([1.0 - (v0 * v0) / a, x, v0], -1), np.stack([x, 1.0 - (v1 * v1) / a, v1], -1),
                  np.stack([-v0, -v1, v2], -1)], -2)
    return R + 0.0


def steps(max_tilt):
    s1 = float(max_tilt) / 8.0
    return [s1, s1 / 8.0, s1 / 8.0 / 8.0]


def tilt_tables(max_tilt):
    """-> fp64 [3, 256, 3, 3]"""
    out = []
    j = (np.arange(256) % 16 - 8).astype(np.float64)
    i = (np.arange(256) // 16 - 8).astype(np.float64)
    for st in steps(max_tilt):
        t = math.tan(math.radians(st))
        out.append(rot(unit(np.stack([j * t, i * t, np.ones(256)], -1))))
    return np.stack(out)


def matmul(B, M):
    """element (r, c) = (B[r,0] M[0,c] + B[r,1] M[1,c]) + B[r,2] M[2,c]; M may carry leading axes"""
    B = np.asarray(B, np.float64)
    M = np.asarray(M, np.float64)
    return (B[:, 0, None] * M[..., None, 0, :] + B[:, 1, None] * M[..., None, 1, :]) + B[:, 2, None] * M[..., None, 2, :]


def s2_of(deg):
    return np.float32(math.sin(math.radians(deg)) ** 2)


def _dot(nm, u):
    """nm fp32 [N, 3], u fp32 [K, 3] or [3] -> fp32 [N, K] or [N]"""
    if u.ndim == 1:
        return (nm[:, 0] * u[0] + nm[:, 1] * u[1]) + nm[:, 2] * u[2]
    return (nm[:, 0:1] * u[None, :, 0] + nm[:, 1:2] * u[None, :, 1]) + nm[:, 2:3] * u[None, :, 2]


def _pick(score, default):
    best = int(score.max()) if len(score) else 0
    return (default, 0) if best <= 0 else (int(np.argmax(score)), best)


def manhattan_frame_ref(normals, max_tilt=30.0, tol=5.0, up=None):
    """-> dict: pose fp64 [4, 4], choice int32 [5], score int64 [5], support int32 [2], B3 fp64 [3, 3] (columns: the
    level frame's axes in the scan's frame, before the heading), A fp64 [3, 3] (with it)"""
    nm = np.ascontiguousarray(np.asarray(normals, np.float32).reshape(-1, 3))
    with np.errstate(all="ignore"):
        m = (nm[:, 0] * nm[:, 0] + nm[:, 1] * nm[:, 1]) + nm[:, 2] * nm[:, 2]
        ok = (m >= np.float32(0.5)) & (m <= np.float32(2.0))
    nm, m = nm[ok], m[ok]
    B = np.eye(3) if up is None else rot(unit(np.asarray(up, np.float64).reshape(3)))
    choice, score = [136, 136, 136, 0, 128], [0, 0, 0, 0, 0]
    zero = np.float32(0)
    if max_tilt > 0:
        tables = tilt_tables(max_tilt)
        for k, st in enumerate(steps(max_tilt)):
            s2 = s2_of(max(float(tol), st))
            u = matmul(B, tables[k])[:, :, 2].astype(np.float32)               # [256, 3]
            d = _dot(nm, u)
            a2 = d * d
            r = np.minimum(a2, np.maximum(m[:, None] - a2, zero))
            v = np.maximum(s2 - r, zero)
            sc = np.trunc(v * SCALE).astype(np.int64).sum(0) if len(nm) else np.zeros(256, np.int64)
            choice[k], score[k] = _pick(sc, 136)
            B = matmul(B, tables[k][choice[k]])
    s2 = s2_of(float(tol))
    B32 = B.astype(np.float32)
    d = _dot(nm, B32[:, 2])
    wall = d * d <= s2
    p, q = _dot(nm[wall], B32[:, 0])[:, None], _dot(nm[wall], B32[:, 1])[:, None]
    ca = sa = None
    for k in (3, 4):
        if k == 3:
            c, s = COARSE[:, 0].astype(np.float32), COARSE[:, 1].astype(np.float32)
        else:
            ca, sa = COARSE[choice[3]]
            c = (ca * FINE[:, 0] - sa * FINE[:, 1]).astype(np.float32)
            s = (sa * FINE[:, 0] + ca * FINE[:, 1]).astype(np.float32)
        d1 = c[None] * p + s[None] * q
        d2 = c[None] * q - s[None] * p
        r = np.minimum(d1 * d1, d2 * d2)
        v = np.maximum(s2 - r, zero)
        sc = np.trunc(v * SCALE).astype(np.int64).sum(0) if len(p) else np.zeros(256, np.int64)
        choice[k], score[k] = _pick(sc, 0 if k == 3 else 128)
    fc, fs = FINE[choice[4]]
    C, S = ca * fc - sa * fs, sa * fc + ca * fs
    t = 128 * choice[3] + choice[4] - 128
    if t >= 16384:
        t -= 32768
        C, S = S, -C
    A = matmul(B, np.array([[C, -S, 0.0], [S, C, 0.0], [0.0, 0.0, 1.0]]))
    pose = np.zeros((4, 4))
    pose[:3, :3] = A.T
    pose[3, 3] = 1.0
    return {"pose": pose, "choice": np.array(choice, np.int32), "score": np.array(score, np.int64),
            "support": np.array([len(nm), int(wall.sum())], np.int32), "B3": B, "A": A, "t": t}


def true_rotation(tilt, azimuth, yaw):
    """room -> scan: a turn by `yaw` about z, then a tilt by `tilt` towards the horizontal direction `azimuth`
    (degrees) -> fp64 [3, 3]"""
    az, ti, ya = math.radians(azimuth), math.radians(tilt), math.radians(yaw)
    T = rot(np.array([math.sin(ti) * math.cos(az), math.sin(ti) * math.sin(az), math.cos(ti)]))
    Z = np.array([[math.cos(ya), -math.sin(ya), 0.0], [math.sin(ya), math.cos(ya), 0.0], [0.0, 0.0, 1.0]])
    return T @ Z


def tilted_room(n, tilt, azimuth, yaw, noise=0.0, clutter=0.25, seed=0):
    """normals of a room as a scan sees it -> (fp32 [n, 3], the rotation room -> scan).  Of the rows that are not
    clutter 40 % are floor and ceiling and 60 % walls in two directions (30 % and 45 % of all at clutter 0.25); clutter is
    uniform on the sphere; signs are random; `noise` degrees of Gaussian noise per component before normalising"""
    rng = np.random.RandomState(seed)
    kind = rng.uniform(size=n)
    rest = 1.0 - clutter
    nm = np.zeros((n, 3))
    flat = kind < 0.4 * rest
    wx = (kind >= 0.4 * rest) & (kind < 0.7 * rest)
    wy = (kind >= 0.7 * rest) & (kind < rest)
    junk = kind >= rest
    nm[flat, 2], nm[wx, 0], nm[wy, 1] = 1.0, 1.0, 1.0
    g = rng.normal(size=(n, 3))
    nm[junk] = g[junk]
    nm += rng.normal(size=(n, 3)) * math.radians(noise)
    nm /= np.linalg.norm(nm, axis=1, keepdims=True)
    nm *= np.where(rng.uniform(size=(n, 1)) < 0.5, -1.0, 1.0)
    R = true_rotation(tilt, azimuth, yaw)
    return (nm @ R.T).astype(np.float32), R


def up_error_deg(res, R):
    """angle between the recovered up axis and the true one"""
    c = float(np.clip(res["B3"][:, 2] @ R[:, 2], -1.0, 1.0))
    return math.degrees(math.acos(c))


def heading_error_deg(res, R):
    """angle of the recovered x axis, seen in the room's frame, to the nearest wall direction"""
    w = R.T @ res["A"][:, 0]
    a = math.degrees(math.atan2(w[1], w[0])) % 90.0
    return min(a, 90.0 - a)


def mixed_case(chunk, seed=0):
    """3 chunk + 5 rows of a room tilted by 14 degrees and turned by 63, 1 degree of noise, with rows that must not vote
    sprinkled in (NaN, +-inf, zero, squared length 0.49 and 2.01) and rows that just may (squared length exactly 0.5
    and 2) -> fp32 [3 chunk + 5, 3]"""
    n = 3 * chunk + 5
    nm, _ = tilted_room(n, 14.0, 200.0, 63.0, noise=1.0, clutter=0.25, seed=seed)
    rng = np.random.RandomState(seed + 1)
    rows = rng.permutation(n)[:90].reshape(9, 10)
    nm[rows[0], 0] = np.nan
    nm[rows[1]] = np.nan
    nm[rows[2], 1] = np.inf
    nm[rows[3], 2] = -np.inf
    nm[rows[4]] = 0.0
    nm[rows[5]] = np.array([0.7, 0.0, 0.0], np.float32)          # 0.49
    nm[rows[6]] = np.array([1.0, -1.0, 0.1], np.float32)         # 2.01
    nm[rows[7]] = np.array([0.5, -0.5, 0.0], np.float32)         # 0.5 exactly
    nm[rows[8]] = np.array([-1.0, 0.0, 1.0], np.float32)         # 2 exactly
    return nm
