"""numpy fp64 restatement of detection_3d_amd/csrc/normals.hip's semantics and the scene the normals tests
run on.  Neighbours come from a k-d tree at 1.001 r, d2 is recomputed in fp64 from the fp32 positions, the candidates
are ordered by (d2, j), cut at max_nn and handed to numpy.linalg.eigh."""
import numpy as np
from scipy.spatial import cKDTree

EDGE_REL = 1e-5


def canonical_sign(n):
    """the component of largest magnitude positive, ties to the lowest axis"""
    n = np.array(n, np.float64)
    k = np.argmax(np.abs(n), axis=-1)
    s = np.where(np.take_along_axis(n, k[..., None], -1)[..., 0] < 0, -1.0, 1.0)
    return n * s[..., None]


def normals_ref(xyz, radius=0.1, max_nn=50, orient=None, tie_scale="radius"):
    """xyz [N, 3] (fp32 values) -> (normals fp64 [N, 3], counts int32 [N], gap [N], edge bool [N]).
    gap = (l1 - l0) / l2 of the kept points' covariance (inf where there is no normal to find); edge: a candidate lies
    within 1e-5 r^2 of r^2, or the max_nn-th and (max_nn + 1)-th distances differ by at most that -- the points where
    fp32 and fp64 may pick different neighbour sets.
    tie_scale='cut' measures the second criterion against the (max_nn + 1)-th distance itself, 1e-5 d2 <= 1e-5 r^2: a
    tighter flag, which fewer points carry.  An fp32 d2 of an exact offset is off by at most 3 * 2^-24 d2 ~ 1.8e-7 d2,
    so the order of two distances is only in doubt within 4e-7 d2; the flag keeps a margin of 25.  A neighbourhood of
    thousands of points inside the radius needs it: its 50th and 51st d2 lie ~3e-7 m^2 apart at d2 ~ 1e-5 m^2, and the
    absolute 1e-5 r^2 = 1e-7 m^2 would flag a quarter of such points."""
    if tie_scale not in ("radius", "cut"):
        raise ValueError(tie_scale)
    p = np.asarray(xyz, np.float32)[:, :3].astype(np.float64)
    n = p.shape[0]
    r = float(np.float32(radius))
    r2 = r * r
    normals = np.tile(np.array([0.0, 0.0, 1.0]), (n, 1))
    counts = np.zeros(n, np.int32)
    gap = np.full(n, np.inf)
    edge = np.zeros(n, bool)
    if n == 0:
        return normals, counts, gap, edge
    balls = cKDTree(p).query_ball_point(p, 1.001 * r)
    for i in range(n):
        j = np.asarray(balls[i], np.int64)
        q = p[j] - p[i]
        d2 = (q * q).sum(1)
        edge[i] = bool(np.any(np.abs(d2 - r2) <= EDGE_REL * r2))
        keep = d2 <= r2
        j, q, d2 = j[keep], q[keep], d2[keep]
        order = np.lexsort((j, d2))
        if order.size > max_nn:
            tol = EDGE_REL * (r2 if tie_scale == "radius" else d2[order[max_nn]])
            if d2[order[max_nn]] - d2[order[max_nn - 1]] <= tol:
                edge[i] = True
            order = order[:max_nn]
        q = q[order]
        counts[i] = q.shape[0]
        if q.shape[0] < 3:
            continue
        c = q - q.mean(0)
        w, v = np.linalg.eigh(c.T @ c / q.shape[0])
        if not w[2] > 0:
            continue
        gap[i] = (w[1] - w[0]) / w[2]
        nv = v[:, 0] / np.linalg.norm(v[:, 0])
        if orient is None:
            nv = canonical_sign(nv)
        elif np.dot(nv, np.asarray(orient, np.float64) - p[i]) < 0:
            nv = -nv
        normals[i] = nv
    return normals, counts, gap, edge


BOX = (1.2, 0.9, 0.8)
SHIFT = (13.7, -4.2, 1.1)
VIEWPOINT = (SHIFT[0] + 0.6, SHIFT[1] + 0.45, SHIFT[2] + 0.4)      # inside the box


def make_scene(n, seed):
    """An open 1.2 x 0.9 x 0.8 m box of five faces (floor, ceiling, x = 0, x = 1.2, y = 0; n // 6 uniform points each), a
    0.4 x 0.4 m wall patch yawed 0.5 rad at (0.3, 0.3, 0.2) with the rest but 16, 3 mm of Gaussian noise on all of those,
    16 isolated points in a slab 2 m away in y; everything shifted by (13.7, -4.2, 1.1).  -> fp32 [n, 3]"""
    rs = np.random.RandomState(seed)
    lx, ly, lz = BOX
    m = n // 6
    faces = []
    for axis, at, ext in ((2, 0.0, (lx, ly)), (2, lz, (lx, ly)), (0, 0.0, (ly, lz)), (0, lx, (ly, lz)), (1, 0.0, (lx, lz))):
        uv = rs.rand(m, 2) * np.array(ext)
        f = np.empty((m, 3))
        f[:, axis] = at
        f[:, [a for a in range(3) if a != axis]] = uv
        faces.append(f)
    k = n - 5 * m - 16
    uv = rs.rand(k, 2) * 0.4
    c, s = np.cos(0.5), np.sin(0.5)
    patch = np.stack([0.3 + uv[:, 0] * c, 0.3 + uv[:, 0] * s, 0.2 + uv[:, 1]], 1)
    pts = np.concatenate(faces + [patch])
    pts = pts + rs.randn(*pts.shape) * 0.003
    lone = np.stack([rs.rand(16) * lx, 2.0 + ly + rs.rand(16) * 0.5, rs.rand(16) * lz], 1)
    pts = np.concatenate([pts, lone]) + np.array(SHIFT)
    return pts.astype(np.float32)


def dense_patch(n, seed):
    """n points within a 5 cm cube on a tilted plane with 1 mm of noise, beside the scene's box -> fp32 [n, 3]"""
    rs = np.random.RandomState(seed)
    uv = rs.rand(n, 2) * 0.05
    pts = np.stack([uv[:, 0], uv[:, 1], 0.3 * uv[:, 0] + 0.2 * uv[:, 1]], 1) + rs.randn(n, 3) * 0.001
    return (pts + np.array(SHIFT) + np.array([0.5, 0.4, 0.35])).astype(np.float32)
