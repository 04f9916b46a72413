"""fp64 numpy restatement of d3d_points_in_boxes (include/d3d_hip.h) and the scenes its tests use.

Definition: point = float32(double(x) - origin) when an origin is given; per box c = float32(cos(double(yaw))),
s = float32(sin(double(yaw))); lx = c (X - xc) - s (Y - yc), ly = s (X - xc) + c (Y - yc), lz = Z - z_bot; member iff
|lx| <= max(d3, grow_yx) / 2, |ly| <= max(d4, grow_yx) / 2, 0 <= lz <= max(dz, grow_z), all closed.  Here everything after
the fp32 inputs is fp64; the kernel works in fp32, so a (point, box) pair whose signed distance to the nearest deciding
face is below TOL is *doubtful* and the tests leave its membership open.  TOL = 1e-4 m is more than ten fp32 ulps at
lattice-scale coordinates (ulp(25) = 1.9e-6; lx is two products and a difference of such numbers)."""
import numpy as np

TOL = 1e-4
DOUBTFUL_CAP = 0.0025      # at most this share of a scene's points may be doubtful


def margins(xyz, boxes, grow=(0.0, 0.0), origin=None):
    """-> (margin [N, K], local [N, K, 3]) in fp64: margin >= 0 iff member, its magnitude the distance to the face that
    decides; NaN points get margin -inf."""
    p = np.asarray(xyz, np.float32)[:, :3]
    if origin is not None:
        p = (p.astype(np.float64) - np.asarray(origin, np.float64)[None]).astype(np.float32)
    p = p.astype(np.float64)
    b = np.asarray(boxes, np.float32).reshape(-1, 7)
    c = np.cos(b[:, 6].astype(np.float64)).astype(np.float32).astype(np.float64)
    s = np.sin(b[:, 6].astype(np.float64)).astype(np.float32).astype(np.float64)
    hx = (np.maximum(b[:, 3], np.float32(grow[0])) * np.float32(0.5)).astype(np.float64)
    hy = (np.maximum(b[:, 4], np.float32(grow[0])) * np.float32(0.5)).astype(np.float64)
    hz = np.maximum(b[:, 5], np.float32(grow[1])).astype(np.float64)
    bd = b.astype(np.float64)
    dx = p[:, None, 0] - bd[None, :, 0]
    dy = p[:, None, 1] - bd[None, :, 1]
    local = np.stack([c[None] * dx - s[None] * dy, s[None] * dx + c[None] * dy, p[:, None, 2] - bd[None, :, 2]], -1)
    local = local + 0.0                                   # -0 -> +0, as the kernel reports its extents
    with np.errstate(invalid="ignore"):
        m = np.minimum(np.minimum(hx[None] - np.abs(local[..., 0]), hy[None] - np.abs(local[..., 1])),
                       np.minimum(local[..., 2], hz[None] - local[..., 2]))
    m = np.where(np.isnan(m), -np.inf, m)
    return m, local


def _extents(local, mask):
    k = mask.shape[1]
    lo = np.full((k, 3), np.inf)
    hi = np.full((k, 3), -np.inf)
    for d in range(3):
        v = local[..., d]
        lo[:, d] = np.where(mask, v, np.inf).min(0, initial=np.inf)
        hi[:, d] = np.where(mask, v, -np.inf).max(0, initial=-np.inf)
    return lo, hi


def points_in_boxes_ref(xyz, boxes, grow=(0.0, 0.0), origin=None, tol=TOL):
    """-> dict: owner int32 [N], count [K], lo / hi fp64 [K, 3] of the exact definition; doubtful bool [N] (some box's
    deciding face is nearer than tol); count_certain / count_possible [K] and lo_in, hi_in (certain members only) /
    lo_out, hi_out (every possible member): the brackets a correct fp32 evaluation stays in."""
    m, local = margins(xyz, boxes, grow, origin)
    n, k = m.shape
    inside = m >= 0
    owner = np.where(inside.any(1), inside.argmax(1), -1).astype(np.int32) if k else np.full(n, -1, np.int32)
    certain, possible = m >= tol, m > -tol
    lo, hi = _extents(local, inside)
    lo_in, hi_in = _extents(local, certain)
    lo_out, hi_out = _extents(local, possible)
    return {"owner": owner, "count": inside.sum(0).astype(np.int32), "lo": lo, "hi": hi,
            "doubtful": (np.abs(m) < tol).any(1) if k else np.zeros(n, bool),
            "count_certain": certain.sum(0), "count_possible": possible.sum(0),
            "lo_in": lo_in, "hi_in": hi_in, "lo_out": lo_out, "hi_out": hi_out}


def scene(seed, N=20000, K=48):
    """-> (xyz fp32 [N, 3], boxes fp32 [K, 7]): wall-like boxes in a 25 x 19 x 2.7 m building, yaws near 0, +-pi/2 and
    +-pi/4; half of the points uniform in the building, half drawn in box frames at U[-0.6, 0.6] x size around random
    boxes, so that some fall just outside."""
    rng = np.random.RandomState(seed)
    b = np.zeros((K, 7))
    b[:, 0] = rng.uniform(0, 25, K)
    b[:, 1] = rng.uniform(0, 19, K)
    b[:, 2] = rng.uniform(0, 0.3, K)
    b[:, 3] = rng.uniform(0.08, 0.3, K)
    b[:, 4] = rng.uniform(0.5, 6, K)
    b[:, 5] = rng.uniform(1, 2.8, K)
    base = np.array([0.0, np.pi / 2 - 1e-3, -np.pi / 2, np.pi / 4, -np.pi / 4])
    b[:, 6] = base[rng.randint(0, len(base), K)] + rng.randn(K) * 0.02
    n_uni = N - N // 2 if K else N
    pts = rng.uniform(0, 1, (n_uni, 3)) * np.array([25.0, 19.0, 2.7])
    if N - n_uni:
        j = rng.randint(0, K, N - n_uni)
        u = rng.uniform(-0.6, 0.6, (N - n_uni, 3)) * b[j, 3:6]
        c, s = np.cos(b[j, 6]), np.sin(b[j, 6])
        near = np.stack([c * u[:, 0] + s * u[:, 1] + b[j, 0], -s * u[:, 0] + c * u[:, 1] + b[j, 1],
                         b[j, 2] + 0.5 * b[j, 5] + u[:, 2]], 1)
        pts = np.concatenate([pts, near])[rng.permutation(N)]
    return pts.astype(np.float32), b.astype(np.float32)


def lattice_case(grow):
    """The exact case: yaw = 0 boxes and points whose coordinates are multiples of 1/64 -- on faces, edges and corners of
    the (grown) boxes, one step inside and one step outside -- so that fp32 and fp64 agree bit for bit.  grow must be
    multiples of 1/32.  -> (xyz fp32, boxes fp32)."""
    step = 1.0 / 64
    boxes = np.array([[2.0, 3.0, 0.5, 0.25, 2.0, 1.5, 0.0],
                      [2.0, 3.5, 0.0, 0.5, 1.0, 2.5, 0.0],        # overlaps the first: shared points, lowest index owns
                      [6.0, 1.0, 0.25, 0.125, 0.75, 0.25, 0.0],
                      [40.0, 40.0, 0.0, 1.0, 1.0, 1.0, 0.0]], np.float32)      # nothing near it: stays empty
    pts = []
    for b in boxes[:3].astype(np.float64):
        hx, hy, hz = max(b[3], grow[0]) / 2, max(b[4], grow[0]) / 2, max(b[5], grow[1])
        xs = b[0] + np.array([-hx - step, -hx, -hx + step, 0.0, hx - step, hx, hx + step])
        ys = b[1] + np.array([-hy - step, -hy, -hy + step, 0.0, hy - step, hy, hy + step])
        zs = b[2] + np.array([-step, 0.0, step, hz / 2, hz - step, hz, hz + step])
        g = np.stack(np.meshgrid(xs, ys, zs, indexing="ij"), -1).reshape(-1, 3)
        pts.append(g)
    pts = np.concatenate(pts)
    assert np.array_equal(pts * 64, np.round(pts * 64))
    return pts.astype(np.float32), boxes


def sampled_wall(box, step=0.02):
    """points on both faces of a yx_zb wall box, every `step` metres along its length and every 0.1 m of its height,
    ends included -> fp64 [M, 3]"""
    xc, yc, zb, d3, d4, dz, yaw = (float(v) for v in box)
    ly = np.linspace(-d4 / 2, d4 / 2, int(round(d4 / step)) + 1)
    lz = np.arange(0.05, dz, 0.1)
    lx = np.array([-d3 / 2, d3 / 2])
    g = np.stack(np.meshgrid(lx, ly, lz, indexing="ij"), -1).reshape(-1, 3)
    c, s = np.cos(yaw), np.sin(yaw)
    return np.stack([c * g[:, 0] + s * g[:, 1] + xc, -s * g[:, 0] + c * g[:, 1] + yc, g[:, 2] + zb], 1)


def room_scene(seed):
    """A rectangular room of four sampled walls and a fifth across its middle, in the file's frame -> (pcl fp32 [N, 9]
    with zero colour and normal, boxes fp32 [5, 7] yx_zb, labels int64 [5]).  Walls along x have yaw pi/2, walls along y
    yaw 0; the room is 6 + seed by 5 m, so every 4 x 4 m window holds a stretch of the middle wall."""
    rng = np.random.RandomState(seed)
    x0, y0 = rng.uniform(-3, 3, 2)
    w, h = 6.0 + seed, 5.0
    boxes = np.array([[x0 + w / 2, y0, 0.0, 0.2, w, 2.6, np.pi / 2],
                      [x0 + w / 2, y0 + h, 0.0, 0.2, w, 2.6, np.pi / 2],
                      [x0, y0 + h / 2, 0.0, 0.2, h, 2.6, 0.0],
                      [x0 + w, y0 + h / 2, 0.0, 0.2, h, 2.6, 0.0],
                      [x0 + w / 2, y0 + h / 2, 0.0, 0.2, h, 2.6, 0.0]], np.float32)
    xyz = np.concatenate([sampled_wall(b) for b in boxes])
    pcl = np.zeros((xyz.shape[0], 9), np.float32)
    pcl[:, :3] = xyz[rng.permutation(xyz.shape[0])]
    return pcl, boxes, np.ones(5, np.int64)
