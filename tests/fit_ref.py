"""numpy restatement of d3d_fit_boxes (include/d3d_hip.h) and the scenes its tests use.  Imports nothing from the package.

Definition.  Q = pi / 65536.  Coarse table C[a] = (cos(a 128 Q), sin(a 128 Q)), fine table F[i] = (cos((i - 128) Q),
sin((i - 128) Q)), a, i = 0..255, fp64.  A row belongs to nothing when its id is negative or >= k or a coordinate (after
p = float32(double(x) - origin), when an origin is given) is not finite.  The coarse direction a is c = float32(C[a].cos),
s = float32(C[a].sin); the fine direction (a, i) is c = float32(Ca Fc - Sa Fs), s = float32(Sa Fc + Ca Fs), every product and
sum an fp64 operation of its own.  Per instance and direction u = c x - s y, v = s x + c y in fp32 (each product and sum
rounded), + 0 so that a zero is +0; umin, umax, vmin, vmax over the rows; area = (double(umax) - double(umin)) *
(double(vmax) - double(vmin)).  Pass 1: the coarse a of the smallest area, the lowest a among equals; pass 2: the fine i
around it likewise.  An instance that is not yaw_free takes a = 0, i = 128.  The box in fp64, rounded once: t = 128 a +
i - 128, theta = t Q; eu = umax - umin, ev = vmax - vmin, mu, mv the middles; xc = c mu + s mv, yc = -s mu + c mv;
free and eu > ev: d3 = ev, d4 = eu, yaw = theta + pi / 2, otherwise d3 = eu, d4 = ev, yaw = theta; yaw >= pi / 2 loses pi;
z_bot = zmin, dz = double(zmax) - double(zmin).  No points: a zero row, count 0, choice (-1, -1), extents +inf / -inf."""
import math

import numpy as np

Q = math.pi / 65536
_A = np.arange(256, dtype=np.float64)
COARSE = np.stack([np.cos(_A * 128 * Q), np.sin(_A * 128 * Q)], 1)
FINE = np.stack([np.cos((_A - 128) * Q), np.sin((_A - 128) * Q)], 1)
FINE_STEP = Q                     # 4.79e-5 rad


def _extents(x, y, c, s):
    """x, y fp32 [n]; c, s fp32 [256] -> umin, umax, vmin, vmax fp32 [256]"""
    c, s = c[:, None], s[:, None]
    u = (c * x[None] - s * y[None]) + np.float32(0)
    v = (s * x[None] + c * y[None]) + np.float32(0)
    return u.min(1), u.max(1), v.min(1), v.max(1)


def _area(e):
    return (e[1].astype(np.float64) - e[0].astype(np.float64)) * (e[3].astype(np.float64) - e[2].astype(np.float64))


def fine_directions(a):
    ca, sa = COARSE[a]
    c = ca * FINE[:, 0] - sa * FINE[:, 1]
    s = sa * FINE[:, 0] + ca * FINE[:, 1]
    return c.astype(np.float32), s.astype(np.float32)


def fit_one(p, free=True):
    """p fp32 [n >= 1, 3] -> (box fp32 [7], choice (a, i), extent fp32 [6])"""
    x, y, z = np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(p[:, 1]), p[:, 2]
    a = 0
    if free:
        a = int(np.argmin(_area(_extents(x, y, COARSE[:, 0].astype(np.float32), COARSE[:, 1].astype(np.float32)))))
    c, s = fine_directions(a)
    e = _extents(x, y, c, s)
    i = int(np.argmin(_area(e))) if free else 128
    umin, umax, vmin, vmax = (np.float64(v[i]) for v in e)
    zmin, zmax = z.min() + np.float32(0), z.max() + np.float32(0)
    theta = np.float64(a * 128 + (i - 128)) * Q
    eu, ev = umax - umin, vmax - vmin
    mu, mv = (umin + umax) * 0.5, (vmin + vmax) * 0.5
    cd, sd = np.float64(c[i]), np.float64(s[i])
    xc, yc = cd * mu + sd * mv, (-sd) * mu + cd * mv
    d3, d4, yaw = eu, ev, theta
    if free and eu > ev:
        d3, d4, yaw = ev, eu, theta + math.pi / 2
    if yaw >= math.pi / 2:
        yaw -= math.pi
    box = np.array([xc, yc, zmin, d3, d4, np.float64(zmax) - np.float64(zmin), yaw], np.float64).astype(np.float32)
    return box, (a, i), np.array([e[0][i], e[1][i], e[2][i], e[3][i], zmin, zmax], np.float32)


def fit_boxes_ref(xyz, instance, k, yaw_free=None, origin=None):
    """-> boxes fp32 [k, 7], count int32 [k], choice int32 [k, 2], extent fp32 [k, 6]"""
    p = np.asarray(xyz, np.float32)[:, :3]
    if origin is not None:
        p = (p.astype(np.float64) - np.asarray(origin, np.float64)[None]).astype(np.float32)
    inst = np.asarray(instance).astype(np.int64)
    ok = (inst >= 0) & (inst < k) & np.isfinite(p).all(1)
    boxes = np.zeros((k, 7), np.float32)
    count = np.zeros(k, np.int32)
    choice = np.full((k, 2), -1, np.int32)
    extent = np.tile(np.array([np.inf, -np.inf], np.float32), (k, 3))
    for g in range(k):
        rows = ok & (inst == g)
        count[g] = rows.sum()
        if count[g]:
            boxes[g], choice[g], extent[g] = fit_one(p[rows], True if yaw_free is None else bool(yaw_free[g]))
    return boxes, count, choice, extent


def yaw_distance(a, b):
    """|a - b| modulo pi"""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % math.pi
    return np.minimum(d, math.pi - d)


def box_points(rng, box, n_inner):
    """the eight corners of a yx_zb box and n_inner points inside it -> fp64 [8 + n_inner, 3]"""
    xc, yc, zb, d3, d4, dz, yaw = (float(v) for v in box)
    g = np.stack(np.meshgrid([-d3 / 2, d3 / 2], [-d4 / 2, d4 / 2], [0, dz], indexing="ij"), -1).reshape(-1, 3)
    u = rng.uniform(-0.5, 0.5, (n_inner, 3)) * np.array([d3, d4, dz])
    u[:, 2] += dz / 2
    g = np.concatenate([g, u])
    c, s = math.cos(yaw), math.sin(yaw)
    return np.stack([c * g[:, 0] + s * g[:, 1] + xc, -s * g[:, 0] + c * g[:, 1] + yc, g[:, 2] + zb], 1)


def random_rectangle(rng, span=60.0):
    """a wall-like box: thickness 0.05-0.4 m, length 0.5-12 m, centre up to `span` m"""
    return np.array([rng.uniform(0, span), rng.uniform(0, span), rng.uniform(0, 3), rng.uniform(0.05, 0.4),
                     rng.uniform(0.5, 12), rng.uniform(0.5, 3), rng.uniform(-math.pi / 2, math.pi / 2 * 0.999)])


def mixed_case(chunk, seed=0):
    """One call that mixes what the sweep can get wrong.  -> (xyz fp32 [N, 3], instance int64 [N], k, yaw_free bool [k]),
    N about 20 000, coordinates up to 80 m: instances of 1, 2, chunk - 1, chunk, chunk + 1 and 3 chunk + 5 points; 300
    instances of 1-7 points; five walls of 2000-3000 points; points on a line along x and along the diagonal, and identical
    points (equal areas: the lowest index); ids without points in the middle and at the end; rows with id -1, ids >= k,
    NaN and inf coordinates; free and fixed yaw mixed; rows shuffled."""
    rng = np.random.RandomState(seed)
    sizes = [1, 2, chunk - 1, chunk, chunk + 1, 3 * chunk + 5] + [int(v) for v in rng.randint(1, 8, 300)] + \
            [int(v) for v in rng.randint(2000, 3001, 5)]
    pts, ids, g = [], [], 0
    for n in sizes:
        while g in (3, 40, 41, 200):                    # ids without points in the middle
            g += 1
        b = random_rectangle(rng, 80.0)
        p = box_points(rng, b, max(n - 8, 0))
        pts.append(p[rng.permutation(len(p))[:n]] if n < 8 else p)
        ids.append(np.full(n, g))
        g += 1
    t = np.linspace(0, 7.5, 60)
    line_x = np.stack([20 + t, np.full_like(t, 33.25), 0.1 * t], 1)
    line_d = np.stack([5 + t, 5 + t, 0.2 * t], 1)
    same = np.tile(np.array([[71.5, 12.25, 1.5]]), (20, 1))
    for p in (line_x, line_d, same):
        pts.append(p)
        ids.append(np.full(len(p), g))
        g += 1
    k = g + 3                                            # ... and at the end
    xyz = np.concatenate(pts).astype(np.float32)
    inst = np.concatenate(ids).astype(np.int64)
    junk = rng.uniform(0, 80, (900, 3)).astype(np.float32)
    junk_id = np.concatenate([np.full(300, -1), np.full(100, -7), np.full(150, k), np.full(50, k + 1000),
                              rng.randint(0, g, 300)]).astype(np.int64)
    junk[600:700, 0] = np.nan
    junk[700:800, 1] = np.inf
    junk[800:850, 2] = -np.inf
    junk[850:900, 2] = np.nan
    xyz, inst = np.concatenate([xyz, junk]), np.concatenate([inst, junk_id])
    perm = rng.permutation(len(xyz))
    free = rng.uniform(size=k) < 0.7
    free[:6] = [True, False, True, True, False, True]
    free[g - 3:g] = True
    return xyz[perm], inst[perm], k, free
