"""numpy fp64 restatement of the semantics of d3d_unproject_* (include/d3d_hip.h), and the analytic scenes
the tests of detection_3d_amd.unproject share.  unproject_ref uses element-wise operations in the stated order only: no
`@`, matmul, dot or cross, which a BLAS or a fused loop may reorder (the scenes and bounds below are free to)."""
import numpy as np


def _shift(a, du, dv, fill):
    """out[f, v, u] = a[f, v + dv, u + du], `fill` where that is outside the image"""
    out = np.full_like(a, fill)
    H, W = a.shape[1:]
    vs, vd = (slice(dv, H), slice(0, H - dv)) if dv >= 0 else (slice(0, H + dv), slice(-dv, H))
    us, ud = (slice(du, W), slice(0, W - du)) if du >= 0 else (slice(0, W + du), slice(-du, W))
    out[:, vd, ud] = a[:, vs, us]
    return out


def _difference(C, z, valid, edge, du, dv):
    """(d [3][F, H, W], has): C(+) - C(-) along one image axis, one-sided where only one neighbour is usable"""
    def usable(s):
        zq = _shift(z, s * du, s * dv, np.nan)
        return _shift(valid, s * du, s * dv, False) & (np.abs(zq - z) <= edge * z)
    hi, lo = usable(1), usable(-1)
    d = [np.where(hi, _shift(c, du, dv, 0.0), c) - np.where(lo, _shift(c, -du, -dv, 0.0), c) for c in C]
    return d, hi | lo


def unproject_ref(depth, intrinsics, extrinsics, color=None, depth_scale=0.001, columns=9, step=1, min_depth=0.0,
                  max_depth=np.inf, edge=0.05, color_div=256.0):
    """-> (rows fp32 [N, columns], pixel_of_point int32 [N], has_normal bool [N]); depth uint16 or float32 [F, H, W]"""
    depth = np.asarray(depth)
    F, H, W = depth.shape
    K = np.broadcast_to(np.asarray(intrinsics, np.float64).reshape(-1, 4), (F, 4))
    E = np.asarray(extrinsics, np.float64).reshape(F, -1, 4)[:, :3, :]
    with np.errstate(all="ignore"):
        z = depth.astype(np.float64) * np.float64(depth_scale) if depth.dtype == np.uint16 else depth.astype(np.float64)
        valid = np.isfinite(z) & (z > 0) & (z >= min_depth) & (z <= max_depth)
        u = np.arange(W, dtype=np.int64)[None, None, :]
        v = np.arange(H, dtype=np.int64)[None, :, None]
        kept = valid & (u % step == 0) & (v % step == 0)
        fx, fy, cx, cy = (K[:, j][:, None, None] for j in range(4))
        R = [[E[:, k, j][:, None, None] for j in range(3)] for k in range(3)]
        t = [E[:, k, 3][:, None, None] for k in range(3)]
        zx, zy = z / fx, z / fy
        C = [(u.astype(np.float64) - cx) * zx, (v.astype(np.float64) - cy) * zy, z]
        cols = [((R[k][0] * C[0] + R[k][1] * C[1]) + R[k][2] * C[2]) + t[k] for k in range(3)]
        if columns >= 6:
            if color is None:
                cols += [np.zeros((F, H, W))] * 3
            elif color.dtype == np.uint8:
                cols += [(color[..., k].astype(np.float64) / np.float64(color_div)).astype(np.float32) for k in range(3)]
            else:
                cols += [color[..., k] for k in range(3)]
        has = np.zeros((F, H, W), bool)
        if columns >= 9:
            a, has_a = _difference(C, z, valid, edge, 1, 0)
            b, has_b = _difference(C, z, valid, edge, 0, 1)
            m = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
            l2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
            has = kept & has_a & has_b & (l2 > 0)
            flip = (m[0] * C[0] + m[1] * C[1]) + m[2] * C[2] > 0
            m = [np.where(flip, -c, c) for c in m]
            length = np.sqrt(l2)
            n = [c / length for c in m]
            cols += [np.where(has, (R[k][0] * n[0] + R[k][1] * n[1]) + R[k][2] * n[2], 0.0) for k in range(3)]
    pix = np.flatnonzero(kept.ravel())
    rows = np.empty((pix.shape[0], columns), np.float32)
    for c in range(columns):
        col = np.broadcast_to(cols[c], (F, H, W)).ravel()[pix]
        rows[:, c] = col if col.dtype == np.float32 else col.astype(np.float32)   # fp32 colours: bit for bit
    return rows, pix.astype(np.int32), has.ravel()[pix]


def rigid(rs, n, spread=40.0):
    """n random camera-to-world matrices [n, 3, 4]: a rotation (QR of a Gaussian matrix, determinant +1) and a
    translation of tens of metres"""
    out = np.zeros((n, 3, 4))
    for i in range(n):
        q, r = np.linalg.qr(rs.randn(3, 3))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 2] = -q[:, 2]
        out[i, :, :3], out[i, :, 3] = q, rs.uniform(-spread, spread, 3)
    return out


def holes_scene(F, H, W, seed=0, float_depth=False):
    """The random-hole input: a smooth surface 1 .. 5 m away with ~30 % of the pixels zero (seeded mask), frame 1
    entirely zero when there are three frames or more (with two it would hold the batch's last pixel), the first and the
    last pixel of the batch valid; uint8 colours; random rigid extrinsics.
    float_depth: fp32 metres instead of uint16 millimetres, with NaN, +inf, negatives and values outside [0.5, 6] m
    sprinkled in (pass min_depth=0.5, max_depth=6.0)."""
    rs = np.random.RandomState(1000 + seed)
    v, u = np.mgrid[0:H, 0:W]
    z = np.stack([2.5 + np.sin(u / 9.0 + f) * 0.8 + np.cos(v / 7.0 - f) * 0.6 + 0.002 * rs.randn(H, W) for f in range(F)])
    z[:, :, W // 2:] += 0.7                                  # a depth edge through every frame
    hole = rs.rand(F, H, W) < 0.3
    if F > 2:
        hole[1] = True
    hole[0, 0, 0] = hole[-1, -1, -1] = False
    if float_depth:
        depth = z.astype(np.float32)
        depth[hole] = 0.0
        for val in (np.nan, np.inf, -1.0, 0.25, 7.5):
            sel = rs.rand(F, H, W) < 0.02
            sel[0, 0, 0] = sel[-1, -1, -1] = False
            depth[sel] = val
    else:
        depth = np.round(z * 1000.0).astype(np.uint16)
        depth[hole] = 0
    color = rs.randint(0, 256, (F, H, W, 3)).astype(np.uint8)
    f_px = 0.9 * W
    intr = np.stack([np.array([f_px + 3.0 * i, f_px - 2.0 * i, 0.5 * (W - 1) + 0.25 * i, 0.5 * (H - 1) - 0.5 * i])
                     for i in range(F)])
    return depth, color, intr, rigid(rs, F)


PLANE = dict(H=60, W=80, f=300.0, normal=np.array([0.35, -0.25, -1.0]) / np.linalg.norm([0.35, -0.25, -1.0]), d=-2.0)


def plane_scene():
    """An fp32 depth image of the tilted plane n . X = d in the camera frame, computed analytically per pixel: the ray
    of pixel (u, v) is r = ((u - cx) / f, (v - cy) / f, 1) and z = d / (n . r).  -> (depth fp32 [1, H, W], intrinsics
    [4], extrinsics [1, 3, 4] (the identity), exact camera-frame points fp64 [H, W, 3])"""
    H, W, f, n, d = (PLANE[k] for k in ("H", "W", "f", "normal", "d"))
    cx, cy = 0.5 * (W - 1), 0.5 * (H - 1)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    r = np.stack([(u - cx) / f, (v - cy) / f, np.ones_like(u)], -1)
    z = d / (r[..., 0] * n[0] + r[..., 1] * n[1] + r[..., 2] * n[2])
    assert (z > 1.0).all()
    extr = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None]
    return z.astype(np.float32)[None], np.array([f, f, cx, cy]), extr, r * z[..., None]


def plane_angle_bound(points):
    """The bound on the angle between a plane pixel's normal and the true normal (derivation: docstring of
    tests/test_unproject_gpu.py::test_plane), from the exact points [H, W, 3]: the largest over the interior pixels of
    2 eps |d| (1 / |a0| + 1 / |b0|) / sin(phi), eps = 2^-24, a0 and b0 the exact central differences and phi the angle
    between them, times 1 + 1e-3, plus 2^-24 for the fp32 rounding of the three components (each by at most 2^-25: sqrt(3) 2^-25 < 2^-24)."""
    a0 = points[1:-1, 2:] - points[1:-1, :-2]
    b0 = points[2:, 1:-1] - points[:-2, 1:-1]
    la, lb = np.linalg.norm(a0, axis=-1), np.linalg.norm(b0, axis=-1)
    sin_phi = np.linalg.norm(np.cross(a0, b0), axis=-1) / (la * lb)
    return float((2.0 * 2.0 ** -24 * abs(PLANE["d"]) * (1.0 / la + 1.0 / lb) / sin_phi).max()) * (1 + 1e-3) + 2.0 ** -24


def angle_to(normals, n):
    """angle [..] between unit-ish vectors normals [.., 3] and n [3], accurate for small angles"""
    n = np.asarray(n, np.float64)
    normals = normals.astype(np.float64)
    return np.arctan2(np.linalg.norm(np.cross(normals, n), axis=-1), normals @ n)


def walls_scene(H=24, W=32, f=40.0):
    """Two fronto-parallel walls at 2 m (left half) and 3 m (right half) meeting at column W // 2; fp32 depth, identity
    extrinsics -> (depth [1, H, W], intrinsics [4], extrinsics [1, 3, 4], the first column of the far wall)"""
    depth = np.full((1, H, W), 2.0, np.float32)
    depth[:, :, W // 2:] = 3.0
    extr = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None]
    return depth, np.array([f, f, 0.5 * (W - 1), 0.5 * (H - 1)]), extr, W // 2


ROOM = np.array([4.0, 3.0, 2.5])


def room_scene(H=48, W=64, half_fov=0.62):
    """The interior of the box [0, 4] x [0, 3] x [0, 2.5] m rendered analytically from 4 cameras inside it (z is up;
    cameras from suncg_cameras' convention: centre, forward, up) -> (depth fp32 [4, H, W], cam_pos [4, 12])"""
    cams = []
    for centre, yaw, pitch in (((1.0, 1.0, 1.2), 0.3, -0.1), ((3.0, 1.0, 1.3), 2.0, 0.15), ((3.0, 2.0, 1.2), 3.6, -0.2),
                               ((1.2, 2.1, 1.1), 5.2, 0.1)):
        t = np.array([np.cos(yaw) * np.cos(pitch), np.sin(yaw) * np.cos(pitch), np.sin(pitch)])
        right = np.cross(t, [0.0, 0.0, 1.0])
        right /= np.linalg.norm(right)
        up = np.cross(right, t)
        yf = np.arctan(np.tan(half_fov) * H / W)
        cams.append(np.concatenate([centre, t, up, [half_fov, yf, 1.0]]))
    cams = np.array(cams)
    f = 0.5 * W / np.tan(half_fov)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    r = np.stack([(u - 0.5 * (W - 1)) / f, (v - 0.5 * (H - 1)) / f, np.ones_like(u)], -1)      # camera frame
    depth = np.zeros((4, H, W), np.float32)
    for i, c in enumerate(cams):
        o, t, up = c[0:3], c[3:6], c[6:9]
        R = np.stack([np.cross(t, up), -up, t], 1)
        d = r @ R.T                                                                             # world directions
        with np.errstate(divide="ignore"):
            far = np.where(d > 0, (ROOM - o) / d, np.where(d < 0, (0.0 - o) / d, np.inf))
        depth[i] = far.min(-1)                        # the ray's z component is 1: the parameter is the depth
    return depth, cams


def room_face_distance(xyz):
    """distance of every point [N, 3] to the nearest face of the room"""
    xyz = xyz.astype(np.float64)
    return np.minimum(np.abs(xyz), np.abs(xyz - ROOM)).min(-1)
