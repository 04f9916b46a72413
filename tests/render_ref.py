"""numpy fp64 restatement of the semantics of d3d_render_* (include/d3d_hip.h): brute force over pixels x
triangles with the same operations in the same order, element-wise only (no `@`, dot or cross, which a BLAS or a fused
loop may reorder), and the scenes the tests of detection_3d_amd.render share."""
import numpy as np

from detection_3d_amd.render import box_mesh, look_at


def camera_space(vertices, extr):
    """p = R^T (x - t) for every vertex: [V, 3] fp64"""
    E = np.asarray(extr, np.float64)
    x = np.asarray(vertices, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        d = [x[:, k] - E[k, 3] for k in range(3)]
        return np.stack([(E[0, k] * d[0] + E[1, k] * d[1]) + E[2, k] * d[2] for k in range(3)], 1)


def _cross(p, q):
    return (p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0])


def edge_normals(a, b, c):
    """(n_bc, n_ca, n_ab, D) of one triangle from its camera-space vertices (sequences of three fp64 scalars)"""
    n0, n1, n2 = _cross(b, c), _cross(c, a), _cross(a, b)
    return n0, n1, n2, (a[0] * n0[0] + a[1] * n0[1]) + a[2] * n0[2]


def render_ref(vertices, triangles, intrinsics, extrinsics, height, width, vertex_color=None, min_depth=0.0,
               max_depth=np.inf, depth_dtype=np.float32, depth_scale=0.001):
    """-> (depth [F, H, W] of depth_dtype, tri int32 [F, H, W], color [F, H, W, 3] or None, z fp64 [F, H, W] (inf where
    nothing was hit))"""
    vertices = np.asarray(vertices, np.float32)
    triangles = np.asarray(triangles, np.int32)
    V, T = vertices.shape[0], triangles.shape[0]
    E = np.asarray(extrinsics, np.float64)
    E = E.reshape(E.shape[0], -1, 4)[:, :3, :]
    F, H, W = E.shape[0], int(height), int(width)
    K = np.broadcast_to(np.asarray(intrinsics, np.float64).reshape(-1, 4), (F, 4))
    in_range = ((triangles >= 0) & (triangles < V)).all(1)
    finite = np.isfinite(vertices).all(1)
    zbest = np.full((F, H, W), np.inf)
    tri = np.full((F, H, W), -1, np.int32)
    eb = np.zeros((3, F, H, W))
    u = np.arange(W, dtype=np.float64)[None, :]
    v = np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        for f in range(F):
            fx, fy, cx, cy = K[f]
            dx, dy = (u - cx) / fx, (v - cy) / fy
            P = camera_space(vertices, E[f])
            for t in range(T):
                if not in_range[t] or not finite[triangles[t]].all():
                    continue
                a, b, c = (tuple(P[i]) for i in triangles[t])
                n0, n1, n2, D = edge_normals(a, b, c)
                e0 = (dx * n0[0] + dy * n0[1]) + n0[2]
                e1 = (dx * n1[0] + dy * n1[1]) + n1[2]
                e2 = (dx * n2[0] + dy * n2[1]) + n2[2]
                S = (e0 + e1) + e2
                inside = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
                z = D / S
                hit = inside & (S != 0) & np.isfinite(z) & (z > 0) & (z >= min_depth) & (z <= max_depth)
                better = hit & (z < zbest[f])                      # ascending t: an equal z keeps the lower index
                zbest[f][better] = z[better]
                tri[f][better] = t
                for k, e in enumerate((e0, e1, e2)):
                    eb[k, f][better] = e[better]
        hit = tri >= 0
        if depth_dtype == np.uint16:
            q = np.rint(np.where(hit, zbest, 0.0) / np.float64(depth_scale))
            depth = np.where((q >= 1) & (q <= 65535), q, 0.0).astype(np.uint16)
        else:
            depth = np.where(hit, zbest, 0.0).astype(np.float32)
        color = None
        if vertex_color is not None:
            vc = np.asarray(vertex_color)
            S = (eb[0] + eb[1]) + eb[2]
            w = [eb[k] / S for k in range(3)]
            corner = triangles[np.maximum(tri, 0)]                                    # [F, H, W, 3]
            col = [(w[0] * vc[corner[..., 0], k].astype(np.float64) + w[1] * vc[corner[..., 1], k].astype(np.float64))
                   + w[2] * vc[corner[..., 2], k].astype(np.float64) for k in range(3)]
            col = np.where(hit[..., None], np.stack(col, -1), 0.0)
            if vc.dtype == np.uint8:
                color = np.clip(np.nan_to_num(np.rint(col), nan=0.0), 0.0, 255.0).astype(np.uint8)
            else:
                color = col.astype(np.float32)
    return depth, tri, color, zbest


def moller_trumbore(orig, d, a, b, c):
    """An independent ray-triangle intersection in fp64 (Moller and Trumbore 1997) -> (t, u, v) of orig + t d, the
    barycentric coordinates of b and c; np.nan where the ray is parallel to the plane"""
    e1, e2 = b - a, c - a
    p = np.cross(d, e2)
    det = e1 @ p
    if det == 0.0:
        return np.nan, np.nan, np.nan
    s = orig - a
    uu = (s @ p) / det
    q = np.cross(s, e1)
    return (e2 @ q) / det, uu, (d @ q) / det


def intrinsics_of(F, H, W):
    """camera 0 has its principal point on the pixel grid's centre exactly; the others differ a little"""
    f_px = 0.9 * W
    return np.stack([np.array([f_px + 3.0 * i, f_px - 2.0 * i, 0.5 * (W - 1) + 0.25 * i, 0.5 * (H - 1) - 0.5 * i])
                     for i in range(F)])


ROOM = np.array([4.0, 3.0, 2.5])
EYE0 = np.array([1.0, 1.0, 1.25])            # camera 0: level, looking along +x: its axes are exact in fp64


def room_boxes():
    """the room as one box (seen from inside: the test is two-sided) and two interior boxes, yx_zb"""
    return np.array([[2.0, 1.5, 0.0, 4.0, 3.0, 2.5, 0.0],
                     [2.6, 1.2, 0.0, 0.5, 0.9, 1.1, 0.4],
                     [3.1, 2.2, 0.3, 0.4, 0.6, 1.5, -0.7]])


def room_cameras(F):
    """level inside the room; rolled and tilted inside it; outside, looking away (F == 2: the first two)"""
    cams = [look_at(EYE0, EYE0 + np.array([1.0, 0.0, 0.0])),
            look_at([3.4, 2.6, 0.9], [0.6, 0.7, 1.5], up=(0.25, -0.1, 1.0)),
            look_at([10.0, 10.0, 1.0], [20.0, 18.0, 1.5])]
    return np.stack(cams[:F])


SPECIAL = ("crossing", "behind", "zero_area", "edge_on", "coincident_lo", "coincident_hi", "covering", "nan_vertex",
           "bad_index", "negative_index")


def exact_scene(F, H, W, uint8_color=False, coincident=True, seed=0):
    """The scene of the exactness tests -> dict(vertices, triangles, color, intr, extr, ids: name -> triangle index,
    strip: the indices of the sub-pixel strip).  About 60 triangles; `coincident=False` leaves the coincident pair's
    second triangle out (the order-independence test)."""
    verts, tris = box_mesh(room_boxes())
    verts, tris = [verts], [tris]
    ids, n_v, n_t = {}, verts[0].shape[0], tris[0].shape[0]

    def add(name, pts, idx=None):
        nonlocal n_v, n_t
        pts = np.asarray(pts, np.float32).reshape(-1, 3)
        idx = np.arange(3).reshape(1, 3) if idx is None else np.asarray(idx).reshape(-1, 3)
        verts.append(pts)
        tris.append((idx + n_v).astype(np.int32))
        if name:
            ids[name] = n_t
        first = n_t
        n_v, n_t = n_v + pts.shape[0], n_t + idx.shape[0]
        return np.arange(first, n_t)

    add("crossing", [[0.5, 1.0, 1.0], [2.0, 0.8, 1.0], [2.0, 1.2, 1.1]])          # camera 0 is at x = 1
    add("behind", [[0.2, 0.5, 1.0], [0.6, 1.5, 1.0], [0.3, 1.0, 2.0]])
    add("zero_area", [[2.0, 0.5, 0.5], [2.25, 0.75, 0.875], [2.5, 1.0, 1.25]])
    add("edge_on", [[2.0, 0.5, 1.25], [3.0, 1.0, 1.25], [2.5, 2.0, 1.25]])        # in the horizontal plane of camera 0
    pair = [[3.5, 0.2, 1.6], [3.5, 0.9, 1.7], [3.6, 0.5, 2.3]]
    add("coincident_lo", pair)
    if coincident:
        add("coincident_hi", pair)             # the same vertices in the same order: the same z to the last bit
    add("covering", [[3.9, -40.0, -30.0], [3.9, 40.0, -30.0], [3.9, 0.0, 50.0]])   # fills the image of camera 0
    # a strip of triangles 0.8 pixels wide and high on the plane x = 3.7, 2.7 m from camera 0
    px = 2.7 / (0.9 * W)
    g = np.arange(24)
    base = np.stack([np.full(24, 3.7), 1.3 + 1.37 * px * g, 2.0 + 0.29 * px * g], 1)
    strip_pts = np.concatenate([base, base + [0.0, 0.8 * px, 0.0], base + [0.0, 0.3 * px, 0.8 * px]])
    strip = add(None, strip_pts, np.stack([g, g + 24, g + 48], 1) - 0)
    add("nan_vertex", [[2.0, 1.0, 1.0], [np.nan, 1.5, 1.0], [2.0, 1.2, 1.6]])
    vertices = np.concatenate(verts)
    triangles = np.concatenate(tris)
    V = vertices.shape[0]
    ids["bad_index"], ids["negative_index"] = n_t, n_t + 1
    triangles = np.concatenate([triangles, np.array([[0, 1, V], [-1, 2, 3]], np.int32)])
    rs = np.random.RandomState(77 + seed)
    color = rs.randint(0, 256, (V, 3)).astype(np.uint8) if uint8_color else rs.rand(V, 3).astype(np.float32)
    return dict(vertices=vertices, triangles=triangles, color=color, intr=intrinsics_of(F, H, W), extr=room_cameras(F),
                ids=ids, strip=strip)


def check_exact_scene(scene, tri, H, W):
    """every special triangle does in the restatement what it is there for (tri: the restatement's [F, H, W])"""
    ids, t0 = scene["ids"], tri[0]
    P = camera_space(scene["vertices"], scene["extr"][0])

    def zs(name):
        return P[scene["triangles"][ids[name]], 2]
    assert (t0 >= 0).mean() >= 0.5 and (tri[0] < 12).any(), "camera 0 sees the room"
    assert (zs("crossing") > 0).any() and (zs("crossing") < 0).any() and (t0 == ids["crossing"]).any()
    assert (zs("behind") < 0).all() and not (tri == ids["behind"]).any()
    assert not (t0 == ids["zero_area"]).any()
    a, b, c = (tuple(p) for p in P[scene["triangles"][ids["edge_on"]]])
    assert edge_normals(a, b, c)[3] == 0.0 and not (t0 == ids["edge_on"]).any()
    assert (t0 == ids["coincident_lo"]).sum() >= 4
    if "coincident_hi" in ids:
        assert not (tri == ids["coincident_hi"]).any()
    assert (t0 == ids["covering"]).any()
    for corner in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):       # the covering triangle contains the whole image
        assert t0[corner] >= 0
    won = np.array([(t0 == s).any() for s in scene["strip"]])
    assert won.any() and not won.all(), "some sub-pixel triangles hit a pixel centre, some none"
    for name in ("nan_vertex", "bad_index", "negative_index"):
        assert not (tri == ids[name]).any()
    if tri.shape[0] > 2:
        assert (tri[2] == -1).all(), "the camera outside sees nothing"
    assert (tri[1] >= 0).mean() >= 0.5


def plane_grid(n=16, seed=3, jitter=0.3):
    """The plane z_w = 0 over [0, n] x [0, n] m as n x n quads with jittered interior vertices (fp32) and mixed winding
    and diagonal -> (vertices [(n + 1)^2, 3], triangles [2 n^2, 3])"""
    rs = np.random.RandomState(seed)
    gy, gx = np.mgrid[0:n + 1, 0:n + 1].astype(np.float64)
    inner = ((gx > 0) & (gx < n) & (gy > 0) & (gy < n)).astype(np.float64)
    x = gx + inner * rs.uniform(-jitter, jitter, gx.shape)
    y = gy + inner * rs.uniform(-jitter, jitter, gy.shape)
    vertices = np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], 1).astype(np.float32)
    tris = []
    for j in range(n):
        for i in range(n):
            v00, v10, v01, v11 = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i, (j + 1) * (n + 1) + i + 1
            pair = [(v00, v10, v11), (v00, v11, v01)] if rs.rand() < 0.5 else [(v00, v10, v01), (v10, v11, v01)]
            for t in pair:
                tris.append(t if rs.rand() < 0.5 else (t[0], t[2], t[1]))
    return vertices, np.asarray(tris, np.int32)


def plane_expectation(intr, extr, H, W, n):
    """For the plane z_w = 0 over [0, n]^2 and one camera: (inside bool [H, W]: the rays of the pixel and of its eight
    neighbours (u +- 1, v +- 1) all meet the plane in front of the camera within the extent, i.e. the pixel is at
    least one pixel inside the outline; z fp64 [H, W]: the analytic ray-plane z-depth)"""
    fx, fy, cx, cy = np.asarray(intr, np.float64)
    E = np.asarray(extr, np.float64)
    v, u = np.mgrid[-1:H + 1, -1:W + 1].astype(np.float64)
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1) @ E[:, :3].T           # world directions
    with np.errstate(all="ignore"):
        z = -E[2, 3] / d[..., 2]
        x, y = E[0, 3] + z * d[..., 0], E[1, 3] + z * d[..., 1]
        ok = (z > 0) & (x >= 0) & (x <= n) & (y >= 0) & (y <= n)
    inside = np.ones((H, W), bool)
    for dv in range(3):
        for du in range(3):
            inside &= ok[dv:dv + H, du:du + W]
    return inside, z[1:-1, 1:-1]


CUPBOARD = np.array([20.0, 9.85, 0.0, 2.0, 0.5, 1.5, 0.0])          # 5 cm in front of the wall face y = 9.55
HIDDEN = np.array([20.0, 9.55, 0.5, 0.4, 0.04, 0.5, 0.0])           # a slab around that face, behind the cupboard's middle
BESIDE = np.array([22.5, 9.55, 0.5, 0.4, 0.04, 0.5, 0.0])           # the same slab beside the cupboard: in plain sight


def building(seed=0):
    """synthetic.make_targets' walls as boxes (in the box convention of primitives they form a cross of two bundles of
    overlapping slabs through (12.5, 9.5)), a floor and a ceiling slab over their bounding box and a cupboard in front
    of the wall face y = 9.55 -> (vertices, triangles, lo [3], hi [3] of the mesh, intrinsics [4], extrinsics [6, 3, 4]
    of six cameras at 64 x 64, 1.3 m above the floor and at least 2.4 m from every wall).  HIDDEN is out of sight: a ray
    from a camera at (cx, cy, 1.3) to a point of it passes the cupboard's back plane y = 9.6 within
    0.2 + 0.05 |cx - 20| / (cy - 9.55) m of x = 20, inside the cupboard's [19, 21] for every camera here, and below
    its top (1.3 m < 1.5 m)."""
    from detection_3d_amd.synthetic import make_targets
    boxes, labels = make_targets(seed)
    walls = boxes[labels == 1].astype(np.float64)
    v = box_mesh(walls)[0].astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    ctr, size = 0.5 * (lo + hi), hi - lo
    slabs = np.array([[ctr[0], ctr[1], lo[2] - 0.1, size[0], size[1], 0.1, 0.0],
                      [ctr[0], ctr[1], hi[2], size[0], size[1], 0.1, 0.0]])
    vertices, triangles = box_mesh(np.concatenate([walls, slabs, CUPBOARD[None]]))
    lo, hi = vertices.min(0).astype(np.float64), vertices.max(0).astype(np.float64)
    views = (((20.0, 14.0, 1.3), (20.0, 9.55, 1.0)), ((24.0, 13.0, 1.3), (18.0, 9.55, 0.8)),
             ((5.0, 14.0, 1.3), (12.5, 9.5, 1.3)), ((5.0, 5.0, 1.3), (12.5, 9.5, 1.0)),
             ((20.0, 5.0, 1.3), (12.5, 9.0, 1.6)), ((16.0, 12.0, 1.3), (30.0, 20.0, 0.5)))
    extr = np.stack([look_at(e, t) for e, t in views])
    for e, _ in views:
        if e[1] > 9.55:
            assert 0.2 + 0.05 * abs(e[0] - 20.0) / (e[1] - 9.55) < 1.0
    return vertices, triangles, lo, hi, np.array([40.0, 40.0, 31.5, 31.5]), extr
