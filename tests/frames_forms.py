"""The designed meshes, cameras and depth frames of tests/test_frames_forms_cpu.py and tests/test_frames_forms_gpu.py, the
numpy restatement of render.hip's tile_rect, and what both modules measure on a case.  No GPU, no torch at import and no
call into the library here: numpy, tests/unproject_ref.py and (inside functions, since it imports the package)
tests/render_ref.py only.

Render cases share one geometry unless they say otherwise: the identity camera, fx = fy = 16, the principal point on a
pixel, and vertices at dyadic depths built from the pixel they should project to (`at_pixel`), so that positions are
exact in fp32 and projections and z exact in fp64.  A render case is a dict: vertices fp32 [V, 3], triangles int32
[T, 3], intr fp64 [F, 4], extr fp64 [F, 3, 4], H, W, and where it has them color, ids (name -> triangle index).

Unproject cases use two cameras of different intrinsics and rigid extrinsics in turn (`cameras`), a smooth surface
1.5 .. 3.5 m away (`surface`) and a mask of the pixels that hold a measurement."""
import numpy as np

from tests.unproject_ref import rigid, unproject_ref

TILE, BATCH, MAX_PX = 16, 256, 1e9                        # kTile, kBatch, kMaxPx of render.hip
THREADS, STEPS = 256, 8                                   # kThreads, kSteps of unproject.hip
RUN = THREADS * STEPS
NONE, BOX, WHOLE = 0, 1, 2                                # what tile_rect gives a (frame, triangle)
F_PX = 16.0
_CACHE = {}


def _rr():
    from tests import render_ref
    return render_ref


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- the restatement of tile_rect ----
def tile_rects(vertices, triangles, intr, extr, H, W):
    """render.hip's tile_rect in fp64 with its order of operations and its 1e9 px rule -> (branch int8 [F, T]: NONE, BOX or
    WHOLE; rect int32 [F, T, 4]: x0, x1, y0, y1 in tiles, meaningful where the branch is not NONE)"""
    vertices = np.asarray(vertices, np.float32)
    triangles = np.asarray(triangles, np.int32)
    E = np.asarray(extr, np.float64).reshape(-1, 3, 4)
    F, V, T = E.shape[0], vertices.shape[0], triangles.shape[0]
    K = np.broadcast_to(np.asarray(intr, np.float64).reshape(-1, 4), (F, 4))
    tx, ty = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    branch, rect = np.zeros((F, T), np.int8), np.zeros((F, T, 4), np.int32)
    listed = ((triangles >= 0) & (triangles < V)).all(1)
    listed[listed] = np.isfinite(vertices[triangles[listed]]).all((1, 2))
    with np.errstate(all="ignore"):
        for f in range(F):
            fx, fy, cx, cy = K[f]
            P = _rr().camera_space(vertices, E[f])
            cam_ok = np.isfinite(K[f]).all() and fx != 0.0 and fy != 0.0
            for t in np.flatnonzero(listed):
                p = P[triangles[t]]
                whole = (0, tx - 1, 0, ty - 1)
                if not (cam_ok and np.isfinite(p).all()):
                    branch[f, t], rect[f, t] = WHOLE, whole
                    continue
                if p[:, 2].max() <= 0.0:
                    continue
                if p[:, 2].min() <= 0.0:
                    branch[f, t], rect[f, t] = WHOLE, whole
                    continue
                u, v = p[:, 0] / p[:, 2] * fx + cx, p[:, 1] / p[:, 2] * fy + cy
                if not ((np.abs(u) < MAX_PX) & (np.abs(v) < MAX_PX)).all():
                    branch[f, t], rect[f, t] = WHOLE, whole
                    continue
                pu0, pu1 = max(np.ceil(u.min() - 1.0), 0.0), min(np.floor(u.max() + 1.0), float(W - 1))
                pv0, pv1 = max(np.ceil(v.min() - 1.0), 0.0), min(np.floor(v.max() + 1.0), float(H - 1))
                if pu0 > pu1 or pv0 > pv1:
                    continue
                branch[f, t] = BOX
                rect[f, t] = (int(pu0) // TILE, int(pu1) // TILE, int(pv0) // TILE, int(pv1) // TILE)
    return branch, rect


def tile_counts(branch, rect, H, W):
    """the list length of every tile: int64 [F, ty, tx]"""
    tx, ty = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    counts = np.zeros((branch.shape[0], ty, tx), np.int64)
    for f, t in zip(*np.nonzero(branch)):
        x0, x1, y0, y1 = rect[f, t]
        counts[f, y0:y1 + 1, x0:x1 + 1] += 1
    return counts


def case_rects(c):
    return tile_rects(c["vertices"], c["triangles"], c["intr"], c["extr"], c["H"], c["W"])


def case_counts(c):
    return tile_counts(*case_rects(c), c["H"], c["W"])


def entries(c):
    """E of every frame: the sum of its rectangles' areas, int64 [F]"""
    return case_counts(c).sum((1, 2))


def render_case_ref(c, key, **kw):
    """render_ref of a case, once per (key, keywords) -> (depth, tri, color, z)"""
    def make():
        return _rr().render_ref(c["vertices"], c["triangles"], c["intr"], c["extr"], c["H"], c["W"],
                                vertex_color=c.get("color"), **kw)
    return cached(("render", key, tuple(sorted((k, str(v)) for k, v in kw.items()))), make)


# ---- render cases ----
IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)


def at_pixel(u, v, z, cx, cy):
    """the camera-space point of depth z on the ray of pixel coordinates (u, v): exact for dyadic z and u, v in quarters"""
    return ((u - cx) / F_PX * z, (v - cy) / F_PX * z, z)


def _case(vertices, triangles, intr, extr, H, W, **more):
    vertices = np.asarray(vertices, np.float64).reshape(-1, 3)
    as32 = vertices.astype(np.float32)
    keep = np.isfinite(vertices)
    assert np.array_equal(as32.astype(np.float64)[keep], vertices[keep]), "a vertex is not exact in fp32"
    intr = np.asarray(intr, np.float64).reshape(-1, 4)
    extr = np.asarray(extr, np.float64).reshape(-1, 3, 4)
    assert intr.shape[0] == extr.shape[0]
    return dict(vertices=as32, triangles=np.asarray(triangles, np.int32).reshape(-1, 3), intr=intr, extr=extr, H=H, W=W,
                **more)


R1_SIZES = (255, 256, 257, 512, 513, 768)
R1_WINDOWS = ((0.0, np.inf), (3.0, np.inf), (6.0, np.inf), (0.0, 3.0), (0.0, 2.125), (3.0, 4.125))
R1_HITS = {255: 85, 256: 86, 257: 86, 512: 171, 513: 171, 768: 256}      # pixels hit without a bound: ceil(T / 3)


def r1_depth(i):
    """the depth of pixel triangle i: layer i % 3 at 2, 4 or 8 m, plus a 1024th of a metre per pixel"""
    i = np.asarray(i)
    return 2.0 ** (1 + i % 3) + (i // 3) / 1024.0


def r1(T, cx=8.0, H=16, W=16):
    """The first T of 768 pixel triangles: triangle i around the centre of pixel i // 3 of a 16 x 16 block (half-width a
    quarter of a pixel, so it contains that centre and no other) in layer i % 3.  Seen through cx = cy = 8 on 16 x 16
    pixels the block is the one tile of the frame; through cx = cy = 12 on 32 x 32 (the guards) it lies across four."""
    i = np.arange(T)
    k, z = i // 3, r1_depth(i)
    pu, pv = (k % 16).astype(np.float64), (k // 16).astype(np.float64)
    corners = [at_pixel(pu + du, pv + dv, z, 8.0, 8.0) for du, dv in ((-0.25, -0.25), (0.25, -0.25), (0.0, 0.25))]
    vertices = np.stack([np.stack(c, 1) for c in corners], 1)                       # [T, 3 corners, 3]
    return _case(vertices, np.arange(3 * T).reshape(T, 3), [F_PX, F_PX, cx, cx], IDENTITY, H, W)


def r7():
    """the guards' view of the R1 mesh: 32 x 32 pixels, the block of pixel triangles at pixels 4 .. 19 of both axes"""
    return r1(768, cx=12.0, H=32, W=32)


R2_DEPTHS = (0.125, 0.375, 0.625, 0.875, 16383.75, 16383.875)
R2_SCALE = 0.25
R2_QUANTA = (0, 2, 2, 4, 65535, 0)


def r2(d):
    """a wall facing the camera at depth d: the square of pixel coordinates [-8, 24]^2 around the 16 x 16 frame"""
    corners = [at_pixel(u, v, d, 8.0, 8.0) for u, v in ((-8.0, -8.0), (24.0, -8.0), (24.0, 24.0), (-8.0, 24.0))]
    return _case(corners, [[0, 1, 2], [0, 2, 3]], [F_PX, F_PX, 8.0, 8.0], IDENTITY, 16, 16)


DENORMAL = np.float32(1e-42)


def r3(uint8_color):
    """Four triangles in the quadrants of a 16 x 16 frame in front of a wall, none with a pixel centre on an edge (a weight
    of exactly 0 times +inf would make a NaN whose sign the platform chooses).  fp32 colours: NaN, +inf and -0.0 in the
    channels of triangle 0, a denormal at all corners of triangle 1, values above 255 in triangle 2, plain ones in triangle
    3; uint8 colours: 0 at all corners of triangle 0, 255 at all corners of triangle 1."""
    pts, tris = [], []
    for q, (u0, v0) in enumerate(((0.5, 0.5), (8.5, 0.5), (0.5, 8.5), (8.5, 8.5))):
        pts += [at_pixel(u0, v0, 2.0 + q, 8.0, 8.0), at_pixel(u0 + 6.75, v0, 2.0 + q, 8.0, 8.0),
                at_pixel(u0, v0 + 6.75, 4.0 + q, 8.0, 8.0)]
        tris.append([3 * q, 3 * q + 1, 3 * q + 2])
    pts += [at_pixel(u, v, 32.0, 8.0, 8.0) for u, v in ((-8.0, -8.0), (24.0, -8.0), (24.0, 24.0), (-8.0, 24.0))]
    tris += [[12, 13, 14], [12, 14, 15]]
    rs = np.random.RandomState(31)
    if uint8_color:
        color = rs.randint(1, 255, (16, 3)).astype(np.uint8)
        color[0:3], color[3:6] = 0, 255
    else:
        color = rs.rand(16, 3).astype(np.float32)
        color[0] = (np.nan, np.inf, -0.0)
        color[1] = (1.0, 300.0, -0.0)
        color[2] = (0.5, 1000.0, -0.0)
        color[3:6] = DENORMAL
        color[6:9] = ((256.5, 1e6, 3e38), (255.5, 2e6, 1e38), (1e4, 3e6, 2e38))
    return _case(pts, tris, [F_PX, F_PX, 8.0, 8.0], IDENTITY, 16, 16, color=color)


R4_H, R4_W, R4_CX, R4_CY = 37, 53, 26.0, 18.0
R4_CAMERAS = ("plain", "fx_negative", "fx_inf", "fx_zero", "fx_nan", "cx_nan", "t_nan")
# the branch tile_rect takes through the plain camera, by name
R4_PLAIN = dict(wall_a=BOX, wall_b=BOX, on_15=BOX, on_16=BOX, on_31_32=BOX, on_last=BOX, on_first=BOX, left=NONE, above=NONE,
                beyond=NONE, below=NONE, near_left=BOX, escape=WHOLE, crossing=WHOLE, behind=NONE, zero_area=BOX,
                nan_vertex=NONE, bad_index=NONE, negative_index=NONE)


def r4_mesh():
    """-> (vertices fp64 [V, 3], triangles, ids); pixel coordinates are those of the plain R4 camera, (u, v)"""
    pts, tris, ids = [], [], {}

    def add(name, *corners):
        ids[name] = len(tris)
        tris.append([len(pts), len(pts) + 1, len(pts) + 2])
        pts.extend(corners)

    def px(u, v, z):
        return at_pixel(float(u), float(v), z, R4_CX, R4_CY)
    add("wall_a", px(-8, -8, 64.0), px(60, -8, 64.0), px(60, 44, 64.0))
    add("wall_b", px(-8, -8, 64.0), px(60, 44, 64.0), px(-8, 44, 64.0))
    add("on_15", px(15, 15, 2.0), px(12, 15, 2.0), px(15, 12, 2.0))                # vertices on pixel centres at tile seams
    add("on_16", px(16, 16, 2.5), px(19, 16, 2.5), px(16, 19, 2.5))
    add("on_31_32", px(32, 31, 3.0), px(35, 31, 3.0), px(32, 34, 3.0))             # row 31, column 32
    add("on_last", px(52, 36, 3.5), px(49, 36, 3.5), px(52, 33, 3.5))              # the last pixel, in the partial tiles
    add("on_first", px(0, 0, 4.0), px(3, 0, 4.0), px(0, 3, 4.0))
    add("left", px(-5, 10, 2.0), px(-2, 10, 2.0), px(-2, 14, 2.0))                 # off the image by more than a pixel
    add("above", px(20, -5, 2.0), px(24, -2, 2.0), px(20, -2, 2.0))
    add("beyond", px(54, 20, 2.0), px(57, 20, 2.0), px(54, 24, 2.0))
    add("below", px(30, 38, 2.0), px(34, 38, 2.0), px(30, 41, 2.0))
    add("near_left", px(-3, 20, 2.0), px(-0.5, 20, 2.0), px(-0.5, 24, 2.0))        # by half a pixel: a box, and no hit
    add("escape", px(20, 20, 2.0), px(24, 20, 2.0), (1.0, 0.0, 1e-12))             # z > 0 and u = 1.6e13 px
    add("crossing", px(40, 5, 2.0), px(44, 5, 2.0), (0.25, -0.5, -1.0))
    add("behind", (0.0, 0.0, -2.0), (1.0, 0.0, -2.0), (0.0, 1.0, -3.0))
    add("zero_area", px(5, 25, 2.0), px(8, 28, 2.0), px(11, 31, 2.0))
    add("nan_vertex", px(30, 10, 2.0), (np.nan, 0.0, 2.0), px(34, 12, 2.0))
    V = len(pts)
    ids["bad_index"], ids["negative_index"] = len(tris), len(tris) + 1
    tris += [[0, 1, V], [-1, 2, 3]]
    return np.asarray(pts, np.float64), np.asarray(tris, np.int32), ids


def _fp32_exact(vertices):
    """1e-12 is not a dyadic number: take its fp32 value as the vertex"""
    return vertices.astype(np.float32).astype(np.float64)


def r4():
    vertices, triangles, ids = r4_mesh()
    intr = np.tile(np.array([F_PX, F_PX, R4_CX, R4_CY]), (len(R4_CAMERAS), 1))
    intr[1, 0], intr[2, 0], intr[3, 0], intr[4, 0], intr[5, 2] = -F_PX, np.inf, 0.0, np.nan, np.nan
    extr = np.tile(IDENTITY, (len(R4_CAMERAS), 1, 1))
    extr[6, 0, 3] = np.nan
    return _case(_fp32_exact(vertices), triangles, intr, extr, R4_H, R4_W, ids=ids)


R5_SHAPES = ((2, 1, 300), (2, 300, 1))


def r5(shape):
    """The R4 mesh in front of a frame one pixel high or wide: the principal point is moved so that row 15 (frame 0) or
    row 36 (frame 1) of the R4 image is the frame's one row, with R4's column 0 at column 100 or 240 (frame 1 has the
    triangle of the last pixel in the frame's last, partial tile, which cuts the wall); for one column, columns 15 and 16
    and R4's row 0 at rows 100 and 280."""
    vertices, triangles, ids = r4_mesh()
    F, H, W = shape
    if H == 1:
        intr = [[F_PX, F_PX, R4_CX + 100, R4_CY - 15], [F_PX, F_PX, R4_CX + 240, R4_CY - 36]]
    else:
        intr = [[F_PX, F_PX, R4_CX - 15, R4_CY + 100], [F_PX, F_PX, R4_CX - 16, R4_CY + 280]]
    return _case(_fp32_exact(vertices), triangles, intr, np.tile(IDENTITY, (2, 1, 1)), H, W, ids=ids)


def render_cases():
    """every render case by name, for the entry counts"""
    out = [(f"r1[{T}]", r1(T)) for T in R1_SIZES]
    out += [(f"r2[{d}]", r2(d)) for d in R2_DEPTHS]
    out += [("r3[fp32]", r3(False)), ("r3[uint8]", r3(True)), ("r4", r4())]
    out += [(f"r5{list(s)}", r5(s)) for s in R5_SHAPES]
    return out + [("r7", r7())]


EXACT_SHAPES = ((3, 37, 53), (2, 96, 131))                # SHAPES of tests/test_render_gpu.py
EXACT_ENTRIES = {(3, 37, 53): 481, (2, 96, 131): 1834}   # all list entries of exact_scene, from tile_rects


def exact_case(shape):
    sc = _rr().exact_scene(*shape)
    return dict(vertices=sc["vertices"], triangles=sc["triangles"], intr=sc["intr"], extr=sc["extr"], H=shape[1],
                W=shape[2])


# ---- unproject cases ----
def cameras(F, seed=21):
    """two cameras in turn"""
    intr = np.array([[70.0, 72.5, 31.25, 15.5], [55.0, 53.0, 30.0, 17.75]])
    extr = rigid(np.random.RandomState(seed), 2)
    pick = np.arange(F) % 2
    return intr[pick], extr[pick]


def surface(F, H, W):
    """z in metres, fp64 [F, H, W]: smooth, 1.5 .. 3.5 m, another phase in every frame"""
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.stack([2.5 + 0.6 * np.sin(u / 9.0 + f) + 0.4 * np.cos(v / 7.0 - f) for f in range(F)])


def depth_image(z, kept=None, float_depth=False):
    """uint16 millimetres or fp32 metres, 0 where `kept` (bool, z's shape) is False"""
    depth = z.astype(np.float32) if float_depth else np.round(z * 1000.0).astype(np.uint16)
    if kept is not None:
        depth[~kept.reshape(z.shape)] = 0
    return depth


def colour_image(shape, seed=22):
    return np.random.RandomState(seed).randint(0, 256, tuple(shape) + (3,)).astype(np.uint8)


U1_SHAPES = ((1, 23, 89), (1, 32, 64), (1, 3, 683), (2, 32, 64), (1, 17, 241))
U1_PIXELS = (2047, 2048, 2049, 4096, 4097)
U2_SHAPE = (3, 32, 64)
U3_STEPS = (2, 3, 16, 100)
U4_SHAPE = (9, 5, 100)


def u2_mask():
    """bool [6144]: run 0: steps 0, 2 and 5 dense, 1, 3 and 6 empty, step 4 keeps lane 63 of wave 3 and step 7 lane 0 of
    wave 0; run 1 empty; run 2 keeps its first and its last pixel"""
    kept = np.zeros(3 * RUN, bool)
    for s in (0, 2, 5):
        kept[s * THREADS:(s + 1) * THREADS] = True
    kept[4 * THREADS + 255] = True
    kept[7 * THREADS] = True
    kept[2 * RUN] = kept[3 * RUN - 1] = True
    return kept


def kept_census(kept):
    """kept pixels per (run, step, wave) of k_up_rows: int64 [G, 8, 4] from the flat mask"""
    kept = np.asarray(kept, bool).ravel()
    G = (kept.size + RUN - 1) // RUN
    padded = np.zeros(G * RUN, bool)
    padded[:kept.size] = kept
    return padded.reshape(G, STEPS, THREADS // 64, 64).sum(-1)


def kept_of(pix, shape):
    kept = np.zeros(int(np.prod(shape)), bool)
    kept[pix] = True
    return kept


def float_colour(shape, kept, seed=23):
    """fp32 colours with -0.0, NaN, a denormal and +inf at the first kept pixels"""
    c = np.random.RandomState(seed).rand(*(tuple(shape) + (3,))).astype(np.float32)
    flat = c.reshape(-1, 3)
    first = np.flatnonzero(kept)[:2]
    flat[first[0]] = (np.float32(-0.0), np.float32(np.nan), DENORMAL)
    flat[first[1]] = (np.float32(np.inf), np.float32(-np.inf), -DENORMAL)
    flat[np.flatnonzero(kept)[-1]] = (DENORMAL, np.float32(-0.0), np.float32(np.nan))
    return c


def unproject_case(name, shape, float_depth=False, mask=None, color="uint8", cams=None):
    """-> dict(depth, color, intr, extr), built once per name"""
    def make():
        z = surface(*shape)
        intr, extr = cameras(shape[0]) if cams is None else cams
        kept = np.ones(z.size, bool) if mask is None else mask
        col = {"uint8": lambda: colour_image(shape), "fp32": lambda: float_colour(shape, kept), None: lambda: None}[color]()
        return dict(depth=depth_image(z, mask, float_depth), color=col, intr=intr, extr=extr)
    return cached(("unproject", name, shape, float_depth, color), make)


def unproject_case_ref(c, key, **kw):
    """unproject_ref of a case at nine columns, once per (key, keywords): fewer columns are its leading ones"""
    def make():
        return unproject_ref(c["depth"], c["intr"], c["extr"], color=c["color"], columns=9, **kw)
    return cached(("unproject_ref", key, tuple(sorted(kw.items()))), make)


def u4_cameras():
    rs = np.random.RandomState(24)
    intr = np.stack([np.array([60.0 + 2 * i, 58.0 - i, 49.5 + 0.25 * i, 2.0 + 0.125 * i]) for i in range(U4_SHAPE[0])])
    return intr, rigid(rs, U4_SHAPE[0])
