"""The designed volumes and frame stacks of tests/test_tsdf_forms_cpu.py and tests/test_tsdf_forms_gpu.py, and what both
measure on a result.  No GPU and no call into the library here: numpy, tests/tsdf_ref.py and tests/tsdf_mesh_ref.py only.

Every volume has voxel 0.25 and the origin (0.5, -1.25, 2.0), its blocks start at BASE = (3, 5, 7), and its tsdf values
are multiples of 1/8 (or the stated special values), so positions of voxels are exact in fp32 and the invariants below
hold without a tolerance.  A case is a dict: blocks = (coords int32 [B, 3] ascending, D, W fp32 [B, 8, 8, 8], C, CW or
None, None), voxel, origin, and what the case adds (min_weights, max_blocks, named voxels)."""
import itertools

import numpy as np

from tests.tsdf_mesh_ref import KIND_DIR, mesh_ref
from tests.tsdf_ref import TsdfRef, room_colors, room_frames

VOXEL, ORIGIN, BASE = 0.25, (0.5, -1.25, 2.0), (3, 5, 7)
SUB, TINY = np.float32(2.0 ** -149), np.float32(2.0 ** -126)      # the smallest subnormal and the smallest normal fp32
_L = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1)     # [8, 8, 8, 3]


# ---- building blocks ----
def dense_to_blocks(coords, *dense):
    """dense arrays [8 nx, 8 ny, 8 nz, ...] over the box that starts at block coords.min(0) -> one [B, 8, 8, 8, ...] each"""
    coords = np.asarray(coords, np.int64)
    lo = coords.min(0)
    out = []
    for a in dense:
        out.append(None if a is None else np.stack(
            [a[tuple(slice(8 * (c[i] - lo[i]), 8 * (c[i] - lo[i]) + 8) for i in range(3))] for c in coords]))
    return out


def cube_coords(n=2, base=BASE):
    """the n^3 blocks base + (0..n-1)^3 in ascending (x, y, z)"""
    return (np.array(list(itertools.product(range(n), repeat=3)), np.int64) + np.array(base, np.int64)).astype(np.int32)


def random_signs(shape, rs):
    """+-k / 8, k in 1..7, the sign and k seeded"""
    return (rs.choice([-1.0, 1.0], shape) * rs.randint(1, 8, shape) / 8.0).astype(np.float32)


def random_colour(shape, rs):
    """C in multiples of 1/256, CW = 0 on a fifth of the voxels and 1..3 elsewhere; C = 0 where CW = 0"""
    C = (rs.randint(0, 256, tuple(shape) + (3,)) / 256.0).astype(np.float32)
    CW = ((rs.rand(*shape) > 0.2) * rs.randint(1, 4, shape)).astype(np.float32)
    C[CW == 0] = 0
    return C, CW


def _case(coords, D, W, C=None, CW=None, **more):
    coords = np.asarray(coords, np.int32)
    order = np.lexsort((coords[:, 2], coords[:, 1], coords[:, 0]))
    pick = lambda a: None if a is None else np.ascontiguousarray(a[order])
    return dict(blocks=(coords[order], pick(D), pick(W), pick(C), pick(CW)), voxel=VOXEL, origin=ORIGIN,
                min_weights=(1,), **more)


def _random8_dense(seed=8):
    rs = np.random.RandomState(seed)
    D = random_signs((16, 16, 16), rs)
    C, CW = random_colour((16, 16, 16), rs)
    return D, np.ones((16, 16, 16), np.float32), C, CW


def random8():
    coords = cube_coords()
    return _case(coords, *dense_to_blocks(coords, *_random8_dense()))


def random1():
    rs = np.random.RandomState(1)
    D = random_signs((1, 8, 8, 8), rs)
    C, CW = random_colour((1, 8, 8, 8), rs)
    return _case(cube_coords(1), D, np.ones_like(D), C, CW)


def checker():
    g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).sum(-1)
    D = np.where(g % 2 == 0, -0.5, 0.5).astype(np.float32)
    coords = cube_coords()
    return _case(coords, *dense_to_blocks(coords, D, np.ones_like(D)))


def closed():
    D, W, C, CW = _random8_dense()
    shell = np.ones((16, 16, 16), bool)
    shell[1:15, 1:15, 1:15] = False
    D = np.where(shell, np.float32(0.5), D)
    coords = cube_coords()
    return _case(coords, *dense_to_blocks(coords, D, W, C, CW))


WEIGHT_VALUES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, np.nan, np.inf, -1.0], np.float32)


def weights():
    D, _, C, CW = _random8_dense()
    W = WEIGHT_VALUES[np.random.RandomState(9).randint(0, len(WEIGHT_VALUES), (16, 16, 16))]
    coords = cube_coords()
    case = _case(coords, *dense_to_blocks(coords, D, W, C, CW))
    case["min_weights"] = (0, 0.5, 1, 2)
    return case


# `signs`: two blocks side by side in x, +1 everywhere but on two lines.  LINE_X runs along x at (y, z) = (2, 2) of the
# pair from x = 4 and passes the blocks' border between x = 7 and 8; LINE_Y runs along y at (x, z) = (2, 5) from y = 2.
LINE_X = np.array([-1.0, -0.0, 1.0, 0.0, -1.0, -SUB, 0.0, SUB, -TINY, TINY, -SUB, 1.0], np.float32)
LINE_Y = np.array([-0.0, -1.0, 1.0], np.float32)


def signs():
    D = np.ones((16, 8, 8), np.float32)
    D[4:16, 2, 2] = LINE_X
    D[2, 2:5, 5] = LINE_Y
    coords = np.array([BASE, (BASE[0] + 1, BASE[1], BASE[2])], np.int32)
    return _case(coords, *dense_to_blocks(coords, D, np.ones_like(D)))


def signs_voxel(x, y, z):
    """the global voxel of (x, y, z) of the block pair"""
    return 8 * np.array(BASE, np.int64) + np.array((x, y, z), np.int64)


NONFINITE_VALUES = np.array([np.nan, np.inf, -np.inf], np.float32)


def nonfinite(twin=False):
    """random8 with 60 voxels set to NaN, +inf and -inf; twin: the same volume with those voxels' W = 0"""
    D, W, C, CW = _random8_dense()
    rs = np.random.RandomState(10)
    at = np.unravel_index(rs.choice(16 ** 3, 60, replace=False), (16, 16, 16))
    D, W = D.copy(), W.copy()
    D[at] = NONFINITE_VALUES[np.arange(60) % 3]
    if twin:
        W[at] = 0
    coords = cube_coords()
    return _case(coords, *dense_to_blocks(coords, D, W, C, CW), bad=np.stack(at, 1) + 8 * np.array(BASE, np.int64))


CORNER_VOXEL = (7, 7, 7)                                  # of block BASE: its seven forward edges each end in another block


def corner(without=0):
    """random8 with voxel CORNER_VOXEL of block BASE inside and its seven forward neighbours outside: a sign changes
    exactly across a block face (+x, +y, +z), a block edge (+xy, +xz, +yz) and the corner the eight blocks share (+xyz).
    without: the forward neighbour o = ox | oy << 1 | oz << 2 of block BASE that is left out, 0 for none"""
    D, W, C, CW = _random8_dense()
    D = D.copy()
    D[7:9, 7:9, 7:9] = 0.5
    D[CORNER_VOXEL] = -0.25
    coords = cube_coords()
    if without:
        coords = np.delete(coords, 4 * (without & 1) + 2 * ((without >> 1) & 1) + ((without >> 2) & 1), 0)
    return _case(coords, *dense_to_blocks(coords, D, W, C, CW))        # block BASE stays, so the dense box starts there


PARITY_BASE = (4, 6, 8)
PARITY_MAX_BLOCKS = 512


def parity():
    """200 blocks at PARITY_BASE + 2 (i, j, k), i, j, k < 6 (the first 200 in ascending order), and 12 blocks with one
    odd coordinate at +x, +y and +z of some of them; through every block the plane lz = 3.5 - shift, shift in {-1, 0, 1}
    by the block's coordinate sum: D = (2 lz - 7 + 2 shift) / 16"""
    even = np.array(list(itertools.product(range(6), repeat=3)), np.int64)[:200] * 2 + np.array(PARITY_BASE, np.int64)
    odd = np.concatenate([even[[5 + 17 * j for j in range(4)]] + np.eye(3, dtype=np.int64)[a] for a in range(3)])
    coords = np.concatenate([even, odd])
    shift = coords.sum(1) % 3 - 1
    D = ((2.0 * _L[None, ..., 2] - 7.0 + 2.0 * shift[:, None, None, None]) / 16.0).astype(np.float32)
    return _case(coords, D, np.ones_like(D), max_blocks=PARITY_MAX_BLOCKS)


def look_frame(eye):
    """One frame of 6 x 8 pixels from `eye`, looking along +x at depths of 3 .. 3.875 m
    -> (depth fp32 [1, 6, 8], intrinsics [1, 4], extrinsics [1, 3, 4])"""
    v, u = np.mgrid[0:6, 0:8]
    depth = (3.0 + ((3 * u + 5 * v) % 8) / 8.0).astype(np.float32)[None]
    intr = np.array([[6.0, 6.0, 3.5, 2.5]])
    extr = np.array([[[0.0, 0.0, 1.0, eye[0]], [1.0, 0.0, 0.0, eye[1]], [0.0, 1.0, 0.0, eye[2]]]])
    return depth, intr, extr


PARITY_TARGET = (14, 14, 12)                              # PARITY_BASE + 2 (5, 4, 2): one of the 16 lattice points left out


def parity_frame():
    """From inside the parity volume towards the middle of block PARITY_TARGET, 3.5 m away: it updates old blocks on the
    way and needs new ones, among them PARITY_TARGET, whose key shares the position of the 200 and so must pass all 128
    full slots of that position and take the turn, in block_touch, whatever order the 200 were inserted in"""
    return look_frame(np.array(ORIGIN) + 8.0 * VOXEL * (np.array(PARITY_TARGET) + 0.5) - np.array([3.5, 0.0, 0.0]))


def nonfinite_frame():
    """from 2.5 m in front of the random8 volume's -x face, at its middle"""
    return look_frame(np.array(ORIGIN) + 8.0 * VOXEL * np.array(BASE) + np.array([-2.5, 2.0, 2.0]))


CORNER_CASES = ("corner",) + tuple(f"corner_without_{o}" for o in range(1, 8))
CASES = dict(random8=random8, random1=random1, checker=checker, closed=closed, weights=weights, signs=signs,
             nonfinite=nonfinite, nonfinite_twin=lambda: nonfinite(twin=True), parity=parity, corner=corner,
             **{f"corner_without_{o}": (lambda o=o: corner(o)) for o in range(1, 8)})
MESH_CASES = ("random8", "random1", "checker", "closed", "weights", "signs", "nonfinite", "parity")
_CACHE = {}


def memo(key, build):
    """build() computed once under `key` and shared, never changed afterwards"""
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def case(name):
    """the case, built once and never changed afterwards"""
    return memo(name, CASES[name])


def case_mesh(name, min_weight=1):
    """mesh_ref of the case, computed once"""
    key = (name, "mesh", min_weight)
    if key not in _CACHE:
        c = case(name)
        _CACHE[key] = mesh_ref(c["blocks"], c["voxel"], c["origin"], min_weight)
    return _CACHE[key]


def case_surface(name, columns=9, min_weight=1):
    """TsdfRef.surface_points of the case, computed once"""
    key = (name, "surface", columns, min_weight)
    if key not in _CACHE:
        _CACHE[key] = load_case(name).surface_points(columns, min_weight)
    return _CACHE[key]


# ---- the loader ----
def load_ref(coords, D, W, C, CW, voxel, origin, trunc=None):
    """a TsdfRef that holds the given blocks, as TsdfVolume.from_blocks does: surface_points and integrate go on from
    there"""
    ref = TsdfRef(voxel, trunc, origin, color=C is not None)
    n = len(coords)
    ref.coords = np.asarray(coords, np.int64).reshape(n, 3).copy()
    ref.index = {tuple(c): j for j, c in enumerate(ref.coords.tolist())}
    ref.D = np.asarray(D, np.float32).reshape(n, 512).copy()
    ref.W = np.asarray(W, np.float32).reshape(n, 512).copy()
    ref.C = np.zeros((n, 512, 3), np.float32) if C is None else np.asarray(C, np.float32).reshape(n, 512, 3).copy()
    ref.CW = np.zeros((n, 512), np.float32) if CW is None else np.asarray(CW, np.float32).reshape(n, 512).copy()
    return ref


def load_case(name):
    c = case(name)
    return load_ref(*c["blocks"], c["voxel"], c["origin"])


def carried_on(name):
    """the loaded case `name` (parity or nonfinite) after integrate of its frame, computed once"""
    frame = dict(parity=parity_frame, nonfinite=nonfinite_frame)[name]
    return memo((name, "carried on"), lambda: load_case(name).integrate(*frame()))


def surface_of(key, ref, columns):
    """ref.surface_points(columns), computed once under `key`"""
    return memo((key, "surface of", columns), lambda: ref.surface_points(columns))


# ---- what the tests measure ----
class Dense(object):
    """the blocks as one array over their bounding box, looked up by global voxel: D (NaN where no block is), W, CW and
    `present`"""

    def __init__(self, blocks):
        coords, D, W, C, CW = blocks
        coords = np.asarray(coords, np.int64)
        self.lo = 8 * coords.min(0)
        n = 8 * (coords.max(0) - coords.min(0) + 1)
        self.D = np.full(n, np.nan, np.float32)
        self.W = np.full(n, np.nan, np.float32)
        self.CW = np.zeros(n, np.float32)
        self.present = np.zeros(n, bool)
        for j, c in enumerate(8 * coords - self.lo):
            s = tuple(slice(c[i], c[i] + 8) for i in range(3))
            self.D[s], self.W[s], self.present[s] = D[j], W[j], True
            if CW is not None:
                self.CW[s] = CW[j]
        self.n = np.array(n)

    def at(self, a, g):
        """a[g] for global voxels g [N, 3] inside the box"""
        q = np.asarray(g, np.int64) - self.lo
        assert ((q >= 0) & (q < self.n)).all()
        return a[q[:, 0], q[:, 1], q[:, 2]]

    def seen(self, min_weight):
        with np.errstate(invalid="ignore"):
            return self.present & (self.W.astype(np.float64) >= min_weight) & np.isfinite(self.D)


def block_of(g):
    """the block coordinate of global voxels [N, 3] as one int64 per row, ascending like (x, y, z)"""
    b = np.asarray(g, np.int64) // 8
    return (b[:, 0] << 32) | (b[:, 1] << 16) | b[:, 2]


def per_block(g):
    """-> (the number of rows in each block, each row's index inside its block) for rows ordered by block"""
    key = block_of(g)
    assert (np.diff(key) >= 0).all()
    uniq, first, counts = np.unique(key, return_index=True, return_counts=True)
    return counts, np.arange(len(key)) - np.repeat(first, counts)


def cell_configurations(blocks, min_weight=1):
    """the corner configurations sum inside(g + c) 2^(cx + 2 cy + 4 cz) of every cell whose eight corners are seen"""
    d = Dense(blocks)
    seen, inside = d.seen(min_weight), d.D < 0
    m = d.n - 1
    sh = lambda a, c: a[tuple(slice(c[i], c[i] + m[i]) for i in range(3))]
    ok, conf = np.ones(m, bool), np.zeros(m, np.int64)
    for c in itertools.product((0, 1), repeat=3):
        ok &= sh(seen, c)
        conf |= sh(inside, c).astype(np.int64) << (c[0] + 2 * c[1] + 4 * c[2])
    return conf[ok]


def vertex_ends(edges):
    """-> (g, h) global voxels [V, 3] of the edge of every vertex"""
    e = np.asarray(edges, np.int64)
    return e[:, :3], e[:, :3] + KIND_DIR[e[:, 3]]


def vertices_on_their_edges(vertices, edges, voxel, origin):
    """The first invariant: a vertex equals X_g on the axes where its edge does not move and lies in [X_g, X_g + voxel]
    on those where it does.  Exact: X is a multiple of the voxel, itself a power of two.  -> strict bool [V]: the vertex
    is at neither end"""
    g, h = vertex_ends(edges)
    Xg = np.asarray(origin, np.float64) + g.astype(np.float64) * voxel
    v = np.asarray(vertices, np.float64)
    move = (h - g) == 1
    assert np.isfinite(v).all()
    assert (v[~move] == Xg[~move]).all()
    assert ((v >= Xg) & (v <= Xg + voxel))[move].all()
    return (~move | ((v > Xg) & (v < Xg + voxel))).all(1)


def triangles_face_outwards(vertices, triangles, edges, blocks, voxel, origin, scope):
    """The second invariant: (v1 - v0) x (v2 - v0) has a positive dot product with the step from the mean of the inside
    corners to the mean of the outside corners; scope "cell": the eight corners of the triangle's cell, "tet": the four
    corners of its tetrahedron (the ends of its vertices' edges).  Where a vertex sits at an end of its edge (D = 0, or
    an s that fp32 rounds away) the triangle may have no area and the product is only required not to be negative.
    -> the number of triangles checked strictly"""
    d = Dense(blocks)
    g, h = vertex_ends(edges)
    tri = np.asarray(triangles, np.int64)
    if len(tri) == 0:
        return 0
    v = np.asarray(vertices, np.float64)[tri]                                     # [T, 3, 3]
    normal = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    ends = np.concatenate([g[tri], h[tri]], 1)                                    # [T, 6, 3]
    cell = ends.min(1)
    assert (ends.max(1) - cell <= 1).all()                                        # the edges lie in one cell
    if scope == "cell":
        corners = cell[:, None, :] + np.array(list(itertools.product((0, 1), repeat=3)), np.int64)[None]
        weight = np.ones(corners.shape[:2])
    else:
        corners = ends                                                            # each corner once or more; weigh by 1 / times
        same = (ends[:, :, None, :] == ends[:, None, :, :]).all(-1)
        weight = 1.0 / same.sum(2)
        assert np.allclose(weight.sum(1), 4.0)                                    # four distinct corners: a tetrahedron
    T = len(tri)
    inside = (d.at(d.D, corners.reshape(-1, 3)) < 0).reshape(T, -1)
    w_in, w_out = weight * inside, weight * ~inside
    assert (w_in.sum(1) > 0).all() and (w_out.sum(1) > 0).all()
    c = corners.astype(np.float64)
    step = (c * w_out[..., None]).sum(1) / w_out.sum(1)[:, None] - (c * w_in[..., None]).sum(1) / w_in.sum(1)[:, None]
    dot = (normal * step).sum(1)
    Xg = np.asarray(origin, np.float64) + g.astype(np.float64) * voxel
    move = (h - g) == 1
    vv = np.asarray(vertices, np.float64)
    strict_v = (~move | ((vv > Xg) & (vv < Xg + voxel))).all(1)
    strict = strict_v[tri].all(1)
    assert (dot >= 0).all(), (scope, int((dot < 0).sum()), T)
    assert (dot[strict] > 0).all(), (scope, int((dot[strict] <= 0).sum()), T)
    return int(strict.sum())


# ---- the hash table of the volume, restated ----
_M64 = (1 << 64) - 1
PROBE_STEP = 8


def table_slots(max_blocks):
    c = 1024
    while c < 2 * max_blocks:
        c <<= 1
    return c


def pack_key(x, y, z):
    return (int(x) << 32) | (int(y) << 16) | int(z)


def hash_key(k):
    intra = ((k >> 32) & 1) << 2 | ((k >> 16) & 1) << 1 | (k & 1)
    k &= ~0x0000000100010001 & _M64
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & _M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & _M64
    k ^= k >> 33
    return (((k & 0xffffffff) << 3) & 0xffffffff) | intra


def table_walk(table, key):
    """the probe sequence of block_find / block_touch / k_tsdf_insert for `key` in table (a list of keys, None = empty)
    -> (the slot that holds the key or the first empty one, the number of times the walk took the slot + 1 turn)"""
    cap = len(table)
    slot, rnd, turns = hash_key(key) & (cap - 1), 0, 0
    for _ in range(cap):
        if table[slot] is None or table[slot] == key:
            return slot, turns
        slot = (slot + PROBE_STEP) & (cap - 1)
        rnd += 1
        if rnd == cap // PROBE_STEP:
            rnd, turns = 0, turns + 1
            slot = (slot + 1) & (cap - 1)
    return -1, turns


def table_census(coords, max_blocks):
    """inserts the coordinates in the order given, then looks every one up -> (slots, the largest number of keys that
    share one position inside a group, insertions that took the turn, look-ups that took the turn)"""
    cap = table_slots(max_blocks)
    table = [None] * cap
    keys = [pack_key(*c) for c in np.asarray(coords).tolist()]
    turned_in = 0
    for k in keys:
        slot, turns = table_walk(table, k)
        assert slot >= 0 and table[slot] is None
        table[slot] = k
        turned_in += turns > 0
    turned_out = sum(table_walk(table, k)[1] > 0 for k in keys)
    share = np.bincount([hash_key(k) & 7 for k in keys], minlength=8).max()
    return cap, int(share), turned_in, turned_out


# ---- frame stacks ----
FRAMES_VOLUME = dict(voxel=0.2, trunc=0.8, origin=(-1.0, -1.0, -1.0))


def frames513(F, color=False):
    """the room's five cameras at 6 x 8 pixels, cycled to F frames -> (depth, intrinsics, extrinsics, uint8 colour or None)"""
    key = ("frames", F, color)
    if key not in _CACHE:
        depth, intr, extr = room_frames(6, 8, near_wall=True)
        col = room_colors(depth) if color else None
        i = np.arange(F) % len(depth)
        _CACHE[key] = (np.ascontiguousarray(depth[i]), np.ascontiguousarray(intr[i]), np.ascontiguousarray(extr[i]),
                       None if col is None else np.ascontiguousarray(col[i]))
    return _CACHE[key]


def frames_ref(F, color=False, calls=None):
    """TsdfRef of frames513(F, color) integrated in `calls` (first, last), default one call; computed once"""
    calls = ((0, F),) if calls is None else calls
    key = ("frames ref", F, color, calls)
    if key not in _CACHE:
        depth, intr, extr, col = frames513(F, color)
        ref = TsdfRef(color=color, **FRAMES_VOLUME)
        for a, b in calls:
            ref.integrate(depth[a:b], intr[a:b], extr[a:b], None if col is None else col[a:b])
        _CACHE[key] = ref
    return _CACHE[key]


PIXELS_VOLUME = dict(voxel=0.25, trunc=1.0, origin=(-8.0, -8.0, -2.0))


def pixels(width, last=True):
    """One frame of 1 x width pixels, a 90 degree fan from (0, 0, 0.5) along +x: depths 2 .. 2.875 m with a hole every
    11th pixel, and 6 m at the last pixel, which alone needs the blocks out there; last=False: that pixel is a hole"""
    u = np.arange(width)
    depth = (2.0 + (u % 8) / 8.0).astype(np.float32)
    depth[u % 11 == 3] = 0
    depth[-1] = 6.0 if last else 0.0
    intr = np.array([[1024.0, 1024.0, 0.5 * (width - 1), 0.0]])
    extr = np.array([[[0.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.5]]])
    return depth[None, None, :], intr, extr


def pixels_ref(width, step=1, last=True):
    key = ("pixels ref", width, step, last)
    if key not in _CACHE:
        depth, intr, extr = pixels(width, last)
        _CACHE[key] = TsdfRef(color=False, **PIXELS_VOLUME).integrate(depth, intr, extr, step=step)
    return _CACHE[key]
