"""The front of every pass restated in numpy, and the designed cases its tests run on: the voxelizer
(detection_3d_amd/csrc/voxelize.hip), the input layer (grid.hip, k_input_backward with it; scan_exclusive_i32 of
scan_sort.hip underneath both), the views of a finished grid (grid_views.hip: locations, sparse <-> dense, anchors) and the
two row helpers at the end of bn.hip (d3d_add, d3d_rows_to_bf16).  numpy only: no GPU, no oracle library.  The references
are plain fp64 / integer restatements; tests/test_front_forms_cpu.py holds them against the oracle and asserts that the
cases sit where their names say, tests/test_front_forms_gpu.py runs the kernels on them."""
import functools
from fractions import Fraction

import numpy as np

SCAN_TILE = 2048                       # kScanTile: elements per tile sum of scan_exclusive_i32
SUM_ROUND = 256                        # kSumThreads: tile sums per round of k_scan_sums
SECOND_ROUND = SUM_ROUND * SCAN_TILE + 1          # 524289: the first length whose tile sums need a second round (a carry)
U24 = 2.0 ** -24                       # unit roundoff of fp32


def bits(a):
    """fp32 array -> its uint32 bit patterns (NaN payloads and the sign of zero compare)"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U24 / (1.0 - k * U24)


# =================================================================================================== voxelizer
def voxelize_reference(pcl, scale, full):
    """-> (coords int64 [M, 3], feats fp32 [M, F], keep bool [N]).  a = double(x) * scale, off = -fmin(a) (a NaN is
    ignored: the kernel's contract), a += off as a second operation, keep 0 <= a < full, trunc; feats[:, :3] = a / scale,
    the other columns untouched."""
    pcl = np.ascontiguousarray(pcl, np.float32)
    n = pcl.shape[0]
    if n == 0:
        return np.zeros((0, 3), np.int64), pcl.copy(), np.zeros(0, bool)
    a = pcl[:, :3].astype(np.float64) * np.float64(scale)
    with np.errstate(invalid="ignore"):
        off = -np.fmin.reduce(a, 0)
        a = a + off
        keep = np.all((a >= 0) & (a < np.asarray(full, np.float64)[None, :]), 1)
        feats = pcl[keep].copy()
        feats[:, :3] = (a[keep] / np.float64(scale)).astype(np.float32)
        return np.trunc(a[keep]).astype(np.int64), feats, keep


SNAN_BITS = 0x7FA00000                 # a signalling NaN: quiet bit clear, payload set
# NaN (not 0x7FC00000: that is the sentinel the outputs are prefilled with), -NaN with payload, +Inf, -Inf, -0, sNaN, the
# subnormals' ends
SPECIAL_BITS = np.array([0x7FC00123, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, SNAN_BITS, 0x00000001, 0x807FFFFF],
                        np.uint32)


def _passthrough(rng, n, nfeat):
    """columns 3.. of a cloud: normal values, every 7th row's first extra column one of SPECIAL_BITS"""
    extra = rng.randn(n, nfeat - 3).astype(np.float32)
    if nfeat > 3 and n:
        rows = np.arange(0, n, 7)
        extra.view(np.uint32)[rows, (rows // 7) % (nfeat - 3)] = SPECIAL_BITS[(rows // 7) % len(SPECIAL_BITS)]
    return extra


VOX_N = (1, 2047, 2048, 2049, 524288, 524289)
VOX_PATTERNS = {                       # name -> (n, nfeat); the kept mask each one intends: vox_intended_keep
    "all-1": (1, 3), "all-2047": (2047, 4), "all-2048": (2048, 9), "all-2049": (2049, 12), "all-524288": (524288, 3),
    "all-524289": (524289, 4),
    "alternate-2049": (2049, 9), "alternate-524289": (524289, 3),
    "last_only-2049": (2049, 4), "last_only-524289": (524289, 3),
    "runs-524289": (524289, 4),        # dropped [2040, 2056) and [524280, 524288), the last point kept
    "run_to_end-2049": (2049, 3),      # dropped [2040, 2049)
    "run_to_end-524289": (524289, 3),  # dropped [524280, 524289)
    "none-2049": (2049, 9), "none-524289": (524289, 3),
}
VOX_PATTERN_FULL = (64, 64, 64)


def vox_intended_keep(name):
    kind, n = name.split("-")
    n = int(n)
    i = np.arange(n)
    if kind == "all":
        return np.ones(n, bool)
    if kind == "alternate":
        return i % 2 == 0
    if kind == "last_only":
        return i == n - 1
    if kind == "runs":
        return ~(((i >= 2040) & (i < 2056)) | ((i >= 524280) & (i < 524288)))
    if kind == "run_to_end":
        return i < (2040 if n == 2049 else 524280)
    assert kind == "none"
    return np.zeros(n, bool)


@functools.lru_cache(maxsize=None)
def vox_pattern_case(name):
    """-> (pcl, scale 50, full).  Kept points lie in [0, 60) voxels of a 64-voxel cube, the first point at the origin of
    the cloud; a dropped point sits 500 voxels out on x.  `none`: full (4, 4, 4), every point 100 voxels out on x or y."""
    n, nfeat = VOX_PATTERNS[name]
    rng = np.random.RandomState(n % 1000 + 7 * nfeat + len(name))
    keep = vox_intended_keep(name)
    u = rng.rand(n, 3) * 60.0
    if name.startswith("none"):
        u = rng.rand(n, 3) * 3.0
        u[np.arange(n) % 2 == 0, 0] += 100.0
        u[np.arange(n) % 2 == 1, 1] += 100.0
        u[0], u[1] = (100.0, 0.0, 0.0), (0.0, 100.0, 0.0)
        full = (4, 4, 4)
    else:
        u[~keep, 0] += 500.0
        u[np.argmax(keep)] = 0.0                       # the first kept point is the minimum on every axis
        full = VOX_PATTERN_FULL
    pcl = np.concatenate([(u / 50.0 - 1.25).astype(np.float32), _passthrough(rng, n, nfeat)], 1)
    pcl.setflags(write=False)
    return pcl, 50.0, full


BOUNDARY_FULL = (100, 50, 200)         # a == full at x = 2, 1, 4 exactly
BOUNDARY_K = (50, 25, 100)             # a == k at x = 1, 0.5, 2 exactly


@functools.lru_cache(maxsize=None)
def vox_boundary_case():
    """scale 50, the minimum 0 on every axis, so a = 50 x exactly (24 x 6 bits).  Per axis d, with the other axes at
    a = 12.5: a = 0; a = k and its fp32 neighbours; the largest fp32 below full; full itself.
    -> (pcl [19, 4], 50, full, rows): rows[i] = (axis, what, expected coordinate or None when dropped)"""
    pts, rows = [(0.0, 0.0, 0.0)], [(-1, "origin", 0)]
    for d in range(3):
        k, f = np.float32(BOUNDARY_K[d] / 50.0), np.float32(BOUNDARY_FULL[d] / 50.0)
        for what, x, want in (("zero", np.float32(0), 0), ("k", k, BOUNDARY_K[d]),
                              ("k_below", np.nextafter(k, np.float32(0)), BOUNDARY_K[d] - 1),
                              ("k_above", np.nextafter(k, np.float32(9)), BOUNDARY_K[d]),
                              ("full_below", np.nextafter(f, np.float32(0)), BOUNDARY_FULL[d] - 1), ("full", f, None)):
            p = [0.25, 0.25, 0.25]
            p[d] = x
            pts.append(tuple(p))
            rows.append((d, what, want))
    xyz = np.array(pts, np.float32)
    pcl = np.concatenate([xyz, np.arange(len(pts), dtype=np.float32)[:, None]], 1)
    pcl.setflags(write=False)
    return pcl, 50.0, BOUNDARY_FULL, rows


@functools.lru_cache(maxsize=None)
def vox_negative_case():
    """every coordinate negative: the shift is positive and a = x * 50 + off takes two roundings' worth of care"""
    rng = np.random.RandomState(11)
    pcl = np.concatenate([(-3.0 + 2.0 * rng.rand(2049, 3)).astype(np.float32), _passthrough(rng, 2049, 9)], 1)
    pcl.setflags(write=False)
    return pcl, 50.0, (4096, 4096, 512)


# Scales whose fp64 significand is full.  (100 / 3 and 1 / 0.03 round to the same double, 0x1.0aaaaaaaaaaabp+5: both
# are kept because both spellings occur; 100 / 7 is a different one.)  For a scale p / q the points xm + (q / 4) t give
# (x - xm) * scale = (p / 4) t up to the scale's own rounding: an integer, with the minimum xm far from zero so that its
# rounded product carries half an ulp of error.  Found by search: the minima (in units of 2^-16) below make the exact
# x * scale - fl(xm * scale) fall just under the integer for several t while the two-rounding value lands on it.
NONDYADIC = {
    "100/3": (100.0 / 3.0, 0.75, (-4000001, -3500003, -4000001)),
    "1/0.03": (1.0 / 0.03, 0.75, (-4000001, -3500003, -4000001)),
    "100/7": (100.0 / 7.0, 1.75, (-3999999, -3500003, -3999999)),
}
NONDYADIC_T = 48


@functools.lru_cache(maxsize=None)
def vox_nondyadic_case(name):
    scale, step, mins = NONDYADIC[name]
    xyz = np.empty((NONDYADIC_T + 1, 3), np.float64)
    for d in range(3):
        xyz[:, d] = mins[d] * 2.0 ** -16 + step * np.arange(NONDYADIC_T + 1)
    f = xyz.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), xyz)                       # every point is an fp32 value
    pcl = np.concatenate([f, np.arange(len(f), dtype=np.float32)[:, None]], 1)
    pcl.setflags(write=False)
    return pcl, scale, (4096, 4096, 4096)


def contraction_sensitive(pcl, scale):
    """bool [N, 3]: where one fused multiply-add (the exact x * scale + off, rounded once: evaluated in rationals) would
    truncate to another integer than the multiply followed by the add"""
    x = np.asarray(pcl, np.float32)[:, :3].astype(np.float64)
    a = x * np.float64(scale)
    off = -np.fmin.reduce(a, 0)
    two = a + off
    out = np.zeros(two.shape, bool)
    for i in range(x.shape[0]):
        for d in range(3):
            exact = Fraction(float(x[i, d])) * Fraction(float(scale)) + Fraction(float(off[d]))
            out[i, d] = int(float(exact)) != int(two[i, d])          # float(Fraction) rounds once, to nearest even
    return out


NONFINITE = ("nan", "+inf", "-inf")


def vox_nonfinite_case(kind):
    """a 300-point cloud with one non-finite coordinate on y of point 150 -> (pcl, scale, full, row)"""
    rng = np.random.RandomState(5)
    pcl = np.concatenate([rng.rand(300, 3).astype(np.float32), _passthrough(rng, 300, 4)], 1)
    pcl[150, 1] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[kind]
    return pcl, 50.0, (4096, 4096, 512), 150


# =================================================================================================== input layer
def input_sites_reference(coords):
    """coords int64 [n, 3 | 4] -> (site of every point int32 [n], locations int32 [n_active, 4]): sites numbered by the
    first occurrence of the row (x, y, z, b) in input order"""
    coords = np.asarray(coords, np.int64)
    n = coords.shape[0]
    if n == 0:
        return np.zeros(0, np.int32), np.zeros((0, 4), np.int32)
    rows = np.concatenate([coords, np.zeros((n, 1), np.int64)], 1) if coords.shape[1] == 3 else coords
    key = ((rows[:, 3] * 32768 + rows[:, 0]) * 32768 + rows[:, 1]) * 32768 + rows[:, 2]
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    site = np.empty(len(first), np.int64)
    site[order] = np.arange(len(first))
    return site[inv.reshape(-1)].astype(np.int32), rows[first[order]].astype(np.int32)


def point_lists_reference(sop, n_active):
    """-> (offsets int32 [n_active + 1], idx int32 [n]): every site's points, ascending point index"""
    sop = np.asarray(sop, np.int64)
    off = np.zeros(n_active + 1, np.int64)
    np.cumsum(np.bincount(sop, minlength=n_active), out=off[1:])
    return off.astype(np.int32), np.argsort(sop, kind="stable").astype(np.int32)


def input_forward_reference(feats, sop, n_active, average):
    """-> (y fp64 [n_active, C] = sum of mult * x, sum of |x| fp64, counts)"""
    x = np.asarray(feats, np.float64)
    off, idx = point_lists_reference(sop, n_active)
    cnt = np.diff(off).astype(np.float64)
    if n_active == 0:
        return np.zeros((0, x.shape[1])), np.zeros((0, x.shape[1])), cnt
    y = np.add.reduceat(x[idx], off[:-1], 0)
    ya = np.add.reduceat(np.abs(x[idx]), off[:-1], 0)
    mult = (1.0 / cnt if average else np.ones_like(cnt))[:, None]
    return y * mult, ya * mult, cnt


def input_backward_reference(d_out, sop, n_active, average):
    """fp64 [n, C]: every point receives mult * g[site]"""
    g = np.asarray(d_out, np.float64)
    cnt = np.bincount(np.asarray(sop, np.int64), minlength=n_active).astype(np.float64)
    mult = 1.0 / cnt[sop] if average else np.ones(len(sop))
    return g[sop] * mult[:, None]


def _cells(rng, count, size):
    """`count` distinct cells of the grid, in random order, int64 [count, 3]"""
    vol = int(size[0]) * int(size[1]) * int(size[2])
    assert count <= vol
    flat = rng.permutation(vol)[:count] if vol <= (1 << 22) else rng.choice(vol, count, replace=False)
    return np.stack([flat // (size[1] * size[2]), (flat // size[2]) % size[1], flat % size[2]], 1).astype(np.int64)


INPUT_CASES = (
    "empty-0", "one_voxel-1", "one_voxel-2", "one_voxel-513", "one_voxel-2049",
    "distinct-1", "distinct-2", "distinct-512", "distinct-513", "distinct-2047", "distinct-2048", "distinct-2049",
    "distinct-524289", "first_is_last-513", "pow2-2047", "straddle-2049", "straddle-524289", "interleaved-512",
    "border-513", "border4-513",
)
INPUT_BIG = ("distinct-524289", "straddle-524289")


@functools.lru_cache(maxsize=None)
def input_case(name):
    """-> (coords int64 [n, 3 | 4], size).  Every case but `first_is_last`, the borders and `one_voxel` of 513 / 2049
    points has power-of-two site counts."""
    kind, n = name.split("-")
    n = int(n)
    rng = np.random.RandomState(n % 977 + len(kind))
    size = (64, 32, 16)
    if kind == "empty":
        c = np.zeros((0, 3), np.int64)
    elif kind == "one_voxel":
        c = np.tile(np.array([[3, 2, 1]], np.int64), (n, 1))
    elif kind == "distinct":
        size = (64, 32, 16) if n <= 2049 else (128, 128, 64)
        c = _cells(rng, n, size)
    elif kind == "first_is_last":
        cells = _cells(rng, 101, size)
        c = cells[rng.randint(0, 100, n)]
        c[-1] = cells[100]                                  # a site seen for the first time at the last point
    elif kind == "pow2":
        counts = 2 ** np.arange(11)                         # sites of 1, 2, 4, ..., 1024 points: 2047 points, shuffled
        c = _cells(rng, 11, size)[rng.permutation(np.repeat(np.arange(11), counts))]
    elif kind == "straddle":
        # point 0 alone, then pairs (1, 2), (3, 4), ...; the last site holds the points n-4 .. n-1 and so lies on both
        # sides of index n - 1 = 2048 / 524288, the first element of the scan's last tile
        size = (64, 32, 16) if n <= 2049 else (128, 128, 64)
        sid = np.concatenate([[0], 1 + np.arange(n - 5) // 2, np.full(4, 1 + (n - 5) // 2)])
        assert len(sid) == n and (n - 5) % 2 == 0
        c = _cells(rng, int(sid.max()) + 1, size)[sid]
    elif kind == "interleaved":
        cells = _cells(rng, n // 4, size)                   # examples 0, 1, 0, 1, ... over the same cells, 2 points each
        i = np.arange(n)
        c = np.concatenate([cells[(i // 2) % (n // 4)], (i % 2)[:, None]], 1)
    else:
        assert kind in ("border", "border4")
        size = (32768, 5, 3)
        corners = np.array([[x, y, z] for x in (0, size[0] - 1) for y in (0, size[1] - 1) for z in (0, size[2] - 1)], np.int64)
        cells = np.concatenate([corners, _cells(rng, 30, size)])
        c = cells[rng.randint(0, len(cells), n)]
        c[:8] = corners
        if kind == "border4":
            c = np.concatenate([c, rng.randint(0, 3, (n, 1))], 1)
    c = np.ascontiguousarray(c, np.int64)
    c.setflags(write=False)
    return c, size


def integer_features(n, planes, seed=0):
    return np.random.RandomState(seed + planes).randint(-4, 5, (n, planes)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def rounding_case():
    """normal data, arbitrary counts: 2049 points over 300 cells of two examples"""
    rng = np.random.RandomState(17)
    cells = np.concatenate([_cells(rng, 300, (64, 32, 16)), rng.randint(0, 2, (300, 1))], 1)
    coords = np.ascontiguousarray(cells[rng.randint(0, 300, 2049)], np.int64)
    return coords, (64, 32, 16), rng.randn(2049, 9).astype(np.float32), rng.randn(300, 9).astype(np.float32)


BAD_POINTS = {                          # name -> (row that replaces point 100 of a valid 4-column cloud)
    "x_is_size": (64, 0, 0, 0), "y_is_size": (0, 32, 0, 0), "z_is_size": (0, 0, 16, 0), "negative": (3, -1, 2, 0),
    "aliases_zero": (65536, 0, 0, 0), "example_32768": (1, 1, 1, 32768), "example_negative": (1, 1, 1, -1),
    "beyond_int32": (1 << 32, 0, 0, 0),
}


# =================================================================================================== views
def sparse_to_dense_reference(feats, loc, size, batch):
    feats = np.asarray(feats, np.float32)
    out = np.zeros((batch, feats.shape[1]) + tuple(size), np.float32)
    out[loc[:, 3], :, loc[:, 0], loc[:, 1], loc[:, 2]] = feats
    return out


def dense_to_sparse_reference(d_out, loc):
    return np.ascontiguousarray(d_out[loc[:, 3], :, loc[:, 0], loc[:, 1], loc[:, 2]])


DENSE_SIZES = ((5, 7, 3), (32, 16, 8))
DENSE_BATCHES = ("b1", "b2", "b3_empty_middle", "b4_trailing")       # name -> (examples present, batch handed over)


@functools.lru_cache(maxsize=None)
def dense_case(size, which, full):
    """-> (coords int64 [n, 4], batch).  Every example present holds the eight corners; `full`: every cell."""
    present, batch = {"b1": ((0,), 1), "b2": ((0, 1), 2), "b3_empty_middle": ((0, 2), 3), "b4_trailing": ((0, 1), 4)}[which]
    rng = np.random.RandomState(sum(size) + len(which))
    corners = np.array([[x, y, z] for x in (0, size[0] - 1) for y in (0, size[1] - 1) for z in (0, size[2] - 1)], np.int64)
    rows = []
    for b in present:
        vol = size[0] * size[1] * size[2]
        cells = _cells(rng, vol if full else max(9, vol // 3), size)
        cells = np.unique(np.concatenate([corners, cells]), axis=0)
        cells = cells[rng.permutation(len(cells))]
        rows.append(np.concatenate([cells, np.full((len(cells), 1), b)], 1))
    c = np.concatenate(rows)
    c = np.ascontiguousarray(c[rng.permutation(len(c))], np.int64)
    c.setflags(write=False)
    return c, batch


def anchors_reference(loc, base, stride, voxel_scale):
    """fp32, the kernel's operation order: p / vs * s + b, and 0 + b for the last four columns -> [n * A, 7]"""
    base = np.asarray(base, np.float32).reshape(-1, 7)
    p = np.asarray(loc)[:, :3].astype(np.float32)
    cent = p / np.float32(voxel_scale) * np.asarray(stride, np.float32)[None, :]
    out = np.empty((p.shape[0], base.shape[0], 7), np.float32)
    out[:, :, :3] = cent[:, None, :] + base[None, :, :3]
    out[:, :, 3:] = np.float32(0) + base[None, :, 3:]
    return out.reshape(-1, 7)


def anchor_base(A, seed):
    rng = np.random.RandomState(seed)
    base = rng.randn(A, 7).astype(np.float32)
    base[0, 0] = base[0, 6] = np.float32(-0.0)             # x + -0 keeps x; 0 + -0 is +0
    base[-1, 2] = np.float32(0.0)
    return base


ANCHOR_SIZES = ((64, 32, 16), (32, 16, 8), (16, 8, 4), (8, 4, 2), (4, 2, 1), (2, 1, 1))     # six maps of one pyramid
ANCHOR_STEPS = (((2, 2, 2), (2, 2, 2)),) * 4 + (((2, 2, 1), (2, 2, 1)),)                    # (filter, stride) between them
ANCHOR_STRIDES = ((8, 8, 4), (16, 16, 8), (32, 32, 16), (64, 64, 32), (128, 128, 64), (256, 256, 64))
ANCHOR_POINTS = 301


@functools.lru_cache(maxsize=None)
def anchor_scene():
    c = _cells(np.random.RandomState(23), ANCHOR_POINTS, ANCHOR_SIZES[0])
    c.setflags(write=False)
    return c


# =================================================================================================== row helpers
def bf16_rne_bits(x):
    """fp32 -> the bf16 bit patterns (uint16) by integer round-to-nearest-even on the fp32 pattern; a NaN stays a NaN
    (quiet bit set: the payload's top bits may all lie in the half that is cut)"""
    u = bits(x).astype(np.uint64)
    rounded = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), rounded)


def rows_to_bf16_reference(x, width):
    out = np.zeros((x.shape[0], width), np.uint16)
    out[:, :x.shape[1]] = bf16_rne_bits(x)
    return out


def bf16_equal(got, want):
    """uint16 patterns equal, except that a NaN only has to be a NaN (sign and payload are the converter's)"""
    got, want = np.asarray(got, np.uint16), np.asarray(want, np.uint16)
    nan = (want & 0x7FFF) > 0x7F80
    return got.shape == want.shape and np.array_equal((got & 0x7FFF) > 0x7F80, nan) and np.array_equal(got[~nan], want[~nan])


BF16_EDGES = np.array([
    0x3F808000, 0x3F818000,            # ties: to even downwards (1.0 + half an ulp), to even upwards
    0x3F808001, 0x3F807FFF,            # just above / below a tie
    0x7F7FFFFF, 0x7F7F8000, 0xFF7F8000, 0x7F7F7FFF,      # the largest finite fp32 and the tie round to +-Inf; below stays finite
    0x00000001, 0x00008000, 0x00018000, 0x807FFFFF,      # subnormals: to +0, a tie to zero, a tie upwards, the largest
    0x7F800000, 0xFF800000, 0x80000000, 0x00000000,
    0x7FC00000, 0x7F800001, 0xFFFFFFFF, SNAN_BITS,       # NaNs, one whose payload lies wholly in the low half
], np.uint32)
BF16_SHAPES = ((1, 8), (9, 16), (20, 32), (32, 32), (32, 64))
BF16_ROWS = (0, 1, 31, 33, 257)


def bf16_case(rows, cin, seed=0):
    rng = np.random.RandomState(seed + rows + cin)
    x = (rng.randn(rows, cin) * 3).astype(np.float32)
    flat = x.reshape(-1).view(np.uint32)
    flat[:len(BF16_EDGES)] = BF16_EDGES[:len(flat)]
    return x


ADD_N = (0, 1, 3, 4, 5, 1023, 1024, 1025, 4 * 256 * 3 - 1, 4 * 256 * 3, 4 * 256 * 3 + 1)


def add_case(n, seed=0):
    rng = np.random.RandomState(seed + n)
    a, b = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    sp = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], np.float32)
    for j in range(min(n, 25)):                              # every pair of specials (Inf - Inf, -0 + 0, -0 + -0, ...) in
        a[j], b[j] = sp[(j + 3) % 5], sp[4 - j // 5]          # front: the scalar tail of n > 25 holds ordinary values
    return a, b


def add_equal(got, a, b):
    """the fp32 sum bit for bit, except that a NaN only has to be a NaN"""
    with np.errstate(invalid="ignore"):
        want = a + b
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])
