"""The training augmentation (detection_3d_amd/csrc/augment.hip) restated in numpy, and the designed cases its tests run
on.  Extends tests/augment_ref.py (the fp64 operations in the kernel's order) by what the designed cases need: a minimum
that ignores a NaN and orders -0.0 below +0.0 (the kernel reduces with fmin and finishes on f64_ordered keys), the offset
with the kernel's two clips, exact integer / rational results and the rounding bounds.  numpy only: no GPU, no library.
tests/test_augment_forms_cpu.py asserts that every case sits where its name says and holds the oracle against scipy,
tests/test_augment_forms_gpu.py runs the kernels on the cases."""
import functools
import itertools
import types
from fractions import Fraction

import numpy as np

from tests import augment_ref as ref
from tests import front_forms as F

U53 = 2.0 ** -53                       # unit roundoff of fp64
U24 = 2.0 ** -24
REDUCE_FULL = 1024 * 256               # reduce_blocks: 1024 workgroups of 256 threads; one more row is a grid-stride trip


def gamma53(k):
    return k * U53 / (1.0 - k * U53)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def frac(v):
    return Fraction(float(v))


# =================================================================================================== parameters
def prm(m, nrm=None, color=None, u1=None, u2=None, origin_offset=0, color_col=-1, normal_col=-1):
    """one scene's d3d_augment_params as plain numpy"""
    z = np.zeros(3)
    return types.SimpleNamespace(m=np.asarray(m, np.float64), nrm=np.eye(3) if nrm is None else np.asarray(nrm, np.float64),
                                 color=z if color is None else np.asarray(color, np.float64),
                                 u1=z if u1 is None else np.asarray(u1, np.float64),
                                 u2=z if u2 is None else np.asarray(u2, np.float64),
                                 origin_offset=int(origin_offset), color_col=int(color_col), normal_col=int(normal_col))


_QUARTER = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))


def rotation_z(c, s):
    return np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])


def matrices(flip, cs, scale):
    """-> (M = diag(flip scale, scale, scale) Rz, F Rz), the products of detection_3d_amd.augment.linear_part /
    normal_matrix (held against them on the CPU)"""
    rz = rotation_z(*cs)
    d = np.ones(3)
    d[0] *= flip
    return (d * float(scale))[:, None] * rz, d[:, None] * rz


QUARTER_FLIP = tuple((flip, k) for flip in (1.0, -1.0) for k in range(4))          # the eight exact matrices


def quarter_matrices(flip, k, scale):
    return matrices(flip, _QUARTER[k], scale)


FREE = (1.0, 0.7321, 1.0731 * 50)      # flip, theta, scale of the rounding cases (no flip: with one, M is symmetric
#                                        and a transposed matrix would not show)


def free_matrices():
    flip, theta, scale = FREE
    return matrices(flip, (np.cos(theta), np.sin(theta)), scale)


# =================================================================================================== references
def min_ordered(a):
    """per-axis minimum that ignores a NaN and takes -0.0 below +0.0 (fmin, then atomicMin on f64_ordered keys)"""
    a = np.asarray(a, np.float64)
    lo = np.fmin.reduce(a, 0)
    neg_zero = ((a == 0) & np.signbit(a)).any(0)
    return np.where(lo == 0, np.where(neg_zero, -0.0, 0.0), lo)


def max_ordered(a):
    a = np.asarray(a, np.float64)
    hi = np.fmax.reduce(a, 0)
    pos_zero = ((a == 0) & ~np.signbit(a)).any(0)
    return np.where(hi == 0, np.where(pos_zero, 0.0, -0.0), hi)


def minmax_finite(a):
    """the six doubles of d3d_augment_transform / d3d_elastic_apply: over the finite values only"""
    a = np.where(np.isfinite(a), a, np.nan)
    return np.concatenate([min_ordered(a), max_ordered(a)])


def offset_reference(lo, hi, full, p):
    """k_aug_offset, operation by operation"""
    off = -lo
    if p.origin_offset:
        q = (np.asarray(full, np.float64) - hi) + lo
        up, dn = np.fmax(q - 0.001, 0.0), np.fmin(q + 0.001, 0.0)
        off = off + (up * p.u1 + dn * p.u2)
    return off


def voxelize_reference(pcl, p, scale, full, points=None):
    """d3d_augment_voxelize -> (coords int64 [M, 3], feats fp32 [M, F], offset [3], keep bool [N])"""
    pcl = np.ascontiguousarray(pcl, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        a = ref.affine(pcl, p.m) if points is None else np.asarray(points, np.float64)
        off = offset_reference(min_ordered(a), max_ordered(a), full, p)
        b = a + off
        keep = np.all((b >= 0) & (b < np.asarray(full, np.float64)), 1)
        bk = b[keep]
        feats = pcl[keep].copy()
        feats[:, 0:3] = (bk / np.float64(scale)).astype(np.float32)
        if p.color_col >= 0:
            c = p.color_col
            feats[:, c:c + 3] = (pcl[keep, c:c + 3].astype(np.float64) + p.color).astype(np.float32)
        if p.normal_col >= 0:
            c = p.normal_col
            feats[:, c:c + 3] = ref.affine(pcl[keep, c:c + 3], p.nrm).astype(np.float32)
    return np.trunc(bk).astype(np.int64), feats, off, keep


def affine_exact(xyz, m, rows):
    """Fraction: (exact a [rows, 3], sum_k |x_k m_kj| [rows, 3])"""
    out, mag = [], []
    for i in rows:
        x = [frac(v) for v in xyz[i, :3]]
        out.append([sum(x[k] * frac(m[k, j]) for k in range(3)) for j in range(3)])
        mag.append([sum(abs(x[k] * frac(m[k, j])) for k in range(3)) for j in range(3)])
    return out, mag


def contraction_sensitive(xyz, m, rows):
    """bool [rows, 3, 2]: where ((x m0 + y m1) + z m2) with ONE fused multiply-add gives other bits than the three
    rounded products and two rounded sums -- [.., 0]: fma(y, m1, x m0), [.., 1]: fma(x, m0, y m1).  (z m2 is 0 in the
    columns x and y and the only term of column z: Rz leaves z alone, so the outer sum has nothing to fuse.)  Evaluated in
    rationals; float(Fraction) rounds once, to nearest even.  Also returns the plain bits."""
    out = np.zeros((len(rows), 3, 2), bool)
    plain = np.zeros((len(rows), 3))
    for r, i in enumerate(rows):
        x, y, z = (frac(v) for v in xyz[i, :3])
        for j in range(3):
            m0, m1, m2 = (frac(m[k, j]) for k in range(3))
            p0, p1, p2 = float(x * m0), float(y * m1), float(z * m2)
            s = float(frac(p0) + frac(p1))
            plain[r, j] = float(frac(s) + frac(p2))
            inner = float(frac(float(frac(p0) + y * m1)) + frac(p2))
            first = float(frac(float(x * m0 + frac(p1))) + frac(p2))
            out[r, j] = (inner != plain[r, j], first != plain[r, j])
    return out, plain


# =================================================================================================== 1 transform
TRANSFORM_CASES = ((1, 3), (255, 4), (256, 9), (257, 12), (262144, 3), (262145, 4), (262145, 12))


@functools.lru_cache(maxsize=None)
def cloud(n, nfeat, seed=0):
    """normal data, fp32 [n, nfeat]; read-only"""
    pcl = (np.random.RandomState(seed + n % 9973 + nfeat).randn(n, nfeat) * 3).astype(np.float32)
    pcl.setflags(write=False)
    return pcl


# =================================================================================================== 2 exact affine
EXACT_N = 300
EXACT_MATRICES = tuple((flip, k, 64.0) for flip, k in QUARTER_FLIP) + ((1.0, 1, 32.0),)


@functools.lru_cache(maxsize=None)
def exact_cloud():
    """nine columns (xyz, three pass-through, a normal) on multiples of 1 / 64, |.| < 8 -> (pcl, the integers 64 pcl):
    every product, sum and difference from the minimum is exact"""
    rng = np.random.RandomState(41)
    ints = rng.randint(-511, 512, (EXACT_N, 9))
    pcl = (ints / 64.0).astype(np.float32)
    pcl.setflags(write=False)
    return pcl, ints


def exact_affine(ints, m):
    """integers: (ints / 64) . m with m's entries 0, +-32, +-64 -> exact doubles"""
    mi = np.round(m * 2).astype(np.int64)                    # m in halves
    assert np.array_equal(mi / 2.0, m)
    return (ints.astype(np.int64) @ mi) / 128.0


# =================================================================================================== 5 filter edges
EDGE_FULL = (100, 50, 200)
EDGE_REST = 12.5                        # the other axes of an edge row
EDGE_TINY = (3 * 2.0 ** -48, 3 * 2.0 ** -49, 3 * 2.0 ** -47)          # 3/4 of the ulp below full: full - that rounds to the
#                                                                       largest double below full (100, 50, 200)
EDGE_ZERO = (0.0, 0.0, 0.0)
EDGE_STEP = 2.0 ** -11                  # the cloud's lattice in voxel units at scale 64: x on multiples of 2^-17


def edge_rows(minimum):
    """the transformed positions a [19, 3] of one edge call, and per row (axis, what, kept).  `minimum`: EDGE_ZERO --
    then b = a -- or EDGE_TINY -- then b = a - tiny, so that a == full lands on the largest double below full."""
    tiny = minimum != EDGE_ZERO
    a, rows = [tuple(minimum)], [(-1, "minimum", True)]
    for d in range(3):
        f = float(EDGE_FULL[d])
        for what, v, kept in (("at_minimum", minimum[d], True), ("full", f, tiny), ("full_below", f - EDGE_STEP, True),
                              ("full_above", f + EDGE_STEP, False), ("inside", 25.0, True), ("far", 4 * f, False)):
            p = [EDGE_REST] * 3
            p[d] = v
            a.append(tuple(p))
            rows.append((d, what, kept))
    return np.array(a, np.float64), rows


def edge_case(flip, k, minimum):
    """the cloud that the quarter / flip matrix at scale 64 maps onto edge_rows(minimum) -> (pcl [19, 4], prm, rows, a);
    column 3 is the row index"""
    m, nrm = quarter_matrices(flip, k, 64.0)
    a, rows = edge_rows(minimum)
    x = a @ (m.T / 4096.0)                                   # M^-1 = M^T / 64^2: a permutation with signs, exact
    pcl = np.concatenate([x, np.arange(len(a))[:, None]], 1).astype(np.float32)
    return pcl, prm(m, nrm), rows, a


BELOW_LO = (-30.25, -20.5, -60.0)       # the lowest and highest transformed rows of the downward-clip edge call: extent
BELOW_HI = (80.75, 40.5, 151.0)         # full + 11 on every axis, so q = -11 and dn = -11 + 0.001
BELOW_EDGE = (-25.25, -15.5, -55.0)     # the row on the lower edge: 5 voxels above the lowest row
BELOW_KINDS = ("at_zero", "ulp_below_zero")


def _offset_axis(lo, hi, full, u1, u2):
    """k_aug_offset on one axis with origin_offset set"""
    q = (float(full) - hi) + lo
    up, dn = max(q - 0.001, 0.0), min(q + 0.001, 0.0)
    return -lo + (up * u1 + dn * u2)


def draw_for_offset(lo, hi, full, target, tries=400):
    """the draw u2 (u1 = 0) at which the downward clip gives the offset `target` to the bit: dn u2 is spaced more finely
    than the offset, so a neighbour of target / dn does it; asserts when none of `tries` neighbours does"""
    dn = min(((float(full) - hi) + lo) + 0.001, 0.0)
    assert dn < 0
    u2 = (target + lo) / dn
    down = up = u2
    for _ in range(tries):
        for cand in (down, up):
            if _offset_axis(lo, hi, full, 0.0, cand) == target:
                return float(cand)
        down, up = np.nextafter(down, -np.inf), np.nextafter(up, np.inf)
    raise AssertionError(f"no draw gives the offset {target!r}")


def below_edge_rows(kind):
    """the transformed positions a [11, 3] of the downward-clip edge call, per row (axis, what, kept), and the offset the
    draws are made for: -edge ("at_zero": the edge row has b == 0, kept) or the double below it ("ulp_below_zero": the
    edge row has b == -ulp(offset), dropped); the rows 2^-11 above and below the edge row in both"""
    edge = np.array(BELOW_EDGE)
    target = -edge if kind == "at_zero" else np.nextafter(-edge, 0.0)
    a, rows = [BELOW_LO, BELOW_HI], [(-1, "lowest", False), (-1, "highest", False)]
    for d in range(3):
        for what, v, kept in (("edge", edge[d], kind == "at_zero"), ("above", edge[d] + EDGE_STEP, True),
                              ("below", edge[d] - EDGE_STEP, False)):
            p = list(edge + EDGE_REST)
            p[d] = v
            a.append(tuple(p))
            rows.append((d, what, kept))
    return np.array(a, np.float64), rows, target


def below_edge_case(flip, k, kind):
    """the cloud that the quarter / flip matrix at scale 64 maps onto below_edge_rows(kind), with the draws u2 that put
    the offset where the kind says -> (pcl [11, 4], prm, rows, a, target offset)"""
    m, nrm = quarter_matrices(flip, k, 64.0)
    a, rows, target = below_edge_rows(kind)
    u2 = [draw_for_offset(BELOW_LO[d], BELOW_HI[d], EDGE_FULL[d], target[d]) for d in range(3)]
    pcl = np.concatenate([a @ (m.T / 4096.0), np.arange(len(a))[:, None]], 1).astype(np.float32)
    return pcl, prm(m, nrm, u2=u2, origin_offset=1), rows, a, target


def ulp_edge_case():
    """fp64 points (the elastic form of d3d_augment_voxelize) around an offset that is a rounded product: per axis a row
    at b == 0, one ulp of the offset below 0, at b == full and at the largest double below full, the extent pinned by a
    lowest and a highest row.  Every axis is in the downward-clip regime (extent above full), so the lowest row is below
    0.  -> (pcl [14, 4], points [14, 3], prm, full, rows)"""
    full = (100, 50, 200)
    lo = np.array([-30.25, -25.5, -60.0])             # off > 0: a row at b ~ full has |a| < full, a grid no coarser
    hi = lo + np.array(full) + np.array([11.0, 7.0, 23.0])
    u1, u2 = [0.3, 0.6, 0.1], [0.73, 0.31, 0.52]

    def reaches_below_full(d, draw):
        """no sum near full is a rounding tie: some double a has a + off == the largest double below full"""
        off = _offset_axis(lo[d], hi[d], full[d], u1[d], draw)
        near = {float(full[d]) - off}
        for _ in range(2):
            near |= {float(np.nextafter(v, s)) for v in near for s in (-np.inf, np.inf)}
        return np.nextafter(float(full[d]), 0.0) in {v + off for v in near}

    for d in range(3):                                       # the axes are independent: one draw each
        draws = [u2[d] + 0.01 * t for t in range(20)]
        u2[d] = next(v for v in draws if reaches_below_full(d, v))          # (StopIteration: no draw in 20)
    p = prm(np.eye(3) * 64, u1=u1, u2=u2, origin_offset=1)
    off = offset_reference(lo, hi, full, p)
    pts, rows = [lo, hi], [(-1, "lowest", False), (-1, "highest", False)]
    inside = -off + 20.0                                     # the other axes of an edge row: b about 20, kept
    for d in range(3):
        f = float(full[d])
        at_full = f - off[d]
        while at_full + off[d] < f:
            at_full = np.nextafter(at_full, np.inf)
        while np.nextafter(at_full, -np.inf) + off[d] >= f:
            at_full = np.nextafter(at_full, -np.inf)          # the lowest a with a + off >= full
        for what, v, kept in (("zero", -off[d], True), ("ulp_below_zero", np.nextafter(-off[d], -np.inf), False),
                              ("full", at_full, False), ("full_below", np.nextafter(at_full, -np.inf), True)):
            q = inside.copy()
            q[d] = v
            pts.append(q)
            rows.append((d, what, kept))
    pts = np.array(pts, np.float64)
    pcl = np.concatenate([np.zeros((len(pts), 3)), np.arange(len(pts))[:, None]], 1).astype(np.float32)
    return pcl, pts, p, full, rows


KEEP_PATTERNS = ("all-2047", "alternate-2048", "last_only-2049", "minimum_only-2049", "all-524289", "alternate-524289",
                 "minimum_only-524289")
PATTERN_FULL = (64, 64, 64)
PATTERN_MATRIX = (-1.0, 1, 64.0)        # flip and a quarter turn


def pattern_keep(name):
    kind, n = name.split("-")
    n = int(n)
    i = np.arange(n)
    return {"all": np.ones(n, bool), "alternate": i % 2 == 0, "last_only": i == n - 1, "minimum_only": i == n // 2}[kind]


@functools.lru_cache(maxsize=None)
def pattern_case(name):
    """kept rows on the 2^-11 lattice of [0, 60)^3 voxels after the map, the first kept row the minimum (0, 0, 0), a
    dropped row 500 voxels further on the transformed x -> (pcl [n, 4], prm); column 3 is the row index (exact)"""
    keep = pattern_keep(name)
    n = keep.size
    rng = np.random.RandomState(n % 1000 + len(name))
    a = rng.randint(0, 60 * 2048, (n, 3)) / 2048.0
    a[~keep, 0] += 500.0
    a[np.argmax(keep)] = 0.0
    m, nrm = quarter_matrices(*PATTERN_MATRIX)
    pcl = np.concatenate([a @ (m.T / 4096.0), np.arange(n)[:, None]], 1).astype(np.float32)
    pcl.setflags(write=False)
    return pcl, prm(m, nrm)


# =================================================================================================== 6 offset
OFFSET_FULL = (64, 64, 64)
OFFSET_DRAWS = {"dyadic": ((0.5, 0.25, 0.75), (0.25, 0.5, 0.125)),
                "random": ((0.3141592653589793, 0.6180339887498949, 0.1234567890123456),
                           (0.9182736455463728, 0.2718281828459045, 0.5772156649015329)),
                "no_draw": ((0.5, 0.25, 0.75), (0.25, 0.5, 0.125))}              # origin_offset = 0: the draws are unused
OFFSET_N = 600


@functools.lru_cache(maxsize=None)
def offset_case(kind):
    """fp64 points whose extent is 40 on x (upward clip), 100 on y (downward clip: rows past full go) and 64 + 2^-11 on z
    (|q| < 0.001: both clips 0) -> (pcl [n, 4], points, prm, full)"""
    rng = np.random.RandomState(7)
    ext = np.array([40.0, 100.0, 64.0 + 2.0 ** -11])
    lo = np.array([-17.25, 3.5, 0.0])
    pts = lo + rng.rand(OFFSET_N, 3) * ext
    pts[0], pts[1] = lo, lo + ext
    pcl = np.concatenate([np.zeros((OFFSET_N, 3)), np.arange(OFFSET_N)[:, None]], 1).astype(np.float32)
    u1, u2 = OFFSET_DRAWS[kind]
    return pcl, pts, prm(np.eye(3) * 64, u1=u1, u2=u2, origin_offset=int(kind != "no_draw")), OFFSET_FULL


def offset_q_case():
    """q - 0.001 == 0 exactly on every axis: the highest row at full and the lowest at the double 0.001, so that
    q = (full - full) + 0.001 -> (pcl, points, prm, full)"""
    pts = np.array([[0.001, 0.001, 0.001], [64.0, 64.0, 64.0], [10.0, 20.0, 30.0], [63.5, 0.5, 1.0]])
    pcl = np.concatenate([np.zeros((4, 3)), np.arange(4)[:, None]], 1).astype(np.float32)
    return pcl, pts, prm(np.eye(3) * 64, u1=(0.5, 0.3, 0.9), u2=(0.25, 0.7, 0.1), origin_offset=1), OFFSET_FULL


# =================================================================================================== 7 signed zeros
def signed_zero_case(order):
    """a flipped cloud (the exact matrix flip, no turn, scale 64) whose transformed x is >= 0 with rows at -0.0 AND at
    +0.0 at the minimum; `order`: 0 as built, 1 reversed -> (pcl [n, 4], prm)"""
    rng = np.random.RandomState(3)
    n = 700
    xyz = rng.randint(0, 512, (n, 3)) / 64.0
    xyz[:, 0] = -xyz[:, 0] - 1.0 / 64                        # a_x = -64 x > 0
    xyz[:, 1:] -= 4.0                                        # y and z of both signs: the zero products' signs vary
    for r in range(5, n, 50):                                # rows on the plane x = 0, both signs of the input zero
        xyz[r, 0] = 0.0 if (r // 50) % 2 else -0.0
    m, nrm = quarter_matrices(-1.0, 0, 64.0)
    pcl = np.concatenate([xyz, np.arange(n)[:, None]], 1).astype(np.float32)
    if order:
        pcl = pcl[::-1].copy()
    return pcl, prm(m, nrm)


# =================================================================================================== 8 columns
LAYOUTS = {                             # name -> (nfeat, colour column, normal column)
    "colour3_normal6": (9, 3, 6), "normal3_colour6": (9, 6, 3), "colour_only": (6, 3, -1), "normal_only": (6, -1, 3),
    "neither": (5, -1, -1), "trailing": (12, 3, 6), "passthrough_between": (10, 4, 7),
}
LAYOUT_N = 515
LAYOUT_COLOR = (0.013, -0.021, 0.004)
BAD_COLUMNS = {                         # name -> (nfeat, colour column, normal column): each a D3D_REQUIRE refusal
    "nfeat_below_3": (2, -1, -1), "colour_in_xyz": (9, 2, -1), "colour_past_end": (9, 7, -1), "normal_in_xyz": (9, -1, 1),
    "normal_past_end": (8, 3, 6),
}


@functools.lru_cache(maxsize=None)
def layout_case(name):
    """free rotation, a colour draw, normal data in the colour and normal columns, SPECIAL_BITS of front_forms in the
    pass-through columns only (a NaN through arithmetic has no pinned payload) -> (pcl, prm, pass-through columns)"""
    nfeat, cc, nc = LAYOUTS[name]
    rng = np.random.RandomState(nfeat + 3 * cc + 7 * nc + 50)
    pcl = rng.randn(LAYOUT_N, nfeat).astype(np.float32)
    used = set(range(3)) | (set(range(cc, cc + 3)) if cc >= 0 else set()) | (set(range(nc, nc + 3)) if nc >= 0 else set())
    free = [c for c in range(nfeat) if c not in used]
    for j, r in enumerate(range(0, LAYOUT_N, 7)):
        if free:
            pcl.view(np.uint32)[r, free[j % len(free)]] = F.SPECIAL_BITS[j % len(F.SPECIAL_BITS)]
    pcl.setflags(write=False)
    m, nrm = free_matrices()
    return pcl, prm(m, nrm, color=LAYOUT_COLOR, color_col=cc, normal_col=nc), free


# =================================================================================================== 9 blur
BLUR_GRIDS = ((3, 3, 3), (1, 2, 5), (5, 1, 2), (2, 5, 1), (7, 4, 3), (9, 8, 7), (8, 8, 4))     # (8, 8, 4): 256 cells
BLUR_NF = (1, 3)


@functools.lru_cache(maxsize=None)
def blur_case(dims, nf):
    raw = np.random.RandomState(sum(dims) + 10 * nf).randn(nf, *dims).astype(np.float32)
    raw.setflags(write=False)
    return raw


def blur_passes(f, count):
    """the first `count` passes of ref.blur (axes 0, 1, 2, 0, 1, 2) of one field"""
    for axis in (0, 1, 2, 0, 1, 2)[:count]:
        f = ref.blur_axis(f, axis)
    return f


IMPULSE_DIMS = (9, 8, 7)
IMPULSES = {"corner": (0, 0, 0), "far_corner": (8, 7, 6), "centre": (4, 4, 3)}


def impulse_case(where):
    f = np.zeros((1,) + IMPULSE_DIMS, np.float32)
    f[(0,) + IMPULSES[where]] = 1.0
    return f


def impulse_support(where):
    """bool [9, 8, 7]: within 2 cells of the impulse on every axis (two 3-tap passes per axis)"""
    idx = np.indices(IMPULSE_DIMS)
    return np.all([np.abs(idx[d] - IMPULSES[where][d]) <= 2 for d in range(3)], 0)


def blur_pass_exact(x, axis, cells):
    """Fraction: one pass of the filter at `cells` (index tuples of the 4-d array) -> (exact, sum |x_k| w)"""
    w = frac(ref.BLUR_W)
    out = []
    for c in cells:
        s = a = Fraction(0)
        for q in (-1, 0, 1):
            r = list(c)
            r[1 + axis] += q
            if 0 <= r[1 + axis] < x.shape[1 + axis]:
                s += frac(x[tuple(r)]) * w
                a += abs(frac(x[tuple(r)])) * w
        out.append((s, a))
    return out


# =================================================================================================== bounds
def blur_bound(exact, mag):
    """one pass: three products and at most two rounding additions per term in fp64 (gamma_3 of u = 2^-53 on
    sum|x_k| w), then one rounding to fp32"""
    g3 = frac(gamma53(3))
    return g3 * mag + frac(U24) * (abs(exact) + g3 * mag)


def sample_bound(corner_mag, value, a, mag):
    """|b - exact| of b = a + disp * mag.  Each of the three weight factors t or 1 - t carries at most 4 roundings of
    absolute size u (a - g_l, g_h - g_l, the quotient, 1 - t; every factor is at most 1), their two products 2 more: 14;
    the product with F one, at most 7 of the 8 additions round (the first adds to 0): 22 roundings on terms of at most
    |F| each -> gamma_22 sum|F| on disp (gamma_24 covers the second-order terms); the product with mag and the final sum
    one rounding each."""
    u = frac(U53)
    m = abs(frac(mag))
    return m * frac(gamma53(24)) * corner_mag * (1 + 2 * u) + 2 * u * (abs(value) * m + abs(frac(a)))


# =================================================================================================== 10 sampling
APPLY_GRIDS = ((2, 2, 2), (5, 4, 3))
APPLY_STEPS = ((6.0, 40.0), (20.0, 160.0), (6.0, 40.0 * 48 / 50))     # (gran, mag); the last magnitude is no integer


@functools.lru_cache(maxsize=None)
def quarter_fields(dims):
    """three distinct fields of quarter-integers in [-2, 2]"""
    f = np.random.RandomState(sum(dims)).randint(-8, 9, (3,) + tuple(dims)) / 4.0
    f = f.astype(np.float32)
    f.setflags(write=False)
    return f


def lattice_axis(d, gran):
    """the nodes of one axis and the quarter points of every cell: 4 (d - 1) + 1 positions, all exact"""
    return -(d - 1) * gran + np.arange(4 * (d - 1) + 1) * (gran / 2.0)


def lattice_points(dims, gran):
    """every combination of the per-axis positions: nodes, faces, cell fractions 0, 1/4, 1/2, 3/4 -- (5, 4, 3): 1989"""
    ax = [lattice_axis(d, gran) for d in dims]
    return np.array(list(itertools.product(*ax)), np.float64)


def lattice_displaced(dims, gran, mag, fields, pts):
    """the exact trilinear value by cell index and fraction in integers (quarters), times mag in one rounding, added in
    one -- no searchsorted, no weights' order: an independent route to the same bits"""
    q = np.stack([np.round((pts[:, d] + (dims[d] - 1) * gran) / (gran / 2.0)).astype(np.int64) for d in range(3)], 1)
    cell = np.minimum(q // 4, np.array(dims) - 2)
    t = (q - 4 * cell) / 4.0                                 # 0, 1/4, 1/2, 3/4, 1
    disp = np.zeros((pts.shape[0], 3))
    for corner in itertools.product((0, 1), repeat=3):
        w = np.prod([t[:, d] if c else 1.0 - t[:, d] for d, c in enumerate(corner)], 0)
        ii = tuple(cell[:, d] + c for d, c in enumerate(corner))
        for f in range(3):
            disp[:, f] += fields[f][ii].astype(np.float64) * w
    return pts + disp * mag, disp


def outside_points(dims, gran):
    """the lattice points of each of the six faces moved one ulp outwards on that face's axis"""
    pts = lattice_points(dims, gran)
    out = []
    for d in range(3):
        g1 = (dims[d] - 1) * gran
        for side in (-1.0, 1.0):
            face = pts[pts[:, d] == side * g1].copy()
            face[:, d] = np.nextafter(face[:, d], side * np.inf)
            out.append(face)
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def random_points(n, dims, gran, seed=0):
    """uniform points over 1.15 times the grid's extent (about a third outside); when n > 1 the middle row is a NaN row
    and the last row lies inside (the row that a launch without its grid-stride trip leaves undisplaced)"""
    rng = np.random.RandomState(seed + n % 977)
    g1 = (np.array(dims) - 1) * gran
    pts = (rng.rand(n, 3) * 2 - 1) * g1 * 1.15
    if n > 1:
        pts[n // 2] = (np.nan, 1.0, 2.0)
        pts[n - 1] = g1 * (0.31, -0.47, 0.12)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def random_fields(dims):
    raw = np.random.RandomState(sum(dims) + 99).randn(3, *dims).astype(np.float32)
    f = np.stack([ref.blur(x) for x in raw])
    f.setflags(write=False)
    return f


def elastic_reference(pts, fields, gran, mag):
    """ref.elastic_pass with a NaN row left as it is (numpy's searchsorted sorts a NaN past the end)"""
    ok = ~np.isnan(pts).any(1)
    out = np.array(pts, np.float64)
    out[ok] = ref.elastic_pass(out[ok], fields, gran, mag)
    return out


def sample_exact(pts, fields, gran, rows):
    """Fraction: the trilinear value of the three fields at pts[rows] (all inside) -> (value [rows][3], sum over the
    cell's corners of |F| [rows][3])"""
    dims = fields.shape[1:]
    out = []
    for i in rows:
        t, cell = [], []
        for d in range(3):
            g0, step = Fraction(-(dims[d] - 1)) * frac(gran), 2 * frac(gran)
            u = (frac(pts[i, d]) - g0) / step
            c = min(max(-(-u.numerator // u.denominator) - 1, 0), dims[d] - 2)           # ceil(u) - 1, clipped
            cell.append(c)
            t.append(u - c)
        val, mag = [Fraction(0)] * 3, [Fraction(0)] * 3
        for corner in itertools.product((0, 1), repeat=3):
            w = Fraction(1)
            for d, c in enumerate(corner):
                w *= t[d] if c else 1 - t[d]
            ii = tuple(cell[d] + c for d, c in enumerate(corner))
            for f in range(3):
                val[f] = val[f] + frac(fields[f][ii]) * w
                mag[f] = mag[f] + abs(frac(fields[f][ii]))
        out.append((val, mag))
    return out


# =================================================================================================== non-finite rows
NONFINITE = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}
NONFINITE_ROW = 150


@functools.lru_cache(maxsize=None)
def scene_cloud(n=300, seed=5):
    """a small scene in metres, nine columns (xyz, colour, normal); read-only"""
    rng = np.random.RandomState(seed)
    nrm = rng.randn(n, 3)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    pcl = np.concatenate([rng.rand(n, 3) * np.array([6.0, 5.0, 2.5]) + 0.25, rng.rand(n, 3), nrm], 1).astype(np.float32)
    pcl.setflags(write=False)
    return pcl


def nonfinite_cloud(kind, axis):
    pcl = np.array(scene_cloud())
    pcl[NONFINITE_ROW, axis] = NONFINITE[kind]
    return pcl
