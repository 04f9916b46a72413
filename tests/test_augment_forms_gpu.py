"""The training augmentation on exact cases: the six kernels and four C entries of detection_3d_amd/csrc/augment.hip
(d3d_augment_transform, d3d_augment_voxelize, d3d_elastic_blur, d3d_elastic_apply) through ctypes, and Augment.__call__
on top of them.

References: tests/augment_forms.py on top of tests/augment_ref.py (numpy fp64 in the kernel's operation order; held
against scipy bit for bit in tests/test_augment_forms_cpu.py, which also asserts that every designed case sits where its
name says).  Everything is compared bit for bit with no row excused: the affine map, offset, filter, trunc, features,
blur, trilinear sampling and the min / max words.  Where the data round, a few hundred elements are also held against
rationals (fractions.Fraction): |a - exact| <= gamma_3 sum|x_k m_kj| for the map, blur_bound and sample_bound of
augment_forms (derived there from the operation counts) for one blur pass and the sampling; gamma_k = k u / (1 - k u),
u = 2^-53.  Every output handed to a C entry is prefilled with a sentinel (NaN, -7 for integers, 7.5 for host doubles)
and followed by guard elements: an unwritten cell or a write past the end fails.

Forms and the tests that reach them:

=========================================================  ======================================================
form                                                       tests
=========================================================  ======================================================
d3d_augment_transform: k_aug_minmax writing fp64 points,   test_transform[n-nfeat] (n = 1, 255, 256, 257, 262144,
1 .. 1024 workgroups, the grid-stride trip from 262145     262145; nfeat = 3, 4, 9, 12): points and six doubles
row_times on exact data: eight flip x quarter matrices at  test_exact_affine[flip-k-scale]: integers, in the
scale 64, one at 32; the normal matrix F Rz                points, coordinates, xyz features and normals
row_times on rounding data, no contraction                 test_rounding_affine (bits, Fraction bound; the rows
                                                           one fused multiply-add would change: CPU module)
d3d_augment_voxelize, identity parameters = d3d_voxelize   test_identity_equals_voxelize[every voxelizer case of
                                                           front_forms: patterns, boundary, negative, non-dyadic
                                                           scales, NaN / +Inf / -Inf, n = 0]
k_aug_flag after each of the eight matrices: b == 0,       test_filter_edges[flip-k-zero / tiny] (no draw),
b == full, the largest double below full; under the        test_filter_edges_below_zero[flip-k-at_zero / ulp_
downward clip b == 0 and one ulp of the offset below 0     below_zero] (u2 made for the offset, to the bit)
the same four edges on fp64 points, a rounded offset       test_filter_edges_to_the_ulp
kept rows and ranks in row order; the scan's second round  test_keep_patterns[all / alternate / last_only /
                                                           minimum_only x 2047 .. 524289]
k_aug_offset: upward clip, downward clip, both 0 in one    test_offset_regimes[dyadic / random / no_draw],
call; q - 0.001 == 0; origin_offset = 0 with draws set     test_offset_margin_exactly_zero
-0.0 and +0.0 at the minimum, two row orders               test_signed_zeros_in_the_minimum
k_aug_write: colour and normal columns in either order,    test_column_layouts[7 layouts] (signalling NaNs,
alone, absent; pass-through columns before and after       denormals, -0.0 pass through bit for bit)
the D3D_REQUIRE refusals of nfeat and the column numbers   test_column_arguments_refused[5], nothing written
d3d_elastic_blur: totals below, at and above 256, thin     test_blur[grid-nf] (`fields` after six passes AND `tmp`
grids, nf = 1 and 3; zero padding                          after five), test_blur_impulse[corner / far / centre]
d3d_elastic_apply on exact lattices: nodes, faces, cell    test_apply_lattice[(2,2,2) / (5,4,3) x (gran, mag)]: a
quarters; one ulp outside each face; three distinct        route without searchsorted or weight order gives the
fields; gran 6 / 20, mag 40 / 160 / 38.4                   same bits; outside: the point's own bits
d3d_elastic_apply on random points, n = 1, 257, 262145;    test_apply_random_points[gran-mag-n] (bits, Fraction
a NaN row; min / max; minmax_host = null                   bound), test_apply_refuses_a_grid_below_2[3]
Augment.__call__, everything on                            test_whole_call_with_elastic (fields drawn again from
                                                           the seeded device generator; every row)
NaN / +Inf / -Inf rows, elastic on and off                 test_nonfinite_rows[kind-axis-elastic / plain],
                                                           _free_rotation[nan / +inf], test_nonfinite_extent
=========================================================  ======================================================

Not reached here: b == 0 and b one ulp below 0 under the SAME offset after a matrix (an fp32 cloud times 64 has no two
rows one ulp of the offset apart: two calls, each with draws made for its offset; the fp64-points form has both in
one); a -0.0 / +0.0 pair at the maximum (the maximum only enters the origin offset); a +Inf row together with
origin_offset (the maximum is +Inf, the offset is not finite and the cloud goes, elastic on or off: not the row-alone
contract); a +Inf input that a negative matrix entry turns into -Inf (the contract is on the transformed coordinate: it
drops the cloud); a cloud without one finite coordinate on an axis (extent 0 by elastic_displace); a merely huge finite
outlier, whose noise grid needs more memory than there is; blur grids of 2^31 cells and clouds of 2^31 / 3 points.

Cost: 152 tests, 3.8 s on an MI355X; the slowest (262145 points through numpy's oracle) 0.2 s.

Fixes these tests asked for: with elastic on, one +Inf or -Inf coordinate made elastic_displace size the noise grid from
|Inf| (int32 garbage, "negative dimension" from torch.randn).  d3d_augment_transform and d3d_elastic_apply now report
the extent of the finite coordinates only, elastic_displace counts an axis without a finite value as extent 0, and the
voxelizer's minimum is untouched.  With the fix taken out (the parent's augment.hip) these fail: test_nonfinite_rows
[+inf / -inf x axis 0, 1, 2 x elastic] (6), test_nonfinite_rows_free_rotation[+inf], test_nonfinite_extent; the NaN and
the plain cases pass either way (fmin and fmax ignore a NaN).  Nothing else in the kernels or the references had to
change: the device minimum is -0.0 in either row order, and every bit-for-bit comparison holds as the code stands.

Sensitivity: each mutation below was built into a scratch copy of the library and this file run against it (152 tests).
Every one fails; none can leave its buffers, for the reason in brackets.

=========================================================  ======================================================
mutation                                                   failing tests
=========================================================  ======================================================
row_times indexes m[3 j + k], a transposed matrix [the     39: test_transform (7), test_exact_affine (5: the odd
same nine doubles]                                         turns; k = 2 by the sign of a zero), test_rounding_
                                                           affine, test_filter_edges (6), _below_zero (4: the odd
                                                           turns without flip), test_keep_patterns (7), test_
                                                           signed_zeros, test_column_layouts (7), _free_rotation
                                                           [+inf]
k_aug_flag keeps b == full [a value that is written, not   10: test_filter_edges[.. zero] (8), test_filter_edges_
an index; kept <= n]                                       to_the_ulp, test_identity_equals_voxelize[boundary]
k_aug_offset swaps u1 and u2 [values]                      21: test_filter_edges_below_zero (16), test_offset_
                                                           regimes[dyadic / random], test_filter_edges_to_the_ulp,
                                                           test_rounding_affine, test_whole_call
k_aug_write adds the colour offset in fp32 [a value]       7: test_column_layouts (the 5 with colour), test_
                                                           rounding_affine, test_whole_call
k_elastic_blur clamps the index at the border [the         17: test_blur (14), test_blur_impulse[corner / far_
clamped index is inside the field]                         corner], test_whole_call
k_elastic_apply tests a < g1 for inside [less is read]     6: test_apply_lattice (all)
k_elastic_apply swaps D1 and D2 in idx, the index clamped  9: test_apply_lattice[5x4x3] (3), test_apply_random_
to the last cell [so that it stays inside]                 points[257 / 262145] (4), test_whole_call, test_
                                                           nonfinite_extent; the cubic (2, 2, 2) cannot notice
k_elastic_apply exchanges tt and 1 - tt [values]           12: test_apply_lattice (6), test_apply_random_points
                                                           [257 / 262145] (4), test_whole_call, _extent
k_aug_minmax and k_elastic_apply stop after one trip       6, cases beyond 262144 rows and only they: test_
[rows stay unvisited: sentinels, an undisplaced point,     transform[262145] (2), test_apply_random_points[262145]
a missed minimum]                                          (2), test_keep_patterns[minimum_only-524289], test_
                                                           identity_equals_voxelize[pattern-last_only-524289]
=========================================================  ======================================================"""
import ctypes

import numpy as np
import pytest
import torch

from tests import augment_forms as A
from tests import augment_ref as ref
from tests import front_forms as F

pytestmark = pytest.mark.gpu

GUARD = 16
INT_SENTINEL = -7
OFFSET_SENTINEL = 7.5


def _L():
    from detection_3d_amd._lib import lib
    return lib()


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)              # (a copy: the cases are read-only)


def _struct(p):
    from detection_3d_amd._lib import AugmentParams
    st = AugmentParams()
    for i in range(9):
        st.m[i], st.nrm[i] = float(p.m.flat[i]), float(p.nrm.flat[i])
    for i in range(3):
        st.color[i], st.u1[i], st.u2[i] = float(p.color[i]), float(p.u1[i]), float(p.u2[i])
    st.origin_offset, st.color_col, st.normal_col = p.origin_offset, p.color_col, p.normal_col
    return st


def _nan_buffer(dev, n, dtype=torch.float32):
    return torch.full((n + GUARD,), float("nan"), dtype=dtype, device=dev)


def _scratch(dev, n):
    nbytes = _L().d3d_augment_scratch_bytes(n)
    return torch.empty(nbytes + 64, dtype=torch.uint8, device=dev), nbytes


def _augment_voxelize(dev, pcl, p, scale, full, points=None, expect_rc=0):
    """d3d_augment_voxelize into sentinel-filled, guarded outputs -> (coords, feats, kept, offset); rows past `kept`
    must be untouched"""
    from detection_3d_amd._lib import ints, ptr, stream_of
    n, nfeat = pcl.shape
    scratch, nbytes = _scratch(dev, n)
    x = _dev(pcl, dev) if n else scratch
    pts = _dev(points, dev) if points is not None else None
    coords = torch.full((n * 3 + GUARD,), INT_SENTINEL, dtype=torch.int64, device=dev)
    feats = _nan_buffer(dev, n * nfeat)
    kept, off = ctypes.c_int(-5), (ctypes.c_double * 3)(*[OFFSET_SENTINEL] * 3)
    st = _struct(p)
    rc = _L().d3d_augment_voxelize(ptr(x), n, nfeat, ptr(pts), ctypes.byref(st), float(scale), ints(list(full)), ptr(coords),
                                   ptr(feats), ctypes.byref(kept), off, ptr(scratch), nbytes, stream_of())
    assert rc == expect_rc, (rc, _L().d3d_last_error())
    torch.cuda.synchronize()
    c, f = coords.cpu().numpy(), feats.cpu().numpy()
    if rc:                                                      # a refusal writes nothing at all
        assert kept.value == -5 and list(off) == [OFFSET_SENTINEL] * 3
        assert (c == INT_SENTINEL).all() and np.isnan(f).all()
        return None
    k = kept.value
    assert 0 <= k <= n
    assert (c[k * 3:] == INT_SENTINEL).all() and np.isnan(f[k * nfeat:]).all(), "a write past the kept rows"
    return c[:k * 3].reshape(k, 3), f[:k * nfeat].reshape(k, nfeat), k, np.array(off[:])


def _check_voxelize(dev, pcl, p, scale, full, points=None):
    """every kept row, its rank, every feature bit and the offset's bits against the reference -> keep"""
    wc, wf, woff, keep = A.voxelize_reference(pcl, p, scale, full, points)
    c, f, k, off = _augment_voxelize(dev, pcl, p, scale, full, points)
    assert k == int(keep.sum())
    assert np.array_equal(A.bits64(off), A.bits64(woff)), (off, woff)
    assert np.array_equal(c, wc)
    assert np.array_equal(F.bits(f), F.bits(wf))
    return keep


def _transform(dev, pcl, p):
    """d3d_augment_transform -> (points fp64 [n, 3], minmax [6]); the points guarded"""
    from detection_3d_amd._lib import check, ptr, stream_of
    n, nfeat = pcl.shape
    x = _dev(pcl, dev)
    pts = _nan_buffer(dev, n * 3, torch.float64)
    scratch = torch.empty(1024, dtype=torch.uint8, device=dev)
    mm = (ctypes.c_double * 6)(*[OFFSET_SENTINEL] * 6)
    st = _struct(p)
    check(_L().d3d_augment_transform(ptr(x), n, nfeat, ctypes.byref(st), ptr(pts), mm, ptr(scratch), 1024, stream_of()))
    torch.cuda.synchronize()
    got = pts.cpu().numpy()
    assert np.isnan(got[n * 3:]).all()
    return got[:n * 3].reshape(n, 3), np.array(mm[:])


def _blur(dev, raw):
    """d3d_elastic_blur -> (fields, tmp), both guarded"""
    from detection_3d_amd._lib import check, ints, ptr, stream_of
    nf, dims, total = raw.shape[0], raw.shape[1:], raw.size
    fields, tmp = _nan_buffer(dev, total), _nan_buffer(dev, total)
    fields[:total] = _dev(raw, dev).reshape(-1)
    check(_L().d3d_elastic_blur(ptr(fields), nf, ints(list(dims)), ptr(tmp), stream_of()))
    torch.cuda.synchronize()
    f, t = fields.cpu().numpy(), tmp.cpu().numpy()
    assert np.isnan(f[total:]).all() and np.isnan(t[total:]).all()
    return f[:total].reshape(raw.shape), t[:total].reshape(raw.shape)


def _apply(dev, pts, fields, gran, mag, expect_rc=0, want_minmax=True):
    """d3d_elastic_apply on a guarded copy of pts -> (displaced points, minmax [6])"""
    from detection_3d_amd._lib import ints, ptr, stream_of
    n = pts.shape[0]
    buf = _nan_buffer(dev, n * 3, torch.float64)
    buf[:n * 3] = _dev(pts, dev).reshape(-1)
    f = _dev(fields, dev)
    scratch = torch.empty(1024, dtype=torch.uint8, device=dev)
    mm = (ctypes.c_double * 6)(*[OFFSET_SENTINEL] * 6)
    rc = _L().d3d_elastic_apply(ptr(buf), n, ptr(f), ints(list(fields.shape[1:])), float(gran), float(mag),
                                mm if want_minmax else None, ptr(scratch), 1024, stream_of())
    assert rc == expect_rc, (rc, _L().d3d_last_error())
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.isnan(got[n * 3:]).all()
    return got[:n * 3].reshape(n, 3), np.array(mm[:])


# =================================================================================================== 1 - 3 affine
@pytest.mark.parametrize("n,nfeat", A.TRANSFORM_CASES)
def test_transform(dev, n, nfeat):
    """the fp64 points and the six min / max doubles, bit for bit, at every launch size"""
    m, nrm = A.free_matrices()
    pcl = A.cloud(n, nfeat)
    pts, mm = _transform(dev, pcl, A.prm(m, nrm))
    want = ref.affine(pcl, m)
    assert np.array_equal(A.bits64(pts), A.bits64(want))
    assert np.array_equal(A.bits64(mm), A.bits64(A.minmax_finite(want)))
    assert np.array_equal(mm, np.concatenate([want.min(0), want.max(0)]))


@pytest.mark.parametrize("flip,k,scale", A.EXACT_MATRICES)
def test_exact_affine(dev, flip, k, scale):
    """multiples of 1 / 64 through the quarter / flip matrices: the integer result, in the points and in the features"""
    pcl, ints = A.exact_cloud()
    m, nrm = A.quarter_matrices(flip, k, scale)
    want = A.exact_affine(ints[:, :3], m)
    pts, mm = _transform(dev, pcl, A.prm(m, nrm))
    assert np.array_equal(A.bits64(pts), A.bits64(ref.affine(pcl, m))) and np.array_equal(pts, want)
    assert np.array_equal(mm, np.concatenate([want.min(0), want.max(0)]))
    p = A.prm(m, nrm, normal_col=6)
    c, f, kept, off = _augment_voxelize(dev, pcl, p, scale, (4096, 4096, 4096))
    b = want - want.min(0)
    assert kept == A.EXACT_N and np.array_equal(off, -want.min(0))
    assert np.array_equal(c, np.trunc(b).astype(np.int64)) and np.array_equal(f[:, :3].astype(np.float64), b / scale)
    assert np.array_equal(f[:, 6:9].astype(np.float64), A.exact_affine(ints[:, 6:9], nrm * 64) / 64)
    assert np.array_equal(F.bits(f[:, 3:6]), F.bits(pcl[:, 3:6]))
    _check_voxelize(dev, pcl, p, scale, (4096, 4096, 4096))


def test_rounding_affine(dev):
    """free rotation, scale 1.0731: the oracle's bits (rows that one fused multiply-add would change are among them:
    asserted on the CPU) and |a - exact| <= gamma_3 sum|x_k m_kj| against rationals"""
    m, nrm = A.free_matrices()
    pcl = A.cloud(2049, 9)
    pts, _ = _transform(dev, pcl, A.prm(m, nrm))
    assert np.array_equal(A.bits64(pts), A.bits64(ref.affine(pcl, m)))
    rows = range(300)
    exact, mag = A.affine_exact(pcl, m, rows)
    g3 = A.frac(A.gamma53(3))
    for i in rows:
        for j in range(3):
            assert abs(A.frac(pts[i, j]) - exact[i][j]) <= g3 * mag[i][j], (i, j)
    sens, plain = A.contraction_sensitive(pcl, m, rows)
    assert sens.any((1, 2)).sum() > 50 and np.array_equal(A.bits64(pts[:300]), A.bits64(plain))
    p = A.prm(m, nrm, color=A.LAYOUT_COLOR, u1=(0.3, 0.6, 0.1), u2=(0.9, 0.2, 0.5), origin_offset=1, color_col=3, normal_col=6)
    assert _check_voxelize(dev, pcl, p, 50.0, (4096, 4096, 4096)).all()


# =================================================================================================== 4 identity
def _voxelize(dev, pcl, scale, full):
    from detection_3d_amd._lib import check, ints, ptr, stream_of
    n, nfeat = pcl.shape
    nbytes = _L().d3d_voxelize_scratch_bytes(n)
    scratch = torch.empty(nbytes + 64, dtype=torch.uint8, device=dev)
    x = _dev(pcl, dev) if n else scratch
    coords = torch.full((n * 3 + GUARD,), INT_SENTINEL, dtype=torch.int64, device=dev)
    feats = _nan_buffer(dev, n * nfeat)
    kept = ctypes.c_int(-1)
    check(_L().d3d_voxelize(ptr(x), n, nfeat, float(scale), ints(list(full)), ptr(coords), ptr(feats), ctypes.byref(kept),
                            ptr(scratch), nbytes, stream_of()))
    torch.cuda.synchronize()
    k = kept.value
    return coords[:k * 3].cpu().numpy().reshape(k, 3), feats[:k * nfeat].cpu().numpy().reshape(k, nfeat), k


def _identity_cases():
    for name in F.VOX_PATTERNS:
        yield "pattern-" + name, (lambda name=name: F.vox_pattern_case(name))
    yield "boundary", lambda: F.vox_boundary_case()[:3]
    yield "negative", F.vox_negative_case
    for name in F.NONDYADIC:
        yield "nondyadic-" + name, (lambda name=name: F.vox_nondyadic_case(name))
    for kind in F.NONFINITE:
        yield "nonfinite-" + kind, (lambda kind=kind: F.vox_nonfinite_case(kind)[:3])
    yield "no_points", lambda: (np.zeros((0, 9), np.float32), 50.0, (4, 4, 4))


_IDENTITY = dict(_identity_cases())


@pytest.mark.parametrize("name", list(_IDENTITY))
def test_identity_equals_voxelize(dev, name):
    """m = diag(scale) and nothing else: the coordinates, every feature bit (signalling NaNs, denormals, -0.0 in the
    pass-through columns) and the kept count of d3d_voxelize; the offset is -min"""
    pcl, scale, full = _IDENTITY[name]()
    wc, wf, wk = _voxelize(dev, pcl, scale, full)
    c, f, k, off = _augment_voxelize(dev, pcl, A.prm(np.eye(3) * float(scale)), scale, full)
    assert k == wk and np.array_equal(c, wc) and np.array_equal(F.bits(f), F.bits(wf))
    rc, rf, keep = F.voxelize_reference(pcl, scale, full)
    assert k == int(keep.sum()) and np.array_equal(c, rc) and np.array_equal(F.bits(f), F.bits(rf))
    if pcl.shape[0]:
        with np.errstate(invalid="ignore"):
            lo = np.fmin.reduce(pcl[:, :3].astype(np.float64) * np.float64(scale), 0)
        assert np.array_equal(off, -lo)
    else:
        assert np.array_equal(off, np.zeros(3))


# =================================================================================================== 5 filter edges
@pytest.mark.parametrize("minimum", [A.EDGE_ZERO, A.EDGE_TINY], ids=["zero", "tiny"])
@pytest.mark.parametrize("flip,k", A.QUARTER_FLIP)
def test_filter_edges(dev, flip, k, minimum):
    """b == 0 kept, b == full dropped, the fp32 neighbours of full; with the tiny minimum, the largest double below full
    kept -- after every quarter / flip matrix"""
    pcl, p, rows, _ = A.edge_case(flip, k, minimum)
    keep = _check_voxelize(dev, pcl, p, 64.0, A.EDGE_FULL)
    assert [bool(v) for v in keep] == [kept for _, _, kept in rows]


@pytest.mark.parametrize("kind", A.BELOW_KINDS)
@pytest.mark.parametrize("flip,k", A.QUARTER_FLIP)
def test_filter_edges_below_zero(dev, flip, k, kind):
    """the lower edge under the downward clip, after every quarter / flip matrix: with draws made for it the offset puts
    the edge row at b == 0 (kept) or one ulp of the offset below 0 (dropped)"""
    pcl, p, rows, _, target = A.below_edge_case(flip, k, kind)
    keep = _check_voxelize(dev, pcl, p, 64.0, A.EDGE_FULL)
    assert [bool(v) for v in keep] == [kept for _, _, kept in rows]
    _, _, _, off = _augment_voxelize(dev, pcl, p, 64.0, A.EDGE_FULL)
    assert np.array_equal(A.bits64(off), A.bits64(target))


def test_filter_edges_to_the_ulp(dev):
    """fp64 points around an offset that is a rounded product: b == 0 and the largest double below full kept, one ulp
    below 0 and b == full dropped, on each axis"""
    pcl, pts, p, full, rows = A.ulp_edge_case()
    keep = _check_voxelize(dev, pcl, p, 64.0, full, points=pts)
    assert [bool(v) for v in keep] == [kept for _, _, kept in rows]


@pytest.mark.parametrize("name", A.KEEP_PATTERNS)
def test_keep_patterns(dev, name):
    """kept rows and their ranks in row order (column 3 is the row index) under flip and a quarter turn; 524289 rows
    take the scan's second round"""
    pcl, p = A.pattern_case(name)
    keep = _check_voxelize(dev, pcl, p, 64.0, A.PATTERN_FULL)
    assert np.array_equal(keep, A.pattern_keep(name))


# =================================================================================================== 6, 7 offset
@pytest.mark.parametrize("kind", list(A.OFFSET_DRAWS))
def test_offset_regimes(dev, kind):
    """one call, one regime per axis: upward clip, downward clip (rows past full go), both clips 0"""
    pcl, pts, p, full = A.offset_case(kind)
    keep = _check_voxelize(dev, pcl, p, 64.0, full, points=pts)
    assert keep.any() and not keep.all()
    _, _, _, off = _augment_voxelize(dev, pcl, p, 64.0, full, points=pts)
    assert np.array_equal(A.bits64(off), A.bits64(ref.offset_of(pts, full, *((p.u1, p.u2) if p.origin_offset else ()))))


def test_offset_margin_exactly_zero(dev):
    pcl, pts, p, full = A.offset_q_case()
    assert _check_voxelize(dev, pcl, p, 64.0, full, points=pts).all()
    _, _, _, off = _augment_voxelize(dev, pcl, p, 64.0, full, points=pts)
    assert np.array_equal(off, np.full(3, -0.001))


def test_signed_zeros_in_the_minimum(dev):
    """rows at -0.0 and at +0.0 share the minimum: -0.0 is the minimum in either row order, so the offset is +0.0 and
    no kept feature is -0.0"""
    got = []
    for order in (0, 1):
        pcl, p = A.signed_zero_case(order)
        assert _check_voxelize(dev, pcl, p, 64.0, (4096, 4096, 4096)).all()
        c, f, k, off = _augment_voxelize(dev, pcl, p, 64.0, (4096, 4096, 4096))
        assert A.bits64(off)[0] == 0 and not np.signbit(f[:, 0]).any()
        _, mm = _transform(dev, pcl, p)
        assert mm[0] == 0 and np.signbit(mm[0])
        got.append((A.bits64(off).tolist(), F.bits(f[np.argsort(f[:, 3])]).tolist()))
    assert got[0] == got[1]


# =================================================================================================== 8 columns
@pytest.mark.parametrize("name", list(A.LAYOUTS))
def test_column_layouts(dev, name):
    """colour = (float)((double)p + c), normal = (float)row_times, wherever the columns are; the others bit for bit"""
    pcl, p, free = A.layout_case(name)
    assert _check_voxelize(dev, pcl, p, 50.0, (4096, 4096, 4096)).all()


@pytest.mark.parametrize("name", list(A.BAD_COLUMNS))
def test_column_arguments_refused(dev, name):
    nfeat, cc, nc = A.BAD_COLUMNS[name]
    pcl = A.cloud(40, nfeat)
    m, nrm = A.free_matrices()
    assert _augment_voxelize(dev, pcl, A.prm(m, nrm, color_col=cc, normal_col=nc), 50.0, (4096, 4096, 4096), expect_rc=-1) is None
    assert b"d3d_augment_voxelize" in _L().d3d_last_error()


# =================================================================================================== 9 blur
@pytest.mark.parametrize("nf", A.BLUR_NF)
@pytest.mark.parametrize("dims", A.BLUR_GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_blur(dev, dims, nf):
    """six passes bit for bit; the sixth lands in `fields`, the fifth is what `tmp` holds"""
    raw = A.blur_case(dims, nf)
    fields, tmp = _blur(dev, raw)
    assert np.array_equal(F.bits(fields), F.bits(np.stack([ref.blur(f) for f in raw])))
    assert np.array_equal(F.bits(tmp), F.bits(np.stack([A.blur_passes(f, 5) for f in raw])))
    if dims == (9, 8, 7):                                       # the last pass against rationals, from the device's own input
        cells = [tuple(c) for c in np.argwhere(np.ones(tmp.shape, bool))[::5]][:300]
        for c, (exact, mag) in zip(cells, A.blur_pass_exact(tmp, 2, cells)):
            assert abs(A.frac(fields[c]) - exact) <= A.blur_bound(exact, mag), c          # gamma_3 sum|x| w, then one fp32 rounding


@pytest.mark.parametrize("where", list(A.IMPULSES))
def test_blur_impulse(dev, where):
    """zero padding: exact +0 outside the 5 x 5 x 5 support, no wrap and no clamp"""
    raw = A.impulse_case(where)
    fields, _ = _blur(dev, raw)
    assert np.array_equal(F.bits(fields[0]), F.bits(ref.blur(raw[0])))
    sup = A.impulse_support(where)
    assert (F.bits(fields[0][~sup]) == 0).all() and (fields[0][sup] > 0).all()


# =================================================================================================== 10 sampling
@pytest.mark.parametrize("gran,mag", A.APPLY_STEPS)
@pytest.mark.parametrize("dims", A.APPLY_GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_apply_lattice(dev, dims, gran, mag):
    """nodes, faces and the quarter points of every cell: exact, so the bits of fp64 in any order; one ulp outside each
    face the point keeps its own bits"""
    fields = A.quarter_fields(dims)
    pts = A.lattice_points(dims, gran)
    want, disp = A.lattice_displaced(dims, gran, mag, fields, pts)
    got, mm = _apply(dev, pts, fields, gran, mag)
    assert np.array_equal(A.bits64(got), A.bits64(want))
    assert np.array_equal(A.bits64(got), A.bits64(ref.elastic_pass(pts, fields, gran, mag)))
    assert np.array_equal(A.bits64(mm), A.bits64(A.minmax_finite(want)))
    out = A.outside_points(dims, gran)
    got, mm = _apply(dev, out, fields, gran, mag)
    assert np.array_equal(A.bits64(got), A.bits64(out))
    assert np.array_equal(A.bits64(mm), A.bits64(A.minmax_finite(out)))


@pytest.mark.parametrize("n", [1, 257, A.REDUCE_FULL + 1])
@pytest.mark.parametrize("gran,mag", A.APPLY_STEPS[1:])
def test_apply_random_points(dev, n, gran, mag):
    """the oracle's bits with nothing excused, about a third of the points outside; a NaN row stays NaN and is ignored
    by the min / max; 262145 rows take the grid-stride loop; the bound against rationals"""
    dims = (5, 4, 3)
    fields = A.random_fields(dims)
    pts = A.random_points(n, dims, gran)
    want = A.elastic_reference(pts, fields, gran, mag)
    got, mm = _apply(dev, pts, fields, gran, mag)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() == (n > 1)
    ok = ~np.isnan(want)
    assert np.array_equal(A.bits64(got[ok]), A.bits64(want[ok]))
    assert np.array_equal(A.bits64(mm), A.bits64(A.minmax_finite(want)))
    g1 = (np.array(dims) - 1) * gran
    rows = np.flatnonzero((np.abs(np.nan_to_num(pts, nan=1e9)) <= g1).all(1))[:200]
    for i, (val, mg) in zip(rows, A.sample_exact(pts, fields, gran, rows)):
        for d in range(3):
            err = abs(A.frac(got[i, d]) - (A.frac(pts[i, d]) + val[d] * A.frac(mag)))
            assert err <= A.sample_bound(mg[d], val[d], pts[i, d], mag), (i, d)       # 22 roundings on sum|F|, then 2
    again, none = _apply(dev, pts, fields, gran, mag, want_minmax=False)       # the asynchronous form: the same points
    assert np.array_equal(A.bits64(again[ok]), A.bits64(want[ok])) and (none == OFFSET_SENTINEL).all()


@pytest.mark.parametrize("dims", [(1, 2, 2), (2, 1, 2), (2, 2, 1)], ids=lambda d: "x".join(map(str, d)))
def test_apply_refuses_a_grid_below_2(dev, dims):
    pts = A.random_points(257, (5, 4, 3), 6.0)
    got, mm = _apply(dev, pts, np.zeros((3,) + dims, np.float32), 6.0, 40.0, expect_rc=-1)
    assert b"below 2" in _L().d3d_last_error()
    ok = ~np.isnan(pts)
    assert np.array_equal(A.bits64(got[ok]), A.bits64(pts[ok])) and (mm == OFFSET_SENTINEL).all()


# =================================================================================================== 11 the whole call
def _cfg():
    from detection_3d_amd.config import get_cfg
    return get_cfg("4c_Fpn432")


def _fixed(aug, p):
    aug.sample_params = lambda: p
    return aug


_TARGETS = {"bbox3d": np.array([[2.0, 1.5, 0.1, 1.0, 2.0, 1.2, 0.3], [4.0, 3.0, 0.0, 0.6, 0.8, 2.0, -1.1]], np.float32),
            "labels": np.array([1, 2], np.int64)}


def _call(dev, aug, pcl):
    tg = {"bbox3d": torch.from_numpy(_TARGETS["bbox3d"].copy()), "labels": torch.from_numpy(_TARGETS["labels"].copy())}
    c, f, t = aug(_dev(pcl, dev), tg, _cfg())
    return c.cpu().numpy(), f.cpu().numpy(), t["bbox3d"].numpy()


def test_whole_call_with_elastic(dev):
    """Augment.__call__ with everything on: the fields drawn again from a device generator seeded with elastic_seed (the
    same shapes in the same order), then the oracle's affine map, two elastic passes, offset and filter -- coordinates
    and feature bits of every row"""
    from detection_3d_amd.augment import Augment, Params, linear_part, normal_matrix
    cfg = _cfg()
    scale, full = cfg.SPARSE3D.VOXEL_SCALE, cfg.SPARSE3D.VOXEL_FULL_SCALE
    pcl = A.scene_cloud(3001, 8)
    p = Params(-1.0, 1.0731, -1, 0.7321, np.array([0.3, 0.6, 0.1]), np.array([0.9, 0.2, 0.5]), np.array(A.LAYOUT_COLOR), 1234567)
    aug = _fixed(Augment(rotate="free", flip_x=True, scale_jitter=0.1, origin_offset=True, elastic=True, color_noise=0.02), p)
    c, f, _ = _call(dev, aug, pcl)
    m, nrm = linear_part(p, scale), normal_matrix(p)
    a = ref.affine(pcl, m)
    gen = torch.Generator(device=dev)
    gen.manual_seed(p.elastic_seed)
    for gran, mag in ((6 * scale // 50, 40 * scale / 50), (20 * scale // 50, 160 * scale / 50)):
        bb = ref.grid_dims(a, gran)
        raw = torch.randn((3,) + bb, dtype=torch.float32, device=dev, generator=gen).cpu().numpy()
        moved = ref.elastic_pass(a, [ref.blur(x) for x in raw], gran, mag)
        assert np.abs(moved - a).max() > 1.0                                  # the distortion moves points
        a = moved
    q = A.prm(m, nrm, color=p.color, u1=p.u1, u2=p.u2, origin_offset=1, color_col=3, normal_col=6)
    wc, wf, _, keep = A.voxelize_reference(pcl, q, scale, full, points=a)
    assert keep.sum() > 2900
    assert np.array_equal(c, wc) and np.array_equal(F.bits(f), F.bits(wf))


# =================================================================================================== non-finite rows
def _nonfinite_params(free):
    """fixed draws whose matrix has no negative entry in the rows that meet the bad coordinate, so that a +Inf stays
    +Inf (or a NaN) after the map: the contract is on the transformed coordinate.  free: theta = -0.5, both c and -s
    positive."""
    from detection_3d_amd.augment import Params
    z = np.zeros(3)
    return Params(1.0, 1.0731, -1 if free else 0, -0.5 if free else 0.0, z, z, np.array(A.LAYOUT_COLOR), 424242)


@pytest.mark.parametrize("elastic", [True, False], ids=["elastic", "plain"])
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("kind", list(A.NONFINITE))
def test_nonfinite_rows(dev, kind, axis, elastic):
    """the voxelizer's contract with elastic on and off: a NaN or +Inf coordinate drops its row alone -- the call returns
    the bits it returns for the cloud without that row, boxes (so the offset) included -- a -Inf one drops the cloud;
    nothing non-finite sizes the noise grid"""
    from detection_3d_amd.augment import Augment
    p = _nonfinite_params(free=False)
    kw = dict(rotate="none", scale_jitter=0.1, elastic=elastic, color_noise=0.02)
    pcl = A.nonfinite_cloud(kind, axis)
    c, f, boxes = _call(dev, _fixed(Augment(**kw), p), pcl)
    if kind == "-inf":                                           # nothing raises; the shift of that axis is +Inf, so are
        assert c.shape == (0, 3) and f.shape == (0, 9)          # the boxes' centres on it, and only they
        assert np.isposinf(boxes[:, axis]).all() and np.isfinite(np.delete(boxes, axis, 1)).all()
        assert np.array_equal(boxes[:, 3:], _call(dev, _fixed(Augment(**dict(kw, elastic=False)), p), pcl)[2][:, 3:])
        return
    wc, wf, wboxes = _call(dev, _fixed(Augment(**kw), p), np.delete(pcl, A.NONFINITE_ROW, 0))
    assert wc.shape[0] == pcl.shape[0] - 1 and np.isfinite(wboxes).all()
    assert np.array_equal(c, wc) and np.array_equal(F.bits(f), F.bits(wf)) and np.array_equal(F.bits(boxes), F.bits(wboxes))


@pytest.mark.parametrize("kind", ["nan", "+inf"])
def test_nonfinite_rows_free_rotation(dev, kind):
    """a bad y under a free rotation reaches the transformed x and y; several bad rows at once"""
    from detection_3d_amd.augment import Augment
    p = _nonfinite_params(free=True)
    kw = dict(rotate="free", scale_jitter=0.1, elastic=True, color_noise=0.02)
    pcl = np.array(A.scene_cloud())
    bad = [3, A.NONFINITE_ROW, 299]
    pcl[bad, 1] = A.NONFINITE[kind]
    c, f, boxes = _call(dev, _fixed(Augment(**kw), p), pcl)
    wc, wf, wboxes = _call(dev, _fixed(Augment(**kw), p), np.delete(pcl, bad, 0))
    assert wc.shape[0] == pcl.shape[0] - 3
    assert np.array_equal(c, wc) and np.array_equal(F.bits(f), F.bits(wf)) and np.array_equal(F.bits(boxes), F.bits(wboxes))


def test_nonfinite_extent(dev):
    """d3d_augment_transform and d3d_elastic_apply report the extent of the finite values only; the bad rows keep their
    values through the displacement"""
    pcl = np.array(A.cloud(257, 4))
    pcl[5, 0], pcl[100, 1], pcl[200, 2] = np.inf, -np.inf, np.nan
    p = A.prm(np.eye(3) * 50.0)
    pts, mm = _transform(dev, pcl, p)
    with np.errstate(invalid="ignore"):
        want = ref.affine(pcl, p.m)
    assert np.array_equal(np.isnan(pts), np.isnan(want)) and np.array_equal(pts[~np.isnan(want)], want[~np.isnan(want)])
    assert np.isfinite(mm).all() and np.array_equal(A.bits64(mm), A.bits64(A.minmax_finite(want)))
    dims = ref.grid_dims(np.where(np.isfinite(want), want, 0.0), 20)
    fields = np.random.RandomState(1).randn(3, *dims).astype(np.float32)
    got, mm = _apply(dev, pts, fields, 20.0, 160.0)
    fin = np.isfinite(want).all(1)
    moved = ref.elastic_pass(want[fin], fields, 20.0, 160.0)
    assert np.array_equal(A.bits64(got[fin]), A.bits64(moved))
    assert np.array_equal(np.isnan(got[~fin]), np.isnan(want[~fin]))
    assert np.array_equal(got[~fin][~np.isnan(want[~fin])], want[~fin][~np.isnan(want[~fin])])
    assert np.array_equal(A.bits64(mm), A.bits64(A.minmax_finite(moved)))
