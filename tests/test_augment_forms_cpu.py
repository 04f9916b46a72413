"""tests/augment_forms.py without a GPU: every designed case sits where its name says (a boundary row really has
b == full, the contraction-sensitive rows exist, the zeros of both signs are at the minimum ...), the references of
augment_forms agree with tests/augment_ref.py where both apply, and the oracle itself -- augment_ref.blur and
augment_ref.elastic_pass -- equals scipy.ndimage.convolve and RegularGridInterpolator bit for bit on every designed
grid and point set."""
import math

import numpy as np
import pytest

from tests import augment_forms as A
from tests import augment_ref as ref
from tests import front_forms as F


# ------------------------------------------------------------------------------------------------------- matrices
def test_matrices_are_the_wrappers():
    from detection_3d_amd.augment import Params, linear_part, normal_matrix
    z = np.zeros(3)
    for flip, k, scale in A.EXACT_MATRICES:
        p = Params(flip, 1.0, k, k * math.pi / 2, z, z, z, 0)
        m, nrm = A.quarter_matrices(flip, k, scale)
        assert np.array_equal(m, linear_part(p, scale)) and np.array_equal(nrm, normal_matrix(p))
        assert set(np.abs(m).ravel().tolist()) == {0.0, scale}
    flip, theta, scale = A.FREE
    p = Params(flip, 1.0731, -1, theta, z, z, z, 0)
    m, nrm = A.free_matrices()
    assert np.array_equal(m, linear_part(p, 50)) and np.array_equal(nrm, normal_matrix(p)) and not np.array_equal(m, m.T)
    assert len({m.tobytes() for m, _ in (A.quarter_matrices(f, k, 64.0) for f, k in A.QUARTER_FLIP)}) == 8


def test_transform_sizes_sit_on_the_launch_edges():
    ns = sorted({n for n, _ in A.TRANSFORM_CASES})
    assert ns == [1, 255, 256, 257, 262144, 262145] and {f for _, f in A.TRANSFORM_CASES} == {3, 4, 9, 12}
    blocks = lambda n: max(1, min(1024, (n + 255) // 256))                   # reduce_blocks
    assert blocks(256) == 1 and blocks(257) == 2 and blocks(262144) == 1024 and A.REDUCE_FULL == 262144
    assert blocks(262145) * 256 < 262145                                      # the first grid-stride trip


# ------------------------------------------------------------------------------------------------------- affine
def test_exact_affine_is_exact_in_any_order():
    pcl, ints = A.exact_cloud()
    assert np.array_equal(pcl.astype(np.float64) * 64, ints)
    seen, shows = set(), []
    for flip, k, scale in A.EXACT_MATRICES:
        m, nrm = A.quarter_matrices(flip, k, scale)
        want = A.exact_affine(ints[:, :3], m)
        assert np.array_equal(ref.affine(pcl, m), want)
        x = pcl[:, :3].astype(np.float64)
        assert np.array_equal((x[:, 2:3] * m[2] + x[:, 1:2] * m[1]) + x[:, 0:1] * m[0], want)      # another order
        assert np.array_equal(np.array(A.affine_exact(pcl, m, range(20))[0], np.float64), want[:20])
        assert np.array_equal(ref.affine(pcl[:, 6:9], nrm), A.exact_affine(ints[:, 6:9], nrm * 64) / 64)
        seen.add(want.tobytes())
        shows.append(not np.array_equal(want, ref.affine(pcl, m.T)))
        assert shows[-1] == (not np.array_equal(m, m.T))
    assert sum(shows) == 3                                                     # a transposed m: the odd turns without flip
    assert len(seen) == len(A.EXACT_MATRICES)                                  # every matrix moves the cloud its own way


def test_rounding_affine_bound_and_contraction_rows():
    m, _ = A.free_matrices()
    pcl = A.cloud(2049, 9)
    a = ref.affine(pcl, m)
    rows = range(300)
    exact, mag = A.affine_exact(pcl, m, rows)
    for i in rows:
        for j in range(3):
            assert abs(A.frac(a[i, j]) - exact[i][j]) <= A.frac(A.gamma53(3)) * mag[i][j]
    sens, plain = A.contraction_sensitive(pcl, m, rows)
    assert np.array_equal(plain, a[:300])                                      # the oracle is the uncontracted form
    assert sens[:, :2, 0].sum() > 20 and sens[:, :2, 1].sum() > 20, sens.sum((0, 1))


# ------------------------------------------------------------------------------------------------------- filter
@pytest.mark.parametrize("minimum", [A.EDGE_ZERO, A.EDGE_TINY], ids=["zero", "tiny"])
@pytest.mark.parametrize("flip,k", A.QUARTER_FLIP)
def test_edge_rows_sit_on_the_edges(flip, k, minimum):
    pcl, p, rows, a = A.edge_case(flip, k, minimum)
    assert np.array_equal(ref.affine(pcl, p.m), a)                             # the map lands on the designed positions
    c, f, off, keep = A.voxelize_reference(pcl, p, 64.0, A.EDGE_FULL)
    assert np.array_equal(off, -np.array(minimum))
    b = a + off
    for i, (d, what, kept) in enumerate(rows):
        assert bool(keep[i]) == kept, (d, what)
        if d < 0:
            continue
        full = float(A.EDGE_FULL[d])
        if what == "at_minimum":
            assert b[i, d] == 0
        if what == "full":
            assert b[i, d] == (full if minimum == A.EDGE_ZERO else np.nextafter(full, 0.0))
        if what == "full_below":
            assert full - 1e-3 < b[i, d] < full
        if what == "full_above":
            assert full < b[i, d] < full + 1e-3
    assert np.array_equal(f[:, 3], np.flatnonzero(keep).astype(np.float32))   # ranks in row order
    # the matrix matters: the identity would keep other rows
    if (flip, k) != (1.0, 0):
        other = A.voxelize_reference(pcl, A.prm(np.eye(3) * 64), 64.0, A.EDGE_FULL)[3]
        assert not np.array_equal(other, keep)


@pytest.mark.parametrize("kind", A.BELOW_KINDS)
@pytest.mark.parametrize("flip,k", A.QUARTER_FLIP)
def test_below_edge_rows_sit_on_the_lower_edge(flip, k, kind):
    """the downward clip after each matrix: the offset is the designed one to the bit, the edge row has b == 0 (kept) or
    b == -ulp(offset) (dropped), its neighbours on the cloud's lattice are kept and dropped"""
    pcl, p, rows, a, target = A.below_edge_case(flip, k, kind)
    assert np.array_equal(ref.affine(pcl, p.m), a)                             # the map lands on the designed positions
    assert np.array_equal(a.min(0), A.BELOW_LO) and np.array_equal(a.max(0), A.BELOW_HI)
    q = (np.array(A.EDGE_FULL, np.float64) - a.max(0)) + a.min(0)
    assert (q == -11).all() and p.origin_offset == 1 and not p.u1.any() and ((p.u2 > 0) & (p.u2 < 1)).all()
    c, f, off, keep = A.voxelize_reference(pcl, p, 64.0, A.EDGE_FULL)
    assert np.array_equal(A.bits64(off), A.bits64(target))
    assert np.array_equal(off, ref.offset_of(a, A.EDGE_FULL, p.u1, p.u2))
    b = a + off
    edge = np.array(A.BELOW_EDGE)
    ulp = -edge - np.nextafter(-edge, 0.0)
    for i, (d, what, kept) in enumerate(rows):
        assert bool(keep[i]) == kept, (d, what)
        if what == "edge":
            assert a[i, d] == edge[d] and b[i, d] == (0.0 if kind == "at_zero" else -ulp[d])
        if what == "above":
            assert 0 < b[i, d] <= A.EDGE_STEP                                  # the next row of the cloud's lattice
        if what == "below":
            assert -A.EDGE_STEP - ulp[d] <= b[i, d] < 0
    assert (ulp > 0).all() and (ulp < 1e-14).all()
    assert np.array_equal(f[:, 3], np.flatnonzero(keep).astype(np.float32))   # ranks in row order
    if (flip, k) != (1.0, 0):                                                  # the matrix matters
        other = A.voxelize_reference(pcl, A.prm(np.eye(3) * 64, u2=p.u2, origin_offset=1), 64.0, A.EDGE_FULL)[3]
        assert not np.array_equal(other, keep)


def test_ulp_edge_rows():
    pcl, pts, p, full, rows = A.ulp_edge_case()
    c, f, off, keep = A.voxelize_reference(pcl, p, 64.0, full, points=pts)
    assert np.array_equal(off, ref.offset_of(pts, full, p.u1, p.u2))
    q = (np.array(full, np.float64) - pts.max(0)) + pts.min(0)
    assert (q + 0.001 < 0).all()                                               # the downward clip on every axis
    b = pts + off
    for i, (d, what, kept) in enumerate(rows):
        assert bool(keep[i]) == kept, (d, what)
        if what == "zero":
            assert b[i, d] == 0
        if what == "ulp_below_zero":
            assert b[i, d] < 0 and b[i, d] == -(np.nextafter(abs(off[d]), np.inf) - abs(off[d]))
        if what == "full":
            assert b[i, d] == full[d]
        if what == "full_below":
            assert b[i, d] == np.nextafter(float(full[d]), 0.0)


@pytest.mark.parametrize("name", A.KEEP_PATTERNS)
def test_keep_patterns(name):
    pcl, p = A.pattern_case(name)
    c, f, off, keep = A.voxelize_reference(pcl, p, 64.0, A.PATTERN_FULL)
    assert np.array_equal(keep, A.pattern_keep(name)) and (off == 0).all()
    assert np.array_equal(f[:, 3], np.flatnonzero(keep).astype(np.float32))
    assert (c.min(0) == 0).all() and (c < 60).all()
    n = pcl.shape[0]
    assert n in (2047, 2048, 2049, F.SECOND_ROUND)


# ------------------------------------------------------------------------------------------------------- offset
@pytest.mark.parametrize("kind", list(A.OFFSET_DRAWS))
def test_offset_regimes(kind):
    pcl, pts, p, full = A.offset_case(kind)
    lo, hi = pts.min(0), pts.max(0)
    q = (np.array(full, np.float64) - hi) + lo
    assert q[0] - 0.001 > 0 and q[1] + 0.001 < 0 and abs(q[2]) < 0.001 and q[2] != 0
    c, f, off, keep = A.voxelize_reference(pcl, p, 64.0, full, points=pts)
    b = pts + off
    if kind == "no_draw":
        assert p.origin_offset == 0 and p.u1.any() and np.array_equal(off, -lo)
        assert np.array_equal(off, ref.offset_of(pts, full))
    else:
        assert np.array_equal(off, ref.offset_of(pts, full, p.u1, p.u2))
        assert off[0] > -lo[0] and off[1] < -lo[1] and off[2] == -lo[2]        # up, down, neither
        assert (b[:, 1] < 0).any()
    assert (b[:, 1] >= full[1]).any() and not keep.all() and keep.any()
    if kind == "dyadic":                                                       # the two products are exact
        up, dn = max(q[0] - 0.001, 0.0), min(q[1] + 0.001, 0.0)
        assert A.frac(up * p.u1[0]) == A.frac(up) * A.frac(p.u1[0]) and A.frac(dn * p.u2[1]) == A.frac(dn) * A.frac(p.u2[1])


def test_offset_q_is_exactly_the_margin():
    pcl, pts, p, full = A.offset_q_case()
    q = (np.array(full, np.float64) - pts.max(0)) + pts.min(0)
    assert (q - 0.001 == 0).all() and (q + 0.001 > 0).all()
    c, f, off, keep = A.voxelize_reference(pcl, p, 64.0, full, points=pts)
    assert np.array_equal(off, np.full(3, -0.001)) and np.array_equal(off, ref.offset_of(pts, full, p.u1, p.u2))
    assert keep.all()                                                           # the highest row is at full - 0.001


def test_signed_zeros_are_at_the_minimum():
    outs = []
    for order in (0, 1):
        pcl, p = A.signed_zero_case(order)
        a = ref.affine(pcl, p.m)
        zero = a[:, 0] == 0
        assert a[:, 0].min() == 0 and (np.signbit(a[zero, 0])).any() and (~np.signbit(a[zero, 0])).any()
        first = np.flatnonzero(zero)
        outs.append(bool(np.signbit(a[first[0], 0])))
        lo = A.min_ordered(a)
        assert lo[0] == 0 and np.signbit(lo[0])                                # -0.0 is the ordered minimum
        c, f, off, keep = A.voxelize_reference(pcl, p, 64.0, (4096, 4096, 4096))
        assert keep.all() and not np.signbit(off[0]) and not np.signbit(f[:, 0]).any()
    assert outs[0] != outs[1]                                                  # the two orders meet the zeros in other order
    # a minimum taken as +0.0 would show: the rows at -0.0 would keep their sign
    assert np.signbit((a[zero, 0] + -0.0)).any()


# ------------------------------------------------------------------------------------------------------- columns
@pytest.mark.parametrize("name", list(A.LAYOUTS))
def test_layouts(name):
    pcl, p, free = A.layout_case(name)
    nfeat, cc, nc = A.LAYOUTS[name]
    assert pcl.shape == (A.LAYOUT_N, nfeat) and (p.color_col, p.normal_col) == (cc, nc)
    c, f, off, keep = A.voxelize_reference(pcl, p, 50.0, (4096, 4096, 4096))
    assert keep.all()
    for col in free:                                                           # pass-through: bit for bit
        assert np.array_equal(F.bits(f[:, col]), F.bits(pcl[:, col]))
    if free:
        assert np.isin(F.SPECIAL_BITS, pcl[:, free].view(np.uint32)).all()
        assert np.isfinite(np.delete(pcl, free, 1)).all()
    if cc >= 0:                                                                # an fp32 addition would round otherwise
        f32 = pcl[:, cc:cc + 3] + p.color.astype(np.float32)
        assert (F.bits(f32) != F.bits(f[:, cc:cc + 3])).sum() >= 10
    if nc >= 0:                                                                # rounded once, not per operation in fp32
        x = pcl[:, nc:nc + 3]
        n32 = np.stack([(x[:, 0] * np.float32(p.nrm[0, j]) + x[:, 1] * np.float32(p.nrm[1, j])) + x[:, 2] * np.float32(p.nrm[2, j])
                        for j in range(3)], 1)
        assert (F.bits(n32) != F.bits(f[:, nc:nc + 3])).sum() > 50
    if name == "trailing":
        assert free == [9, 10, 11]
    for nfeat, cc, nc in A.BAD_COLUMNS.values():                               # each breaks one requirement
        assert nfeat < 3 or (0 <= cc < 3) or cc + 3 > nfeat or (0 <= nc < 3) or nc + 3 > nfeat


# ------------------------------------------------------------------------------------------------------- scipy
def _scipy_blur(raw):
    import scipy.ndimage as ndimage
    noise = raw
    for axis in (0, 1, 2, 0, 1, 2):
        shape = [1, 1, 1]
        shape[axis] = 3
        w = np.ones(shape).astype("float32") / 3
        noise = ndimage.convolve(noise, w, mode="constant", cval=0)
    return noise


def test_blur_oracle_equals_scipy_bits():
    pytest.importorskip("scipy")
    totals = set()
    for dims in A.BLUR_GRIDS:
        for nf in A.BLUR_NF:
            raw = A.blur_case(dims, nf)
            totals.add(raw.size)
            for f in raw:
                got = ref.blur(f)
                assert got.dtype == np.float32 and np.array_equal(F.bits(got), F.bits(_scipy_blur(f)))
                assert np.array_equal(F.bits(A.blur_passes(f, 6)), F.bits(got))
    assert min(totals) < 256 and 256 in totals and max(totals) > 256
    for dims in A.APPLY_GRIDS:
        for f, raw in zip(A.random_fields(dims), np.random.RandomState(sum(dims) + 99).randn(3, *dims).astype(np.float32)):
            assert np.array_equal(F.bits(f), F.bits(_scipy_blur(raw)))


@pytest.mark.parametrize("where", list(A.IMPULSES))
def test_impulse_support(where):
    pytest.importorskip("scipy")
    f = A.impulse_case(where)[0]
    got = ref.blur(f)
    assert np.array_equal(F.bits(got), F.bits(_scipy_blur(f)))
    sup = A.impulse_support(where)
    assert (got[sup] > 0).all() and (F.bits(got[~sup]) == 0).all()            # +0 outside: no wrap, no clamp
    assert sup.sum() == {"corner": 27, "far_corner": 27, "centre": 125}[where]


def _scipy_pass(pts, fields, gran, mag):
    from scipy.interpolate import RegularGridInterpolator
    ax = [np.linspace(-(b - 1) * gran, (b - 1) * gran, b) for b in fields.shape[1:]]
    interp = [RegularGridInterpolator(ax, n, bounds_error=0, fill_value=0) for n in fields]
    return pts + np.hstack([i(pts)[:, None] for i in interp]) * mag


@pytest.mark.parametrize("gran,mag", A.APPLY_STEPS)
@pytest.mark.parametrize("dims", A.APPLY_GRIDS)
def test_sampling_oracle_equals_scipy_bits_and_the_lattice_is_exact(dims, gran, mag):
    pytest.importorskip("scipy")
    fields = A.quarter_fields(dims)
    assert len({f.tobytes() for f in fields}) == 3 and np.array_equal(fields * 4, np.round(fields * 4))
    pts = A.lattice_points(dims, gran)
    assert len(pts) == int(np.prod([4 * (d - 1) + 1 for d in dims]))
    g1 = (np.array(dims) - 1) * gran
    assert (np.abs(pts) <= g1).all()
    for d in range(3):                                                         # nodes, faces, every quarter of every cell
        assert set(np.unique(pts[:, d])) == set(A.lattice_axis(dims[d], gran)) and {-g1[d], g1[d]} <= set(pts[:, d])
    want, disp = A.lattice_displaced(dims, gran, mag, fields, pts)
    got = ref.elastic_pass(pts, fields, gran, mag)
    assert np.array_equal(A.bits64(got), A.bits64(want))                       # exact: any order gives these bits
    assert np.array_equal(A.bits64(got), A.bits64(_scipy_pass(pts, fields, gran, mag)))
    assert len({tuple(r) for r in disp}) > len(pts) // 3                       # the three fields displace differently
    assert not np.array_equal(disp[:, 0], disp[:, 1]) and not np.array_equal(disp[:, 1], disp[:, 2])
    out = A.outside_points(dims, gran)
    assert (np.abs(out) > g1).any(1).all()
    assert np.array_equal(A.bits64(ref.elastic_pass(out, fields, gran, mag)), A.bits64(out))
    assert np.array_equal(A.bits64(_scipy_pass(out, fields, gran, mag)), A.bits64(out))
    inside_again = ref.elastic_pass(np.clip(out, -g1, g1), fields, gran, mag) - np.clip(out, -g1, g1)
    assert (inside_again != 0).any()                                           # ... where the face itself is displaced


@pytest.mark.parametrize("n", [1, 257, 3001])
def test_random_points_oracle_equals_scipy_bits_and_bound(n):
    pytest.importorskip("scipy")
    dims, (gran, mag) = (5, 4, 3), A.APPLY_STEPS[2]
    fields = A.random_fields(dims)
    pts = A.random_points(n, dims, gran)
    ok = ~np.isnan(pts).any(1)
    assert ok.sum() == n - (n > 1)
    got = A.elastic_reference(pts, fields, gran, mag)
    assert np.array_equal(A.bits64(got[ok]), A.bits64(_scipy_pass(pts[ok], fields, gran, mag)))
    g1 = (np.array(dims) - 1) * gran
    inside = ok & (np.abs(np.nan_to_num(pts)) <= g1).all(1)
    if n > 1:
        assert 0.5 < inside.mean() < 0.8 and np.isnan(got[~ok, 0]).all()
        assert inside[n - 1] and (got[n - 1] != pts[n - 1]).all()              # the last row is displaced on every axis
    assert np.array_equal(A.bits64(got[ok & ~inside]), A.bits64(pts[ok & ~inside]))
    rows = np.flatnonzero(inside)[:200]
    for i, (val, mg) in zip(rows, A.sample_exact(pts, fields, gran, rows)):
        for d in range(3):
            assert abs(A.frac(got[i, d]) - (A.frac(pts[i, d]) + val[d] * A.frac(mag))) <= A.sample_bound(mg[d], val[d], pts[i, d], mag)


def test_blur_pass_bound_holds_for_the_oracle():
    raw = A.blur_case((9, 8, 7), 3)
    five = np.stack([A.blur_passes(f, 5) for f in raw])
    six = np.stack([ref.blur(f) for f in raw])
    cells = [tuple(c) for c in np.argwhere(np.ones(five.shape, bool))[::5]][:300]
    for c, (exact, mag) in zip(cells, A.blur_pass_exact(five, 2, cells)):
        assert abs(A.frac(six[c]) - exact) <= A.blur_bound(exact, mag)


# ------------------------------------------------------------------------------------------------------- non-finite
def test_nonfinite_extent_is_taken_from_finite_values():
    a = np.array([[1.0, -2.0, 3.0], [np.inf, np.nan, -np.inf], [-0.5, 4.0, 2.0]])
    assert np.array_equal(A.minmax_finite(a), [-0.5, -2.0, 2.0, 1.0, 4.0, 3.0])
    for kind in A.NONFINITE:
        for axis in range(3):
            pcl = A.nonfinite_cloud(kind, axis)
            bad = ~np.isfinite(pcl).all(1)
            assert bad.sum() == 1 and bad[A.NONFINITE_ROW]
