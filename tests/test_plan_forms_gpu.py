"""Every build form of the rulebook plans (detection_3d_amd/csrc/plan.hip, grid_chain.hip, grid.hip) against exact tables.

Reference: the CPU oracle alone (oracle.subm_nbr, oracle.conv_rules scattered into nbr / nbr_dec, the identity table
for a 1x1x1 filter), through tests/plan_forms.py.  All results are integers: every comparison is exact.  Every case
builds through the C entry points, reads d3d_plan_last_form and asserts it equals plan_forms.expect_plan_form, exports
the raw plan (d3d_plan_export: rows, nbrT, blkmask) and runs check_plan_valid (permutation, -1 padding, nbrT the table
of its rows, blkmask exactly the OR of its 32 rows' masks, a mask class in ascending id order) and check_plan_order (the
order the form defines); the rule count must be the oracle's and the `executed` value of d3d_plan_stats 32 x the
popcounts of the model's block masks.  The conditions the scenes must meet (many masks and colliding hashed keys, a
class across a block boundary, two popcounts, duplicates) are asserted on the oracle's tables in
tests/test_plan_forms_cpu.py.

Forms the builder can select and the tests that reach them:

=========================================================  ====================================================
form                                                       tests
=========================================================  ====================================================
identity plan (k_identity_plan), 1x1x1 submanifold         test_identity_and_declined_half_probe
plain probes (k_subm_nbr) + single-workgroup sort          test_submanifold[scene-n-filter] mode 1, n <= 8192;
(k_plan_small, masks handed in; K <= 11 plain key,         test_submanifold_border_and_two_examples;
K = 27 hashed key) + k_plan_finish                         test_prefetch (the build without prefetch)
plain probes + radix sort (1 pass of 8 bits at K = 3,      test_submanifold mode 1 at 8193 and 20000 sites
9 bits at K = 9, 3 x 9 bits at K = 27) + k_plan_finish
half-probe form (k_subm_nbr_sym, prefilled table and       test_submanifold mode 2 (every count, both sorts);
masks) + either sort                                       test_submanifold_border_and_two_examples mode 2
half-probe declined (even filter, K = 1)                   test_identity_and_declined_half_probe
prefetched level-0 plan: probes, radix sort (n_dev form)   test_prefetch[points-mode] (plain and half-probe,
and k_plan_finish sized by the point count, site count     prefill on the library's stream), with the input
on the device; point lists by bound on the library's       layer's numbering and mean features of that build
stream
strided plan, masks in the finalisation (k_plan_small's    test_strided[geometry-n_out]: K = 8 / 27 / 4 / 16 /
own loop, k_row_mask), single-workgroup and radix sort     32 (plan_key without popcount at K > 27; 4 passes of
(1 pass at K = 8, 2 at K = 16, 3 at K = 27, 4 at K = 32);  8 bits), both grid builds
grid by k_conv_grid_small (<= 4096 entries) and by the
tiled chain
deconvolution view (kind 2), finalised lazily from         test_deconv_view[geometry-n_in]
nbr_dec, both sorts
the chain on the library's thread                          test_library_thread_builds_the_same_tables
radix digits wider than the sorted bits (K < 8, 11, 19..)  test_radix_sort_ignores_key_bits_above_the_sorted_bits,
                                                           test_strided[proj4-8192 / 8193], test_deconv_view[proj4-8193]
=========================================================  ====================================================

Not reached here: the AUTOMATIC half-probe threshold (262144 sites and more: tests/test_fullsize_gpu.py runs it on a
natural scene; d3d_subm_probe_mode 2 runs the same kernel at every size above); the empty plan and the empty grid level
(family 0 / grid 3: nothing is launched; tests/test_scn_gpu.py::test_empty_scene_builds_empty_levels); and the branch of
d3d_subm_prepare that finalises a prefetched table without a prefetched plan, which no call sequence reaches any more
(the prefetch always enqueues the whole plan).  Every test that changes the probe mode restores it in `finally`."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import oracle
from tests import plan_forms as P

pytestmark = pytest.mark.gpu


def _L():
    from detection_3d_amd._lib import lib
    return lib()


def plan_last_form():
    buf = (ctypes.c_int * len(P.PLAN_FIELDS))()
    assert _L().d3d_plan_last_form(buf, len(P.PLAN_FIELDS)) == len(P.PLAN_FIELDS)
    return dict(zip(P.PLAN_FIELDS, list(buf)))


@contextlib.contextmanager
def probe_mode(mode):
    was = _L().d3d_subm_probe_mode(-1)
    try:
        _L().d3d_subm_probe_mode(mode)
        yield
    finally:
        _L().d3d_subm_probe_mode(was)


def _build_input(dev, coords, size, prefetch=None):
    """d3d_input_layer_build_prefetch on the current stream -> (metadata, site count)"""
    from detection_3d_amd._lib import check, ints, ptr, stream_of
    from detection_3d_amd.sparseconvnet import SCN
    md = SCN.Metadata_3()
    c = torch.from_numpy(np.array(coords, np.int64)).to(dev)          # (a copy: the scenes are read-only)
    na = ctypes.c_int(0)
    check(_L().d3d_input_layer_build_prefetch(md._h, ptr(c), c.shape[0], c.shape[1], ints(list(size)), 1, 4,
                                              ints(list(prefetch)) if prefetch is not None else None, stream_of(),
                                              ctypes.byref(na)))
    md._in_active = na.value
    md._coords = c                                   # (kept alive while the build's kernels may read it)
    return md, na.value


def _subm_prepare(md, size, filt):
    from detection_3d_amd._lib import check, ints, stream_of
    nr = ctypes.c_long(-1)
    check(_L().d3d_subm_prepare(md._h, ints(list(size)), ints(list(filt)), stream_of(), ctypes.byref(nr)))
    return nr.value


def _export(md, kind, in_size, filt, stride=None):
    p = md.export_plan(kind, list(in_size), list(filt), list(stride) if stride is not None else None)
    torch.cuda.synchronize()
    out = {k: p[k] for k in ("K", "n_rows", "n_in", "n_blk")}
    out["rows"] = p["rows"].cpu().numpy()
    out["nbrT"] = p["nbrT"].cpu().numpy()
    out["blkmask"] = p["blkmask"].cpu().numpy().view(np.uint32)
    return out


def _stats(md, kind, in_size, filt, stride=None):
    from detection_3d_amd._lib import check, ints, stream_of
    nb, ex, ru = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_long(0)
    check(_L().d3d_plan_stats(md._h, kind, ints(list(in_size)), ints(list(filt)),
                              ints(list(stride) if stride is not None else [0, 0, 0]), ctypes.byref(nb), ctypes.byref(ex),
                              ctypes.byref(ru), stream_of()))
    return nb.value, ex.value, ru.value


def _check_plan(md, kind, in_size, filt, stride, nbr, n_rules, family, n_in=None):
    """steps 3-7 of every case: export, validity, order, rule count, executed steps -> the exported plan"""
    plan = _export(md, kind, in_size, filt, stride)
    masks = P.masks_of(nbr)
    P.check_plan_valid(plan, nbr)
    P.check_plan_order(plan, masks, family)
    if n_in is not None:
        assert plan["n_in"] == n_in
    n_blocks, executed, rules = _stats(md, kind, in_size, filt, stride)
    assert n_blocks == plan["n_blk"] and rules == n_rules
    assert executed == P.model_executed(masks, plan["K"], family)
    return plan


# ------------------------------------------------------------------------------------------------ submanifold
def _subm_case(dev, scene, n, filt, mode):
    coords, size = P.subm_scene(scene, n)
    nbr, _, total = P.subm_reference(scene, n, filt)
    K = int(np.prod(filt))
    with probe_mode(mode):
        md, na = _build_input(dev, coords, size)
        assert na == n
        plan_last_form()
        got_rules = _subm_prepare(md, size, filt)
        form = plan_last_form()
    want = P.expect_plan_form(P.SUBM, n, K, filt, probe_mode=mode)
    assert form == want, (form, want)
    assert got_rules == total
    _check_plan(md, P.SUBM, size, filt, None, nbr, total, want["family"], n_in=n)
    return want


@pytest.mark.parametrize("filt", P.SUBM_FILTERS, ids=lambda f: "x".join(map(str, f)))
@pytest.mark.parametrize("n", P.SUBM_COUNTS)
@pytest.mark.parametrize("scene", ["blob", "structured"])
def test_submanifold(dev, scene, n, filt):
    """plain (mode 1) and half-probe (mode 2) neighbour tables at the block, probe-workgroup, transpose-tile and
    single-workgroup-sort edges and over several radix tiles: the same exact plan either way"""
    for mode, probe in ((1, P.PLAIN), (2, P.HALF)):
        want = _subm_case(dev, scene, n, filt, mode)
        assert want["probe"] == probe and want["family"] == (P.SMALL if n <= P.SMALL_MAX else P.RADIX)


@pytest.mark.parametrize("n", P.EXTRA_COUNTS)
@pytest.mark.parametrize("scene", ["border", "two"])
def test_submanifold_border_and_two_examples(dev, scene, n):
    """sites at coordinate 0 and size - 1 of every axis (probes that leave the grid), and two examples that share
    coordinates (no rule may cross them)"""
    for filt in P.SUBM_FILTERS:
        for mode in (1, 2):
            _subm_case(dev, scene, n, filt, mode)


@pytest.mark.parametrize("n", P.IDENTITY_COUNTS)
def test_identity_and_declined_half_probe(dev, n):
    """mode 2 takes the half-probe form only where subm_nbr_is_sym allows: an even filter keeps the plain probes, the
    1x1x1 filter its identity plan"""
    with probe_mode(2):
        want = _subm_case(dev, "blob", n, (1, 1, 1), 2)
        assert want["family"] == P.IDENTITY and want["probe"] == P.NO_PROBE
        want = _subm_case(dev, "blob", n, (2, 2, 2), 2)
        assert want["probe"] == P.PLAIN
        assert _L().d3d_subm_probe_mode(-1) == 2
    assert _L().d3d_subm_probe_mode(-1) == 0


def test_probe_mode_and_form_record(dev):
    L = _L()
    was = L.d3d_subm_probe_mode(-1)
    try:
        assert was == 0
        assert L.d3d_subm_probe_mode(2) == 0 and L.d3d_subm_probe_mode(-1) == 2
        assert L.d3d_subm_probe_mode(5) == 2 and L.d3d_subm_probe_mode(-1) == 2        # out of range: ignored
        assert L.d3d_subm_probe_mode(1) == 2
    finally:
        L.d3d_subm_probe_mode(was)
    plan_last_form()
    assert plan_last_form() == dict.fromkeys(P.PLAN_FIELDS, 0)                         # cleared on read
    assert L.d3d_plan_last_form(None, 0) == len(P.PLAN_FIELDS)
    # a missing plan: the error of d3d_export_rules; null buffers: the sizes only
    from detection_3d_amd._lib import D3DError, check, ints, stream_of
    coords, size = P.subm_scene("blob", 33)
    md, _ = _build_input(dev, coords, size)
    dims = (ctypes.c_int * 4)()
    with pytest.raises(D3DError, match="rulebook not built"):
        check(L.d3d_plan_export(md._h, 0, ints(list(size)), ints([3, 3, 3]), ints([0, 0, 0]), None, None, None, dims,
                                stream_of()))
    _subm_prepare(md, size, (3, 3, 3))
    check(L.d3d_plan_export(md._h, 0, ints(list(size)), ints([3, 3, 3]), ints([0, 0, 0]), None, None, None, dims, stream_of()))
    assert list(dims) == [27, 33, 33, 2]
    # a cached plan records nothing
    plan_last_form()
    _subm_prepare(md, size, (3, 3, 3))
    assert plan_last_form() == dict.fromkeys(P.PLAN_FIELDS, 0)


# ------------------------------------------------------------------------------------------------ prefetched level 0
@pytest.mark.parametrize("mode", [0, 2], ids=["plain", "half"])
@pytest.mark.parametrize("points", P.PREFETCH_POINTS)
def test_prefetch(dev, points, mode):
    """The production form of the level-0 rulebook (FPN_Net builds it through d3d_input_layer_build_prefetch): probes,
    radix sort and k_plan_finish sized by the POINT count with the site count on the device, the half-probe prefill and
    the point lists on the library's own stream."""
    from detection_3d_amd._lib import check, ptr, stream_of
    filt, K = (3, 3, 3), 27
    coords = P.duplicated_points(points, points)
    size = P.SUBM_SIZE
    sop, loc = oracle.input_sites(coords)
    n = loc.shape[0]
    nbr, total = P.subm_table(loc, filt)
    rng = np.random.RandomState(points)
    feats = rng.randn(points, 5).astype(np.float32)
    with probe_mode(mode):
        plan_last_form()
        md, na = _build_input(dev, coords, size, prefetch=filt)
        form = plan_last_form()                                  # read right after the build
        want = P.expect_plan_form(P.SUBM, n, K, filt, prefetch_points=points, probe_mode=mode)
        assert na == n and form == want, (form, want)
        assert want["family"] == P.BOUND and want["probe"] == (P.HALF if mode == 2 else P.PLAIN)
        assert _subm_prepare(md, size, filt) == total            # the same stream: that plan, nothing new enqueued
        assert plan_last_form() == dict.fromkeys(P.PLAN_FIELDS, 0)
    _check_plan(md, P.SUBM, size, filt, None, nbr, total, P.BOUND, n_in=n)          # radix order below 8193 rows too
    # the input layer of the same build: site numbering, point lists built by bound on the library's stream
    assert np.array_equal(md.getSpatialLocations(list(size)).cpu().numpy(), loc.astype(np.int64))
    f = torch.from_numpy(feats).to(dev)
    out = torch.empty((n, feats.shape[1]), dtype=torch.float32, device=dev)
    check(_L().d3d_input_layer_forward(md._h, ptr(f), feats.shape[1], ptr(out), stream_of()))
    assert np.array_equal(out.cpu().numpy(), oracle.input_forward(feats, sop, n, True))
    off, idx = md.export_input_rules(points)
    rules = oracle.input_rule_table(sop, n)
    off, idx = off.cpu().numpy(), idx.cpu().numpy()
    assert np.array_equal(np.diff(off), rules[:, 0]) and off[0] == 0
    for r in rng.randint(0, n, 50):
        assert np.array_equal(idx[off[r]:off[r + 1]], rules[r, 1:1 + rules[r, 0]])
    # the same scene without prefetch: the same rule set, a valid plan in the order of its own family
    with probe_mode(mode):
        md2, na2 = _build_input(dev, coords, size)
        assert na2 == n and plan_last_form() == dict.fromkeys(P.PLAN_FIELDS, 0)
        assert _subm_prepare(md2, size, filt) == total
        form2 = plan_last_form()
    want2 = P.expect_plan_form(P.SUBM, n, K, filt, probe_mode=mode)
    assert form2 == want2 and want2["family"] == (P.SMALL if n <= P.SMALL_MAX else P.RADIX)
    _check_plan(md2, P.SUBM, size, filt, None, nbr, total, want2["family"], n_in=n)
    from tests.helpers import canon_rules
    ra = canon_rules(md.export_rules(0, list(size), list(filt)).cpu().numpy())
    rb = canon_rules(md2.export_rules(0, list(size), list(filt)).cpu().numpy())
    assert ra.shape[0] == total and np.array_equal(ra, rb)


# ------------------------------------------------------------------------------------------------ strided and deconvolution
def _conv_prepare(md, name):
    from detection_3d_amd._lib import check, ints, stream_of
    filt, stride, size, out_size = P.GEOMETRIES[name]
    n_out, nr = ctypes.c_int(-1), ctypes.c_long(-1)
    check(_L().d3d_conv_prepare(md._h, ints(list(size)), ints(list(out_size)), ints(list(filt)), ints(list(stride)),
                                stream_of(), ctypes.byref(n_out), ctypes.byref(nr)))
    return n_out.value, nr.value


@pytest.mark.parametrize("n_out", P.STRIDED_OUT_COUNTS)
@pytest.mark.parametrize("name", list(P.GEOMETRIES))
def test_strided(dev, name, n_out):
    """kind 1: masks computed in the finalisation, K = 8 / 27 / 4 / 16 / 32, the row-count edges of the sorts and both
    grid builds"""
    filt, stride, size, out_size = P.GEOMETRIES[name]
    K = int(np.prod(filt))
    coords = P.strided_coords(name, ("out", n_out))
    lo, nbr, _, n_rules = P.strided_reference(name, ("out", n_out))
    md, na = _build_input(dev, coords, size)
    assert na == coords.shape[0]
    plan_last_form()
    got_out, got_rules = _conv_prepare(md, name)
    form = plan_last_form()
    want = P.expect_plan_form(P.STRIDED, n_out, K, filt, grid_entries=na * P.max_out(filt, stride, out_size))
    assert form == want, (form, want)
    assert want["masks"] == 0 and want["probe"] == P.NO_PROBE
    assert want["grid"] == (P.GRID_SMALL if n_out <= 33 else P.GRID_TILED)
    assert got_out == n_out and got_rules == n_rules
    assert np.array_equal(md.getSpatialLocations(list(out_size)).cpu().numpy(), lo.astype(np.int64))
    _check_plan(md, P.STRIDED, size, filt, stride, nbr, n_rules, want["family"], n_in=na)


@pytest.mark.parametrize("n_in", P.DECONV_IN_COUNTS)
@pytest.mark.parametrize("name", list(P.GEOMETRIES))
def test_deconv_view(dev, name, n_in):
    """kind 2, finalised lazily from nbr_dec by d3d_deconv_prepare: rows are the fine sites"""
    from detection_3d_amd._lib import check, ints, stream_of
    filt, stride, size, out_size = P.GEOMETRIES[name]
    K = int(np.prod(filt))
    coords = P.strided_coords(name, ("in", n_in))
    lo, _, dec, n_rules = P.strided_reference(name, ("in", n_in))
    md, na = _build_input(dev, coords, size)
    assert na == n_in
    got_out, _ = _conv_prepare(md, name)
    assert got_out == lo.shape[0]
    plan_last_form()
    nr = ctypes.c_long(-1)
    check(_L().d3d_deconv_prepare(md._h, ints(list(out_size)), ints(list(size)), ints(list(filt)), ints(list(stride)),
                                  stream_of(), ctypes.byref(nr)))
    form = plan_last_form()
    want = P.expect_plan_form(P.DECONV, n_in, K, filt)
    assert form == want, (form, want)
    assert want["masks"] == 0 and want["probe"] == P.NO_PROBE and want["grid"] == P.NO_GRID
    assert want["family"] == (P.SMALL if n_in <= P.SMALL_MAX else P.RADIX) and nr.value == n_rules
    _check_plan(md, P.DECONV, size, filt, stride, dec, n_rules, want["family"], n_in=lo.shape[0])


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("bits", [3, 4, 11, 19, 21, 27])
def test_radix_sort_ignores_key_bits_above_the_sorted_bits(dev, bits, desc):
    """Regression: the radix sort took whole 8- to 10-bit digits, so where they cover more than `bits` (4 bits: one digit
    of 8; 19 bits: 2 x 10) the key bits above -- in a plan key the row's popcount -- were sorted too, and a K = 4
    projection plan of more than 8192 rows came out ordered by (popcount, mask) instead of by mask (found by
    test_strided[proj4-8193]).  The last digit is now cut to the bits that remain."""
    from detection_3d_amd._lib import check, ptr, stream_of
    n = 9000
    rng = np.random.RandomState(bits)
    keys = rng.randint(0, 1 << 32, n, dtype=np.int64).astype(np.uint32)
    keys[: n // 2] = keys[n // 2: 2 * (n // 2)] ^ np.uint32(0xFFFFFFFF << bits & 0xFFFFFFFF)    # equal low bits, other high bits
    vals = np.arange(n, dtype=np.int32)
    k = torch.from_numpy(keys.view(np.int32)).to(dev)
    v = torch.from_numpy(vals).to(dev)
    vo = torch.empty_like(v)
    nb = _L().d3d_sort_scratch_bytes(n, bits)
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    check(_L().d3d_sort_pairs(ptr(k), ptr(v), n, bits, int(desc), None, ptr(vo), ptr(scratch), nb, stream_of()))
    torch.cuda.synchronize()
    low = (keys & np.uint32((1 << bits) - 1)).astype(np.int64)
    assert np.array_equal(vo.cpu().numpy(), np.argsort(-low if desc else low, kind="stable").astype(np.int32))


# ------------------------------------------------------------------------------------------------ the library's thread
def test_library_thread_builds_the_same_tables(dev):
    """the pyramid of test_scn_gpu.py::test_geometry_chain_on_the_library_thread_equals_the_calls_made_in_line, built by
    single calls and by d3d_geometry_async_start: the raw tables are equal array for array (the form record lives on
    the library's threads, so it is not asserted here)"""
    from detection_3d_amd import sparseconvnet as scn
    from tests.helpers import small_scene
    size = (256, 256, 32)
    _, coords, feats = small_scene(21, 60000, (5.0, 4.0, 0.6), size)
    inp = [torch.from_numpy(coords), torch.from_numpy(feats).to(dev)]
    specs, cur = [], list(size)
    for _ in range(4):
        nxt = [v // 2 for v in cur]
        specs.append([1] + cur + nxt + [2, 2, 2] + [2, 2, 2])
        cur = nxt
    specs.append([1] + cur + [cur[0], cur[1], 1] + [1, 1, cur[2]] + [1, 1, 1])
    views = [[0] + sp[1:4] + sp[1:4] + [3, 3, 3] + [1, 1, 1] for sp in specs[:4]]
    views += [[2] + sp[4:7] + sp[1:4] + sp[7:10] + sp[10:13] for sp in specs[:4]]
    with torch.no_grad():
        a = scn.InputLayer(3, size, mode=4)(inp)
        b = scn.InputLayer(3, size, mode=4)(inp)
    for sp in specs:
        scn.SCN.Convolution_prepare(sp[1:4], sp[4:7], sp[7:10], sp[10:13], a.metadata)
    for v in views:
        if v[0] == 0:
            scn.SCN.SubmanifoldConvolution_prepare(v[1:4], v[7:10], a.metadata)
        else:
            scn.SCN.Deconvolution_prepare(v[1:4], v[4:7], v[7:10], v[10:13], a.metadata)
    main = torch.cuda.current_stream(dev)
    geo, plan = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    md = b.metadata
    geo.wait_stream(main)
    plan.wait_stream(main)
    md.set_geometry_stream(geo.cuda_stream)
    md.set_plan_stream(plan.cuda_stream)
    try:
        md.geometry_async_start(specs + views, geo.cuda_stream, plan.cuda_stream)
        md.geometry_async_wait(len(specs) + len(views) - 1, main.cuda_stream)
        md.geometry_async_finish()
    finally:
        main.wait_stream(geo)
        main.wait_stream(plan)
        md.set_plan_stream(None)
        md.set_geometry_stream(None)
    torch.cuda.synchronize()
    for e in specs + views:
        kind = e[0]
        key = (kind, e[4:7] if kind == 2 else e[1:4], e[7:10], e[10:13] if kind else None)
        pa, pb = _export(a.metadata, *key), _export(md, *key)
        assert pa["n_rows"] > 0
        for k in ("K", "n_rows", "n_in", "n_blk"):
            assert pa[k] == pb[k], (key, k)
        for k in ("rows", "nbrT", "blkmask"):
            assert np.array_equal(pa[k], pb[k]), (key, k)
