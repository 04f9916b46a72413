"""The front of every pass on exact cases: the voxelizer (detection_3d_amd/csrc/voxelize.hip), the input layer (grid.hip,
k_input_backward with it), the exclusive scan under both (scan_exclusive_i32, scan_sort.hip), the views of a finished
grid (grid_views.hip) and the row helpers at the end of bn.hip.

References: tests/front_forms.py (numpy fp64 / integers; held against the CPU oracle in tests/test_front_forms_cpu.py,
which also asserts that every designed case sits where its name says).  Integer results and everything whose arithmetic
is exact by design (integer features, power-of-two counts) are compared bit for bit; fp32 sums of normal data bit for bit
with the oracle AND per element against |got - y| <= gamma(cnt + 2) * sum|x| / cnt, gamma(k) = k u / (1 - k u), u = 2^-24
(one rounding of 1 / cnt, one per product, cnt - 1 additions).  Every output handed to a C entry is prefilled with a
sentinel (NaN, or -7 for integers) and followed by guard elements: an unwritten cell or a write past the end fails.

Forms and the tests that reach them:

=========================================================  ======================================================
form                                                       tests
=========================================================  ======================================================
d3d_voxelize: k_vox_min (1 .. 1024 workgroups, grid        test_voxelize_patterns[all / alternate / last_only /
stride from 262145 points), k_vox_flag, the scan, the      runs / run_to_end / none x n], test_voxelize_boundary,
pinned read-back, k_vox_write; n = 0                       test_voxelize_negative_cloud, test_voxelize_no_points
uncontracted x * scale + (-min) at a full significand      test_voxelize_nondyadic_scales[100/3, 1/0.03, 100/7]
NaN / +Inf / -Inf coordinates (the contract)               test_voxelize_nonfinite[nan, +inf, -inf]
scan_exclusive_i32: one tile, 2 tiles, 256 tiles, 257      test_voxelize_patterns (n = 1 .. 524289, flags 0 / 1),
tiles = a second round of k_scan_sums with its carry,      test_input_layer[distinct-524289, straddle-524289] (the
total on the device and none                               flag scan and, without a total, the count scan of both
                                                           point-list forms)
k_insert_points / k_flag_first / k_assign_input_sites:     test_input_layer[every case] x {plain, prefetch},
first-occurrence numbering; table capacity 2 n exactly     test_input_layer_module
and the next power of two (512, 513)
build_point_lists, lazy (bits from the site count; one     test_input_layer[...] plain: one_voxel (1 bit), pow2,
bit for a single site)                                     straddle, distinct, first_is_last, interleaved, border
build_point_lists by bound (counters, scan, sort over n    test_input_layer[...] prefetch: the same tables, every
"sites" on the library's stream, beside the prefetched     site compared; d3d_plan_last_form says family 4 sized
level-0 plan)                                              by the point count
k_input_forward / k_input_backward, mean (mode 4) and      test_input_layer (both modes, planes 1, 3, 9, 32, exact
sum (mode 3)                                               integers), test_input_layer_rounding, _module (autograd)
coordinates outside the grid (the bad-point word)          test_input_layer_refuses_points_outside[8 rows x 2]
k_locations, input grid and two strided levels             test_locations_of_strided_levels
k_sparse_to_dense and its backward: C entries, module,     test_sparse_to_dense[size-batch-fill], test_sparse_to_
autograd; a strided level; batch below the examples        dense_strided_level, test_sparse_to_dense_refuses_a_
                                                           batch_below_the_examples
k_anchors (A = 1, 4, 5, 16), k_anchors_maps (1, 2, 6       test_anchors[vs], test_anchor_generator_falls_back_to_
maps, A = 1 .. 4), AnchorGenerator.forward_cat fallback    one_launch_per_map
k_add: float4 body, scalar tail                            test_add, test_add_feature_planes
k_rows_to_bf16                                             test_rows_to_bf16[cin-width]
=========================================================  ======================================================

Not reached here: an arena too small for the prefetched tables (the build then silently takes the plain form: asserted
NOT to happen through d3d_plan_last_form); the half-probe prefill beside the insertion (tests/test_plan_forms_gpu.py::
test_prefetch[half]); clouds of 2^31 / nfeat points and more (the voxelizer indexes with size_t; nothing of that size
fits a quick test); d3d_input_layer_build with a geometry stream set (tests/test_scn_gpu.py); k_grid_extent's dense index
(reached through the RoI pooler, tests/test_roi_forms_gpu.py), which the new coordinate check now keeps inside its box.

Sensitivity: each mutation below was built into a scratch copy of the library and this file run against it (125 tests).
Every one fails; none can leave its buffers, for the reason in brackets.

=========================================================  ======================================================
mutation                                                   failing tests
=========================================================  ======================================================
k_scan_sums starts every round of 256 tile sums at 0       8, the 524289 cases and only they: test_voxelize_
instead of the carry [ranks and totals only shrink: every  patterns[all / alternate / runs / run_to_end-524289],
rank stays below the true one]                             test_input_layer[distinct / straddle-524289 x mode]
k_scan_tiles omits wave_off [ranks only shrink]            109: every case of more than 512 elements
k_insert_points stores `first` without atomicMin [one      38: test_input_layer (the cases with several points per
point per slot still flags itself: the count is right,     site), _module, _rounding, _refuses_points_outside
the numbering is not]                                      (the valid build behind the refusal)
build_point_lists sorts with one bit too few [still a      48: test_input_layer (both forms), _module, _rounding,
permutation of the point indices]                          _refuses_points_outside
k_input_forward applies 1 / cnt in sum mode [a value]      17: test_input_layer[... sum], _module[sum], _rounding[sum]
k_input_backward omits 1 / cnt in mean mode [a value]      17: test_input_layer[... mean], _module[mean], _rounding
k_vox_flag keeps a == full [the coordinate is a value      1: test_voxelize_boundary
that is written, never an index; kept <= n]
k_rows_to_bf16 truncates [a value]                         5: test_rows_to_bf16[every shape]
k_add drops its tail loop [elements stay unwritten]        2: test_add, test_add_feature_planes
=========================================================  ======================================================

No mutation was run for a swapped axis of the dense views: it would write outside the volume; the sizes (5, 7, 3) and
(32, 16, 8), all extents different with every corner occupied, cover it by design."""
import ctypes
import types

import numpy as np
import pytest
import torch

import oracle
from tests import front_forms as F
from tests import plan_forms as P

pytestmark = pytest.mark.gpu

GUARD = 16
INT_SENTINEL = -7


def _L():
    from detection_3d_amd._lib import lib
    return lib()


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)              # (a copy: the cases are read-only)


def _nan_buffer(dev, n):
    """fp32 [n + GUARD] of NaN: the first n are the output"""
    return torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev)


def _int_buffer(dev, n, dtype):
    return torch.full((n + GUARD,), INT_SENTINEL, dtype=dtype, device=dev)


def _guard_intact(buf, n):
    tail = buf[n:].cpu().numpy()
    return bool(np.isnan(tail).all()) if tail.dtype.kind == "f" else bool((tail == INT_SENTINEL).all())


def plan_last_form():
    buf = (ctypes.c_int * len(P.PLAN_FIELDS))()
    assert _L().d3d_plan_last_form(buf, len(P.PLAN_FIELDS)) == len(P.PLAN_FIELDS)
    return dict(zip(P.PLAN_FIELDS, list(buf)))


# =================================================================================================== voxelizer
def _voxelize_raw(dev, pcl, scale, full):
    """d3d_voxelize into sentinel-filled, guarded outputs -> (coords, feats, kept); rows past `kept` must be untouched"""
    from detection_3d_amd._lib import check, ints, ptr, stream_of
    n, nfeat = pcl.shape
    x = _dev(pcl, dev)
    coords, feats = _int_buffer(dev, n * 3, torch.int64), _nan_buffer(dev, n * nfeat)
    nbytes = _L().d3d_voxelize_scratch_bytes(n)
    scratch = torch.empty(nbytes + 64, dtype=torch.uint8, device=dev)
    kept = ctypes.c_int(-1)
    check(_L().d3d_voxelize(ptr(x) if n else ptr(scratch), n, nfeat, float(scale), ints(list(full)), ptr(coords), ptr(feats),
                            ctypes.byref(kept), ptr(scratch), nbytes, stream_of()))
    torch.cuda.synchronize()
    k = kept.value
    c, f = coords.cpu().numpy(), feats.cpu().numpy()
    assert (c[k * 3:] == INT_SENTINEL).all() and np.isnan(f[k * nfeat:]).all(), "a write past the kept rows"
    return c[:k * 3].reshape(k, 3), f[:k * nfeat].reshape(k, nfeat), k


def _check_voxelize(dev, pcl, scale, full, wrapper=False):
    want_c, want_f, keep = F.voxelize_reference(pcl, scale, full)
    c, f, k = _voxelize_raw(dev, pcl, scale, full)
    assert k == int(keep.sum())
    assert np.array_equal(c, want_c)
    assert np.array_equal(F.bits(f), F.bits(want_f))          # xyz by value, the other columns bit for bit (NaN payloads)
    if wrapper:
        from detection_3d_amd.voxelize import voxelize
        wc, wf = voxelize(_dev(pcl, dev), scale, full)
        assert np.array_equal(wc.cpu().numpy(), want_c) and np.array_equal(F.bits(wf.cpu().numpy()), F.bits(want_f))
    return keep


@pytest.mark.parametrize("name", list(F.VOX_PATTERNS))
def test_voxelize_patterns(dev, name):
    pcl, scale, full = F.vox_pattern_case(name)
    keep = _check_voxelize(dev, pcl, scale, full, wrapper=pcl.shape[0] <= 2049)
    assert np.array_equal(keep, F.vox_intended_keep(name))


def test_voxelize_boundary(dev):
    pcl, scale, full, rows = F.vox_boundary_case()
    keep = _check_voxelize(dev, pcl, scale, full, wrapper=True)
    assert [bool(k) for k in keep] == [want is not None for _, _, want in rows]


def test_voxelize_negative_cloud(dev):
    assert _check_voxelize(dev, *F.vox_negative_case(), wrapper=True).all()


@pytest.mark.parametrize("name", list(F.NONDYADIC))
def test_voxelize_nondyadic_scales(dev, name):
    """points at which one fused multiply-add would truncate to the integer below (asserted on the CPU)"""
    pcl, scale, full = F.vox_nondyadic_case(name)
    assert _check_voxelize(dev, pcl, scale, full, wrapper=True).all()


@pytest.mark.parametrize("kind", F.NONFINITE)
def test_voxelize_nonfinite(dev, kind):
    """the contract of voxelize.py: NaN and +Inf drop their point, -Inf drops the cloud"""
    pcl, scale, full, row = F.vox_nonfinite_case(kind)
    keep = _check_voxelize(dev, pcl, scale, full, wrapper=True)
    if kind == "-inf":
        assert not keep.any()
    else:
        assert not keep[row] and keep.sum() == len(keep) - 1


def test_voxelize_no_points(dev):
    c, f, k = _voxelize_raw(dev, np.zeros((0, 9), np.float32), 50.0, (4, 4, 4))
    assert k == 0
    from detection_3d_amd.voxelize import voxelize
    wc, wf = voxelize(torch.zeros((0, 4), device=dev), 50, (4, 4, 4))
    assert wc.shape == (0, 3) and wf.shape == (0, 4)


# =================================================================================================== input layer
PREFETCH = (3, 3, 3)


def _build(dev, coords, size, mode, prefetch, md=None, expect_rc=0):
    """d3d_input_layer_build_prefetch on the current stream -> (metadata, site count, return code)"""
    from detection_3d_amd._lib import check, ints, ptr, stream_of
    from detection_3d_amd.sparseconvnet import SCN
    md = md or SCN.Metadata_3()
    c = _dev(coords, dev)
    na = ctypes.c_int(-1)
    plan_last_form()
    rc = _L().d3d_input_layer_build_prefetch(md._h, ptr(c) if c.shape[0] else None, c.shape[0], c.shape[1],
                                             ints(list(size)), 1, mode, ints(list(prefetch)) if prefetch else None,
                                             stream_of(), ctypes.byref(na))
    assert rc == expect_rc, (rc, _L().d3d_last_error())
    if rc == 0:
        form = plan_last_form()
        if prefetch and c.shape[0]:                            # the prefetched form was taken, sized by the points
            assert form["family"] == P.BOUND and form["n_bound"] == c.shape[0] and form["n_rows"] == na.value, form
        else:
            assert form == dict.fromkeys(P.PLAN_FIELDS, 0)
    md._in_active = na.value
    md._coords = c                                             # (kept alive while the build's kernels may read it)
    return md, na.value, rc


def _tables(dev, md, size, n, na):
    """locations and the exported point lists, each into a guarded buffer"""
    from detection_3d_amd._lib import check, ints, ptr, stream_of
    loc = _int_buffer(dev, na * 4, torch.int64)
    check(_L().d3d_get_spatial_locations(md._h, ints(list(size)), ptr(loc), stream_of()))
    off, idx = _int_buffer(dev, na + 1, torch.int32), _int_buffer(dev, n, torch.int32)
    check(_L().d3d_input_layer_export(md._h, ptr(off), ptr(idx), stream_of()))
    torch.cuda.synchronize()
    assert _guard_intact(loc, na * 4) and _guard_intact(off, na + 1) and _guard_intact(idx, n)
    return loc[:na * 4].cpu().numpy().reshape(na, 4), off[:na + 1].cpu().numpy(), idx[:n].cpu().numpy()


def _forward(dev, md, x, na):
    from detection_3d_amd._lib import check, ptr, stream_of
    planes = x.shape[1]
    xt = _dev(x, dev) if x.shape[0] else torch.zeros((1, planes), device=dev)
    out = _nan_buffer(dev, na * planes)
    check(_L().d3d_input_layer_forward(md._h, ptr(xt), planes, ptr(out), stream_of()))
    torch.cuda.synchronize()
    assert _guard_intact(out, na * planes)
    return out[:na * planes].cpu().numpy().reshape(na, planes)


def _backward(dev, md, g, n):
    from detection_3d_amd._lib import check, ptr, stream_of
    planes = g.shape[1]
    gt = _dev(g, dev) if g.shape[0] else torch.zeros((1, planes), device=dev)
    d_in = _nan_buffer(dev, n * planes)                        # every point belongs to a site: all of it is written
    check(_L().d3d_input_layer_backward(md._h, ptr(gt), planes, ptr(d_in), stream_of()))
    torch.cuda.synchronize()
    assert _guard_intact(d_in, n * planes)
    return d_in[:n * planes].cpu().numpy().reshape(n, planes)


def _reference(name):
    coords, size = F.input_case(name)
    sop, loc = F.input_sites_reference(coords)
    off, idx = F.point_lists_reference(sop, loc.shape[0])
    return coords, size, sop, loc, off, idx


_REF = {}


def _input_reference(name):
    if name not in _REF:
        _REF.clear()                                           # (one case at a time: the big ones are 10s of MB)
        _REF[name] = _reference(name)
    return _REF[name]


@pytest.mark.parametrize("mode", [3, 4], ids=["sum", "mean"])
@pytest.mark.parametrize("name", F.INPUT_CASES)
def test_input_layer(dev, name, mode):
    """both builds (plain: lists sorted lazily by the site count; prefetch: lists by bound on the library's stream) give
    the reference's numbering, EVERY site's point list, and exact features forward and backward"""
    coords, size, sop, loc, off, idx = _input_reference(name)
    n, na = coords.shape[0], loc.shape[0]
    cnt = np.diff(off)
    exact = mode == 3 or bool(((cnt & (cnt - 1)) == 0).all())
    got = {}
    for prefetch in (None, PREFETCH):
        md, got_na, _ = _build(dev, coords, size, mode, prefetch)
        assert got_na == na
        gl, go, gi = _tables(dev, md, size, n, na)
        assert np.array_equal(gl, loc.astype(np.int64))
        assert np.array_equal(go, off) and np.array_equal(gi, idx)          # every site, ascending point index
        feats = {}
        for planes in ((1, 3, 9, 32) if n <= 2049 else (1, 9)):
            x, g = F.integer_features(n, planes), F.integer_features(na, planes, seed=5)
            y = _forward(dev, md, x, na)
            d = _backward(dev, md, g, n)
            want_y, want_abs, _ = F.input_forward_reference(x, sop, na, mode == 4)
            want_d = F.input_backward_reference(g, sop, na, mode == 4)
            if exact:
                assert np.array_equal(y.astype(np.float64), want_y) and np.array_equal(d.astype(np.float64), want_d)
            else:
                assert (np.abs(y - want_y) <= F.gamma(cnt + 2)[:, None] * want_abs).all()
                assert (np.abs(d - want_d) <= F.gamma(2) * np.abs(want_d)).all()
                assert np.array_equal(y, oracle.input_forward(x, sop, na, True))
                assert np.array_equal(d, oracle.input_backward(g, sop, na, True))
            feats[planes] = (y, d)
        got[prefetch] = feats
    for planes in got[None]:                                    # the two builds agree bit for bit
        for a, b in zip(got[None][planes], got[PREFETCH][planes]):
            assert np.array_equal(F.bits(a), F.bits(b))


@pytest.mark.parametrize("mode", [3, 4], ids=["sum", "mean"])
def test_input_layer_rounding(dev, mode):
    """normal data, arbitrary counts: bit-equal to the oracle (the same fp32 operations in the same order) and within
    the rounding bound of the fp64 result"""
    coords, size, x, g = F.rounding_case()
    sop, loc = F.input_sites_reference(coords)
    na = loc.shape[0]
    g = g[:na]
    want_y, want_abs, cnt = F.input_forward_reference(x, sop, na, mode == 4)
    want_d = F.input_backward_reference(g, sop, na, mode == 4)
    for prefetch in (None, PREFETCH):
        md, got_na, _ = _build(dev, coords, size, mode, prefetch)
        assert got_na == na
        y, d = _forward(dev, md, x, na), _backward(dev, md, g, coords.shape[0])
        assert np.array_equal(F.bits(y), F.bits(oracle.input_forward(x, sop, na, mode == 4)))
        assert np.array_equal(F.bits(d), F.bits(oracle.input_backward(g, sop, na, mode == 4)))
        assert (np.abs(y - want_y) <= F.gamma(cnt + 2)[:, None] * want_abs).all()
        assert (np.abs(d - want_d) <= F.gamma(2) * np.abs(want_d)).all()
    if mode == 3:                                               # the modes differ: a sum is not a mean
        assert not np.array_equal(y, oracle.input_forward(x, sop, na, True))


@pytest.mark.parametrize("on_device", [False, True], ids=["host_coords", "device_coords"])
@pytest.mark.parametrize("mode", [3, 4], ids=["sum", "mean"])
@pytest.mark.parametrize("name", ["pow2-2047", "interleaved-512", "border-513"])
def test_input_layer_module(dev, name, mode, on_device):
    """scn.InputLayer: 3 and 4 coordinate columns, coordinates on the host and on the device, features as a strided
    column slice, gradients through autograd; with and without the prefetch hook"""
    from detection_3d_amd import sparseconvnet as scn
    coords, size = F.input_case(name)
    sop, loc = F.input_sites_reference(coords)
    n, na = coords.shape[0], loc.shape[0]
    c = torch.from_numpy(np.array(coords))
    c = c.to(dev) if on_device else c
    for planes, hook in ((3, False), (9, True)):
        cloud = torch.from_numpy(F.integer_features(n, planes + 3)).to(dev)
        feats = cloud[:, 3:].detach().requires_grad_(True)
        assert not feats.is_contiguous()
        g = F.integer_features(na, planes, seed=5)
        if hook:
            scn.SCN.set_after_input_build(lambda m, s, run: None, PREFETCH)
        try:
            t = scn.InputLayer(3, size, mode=mode)([c, feats])
        finally:
            scn.SCN.set_after_input_build(None)
        assert np.array_equal(t.get_spatial_locations().cpu().numpy(), loc.astype(np.int64))
        t.features.backward(torch.from_numpy(g).to(dev))
        x = cloud[:, 3:].cpu().numpy()
        want_y, want_abs, cnt = F.input_forward_reference(x, sop, na, mode == 4)
        want_d = F.input_backward_reference(g, sop, na, mode == 4)
        y, d = t.features.detach().cpu().numpy(), feats.grad.cpu().numpy()
        if mode == 3 or name != "border-513":
            assert np.array_equal(y.astype(np.float64), want_y) and np.array_equal(d.astype(np.float64), want_d)
        else:
            assert np.array_equal(y, oracle.input_forward(x, sop, na, True))
            assert np.array_equal(d, oracle.input_backward(g, sop, na, True))
            assert (np.abs(y - want_y) <= F.gamma(cnt + 2)[:, None] * want_abs).all()


def _valid_scene_matches(dev, md, mode, prefetch):
    """the handle builds a valid scene that matches the oracle"""
    coords, size, x, g = F.rounding_case()
    sop, loc = oracle.input_sites(coords)
    na = loc.shape[0]
    md, got_na, _ = _build(dev, coords, size, mode, prefetch, md=md)
    assert got_na == na
    gl, go, gi = _tables(dev, md, size, coords.shape[0], na)
    rules = oracle.input_rule_table(sop, na)
    assert np.array_equal(gl, loc.astype(np.int64)) and np.array_equal(np.diff(go), rules[:, 0])
    for r in range(na):
        assert np.array_equal(gi[go[r]:go[r + 1]], rules[r, 1:1 + rules[r, 0]])
    assert np.array_equal(_forward(dev, md, x, na), oracle.input_forward(x, sop, na, mode == 4))


@pytest.mark.parametrize("prefetch", [None, PREFETCH], ids=["plain", "prefetch"])
@pytest.mark.parametrize("bad", list(F.BAD_POINTS))
def test_input_layer_refuses_points_outside(dev, bad, prefetch):
    """a coordinate outside [0, size) or an example index outside [0, 32768): D3D_ERR_ARG that names the point, nothing
    entered, and the same handle then builds a valid scene"""
    from detection_3d_amd._lib import ints
    from detection_3d_amd.sparseconvnet import SCN
    coords, size, _, _ = F.rounding_case()
    coords = np.array(coords)
    coords[100] = F.BAD_POINTS[bad]
    md = SCN.Metadata_3()
    used = md.arena_used()
    md, na, rc = _build(dev, coords, size, 4, prefetch, md=md, expect_rc=-1)
    msg = _L().d3d_last_error().decode()
    assert "point 100" in msg and "outside" in msg, msg
    assert na == 0 and md.arena_used() == used == 0
    n = ctypes.c_int(-1)
    assert _L().d3d_get_n_active(md._h, ints(list(size)), ctypes.byref(n)) == -4            # D3D_ERR_STATE: no grid
    assert _L().d3d_input_layer_forward(md._h, None, 3, None, None) == -4                    # ... and no input layer
    assert plan_last_form() == dict.fromkeys(P.PLAN_FIELDS, 0)
    _valid_scene_matches(dev, md, 4, prefetch)
    if prefetch:                                                # the prefetched plan of the valid build is a whole one
        nr = ctypes.c_long(-1)
        from detection_3d_amd._lib import check, stream_of
        check(_L().d3d_subm_prepare(md._h, ints(list(size)), ints(list(PREFETCH)), stream_of(), ctypes.byref(nr)))
        _, loc = oracle.input_sites(F.rounding_case()[0])
        assert nr.value == oracle.subm_nbr(loc, list(PREFETCH))[1]


# =================================================================================================== views
def _conv_prepare(md, size, out_size, filt, stride):
    from detection_3d_amd.sparseconvnet import SCN
    return SCN.Convolution_prepare(list(size), list(out_size), list(filt), list(stride), md)


def test_locations_of_strided_levels(dev):
    coords = F.anchor_scene()
    md, na, _ = _build(dev, coords, F.ANCHOR_SIZES[0], 4, None)
    _, loc = oracle.input_sites(coords)
    counts = [na]
    for i in range(2):
        filt, stride = F.ANCHOR_STEPS[i]
        n_out = _conv_prepare(md, F.ANCHOR_SIZES[i], F.ANCHOR_SIZES[i + 1], filt, stride)
        loc, _ = oracle.conv_rules(loc, list(filt), list(stride), list(F.ANCHOR_SIZES[i + 1]))
        assert n_out == loc.shape[0]
        counts.append(n_out)
        out = _int_buffer(dev, n_out * 4, torch.int64)
        from detection_3d_amd._lib import check, ints, ptr, stream_of
        check(_L().d3d_get_spatial_locations(md._h, ints(list(F.ANCHOR_SIZES[i + 1])), ptr(out), stream_of()))
        torch.cuda.synchronize()
        assert _guard_intact(out, n_out * 4)
        assert np.array_equal(out[:n_out * 4].cpu().numpy().reshape(-1, 4), loc.astype(np.int64))
    assert all(c % 64 for c in counts), counts


def _dense_forward(dev, md, size, feats, batch, expect_rc=0):
    from detection_3d_amd._lib import ints, ptr, stream_of
    planes = feats.shape[1]
    total = batch * planes * size[0] * size[1] * size[2]
    out = _nan_buffer(dev, total)
    f = _dev(feats, dev)
    rc = _L().d3d_sparse_to_dense_forward(md._h, ints(list(size)), ptr(f), planes, batch, ptr(out), stream_of())
    assert rc == expect_rc, (rc, _L().d3d_last_error())
    torch.cuda.synchronize()
    assert _guard_intact(out, total)
    return out[:total].cpu().numpy().reshape((batch, planes) + tuple(size)), out


def _dense_backward(dev, md, size, d_out, n):
    from detection_3d_amd._lib import check, ints, ptr, stream_of
    planes = d_out.shape[1]
    d_in = _nan_buffer(dev, n * planes)
    g = _dev(d_out, dev)
    check(_L().d3d_sparse_to_dense_backward(md._h, ints(list(size)), ptr(g), planes, ptr(d_in), stream_of()))
    torch.cuda.synchronize()
    assert _guard_intact(d_in, n * planes)
    return d_in[:n * planes].cpu().numpy().reshape(n, planes)


@pytest.mark.parametrize("full", [False, True], ids=["sparse", "full"])
@pytest.mark.parametrize("which", F.DENSE_BATCHES)
@pytest.mark.parametrize("size", F.DENSE_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_sparse_to_dense(dev, size, which, full):
    """every dense cell, forward and backward, through the C entries (guarded buffers) and the module under autograd"""
    from detection_3d_amd import sparseconvnet as scn
    coords, batch = F.dense_case(size, which, full)
    _, loc = F.input_sites_reference(coords)
    n = loc.shape[0]
    md, na, _ = _build(dev, coords, size, 4, None)
    assert na == n
    for planes in (1, 3, 32):
        rng = np.random.RandomState(planes)
        feats = rng.randn(n, planes).astype(np.float32)
        want = F.sparse_to_dense_reference(feats, loc, size, batch)
        dense, _ = _dense_forward(dev, md, size, feats, batch)
        assert np.array_equal(F.bits(dense), F.bits(want))                  # the empty cells are +0, none is left NaN
        d_out = rng.randn(*want.shape).astype(np.float32)
        assert np.array_equal(_dense_backward(dev, md, size, d_out, n), F.dense_to_sparse_reference(d_out, loc))
        # the module: forward, and the gradient through autograd
        f = torch.from_numpy(feats).to(dev).requires_grad_(True)
        t = scn.SparseConvNetTensor(f, md, torch.tensor(list(size)))
        out = scn.SparseToDense(3, planes)(t, batch_size=batch)
        assert np.array_equal(out.detach().cpu().numpy(), want)
        out.backward(torch.from_numpy(d_out).to(dev))
        assert np.array_equal(f.grad.cpu().numpy(), F.dense_to_sparse_reference(d_out, loc))
    if which in ("b1", "b2"):                                               # the batch the module works out itself
        with torch.no_grad():
            assert tuple(scn.SparseToDense(3, 3)(scn.SparseConvNetTensor(f[:, :3].contiguous(), md, torch.tensor(list(size)))).shape) \
                == (batch, 3) + tuple(size)


def test_sparse_to_dense_strided_level(dev):
    size, out_size = (32, 16, 8), (16, 8, 4)
    coords, batch = F.dense_case(size, "b3_empty_middle", False)
    md, na, _ = _build(dev, coords, size, 4, None)
    n_out = _conv_prepare(md, size, out_size, (2, 2, 2), (2, 2, 2))
    _, loc0 = oracle.input_sites(coords)
    loc, _ = oracle.conv_rules(loc0, [2, 2, 2], [2, 2, 2], list(out_size))
    assert n_out == loc.shape[0] and n_out % 64
    rng = np.random.RandomState(4)
    feats = rng.randn(n_out, 3).astype(np.float32)
    want = F.sparse_to_dense_reference(feats, loc, out_size, batch)
    dense, _ = _dense_forward(dev, md, out_size, feats, batch)
    assert np.array_equal(F.bits(dense), F.bits(want))
    d_out = rng.randn(*want.shape).astype(np.float32)
    assert np.array_equal(_dense_backward(dev, md, out_size, d_out, n_out), F.dense_to_sparse_reference(d_out, loc))
    # the strided level knows its examples too
    _, buf = _dense_forward(dev, md, out_size, feats, 2, expect_rc=-1)
    assert "batch 2" in _L().d3d_last_error().decode() and bool(torch.isnan(buf).all())


def test_sparse_to_dense_refuses_a_batch_below_the_examples(dev):
    """batch 1 on a two-example grid: D3D_ERR_ARG in front of the zero fill and the launch, nothing written; the handle
    then serves the right batch"""
    from detection_3d_amd import sparseconvnet as scn
    from detection_3d_amd._lib import D3DError
    size = (5, 7, 3)
    coords, batch = F.dense_case(size, "b2", False)
    _, loc = F.input_sites_reference(coords)
    md, na, _ = _build(dev, coords, size, 4, None)
    feats = np.random.RandomState(1).randn(na, 3).astype(np.float32)
    _, buf = _dense_forward(dev, md, size, feats, 1, expect_rc=-1)
    msg = _L().d3d_last_error().decode()
    assert "batch 1" in msg and "index 1" in msg, msg
    assert bool(torch.isnan(buf).all())                                     # not even the zero fill
    t = scn.SparseConvNetTensor(torch.from_numpy(feats).to(dev), md, torch.tensor(list(size)))
    with torch.no_grad(), pytest.raises(D3DError, match="batch 1"):
        scn.SparseToDense(3, 3)(t, batch_size=1)
    dense, _ = _dense_forward(dev, md, size, feats, batch)
    assert np.array_equal(F.bits(dense), F.bits(oracle.sparse_to_dense(feats, loc, size, batch)))


def _pyramid(dev):
    """six maps of one metadata -> (metadata, [locations of every map])"""
    coords = F.anchor_scene()
    md, _, _ = _build(dev, coords, F.ANCHOR_SIZES[0], 4, None)
    locs = []
    for i, (filt, stride) in enumerate(F.ANCHOR_STEPS):
        _conv_prepare(md, F.ANCHOR_SIZES[i], F.ANCHOR_SIZES[i + 1], filt, stride)
    for s in F.ANCHOR_SIZES:
        locs.append(md.getSpatialLocations(list(s)).cpu().numpy())
    return md, locs


@pytest.mark.parametrize("vs", [50.0, float(np.float32(100.0 / 3.0))], ids=["50", "100/3"])
def test_anchors(dev, vs):
    """d3d_anchors (A = 1, 4, 5, 16) and d3d_anchors_maps (1, 2, 6 maps, A = 1 .. 4): the fp32 reference bit for bit, and
    each other"""
    from detection_3d_amd._lib import check, floats, ints, ptr, stream_of
    md, locs = _pyramid(dev)
    counts = [l.shape[0] for l in locs]
    assert counts[0] == F.ANCHOR_POINTS and all(c > 0 for c in counts)
    per_map = {}
    for A in (1, 2, 3, 4, 5, 16):
        for i, (size, loc) in enumerate(zip(F.ANCHOR_SIZES, locs)):
            if A > 4 and i > 1:
                continue
            base = F.anchor_base(A, 10 * A + i)
            out = _nan_buffer(dev, loc.shape[0] * A * 7)
            check(_L().d3d_anchors(md._h, ints(list(size)), floats([float(v) for v in base.reshape(-1)]), A,
                                   floats([float(v) for v in F.ANCHOR_STRIDES[i]]), vs, ptr(out), stream_of()))
            torch.cuda.synchronize()
            assert _guard_intact(out, loc.shape[0] * A * 7)
            got = out[:loc.shape[0] * A * 7].cpu().numpy().reshape(-1, 7)
            assert np.array_equal(F.bits(got), F.bits(F.anchors_reference(loc, base, F.ANCHOR_STRIDES[i], vs))), (A, i)
            per_map[A, i] = got
    for A in (1, 2, 3, 4):
        for n_maps in (1, 2, 6):
            bounds = np.cumsum([0] + counts[:n_maps])
            assert all(b % (256 // A) for b in bounds[1:])                  # map boundaries inside a workgroup
            total = int(bounds[-1]) * A * 7
            out = _nan_buffer(dev, total)
            bases = [float(v) for i in range(n_maps) for v in F.anchor_base(A, 10 * A + i).reshape(-1)]
            check(_L().d3d_anchors_maps(md._h, n_maps, ints([v for s in F.ANCHOR_SIZES[:n_maps] for v in s]), floats(bases), A,
                                        floats([float(v) for s in F.ANCHOR_STRIDES[:n_maps] for v in s]), vs, ptr(out),
                                        stream_of()))
            torch.cuda.synchronize()
            assert _guard_intact(out, total)
            want = np.concatenate([per_map[A, i] for i in range(n_maps)])
            assert np.array_equal(F.bits(out[:total].cpu().numpy().reshape(-1, 7)), F.bits(want)), (A, n_maps)


@pytest.mark.parametrize("A,n_maps", [(5, 2), (4, 6), (2, 3)])
def test_anchor_generator_falls_back_to_one_launch_per_map(dev, A, n_maps, monkeypatch):
    """AnchorGenerator.forward_cat: one d3d_anchors_maps launch where it serves (A <= 4, at most 6 maps), else one
    d3d_anchors launch per map (A = 5; and 7 maps, here forced by the switch): the same anchors either way"""
    from detection_3d_amd import detector
    from detection_3d_amd import sparseconvnet as scn
    md, locs = _pyramid(dev)
    yaws = [0.0, -1.57, -0.785, 0.785, 0.3][:A]
    rpn = types.SimpleNamespace(YAWS=yaws, RATIOS=[1.0, 0.5, 2.0, 1.5, 0.7][:A],
                                ANCHOR_SIZES_3D=[[0.4 + 0.1 * i, 0.8, 1.2 + i] for i in range(n_maps)],
                                USE_YAWS=[i % 2 == 0 for i in range(n_maps)],
                                ANCHOR_STRIDE=[list(s) for s in F.ANCHOR_STRIDES[:n_maps]])
    cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(RPN=rpn), SPARSE3D=types.SimpleNamespace(VOXEL_SCALE=50))
    maps = [scn.SparseConvNetTensor(torch.zeros((locs[i].shape[0], 1), device=dev), md, torch.tensor(list(F.ANCHOR_SIZES[i])))
            for i in range(n_maps)]
    got = {}
    for one in (True, False):
        monkeypatch.setattr(detector, "_ANCHORS_ONE_LAUNCH", one)
        got[one] = detector.AnchorGenerator(cfg).forward_cat(maps).cpu().numpy()
    gen = detector.AnchorGenerator(cfg)
    want = np.concatenate([F.anchors_reference(locs[i], gen.cell_anchors[i].numpy(), F.ANCHOR_STRIDES[i], 50) for i in range(n_maps)])
    assert np.array_equal(F.bits(got[True]), F.bits(want)) and np.array_equal(F.bits(got[False]), F.bits(want))
    with torch.no_grad():
        tensors = torch.cat(gen(maps), 0).cpu().numpy()
    assert np.array_equal(tensors, want)


# =================================================================================================== row helpers
def test_add(dev):
    """d3d_add: the fp32 sum bit for bit (a NaN a NaN), float4 body and scalar tail, nothing past n"""
    from detection_3d_amd._lib import check, ptr, stream_of
    for n in F.ADD_N:
        a, b = F.add_case(n)
        # (prefilled with a finite value: a sum may be a NaN, and an unwritten NaN would pass for it)
        buf = torch.full((n + 4 + GUARD,), -123.0, dtype=torch.float32, device=dev)
        out = buf[4:]
        assert out.data_ptr() % 16 == 0
        at, bt = _dev(a, dev), _dev(b, dev)
        check(_L().d3d_add(ptr(at) if n else None, ptr(bt) if n else None, ptr(out) if n else None, n, stream_of()))
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:4] == -123.0).all() and (got[4 + n:] == -123.0).all(), n
        assert F.add_equal(got[4:4 + n], a, b), n
        with np.errstate(invalid="ignore"):
            assert not (a + b == -123.0).any()


def test_add_feature_planes(dev):
    from detection_3d_amd import sparseconvnet as scn
    size = torch.tensor([8, 8, 8])
    a, b = F.add_case(1025 * 3)
    a, b = a.reshape(1025, 3), b.reshape(1025, 3)
    with torch.no_grad():
        ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        got = scn.add_feature_planes([scn.SparseConvNetTensor(ta, None, size), scn.SparseConvNetTensor(tb, None, size)])
        assert F.add_equal(got.features.cpu().numpy().reshape(-1), a.reshape(-1), b.reshape(-1))
        wide = torch.from_numpy(np.concatenate([b, b], 1)).to(dev)          # a non-contiguous second operand
        got = scn.add_feature_planes([scn.SparseConvNetTensor(ta, None, size), scn.SparseConvNetTensor(wide[:, 3:], None, size)])
        assert not wide[:, 3:].is_contiguous()
        assert F.add_equal(got.features.cpu().numpy().reshape(-1), a.reshape(-1), b.reshape(-1))
        # bf16 storage: an fp32 sum, one rounding
        ha, hb = ta.to(torch.bfloat16), tb.to(torch.bfloat16)
        got = scn.add_feature_planes([scn.SparseConvNetTensor(ha, None, size), scn.SparseConvNetTensor(hb, None, size)])
        assert got.features.dtype == torch.bfloat16
        with np.errstate(invalid="ignore"):
            s = ha.float().cpu().numpy() + hb.float().cpu().numpy()
        assert F.bf16_equal(got.features.view(torch.int16).cpu().numpy().view(np.uint16), F.bf16_rne_bits(s))


@pytest.mark.parametrize("cin,width", F.BF16_SHAPES)
def test_rows_to_bf16(dev, cin, width):
    """round to nearest even on every edge, padding columns exactly +0, nothing past the rows"""
    from detection_3d_amd._lib import check, ptr, stream_of
    from detection_3d_amd.sparseconvnet import SCN
    for rows in F.BF16_ROWS:
        x = F.bf16_case(rows, cin)
        want = F.rows_to_bf16_reference(x, width)
        buf = torch.full((rows * width + GUARD,), 0x7FC1, dtype=torch.int16, device=dev)
        xt = _dev(x, dev)
        check(_L().d3d_rows_to_bf16(ptr(xt) if rows else None, rows, cin, width, ptr(buf), stream_of()))
        torch.cuda.synchronize()
        got = buf.cpu().numpy().view(np.uint16)
        assert (got[rows * width:] == 0x7FC1).all()
        got = got[:rows * width].reshape(rows, width)
        assert F.bf16_equal(got, want), (rows, cin, width)
        assert (got[:, cin:] == 0).all()                                    # +0, not -0
        if rows:
            assert F.bf16_equal(SCN.rows_to_bf16(xt, width).view(torch.int16).cpu().numpy().view(np.uint16), want)
