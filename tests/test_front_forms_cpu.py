"""tests/front_forms.py without a GPU: the designed cases sit where their names say, the references equal the CPU oracle
(oracle.voxelize, input_sites, input_rule_table, input_forward, input_backward, sparse_to_dense, OracleDetector.anchors;
torch's CPU .to(bfloat16) for the bf16 rounding) on every designed case -- except the NaN and +Inf coordinates,
where the voxelizer's contract departs from numpy's min on purpose -- and the argument checks of the touched entry
points that return before any GPU work."""
import ctypes
import types

import numpy as np
import pytest
import torch

import oracle
from oracle.detector_port import OracleDetector
from tests import front_forms as F


# ------------------------------------------------------------------------------------------------------- voxelizer
def _vox_equal_oracle(pcl, scale, full):
    c, f, keep = F.voxelize_reference(pcl, scale, full)
    with np.errstate(invalid="ignore"):
        oc, of = oracle.voxelize(np.array(pcl), scale, full)
    assert np.array_equal(c, oc) and np.array_equal(F.bits(f), F.bits(of))
    return c, f, keep


@pytest.mark.parametrize("name", list(F.VOX_PATTERNS))
def test_vox_patterns_keep_what_they_intend(name):
    pcl, scale, full = F.vox_pattern_case(name)
    assert pcl.shape == F.VOX_PATTERNS[name] and pcl.shape[0] in F.VOX_N
    c, f, keep = _vox_equal_oracle(pcl, scale, full)
    want = F.vox_intended_keep(name)
    assert np.array_equal(keep, want) and c.shape[0] == want.sum()
    if pcl.shape[1] > 3:                                     # the specials are there, and survive in the reference
        extra = pcl[:, 3:].view(np.uint32)
        assert np.isin(F.SPECIAL_BITS[:min(len(F.SPECIAL_BITS), (pcl.shape[0] + 6) // 7)], extra).all()
        assert np.array_equal(f[:, 3:].view(np.uint32), extra[keep])


def test_vox_pattern_shares():
    sizes = {F.VOX_PATTERNS[k][0] for k in F.VOX_PATTERNS}
    assert sizes == set(F.VOX_N) and {F.VOX_PATTERNS[k][1] for k in F.VOX_PATTERNS} == {3, 4, 9, 12}
    runs = F.vox_intended_keep("runs-524289")
    assert not runs[2047] and not runs[2048] and runs[2039] and runs[2056]          # a dropped run across index 2048
    assert not runs[524287] and runs[524288] and runs[524279]                       # ... and up to the last tile
    end = F.vox_intended_keep("run_to_end-524289")
    assert not end[524287] and not end[524288] and end[524279]                      # across index 524288
    assert F.SECOND_ROUND == 524289 and (F.SECOND_ROUND + F.SCAN_TILE - 1) // F.SCAN_TILE == F.SUM_ROUND + 1


def test_vox_boundary_points_sit_where_intended():
    pcl, scale, full, rows = F.vox_boundary_case()
    a = pcl[:, :3].astype(np.float64) * scale                # exact: 24-bit x 6-bit products; the minimum is 0
    assert (a.min(0) == 0).all()
    c, f, keep = _vox_equal_oracle(pcl, scale, full)
    out = np.full(len(rows), -1)
    out[keep] = np.arange(keep.sum())
    for i, (d, what, want) in enumerate(rows):
        if d < 0:
            continue
        assert keep[i] == (want is not None), (d, what)
        if what == "k":
            assert a[i, d] == F.BOUNDARY_K[d]
        if what == "k_below":
            assert F.BOUNDARY_K[d] - 1e-4 < a[i, d] < F.BOUNDARY_K[d]
        if what == "k_above":
            assert F.BOUNDARY_K[d] < a[i, d] < F.BOUNDARY_K[d] + 1e-4
        if what == "full":
            assert a[i, d] == full[d]
        if what == "full_below":
            assert full[d] - 1e-4 < a[i, d] < full[d]
        if want is not None:
            assert c[out[i], d] == want, (d, what)


def test_vox_negative_cloud_has_a_positive_shift():
    pcl, scale, full = F.vox_negative_case()
    assert (pcl[:, :3] < 0).all()
    c, _, keep = _vox_equal_oracle(pcl, scale, full)
    assert keep.all() and (c.min(0) == 0).all()


@pytest.mark.parametrize("name", list(F.NONDYADIC))
def test_vox_nondyadic_points_are_sensitive_to_contraction(name):
    pcl, scale, full = F.vox_nondyadic_case(name)
    assert (np.float64(scale).view(np.uint64) & np.uint64(0xFFF)) != 0          # a full significand
    sens = F.contraction_sensitive(pcl, scale)
    assert sens.any(0).all() and sens.sum() >= 6, sens.sum()                     # on every axis
    c, _, keep = _vox_equal_oracle(pcl, scale, full)
    assert keep.all()
    # at those points the uncontracted value is the integer itself
    a = pcl[:, :3].astype(np.float64) * scale
    two = a - a.min(0)
    assert (two[sens] == np.rint(two[sens])).all()


def test_vox_dyadic_scale_cannot_see_a_contraction():
    pcl, scale, _ = F.vox_negative_case()
    assert not F.contraction_sensitive(pcl[:200], scale).any()


@pytest.mark.parametrize("kind", F.NONFINITE)
def test_vox_nonfinite_contract(kind):
    pcl, scale, full, row = F.vox_nonfinite_case(kind)
    c, f, keep = F.voxelize_reference(pcl, scale, full)
    with np.errstate(invalid="ignore"):
        oc, of = oracle.voxelize(pcl, scale, full)
    if kind == "-inf":
        assert not keep.any() and oc.shape[0] == 0
    else:
        assert not keep[row] and keep.sum() == len(keep) - 1
        # numpy's min propagates the NaN and the whole cloud goes; an Inf becomes that NaN in the recipe's product with the
        # diagonal matrix (Inf * 0)
        assert oc.shape[0] == 0
        # ... while min() over the points that are kept gives the contract's result
        clean = np.delete(pcl, row, 0)
        oc, of = oracle.voxelize(clean, scale, full)
        assert np.array_equal(c, oc) and np.array_equal(F.bits(f), F.bits(of))


def test_vox_reference_on_no_points():
    c, f, keep = F.voxelize_reference(np.zeros((0, 9), np.float32), 50.0, (4, 4, 4))
    assert c.shape == (0, 3) and f.shape == (0, 9) and keep.shape == (0,)


# ------------------------------------------------------------------------------------------------------ input layer
@pytest.mark.parametrize("name", F.INPUT_CASES)
def test_input_cases_and_references(name):
    coords, size = F.input_case(name)
    kind, n = name.split("-")
    n = int(n)
    assert coords.shape[0] == n and coords.shape[1] == (4 if kind in ("interleaved", "border4") else 3)
    assert (coords[:, :3] >= 0).all() and (coords[:, :3] < np.array(size)).all()
    sop, loc = F.input_sites_reference(coords)
    if n:
        osop, oloc = oracle.input_sites(coords)
        assert np.array_equal(sop, osop) and np.array_equal(loc, oloc)
    na = loc.shape[0]
    off, idx = F.point_lists_reference(sop, na)
    cnt = np.diff(off)
    if n:
        rules = oracle.input_rule_table(sop, na)
        assert np.array_equal(cnt, rules[:, 0])
        for r in (range(na) if na <= 2049 else np.random.RandomState(0).randint(0, na, 2000)):
            assert np.array_equal(idx[off[r]:off[r + 1]], rules[r, 1:1 + rules[r, 0]])
    pow2 = bool(((cnt & (cnt - 1)) == 0).all())
    assert pow2 == (kind not in ("first_is_last", "border", "border4") and not (kind == "one_voxel" and n & (n - 1)))
    if kind == "one_voxel":
        assert na == 1 and cnt[0] == n
    if kind == "distinct":
        assert na == n
    if kind == "first_is_last":
        assert sop[-1] == na - 1 and cnt[-1] == 1
    if kind == "pow2":
        assert sorted(cnt.tolist()) == [2 ** k for k in range(11)]
    if kind == "straddle":
        assert idx[off[na - 1]:off[na]].tolist() == [n - 4, n - 3, n - 2, n - 1] and (n - 1) % F.SCAN_TILE == 0
    if kind == "interleaved":
        assert coords[:, 3].tolist() == [0, 1] * (n // 2) and na == n // 2 and (cnt == 2).all()
        assert len(np.unique(loc[:, :3], axis=0)) == na // 2                 # the same cells in both examples
    if kind in ("border", "border4"):
        assert size == (32768, 5, 3)
        for d in range(3):
            assert {0, size[d] - 1} <= set(loc[:, d].tolist())
    # capacity edges: 2 n a power of two exactly at 512, the next one at 513
    if n in (512, 513):
        assert (1 << int(2 * n - 1).bit_length()) == (1024 if n == 512 else 2048)
    # features: exact arithmetic in both modes where the counts are powers of two, in sum mode always
    for planes in ((1, 3, 9, 32) if n <= 2049 else (1, 9)):
        x = F.integer_features(n, planes)
        g = F.integer_features(na, planes, seed=5)
        for average in (False, True):
            y, _, _ = F.input_forward_reference(x, sop, na, average)
            d = F.input_backward_reference(g, sop, na, average)
            if pow2 or not average:
                assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
                assert np.array_equal(d.astype(np.float32).astype(np.float64), d)
                if n:
                    assert np.array_equal(oracle.input_forward(x, sop, na, average).astype(np.float64), y)
                    assert np.array_equal(oracle.input_backward(g, sop, na, average).astype(np.float64), d)


def test_second_round_cases_cross_the_carry():
    for name in F.INPUT_BIG:
        coords, _ = F.input_case(name)
        sop, loc = F.input_sites_reference(coords)
        assert coords.shape[0] == F.SECOND_ROUND                             # the flag scan: 257 tiles
    # the count scan of the lazy point lists covers n_active + 1 elements: 257 tiles when every point is a site (the lists
    # by bound scan n + 1 whatever the sites are)
    assert F.input_sites_reference(F.input_case("distinct-524289")[0])[1].shape[0] + 1 >= F.SECOND_ROUND


def test_rounding_case_bound_holds_for_the_oracle():
    coords, size, x, g = F.rounding_case()
    sop, loc = F.input_sites_reference(coords)
    na = loc.shape[0]
    assert 200 < na <= 300
    for average in (False, True):
        y, ya, cnt = F.input_forward_reference(x, sop, na, average)
        got = oracle.input_forward(x, sop, na, average).astype(np.float64)
        assert (np.abs(got - y) <= F.gamma(cnt + 2)[:, None] * ya).all()
        d = F.input_backward_reference(g[:na], sop, na, average)
        gd = oracle.input_backward(g[:na], sop, na, average).astype(np.float64)
        assert (np.abs(gd - d) <= F.gamma(2) * np.abs(d)).all()
    assert cnt.max() > 8 and len(set(cnt.tolist())) > 5 and ((cnt.astype(int) & (cnt.astype(int) - 1)) != 0).any()


def test_bad_points_are_outside():
    for name, row in F.BAD_POINTS.items():
        x, y, z, b = row
        assert not (0 <= x < 64 and 0 <= y < 32 and 0 <= z < 16 and 0 <= b < 32768), name
    assert F.BAD_POINTS["aliases_zero"][0] & 0xFFFF == 0                     # what the 16-bit site key would make of it


# ------------------------------------------------------------------------------------------------------------ views
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("which", F.DENSE_BATCHES)
@pytest.mark.parametrize("size", F.DENSE_SIZES)
def test_dense_cases_and_reference(size, which, full):
    coords, batch = F.dense_case(size, which, full)
    sop, loc = F.input_sites_reference(coords)
    assert loc.shape[0] == coords.shape[0] and len(set(size)) == 3           # distinct sites, all extents different
    present = sorted(set(coords[:, 3].tolist()))
    assert batch > max(present)
    assert {"b1": [0], "b2": [0, 1], "b3_empty_middle": [0, 2], "b4_trailing": [0, 1]}[which] == present
    for b in present:
        own = {tuple(r) for r in coords[coords[:, 3] == b, :3].tolist()}
        assert {(x, y, z) for x in (0, size[0] - 1) for y in (0, size[1] - 1) for z in (0, size[2] - 1)} <= own
        if full:
            assert len(own) == size[0] * size[1] * size[2]
    for planes in (1, 3, 32):
        feats = np.random.RandomState(planes).randn(loc.shape[0], planes).astype(np.float32)
        want = F.sparse_to_dense_reference(feats, loc, size, batch)
        assert np.array_equal(want, oracle.sparse_to_dense(feats, loc, size, batch))
        assert np.array_equal(F.dense_to_sparse_reference(want, loc), feats)
        assert (want != 0).sum() == (feats != 0).sum()


@pytest.mark.parametrize("vs", [50, float(np.float32(100.0 / 3.0))])
def test_anchor_reference_is_the_oracle(vs):
    rng = np.random.RandomState(3)
    locs = [np.concatenate([rng.randint(0, s, (37 + 11 * i, 1)) for s in F.ANCHOR_SIZES[0]] + [np.zeros((37 + 11 * i, 1), int)], 1)
            for i in range(3)]
    rpn = types.SimpleNamespace(ANCHOR_SIZES_3D=[[0.4, 0.8, 1.2], [1.0, 2.0, 3.0], [0.3, 0.3, 0.3]], USE_YAWS=[1, 0, 1],
                                ANCHOR_STRIDE=[list(s) for s in F.ANCHOR_STRIDES[:3]], YAWS=[0, -1.57, -0.785, 0.785],
                                RATIOS=[1.0, 0.5, 2.0, 1.5])
    orc = OracleDetector.__new__(OracleDetector)
    orc.cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(RPN=rpn), SPARSE3D=types.SimpleNamespace(VOXEL_SCALE=vs))
    want = orc.anchors(locs)
    got = []
    for size3, use_yaw, stride, loc in zip(rpn.ANCHOR_SIZES_3D, rpn.USE_YAWS, rpn.ANCHOR_STRIDE, locs):
        base = np.zeros((4, 7), np.float32)
        for j in range(4):
            if use_yaw:
                base[j, 3:6], base[j, 6] = size3, rpn.YAWS[j]
            else:
                base[j, 3:6] = np.float32(size3) * np.float32(rpn.RATIOS[j])
        got.append(F.anchors_reference(loc, base, stride, vs))
    assert np.array_equal(F.bits(np.concatenate(got)), F.bits(want))


def test_anchor_bases_and_map_boundaries():
    for A in (1, 4, 5, 16):
        b = F.anchor_base(A, A)
        assert np.signbit(b[0, 0]) and b[0, 0] == 0 and np.signbit(b[0, 6])
        out = F.anchors_reference(np.array([[3, 0, 1, 0]]), b, (8, 8, 4), 50)
        assert not np.signbit(out[0, 6]) and out[0, 0] == np.float32(3) / np.float32(50) * np.float32(8)
    assert len(F.ANCHOR_SIZES) == 6 and len(set(F.ANCHOR_SIZES)) == 6 and F.ANCHOR_STRIDES[0] == (8, 8, 4)
    assert F.ANCHOR_POINTS % 64 and all(F.ANCHOR_POINTS % (256 // A) for A in (1, 2, 4))


# ------------------------------------------------------------------------------------------------------ row helpers
@pytest.mark.parametrize("cin,width", F.BF16_SHAPES)
def test_bf16_reference_is_torch(cin, width):
    for rows in F.BF16_ROWS:
        x = F.bf16_case(rows, cin)
        want = torch.nn.functional.pad(torch.from_numpy(x), (0, width - cin)).to(torch.bfloat16).view(torch.int16).numpy()
        assert F.bf16_equal(want.view(np.uint16), F.rows_to_bf16_reference(x, width))
    x = F.bf16_case(257, 32)
    assert np.isin(F.BF16_EDGES, F.bits(x)).all()
    r = F.bf16_rne_bits(F.BF16_EDGES.view(np.float32))
    assert r[:4].tolist() == [0x3F80, 0x3F82, 0x3F81, 0x3F80]               # ties of both parities, and beside them
    assert r[4:8].tolist() == [0x7F80, 0x7F80, 0xFF80, 0x7F7F]              # the overflow to Inf
    assert r[8:12].tolist() == [0x0000, 0x0000, 0x0002, 0x8080]             # subnormals
    assert r[12:16].tolist() == [0x7F80, 0xFF80, 0x8000, 0x0000]
    assert ((r[16:] & 0x7FFF) > 0x7F80).all()                               # a NaN stays a NaN


def test_add_cases_hold_the_specials():
    assert {0, 1, 3, 4, 5, 1023, 1024, 1025, 3071, 3073} <= set(F.ADD_N)
    a, b = F.add_case(1025)
    with np.errstate(invalid="ignore"):
        s = a + b
    assert np.isnan(s).sum() >= 9 + 2 and np.isinf(s).any() and np.signbit(s[s == 0]).any() and (~np.signbit(s[s == 0])).any()
    assert F.add_equal(s, a, b) and not F.add_equal(np.where(s == 0, np.float32(0), s), a, b)


# ------------------------------------------------------------------------------------------------- argument checks
@pytest.fixture(scope="module")
def lib():
    from detection_3d_amd import _lib
    from detection_3d_amd.build import build_library
    build_library()
    return _lib.lib()


def _err(rc):
    from detection_3d_amd import _lib
    assert rc == -1                                                          # D3D_ERR_ARG
    return _lib.lib().d3d_last_error().decode()


def test_front_entries_refuse_bad_arguments(lib):
    """checks that return before anything touches a device"""
    vp = ctypes.c_void_p
    d = vp(4096)
    i3, one = (ctypes.c_int * 3)(8, 8, 8), ctypes.c_int(0)
    f7, f3 = (ctypes.c_float * (7 * 16))(), (ctypes.c_float * 18)()
    # voxelizer
    vox = lib.d3d_voxelize
    assert "bad arguments" in _err(vox(None, 4, 3, 50.0, i3, d, d, ctypes.byref(one), d, 1 << 20, None))
    assert "bad arguments" in _err(vox(d, 4, 2, 50.0, i3, d, d, ctypes.byref(one), d, 1 << 20, None))          # nfeat < 3
    assert "bad arguments" in _err(vox(d, -1, 3, 50.0, i3, d, d, ctypes.byref(one), d, 1 << 20, None))
    assert "bad arguments" in _err(vox(d, 4, 3, 50.0, None, d, d, ctypes.byref(one), d, 1 << 20, None))
    assert "bad arguments" in _err(vox(d, 4, 3, 50.0, i3, d, d, None, d, 1 << 20, None))
    assert "scratch" in _err(vox(d, 4, 3, 50.0, i3, d, d, ctypes.byref(one), d, lib.d3d_voxelize_scratch_bytes(4) - 1, None))
    one.value = 7
    assert vox(d, 0, 3, 50.0, i3, d, d, ctypes.byref(one), d, 1 << 20, None) == 0 and one.value == 0             # no points
    assert lib.d3d_voxelize_scratch_bytes(F.SECOND_ROUND) >= 1024 + 8 * F.SECOND_ROUND + 4 * (F.SUM_ROUND + 1)
    # input layer: what is refused before the handle is looked at
    build = lib.d3d_input_layer_build_prefetch
    assert "null argument" in _err(build(None, d, 4, 3, i3, 1, 4, None, None, ctypes.byref(one)))
    assert "null argument" in _err(build(d, d, 4, 3, None, 1, 4, None, None, ctypes.byref(one)))
    assert "null argument" in _err(build(d, d, 4, 3, i3, 1, 4, None, None, None))
    assert "columns" in _err(build(d, d, 4, 5, i3, 1, 4, None, None, ctypes.byref(one)))
    assert "columns" in _err(build(d, d, 4, 2, i3, 1, 4, None, None, ctypes.byref(one)))
    assert "mode" in _err(build(d, d, 4, 3, i3, 1, 2, None, None, ctypes.byref(one)))
    assert "bad coords" in _err(build(d, None, 4, 3, i3, 1, 4, None, None, ctypes.byref(one)))
    assert "bad coords" in _err(build(d, d, -1, 3, i3, 1, 4, None, None, ctypes.byref(one)))
    assert "bad arguments" in _err(lib.d3d_input_layer_forward(None, d, 3, d, None))
    assert "bad arguments" in _err(lib.d3d_input_layer_forward(d, d, 0, d, None))
    assert "bad arguments" in _err(lib.d3d_input_layer_backward(None, d, 3, d, None))
    assert "bad arguments" in _err(lib.d3d_input_layer_backward(d, d, 0, d, None))
    assert "null argument" in _err(lib.d3d_input_layer_export(d, None, d, None))
    # views
    assert "null argument" in _err(lib.d3d_get_spatial_locations(None, i3, d, None))
    assert "null argument" in _err(lib.d3d_get_spatial_locations(d, None, d, None))
    for A in (0, 17):
        assert "anchors: bad arguments" in _err(lib.d3d_anchors(d, i3, f7, A, f3, 50.0, d, None))
    assert "anchors: bad arguments" in _err(lib.d3d_anchors(d, i3, f7, 4, f3, 0.0, d, None))
    assert "anchors: bad arguments" in _err(lib.d3d_anchors(d, i3, None, 4, f3, 50.0, d, None))
    assert "anchors: bad arguments" in _err(lib.d3d_anchors(None, i3, f7, 4, f3, 50.0, d, None))
    i18 = (ctypes.c_int * 21)(*([8] * 21))
    for n_maps, A in ((0, 4), (7, 4), (2, 0), (2, 5)):
        assert "anchors_maps" in _err(lib.d3d_anchors_maps(d, n_maps, i18, f7, A, f3, 50.0, d, None))
    assert "anchors_maps" in _err(lib.d3d_anchors_maps(d, 2, i18, f7, 4, f3, -1.0, d, None))
    s2d = lib.d3d_sparse_to_dense_forward
    assert "bad arguments" in _err(s2d(d, i3, d, 0, 1, d, None))
    assert "bad arguments" in _err(s2d(d, i3, d, 3, 0, d, None))
    assert "bad arguments" in _err(s2d(d, i3, d, 3, 1, None, None))
    assert "bad arguments" in _err(s2d(None, i3, d, 3, 1, d, None))
    assert "bad arguments" in _err(lib.d3d_sparse_to_dense_backward(d, i3, d, 0, d, None))
    assert "bad arguments" in _err(lib.d3d_sparse_to_dense_backward(None, i3, d, 3, d, None))
    # row helpers
    assert lib.d3d_add(None, None, None, 0, None) == 0
    for a, b, o in ((None, d, d), (d, None, d), (d, d, None)):
        assert "null pointer" in _err(lib.d3d_add(a, b, o, 4, None))
    r2b = lib.d3d_rows_to_bf16
    for rows, cin, width in ((-1, 9, 16), (4, 0, 16), (4, 17, 16), (4, 9, 12), (4, 9, 0)):
        assert "rows_to_bf16" in _err(r2b(d, rows, cin, width, d, None))
    assert r2b(None, 0, 9, 16, None, None) == 0
    assert "null or unaligned" in _err(r2b(d, 4, 9, 16, vp(4096 + 8), None))
    assert "null or unaligned" in _err(r2b(None, 4, 9, 16, d, None))
