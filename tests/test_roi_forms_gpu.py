"""Every rotated-RoIAlign launch form on the MI355X against fp64 results: the sparse forward (fp32 and bf16 rows, hash and
dense-index lookup, host crop and device extent, one level and several, both layouts), the atomic backward, its
fixed-order form, the bf16 gradient forms, and the dense kernels.

Every case calls through the wrappers of detection_3d_amd/roi_align_rotated_3d.py, reads d3d_roi_last_form and asserts
it equals tests.roi_forms.expect_roi (the dispatch arithmetic of the roi_*.hip files restated from their constants, itself
checked in test_roi_forms_cpu.py), and then compares what the kernels wrote, element by element, with the fp64
reference of tests.roi_forms:

* exact cases -- yaw 0, dyadic geometry (every sample on the 1/8-pixel lattice), values and gradients non-zero integers
  in +-{1..4}, NS a power of two: every result is an fp32 number whatever the order of the sums, so fp32 outputs match
  to the bit and bf16 outputs are the round-to-nearest-even of the exact value, to the bit.  A lost or doubled tap, a bin
  not written or a wrong channel changes bits.
* rounding cases -- normal data with per-channel scales 1, 1/64 and 64, arbitrary yaw, no lattice: every element within
  position bound x slope + gamma_n x magnitude (+ half a bf16 ulp), derived in tests/roi_forms.py and shown in
  test_roi_forms_cpu.py to reject a lost tap, a lost partial step, a wrong count, swapped corners, a flipped sine, the
  wrong z test, a doubled record and a lost chunk partial.

form                                                          tests
============================================================  =========================================================
k_roi_sparse<float / bf16>, C 1 .. 256: scalar loads at odd   test_forward[fwd_channels]
C, pair loads, a second 128-channel chunk of 1 pair / ragged
bins 1 .. 192: fewer groups than waves, ragged last group,    test_forward[bins]
one group per wave, the workload's 6x8x4
NS 1, 8, 27 and adaptive 6, 32, 30, 4 (steps of 8 with a      test_forward[subsamples]; the merged-cell list lengths
partial last step); the 8 / 4 / 2 / 1 ladder over lists of    0, 1, 2, 3, 4-7, 8, 9-15, >= 16 are asserted from the
0 .. 60 merged cells                                          reference's tap list in test_roi_forms_cpu.py
hash lookup + host crop (autograd wrapper, layout 0);         every case of test_forward runs both
dense index + device extent (_into, crop None, layout 1)
hash lookup + device extent (dense index declined above       test_lookup_far
kDenseMaxCells: 4001 x 4001 x 501 cells)
RoIs of the second example (hash and dense index)             every case: RoI n belongs to example n % 2
roi_levels with level 0 .. 3 (single-level entry); the        test_levels
levels entry with 1 .. 4 maps of strides 1, 2, 4, 8; rows of
level -1, of a level without a map and of level 7 untouched
geometry edges: size below a pixel, box outside, cut by each  test_forward[edges], test_backward[edges],
face, z above the map (forward clamps, backward drops),       test_fixed_order[edges]
centre in the -1 .. 0 band, K = 0, K = 1, no site in the box
k_roi_sparse_bwd<float>: C 1 .. 130 (1 .. 3 chunks of 64)     test_backward[bwd_channels]
bins 1 .. 192 and the LDS limit of 255 bins; 256 refused by   test_backward[bins, bwd_only_bins]; test_256_bins_refused
the fp32 and the bf16 entry
k_roi_sparse_bwd<bf16> + k_roi_f32_to_bf16 (tail 0 .. 3)      test_backward[.., bf16]; test_backward[cvt_tails]
fixed-order form, fp32 and bf16: k_roi_det_transpose / taps   test_fixed_order[det_channels, bins, bwd_only_bins,
/ bounds / sum / join; C 1 .. 320 (second pass above 256);    edges, det_lists]; twice the same bits; the exact class
lists over >= 3 chunks, ending / starting on a chunk          equals the atomic form; the chunk counts are asserted
boundary, rows without records; fp32 added to a non-zero      with the grid's own row numbers; sampling_ratio 0 refused
buffer, bf16 written over NaN                                 (test_fixed_order_refuses_adaptive_sampling)
fixed-order form at sampling_ratio 1, 2, 3: NS 1, 8 and 27    test_fixed_order[subsamples]
(`pos` carried over the steps of k_roi_det_taps, the s < NS
guard of the partial step, one bin's records from several
steps in one row's list)
k_roi_dense, k_roi_dense_bwd: B 2, C 1 and 5, the same bins   test_dense
and sub-sample counts

Largest error / bound seen on the MI355X per check, with the case that gave it (test_zz_margins prints them; recorded,
not used to set anything).  Every exact check: equal bits.
  forward fp32                      0.0043  test_dense, C = 5, 6x8x4 bins (sparse forms: 0.0041, fwd_channels C = 256)
  forward bf16                      0.953   test_levels, levels entry with 3 maps, level 2 (the output's own rounding)
  backward fp32                     0.0114  test_backward[bins], 1x1x1 (atomic and fixed-order forms alike; the
                                            fixed-order cases at sampling_ratio 1, 2, 3 stay below it)
  backward bf16                     0.968   test_fixed_order[det_channels], C = 320 (the output's own rounding)
  backward fp32, added to a buffer  0.751   test_fixed_order_adds_to_the_buffer, many rows (the one rounding of the
                                            sum with the buffer's value, which is most of that bound)
The fp32 ratios are small because the bound is a worst case (every sample moved by the whole position bound against the
channel's steepest cell, every rounding in one direction); the mutants of test_roi_forms_cpu.py show it still separates
a kernel that loses one tap from one that does not.

Not reached, and why:
* k_roi_prepare: its bit-for-bit equality with the host chain is tests/test_boxes_gpu.py's; not duplicated.
* the dense backward under torch.use_deterministic_algorithms: it raises (tests/test_deterministic_gpu.py).
* record counts near 2^31 (roi_det_layout's refusal): the scratch alone would be tens of GB.
* maps with an axis above 65535 cells: pack_key holds 16 bits per coordinate; the grids refuse such sizes earlier.
"""
import ctypes
import json

import numpy as np
import pytest
import torch

from tests import roi_forms as Rf
from tests.roi_forms import BF16, F32

pytestmark = pytest.mark.gpu


def _scn():
    from detection_3d_amd import sparseconvnet as scn
    return scn


def _ops():
    from detection_3d_amd import roi_align_rotated_3d as ops
    return ops


def roi_last_form():
    from detection_3d_amd._lib import lib
    buf = (ctypes.c_int * len(Rf.ROI_FIELDS))()
    n = lib().d3d_roi_last_form(buf, len(Rf.ROI_FIELDS))
    assert n == len(Rf.ROI_FIELDS)
    return dict(zip(Rf.ROI_FIELDS, list(buf)))


def assert_form(tag, want, got=None):
    got = roi_last_form() if got is None else got
    assert got == want, f"{tag}: the launch form differs: " + ", ".join(
        f"{k} = {got[k]} (expected {want[k]})" for k in Rf.ROI_FIELDS if got[k] != want[k])


def to_dev(a, dev, typ=F32):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    return t.bfloat16() if typ == BF16 else t        # bf16 cases hold bf16 numbers already: no rounding here


def to_np(t):
    return t.detach().float().cpu().numpy()


_ref = Rf.cached_case


@pytest.fixture(scope="module", autouse=True)
def _own_margins():
    """the recorded ratios are this module's: another module's checks in the same process do not count"""
    Rf.MARGINS.clear()
    Rf.WORST.clear()
    yield


def _tensor(dev, case, typ, requires_grad=False):
    """the case's map as a SparseConvNetTensor; perm[i] = the case's site of the grid's row i"""
    scn = _scn()
    m = case["map"]
    t = scn.InputLayer(3, case["size"], mode=4)([torch.from_numpy(m.sites.copy()), torch.ones((m.n, 1), device=dev)])
    loc = t.get_spatial_locations().cpu().numpy()
    perm = m.find(loc[:, 3], loc[:, 0], loc[:, 1], loc[:, 2])
    assert loc.shape[0] == m.n and (perm >= 0).all()
    feats = to_dev(np.asarray(m.feats)[perm], dev, typ).requires_grad_(requires_grad)
    return scn.SparseConvNetTensor(feats, t.metadata, t.spatial_size), perm


def _tag(gname, sp, exact, typ):
    return f"{gname} / {sp['name']} {'exact' if exact else 'rounding'} {'bf16' if typ == BF16 else 'fp32'}"


def _cases(gname, typ, det=False):
    for sp in Rf.GROUPS[gname]:
        if det and sp["sr"] <= 0:
            continue
        for exact in Rf.kinds(sp):
            case, R = _ref(sp, exact, typ)
            yield sp, exact, case, R


TYPES = [F32, BF16]
SENTINEL = 7.0


# -------------------------------------------------------------------------------------------------------- forward
def _forward_both(dev, tag, case, R, typ, far=False):
    ops = _ops()
    exact, bf16 = case["exact"], typ == BF16
    K, C, bins, sr = case["K"], case["C"], case["bins"], case["sr"]
    t, _ = _tensor(dev, case, typ)
    rois = torch.from_numpy(case["rois"]).to(dev)
    index = Rf.INDEX if Rf.dense_index_taken(case["map"].extent() + (case["examples"],)) else Rf.HASH
    assert far == (index == Rf.HASH)
    roi_last_form()
    with torch.no_grad():
        got = ops.roi_align_rotated_3d_sparse(t, rois, case["scale"], *bins, sr, crop=list(case["crop"]))
    assert_form(tag + " crop", Rf.expect_roi(Rf.SPARSE, typ, K, C, bins, sr, Rf.HASH, Rf.CROP, 1))
    assert got.dtype == t.features.dtype
    Rf.check_forward(tag + " crop", to_np(got), R, exact, bf16)
    inner = torch.full((K, bins[0], bins[1], C, bins[2]), SENTINEL, dtype=t.features.dtype, device=dev)
    ops.roi_align_rotated_3d_sparse_into(inner, t, rois, case["scale"], sr, crop=None, channels_inner=True)
    assert_form(tag + " extent", Rf.expect_roi(Rf.SPARSE, typ, K, C, bins, sr, index, Rf.DEVICE, 1))
    Rf.check_forward(tag + " extent", to_np(inner.permute(0, 3, 1, 2, 4)), R, exact, bf16)


@pytest.mark.parametrize("typ", TYPES)
@pytest.mark.parametrize("gname", ["fwd_channels", "bins", "subsamples", "edges"])
def test_forward(dev, gname, typ):
    for sp, exact, case, R in _cases(gname, typ):
        _forward_both(dev, _tag(gname, sp, exact, typ), case, R, typ)


@pytest.mark.parametrize("typ", TYPES)
def test_lookup_far(dev, typ):
    for sp, exact, case, R in _cases("lookup_far", typ):
        _forward_both(dev, _tag("lookup_far", sp, exact, typ), case, R, typ, far=True)


@pytest.mark.parametrize("typ", TYPES)
@pytest.mark.parametrize("exact", [True, False])
def test_levels(dev, typ, exact):
    """four maps of strides 1, 2, 4, 8 in one metadata (a chain of size-2 stride-2 convolutions builds the grids)"""
    scn, ops = _scn(), _ops()
    bf16 = typ == BF16
    base = Rf.small_sites(np.random.RandomState(77))
    t = scn.InputLayer(3, (64, 64, 32), mode=4)([torch.from_numpy(base.copy()), torch.ones((base.shape[0], 32), device=dev)])
    down = scn.Convolution(3, 32, 32, [2, 2, 2], [2, 2, 2], False).to(dev)
    maps, refs, rois, levels = [], [], [], []
    with torch.no_grad():
        for l, sp in enumerate(Rf.LEVEL_SPECS):
            case, R = _ref(sp, exact, typ)
            loc = t.get_spatial_locations().cpu().numpy()
            perm = case["map"].find(loc[:, 3], loc[:, 0], loc[:, 1], loc[:, 2])
            assert loc.shape[0] == case["map"].n and (perm >= 0).all(), f"the sites of level {l}"
            maps.append(scn.SparseConvNetTensor(to_dev(np.asarray(case["map"].feats)[perm], dev, typ), t.metadata,
                                                t.spatial_size))
            refs.append((case, R))
            rois.append(case["rois"])
            levels += [l] * case["K"]
            if l < 3:
                t = down(t)
    C, bins, sr = refs[0][0]["C"], refs[0][0]["bins"], refs[0][0]["sr"]
    rois = np.concatenate(rois)
    levels = np.array(levels, np.int32)
    own = levels.copy()
    levels[::4] = -1                                  # padding rows
    levels[2] = 7                                     # past the last level
    K = rois.shape[0]
    r_dev, l_dev = torch.from_numpy(rois).to(dev), torch.from_numpy(levels).to(dev)
    scales = [c["scale"] for c, _ in refs]
    dt = maps[0].features.dtype

    def compare(tag, got, pooled, layout1):
        got = to_np(got.permute(0, 3, 1, 2, 4) if layout1 else got)
        at = 0
        for l, (case, R) in enumerate(refs):
            rows = np.arange(at, at + case["K"])
            at += case["K"]
            sel = levels[rows] == l if l in pooled else np.zeros(rows.size, bool)
            sub = Rf.Ref()
            sub.out, sub.mag, sub.slope, sub.pos, sub.ns = R.out[sel], R.mag[sel], R.slope[sel], R.pos[sel], R.ns[sel]
            Rf.check_forward(f"{tag} level {l}", got[rows[sel]], sub, exact, bf16)
            assert (got[rows[~sel]] == SENTINEL).all(), f"{tag}: a row of level {l} that is not pooled was written"

    for n_levels in (1, 2, 3, 4):
        for layout1 in (True, False):
            shape = (K, bins[0], bins[1], C, bins[2]) if layout1 else (K, C) + bins
            out = torch.full(shape, SENTINEL, dtype=dt, device=dev)
            roi_last_form()
            ops.roi_align_rotated_3d_sparse_levels_into(out, maps[:n_levels], r_dev, scales[:n_levels], sr, l_dev,
                                                        channels_inner=layout1)
            assert_form(f"levels {n_levels}", Rf.expect_roi(Rf.SPARSE, typ, K, C, bins, sr, Rf.INDEX, Rf.DEVICE, n_levels))
            compare(f"levels entry, {n_levels} maps, layout {int(layout1)}", out, set(range(n_levels)), layout1)
    for l in range(4):
        out = torch.full((K, C) + bins, SENTINEL, dtype=dt, device=dev)
        roi_last_form()
        ops.roi_align_rotated_3d_sparse_into(out, maps[l], r_dev, scales[l], sr, crop=None, roi_levels=l_dev, level=l,
                                             channels_inner=False)
        assert_form(f"level {l}", Rf.expect_roi(Rf.SPARSE, typ, K, C, bins, sr, Rf.INDEX, Rf.DEVICE, 1))
        compare(f"single-level entry, level {l}", out, {l}, False)
    assert (own != levels).sum() >= 8


# ------------------------------------------------------------------------------------------------------- backward
def _grad(dev, case, typ, deterministic):
    """the gradient of the feature rows through the autograd wrapper, in the case's site order, the record the
    backward's thread left, and perm (the case's site of every grid row)"""
    ops = _ops()
    t, perm = _tensor(dev, case, typ, requires_grad=True)
    rois = torch.from_numpy(case["rois"]).to(dev)
    # the record belongs to the thread that launched: autograd's worker.  A hook on the rows' gradient runs on that
    # thread right after the RoIAlign node and reads (and clears) the record there; a call that launches nothing leaves
    # the record as it is, so every backward in this file goes through here and leaves that thread's record cleared
    seen = []
    t.features.register_hook(lambda g: seen.append(roi_last_form()))
    was, was_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(deterministic)
    try:
        out = ops.roi_align_rotated_3d_sparse(t, rois, case["scale"], *case["bins"], case["sr"], crop=list(case["crop"]))
        roi_last_form()
        out.backward(to_dev(case["top"], dev, typ))
    finally:
        torch.use_deterministic_algorithms(was, warn_only=was_warn)
    g = t.features.grad
    assert g.dtype == t.features.dtype and g.shape == t.features.shape
    got = np.empty(g.shape, np.float32)
    got[perm] = to_np(g)
    return got, seen, perm


@pytest.mark.parametrize("typ", TYPES)
@pytest.mark.parametrize("gname", ["bwd_channels", "bins", "bwd_only_bins", "subsamples", "edges", "cvt_tails"])
def test_backward(dev, gname, typ):
    for sp, exact, case, R in _cases(gname, typ):
        tag = _tag(gname, sp, exact, typ)
        got, seen, _ = _grad(dev, case, typ, False)
        want = Rf.expect_roi(Rf.SPARSE_BWD, typ, case["K"], case["C"], case["bins"], case["sr"], n_rows=case["map"].n)
        assert len(seen) == 1
        assert_form(tag, want, seen[0])
        Rf.check_backward(tag, got, R, exact, typ == BF16)


@pytest.mark.parametrize("typ", TYPES)
@pytest.mark.parametrize("gname", ["det_channels", "bins", "bwd_only_bins", "subsamples", "edges", "det_lists"])
def test_fixed_order(dev, gname, typ):
    assert torch.utils.deterministic.fill_uninitialized_memory      # the bf16 gradient is written over a NaN-filled buffer
    spans, ends_on, starts_on, empty = 0, 0, 0, 0
    for sp, exact, case, R in _cases(gname, typ, det=True):
        tag = _tag(gname, sp, exact, typ) + " fixed order"
        got, seen, perm = _grad(dev, case, typ, True)
        want = Rf.expect_roi(Rf.DET, typ, case["K"], case["C"], case["bins"], case["sr"], n_rows=case["map"].n)
        assert len(seen) == 1
        assert_form(tag, want, seen[0])
        Rf.check_backward(tag, got, R, exact, typ == BF16)
        again, _, perm2 = _grad(dev, case, typ, True)
        assert Rf.same_bits(got, again) and np.array_equal(perm, perm2), f"{tag}: two runs differ"
        if exact:
            atomic, _, _ = _grad(dev, case, typ, False)
            assert Rf.same_bits(got, atomic), f"{tag}: differs from the atomic form"
        # the row lists as the device sorts them: by the grid's row number of a site
        row_of = np.empty(case["map"].n, np.int64)
        row_of[perm] = np.arange(case["map"].n)
        bt = R.btaps.copy()
        bt[:, 0] = row_of[bt[:, 0]]
        _, beg, end = Rf.record_lists(bt, case["map"].n)
        have = end > beg
        spans = max(spans, int(np.where(have, (end - 1) // Rf.DET_CHUNK - beg // Rf.DET_CHUNK + 1, 0).max(initial=0)))
        ends_on += int((have & (end % Rf.DET_CHUNK == 0)).sum())
        starts_on += int((have & (beg % Rf.DET_CHUNK == 0) & (beg > 0)).sum())
        empty += int((~have).sum())
    if gname == "det_lists":
        assert spans >= 3 and ends_on >= 1 and starts_on >= 1 and empty >= 1, (spans, ends_on, starts_on, empty)


@pytest.mark.parametrize("exact", [True, False])
def test_fixed_order_adds_to_the_buffer(dev, exact):
    """the fp32 entry point accumulates into d_feats: a non-zero buffer (small integers in the exact class)"""
    ops = _ops()
    for sp in Rf.DET_LISTS:
        if not sp["exact" if exact else "rounding"]:
            continue
        case, R = _ref(sp, exact, F32)
        t, perm = _tensor(dev, case, F32)
        rng = np.random.RandomState(5)
        base = Rf.exact_values(rng, (case["map"].n, case["C"])) if exact else Rf.rounding_values(rng, case["map"].n, case["C"], False)
        d = to_dev(base[perm], dev)
        roi_last_form()
        ops._sparse_backward_deterministic(to_dev(case["top"], dev), torch.from_numpy(case["rois"]).to(dev), t.metadata,
                                           t.spatial_size.tolist(), list(case["crop"]), case["scale"], *case["bins"],
                                           case["sr"], d)
        assert_form(sp["name"], Rf.expect_roi(Rf.DET, F32, case["K"], case["C"], case["bins"], case["sr"], n_rows=case["map"].n))
        got = np.empty(base.shape, np.float32)
        got[perm] = to_np(d)
        Rf.check_backward(sp["name"] + " into a non-zero buffer", got, R, exact, False, base=base)


def test_fixed_order_refuses_adaptive_sampling(dev):
    from detection_3d_amd._lib import D3DError
    ops = _ops()
    sp = Rf.SUBSAMPLES[4]
    assert sp["sr"] == 0
    case, _ = _ref(sp, True, F32)
    t, _ = _tensor(dev, case, F32)
    d = torch.zeros((case["map"].n, case["C"]), device=dev)
    roi_last_form()
    with pytest.raises(D3DError, match="sampling_ratio"):
        ops._sparse_backward_deterministic(to_dev(case["top"], dev), torch.from_numpy(case["rois"]).to(dev), t.metadata,
                                           t.spatial_size.tolist(), list(case["crop"]), case["scale"], *case["bins"], 0, d)
    assert roi_last_form() == dict.fromkeys(Rf.ROI_FIELDS, 0) and not bool(d.any())
    with pytest.raises(RuntimeError, match="deterministic"):          # and the wrapper, as torch's own ops do
        _grad(dev, case, F32, True)


def test_256_bins_refused(dev):
    """4 x 8 x 8 bins: the backward's tile passes the 64 KB of LDS; the library's error, and no launch"""
    from detection_3d_amd._lib import D3DError, check, ints, lib, ptr, stream_of
    bins = Rf.REFUSED_BINS
    case, _ = _ref(Rf.BINS[2], True, F32)
    t, _ = _tensor(dev, case, F32)
    K, C = case["K"], case["C"]
    rois = torch.from_numpy(case["rois"]).to(dev)
    top = torch.ones((K, C) + bins, device=dev)
    d = torch.zeros((case["map"].n, C), device=dev)
    roi_last_form()
    with pytest.raises(D3DError, match="too large"):
        check(lib().d3d_roi_align_rotated_3d_sparse_backward(
            t.metadata._h, ints(t.spatial_size.tolist()), ptr(top), C, ints(list(case["crop"])), ptr(rois), K,
            float(case["scale"]), *bins, 2, ptr(d), stream_of()))
    assert roi_last_form() == dict.fromkeys(Rf.ROI_FIELDS, 0) and not bool(d.any())
    n_rows = case["map"].n                                             # the bf16 entry has the same tile
    nbytes = int(lib().d3d_roi_align_rotated_3d_sparse_backward_bf16_scratch_bytes(C, n_rows))
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    d16 = torch.full((n_rows, C), SENTINEL, dtype=torch.bfloat16, device=dev)
    top16 = top.bfloat16()
    with pytest.raises(D3DError, match="too large"):
        check(lib().d3d_roi_align_rotated_3d_sparse_backward_bf16(
            t.metadata._h, ints(t.spatial_size.tolist()), ptr(top16), C, ints(list(case["crop"])), ptr(rois), K,
            float(case["scale"]), *bins, 2, ptr(d16), n_rows, ptr(scratch), nbytes, stream_of()))
    assert roi_last_form() == dict.fromkeys(Rf.ROI_FIELDS, 0) and bool((d16 == SENTINEL).all())
    with torch.no_grad():                                              # the forward takes them
        out = _ops().roi_align_rotated_3d_sparse(t, rois, case["scale"], *bins, 2, crop=list(case["crop"]))
    assert_form("256 bins forward", Rf.expect_roi(Rf.SPARSE, F32, K, C, bins, 2, Rf.HASH, Rf.CROP, 1))
    R = Rf.roi_ref(case["rois"], case["scale"], case["map"], case["crop"], bins, 2)
    Rf.check_forward("256 bins forward", to_np(out), R, False, False)


# ---------------------------------------------------------------------------------------------------------- dense
def test_dense(dev):
    ops = _ops()
    for sp, exact, case, R in _cases("dense", F32):
        tag = _tag("dense", sp, exact, F32)
        H, W, Z = case["crop"]
        K, C, bins, sr = case["K"], case["C"], case["bins"], case["sr"]
        dense = np.moveaxis(np.asarray(case["map"].feats, np.float32).reshape(case["examples"], H, W, Z, C), -1, 1)
        x = to_dev(dense, dev).requires_grad_(True)
        seen = []
        x.register_hook(lambda g: seen.append(roi_last_form()))
        roi_last_form()
        out = ops.roi_align_rotated_3d_forward(x, torch.from_numpy(case["rois"]).to(dev), case["scale"], *bins, sr)
        assert_form(tag, Rf.expect_roi(Rf.DENSE, F32, K, C, bins))
        Rf.check_forward(tag, to_np(out), R, exact, False)
        out.backward(to_dev(case["top"], dev))
        assert_form(tag + " backward", Rf.expect_roi(Rf.DENSE_BWD, F32, K, C, bins), seen[0])
        Rf.check_backward(tag + " backward", np.moveaxis(to_np(x.grad), 1, -1).reshape(-1, C), R, exact, False)


# --------------------------------------------------------------------------------------------------------- record
def test_read_clears_the_record(dev):
    from detection_3d_amd._lib import lib
    case, _ = _ref(Rf.BINS[2], True, F32)
    t, _ = _tensor(dev, case, F32)
    with torch.no_grad():
        _ops().roi_align_rotated_3d_sparse(t, torch.from_numpy(case["rois"]).to(dev), case["scale"], *case["bins"], 2,
                                          crop=list(case["crop"]))
    assert roi_last_form()["family"] == Rf.SPARSE
    assert roi_last_form() == dict.fromkeys(Rf.ROI_FIELDS, 0)
    assert lib().d3d_roi_last_form(None, 0) == len(Rf.ROI_FIELDS)


def test_zz_margins(dev):
    """the largest error every check saw, as a fraction of its bound (printed for DESIGN.md; sets nothing)"""
    assert Rf.MARGINS and all(0 <= v <= 1 for v in Rf.MARGINS.values())
    print("\nROI_MARGINS " + json.dumps({k: [round(v, 4), Rf.WORST[k]] for k, v in sorted(Rf.MARGINS.items())}))
