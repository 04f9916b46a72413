"""The references and cases of tests/tail_forms.py without a GPU: the launch forms the head cases reach, the exactness
headroom and the sharpness of the rounding bound of every head case, the packing against detector.py's, the bf16
rounding against torch's, the decode cases against the oracle, the selection reference against its torch spelling, the
radix pass every pass case decides in, and the argument checks of the head entries that return before a launch."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from tests import tail_forms as F

RPN = F.rpn_cases()
MLP = F.mlp_cases()
SEL = F.select_cases()


# ------------------------------------------------------------------------------------------------------------- forms
def test_cases_reach_every_form():
    got = {(C // 32, F.slices(C, a)) for C, a, _ in RPN} | {(C // 32, F.slices(C, a)) for C, a, _, _ in MLP}
    assert got == set(F.all_ws())
    assert set(F.all_ws()) == {(4, 1), (4, 2), (4, 4), (8, 1), (8, 2), (8, 4), (8, 8), (16, 1), (16, 2), (16, 4), (16, 8)}
    named = {128: (1, 2, 3, 4), 256: (1, 2, 3, 5, 8), 512: (1, 2, 3, 5, 9, 16)}
    for cases in (RPN, [(C, a, None) for C, a, _, _ in MLP]):
        for C, tiles in named.items():
            mine = {F.out_tiles(a) for c, a, _ in cases if c == C}
            if C == 512 and cases is RPN:
                assert not mine
                continue
            assert set(tiles) <= mine, (C, mine)
            # every (out_tiles, S) of this channel count that has its own S
            assert {s for _, s in F.all_forms(C)} == {F.slices(C, a) for c, a, _ in cases if c == C}
            assert any(8 * a == C for c, a, _ in cases if c == C)                     # the gate
            assert any(8 * a % 32 for c, a, _ in cases if c == C)
    assert {1, 3, 5, 13} <= {a for _, a, _ in RPN} | {a for _, a, _, _ in MLP}
    # the C entry's own check (out_tiles <= C / 32) admits exactly 8a <= C: nothing wider than the Python gate
    for C in (128, 256, 512):
        assert all((F.out_tiles(a) <= C // 32) == (8 * a <= C) for a in range(1, C))


def test_layouts():
    totals = {sum(l) for l in F.LAYOUTS}
    assert {0, 1, 31, 32, 33, 65} <= totals
    assert {len(l) for l in F.LAYOUTS} >= {1, 2, 6}
    starts = [np.cumsum(l)[:-1] for l in F.LAYOUTS if sum(l)]
    assert any((s % 32 != 0).any() for s in starts) and any(((s % 32 == 0) & (s > 0)).any() for s in starts)
    live = [l for l in F.LAYOUTS if sum(l)]
    assert any(l[0] == 0 for l in live) and any(l[-1] == 0 for l in live)
    assert any(0 in l[1:-1] for l in live)
    for C in (128, 256):
        assert {rows for c, _, rows in RPN if c == C} == {tuple(l) for l in F.LAYOUTS}
    assert {n for _, _, n, _ in MLP} == set(F.MLP_ROWS)
    assert {(C, r) for C, _, _, r in MLP} == {(C, r) for C in (128, 256, 512) for r in (0, 1)}


def _head_variants():
    for C, a, rows in RPN:
        if sum(rows):
            yield ("rpn", C, a, sum(rows), 0, False)
            yield ("rpn_bf16", C, a, sum(rows), 0, True)
    for C, a, n, relu_in in MLP:
        yield ("mlp", C, a, n, relu_in, False)


VARIANTS = sorted(set(_head_variants()))


@pytest.mark.parametrize("C", [128, 256, 512])
def test_exact_data_is_exact_in_fp32(C):
    rounded = 0
    for entry, c, a, n, relu_in, bf16 in VARIANTS:
        if c != C:
            continue
        d = F.head_data(C, a, n, True, seed=a + n)
        for k in ("x", "w1", "b1", "w2", "b2"):
            assert (d[k] == np.round(d[k])).all() and (np.abs(d[k]) <= 8).all()
            if bf16:
                assert np.array_equal(F.bf16_round(d[k]), d[k])
        assert (d["w1"] != 0).all() and (d["w2"] != 0).all() and (d["b1"] != 0).all() and (d["b2"] != 0).all()
        assert F.exact_headroom(d, relu_in, bf16) < 2 ** 24, (entry, C, a, n)
        t, out = F.head_reference(d, relu_in, bf16)
        assert np.array_equal(t.astype(np.float32).astype(np.float64), t)
        assert np.array_equal(out.astype(np.float32).astype(np.float64), out)
        if entry == "mlp":                                  # stage 2 launched apart: the rows are t
            d2 = dict(d, x=t.astype(np.float32))
            assert F.exact_headroom(d2, False, False, 2) < 2 ** 24
        if bf16:
            rounded += int((F.head_reference(d, relu_in, False)[0] != t).sum())
    if C < 512:
        assert rounded > 0                                  # the bf16 rounding of t does something in the exact cases


@pytest.mark.parametrize("C", [128, 256, 512])
def test_rounding_bound_fails_without_the_largest_product(C):
    """in every element of every case: removing the largest term of the element's reference sum moves it by more than
    the bound (so does any error of that size: a dropped product, a wrong operand)"""
    for entry, c, a, n, relu_in, bf16 in VARIANTS:
        if c != C:
            continue
        d = F.head_data(C, a, n, False, seed=a + n, bf16=bf16)
        bt, bo = F.rounding_bound(d, C, a, relu_in, bf16)
        p1, p2 = F.largest_products(d, relu_in, bf16)
        assert (p2 > bo).all(), (entry, C, a, n, float((p2 / bo).min()))
        if entry == "mlp":
            live = p1 > 0                                   # (relu_in can zero a whole row's terms: never here)
            assert live.all() and (p1 > bt).all(), (entry, C, a, n)
            t, _ = F.head_reference(d, relu_in, False)
            d2 = dict(d, x=t.astype(np.float32))
            _, bo2 = F.rounding_bound(d2, C, a, False, False, 2)
            assert (F.largest_products(d2, False, False, 2)[1] > bo2).all()


def test_bf16_rounding_is_torchs():
    rng = np.random.RandomState(0)
    x = np.concatenate([rng.randn(4000).astype(np.float32) * 100, np.arange(0, 5000, dtype=np.float32),
                        np.array([0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001, 0x7f7fffff, 0x00000001, 0x80000000,
                                  0x7f800000, 0xff800000], np.uint32).view(np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(F.bf16_bits(x), want)
    assert np.isnan(F.bf16_round(np.array([np.nan], np.float32))).all()


def test_packing_is_the_detectors():
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.detector import RPNHead, _pack_linear
    rng = np.random.RandomState(1)
    for C, cout in ((128, 8), (128, 104), (256, 256), (512, 40), (512, 512)):
        w = rng.randn(cout, C).astype(np.float32)
        mine = F.pack_f32(w)
        assert mine.shape == (C // 4, (cout + 31) // 32 * 32, 4)
        assert np.array_equal(mine, _pack_linear(torch.from_numpy(w)).numpy())
        assert (mine[:, cout:, :] == 0).all()               # padding columns
        g, co, j = 3, cout - 1, 2
        assert mine[g, co, j] == w[co, 4 * g + j]
    for C, a in ((128, 5), (256, 32)):
        head = RPNHead(get_cfg("4c_Fpn432"), C, a).eval()
        with torch.no_grad():
            for p in head.parameters():
                p.copy_(torch.randn_like(p))
        w1 = head.conv.weight.detach().view(C, C).numpy()
        w2 = torch.cat([head.cls_logits.weight.detach().view(-1, C), head.bbox_pred.weight.detach().view(-1, C)]).numpy()
        b2 = torch.cat([head.cls_logits.bias.detach(), head.bbox_pred.bias.detach()]).numpy()
        assert head.num_anchors_per_location * head.seperate_rpn == a
        p1, pb1, p2, pb2 = head._packed(torch.float32)
        assert np.array_equal(p1.numpy(), F.pack_f32(w1)) and np.array_equal(p2.numpy(), F.pack_f32(w2))
        assert np.array_equal(pb2.numpy(), b2) and np.array_equal(pb1.numpy(), head.conv.bias.detach().numpy())
        q1, _, q2, _ = head._packed(torch.bfloat16)
        assert np.array_equal(q1.view(torch.int16).numpy().view(np.uint16), F.pack_bf16(w1))
        assert np.array_equal(q2.view(torch.int16).numpy().view(np.uint16), F.pack_bf16(w2))
        assert (F.pack_bf16(w2)[:, 8 * a:, :] == 0).all()
        assert F.pack_bf16(w2)[2, 8 * a - 1, 5] == F.bf16_bits(w2)[8 * a - 1, 8 * 2 + 5]


# -------------------------------------------------------------------------------------------------- argument checks
@pytest.fixture(scope="module")
def lib():
    from detection_3d_amd import _lib
    from detection_3d_amd.build import build_library
    build_library()
    return _lib.lib()


def _err(rc):
    from detection_3d_amd import _lib
    assert rc != 0
    return _lib.lib().d3d_last_error().decode()


def test_head_entries_refuse_bad_arguments(lib):
    """checks that return before anything touches a device (beside those of test_bf16_heads_cpu.py)"""
    vp = ctypes.c_void_p
    d = vp(4096)
    rows1, maps1 = (ctypes.c_int * 1)(64), (vp * 1)(d)
    rows7, maps7 = (ctypes.c_int * 7)(*([8] * 7)), (vp * 7)(*([d] * 7))
    for fn in (lib.d3d_rpn_head, lib.d3d_rpn_head_bf16):
        assert "channels" in _err(fn(maps1, rows1, 1, 192, d, d, d, d, 4, d, d, None))
        assert "maps" in _err(fn(maps1, rows1, 0, 128, d, d, d, d, 4, d, d, None))
        assert "maps" in _err(fn(maps7, rows7, 7, 128, d, d, d, d, 4, d, d, None))
        assert "bad arguments" in _err(fn(maps1, rows1, 1, 128, d, d, d, d, 0, d, d, None))
        assert "output columns" in _err(fn(maps1, rows1, 1, 128, d, d, d, d, 17, d, d, None))
        assert "output columns" in _err(fn(maps1, rows1, 1, 256, d, d, d, d, 33, d, d, None))
        assert "map 0" in _err(fn((vp * 1)(None), rows1, 1, 128, d, d, d, d, 4, d, d, None))
        assert "map 0" in _err(fn(maps1, (ctypes.c_int * 1)(-1), 1, 128, d, d, d, d, 4, d, d, None))
    m = lib.d3d_mlp_heads
    assert "channels" in _err(m(d, 64, 192, 0, d, d, d, d, d, 4, d, d, None))
    assert "channels" in _err(m(d, -1, 128, 0, d, d, d, d, d, 4, d, d, None))
    assert "rectified" in _err(m(d, 64, 128, 1, None, None, None, d, d, 4, d, d, None))       # relu_in without stage 1
    assert "bad arguments" in _err(m(d, 64, 128, 0, d, d, None, None, None, 0, None, None, None))   # stage 1, no t_out
    assert "bad arguments" in _err(m(d, 64, 128, 0, None, None, None, None, None, 0, None, None, None))   # no stage
    assert "bad arguments" in _err(m(d, 64, 128, 0, d, None, d, None, None, 0, None, None, None))         # no b1
    assert "bad arguments" in _err(m(d, 64, 128, 0, d, d, d, d, d, 0, d, d, None))                          # a = 0
    assert "bad arguments" in _err(m(d, 64, 128, 0, d, d, d, d, d, 4, None, d, None))                       # no output
    assert "null input" in _err(m(None, 64, 128, 0, d, d, d, d, d, 4, d, d, None))
    assert "output columns" in _err(m(d, 64, 128, 0, d, d, d, d, d, 17, d, d, None))
    assert "output columns" in _err(m(d, 64, 512, 0, d, d, d, d, d, 65, d, d, None))
    # nothing to do: no rows (no launch, no device)
    assert m(None, 0, 128, 0, d, d, d, d, d, 4, d, d, None) == 0
    assert lib.d3d_rpn_head(maps1, (ctypes.c_int * 1)(0), 1, 128, d, d, d, d, 4, d, d, None) == 0
    assert lib.d3d_rpn_head_bf16(maps1, (ctypes.c_int * 1)(0), 1, 128, d, d, d, d, 4, None, None, None) == 0


# --------------------------------------------------------------------------------------------------------- box decode
def _nan_equal_bits(a, b):
    return ((F.bits(a) == F.bits(b)) | (np.isnan(a) & np.isnan(b))).all()


@pytest.mark.parametrize("clip", F.CLIPS)
@pytest.mark.parametrize("weights", F.WEIGHTS)
def test_nonfinite_decode_cases_on_the_oracle(clip, weights):
    enc, anchors, expect = F.nonfinite_cases()
    out = oracle.box_decode(enc * np.array(weights, np.float32), anchors, weights, clip)
    assert np.array_equal(~np.isfinite(out), expect)
    clean_e, clean_a = F.decode_rows(enc.shape[0], 11)
    clean = oracle.box_decode(clean_e * np.array(weights, np.float32), clean_a, weights, clip)
    touched = expect.copy()
    touched[:, 3:6] |= np.isposinf(enc[:, 3:6])
    assert np.array_equal(F.bits(out)[~touched], F.bits(clean)[~touched])
    # a NaN size delta stays a NaN (torch.clamp(max=)), a +inf one is the clip
    rows = np.nonzero(np.isnan(enc[:, 3:6]).any(1))[0]
    assert rows.size == 3 and np.isnan(out[rows, 3 + np.arange(3)]).all()
    rows = np.nonzero(np.isposinf(enc[:, 3:6]).any(1))[0]
    got = out[rows, 3 + np.arange(3)]
    assert np.array_equal(got, (np.float32(clip) + np.float32(1)) * anchors[rows, 3 + np.arange(3)])
    t = torch.clamp(torch.from_numpy(enc[:, 3:6]), max=clip).numpy()
    assert np.array_equal(np.isnan(t), np.isnan(enc[:, 3:6]))


@pytest.mark.parametrize("clip", F.CLIPS)
@pytest.mark.parametrize("weights", F.WEIGHTS[::2])
def test_clip_cases_sit_on_the_clip(clip, weights):
    enc, anchors, vals = F.clip_cases(clip, weights)
    c = np.float32(clip)
    assert vals[0] < c == vals[1] < vals[2] and np.nextafter(vals[0], vals[2]) == c == np.nextafter(vals[2], vals[0])
    slot = 3 + np.arange(9) // 3
    t = enc[np.arange(9), slot] / np.array(weights, np.float32)[slot]
    assert np.array_equal(t, vals)                                    # the division gives the designed value back
    out = oracle.box_decode(enc, anchors, weights, clip)
    assert np.array_equal(out[np.arange(9), slot], (np.minimum(vals, c) + np.float32(1)) * anchors[np.arange(9), slot])


def test_yaw_cases_sit_on_the_wrap():
    enc, anchors, target = F.yaw_cases()
    n = target.shape[0]
    assert np.array_equal((enc[:n, 6] + anchors[:n, 6]).astype(np.float32), target)
    half = F.PI32 / np.float32(2)
    assert np.array_equal(target[:9] / half, np.round(target[:9] / half)) and (np.round(target[:9] / half) % 2 == 1).all()
    out = oracle.box_decode(enc, anchors)
    assert np.isfinite(out).all() and (np.abs(out[:, 6]) <= 1.5708 + 0.07).all()     # 1e6: an fp32 ulp is 1/16
    assert (np.abs(enc[n:, 6]) >= 1e6).all()


def test_box_reg_weights_of_the_configs_are_covered():
    from detection_3d_amd.config import get_cfg
    for name in ("4c_Fpn432", "3G6c_Fpn4321"):
        assert tuple(float(w) for w in get_cfg(name).MODEL.ROI_HEADS.BBOX_REG_WEIGHTS) in F.WEIGHTS


# ----------------------------------------------------------------------------------------------------------- selection
def _torch_select(c):
    """the tensor ending of PostProcessor.forward on the same keep / n_keep / prob"""
    keep, nk, n_max, nc, D = torch.from_numpy(c["keep"]), torch.from_numpy(c["nk"]), c["n_max"], c["nc"], c["D"]
    prob, boxes = torch.from_numpy(c["prob"]), torch.from_numpy(c["boxes"])
    valid = (torch.arange(n_max).view(1, -1) < nk.view(-1, 1)).view(-1)
    flat_all = torch.where(valid, keep.view(-1), torch.zeros_like(keep.view(-1))).long()
    s_all = torch.where(valid, prob[flat_all], prob.new_full((), -1.0))
    if 0 < D < s_all.shape[0]:
        thresh = torch.sort(s_all, descending=True)[0][D - 1]
        sel = s_all >= thresh.clamp_min(0.0)
    else:
        sel = s_all >= 0.0
    flat = flat_all[sel]
    return boxes[flat].numpy(), prob[flat].numpy(), (flat % nc).numpy(), flat_all.numpy(), s_all.numpy()


@pytest.mark.parametrize("c", SEL, ids=[c["name"] for c in SEL])
def test_select_reference_is_the_tensor_ending(c):
    b, s, l = F.select_reference(c["keep"], c["nk"], c["n_max"], c["prob"], c["boxes"], c["nc"], c["D"])
    tb, ts, tl, tflat, tsall = _torch_select(c)
    assert np.array_equal(F.bits(b), F.bits(tb)) and np.array_equal(F.bits(s), F.bits(ts)) and np.array_equal(l, tl)
    flat, s_all = F.candidates(c["keep"], c["nk"], c["n_max"], c["prob"])
    assert np.array_equal(flat, tflat) and np.array_equal(F.bits(s_all), F.bits(tsall))
    assert not np.isnan(s).any()                                          # a NaN is never selected
    # ... and the key order is the float order, NaN on top, the zeros equal
    fin = s_all[~np.isnan(s_all)]
    o = np.argsort(fin, kind="stable")
    assert (np.diff(F.f32_key(fin[o]).astype(np.int64)) >= 0).all()
    assert ((np.diff(F.f32_key(fin[o]).astype(np.int64)) == 0) == (fin[o][1:] == fin[o][:-1])).all()


def test_selection_cases_are_what_their_names_say():
    by = F.cases_by_name()
    sizes = {c["nseg"] * c["n_max"] for c in SEL}
    assert {1, 1023, 1024, 1025, 2049, 8192} <= sizes
    for N in (1, 1023, 1024, 1025, 2049, 8192):
        assert {0, 1, N - 1, N, N + 1} <= {c["D"] for c in SEL if c["nseg"] * c["n_max"] == N}
    for p in (1, 2, 3, 4):
        for name in (f"pass{p}", f"pass{p}_segments"):
            c = by[name]
            _, s = F.candidates(c["keep"], c["nk"], c["n_max"], c["prob"])
            assert F.decided_pass(s, c["D"]) == p, name
            if p > 1:
                assert F.decided_pass(s, c["D"]) > F.decided_pass(s[:1], 1)
            k = F.f32_key(s)
            kd = np.sort(k)[::-1][c["D"] - 1]
            assert (k == kd).sum() > 1                                    # ties on the threshold
    c = by["bin0_pass1_neg_inf"]
    _, s = F.candidates(c["keep"], c["nk"], c["n_max"], c["prob"])
    assert F.dth_bin(s, c["D"], 1) == 0 and F.dth_largest(s, c["D"]) == -np.inf
    c = by["bin0_zero"]
    _, s = F.candidates(c["keep"], c["nk"], c["n_max"], c["prob"])
    assert [F.dth_bin(s, c["D"], p) for p in (2, 3, 4)] == [0, 0, 0] and F.dth_largest(s, c["D"]) == 0
    c = by["few_survivors"]
    _, s = F.candidates(c["keep"], c["nk"], c["n_max"], c["prob"])
    assert F.dth_largest(s, c["D"]) == -1 and len(F.select_reference(*[c[k] for k in ("keep", "nk", "n_max", "prob", "boxes", "nc", "D")])[1]) == 50
    c = by["all_equal"]
    assert len(F.select_reference(*[c[k] for k in ("keep", "nk", "n_max", "prob", "boxes", "nc", "D")])[1]) == 1400 > c["D"]
    sel = lambda name: F.select_reference(*[by[name][k] for k in ("keep", "nk", "n_max", "prob", "boxes", "nc", "D")])[1]
    assert np.signbit(sel("zeros_all_stay")[sel("zeros_all_stay") == 0]).any()             # -0.0 stays
    assert np.signbit(sel("zeros_D_above_positive")[sel("zeros_D_above_positive") == 0]).any()
    assert (sel("negative_scores_D0") >= 0).all() and len(sel("negative_scores_D0")) < 400
    assert len(sel("nan_is_dth")) == 0 and len(sel("nan_is_first")) == 0 and len(sel("nan_all")) == 0
    assert len(sel("nan_below_D")) == 20
    q = by["nan_D0"]["prob"]
    assert (np.isnan(q) & np.signbit(q)).any() and (np.isnan(q) & ~np.signbit(q)).any()
    assert {c["nc"] for c in SEL} >= {2, 9}


@pytest.mark.parametrize("K", [0, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("nc", [2, 5])
def test_post_scores_and_order_references(K, nc):
    prob, thresh = F.post_scores_case(K, nc)
    sc, counts = F.post_scores_reference(prob, thresh)
    p = torch.from_numpy(prob)
    cand = p[:, 1:].t() > thresh
    want = torch.where(cand, p[:, 1:].t(), p.new_full((), -1.0))
    assert np.array_equal(F.bits(sc), F.bits(want.numpy())) and np.array_equal(counts, cand.sum(1).numpy())
    if K >= 63:
        assert (prob[:, 1:] == np.float32(thresh)).any() and np.isnan(prob[:, 1:]).any()
        assert (sc[(prob[:, 1:] == np.float32(thresh)).T] == -1).all()
    idx = torch.sort(want, dim=1, descending=True, stable=True)[1]
    order = F.post_order_reference(idx.numpy(), nc)
    assert np.array_equal(order, (idx * nc + torch.arange(1, nc).view(-1, 1)).to(torch.int32).numpy())


def test_gather_kept_reference_is_torch_clamp():
    rng = np.random.RandomState(2)
    boxes = rng.randn(40, 7).astype(np.float32)
    boxes[3, 3], boxes[5, 4], boxes[7, 5] = np.nan, -0.0, -np.inf
    scores = rng.rand(40).astype(np.float32)
    keep = rng.permutation(40).astype(np.int32)
    for min_size in (0.0, 0.001, 0.3):
        b, s = F.gather_kept_reference(boxes, scores, keep, 25, 32, min_size)
        want = torch.from_numpy(boxes[np.where(np.arange(32) < 25, keep[:32], 0)])
        want[:, 3:6] = torch.clamp(want[:, 3:6], min=min_size)
        assert np.array_equal(b, want.numpy(), equal_nan=True)            # (numerically: -0.0 == 0.0)
        assert np.array_equal(np.isnan(b), np.isnan(want.numpy()))
        assert (b[25:] == b[25]).all() and np.array_equal(s[25:], np.full(7, scores[0]))
