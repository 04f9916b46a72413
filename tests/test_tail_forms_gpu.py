"""Every launch form of the detector tail against exact results: the RPN / box-head kernel (csrc/rpn_head.hip), the box
decode (box_decode_one of d3d_internal.h behind k_box_decode and d3d_topk_segments) and the final selection and gathers
(csrc/box_tail.hip from k_post_scores down).  tests/tail_forms.py holds the references and the designed cases,
tests/test_tail_forms_cpu.py checks them without a GPU.

The C entries are called through ctypes as they are, with operands packed by tail_forms (the Python packing is compared
with it on the CPU and run in the *_module tests).  Every output is prefilled with NaN (integers: a sentinel) in a
buffer a few rows longer than needed, and the rows past the end must still hold it.  Heads: every case runs on exact
data (small dense integers: fp32 outputs and t equal the fp64 reference bit for bit, the bf16 head after rounding t once
as st1(unsigned short *, float) does) and on rounding data (|got - ref| <= the per-element bound of
tail_forms.rounding_bound).  Decode and selection: bit for bit (where both sides hold a NaN, whatever its bits).

  form                                   reached by
  k_rpn_head<128, false>, entry rpn      test_rpn_head[128-*-f32]: a = 1, 4, 5, 8, 12, 13, 16 (out_tiles 1, 1, 2, 2, 3, 4,
                                         4; S = 4, 4, 2, 2, 1, 1, 1; 8a = C at a = 16, the widest a the entry takes)
  k_rpn_head<256, false>, entry rpn      test_rpn_head[256-*-f32]: a = 1, 3, 8, 12, 17, 32 (out_tiles 1, 1, 2, 3, 5, 8;
                                         S = 8, 8, 4, 2, 1, 1; 8a = C at a = 32)
  k_rpn_head_bf16<128>, <256>            test_rpn_head[*-bf16]: the same a
  map layouts (both entries, both C)     test_rpn_head[*-rows*]: 1, 2, 6 maps; totals 1, 31, 32, 33, 65; a boundary inside
                                         a block (20 | 13) and on a block edge (32 | 33); an empty map first, in the
                                         middle, last (null pointers); test_rpn_head_nothing_to_do: [0], [0, 0, 0]
  k_rpn_head<C, relu_in> for C = 128,    test_mlp_heads[*]: each case fused with t_out, fused without, stage 1 alone,
  256, 512, relu_in 0 / 1; stages 1,     stage 2 alone on the t of stage 1 (the same bits as fused); a = 1 .. 64: at 512
  2, 3; t_out null or not                out_tiles 1, 2, 2, 3, 5, 9, 16 with S = 8, 8, 8, 4, 2, 1, 1; rows 1, 31, 32, 33, 65
  locality                               test_rpn_head_locality, test_mlp_heads_locality: a NaN row, a row of +-inf
                                         (relu_in: a NaN goes through the input relu), every other row the same bits
  Python packing                         test_rpn_head_module[f32 / bf16] (RPNHead._packed), test_mlp_heads_module
                                         (_pack_linear through _fc7_and_heads and FPNPredictor.forward)
  d3d_box_decode, _rows, _classes        test_decode_nonfinite[*] (NaN, +inf, -inf in each of the 7 encoding and 7 anchor
                                         slots, which outputs stop being finite), test_decode_clip[*] (the clip, one ulp
                                         below, one above; log(1000) and 10000), test_decode_weights, test_decode_yaw,
                                         test_decode_sizes[1, 255, 256, 257], test_decode_rows_orders,
                                         test_decode_classes[2, 5, 9]
  decode fused into d3d_topk_segments    test_decode_fused_in_topk (a NaN regression row among the selected)
  d3d_post_select                        test_post_select[*]: N = 1, 1023, 1024, 1025, 2049, 8192 (1, 2, 8 candidates per
                                         thread, a short last range), D = 0, 1, N - 1, N, N + 1, 200 and above the
                                         survivors, pass1 .. pass4, bin0_*, all_equal*, nk_*, nc2 / nc9, zeros_*,
                                         negative_*, nan_*; out_n in device memory and in a pinned host word
  d3d_post_gather                        test_post_select[*] (the same inputs)
  d3d_post_scores, d3d_post_order        test_post_scores_and_order[K = 0, 1, 63, 64, 65, 257; nc = 2, 5]: prob == thresh,
                                         NaN, counts into a dirty buffer, twice
  d3d_gather_kept                        test_gather_kept[*]: n_keep 0, P, above P; min_size 0 and 0.001 against NaN and
                                         -0.0 sizes; count_out null and pinned
  PostProcessor.forward, both endings    test_post_processor_endings_agree (the cap and d3d_topk_max forced by
                                         monkeypatch, each and both)

Cost: the module's 255 tests take 4.4 s on an MI355X; the largest launch is one workgroup of 8192 candidates or 65 rows.

Fixes these tests asked for.  box_decode_one clamped the size deltas with fminf, which turns a NaN delta into the clip
(a finite box 10001 times the anchor): with fminf restored 11 tests fail, test_decode_nonfinite[*] (all 6),
test_decode_classes[2, 5, 9], test_decode_rows_orders and test_decode_fused_in_topk, nothing else.  k_post_select
compared keys that put -0.0 below 0.0 and a positive NaN above +inf: with the old keys 12 tests fail,
test_post_select[zeros_all_stay, zeros_D_above_positive, zeros_padding_thresh, negative_scores_D0,
negative_scores_thresh, nan_D0, nan_below_D, nan_is_dth, nan_is_first, nan_D_N, nan_all, nan_and_inf], nothing else.

Mutants (arithmetic only, built apart, the module run once with each, not kept):
  stage 2 adds slices 1 .. S - 1 only    the 56 test_rpn_head and 28 test_mlp_heads cases with S > 1, test_rpn_head_module
                                         [f32, bf16] and test_mlp_heads_module fail; every S = 1 case passes
  `h ^ 1` in tile_product's weight       all 66 test_rpn_head and 35 test_mlp_heads cases and the three module tests
  address (both types)                   fail
  b2 not added                           the same 104 tests fail
  fminf / the old keys                   above
(the locality and nothing-to-do tests compare two runs of the same library with each other and pass under all of them)

Not reached: a stream other than the current one; rows near the 2^31 / 7a limit of the head entries (the argument
check alone, no launch); more than 65 rows per head case (test_bf16_heads_gpu.py and the detector tests run thousands);
-0.0 class probabilities through PostProcessor.forward (a softmax gives none; d3d_post_select sees them in
test_post_select) and NaN ones past the candidate lists (NaN rows are no candidates: test_post_processor_endings_agree
[299-5-30]; the kernels see NaN scores in test_post_select and test_post_scores_and_order); n_max above d3d_topk_max() for real (the branch is forced instead);
d3d_rpn_head with a wider than C / 8: the entry's own check admits exactly 8a <= C, the same set as the Python gate."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from tests import tail_forms as F

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAD = 3                      # rows allocated past the end of every output
SENT_I = -7


def _lib():
    from detection_3d_amd._lib import lib
    return lib()


def _call(rc):
    from detection_3d_amd._lib import check
    check(rc)
    torch.cuda.synchronize()


def P(t):
    from detection_3d_amd._lib import ptr
    return ptr(t)


def S():
    from detection_3d_amd._lib import stream_of
    return stream_of()


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _untouched(buf, used):
    tail = buf.reshape(-1)[used:]
    return bool(torch.isnan(tail).all()) if tail.is_floating_point() else bool((tail == SENT_I).all())


def same(a, b):
    """bit for bit, or a NaN on both sides"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(((F.bits(a) == F.bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ----------------------------------------------------------------------------------------------------------------------
# heads
def run_rpn(dev, d, rows, C, a, bf16):
    """d3d_rpn_head / d3d_rpn_head_bf16 over the maps `rows` of d["x"] -> obj [n, a], reg [n, 7a] (numpy)"""
    L = _lib()
    n = sum(rows)
    x = T(d["x"], dev)
    if bf16:
        x = x.to(torch.bfloat16)
        assert np.array_equal(x.float().cpu().numpy(), d["x"], equal_nan=True)
    parts = [x[s:s + r].clone() if r else None for s, r in zip(np.cumsum((0,) + tuple(rows[:-1])), rows)]
    if bf16:
        w1, w2 = T(F.pack_bf16(d["w1"]).view(np.int16), dev), T(F.pack_bf16(d["w2"]).view(np.int16), dev)
    else:
        w1, w2 = T(F.pack_f32(d["w1"]), dev), T(F.pack_f32(d["w2"]), dev)
    b1, b2 = T(d["b1"], dev), T(d["b2"], dev)
    obj = torch.full(((n + PAD) * a,), NAN, dtype=torch.float32, device=dev)
    reg = torch.full(((n + PAD) * 7 * a,), NAN, dtype=torch.float32, device=dev)
    maps = (ctypes.c_void_p * len(rows))(*[None if p is None else p.data_ptr() for p in parts])
    rws = (ctypes.c_int * len(rows))(*rows)
    fn = L.d3d_rpn_head_bf16 if bf16 else L.d3d_rpn_head
    _call(fn(maps, rws, len(rows), C, P(w1), P(b1), P(w2), P(b2), a, P(obj), P(reg), S()))
    assert _untouched(obj, n * a) and _untouched(reg, n * 7 * a), "written past the last row"
    return obj[:n * a].view(n, a).cpu().numpy(), reg[:n * 7 * a].view(n, 7 * a).cpu().numpy()


def run_mlp(dev, x, C, relu_in, d, a, stage1, stage2, want_t):
    """d3d_mlp_heads -> (t or None, out_a or None, out_7a or None)"""
    L = _lib()
    n = x.shape[0]
    xt = T(x, dev)
    w1, b1 = (T(F.pack_f32(d["w1"]), dev), T(d["b1"], dev)) if stage1 else (None, None)
    w2, b2 = (T(F.pack_f32(d["w2"]), dev), T(d["b2"], dev)) if stage2 else (None, None)
    t = torch.full(((n + PAD) * C,), NAN, dtype=torch.float32, device=dev) if want_t else None
    oa = torch.full(((n + PAD) * a,), NAN, dtype=torch.float32, device=dev) if stage2 else None
    o7 = torch.full(((n + PAD) * 7 * a,), NAN, dtype=torch.float32, device=dev) if stage2 else None
    _call(L.d3d_mlp_heads(P(xt), n, C, int(relu_in), P(w1), P(b1), P(t), P(w2), P(b2), a if stage2 else 0, P(oa), P(o7),
                          S()))
    for buf, used in ((t, n * C), (oa, n * a), (o7, n * 7 * a)):
        assert buf is None or _untouched(buf, used), "written past the last row"
    return (None if t is None else t[:n * C].view(n, C).cpu().numpy(),
            None if oa is None else oa[:n * a].view(n, a).cpu().numpy(),
            None if o7 is None else o7[:n * 7 * a].view(n, 7 * a).cpu().numpy())


def check_exact(tag, got, want):
    w = want.astype(np.float32)
    assert np.array_equal(w.astype(np.float64), want)
    bad = np.argwhere(F.bits(got) != F.bits(w))
    assert bad.size == 0, (tag, "exact", len(bad), "first", tuple(bad[0]), float(got[tuple(bad[0])]), float(w[tuple(bad[0])]))


def check_bound(tag, got, want, bound):
    err = np.abs(got.astype(np.float64) - want)
    bad = np.argwhere(~(err <= bound))
    assert bad.size == 0, (tag, "rounding", len(bad), "first", tuple(bad[0]), float(err[tuple(bad[0])]),
                           float(bound[tuple(bad[0])]))


RPN_IDS = [f"{C}-a{a}-rows{'_'.join(map(str, rows))}" for C, a, rows in F.rpn_cases()]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", [c for c in F.rpn_cases() if sum(c[2])], ids=[i for i, c in zip(RPN_IDS, F.rpn_cases()) if sum(c[2])])
def test_rpn_head(dev, case, dtype):
    C, a, rows = case
    bf16, n = dtype == "bf16", sum(rows)
    for exact in (True, False):
        d = F.head_data(C, a, n, exact, seed=a + n, bf16=bf16)
        obj, reg = run_rpn(dev, d, rows, C, a, bf16)
        _, want = F.head_reference(d, False, bf16)
        got = np.concatenate([obj, reg], 1)
        if exact:
            check_exact((C, a, rows, dtype), got, want)
        else:
            check_bound((C, a, rows, dtype), got, want, F.rounding_bound(d, C, a, False, bf16)[1])


def test_rpn_head_nothing_to_do(dev):
    """every map empty (null pointers): no launch, the outputs keep what they held"""
    L = _lib()
    d = F.head_data(128, 4, 1, True, seed=1)
    w1, w2, b1, b2 = T(F.pack_f32(d["w1"]), dev), T(F.pack_f32(d["w2"]), dev), T(d["b1"], dev), T(d["b2"], dev)
    q1, q2 = T(F.pack_bf16(d["w1"]).view(np.int16), dev), T(F.pack_bf16(d["w2"]).view(np.int16), dev)
    for rows in ((0,), (0, 0, 0)):
        for fn, u1, u2 in ((L.d3d_rpn_head, w1, w2), (L.d3d_rpn_head_bf16, q1, q2)):
            obj = torch.full((64,), NAN, device=dev)
            reg = torch.full((64 * 7,), NAN, device=dev)
            maps = (ctypes.c_void_p * len(rows))(*([None] * len(rows)))
            _call(fn(maps, (ctypes.c_int * len(rows))(*rows), len(rows), 128, P(u1), P(b1), P(u2), P(b2), 4, P(obj), P(reg), S()))
            assert _untouched(obj, 0) and _untouched(reg, 0)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("C,a", [(128, 4), (256, 17)])
def test_rpn_head_locality(dev, C, a, dtype):
    """a NaN row and a row of +-inf (one in a block of its own rows, one across a map boundary): the other rows keep
    their bits"""
    bf16, rows = dtype == "bf16", (20, 13, 32)
    d = F.head_data(C, a, 65, True, seed=5, bf16=bf16)
    base = np.concatenate(run_rpn(dev, d, rows, C, a, bf16), 1)
    bad = dict(d, x=d["x"].copy())
    bad["x"][3] = np.nan
    bad["x"][21, ::2], bad["x"][21, 1::2] = np.inf, -np.inf
    bad["x"][64, 7] = np.nan
    got = np.concatenate(run_rpn(dev, bad, rows, C, a, bf16), 1)
    others = np.setdiff1d(np.arange(65), [3, 21, 64])
    assert np.array_equal(F.bits(got[others]), F.bits(base[others]))
    assert np.isnan(got[[3, 21, 64]]).all()          # (inf - inf in every column: the weights are dense)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rpn_head_module(dev, dtype):
    """RPNHead: its own packing (and cache) in front of the same launch, three maps"""
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.detector import RPNHead
    C, a, rows, bf16 = 128, 5, (20, 13, 32), dtype == "bf16"
    d = F.head_data(C, a, 65, True, seed=8, bf16=bf16)
    head = RPNHead(get_cfg("4c_Fpn432"), C, a).to(dev).eval()
    with torch.no_grad():
        head.conv.weight.copy_(T(d["w1"], dev).view(C, C, 1, 1))
        head.conv.bias.copy_(T(d["b1"], dev))
        head.cls_logits.weight.copy_(T(d["w2"][:a], dev).view(a, C, 1, 1))
        head.cls_logits.bias.copy_(T(d["b2"][:a], dev))
        head.bbox_pred.weight.copy_(T(d["w2"][a:], dev).view(7 * a, C, 1, 1))
        head.bbox_pred.bias.copy_(T(d["b2"][a:], dev))
        x = T(d["x"], dev).to(torch.bfloat16 if bf16 else torch.float32)
        feats = [x[0:20].contiguous(), x[20:33].contiguous(), x[33:65].contiguous()]
        assert head._fused_ok(feats)
        obj, reg = head(feats)
    _, want = F.head_reference(d, False, bf16)
    got = np.concatenate([obj.reshape(65, a).cpu().numpy(), reg.reshape(65, 7 * a).cpu().numpy()], 1)
    check_exact(("module", dtype), got, want)


MLP_IDS = [f"{C}-a{a}-n{n}-relu{r}" for C, a, n, r in F.mlp_cases()]


@pytest.mark.parametrize("case", F.mlp_cases(), ids=MLP_IDS)
def test_mlp_heads(dev, case):
    C, a, n, relu_in = case
    for exact in (True, False):
        d = F.head_data(C, a, n, exact, seed=a + n)
        t, oa, o7 = run_mlp(dev, d["x"], C, relu_in, d, a, True, True, True)              # fused, t_out
        _, oa2, o72 = run_mlp(dev, d["x"], C, relu_in, d, a, True, True, False)           # fused, no t_out
        t1, _, _ = run_mlp(dev, d["x"], C, relu_in, d, a, True, False, True)              # stage 1
        _, oa3, o73 = run_mlp(dev, t1, C, 0, d, a, False, True, False)                    # stage 2 on its result
        assert np.array_equal(F.bits(t), F.bits(t1))
        for x, y in ((oa2, o72), (oa3, o73)):
            assert np.array_equal(F.bits(x), F.bits(oa)) and np.array_equal(F.bits(y), F.bits(o7))
        want_t, want = F.head_reference(d, relu_in, False)
        got = np.concatenate([oa, o7], 1)
        if exact:
            check_exact((case, "t"), t, want_t)
            check_exact((case, "out"), got, want)
        else:
            bt, bo = F.rounding_bound(d, C, a, relu_in, False)
            check_bound((case, "t"), t, want_t, bt)
            check_bound((case, "out"), got, want, bo)
            # stage 2 alone against ITS reference: the rows it was given
            d2 = dict(d, x=t1)
            check_bound((case, "stage 2"), np.concatenate([oa3, o73], 1), F.head_reference(d2, False, False, 2)[1],
                        F.rounding_bound(d2, C, a, False, False, 2)[1])


def test_mlp_heads_no_rows(dev):
    d = F.head_data(128, 4, 1, True, seed=1)
    t, oa, o7 = run_mlp(dev, d["x"][:0], 128, 1, d, 4, True, True, True)
    assert t.shape == (0, 128) and oa.shape == (0, 4) and o7.shape == (0, 28)


@pytest.mark.parametrize("C,a", [(128, 5), (256, 8), (512, 17)])
def test_mlp_heads_locality(dev, C, a):
    d = F.head_data(C, a, 65, True, seed=6)
    base = run_mlp(dev, d["x"], C, 1, d, a, True, True, True)
    x = d["x"].copy()
    x[3] = np.nan                                      # through the input relu: stays a NaN
    x[40, ::2], x[40, 1::2] = np.inf, -np.inf          # relu: +inf and 0
    x[64, 5] = np.nan
    got = run_mlp(dev, x, C, 1, d, a, True, True, True)
    others = np.setdiff1d(np.arange(65), [3, 40, 64])
    for g, b in zip(got, base):
        assert np.array_equal(F.bits(g[others]), F.bits(b[others]))
        assert np.isnan(g[[3, 64]]).all() and not np.isfinite(g[40]).any()


def test_mlp_heads_module(dev, monkeypatch):
    """_pack_linear and the two callers of d3d_mlp_heads in detector.py (the fused box MLP, off by default): fc7 with
    the predictor's heads in one launch, and FPNPredictor.forward on its own"""
    from torch import nn
    from detection_3d_amd import detector
    from detection_3d_amd.config import get_cfg
    monkeypatch.setattr(detector, "_FUSED_BOX_MLP", True)
    cfg = get_cfg("4c_Fpn432")
    pred = detector.FPNPredictor(cfg).to(dev).eval()
    C, a, n = pred.cls_score.in_features, pred.cls_score.out_features, 33
    assert C == 512
    d = F.head_data(C, a, n, True, seed=9)
    fe = detector.FPN2MLPFeatureExtractor.__new__(detector.FPN2MLPFeatureExtractor)
    nn.Module.__init__(fe)
    fe.fc7 = nn.Linear(C, C).to(dev)
    with torch.no_grad():
        fe.fc7.weight.copy_(T(d["w1"], dev))
        fe.fc7.bias.copy_(T(d["b1"], dev))
        pred.cls_score.weight.copy_(T(d["w2"][:a], dev))
        pred.cls_score.bias.copy_(T(d["b2"][:a], dev))
        pred.bbox_pred.weight.copy_(T(d["w2"][a:], dev))
        pred.bbox_pred.bias.copy_(T(d["b2"][a:], dev))
        want_t, want = F.head_reference(d, True, False)
        h6 = T(d["x"], dev)
        x_alone = fe._fc7_and_heads(h6)                                    # stage 1 only
        assert getattr(x_alone, "_d3d_heads", None) is None
        la, ra = pred(x_alone)                                             # stage 2 only
        fe._heads = pred
        x = fe._fc7_and_heads(h6)                                          # fused
        assert x._d3d_heads is not None
        lf, rf = pred(x)
    for xx, l, r in ((x_alone, la, ra), (x, lf, rf)):
        check_exact("module t", xx.cpu().numpy(), want_t)
        check_exact("module out", np.concatenate([l.cpu().numpy(), r.cpu().numpy()], 1), want)


# ----------------------------------------------------------------------------------------------------------------------
# box decode
def decode(dev, enc, anchors, weights=(1.0,) * 7, clip=10000.0, rows=None, nc=1):
    """d3d_box_decode / _rows / _classes -> [n_out, 7]"""
    from detection_3d_amd._lib import floats
    L = _lib()
    e, an = T(enc, dev), T(anchors, dev)
    n_out = (enc.shape[0] * nc) if rows is None else rows.shape[0]
    out = torch.full(((n_out + PAD) * 7,), NAN, dtype=torch.float32, device=dev)
    if rows is not None:
        r = T(rows.astype(np.int64), dev)
        _call(L.d3d_box_decode_rows(P(e), P(an), P(r), n_out, floats(weights), float(clip), P(out), S()))
    elif nc != 1:
        _call(L.d3d_box_decode_classes(P(e), P(an), enc.shape[0], nc, floats(weights), float(clip), P(out), S()))
    else:
        _call(L.d3d_box_decode(P(e), P(an), enc.shape[0], floats(weights), float(clip), P(out), S()))
    assert _untouched(out, n_out * 7)
    return out[:n_out * 7].view(n_out, 7).cpu().numpy()


@pytest.mark.parametrize("clip", F.CLIPS)
@pytest.mark.parametrize("weights", F.WEIGHTS)
def test_decode_nonfinite(dev, weights, clip):
    enc, anchors, expect = F.nonfinite_cases()
    enc = enc * np.array(weights, np.float32)
    got = decode(dev, enc, anchors, weights, clip)
    assert np.array_equal(~np.isfinite(got), expect)
    assert same(got, oracle.box_decode(enc, anchors, weights, clip))


@pytest.mark.parametrize("clip", F.CLIPS)
@pytest.mark.parametrize("weights", F.WEIGHTS[::2])
def test_decode_clip(dev, weights, clip):
    enc, anchors, vals = F.clip_cases(clip, weights)
    got = decode(dev, enc, anchors, weights, clip)
    want = oracle.box_decode(enc, anchors, weights, clip)
    assert np.array_equal(F.bits(got), F.bits(want))
    slot = 3 + np.arange(9) // 3
    assert np.array_equal(got[np.arange(9), slot], (np.minimum(vals, np.float32(clip)) + np.float32(1)) * anchors[np.arange(9), slot])


def test_decode_weights(dev):
    enc, anchors = F.decode_rows(300, 21)
    enc[::3, 3:6] *= 40                                                    # some size deltas above log(1000)
    for weights in F.WEIGHTS:
        for clip in F.CLIPS:
            assert np.array_equal(F.bits(decode(dev, enc, anchors, weights, clip)), F.bits(oracle.box_decode(enc, anchors, weights, clip)))


def test_decode_yaw(dev):
    enc, anchors, _ = F.yaw_cases()
    got = decode(dev, enc, anchors)
    assert np.array_equal(F.bits(got), F.bits(oracle.box_decode(enc, anchors)))
    assert np.isfinite(got).all()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_decode_sizes(dev, n):
    enc, anchors = F.decode_rows(n, n)
    assert np.array_equal(F.bits(decode(dev, enc, anchors)), F.bits(oracle.box_decode(enc, anchors)))


def test_decode_rows_orders(dev):
    """repeated, descending and out-of-order row ids; a NaN size delta in a gathered row"""
    enc, anchors = F.decode_rows(300, 4)
    enc[17, 4] = np.nan
    for rows in (np.array([5, 5, 5, 299, 0, 0, 17]), np.arange(299, -1, -1), np.random.RandomState(0).permutation(300)[:257],
                 np.array([17])):
        got = decode(dev, enc, anchors, rows=rows, clip=F.CLIPS[0])
        want = oracle.box_decode(enc[rows], anchors[rows], clip=F.CLIPS[0])
        assert same(got, want)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).sum() == (rows == 17).sum()


@pytest.mark.parametrize("nc", [2, 5, 9])
def test_decode_classes(dev, nc):
    """[n, 7 nc] encodings against the row's one anchor (src / nc); n * nc is no multiple of 256"""
    n = 61
    assert (n * nc) % 256
    enc, _ = F.decode_rows(n * nc, nc)
    _, anchors = F.decode_rows(n, 50 + nc)
    enc[nc + 1, 5] = np.nan
    enc = enc.reshape(n, 7 * nc)
    weights = F.WEIGHTS[1]
    got = decode(dev, enc, anchors, weights, nc=nc).reshape(n, nc, 7)
    for c in range(nc):
        assert same(got[:, c], oracle.box_decode(enc[:, 7 * c:7 * c + 7], anchors, weights)), c
    assert np.isnan(got).sum() == 1 and np.isnan(got[1, 1, 5])


def test_decode_fused_in_topk(dev):
    """the decode of the selected rows inside d3d_topk_segments: a NaN size delta among them stays a NaN"""
    from detection_3d_amd import box_ops
    n, k = 700, 300
    rng = np.random.RandomState(12)
    vals = rng.permutation(n).astype(np.float32)
    reg, anchors = F.decode_rows(n, 13)
    best, later = int(np.argmax(vals)), int(np.argsort(-vals)[200])
    reg[best, 3], reg[later, 5] = np.nan, np.nan
    reg[int(np.argmin(vals)), 4] = np.nan                                  # not selected
    tk = box_ops.topk_segments(T(vals, dev), k, reg=T(reg, dev), anchors=T(anchors, dev))
    torch.cuda.synchronize()
    idx = np.argsort(-vals, kind="stable")[:k]
    assert np.array_equal(tk["idx"][0].cpu().numpy(), idx)
    got, want = tk["props"][0].cpu().numpy(), oracle.box_decode(reg[idx], anchors[idx])
    assert same(got, want)
    assert np.isnan(got).sum() == 2 and np.isnan(got[0, 3]) and np.isnan(got[200, 5])


# ----------------------------------------------------------------------------------------------------------------------
# final selection
SEL = F.select_cases()


def _pinned_word():
    return torch.full((1,), -1, dtype=torch.int32).pin_memory()


@pytest.mark.parametrize("c", SEL, ids=[c["name"] for c in SEL])
def test_post_select(dev, c):
    L = _lib()
    nseg, n_max, nc, D = c["nseg"], c["n_max"], c["nc"], c["D"]
    N = nseg * n_max
    keep, nk, prob, boxes = T(c["keep"], dev), T(c["nk"], dev), T(c["prob"], dev), T(c["boxes"], dev)
    wb, ws, wl = F.select_reference(c["keep"], c["nk"], n_max, c["prob"], c["boxes"], nc, D)
    for pinned in (False, True):
        ob = torch.full(((N + PAD) * 7,), NAN, device=dev)
        os_ = torch.full((N + PAD,), NAN, device=dev)
        ol = torch.full((N + PAD,), SENT_I, dtype=torch.int64, device=dev)
        on = _pinned_word() if pinned else torch.full((1,), -1, dtype=torch.int32, device=dev)
        _call(L.d3d_post_select(P(keep), P(nk), nseg, n_max, P(prob), P(boxes), nc, D, P(ob), P(os_), P(ol), P(on), S()))
        m = int(on[0])
        assert m == ws.shape[0], (c["name"], m, ws.shape[0])
        assert _untouched(ob, m * 7) and _untouched(os_, m) and _untouched(ol, m)
        assert np.array_equal(F.bits(ob[:m * 7].view(m, 7).cpu().numpy()), F.bits(wb))
        assert np.array_equal(F.bits(os_[:m].cpu().numpy()), F.bits(ws))
        assert np.array_equal(ol[:m].cpu().numpy(), wl)
    # d3d_post_gather on the same inputs
    flat, s = F.candidates(c["keep"], c["nk"], n_max, c["prob"])
    gs = torch.full((N + PAD,), NAN, device=dev)
    gf = torch.full((N + PAD,), SENT_I, dtype=torch.int64, device=dev)
    _call(L.d3d_post_gather(P(keep), P(nk), nseg, n_max, P(prob), P(gs), P(gf), S()))
    assert _untouched(gs, N) and _untouched(gf, N)
    assert np.array_equal(F.bits(gs[:N].cpu().numpy()), F.bits(s)) and np.array_equal(gf[:N].cpu().numpy(), flat)


def test_post_select_nothing(dev):
    """no segments / n_max = 0: out_n = 0 without a launch"""
    L = _lib()
    for nseg, n_max in ((0, 5), (3, 0)):
        on = torch.full((1,), -1, dtype=torch.int32, device=dev)
        _call(L.d3d_post_select(None, None, nseg, n_max, None, None, 2, 10, None, None, None, P(on), S()))
        assert int(on[0]) == 0
        _call(L.d3d_post_gather(None, None, nseg, n_max, None, None, None, S()))


@pytest.mark.parametrize("K", [0, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("nc", [2, 5])
def test_post_scores_and_order(dev, K, nc):
    L = _lib()
    prob, thresh = F.post_scores_case(K, nc)
    want_sc, want_counts = F.post_scores_reference(prob, thresh)
    p = T(prob, dev)
    counts = torch.full((nc - 1 + PAD,), 12345, dtype=torch.int32, device=dev)           # dirty
    for _ in range(2):                                                                  # ... and dirty with its own result
        sc = torch.full(((nc - 1) * K + PAD,), NAN, device=dev)
        _call(L.d3d_post_scores(P(p), K, nc, thresh, P(sc), P(counts), S()))
        assert np.array_equal(counts[:nc - 1].cpu().numpy(), want_counts) and bool((counts[nc - 1:] == 12345).all())
        assert _untouched(sc, (nc - 1) * K)
        assert np.array_equal(F.bits(sc[:(nc - 1) * K].view(nc - 1, K).cpu().numpy()), F.bits(want_sc))
    idx = np.stack([np.random.RandomState(j).permutation(K) for j in range(nc - 1)]).astype(np.int64).reshape(nc - 1, K)
    order = torch.full(((nc - 1) * K + PAD,), SENT_I, dtype=torch.int32, device=dev)
    idx_ = T(idx, dev)
    _call(L.d3d_post_order(P(idx_), K, nc, P(order), S()))
    assert _untouched(order, (nc - 1) * K)
    assert np.array_equal(order[:(nc - 1) * K].view(nc - 1, K).cpu().numpy(), F.post_order_reference(idx, nc))


@pytest.mark.parametrize("min_size", [0.0, 0.001])
@pytest.mark.parametrize("n_keep", [0, 300, 1000])
@pytest.mark.parametrize("pinned", [False, True])
def test_gather_kept(dev, n_keep, min_size, pinned):
    """n_keep = 0 (every row repeats candidate 0), P, above P; NaN and -0.0 sizes against min_size"""
    L = _lib()
    Pn, M = 300, 500
    rng = np.random.RandomState(n_keep + 1)
    boxes = rng.randn(M, 7).astype(np.float32)
    boxes[0, 3], boxes[0, 4] = np.nan, -0.0
    boxes[::9, 5], boxes[1::9, 3], boxes[2::9, 4] = np.nan, -0.0, 0.0005
    scores = rng.rand(M).astype(np.float32)
    keep = rng.permutation(M).astype(np.int32)
    wb, ws = F.gather_kept_reference(boxes, scores, keep, n_keep, Pn, min_size)
    ob = torch.full(((Pn + PAD) * 7,), NAN, device=dev)
    os_ = torch.full((Pn + PAD,), NAN, device=dev)
    word = _pinned_word() if pinned else None
    b_, s_, k_, n_ = T(boxes, dev), T(scores, dev), T(keep, dev), T(np.array([n_keep], np.int32), dev)
    _call(L.d3d_gather_kept(P(b_), P(s_), P(k_), P(n_), Pn, min_size, P(ob), P(os_), P(word), S()))
    assert word is None or int(word[0]) == n_keep
    assert torch.isnan(ob[Pn * 7:]).all() and _untouched(os_, Pn)
    assert same(ob[:Pn * 7].view(Pn, 7).cpu().numpy(), wb) and np.array_equal(F.bits(os_[:Pn].cpu().numpy()), F.bits(ws))
    assert np.array_equal(np.isnan(ob[:Pn * 7].view(Pn, 7).cpu().numpy()), np.isnan(wb))


def _post_inputs(dev, K, nc, seed):
    rng = np.random.RandomState(seed)
    logits = (np.round(rng.randn(K, nc) * 2) / 2).astype(np.float32)      # half-integer logits: rows repeat, scores tie
    logits[::4] = logits[min(1, K - 1)]
    reg = (rng.randn(K, 7 * nc) * 0.1).astype(np.float32)
    props = np.concatenate([rng.rand(K, 3) * [12, 12, 2], 0.4 + rng.rand(K, 3) * 1.5, (rng.rand(K, 1) - 0.5) * 3], 1)
    return T(logits, dev), T(reg, dev), T(props.astype(np.float32), dev)


def _same_dicts(a, b):
    for k in ("bbox3d", "scores", "labels"):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        assert np.array_equal(F.bits(x), F.bits(y)) if x.dtype == np.float32 else np.array_equal(x, y), k


@pytest.mark.parametrize("K,nc,D", [(300, 5, 40), (300, 5, 0), (257, 2, 10), (64, 9, 200), (1, 3, 1), (299, 5, 30)])
def test_post_processor_endings_agree(dev, monkeypatch, K, nc, D):
    """PostProcessor.forward ends with d3d_post_select or, above its cap, with d3d_post_gather and tensor ops: the same
    dicts; the post_scores / post_order branch (n_max above d3d_topk_max) gives them too"""
    from detection_3d_amd import box_ops, detector
    from detection_3d_amd.config import get_cfg
    post = detector.PostProcessor(get_cfg("4c_Fpn432"))
    post.detections_per_img = D
    logits, reg, props = _post_inputs(dev, K, nc, K + nc)
    if K == 299:
        logits[5::50, 2] = NAN                # rows whose probabilities are all NaN: never candidates, in any branch
    kernel = post(logits, reg, props)
    assert not torch.isnan(kernel["scores"]).any()
    if K > 1:
        assert kernel["scores"].shape[0] > 0
    if D == 40:
        assert kernel["scores"].shape[0] >= D
    with monkeypatch.context() as m:
        m.setattr(detector, "_POST_SELECT_CAP", [0])
        tensor = post(logits, reg, props)
    _same_dicts(kernel, tensor)
    with monkeypatch.context() as m:
        m.setattr(box_ops, "topk_max", lambda: 0)
        no_topk = post(logits, reg, props)
        m.setattr(detector, "_POST_SELECT_CAP", [0])
        neither = post(logits, reg, props)
    _same_dicts(kernel, no_topk)
    _same_dicts(kernel, neither)
    import torch.nn.functional as Fn
    want = post._select_reference(Fn.softmax(logits, -1), box_ops.box_decode(reg, props, post.weights))
    _same_dicts(kernel, want)
