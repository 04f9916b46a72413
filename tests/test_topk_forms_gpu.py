"""Every form of the exact top-k selection (csrc/topk.hip: k_topk_select behind d3d_topk_segments and d3d_rotate_nms_3d)
against the defined order in plain numpy (tests/topk_forms.py holds the cases, built from key bits, and reference_topk;
tests/test_topk_forms_cpu.py checks them without a GPU).

d3d_topk_segments is called through ctypes as it is.  Every output is prefilled with a sentinel, every case runs WITH key
scratch and WITHOUT it whatever its size, the two runs must give the same bytes, and both must equal the reference bit for
bit: indices, scores and counts, rows [min(k, elements), k) still the sentinel.  Nothing here takes a tolerance.

  form / decision          reached by
  no key scratch           every case: n = 1 .. 70001 (box_ops.topk_segments uses it below n = 8192 only)
  key scratch              every case: n = 1, 3, 4, 5 (n4 padding, one 16-byte group), 63 .. 65, 1023 .. 1025, 4095 .. 4097
                           (one outer round of 16384), 16383, 16384 (exactly one round), 16385 (second round, one group),
                           32769, 70001; segments > 1: the layout cases (scratch row s at s * n4, n = 1301, n4 = 1304)
  misaligned scratch       test_misaligned_scratch_is_the_form_without (pointer + 8: the entry falls back)
  radix levels             test_cases[level*]: the k-th key decided at level 1, 2, 3; in bin 0 (NaN) / 3 (-inf) / 2044
                           (+inf) / 1023 / 1024 of level 1, bin 0 / 2047 / 1023 of level 2, bin 0 / 1023 / 511 of level 3
                           (thread 1023, thread 0 and thread 512 of find_bin_from_top); the keys above all in one bin /
                           one per bin
  hist_add (wbin, wcnt)    test_cases[hist_*]: one bin per wave, a / b per lane, a new bin every wave, 64 distinct bins,
                           ramps, a run across a pass edge (1024 without scratch, 16384 with); each at the three levels,
                           as element patterns and stretched by 4 (the lane pattern of the scratch form)
  all_ties / ranked        test_cases[ties_*]: n_eq == need_eq, need_eq = 1, n_eq - 1, ties in the last thread's range
                           only, across a range edge, across threads 63 | 64, everything equal
  sort sizes               P = 128 .. 4096 through k = 1, 127, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4095,
                           4096 and k > n
  values                   negatives, zeros of both signs, +-inf, denormals, NaN of both signs (top, threshold, all)
  layouts                  (1, 0, 1), (G, 1, G) for G = 1, 3, (1, K, 4); 1 .. 3 examples, interleaved, with a tail, with
                           5 elements, with none; min_value counts
  outputs                  test_every_subset_of_outputs (16 subsets, idx_map with groups and examples),
                           test_props_equal_the_oracle_decode
  sigmoid                  test_sigmoid_form: ordinary, saturated to 1.0 and 0.0, denormal results
  d3d_rotate_nms_3d        test_rotate_nms_entry: with and without key scratch behind the NMS scratch

Cost: every launch is one workgroup per segment; the module's 383 tests take 3.6 s on an MI355X (837 launches, 0.04 s of
it between launch and synchronise), 1.34 M elements compared.

With `topk_key`'s zero rule taken out, test_cases[zeros_minus_first] differs first in row 0 (72 tests fail: the zeros_*
and denormals_* cases, the size and layout cases whose k reaches the zeros, test_rotate_nms_entry[*-zeros]); with its NaN
rule taken out, test_cases[nan_k1] differs first in row 0 (96 tests fail: nan_*, level1_nan_*, level1_neg_inf_*, every
layout case, test_nan_min_value_count_has_one_writer, test_rotate_nms_entry[*-nan], test_sigmoid_form[saturated]).

Not reached: k > d3d_topk_max() and the other rejected arguments (test_argument_checks sees the return code only), n above
70001 (test_boxes_gpu.py runs 160 000 through the wrapper; nothing near the 2^31 limit of the int element index), more
than 12 segments in one launch, a stream other than the current one."""
import ctypes
import time

import numpy as np
import pytest
import torch

import oracle
from tests import topk_forms as F

pytestmark = pytest.mark.gpu
CASES = F.cases_by_name()
SENT_I, SENT_F = -7, np.float32(-12345.0)
TOTAL = {"elements": 0, "launches": 0, "seconds": 0.0}
OUTPUTS = ("idx32", "idx64", "scores")


def _lib():
    from detection_3d_amd._lib import lib
    return lib()


_BUF = {}


def _scratch(dev, nbytes):
    """a 16-byte aligned device buffer of at least nbytes (+ 16, for the misaligned form)"""
    if _BUF.get("n", 0) < nbytes + 16:
        _BUF["buf"] = None
        _BUF["buf"] = torch.empty(max(nbytes + 16, 1 << 20), dtype=torch.uint8, device=dev)
        _BUF["n"] = _BUF["buf"].numel()
        assert _BUF["buf"].data_ptr() % 16 == 0
    return _BUF["buf"]


def run(dev, c, scratch, outputs=OUTPUTS, idx_map=None, sigmoid=False, reg=None, anchors=None, vals_dev=None,
        scratch_offset=0, check_rc=True):
    """d3d_topk_segments on case c -> dict of numpy arrays, every output prefilled with its sentinel.  scratch: give the
    key scratch (d3d_topk_scratch_bytes) or none"""
    from detection_3d_amd._lib import check, ptr, stream_of
    L = _lib()
    S, k, n = c["n_groups"] * c["n_examples"], c["k"], c["n"]
    vt = torch.from_numpy(c["vals"].copy()).to(dev) if vals_dev is None else vals_dev   # (the cases are read-only)
    et = None if c["example"] is None else torch.from_numpy(c["example"]).to(dev)
    out = {"idx32": torch.full((S, max(k, 1)), SENT_I, dtype=torch.int32, device=dev) if "idx32" in outputs else None,
           "idx64": torch.full((S, max(k, 1)), SENT_I, dtype=torch.int64, device=dev) if "idx64" in outputs else None,
           "scores": torch.full((S, max(k, 1)), float(SENT_F), dtype=torch.float32, device=dev) if "scores" in outputs else None,
           "props": torch.full((S, max(k, 1), 7), float(SENT_F), dtype=torch.float32, device=dev) if "props" in outputs else None,
           "counts": torch.full((S,), SENT_I, dtype=torch.int32, device=dev)}
    nbytes = int(L.d3d_topk_scratch_bytes(n, S)) if scratch else 0
    buf = _scratch(dev, nbytes) if scratch else None
    sp = ctypes.c_void_p(buf.data_ptr() + scratch_offset) if scratch else None
    mv = ctypes.byref(ctypes.c_float(float(c["min_value"]))) if c["min_value"] is not None else None
    im = (ctypes.c_int * 3)(*idx_map) if idx_map is not None else None
    rt = None if reg is None else torch.from_numpy(reg).to(dev)
    at = None if anchors is None else torch.from_numpy(anchors).to(dev)
    t0 = time.perf_counter()
    rc = L.d3d_topk_segments(ptr(vt), n, c["elem_stride"], c["group_stride"], c["n_groups"], ptr(et), c["n_examples"], k,
                             int(sigmoid), mv, im, ptr(rt), 0 if reg is None else reg.shape[1], ptr(at), 10000.0,
                             ptr(out["idx32"]), ptr(out["idx64"]), ptr(out["scores"]), ptr(out["props"]), ptr(out["counts"]),
                             sp, nbytes, stream_of())
    torch.cuda.synchronize()
    TOTAL["seconds"] += time.perf_counter() - t0
    TOTAL["launches"] += 1
    if check_rc:
        check(rc)
    res = {name: None if t is None else t.cpu().numpy() for name, t in out.items()}
    res["rc"] = rc
    return res


def same_bytes(a, b):
    return all((a[name] is None and b[name] is None) or a[name].tobytes() == b[name].tobytes()
               for name in ("idx32", "idx64", "scores", "props", "counts"))


def both(dev, c, **kw):
    """with key scratch and without: the same bytes.  -> the result"""
    with_, without = run(dev, c, True, **kw), run(dev, c, False, **kw)
    assert same_bytes(with_, without), c["name"]
    return with_


def compare(c, got, want, idx_map=(1, 0, 0), score_of=None):
    """got against the reference segments `want`, bit for bit; rows past min(k, elements) hold the sentinel"""
    k = c["k"]
    for s, (idx, vals, cnt, m) in enumerate(want):
        g = s % c["n_groups"]
        assert got["counts"][s] == cnt, (c["name"], s, "count", int(got["counts"][s]), cnt)
        TOTAL["elements"] += 1
        if score_of is not None:
            vals = score_of(g)[idx]
        for name, ref in (("idx32", idx * idx_map[0] + idx_map[1] + g * idx_map[2]), ("idx64", idx), ("scores", vals)):
            if got[name] is None:
                continue
            row = got[name][s]
            a, b = (F.bits(row[:m]), F.bits(ref)) if name == "scores" else (row[:m].astype(np.int64), ref)
            bad = np.nonzero(a != b)[0]
            if name == "scores" and score_of is not None:    # a COMPUTED NaN (sigmoid of a NaN): a NaN, whatever its bits
                bad = np.nonzero((a != b) & ~(np.isnan(row[:m]) & np.isnan(ref)))[0]
            assert bad.size == 0, (c["name"], name, "segment", s, "first differing row", int(bad[0]), a[bad[0]], b[bad[0]])
            if k > 0:
                sent = F.bits(np.array([SENT_F]))[0] if name == "scores" else SENT_I
                rest = F.bits(row[m:k]) if name == "scores" else row[m:k]
                assert (rest == sent).all(), (c["name"], name, "segment", s, "written past row", m)
            TOTAL["elements"] += max(k, 0)


# --------------------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("name", list(CASES))
def test_cases(dev, name):
    c = CASES[name]
    compare(c, both(dev, c), F.reference_case(c))


# ------------------------------------------------------------------------------------------------------------ outputs
def test_every_subset_of_outputs(dev):
    """each of the 16 subsets of idx32 / idx64 / scores / props non-null, idx_map with several groups and examples"""
    rng = np.random.RandomState(4)
    c = CASES["layout_columns_G3_B2_tail_k40"]
    n, G = c["n"], 3
    reg = (rng.randn(n, 7 * G) * 0.2).astype(np.float32)
    anchors = np.concatenate([rng.rand(n, 3) * 20, 0.2 + rng.rand(n, 3) * 3, (rng.rand(n, 1) - 0.5) * 3], 1).astype(np.float32)
    want = F.reference_case(c)
    idx_map = (5, 11, 1000)
    props = None
    for mask in range(16):
        outs = tuple(name for bit, name in enumerate(OUTPUTS + ("props",)) if mask >> bit & 1)
        kw = dict(reg=reg, anchors=anchors) if "props" in outs else {}
        got = both(dev, c, outputs=outs, idx_map=idx_map, **kw)
        assert [name for name in OUTPUTS + ("props",) if got[name] is not None] == list(outs)
        compare(c, got, want, idx_map=idx_map)
        if "props" in outs:
            props = got["props"] if props is None else props
            assert got["props"].tobytes() == props.tobytes()
    # the mapped index separates groups: dropping g * idx_map[2] would repeat group 0's numbers
    got = both(dev, c, outputs=("idx32",), idx_map=idx_map)
    assert got["idx32"][1, 0] - 1000 == want[1][0][0] * 5 + 11 and got["idx32"][5, 0] - 2000 == want[5][0][0] * 5 + 11


def test_props_equal_the_oracle_decode(dev):
    """the RPN layout: class-group columns, an example index per element, sigmoid and the decode fused in"""
    rng = np.random.RandomState(6)
    base = CASES["layout_columns_G3_B3_tail_k40"]
    n, G = base["n"], 3
    c = dict(base, vals=(rng.randn(n * G) * 3).astype(np.float32), k=300)
    c["vals"][::5] = 25.0
    reg = (rng.randn(n, 7 * G) * 0.2).astype(np.float32)
    anchors = np.concatenate([rng.rand(n, 3) * 20, 0.2 + rng.rand(n, 3) * 3, (rng.rand(n, 1) - 0.5) * 3], 1).astype(np.float32)
    sig = torch.sigmoid(torch.from_numpy(c["vals"]).to(dev)).cpu().numpy()
    score_of = lambda g: sig[g + np.arange(n) * G]
    want = F.reference_case(c, values_of=score_of)
    got = both(dev, c, outputs=OUTPUTS + ("props",), sigmoid=True, reg=reg, anchors=anchors)
    compare(c, got, want, score_of=score_of)
    for s, (idx, _, cnt, m) in enumerate(want):
        g = s % G
        ref = oracle.box_decode(reg[idx, 7 * g:7 * g + 7], anchors[idx])
        assert np.array_equal(F.bits(got["props"][s, :m]), F.bits(ref)), s
        assert (F.bits(got["props"][s, m:]) == F.bits(np.array([SENT_F]))[0]).all()
        TOTAL["elements"] += 7 * c["k"]


# ------------------------------------------------------------------------------------------------------------ sigmoid
@pytest.mark.parametrize("family", F.SIGMOID_FAMILIES)
def test_sigmoid_form(dev, family):
    """scores = the bits of torch.sigmoid of the same device tensor; the order is the defined one on those bits"""
    x = F.sigmoid_logits(family)
    n = x.shape[0]
    xt = torch.from_numpy(x).to(dev)
    sig = torch.sigmoid(xt).cpu().numpy()
    if family == "saturated":
        assert (sig == 1.0).sum() > 100 and (sig == 0.0).sum() > 100 and np.isnan(sig).any()
    if family == "denormal":
        tiny = (sig > 0) & (sig < np.float32(1.1754944e-38))
        assert tiny.sum() > n // 2 and (sig == 0.0).any()
    for k in (1, n // 3, n):
        c = F.case(f"sigmoid_{family}_k{k}", x, k)
        got = both(dev, c, sigmoid=True, vals_dev=xt)
        compare(c, got, F.reference_case(c, values_of=lambda g: sig), score_of=lambda g: sig)
    for k, mv in ((n, 0.5), (n, 0.0), (n // 2, 1.0)):
        c = F.case(f"sigmoid_{family}_min{mv}", x, k, min_value=mv)
        got = both(dev, c, sigmoid=True, vals_dev=xt)
        compare(c, got, F.reference_case(c, values_of=lambda g: sig), score_of=lambda g: sig)


# ------------------------------------------------------------------------------------------------------------ scratch
@pytest.mark.parametrize("name", ["size_n16385_k2049", "nan_k5", "layout_rows_B2_interleaved_k40"])
def test_misaligned_scratch_is_the_form_without(dev, name):
    """a scratch pointer 8 bytes off a 16-byte boundary: the entry drops it, the result is the one without scratch"""
    c = CASES[name]
    got = run(dev, c, True, scratch_offset=8)
    assert same_bytes(got, run(dev, c, False))
    compare(c, got, F.reference_case(c))


# ---------------------------------------------------------------------------------------------------- rotate_nms_3d
def _rotate_nms(dev, boxes, scores, pre, with_keys):
    from detection_3d_amd._lib import check, ptr, stream_of
    L = _lib()
    n = boxes.shape[0]
    k = min(n, pre)
    nbytes = int(L.d3d_rotate_nms_3d_scratch_bytes(k, n if with_keys else 0))
    assert (nbytes > int(L.d3d_rotate_nms_3d_scratch_bytes(k, 0))) == with_keys
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    bt, st = torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev)
    keep = torch.full((k,), SENT_I, dtype=torch.int64, device=dev)
    nk = torch.full((1,), SENT_I, dtype=torch.int32, device=dev)
    n_host = ctypes.c_int(-1)
    check(L.d3d_rotate_nms_3d(ptr(bt), ptr(st), n, pre, 0, 0.5, 0.0, 0.0, ptr(keep), ptr(nk), ctypes.byref(n_host), ptr(buf),
                              nbytes, stream_of()))
    torch.cuda.synchronize()
    assert int(nk[0]) == n_host.value
    return keep.cpu().numpy(), n_host.value


@pytest.mark.parametrize("kind", F.NMS_SCORE_KINDS)
@pytest.mark.parametrize("n,pre", [(300, 128), (9001, 2000)])
def test_rotate_nms_entry(dev, kind, n, pre):
    """well-separated boxes: nothing is suppressed, the keep list is the selection -- with the key scratch behind the
    NMS scratch and without it, against the oracle port's boxlist_nms_3d"""
    from oracle.detector_port import nms_clamped
    boxes, scores = F.separated_boxes(n), F.nms_scores(kind, n)
    want = nms_clamped(boxes, scores, 0.5, (0.0, 0.0), n, pre_max=pre)
    assert len(want) == min(n, pre) and np.array_equal(want, F.reference_topk(scores, pre)[0])
    for with_keys in (False, True):
        keep, nk = _rotate_nms(dev, boxes, scores, pre, with_keys)
        assert nk == len(want) and np.array_equal(keep, want), (kind, with_keys, np.nonzero(keep != want)[0][:3])
        TOTAL["elements"] += len(want) + 1


# ------------------------------------------------------------------------------------------------------- determinism
def test_nan_min_value_count_has_one_writer(dev):
    """the NaN min_value case 20 times in one process: the same bytes every time (the count is written once)"""
    c = CASES[F.NAN_MIN_VALUE_REPEAT]
    want = F.reference_case(c)
    first = both(dev, c)
    compare(c, first, want)
    for scratch in (True, False) * 10:
        again = run(dev, c, scratch)
        assert again["counts"].tolist() == first["counts"].tolist() == [want[0][2]] and same_bytes(again, first)


# ---------------------------------------------------------------------------------------------------------- arguments
def test_argument_checks(dev):
    L = _lib()
    assert L.d3d_topk_max() == F.TOPK_MAX
    assert L.d3d_topk_scratch_bytes(5, 3) == 3 * 8 * 4 and L.d3d_topk_scratch_bytes(0, 3) == 0
    v = np.arange(10, dtype=np.float32)
    assert run(dev, F.case("k_above_max", v, F.TOPK_MAX + 1), False, check_rc=False)["rc"] != 0
    two = F.case("examples_without_index", v, 3, n_examples=2)
    got = run(dev, two, False, check_rc=False)
    assert got["rc"] != 0 and (got["counts"] == SENT_I).all()
    rng = np.random.RandomState(0)
    anchors = np.abs(rng.randn(10, 7)).astype(np.float32)
    got = run(dev, F.case("props_without_reg", v, 3), False, outputs=("props",), anchors=anchors, check_rc=False)
    assert got["rc"] != 0 and (got["props"] == SENT_F).all()
    for c in (F.case("n_zero", np.zeros(0, np.float32), 5, n_groups=1),
              F.case("k_zero", v, 0),
              F.case("n_zero_segments", np.zeros(0, np.float32), 5, n=0, n_groups=3)):
        for scratch in (False, True):
            got = run(dev, c, scratch)
            assert (got["counts"] == 0).all() and (got["idx64"] == SENT_I).all() and (got["scores"] == SENT_F).all()
    assert L.d3d_topk_segments(None, 10, 1, 0, 1, None, 1, 3, 0, None, None, None, 0, None, 0.0, None, None, None, None, None,
                               None, 0, None) != 0                              # null counts


def test_zz_totals(dev):
    """(runs last in this module) what the module compared, for the record"""
    if TOTAL["launches"] == 0:                      # (run on its own)
        test_cases(dev, "zeros_minus_first")
    print(f"\ntopk forms: {TOTAL['elements']} elements compared, 0 differing; {TOTAL['launches']} launches, "
          f"{TOTAL['seconds']:.2f} s in launch + synchronise")
    assert TOTAL["launches"] > 0 and TOTAL["elements"] > 0
