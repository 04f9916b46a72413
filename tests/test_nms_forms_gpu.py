"""Every sweep form of the rotated NMS (csrc/nms.hip: k_nms_prep -> k_nms_pairs -> k_nms_eval -> sweep) at its size
edges, on scenes whose suppression graph is known in exact rational arithmetic, and the pair decision of k_nms_pairs /
k_nms_eval on families of hard box pairs against the CPU oracle (tests/nms_forms.py holds the scenes, the references and
the doubtful band; tests/test_nms_forms_cpu.py checks them without a GPU).

Every case runs under d3d_nms_sweep_mode 1 (register sweep) and 2 (LDS sweep), asserts the record of d3d_nms_last_form
against nms_forms.expect_form, and requires the same keep lists and counts from both and from the expected list.

  form                 reached by
  k_nms_sweep (regs)   every test below, mode 1: ncb 1 .. 64, chunk counts 1, 2, 3, 4, 5 (not a multiple of 3), 16, 17, 32,
                       33, 63, 64; segments 1, 3, 7 and 64 .. 300
  k_nms_sweep_lds<16>  test_size_edges n <= 1024 (ncb 1, 2, 3, 4, 5, 16: odd and even row words, chunk counts that are
                       and are not a multiple of kSwStages), test_structures (but clique_every_chunk), test_caps,
                       test_null_order_layout, test_pair_decisions (n_max = 2, up to 300 segments)
  k_nms_sweep_lds<32>  test_size_edges n = 1025 (ncb 17, the first of the template), 2047, 2048 (ncb 32)
  k_nms_sweep_lds<64>  test_size_edges n = 2049 (ncb 33), 4032 (ncb 63, 65,536 B of LDS), 4033 and 4096 (ncb 64, 66,560 B,
                       above 64 KiB and accepted as it is), test_structures[clique_every_chunk],
                       test_batched_ragged_segments (n_max 2049, counts 2049, 0, 1, 64, 65, 1000, 3000)
  entries              d3d_rotate_nms_3d_sorted and d3d_rotate_nms_3d (shuffled input, tied scores; n <= d3d_topk_max())
                       in test_size_edges, d3d_rotate_nms_3d_batched itself everywhere else

  fixed-point loop     path64 / path64_reversed (64 steps in one chunk), path128 (across a chunk boundary), clique64,
                       chunk_all_suppressed (alive == 0), the partly filled last chunks of the size edges (alive mask)
  early stop           test_caps: caps 64 / 128 / 192 / 256 end the sweep behind each of the four pipeline stages, 257 in
                       the first stage of the second round, 1 / 63 / 65 inside a chunk; survivors and survivors + 1; 0
  pair geometry        test_pair_decisions, test_identical_boxes_at_threshold_one

Not reached: more than 4096 candidates (rejected by the entry point: test_limits), the stop_s hand-off with a loader
wave that is a whole chunk late (a timing, not an input; see the comment in k_nms_sweep_lds), scratch buffers smaller
than required (rejected), and n_max > 0 with more than 300 segments."""
import ctypes

import numpy as np
import pytest
import torch

from tests import nms_forms as F

pytestmark = pytest.mark.gpu
MODES = (F.MODE_REGS, F.MODE_LDS)
SEEN = set()                      # (family, ncbmax) reported by d3d_nms_last_form in this process


def _lib():
    from detection_3d_amd._lib import lib
    return lib()


def last_form():
    buf = (ctypes.c_int * len(F.NMS_FIELDS))()
    n = _lib().d3d_nms_last_form(buf, len(F.NMS_FIELDS))
    assert n == len(F.NMS_FIELDS)
    form = dict(zip(F.NMS_FIELDS, buf))
    SEEN.add((form["family"], form["ncbmax"]))
    return form


class sweep_mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.was = _lib().d3d_nms_sweep_mode(-1)
        _lib().d3d_nms_sweep_mode(self.mode)

    def __exit__(self, *exc):
        _lib().d3d_nms_sweep_mode(self.was)


_SCRATCH = {}


def run_batched(dev, boxes, order, stride, counts, segments, n_max, thr, clamp=(0.0, 0.0), cap=0):
    """d3d_rotate_nms_3d_batched as it is: -> (keep [segments, n_max], n_keep [segments]) as numpy; both buffers are
    prefilled, so an entry the launch did not write shows as -7"""
    from detection_3d_amd._lib import check, ptr, stream_of
    L = _lib()
    bt = torch.from_numpy(np.ascontiguousarray(boxes, np.float32)).to(dev)
    ot = None if order is None else torch.from_numpy(np.ascontiguousarray(order, np.int32)).to(dev)
    ct = None if counts is None else torch.from_numpy(np.ascontiguousarray(counts, np.int32)).to(dev)
    nbytes = L.d3d_nms_batched_scratch_bytes(segments, n_max)
    if _SCRATCH.get("n", 0) < nbytes:
        _SCRATCH["buf"] = None
        _SCRATCH["buf"] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _SCRATCH["n"] = nbytes
    keep = torch.full((segments, max(n_max, 1)), -7, dtype=torch.int32, device=dev)
    nk = torch.full((segments,), -7, dtype=torch.int32, device=dev)
    last_form()
    check(L.d3d_rotate_nms_3d_batched(ptr(bt), ptr(ot), int(stride), ptr(ct), int(segments), int(n_max), float(thr),
                                      float(clamp[0]), float(clamp[1]), int(cap), ptr(keep), ptr(nk), ptr(_SCRATCH["buf"]),
                                      _SCRATCH["n"], stream_of()))
    torch.cuda.synchronize()
    return keep.cpu().numpy(), nk.cpu().numpy()


def both_modes(dev, want_segments, *args, **kw):
    """runs run_batched in both sweep modes, asserts the form records and that the two give the same lists; -> (keep
    lists per segment, counts)"""
    segments, n_max, cap = args[4], args[5], kw.get("cap", 0)
    out = []
    for mode in MODES:
        with sweep_mode(mode):
            keep, nk = run_batched(dev, *args, **kw)
            assert last_form() == F.expect_form(n_max, mode, segments, cap), (mode, n_max)
        assert nk.min() >= 0 and nk.max() <= n_max                   # every count was written
        out.append(([keep[b, :nk[b]].tolist() for b in range(segments)], nk.tolist()))
    assert out[0] == out[1]
    return out[0]


def one_list(dev, scene, cap=0):
    n = scene["boxes"].shape[0]
    lists, nk = both_modes(dev, 1, scene["boxes"], None, 0, None, 1, n, scene["thr"], cap=cap)
    return lists[0]


# ------------------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("n", F.SIZES)
def test_size_edges(dev, n):
    from detection_3d_amd import box_ops
    sc = F.size_scene(n)
    want = sc["keep"]
    bt = torch.from_numpy(sc["boxes"]).to(dev)
    sb, ss, slot = F.shuffled_with_ties(sc, n)
    for mode in MODES:
        with sweep_mode(mode):
            last_form()
            keep, nk = box_ops._nms_sorted(bt, sc["thr"])
            assert last_form() == F.expect_form(n, mode), (n, mode)
            assert int(nk) == len(want) and keep[:int(nk)].tolist() == want, (n, mode)
            if n <= box_ops.topk_max():
                got = box_ops.rotate_nms_3d(torch.from_numpy(sb).to(dev), torch.from_numpy(ss).to(dev), None, None, sc["thr"])
                assert last_form() == F.expect_form(n, mode), (n, mode)
                assert got.tolist() == slot[want].tolist(), (n, mode)
    assert box_ops.topk_max() >= F.N_LIMIT


# ------------------------------------------------------------------------------------------------------- structure
@pytest.mark.parametrize("name", F.STRUCTURES)
def test_structures(dev, name):
    sc = F.structure_scene(name)
    assert one_list(dev, sc) == sc["keep"]


# ------------------------------------------------------------------------------------------------------------ caps
@pytest.mark.parametrize("name", ["all_isolated", "mixed1100"])
def test_caps(dev, name):
    sc = F.structure_scene(name)
    full = sc["keep"]
    n = sc["boxes"].shape[0]
    assert len(full) > 257
    for cap in (1, 63, 64, 65, 128, 192, 256, 257, len(full), len(full) + 1, 0):
        lists, nk = both_modes(dev, 1, sc["boxes"], None, 0, None, 1, n, sc["thr"], cap=cap)
        assert nk[0] == (min(len(full), cap) if cap else len(full)), cap
        assert lists[0] == full[:nk[0]], cap


# --------------------------------------------------------------------------------------------------------- batched
def test_batched_ragged_segments(dev):
    sc = F.size_scene(2049)
    n_max, stride = 2049, 2049 + 13
    counts = np.array([2049, 0, 1, 64, 65, 1000, 3000], np.int32)
    rng = np.random.RandomState(9)
    order = rng.randint(0, n_max, (len(counts), stride)).astype(np.int32)     # garbage past each count (valid rows)
    want = []
    for b, c in enumerate(counts):
        sel = rng.permutation(n_max)[:min(int(c), n_max)]
        order[b, :len(sel)] = sel
        want.append([int(sel[k]) for k in F.restrict(sc, sel)[2]])
    lists, nk = both_modes(dev, len(counts), sc["boxes"], order, stride, counts, len(counts), n_max, sc["thr"])
    assert nk == [len(w) for w in want] and nk[1] == 0 and nk[2] == 1
    assert lists == want
    assert nk[0] < 2049 and nk[6] < 2049 and want[0] != want[6]


def test_null_order_layout(dev):
    """order == NULL, counts == NULL: segment b is rows b * stride .. + n_max, keep holds box rows"""
    n_max, stride, B = 130, 140, 3
    boxes = np.zeros((B * stride, 7), np.float32)
    want = []
    for b in range(B):
        sc = F.mixed_scene(n_max, 50 + b)
        boxes[b * stride:b * stride + n_max] = sc["boxes"]
        boxes[b * stride + n_max:(b + 1) * stride] = sc["boxes"][0]          # rows between the segments: never read
        want.append([b * stride + k for k in sc["keep"]])
    lists, nk = both_modes(dev, B, boxes, None, stride, None, B, n_max, 0.5)
    assert lists == want


# ----------------------------------------------------------------------------------------------------------- pairs
def _pairs(dev, a, b, thr, clamp):
    n = a.shape[0]
    two = np.empty((2 * n, 7), np.float32)
    two[0::2], two[1::2] = a, b
    lists, nk = both_modes(dev, n, two, None, 2, None, n, 2, thr, clamp=clamp)
    nk = np.asarray(nk)
    assert np.all((nk == 1) | (nk == 2))
    for p in range(n):
        assert lists[p] == ([2 * p] if nk[p] == 1 else [2 * p, 2 * p + 1])
    return nk == 1


@pytest.mark.parametrize("name", sorted(F.FAMILY_RECORD))
def test_pair_decisions(dev, name):
    m = F.measure()
    f, r = m["inputs"][name], m["families"][name]
    assert f["a"].shape[0] <= F.N_LIMIT
    got = _pairs(dev, f["a"], f["b"], f["thr"], f["clamp"])
    sure = ~r["doubtful"]
    assert r["doubtful"].mean() <= F.DOUBTFUL_CAP
    bad = np.nonzero((got != r["suppress"]) & sure)[0]
    assert bad.size == 0, (name, bad[:10], r["gate"][bad[:10]], r["iou"][bad[:10]])
    if r["both"]:
        assert got[sure].any() and (~got[sure]).any()


def test_identical_boxes_at_threshold_one(dev):
    two = F.identical_at_one()
    assert _pairs(dev, two[0::2], two[1::2], 1.0, (0.0, 0.0)).all()


# ---------------------------------------------------------------------------------------------------------- record
def test_limits_switch_and_record(dev):
    from detection_3d_amd import box_ops
    from detection_3d_amd._lib import D3DError
    L = _lib()
    was = L.d3d_nms_sweep_mode(-1)
    try:
        assert L.d3d_nms_sweep_mode(1) == was and L.d3d_nms_sweep_mode(-1) == 1
        assert L.d3d_nms_sweep_mode(7) == 1 and L.d3d_nms_sweep_mode(-1) == 1       # out of range: ignored
        assert L.d3d_nms_sweep_mode(0) == 1
        sc = F.size_scene(65)
        last_form()
        keep, nk = run_batched(dev, sc["boxes"], None, 0, None, 1, 65, 0.5)            # mode 0 is the LDS form
        assert last_form() == F.expect_form(65, F.MODE_DEFAULT) and keep[0, :nk[0]].tolist() == sc["keep"]
        assert last_form() == dict.fromkeys(F.NMS_FIELDS, 0)                           # cleared by the read
        keep, nk = run_batched(dev, sc["boxes"], None, 0, None, 1, 0, 0.5)             # nothing launched
        assert nk.tolist() == [0] and last_form() == dict.fromkeys(F.NMS_FIELDS, 0)
        assert L.d3d_nms_last_form(None, 0) == len(F.NMS_FIELDS)
        with pytest.raises(D3DError):
            run_batched(dev, np.zeros((4097, 7), np.float32), None, 0, None, 1, 4097, 0.5)
    finally:
        L.d3d_nms_sweep_mode(was)


def test_all_four_sweep_forms_were_reported(dev):
    """(runs last in this module) the suite's own process has been through every sweep form"""
    if not {(F.REGS, 0), (F.LDS, 16), (F.LDS, 32), (F.LDS, 64)} <= SEEN:
        for n in (64, 1025, 2049):
            for mode in MODES:
                with sweep_mode(mode):
                    sc = F.size_scene(n)
                    run_batched(dev, sc["boxes"], None, 0, None, 1, n, sc["thr"])
                    last_form()
    assert {(F.REGS, 0), (F.LDS, 16), (F.LDS, 32), (F.LDS, 64)} <= SEEN
