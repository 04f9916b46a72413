"""Label assignment (csrc/box_match.hip: d3d_match_segments = k_match_pass1 / k_match_pass2) and the IoU matrix it shares its
device code with (k_iou_matrix: d3d_boxes_iou_3d, d3d_rotate_iou_eval) against results that involve neither the library
nor, on lattice boxes, the oracle (tests/match_forms.py holds the boxes, the numpy Matcher and the scenes;
tests/test_match_forms_cpu.py checks them without a GPU).

  matrix, lattice     29 hard pair families on both sides of the 64 x 64 tile edge, N, K in {1, 63, 64, 65, 129}, four
                      criteria, four clamp sets, only_xy on and off, and 200 x 300 random lattice boxes: every element
                      bit-equal to the exact expectation, none excused
  matrix, rotated     the rotated hard families of tests/nms_forms.py as 300 x 300 matrices against the oracle: every
                      element within 1e-4 x max(1, |want|), NaN where the oracle has NaN, fewer than 1e-3 of the elements
                      differing in bits.  Measured on an MI355X: 0 of 3,007,008 elements differ (17 families, criterion
                      -1 unclamped and criterion 2 with the targets' clamps), largest error 0
  matcher             every scene of match_forms.SCENE_NAMES (rule scenes, size and layout cases) in the modes rpn, roi
                      and eq: `matched` equal to the numpy Matcher over the exact qualities, ties included, and `reg`
                      bit-equal to box_encode restated in fp32 numpy -- no element differs, so no allowance is made
  non-finite          one NaN (either sign), +Inf or -Inf field in a GT row or a prediction: the matrix has NaN where the
                      oracle has NaN and equal bits elsewhere, `matched` equals the numpy Matcher over the oracle's matrix

What fails when a fix in csrc/box_match.hip or box_geometry.inc is taken out again (each one alone, measured on an MI355X):
  `v < bound ? bound : v` clamps in load_box   test_non_finite_matrix (gt[3]=nan, gt[5]=nan, pred[3]=nan, pred[5]=nan and their
                                               -nan forms), test_non_finite_matcher, the rotated family non_finite
  NaN z factor in iou_pair                     test_non_finite_matrix (gt[2]=nan, gt[5]=nan, pred[2]=nan, pred[5]=nan, -nan),
                                               test_non_finite_matcher, the rotated family non_finite
  NaN of either sign on top in the ordered key test_non_finite_matcher[rpn] and [eq]: pred[2]=inf, pred[2]=-inf, pred[3]=-nan,
                                               pred[4]=-nan (the device gives these qualities as NaN with the sign bit set)
  no bounding-box early-out for a zero size    test_matrix_rotated_families_against_the_oracle, family tiny_sizes (800 of
                                               90,000 elements NaN where the oracle has a value, criterion -1)"""
import numpy as np
import pytest
import torch

from tests import match_forms as F

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _t(dev, a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype, order="C")).to(dev)


def iou_3d(dev, rows, cols, clamps, criterion, only_xy=False):
    """d3d_boxes_iou_3d as it is -> numpy [M, N]; the output is prefilled, so an element the launch skipped shows as -7"""
    from detection_3d_amd._lib import check, floats, lib, ptr, stream_of
    t, a = _t(dev, rows), _t(dev, cols)
    out = torch.full((t.shape[0], a.shape[0]), -7.0, dtype=torch.float32, device=dev)
    check(lib().d3d_boxes_iou_3d(ptr(t), t.shape[0], ptr(a), a.shape[0], floats(clamps), int(criterion), int(only_xy),
                                 ptr(out), stream_of()))
    return out.cpu().numpy()


def iou_eval(dev, rows, cols, criterion):
    from detection_3d_amd._lib import check, lib, ptr, stream_of
    t, a = _t(dev, rows[:, [0, 1, 3, 4, 6]]), _t(dev, cols[:, [0, 1, 3, 4, 6]])
    out = torch.full((t.shape[0], a.shape[0]), -7.0, dtype=torch.float32, device=dev)
    check(lib().d3d_rotate_iou_eval(ptr(t), t.shape[0], ptr(a), a.shape[0], int(criterion), ptr(out), stream_of()))
    return out.cpu().numpy()


def _assert_bits(got, want, ctx):
    bad = np.nonzero(F.bits(got) != F.bits(want))
    assert bad[0].size == 0, (ctx, bad[0].size, bad[0][:6], bad[1][:6], got[bad][:6], want[bad][:6])


# ----------------------------------------------------------------------------------------------------------- matrix
@pytest.mark.parametrize("criterion", F.CRITERIA)
def test_matrix_lattice_families_at_tile_edges(dev, criterion):
    R, C, idx = F.family_matrix()
    names, Rp, Cp = F.pair_families()
    for clamps in F.CLAMP_SETS:
        for only_xy in (False, True):
            want = F.exact_iou(Rp, Cp, clamps, criterion, only_xy)[np.ix_(idx, idx)]
            for n in F.MATRIX_SIZES:
                for k in F.MATRIX_SIZES:
                    got = iou_3d(dev, R[:n], C[:k], clamps, criterion, only_xy)
                    _assert_bits(got, want[:n, :k], (clamps, only_xy, n, k))
    want = F.exact_iou(Rp, Cp, F.CLAMP_SETS[0], criterion, True)[np.ix_(idx, idx)]
    for n in F.MATRIX_SIZES:
        for k in F.MATRIX_SIZES:
            _assert_bits(iou_eval(dev, R[:n], C[:k], criterion), want[:n, :k], ("eval", n, k))
    # the transposed roles: the column box's extents never choose the criterion-2 branch, the row box's do
    wt = F.exact_iou(Cp, Rp, F.CLAMP_SETS[1], criterion)[np.ix_(idx, idx)]
    _assert_bits(iou_3d(dev, C, R, F.CLAMP_SETS[1], criterion), wt, "transposed")


@pytest.mark.parametrize("clamps", F.CLAMP_SETS)
def test_matrix_random_lattice(dev, clamps):
    a, b = F.random_lattice(200, 1), F.random_lattice(300, 2)
    for criterion in F.CRITERIA:
        _assert_bits(iou_3d(dev, a, b, clamps, criterion), F.exact_iou(a, b, clamps, criterion), (clamps, criterion))
    _assert_bits(iou_eval(dev, a, b, 2), F.exact_iou(a, b, F.CLAMP_SETS[0], 2, True), "eval")


def test_matrix_rotated_families_against_the_oracle(dev):
    """the project's contract on rotated boxes: 1e-4 x max(1, |want|) on every element, NaN where the oracle has NaN,
    fewer than 1e-3 of the elements differing in bits (measured: see the module's docstring)"""
    import oracle
    from tests import nms_forms
    total = differ = 0
    worst = ("", 0.0)
    for name, f in nms_forms.families().items():
        if name in ("tiny_sizes_clamped", "non_finite_clamped"):            # the NMS's own clamp variants
            continue
        for clamps, criterion in ((F.CLAMP_SETS[0], -1), (F.CLAMP_SETS[1], 2)):
            want = oracle.boxes_iou_3d(f["a"], f["b"], F.aug_dict(clamps), criterion)
            got = iou_3d(dev, f["a"], f["b"], clamps, criterion)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan), (name, criterion, int((np.isnan(got) != nan).sum()))
            ok = ~nan & np.isfinite(want)
            assert np.array_equal(got[~nan & ~ok], want[~nan & ~ok]), name                     # infinities
            err = np.abs(got[ok].astype(np.float64) - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
            if err.size and err.max() > worst[1]:
                worst = (name, float(err.max()))
            assert err.size == 0 or err.max() <= 1e-4, (name, criterion, float(err.max()))
            total += want.size
            differ += int((~F.same_bits(got, want)).sum())
    print("rotated families: %d of %d elements differ in bits (%.3g); largest error %.3g in %s"
          % (differ, total, differ / total, worst[1], worst[0]))
    assert differ < 1e-3 * total, (differ, total)


# ---------------------------------------------------------------------------------------------------------- matcher
def run_match(dev, sc, m, want_reg=True):
    from detection_3d_amd import box_ops
    matched, reg = box_ops.match_segments(_t(dev, sc["gt"]), sc["off"], _t(dev, sc["pred"]), _t(dev, sc["seg"], np.int32),
                                          F.aug_dict(m["clamps"]), criterion=m["criterion"], yaw_threshold=m["yaw"],
                                          high=m["high"], low=m["low"], allow_low_quality=m["lq"],
                                          encode_weights=m["weights"], want_reg=want_reg)
    return matched.cpu().numpy(), None if reg is None else reg.cpu().numpy()


def _assert_match(got, reg, e, ctx, nan_ok=False):
    bad = np.nonzero(got != e["matched"])[0]
    assert bad.size == 0, (ctx, bad.size, bad[:8], got[bad[:8]], e["matched"][bad[:8]])
    same = F.same_bits(reg, e["reg"]) if nan_ok else F.bits(reg) == F.bits(e["reg"])
    bad = np.nonzero(~same)
    assert bad[0].size == 0, (ctx, bad[0].size, bad[0][:6], bad[1][:6], reg[bad][:6], e["reg"][bad][:6])


@pytest.mark.parametrize("mode", sorted(F.MODES))
@pytest.mark.parametrize("name", F.SCENE_NAMES)
def test_match_scenes(dev, name, mode):
    sc, e = F.scene(name), F.expect(name, mode)
    got, reg = run_match(dev, sc, F.MODES[mode])
    _assert_match(got, reg, e, (name, mode))


def test_scratch_padding_and_no_reg(dev):
    """d3d_match_segments on a scratch buffer of exactly the required size, filled with a pattern: the bytes between its
    three arrays and behind them stay as they were, the result does not depend on what the buffer held, and without a
    regression buffer `matched` is the same"""
    from detection_3d_amd import _lib
    from detection_3d_amd._lib import check, floats, lib, ptr, stream_of
    sc, m, e = F.scene("s5_chunks_sorted"), F.MODES["rpn"], F.expect("s5_chunks_sorted", "rpn")
    N, M, S = sc["pred"].shape[0], sc["gt"].shape[0], len(sc["off"]) - 1
    need = int(lib().d3d_match_segments_scratch_bytes(M, N))
    nb, mb = (N * 4 + 255) & ~255, (M * 4 + 255) & ~255
    assert need == 2 * nb + M * 4 and N * 4 < nb and M * 4 < mb
    guard = 4096
    gt, pred, seg = _t(dev, sc["gt"]), _t(dev, sc["pred"]), _t(dev, sc["seg"], np.int32)
    for with_reg in (True, False):
        buf = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=dev)
        matched = torch.full((N,), -7, dtype=torch.int32, device=dev)
        reg = torch.full((N, 7), -7.0, dtype=torch.float32, device=dev) if with_reg else None
        check(lib().d3d_match_segments(ptr(gt), _lib.ints(sc["off"]), S, ptr(pred), N, ptr(seg), floats(m["clamps"]),
                                       m["criterion"], float(m["yaw"]), float(m["high"]), float(m["low"]), 1,
                                       floats(m["weights"]), ptr(matched), ptr(reg), ptr(buf), need, stream_of()))
        torch.cuda.synchronize()
        b = buf.cpu().numpy()
        for lo, hi in ((N * 4, nb), (nb + N * 4, 2 * nb), (2 * nb + M * 4, need + guard)):
            assert (b[lo:hi] == 0xA5).all(), (with_reg, lo, hi)
        assert np.array_equal(matched.cpu().numpy(), e["matched"])
        if with_reg:
            assert np.array_equal(F.bits(reg.cpu().numpy()), F.bits(e["reg"]))
    got, reg = run_match(dev, sc, m, want_reg=False)
    assert reg is None and np.array_equal(got, e["matched"])


# ------------------------------------------------------------------------------------------------------- non-finite
@pytest.mark.parametrize("clamps", (F.CLAMP_SETS[0], F.CLAMP_SETS[2]))
def test_non_finite_matrix(dev, clamps):
    """NaN where the oracle has NaN, equal bits elsewhere.  With fmaxf clamps in load_box the cases gt[3]=nan, gt[5]=nan,
    pred[3]=nan, pred[5]=nan (and -nan) come out finite; with fminf / fmaxf on the z bounds in iou_pair so do gt[2]=nan
    and pred[2]=nan"""
    import oracle
    gt, pred, S, labels = F.non_finite_boxes()
    for criterion in (-1, 2):
        want = oracle.boxes_iou_3d(gt, pred, F.aug_dict(clamps), criterion)
        got = iou_3d(dev, gt, pred, clamps, criterion)
        bad = np.nonzero(~F.same_bits(got, want))
        where = sorted({labels[i // 3] for i, j in zip(*bad) if i // 3 == j // 3})      # in the variants' own blocks
        assert bad[0].size == 0, (criterion, bad[0].size, where[:12], got[bad][:6], want[bad][:6])


@pytest.mark.parametrize("mode", sorted(F.MODES))
def test_non_finite_matcher(dev, mode):
    """every variant is a segment of its own.  Besides the cases of test_non_finite_matrix, a quality that is a NaN with
    the sign bit set (pred[k]=-nan, gt[k]=-nan) must make its GT row's `highest` NaN as q.max(1) does:
    f32_ordered_nan_top has to put a NaN of either sign on top"""
    sc, e = F.scene("non_finite"), F.expect("non_finite", mode)
    got, reg = run_match(dev, sc, F.MODES[mode])
    _, _, _, labels = F.non_finite_boxes()
    bad = np.nonzero(got != e["matched"])[0]
    assert bad.size == 0, (mode, sorted({labels[p // 3] for p in bad}), got[bad[:8]], e["matched"][bad[:8]])
    _assert_match(got, reg, e, ("non_finite", mode), nan_ok=True)
