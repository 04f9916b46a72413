"""What the label-assignment and IoU-matrix tests share and a machine without a GPU can check (test_match_forms_cpu.py):
lattice boxes whose qualities are known as one fp32 bit pattern, an independent Matcher and box_encode in numpy, and scenes
that aim at every rule of the Matcher and every size edge of d3d_match_segments.  Imports neither torch nor the library.

Boxes are yx_zb rows (x, y, z0, d3, d4, dz, yaw); d3 is the extent along x at yaw 0.  The matrix entry of a row box
(target / GT) and a column box (anchor / prediction) is

    v = criterion(BEV intersection, area_col, area_row)         fp64 ratio of fp32 areas, rounded to fp32
    v = 1 if the five BEV fields (x, y, clamped d3, d4, yaw) agree  (check_same_boxes)
    v = v * (overlap / common)                                    fp32, the z intervals [z0, z0 + clamped dz]

LATTICE.  yaw = 0 and every coordinate, size and clamp a multiple of 1/8 with magnitude below 64: corners, areas and the
intersection rectangle are exact in fp32, the ratio is one correctly rounded fp64 quotient of exact operands
(fractions.Fraction -> float), and every later step is a single IEEE operation -- the expected value is one bit pattern
and no pair needs an allowance.  Criterion -1 is I / (A_col + A_row - I), 0 is I / A_col, 1 is I / A_row, 2 is
I / (A_row + max(0, A_col / 2 - I)) when the ROW box is "small" (fp32 min / max of its clamped extents < 0.25) and
criterion -1 otherwise.  d3 is clamped to at least the _Y value and dz to at least the _Z value, d4 never; targets and
anchors separately.

MATCHER.  matcher_np restates modeling/matcher.py over an [M, N] quality matrix: argmax with the lowest row on ties,
`< low` -> -1, `< high` -> -2 in fp32, the low-quality restore where q == highest (ties included) and the ignore rule
q > max(0.02, highest - 0.05) on would-be negatives; NaN as numpy gives it (a NaN maximum keeps its argmax, a NaN
`highest` restores and ignores nothing).  box_encode_np restates BoxCoder3D.encode in fp32, operation by operation.

SCENES.  ATOMS are small groups of GT rows and predictions in a cell of their own, each aimed at one rule, with the
outcome the rule must give ("designed") and the outcome without it ("naive"); rules_scene() holds each once, and the
size cases tile them, so every size edge carries real decisions.  Rotated predictions (the yaw-mask atom) have no exact
IoU: their columns come from the CPU oracle, and the builder asserts that each such value lies at least MARGIN = 4e-4
(four times the 1e-4 the project holds the kernel to against the oracle) from everything it is compared with."""
from fractions import Fraction

import numpy as np

U = 8                                   # lattice units per metre
LIMIT = 64 * U
MARGIN = 4e-4
F32 = np.float32

CLAMP_SETS = ((0.0, 0.0, 0.0, 0.0), (0.375, 0.75, 0.0, 0.0), (0.375, 0.75, 0.375, 0.75), (0.0, 0.0, 0.375, 0.75))
CRITERIA = (-1, 0, 1, 2)


def aug_dict(clamps):
    return dict(target_Y=clamps[0], target_Z=clamps[1], anchor_Y=clamps[2], anchor_Z=clamps[3])


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_bits(got, want):
    """elementwise: equal bit patterns, or both NaN"""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


# ------------------------------------------------------------------------------------------------- exact qualities
def _lattice(b, cy, cz):
    """float32 [n, 7] lattice rows -> int64 [n, 6] in units of 1/8 with d3 and dz clamped"""
    b = np.asarray(b, np.float64).reshape(-1, 7)
    v = b[:, :6] * U
    q = np.rint(v).astype(np.int64)
    assert np.array_equal(q, v) and np.all(b[:, 6] == 0) and np.all(np.abs(q) < LIMIT), "not a lattice box"
    ky, kz = cy * U, cz * U
    assert ky == int(ky) and kz == int(kz)
    q[:, 3] = np.maximum(q[:, 3], int(ky))
    q[:, 5] = np.maximum(q[:, 5], int(kz))
    return q


_RATIO = {}


def _ratio(criterion, I, ar, ac, small):
    """the criterion's exact ratio, rounded to fp64 and then to fp32 as the contract does.  I, ar (row area), ac (column
    area) are integers in units of 1 / (16 * 16)"""
    key = (criterion, I, ar, ac, small)
    if key not in _RATIO:
        I_, ar_, ac_ = Fraction(I), Fraction(ar), Fraction(ac)
        iou = I_ / (ac_ + ar_ - I_)
        if criterion == -1:
            r = iou
        elif criterion == 0:
            r = I_ / ac_
        elif criterion == 1:
            r = I_ / ar_
        elif criterion == 2:
            r = I_ / (ar_ + max(Fraction(0), ac_ / 2 - I_)) if small else iou
        else:
            raise ValueError(criterion)
        _RATIO[key] = F32(float(r))
    return _RATIO[key]


def exact_iou(rows, cols, clamps=(0.0, 0.0, 0.0, 0.0), criterion=-1, only_xy=False):
    """the one fp32 value the contract gives for every (row, column) pair of lattice boxes -> float32 [M, N]"""
    r, c = _lattice(rows, clamps[0], clamps[1]), _lattice(cols, clamps[2], clamps[3])
    M, N = r.shape[0], c.shape[0]
    out = np.zeros((M, N), F32)
    if M == 0 or N == 0:
        return out
    # bounds in units of 1/16 (half sizes stay integers)
    ix = (np.minimum((2 * r[:, 0] + r[:, 3])[:, None], (2 * c[:, 0] + c[:, 3])[None])
          - np.maximum((2 * r[:, 0] - r[:, 3])[:, None], (2 * c[:, 0] - c[:, 3])[None]))
    iy = (np.minimum((2 * r[:, 1] + r[:, 4])[:, None], (2 * c[:, 1] + c[:, 4])[None])
          - np.maximum((2 * r[:, 1] - r[:, 4])[:, None], (2 * c[:, 1] - c[:, 4])[None]))
    ar, ac = 4 * r[:, 3] * r[:, 4], 4 * c[:, 3] * c[:, 4]
    assert np.all(ar > 0) and np.all(ac > 0), "zero area"
    d3, d4 = (r[:, 3] / U).astype(F32), (r[:, 4] / U).astype(F32)
    small = (np.minimum(d3, d4) / np.maximum(d3, d4)) < F32(0.25)                    # the fp32 quotient
    for i, j in zip(*np.nonzero((ix > 0) & (iy > 0))):
        out[i, j] = _ratio(criterion, int(ix[i, j] * iy[i, j]), int(ar[i]), int(ac[j]), bool(small[i]))
    same = np.ones((M, N), bool)
    for k in (0, 1, 3, 4):
        same &= r[:, k][:, None] == c[:, k][None]
    out[same] = F32(1.0)
    if not only_xy:
        rz0, cz0 = (r[:, 2] / U).astype(F32), (c[:, 2] / U).astype(F32)
        rz1, cz1 = rz0 + (r[:, 5] / U).astype(F32), cz0 + (c[:, 5] / U).astype(F32)
        overlap = np.minimum(cz1[None], rz1[:, None]) - np.maximum(cz0[None], rz0[:, None])
        common = np.maximum(cz1[None], rz1[:, None]) - np.minimum(cz0[None], rz0[:, None])
        out = out * (overlap / common)
    return out.astype(F32)


def rows_from_units(q):
    """integer rows (x, y, z0, d3, d4, dz) in units of 1/8 -> float32 [n, 7], yaw 0"""
    q = np.asarray(q, np.int64).reshape(-1, 6)
    b = np.zeros((q.shape[0], 7), F32)
    b[:, :6] = q.astype(np.float64) / U
    return b


def random_lattice(n, seed, span=24):
    """n random lattice boxes in a span x span x 4 region: many overlap, many share an edge line, many z intervals miss"""
    rng = np.random.RandomState(seed)
    q = np.zeros((n, 6), np.int64)
    q[:, 0:2] = rng.randint(4 * U, (4 + span) * U, (n, 2))
    q[:, 2] = rng.randint(0, 4 * U, n)
    q[:, 3:5] = rng.randint(1, 8 * U, (n, 2))
    q[:, 5] = rng.randint(1, 2 * U, n)
    q[::5, 0] = (q[::5, 0] // (2 * U)) * 2 * U                  # coarser centres and sizes: collinear edges
    q[::5, 3] = np.maximum(2 * U, (q[::5, 3] // (2 * U)) * 2 * U)
    return rows_from_units(q)


# ------------------------------------------------------------------------------------------- families for the matrix
def pair_families():
    """-> (names [P], rows float32 [P, 7], cols float32 [P, 7]): hard pair p is (rows[p], cols[p]).  All sit around one
    spot, so that the other entries of a matrix built from them are mostly non-trivial as well."""
    X, Y = 8 * U, 8 * U
    B = (X, Y, 0, 3 * U, U, U)
    fam = []

    def add(name, row, col):
        fam.append((name, row, col))

    def moved(b, dx=0, dy=0, dz=0, **size):
        return (b[0] + dx, b[1] + dy, b[2] + dz, size.get("d3", b[3]), size.get("d4", b[4]), size.get("dzz", b[5]))

    add("identical_equal_z", B, B)
    add("identical_shifted_z", B, moved(B, dz=U // 2))
    add("identical_touching_z", B, moved(B, dz=U))
    add("identical_disjoint_z", B, moved(B, dz=2 * U))
    add("touch_x", B, moved(B, dx=3 * U))
    add("touch_y", B, moved(B, dy=U))
    add("touch_corner", B, moved(B, dx=3 * U, dy=U))
    add("touch_x_other_side", moved(B, dx=3 * U), B)
    add("shared_edge_part", B, moved(B, dx=3 * U, dy=U // 2))
    add("col_contained", B, moved(B, dx=2, d3=U, d4=U // 2))
    add("row_contained", moved(B, dx=-3, d3=U, d4=U // 2), B)
    add("crossing", B, moved(B, d3=U, d4=3 * U))
    add("ratio_quarter_row", moved(B, d3=4 * U, d4=U), moved(B, dx=U))
    add("ratio_below_row", moved(B, d3=4 * U, d4=U - 1), moved(B, dx=U))
    add("ratio_above_row", moved(B, d3=4 * U, d4=U + 1), moved(B, dx=U))
    add("ratio_quarter_col", moved(B, dx=U), moved(B, d3=4 * U, d4=U))
    add("ratio_below_col", moved(B, dx=U), moved(B, d3=4 * U, d4=U - 1))
    add("ratio_above_col", moved(B, dx=U), moved(B, d3=4 * U, d4=U + 1))
    add("ratio_below_row_tall", moved(B, d3=U - 1, d4=4 * U), moved(B, dx=2))
    add("row_d3_below_clamp", moved(B, d3=2, d4=2 * U), moved(B, dx=1, d3=2, d4=2 * U))
    add("col_d3_below_clamp", moved(B, dx=1), moved(B, d3=2, d4=2 * U))
    add("both_d3_below_clamp_same", moved(B, d3=1, d4=U), moved(B, d3=2, d4=U))
    add("row_dz_below_clamp", moved(B, dzz=U // 2), moved(B, dx=U, dz=U // 2))
    add("col_dz_below_clamp", moved(B, dx=U), moved(B, dzz=2, dz=U - 2))
    add("apart_z_overlaps", B, moved(B, dx=5 * U, dz=2))
    add("apart_z_disjoint", B, moved(B, dx=5 * U, dy=3 * U, dz=3 * U))
    add("overlap_z_touching", B, moved(B, dx=U, dz=U))
    add("overlap_z_apart", B, moved(B, dx=U, dz=3 * U))
    add("overlap_z_apart_below", B, moved(B, dx=-U, dy=2, dz=-3 * U))
    names = [f[0] for f in fam]
    return names, rows_from_units([f[1] for f in fam]), rows_from_units([f[2] for f in fam])


MATRIX_SIZES = (1, 63, 64, 65, 129)


def family_matrix(n=129):
    """rows / cols of an n x n matrix that holds hard pair p at every (p + a P, p + b P): with P < 32 and n = 129 each
    pair sits in tile (0, 0), in (1, 1) and across both tile edges; the top-left N x K corner serves the smaller sizes"""
    names, R, C = pair_families()
    P = len(names)
    assert P < 32 and 64 % P != 0
    idx = np.arange(n) % P
    return R[idx], C[idx], idx


NF_GT, NF_PRED = 3, 3


def non_finite_boxes():
    """-> (gt float32 [S * 3, 7], pred float32 [S * 3, 7], S, labels): variant s = GT rows 3 s .. 3 s + 2 and predictions
    3 s .. 3 s + 2 with ONE field of its first GT row or its first prediction replaced by NaN, -NaN, +Inf or -Inf.  The
    third GT row's best finite quality is a weak one with the third prediction: restored by the low-quality rule when
    the row's `highest` is finite, left alone when a NaN in the row makes it NaN"""
    g = rows_from_units([(2 * U, 12, 0, 3 * U, U, U), (2 * U + 4, 12, 0, 3 * U, U, U), (2 * U + 28, 12, 0, 3 * U, U, U)])
    p = rows_from_units([(2 * U, 12, 0, 3 * U, U, U), (2 * U + 7, 12, 0, 3 * U, U, U), (2 * U + 12, 12, 2, 3 * U, U, U)])
    neg_nan = np.array([0xffc00000], np.uint32).view(F32)[0]
    gts, preds, labels = [], [], []
    for side in ("gt", "pred"):
        for k in range(7):
            for name, val in (("nan", F32(np.nan)), ("-nan", neg_nan), ("inf", F32(np.inf)), ("-inf", F32(-np.inf))):
                gg, pp = g.copy(), p.copy()
                (gg if side == "gt" else pp)[0, k] = val
                gts.append(gg)
                preds.append(pp)
                labels.append("%s[%d]=%s" % (side, k, name))
    return np.concatenate(gts), np.concatenate(preds), len(labels), labels


# ----------------------------------------------------------------------------------------------- Matcher, box_encode
def matcher_np(q, high, low, allow_low_quality):
    """modeling/matcher.py over q float32 [M >= 1, N] -> int64 [N]: row of the matched GT, -1 below `low`, -2 between"""
    q = np.asarray(q, F32)
    assert q.ndim == 2 and q.shape[0] >= 1
    with np.errstate(invalid="ignore"):
        best = q.max(axis=0)                                  # NaN propagates, as torch.max(dim=0)
        arg = q.argmax(axis=0).astype(np.int64)               # first maximum; the first NaN if there is one
        out = arg.copy()
        below = best < F32(low)
        out[below] = -1
        out[~below & (best < F32(high))] = -2
        if allow_low_quality:
            highest = q.max(axis=1)
            tie = (q == highest[:, None]).any(axis=0)
            out[tie] = arg[tie]
            thr = np.maximum(F32(0.02), highest - F32(0.05))  # np.maximum keeps a NaN, as torch.max
            near = (q > thr[:, None]).any(axis=0)
            out[near & (out == -1)] = -2
    return out


PI32 = F32(3.14159265358979323846)
INV_PI32 = F32(1.0) / PI32


def limit_period_np(v, offset=0.5):
    v = np.asarray(v, F32)
    return v - np.floor(v * INV_PI32 + F32(offset)) * PI32


def box_encode_np(g, a, w):
    """BoxCoder3D.encode (smooth_dim) of targets g on anchors a, both float32 [n, 7], in fp32, operation by operation"""
    g, a, w = np.asarray(g, F32), np.asarray(a, F32), np.asarray(w, F32)
    with np.errstate(all="ignore"):
        diag = np.sqrt(a[:, 4] * a[:, 4] + a[:, 3] * a[:, 3])
        e = np.stack([(g[:, 0] - a[:, 0]) / diag, (g[:, 1] - a[:, 1]) / diag, (g[:, 2] - a[:, 2]) / a[:, 5],
                      g[:, 3] / a[:, 3] - F32(1), g[:, 4] / a[:, 4] - F32(1), g[:, 5] / a[:, 5] - F32(1),
                      limit_period_np(g[:, 6] - a[:, 6])], axis=1)
        return (e * w[None]).astype(F32)


# ------------------------------------------------------------------------------------------------------------ modes
MODES = {
    # RPN labels: criterion 2, yaw mask, low-quality matches, the targets' clamps only
    "rpn": dict(criterion=2, yaw=0.7, lq=True, high=0.5, low=0.3, clamps=CLAMP_SETS[1], weights=(1.0,) * 7),
    # RoI labels: criterion -1, no mask, no low-quality matches, both clamps, encode weights
    "roi": dict(criterion=-1, yaw=4.0, lq=False, high=0.5, low=0.3, clamps=CLAMP_SETS[2],
                weights=(10.0, 10.0, 10.0, 5.0, 5.0, 5.0, 3.0)),
    # one threshold: nothing is "between" but what the ignore rule puts there
    "eq": dict(criterion=-1, yaw=4.0, lq=True, high=0.5, low=0.5, clamps=CLAMP_SETS[0], weights=(1.0,) * 7),
}
YAW_T = F32(0.7)
YAW_BELOW, YAW_ABOVE = np.nextafter(YAW_T, F32(0)), np.nextafter(YAW_T, F32(1))


def yaw_mask(gt, pred, thr):
    with np.errstate(invalid="ignore"):
        d = np.abs(limit_period_np(gt[:, 6][:, None] - pred[:, 6][None]))
        return (d < F32(thr)).astype(F32)


def quality(gt, pred, mode, check_margin=True):
    """the Matcher's input for one segment: exact on lattice columns, the oracle's on rotated or non-finite ones (with
    the margin asserted for every unmasked finite value among them), times the yaw mask"""
    m = MODES[mode] if isinstance(mode, str) else mode
    gt, pred = np.asarray(gt, F32), np.asarray(pred, F32)
    q = np.zeros((gt.shape[0], pred.shape[0]), F32)
    lat_g = np.isfinite(gt).all(axis=1) & (gt[:, 6] == 0)
    lat_p = np.isfinite(pred).all(axis=1) & (pred[:, 6] == 0)
    exact = lat_g[:, None] & lat_p[None]
    if lat_g.any() and lat_p.any():
        q[np.ix_(lat_g, lat_p)] = exact_iou(gt[lat_g], pred[lat_p], m["clamps"], m["criterion"])
    if not exact.all():
        import oracle
        o = oracle.boxes_iou_3d(gt, pred, aug_dict(m["clamps"]), m["criterion"])
        q = np.where(exact, q, o)
    with np.errstate(invalid="ignore"):
        if not m["yaw"] > 1.58:
            q = q * yaw_mask(gt, pred, m["yaw"])
        if check_margin and not exact.all():
            _assert_margin(q, ~exact & np.isfinite(q) & (q != 0), m)
    return q.astype(F32)


def _assert_margin(q, soft, m):
    """every inexact non-zero quality keeps MARGIN to all it is compared with: the thresholds, the other entries of its
    column, its row's maximum (which it is not), that maximum - 0.05, and 0.02"""
    q64 = q.astype(np.float64)
    for i, j in zip(*np.nonzero(soft)):
        v = q64[i, j]
        others = np.delete(q64[:, j], i)
        row_max = np.nanmax(np.delete(q64[i], j)) if q.shape[1] > 1 else -np.inf
        against = [m["low"], m["high"], 0.02, row_max, row_max - 0.05] + others[np.isfinite(others)].tolist()
        gap = min(abs(v - x) for x in against)
        assert gap >= MARGIN and v < row_max, ("margin", i, j, v, gap, row_max)


# ------------------------------------------------------------------------------------------------------------ atoms
# GT rows (x, y, z0, d3, d4, dz) and predictions (x, y, z0, d3, d4, dz, yaw, designed, naive, rule) relative to a cell's
# corner, lengths in units of 1/8.  designed / naive: the outcome in mode "rpn" of rules_scene() (local GT row, -1, -2)
# with the rule and without it.  The first prediction of an atom is the one its GT rows need most.
CELL_X, CELL_Y, CELL_Z = 8 * U, 4 * U, 4 * U
# jitter stays below 64; 7 x 14 cells per layer: the atom above or below another one is 8 k places further in ATOM_ORDER, so the
# rotated predictions of "yaw" never face the two identical rows of "dup_gt" (equal entries in an inexact column)
CELLS_X, CELLS_Y, CELLS_Z = LIMIT // CELL_X - 1, LIMIT // CELL_Y - 2, LIMIT // CELL_Z - 1
GX, GY = 2 * U, 12                       # the GT's centre in its cell
G31 = (GX, GY, 0, 3 * U, U, U)           # 3 x 1 x 1: shifted by s along x, IoU = (3 - s) / (3 + s)


def _p(dx=0, dy=0, z0=0, d3=3 * U, d4=U, dz=U, yaw=0.0, want=None, naive=None, rule=""):
    return (GX + dx, GY + dy, z0, d3, d4, dz, yaw, want, want if naive is None else naive, rule)


ATOMS = {
    "half": ([G31], [
        _p(0, want=0, rule="on_top"),
        _p(U, want=0, naive=-2, rule="exactly_high"),                    # 2 / 4 == high: not below it
        _p(U - 1, want=0, rule="step_above_high"),                       # 17 / 31
        _p(U + 1, want=-2, rule="step_below_high")]),                    # 15 / 33
    "low": ([(GX, GY, 0, 13, U, U)], [                                    # 13/8 x 1: shift 7/8 gives 6 / 20 = 3 / 10
        _p(0, d3=13, want=0, rule="on_top"),
        _p(7, d3=13, want=-2, naive=-1, rule="exactly_low"),             # fp32(3 / 10) == fp32(0.3): between
        _p(6, d3=13, want=-2, rule="step_above_low"),                    # 7 / 19
        _p(8, d3=13, want=-1, rule="step_below_low")]),                  # 5 / 21
    "dup_gt": ([G31, G31], [
        _p(0, want=0, naive=1, rule="duplicate_gt"),
        _p(1, want=0, naive=1, rule="duplicate_gt")]),                   # 23 / 25 with both rows
    "dup_pred": ([G31], [
        _p(U + 1, want=0, naive=-2, rule="duplicate_pred_restored"),     # 15 / 33 is this GT's best, twice
        _p(U + 1, want=0, naive=-2, rule="duplicate_pred_restored")]),
    "restore": ([G31], [
        _p(2 * U, want=0, naive=-1, rule="best_below_low_restored"),     # 1 / 5; ignore threshold 0.2 - 0.05
        _p(2 * U + 1, want=-2, naive=-1, rule="ignored_inside"),         # 7 / 41 = 0.1707 > 0.15
        _p(2 * U + 2, want=-1, rule="ignored_outside")]),                # 6 / 42 = 0.1429
    "floor": ([G31], [
        _p(22, want=0, naive=-1, rule="best_below_low_restored"),        # 2 / 46; highest - 0.05 < 0: the floor 0.02
        _p(23, want=-2, naive=-1, rule="floor_inside"),                  # 1 / 47 = 0.0213
        _p(23, d4=2 * U, want=-1, rule="floor_outside")]),               # 1 / 71 = 0.0141
    "neg": ([G31], [
        _p(0, want=0, rule="on_top"),
        _p(0, z0=2 * U, want=-1, rule="negative_only"),                  # same BEV, z apart: 1 x (-1 / 3)
        _p(0, z0=U, want=-1, rule="z_touching")]),                       # 1 x (0 / 2)
    "yaw": ([(GX, GY, 0, 2 * U, 2 * U, U)], [
        _p(0, d3=2 * U, d4=2 * U, want=0, rule="on_top"),
        _p(0, d3=2 * U, d4=2 * U, yaw=YAW_T, want=-1, naive=0, rule="yaw_at_threshold"),
        _p(0, d3=2 * U, d4=2 * U, yaw=YAW_BELOW, want=0, rule="yaw_step_below"),
        _p(0, d3=2 * U, d4=2 * U, yaw=YAW_ABOVE, want=-1, naive=0, rule="yaw_step_above"),
        _p(0, d3=2 * U, d4=2 * U, yaw=-YAW_T, want=-1, naive=0, rule="yaw_at_threshold"),
        _p(0, d3=2 * U, d4=2 * U, yaw=-YAW_BELOW, want=0, rule="yaw_step_below"),
        _p(0, d3=2 * U, d4=2 * U, yaw=-YAW_ABOVE, want=-1, naive=0, rule="yaw_step_above")]),
    "wall": ([(GX, GY, 0, 4 * U, U - 1, U)], [                            # extents ratio 7 / 32: "small" under criterion 2
        _p(0, d3=4 * U, d4=U - 1, want=0, rule="on_top"),
        _p(2 * U, d3=4 * U, d4=U - 1, want=0, naive=-2, rule="criterion2_small"),       # 1 / 2 there, IoU 1 / 3
        _p(2 * U + 1, d3=4 * U, d4=U - 1, want=-2, rule="criterion2_small_below")]),    # 105 / 231
    "thin": ([(GX, GY, 0, 2, 2 * U, U // 2)], [                           # d3 and dz below the targets' clamps
        _p(0, d3=2, d4=2 * U, dz=U // 2, want=0, naive=-2, rule="clamped_one_side")]),   # (2 / 3) x fp32(2 / 3), restored
}
ATOM_ORDER = ("half", "low", "dup_gt", "dup_pred", "restore", "floor", "neg", "yaw", "wall", "thin")
RULES = sorted({p[9] for _, ps in ATOMS.values() for p in ps})


def _cell(c):
    assert 0 <= c < CELLS_X * CELLS_Y * CELLS_Z, "out of cells"
    return (c % CELLS_X) * CELL_X, ((c // CELLS_X) % CELLS_Y) * CELL_Y, (c // (CELLS_X * CELLS_Y)) * CELL_Z


def _place(name, c):
    """atom `name` in cell c -> (gt float32 [g, 7], pred float32 [p, 7], tags [(rule, designed, naive)])"""
    ox, oy, oz = _cell(c)
    gts, preds = ATOMS[name]
    g = rows_from_units([(x + ox, y + oy, z + oz, a, b, d) for x, y, z, a, b, d in gts])
    p = rows_from_units([(t[0] + ox, t[1] + oy, t[2] + oz, t[3], t[4], t[5]) for t in preds])
    p[:, 6] = [t[6] for t in preds]
    return g, p, [(t[9], t[7], t[8]) for t in preds]


def _segment(m, n, cells, rng):
    """m GT rows and n predictions: atoms in turn, one cell each; the atoms' first predictions come first, then their
    others, then jittered copies of the GT rows until there are n (fewer than the atoms hold: the tail is cut)"""
    gts, first, rest = [], [], []
    while sum(g.shape[0] for g in gts) < m:
        name = ATOM_ORDER[cells[0] % len(ATOM_ORDER)]
        if len(ATOMS[name][0]) > m - sum(g.shape[0] for g in gts):
            name = "half"
        g, p, _ = _place(name, cells[0])
        cells[0] += 1
        gts.append(g)
        first.append(p[:1])
        rest.append(p[1:])
    gt = np.concatenate(gts) if gts else np.zeros((0, 7), F32)
    pred = np.concatenate(first + rest) if gts else np.zeros((0, 7), F32)
    extra = n - pred.shape[0]
    if extra > 0:
        if m:
            base = gt[np.arange(extra) % m].copy()
        else:
            ox, oy, oz = _cell(cells[0])
            cells[0] += 1
            base = np.tile(rows_from_units([(GX + ox, GY + oy, oz, 3 * U, U, U)]), (extra, 1))
        base[:, 0] += rng.randint(-2 * U, 2 * U + 1, extra) / F32(U)
        base[:, 1] += rng.randint(-U, U + 1, extra) / F32(U)
        base[:, 2] += rng.choice([0, 0, 0, 2, -4, U], extra) / F32(U)
        base[:, 3] = np.maximum(base[:, 3] + rng.choice([0, 0, -4, 4], extra) / F32(U), F32(1.0 / U))
        pred = np.concatenate([pred, base.astype(F32)])
    return gt, pred[:n]


def _order(seg, kind, rng):
    n = seg.shape[0]
    if kind == "sorted":
        return np.arange(n)
    if kind == "interleaved":                                  # round robin over the segments
        rank = np.zeros(n, np.int64)
        for s in np.unique(seg):
            rows = np.nonzero(seg == s)[0]
            rank[rows] = np.arange(rows.size)
        return np.lexsort((seg, rank))
    if kind == "permuted":
        return rng.permutation(n)
    raise ValueError(kind)


def make_scene(name, gt_counts, pred_counts, order="sorted", seed=0, stray=()):
    """segments with gt_counts[s] GT rows and pred_counts[s] predictions; `stray`: segment ids outside [0, S) given to
    that many further predictions -> dict(name, gt, off, pred, seg)"""
    assert len(gt_counts) == len(pred_counts)
    rng = np.random.RandomState(seed)
    cells = [0]
    gts, preds, segs, off = [], [], [], [0]
    for s, (m, n) in enumerate(zip(gt_counts, pred_counts)):
        g, p = _segment(m, n, cells, rng)
        gts.append(g)
        preds.append(p)
        segs.append(np.full(p.shape[0], s, np.int32))
        off.append(off[-1] + m)
    if stray:
        g, p = _segment(0, len(stray), cells, rng)
        preds.append(p)
        segs.append(np.asarray(stray, np.int32))
    gt, pred, seg = np.concatenate(gts), np.concatenate(preds), np.concatenate(segs)
    o = _order(seg, order, rng)
    return dict(name=name, gt=np.ascontiguousarray(gt, F32), off=off, pred=np.ascontiguousarray(pred[o], F32),
                seg=np.ascontiguousarray(seg[o], np.int32))


def rules_scene():
    """every atom once, one cell each, one segment -> scene with tags[p] = (rule, designed, naive), the designed and naive
    outcomes as GT rows of the scene"""
    gts, preds, tags, m = [], [], [], 0
    for c, name in enumerate(ATOM_ORDER):
        g, p, t = _place(name, c)
        gts.append(g)
        preds.append(p)
        tags += [(rule, want + m if want >= 0 else want, naive + m if naive >= 0 else naive) for rule, want, naive in t]
        m += g.shape[0]
    pred = np.concatenate(preds)
    return dict(name="rules", gt=np.concatenate(gts), off=[0, m], pred=pred, seg=np.zeros(pred.shape[0], np.int32),
                tags=tags)


def lonely_scene():
    """a GT row without any prediction near it: its `highest` is 0, so every prediction whose quality with it is +-0 --
    all of them -- ties it and gets its own argmax back, whatever the thresholds say (matcher.py:131-147 as it is)"""
    sc = rules_scene()
    ox, oy, oz = _cell(len(ATOM_ORDER) + 3)
    far = rows_from_units([(GX + ox, GY + oy, oz, 3 * U, U, U)])
    gt = np.concatenate([sc["gt"][:3], far, sc["gt"][3:]])
    return dict(name="lonely_gt", gt=gt, off=[0, gt.shape[0]], pred=sc["pred"], seg=sc["seg"])


def cross_block_scene():
    """one segment over three blocks of 256 predictions: row 0's best prediction (15 / 33, restored) is the last
    prediction of the launch, and a tie for it is the first; a second segment shares the blocks"""
    sc = make_scene("cross_block", [40, 30], [420, 180], "interleaved", seed=11)
    ox, oy, oz = _cell(200)
    g = rows_from_units([(GX + ox, GY + oy, oz, 3 * U, U, U)])
    tie = rows_from_units([(GX + ox + U + 1, GY + oy, oz, 3 * U, U, U)])
    near = rows_from_units([(GX + ox + 2 * U + 2, GY + oy, oz, 3 * U, U, U)])           # 6 / 42: a would-be negative
    sc["gt"] = np.concatenate([g, sc["gt"]])
    sc["off"] = [0] + [o + 1 for o in sc["off"][1:]]
    sc["pred"] = np.concatenate([tie, sc["pred"][:300], near, sc["pred"][300:], tie])
    sc["seg"] = np.concatenate([[0], sc["seg"][:300], [0], sc["seg"][300:], [0]]).astype(np.int32)
    assert sc["pred"].shape[0] == 603 and sc["seg"][0] == 0 and sc["seg"][-1] == 0
    return sc


def non_finite_scene():
    gt, pred, S, _ = non_finite_boxes()
    return dict(name="non_finite", gt=gt, off=list(range(0, NF_GT * S + 1, NF_GT)), pred=pred,
                seg=np.repeat(np.arange(S, dtype=np.int32), NF_PRED))


def _s256_counts():
    g = [(0, 1, 2, 1, 0, 3, 1, 2)[s % 8] for s in range(256)]
    g[0] = g[1] = g[128] = g[129] = g[254] = g[255] = 0                # empty segments first, in the middle and last
    p = [3 * g[s] + 1 for s in range(256)]
    return g, p


SCENE_SPECS = {
    # name: (GT rows per segment, predictions per segment, order, stray ids)
    "n1_m1": ([1], [1], "sorted", ()),
    "n255": ([85], [255], "sorted", ()),
    "n256": ([85], [256], "sorted", ()),
    "n257": ([86], [257], "permuted", ()),
    "n513": ([170], [513], "permuted", ()),
    "m255": ([255], [760], "sorted", ()),
    "m256": ([256], [770], "permuted", ()),
    "m257": ([257], [780], "sorted", ()),
    "m513": ([513], [1499], "permuted", ()),
    "n513_m1": ([1], [513], "sorted", ()),
    "n257_m513": ([513], [257], "sorted", ()),                         # most GT rows without a prediction of their own
    "s2_empty_first": ([0, 257], [300, 760], "sorted", ()),            # block 0: no row has GT
    "s2_empty_last": ([256, 0], [760, 256], "interleaved", ()),
    "s5_empty_middle": ([255, 0, 256, 0, 1], [600, 30, 650, 20, 13], "interleaved", ()),
    "s5_chunks_shared": ([140, 1, 257, 0, 200], [400, 10, 700, 40, 340], "permuted", ()),   # GT rows in 3 chunks
    "s5_chunks_sorted": ([60, 130, 257, 0, 20], [175, 380, 750, 11, 60], "sorted", ()),
    "s256": _s256_counts() + ("permuted", ()),
    "s256_sorted": _s256_counts() + ("sorted", ()),
    "stray_ids": ([12, 24], [100, 150], "interleaved", (-1, 2, 1000, -2147483648, 2147483647, 256, -1)),
}
SCENE_NAMES = ("rules", "lonely_gt", "cross_block") + tuple(SCENE_SPECS)
_SCENES = {}


def scene(name):
    """the scene `name`, built once and left unchanged"""
    if name not in _SCENES:
        if name == "rules":
            sc = rules_scene()
        elif name == "lonely_gt":
            sc = lonely_scene()
        elif name == "cross_block":
            sc = cross_block_scene()
        elif name == "non_finite":
            sc = non_finite_scene()
        else:
            g, p, order, stray = SCENE_SPECS[name]
            sc = make_scene(name, g, p, order, seed=len(name) + sum(g), stray=stray)
        assert sc["pred"].shape[0] < 1500 and sc["gt"].shape[0] < 1300 and len(sc["off"]) - 1 <= 256
        for a in (sc["gt"], sc["pred"], sc["seg"]):
            a.setflags(write=False)
        _SCENES[name] = sc
    return _SCENES[name]


_EXPECT = {}


def expect(name, mode):
    """-> dict(matched int32 [N] (global GT rows, -1, -2), reg float32 [N, 7], q: the per-segment quality matrices)"""
    key = (name, mode if isinstance(mode, str) else id(mode))
    if key in _EXPECT:
        return _EXPECT[key]
    sc, m = scene(name), (MODES[mode] if isinstance(mode, str) else mode)
    N, S = sc["pred"].shape[0], len(sc["off"]) - 1
    matched = np.full(N, -1, np.int32)
    reg = np.zeros((N, 7), F32)
    qs = {}
    for s in range(S):
        lo, hi = sc["off"][s], sc["off"][s + 1]
        rows = np.nonzero(sc["seg"] == s)[0]
        if hi == lo or rows.size == 0:
            continue
        q = quality(sc["gt"][lo:hi], sc["pred"][rows], m, check_margin=name != "non_finite")
        loc = matcher_np(q, m["high"], m["low"], m["lq"])
        matched[rows] = np.where(loc >= 0, loc + lo, loc)
        reg[rows] = box_encode_np(sc["gt"][np.maximum(loc, 0) + lo], sc["pred"][rows], m["weights"])
        qs[s] = q
    _EXPECT[key] = dict(matched=matched, reg=reg, q=qs)
    return _EXPECT[key]
