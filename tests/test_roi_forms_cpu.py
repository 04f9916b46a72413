"""What test_roi_forms_gpu.py relies on, checked without a GPU: the fp64 reference of tests.roi_forms against the oracle
the suite already trusts, the comparators against an fp32 model of the kernels and against mutants of it, the coverage
the case lists claim (read from the reference's tap lists), the exactness preconditions, the generators' termination
and discontinuity margins, and expect_roi against the constants of the roi_*.hip files.

`device_forward` / `device_backward` are a numpy float32 transcription of the kernels' arithmetic (roi_geom, sample_pos,
tri_setup, the merge of a step's 64 taps by cell with the butterfly's pairing, the list sums in list order, the division;
the atomic backward in (RoI, bin, step, cell) order; the fixed-order backward with its stable sort, its chunks of 64
records, partials and join).  It models the device; it is not a reference.  It passes every comparator on every case;
the worst ratio of its error to the bound (printed by test_model_passes_every_comparator):
  rounding class  forward fp32 0.0044, forward bf16 0.953, backward fp32 0.0114, backward bf16 0.968
  exact class     bit for bit
(the bf16 ratios are the half-ulp of the one output rounding, which the bound allows exactly once).

Mutants of the model must fail: each in every exact case that has the feature it breaks, and in at least one rounding
case of every axis row that has the feature."""
import math
import os
import re

import numpy as np
import pytest

from tests import roi_forms as Rf
from tests.roi_forms import BF16, F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# --------------------------------------------------------------------------------------------- the device model
def _geom32(roi, scale, bins, sr, mutant):
    r = Rf.f32(roi)
    s = F(scale)
    PH, PW, PZ = bins
    g = dict(b=int(r[0]), cw=r[1] * s, ch=r[2] * s, cz=r[3] * s)
    rw, rh, rz = max(r[4] * s, F(1)), max(r[5] * s, F(1)), max(r[6] * s, F(1))
    theta = F(np.float64(r[7]) * 3.14159265358979323846 / 180.0)
    g.update(bh=rh / F(PH), bw=rw / F(PW), bz=rz / F(PZ))
    g["gh"] = sr if sr > 0 else int(math.ceil(rh / F(PH)))
    g["gw"] = sr if sr > 0 else int(math.ceil(rw / F(PW)))
    g["gz"] = sr if sr > 0 else int(math.ceil(rz / F(PZ)))
    g.update(sh=F(-np.float64(rh) / 2.0), sw=F(-np.float64(rw) / 2.0), sz=F(-np.float64(rz) / 2.0))
    g["cosT"], g["sinT"] = F(math.cos(np.float64(theta))), F(math.sin(np.float64(theta)))
    if mutant == "sin":
        g["sinT"] = -g["sinT"]
    return g


def _axis32(v, n):
    v = np.where(v <= 0, F(0), v)
    lo = v.astype(np.int64)
    top = lo >= n - 1
    lo = np.where(top, n - 1, lo)
    hi = np.where(top, n - 1, lo + 1)
    v = np.where(top, lo.astype(F), v)
    l = (v - lo.astype(F)).astype(F)
    return lo, hi, (F(1) - l).astype(F), l


def positions32(g, bins):
    """sample_pos in fp32, operation by operation: y, x, z [NB, NS]"""
    NB, NS = Rf.nb_of(bins), g["gh"] * g["gw"] * g["gz"]
    ph, pw, pz = (a.astype(F)[:, None] for a in np.unravel_index(np.arange(NB), bins))
    iy, ix, iz = ((a.astype(F) + F(.5))[None, :] for a in np.unravel_index(np.arange(NS), (g["gh"], g["gw"], g["gz"])))
    yy = (g["sh"] + ph * g["bh"]) + iy * g["bh"] / F(g["gh"])
    xx = (g["sw"] + pw * g["bw"]) + ix * g["bw"] / F(g["gw"])
    zz = (g["sz"] + pz * g["bz"]) + iz * g["bz"] / F(g["gz"])
    x = (xx * g["cosT"] + yy * g["sinT"]) + g["cw"]
    y = (yy * g["cosT"] - xx * g["sinT"]) + g["ch"]
    z = zz + g["cz"] + F(0) * x
    assert x.dtype == F and y.dtype == F and z.dtype == F
    return y, x, z


def device_taps(case, n, backward, mutant=None):
    """site [NB, steps, 64] and fp32 weight [NB, steps, 64] per lane = 8 (sub-sample of the step) + corner; NS"""
    bins, crop, m = case["bins"], case["crop"], case["map"]
    PH, PW, PZ = bins
    H, W, Z = crop
    g = _geom32(case["rois"][n], case["scale"], bins, case["sr"], mutant)
    NB, NS = Rf.nb_of(bins), g["gh"] * g["gw"] * g["gz"]
    y, x, z = positions32(g, bins)
    ok = ~((y < -1.0) | (y > H) | (x < -1.0) | (x > W) | (z < -1.0))
    drop_z = backward
    if mutant == "fwd_z" and not backward:
        drop_z = True
    if mutant == "bwd_no_z" and backward:
        drop_z = False
    if drop_z:
        ok &= ~(z > Z)
    yl, yh, hy, ly = _axis32(y, H)
    xl, xh, hx, lx = _axis32(x, W)
    zl, zh, hz, lz = _axis32(z, Z)
    steps = Rf.cdiv(NS, 8)
    site = np.full((NB, steps * 8, 8), -1, np.int64)
    w = np.zeros((NB, steps * 8, 8), F)
    for q in range(8):
        zb, yb, xb = q >> 2, (q >> 1) & 1, q & 1
        ky, kx = (yh if yb else yl), (xh if xb else xl)
        if mutant == "swap_yx":
            ky, kx = (yh if xb else yl), (xh if yb else xl)
        s = m.find(g["b"], ky, kx, zh if zb else zl)
        site[:, :NS, q] = np.where(ok, s, -1)
        w[:, :NS, q] = ((ly if yb else hy) * (lx if xb else hx)) * (lz if zb else hz)
    if mutant == "drop_partial_step" and NS % 8:
        site[:, (NS // 8) * 8:, :] = -1
    w = np.where(site >= 0, w, F(0))
    return site.reshape(NB, steps, 64), w.reshape(NB, steps, 64), NS


def merged_lists(site, w):
    """per (bin, step): the cells in order of their first lane, each with the butterfly sum of its lanes' weights.
    -> cell [NB, steps, L], weight [NB, steps, L], length [NB, steps]"""
    same = site[..., :, None] == site[..., None, :]                     # [.., lane j, lane i]: i holds j's cell
    a = np.where(same, w[..., None, :], F(0)).astype(F)
    for d in (32, 16, 8, 4, 2, 1):                                      # __shfl_xor by d: lane i adds lane i ^ d
        a = (a[..., :d] + a[..., d:2 * d]).astype(F)
    wsum = a[..., 0]
    first = (site >= 0) & (np.argmax(same, -1) == np.arange(64))
    order = np.argsort(~first, axis=-1, kind="stable")
    L = max(int(first.sum(-1).max()), 1) if first.size else 1
    order = order[..., :L]
    cell = np.take_along_axis(site, order, -1)
    cw = np.take_along_axis(wsum, order, -1)
    valid = np.take_along_axis(first, order, -1)
    return np.where(valid, cell, -1), np.where(valid, cw, F(0)), first.sum(-1)


def _round_out(a, bf16):
    return Rf.bf16_round(a) if bf16 else a.astype(F)


def device_forward(case, bf16, mutant=None):
    m, bins = case["map"], case["bins"]
    K, C, NB = case["K"], case["C"], Rf.nb_of(bins)
    feats = np.vstack([Rf.f32(m.feats), np.zeros((1, C), F)])
    if mutant == "odd_c":
        feats[:, C - 2] = 0
    out = np.zeros((K, C, NB), F)
    dropped = mutant != "drop_tap"
    for n in range(K):
        site, w, NS = device_taps(case, n, False, mutant)
        cell, cw, _ = merged_lists(site, w)
        if not dropped and (cell >= 0).any():
            i = np.unravel_index(np.argmax(np.where(cell >= 0, cw, -1)), cw.shape)
            cell[i], cw[i] = -1, F(0)
            dropped = True
        acc = np.zeros((NB, C), F)
        for st in range(cell.shape[1]):
            for p in range(cell.shape[2]):
                sel = cell[:, st, p] >= 0
                if sel.any():
                    acc[sel] = acc[sel] + (cw[sel, st, p, None] * feats[cell[sel, st, p]]).astype(F)
        count = F(Rf.cdiv(NS, 8) * 8 if mutant == "count_up" else NS)
        res = (acc / count).astype(F)
        if mutant == "ragged_group":
            res[(NB // Rf.ROI_G) * Rf.ROI_G:] = 0
        out[n] = res.T
    return _round_out(out, bf16).reshape((K, C) + tuple(bins))


def device_records(case, mutant=None):
    """the records of the backward in (RoI, bin, step, cell) order: site, source (RoI, bin), merged weight, NS"""
    K, NB = case["K"], Rf.nb_of(case["bins"])
    rs, rn, rb, rw, rc = [], [], [], [], []
    for n in range(K):
        site, w, NS = device_taps(case, n, True, mutant)
        cell, cw, _ = merged_lists(site, w)
        have = cell >= 0                                                   # C order = (bin, step, position)
        b = np.broadcast_to(np.arange(NB)[:, None, None], cell.shape)
        rs.append(cell[have]); rn.append(np.full(int(have.sum()), n)); rb.append(b[have]); rw.append(cw[have])
        rc.append(np.full(int(have.sum()), Rf.cdiv(NS, 8) * 8 if mutant == "count_up" else NS))
    cat = lambda v, t: np.concatenate(v).astype(t) if v else np.zeros(0, t)
    rec = [cat(rs, np.int64), cat(rn, np.int64), cat(rb, np.int64), cat(rw, F), cat(rc, np.int64)]
    if mutant == "drop_tap" and rec[0].size:
        keep = np.ones(rec[0].size, bool)
        keep[np.argmax(rec[3])] = False
        rec = [r[keep] for r in rec]
    if mutant == "dup_record" and rec[0].size:
        i = int(np.argmax(rec[3]))
        rec = [np.insert(r, i, r[i]) for r in rec]
    return rec


def device_backward(case, bf16, det, mutant=None, base=None):
    """d_feats [n, C]: det = False the atomic form (fp32 sums; bf16: rounded in one pass), det = True the fixed-order form"""
    m, C = case["map"], case["C"]
    NB = Rf.nb_of(case["bins"])
    top = Rf.f32(case["top"]).reshape(case["K"], C, NB)
    site, rn, rb, rw, rc = device_records(case, mutant)
    d = np.zeros((m.n, C), F) if base is None else Rf.f32(base).copy()
    t = top[rn, :, rb] if site.size else np.zeros((0, C), F)             # [records, C]
    if not det:
        val = ((t * rw[:, None]).astype(F) / rc.astype(F)[:, None]).astype(F)
        np.add.at(d, site, val)
        return _round_out(d, bf16)
    wq = (rw / rc.astype(F)).astype(F)
    order = np.argsort(site, kind="stable")
    skey = site[order]
    beg, end = np.searchsorted(skey, np.arange(m.n), "left"), np.searchsorted(skey, np.arange(m.n), "right")
    prod = (wq[order][:, None] * t[order]).astype(F)

    def run(a, b):
        acc = np.zeros(C, F)
        for i in range(a, b):
            acc = (acc + prod[i]).astype(F)
        return acc
    for row in np.nonzero(end > beg)[0]:
        a, b = int(beg[row]), int(end[row])
        c0, c1 = a // Rf.DET_CHUNK, (b - 1) // Rf.DET_CHUNK
        if c0 == c1:
            acc = run(a, b)
        else:
            acc = np.zeros(C, F)
            last = c1 - 1 if mutant == "drop_chunk_tail" else c1
            for k in range(c0, last + 1):
                acc = (acc + run(max(a, k * Rf.DET_CHUNK), min(b, (k + 1) * Rf.DET_CHUNK))).astype(F)
        d[row] = Rf.bf16_round(acc) if bf16 else (d[row] + acc).astype(F)
    return d


# ------------------------------------------------------------------------------------------ what has which feature
def _has_feature(mutant, case, R, backward, det):
    K, C, NB = case["K"], case["C"], Rf.nb_of(case["bins"])
    taps = R.btaps if backward else R.taps
    if K == 0 or taps.shape[0] == 0:
        return False
    if mutant in ("drop_partial_step", "count_up"):
        return bool((R.ns % 8 != 0).any())
    if mutant == "ragged_group":
        return NB % Rf.ROI_G != 0 and bool((R.out.reshape(K, C, NB)[:, :, (NB // Rf.ROI_G) * Rf.ROI_G:] != 0).any())
    if mutant == "odd_c":
        return C % 2 == 1 and C >= 3
    if mutant == "sin":
        return not case["exact"]
    if mutant in ("fwd_z", "bwd_no_z"):
        return R.taps.shape[0] != R.btaps.shape[0]
    if mutant == "drop_chunk_tail":
        _, beg, end = Rf.record_lists(R.btaps, case["map"].n)
        return bool(((end > beg) & (beg // Rf.DET_CHUNK != (end - 1) // Rf.DET_CHUNK)).any())
    return True


FWD_MUTANTS = ("drop_tap", "drop_partial_step", "count_up", "ragged_group", "odd_c", "swap_yx", "sin", "fwd_z")
BWD_MUTANTS = ("drop_tap", "drop_partial_step", "count_up", "swap_yx", "sin", "bwd_no_z", "dup_record")
DET_MUTANTS = BWD_MUTANTS + ("drop_chunk_tail",)

FWD_GROUPS = ("fwd_channels", "bins", "subsamples", "lookup_far", "edges", "levels", "dense")
BWD_GROUPS = ("bwd_channels", "bins", "bwd_only_bins", "subsamples", "edges", "cvt_tails", "dense")
DET_GROUPS = ("det_channels", "bins", "bwd_only_bins", "subsamples", "edges", "det_lists")


def _cases(groups, det=False):
    for gname in groups:
        for sp in Rf.GROUPS[gname]:
            if det and sp["sr"] <= 0:
                continue
            for exact in Rf.kinds(sp):
                for typ in (F32, BF16):
                    if sp["scene"] == "dense" and typ == BF16:
                        continue
                    yield gname, sp, exact, typ


_ref = Rf.cached_case


def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------------- tests
def test_model_passes_every_comparator():
    Rf.MARGINS.clear()
    for gname, sp, exact, typ in _cases(FWD_GROUPS):
        case, R = _ref(sp, exact, typ)
        Rf.check_forward(f"{gname} {sp['name']}", device_forward(case, typ == BF16), R, exact, typ == BF16)
    for gname, sp, exact, typ in _cases(BWD_GROUPS):
        case, R = _ref(sp, exact, typ)
        Rf.check_backward(f"{gname} {sp['name']}", device_backward(case, typ == BF16, False), R, exact, typ == BF16)
    for gname, sp, exact, typ in _cases(DET_GROUPS, det=True):
        case, R = _ref(sp, exact, typ)
        got = device_backward(case, typ == BF16, True)
        Rf.check_backward(f"{gname} {sp['name']} fixed order", got, R, exact, typ == BF16)
        if exact:
            assert Rf.same_bits(got, device_backward(case, typ == BF16, False))
    print("\nROI_MODEL_MARGINS", {k: round(v, 4) for k, v in sorted(Rf.MARGINS.items())})
    assert all(0 <= v <= 1 for v in Rf.MARGINS.values())


def _mutants(groups, mutants, run, backward, det):
    had = {}
    for gname, sp, exact, typ in _cases(groups, det=det):
        case, R = _ref(sp, exact, typ)
        for mu in mutants:
            if not _has_feature(mu, case, R, backward, det):
                continue
            failed = _fails(lambda: run(case, R, typ == BF16, mu, exact))
            if exact:
                assert failed, f"{mu} survives the exact case {gname} / {sp['name']} (storage type {typ})"
            k = (gname, mu, exact, typ)
            had[k] = had.get(k, False) or failed
    alive = [k for k, v in had.items() if not v]
    assert not alive, f"mutants that survive a whole axis row: {alive}"
    assert {k[1] for k in had} == set(mutants)


def test_forward_mutants_fail():
    _mutants(FWD_GROUPS, FWD_MUTANTS,
             lambda c, R, bf, mu, ex: Rf.check_forward(mu, device_forward(c, bf, mu), R, ex, bf), False, False)


def test_backward_mutants_fail():
    _mutants(BWD_GROUPS, BWD_MUTANTS,
             lambda c, R, bf, mu, ex: Rf.check_backward(mu, device_backward(c, bf, False, mu), R, ex, bf), True, False)


def test_fixed_order_mutants_fail():
    _mutants(DET_GROUPS, DET_MUTANTS,
             lambda c, R, bf, mu, ex: Rf.check_backward(mu, device_backward(c, bf, True, mu), R, ex, bf), True, True)


def test_reference_agrees_with_the_oracle():
    """the fp32 oracle the suite already trusts: inside the rounding bound on the rounding cases, the same bits on the
    exact ones (forward and backward, on the map made dense over its crop)"""
    import oracle
    Rf.MARGINS.clear()
    for gname in ("fwd_channels", "bwd_channels", "bins", "bwd_only_bins", "subsamples", "edges", "levels", "dense"):
        for sp in Rf.GROUPS[gname]:
            if sp["C"] > 130:
                continue
            for exact in Rf.kinds(sp):
                case, R = _ref(sp, exact, F32)
                m, (H, W, Z), C, K = case["map"], case["crop"], case["C"], case["K"]
                dense = np.zeros((case["examples"], C, H, W, Z), np.float32)
                s = m.sites
                dense[s[:, 3], :, s[:, 0], s[:, 1], s[:, 2]] = m.feats
                args = (case["scale"],) + case["bins"] + (case["sr"],)
                tag = f"oracle {gname} {sp['name']}"
                Rf.check_forward(tag, oracle.roi_align_rotated_3d(dense, case["rois"], *args), R, exact, False)
                if Rf.bwd_bins_ok(case["bins"]) and K:
                    g = oracle.roi_align_rotated_3d_backward(case["top"], case["rois"], *args, dense.shape)
                    Rf.check_backward(tag, g[s[:, 3], :, s[:, 0], s[:, 1], s[:, 2]], R, exact, False)


def _all_lengths(groups, backward=False):
    out = []
    for gname in groups:
        for sp in Rf.GROUPS[gname]:
            for exact in Rf.kinds(sp):
                case, R = _ref(sp, exact, F32)
                out.append(Rf.list_lengths(R.btaps if backward else R.taps, case["K"], Rf.nb_of(case["bins"]), R.steps))
    return np.concatenate(out)


def test_merged_list_lengths_reach_the_whole_ladder():
    """the 8 / 4 / 2 / 1 remainder ladder of k_roi_sparse runs over lists of these lengths"""
    L = _all_lengths(("fwd_channels", "bins", "subsamples", "lookup_far", "edges", "levels"))
    for lo, hi in ((0, 0), (1, 1), (2, 2), (3, 3), (4, 7), (8, 8), (9, 15), (16, 64)):
        assert ((L >= lo) & (L <= hi)).sum() >= 3, (lo, hi)
    assert {int(v) % 8 for v in L} == set(range(8))
    assert L.max() <= 64


def test_fixed_order_lists_reach_their_forms():
    """Chunk positions are counted here in the reference's site numbering; the device sorts by the grid's row numbers,
    so test_roi_forms_gpu.py repeats the chunk counts with the rows the grid gave (test_fixed_order[det_lists])."""
    case, R = _ref(Rf.SUBSAMPLES[2], False, F32)                      # sampling_ratio 3: NS = 27, three steps and one of 3
    assert case["sr"] == 3 and R.steps.max() == 4
    t = R.btaps
    per_bin = np.unique(t[:, :3], axis=0, return_counts=True)[1]     # steps of one bin that reach one row
    assert per_bin.max() >= 2 and set(np.unique(t[:, 3])) == {0, 1, 2, 3}
    spans, ends_on, starts_on, empty = 0, 0, 0, 0
    for sp in Rf.DET_LISTS:
        for exact in Rf.kinds(sp):
            case, R = _ref(sp, exact, F32)
            _, beg, end = Rf.record_lists(R.btaps, case["map"].n)
            have = end > beg
            nch = np.where(have, (end - 1) // Rf.DET_CHUNK - beg // Rf.DET_CHUNK + 1, 0)
            spans = max(spans, int(nch.max()))
            ends_on += int((have & (end % Rf.DET_CHUNK == 0)).sum())
            starts_on += int((have & (beg % Rf.DET_CHUNK == 0) & (beg > 0)).sum())
            empty += int((~have).sum())
            assert R.btaps.shape[0] <= Rf.expect_roi(Rf.DET, F32, case["K"], case["C"], case["bins"], case["sr"],
                                                     n_rows=case["map"].n)["n_max"]
    assert spans >= 3 and ends_on >= 1 and starts_on >= 1 and empty >= 1, (spans, ends_on, starts_on, empty)


def test_geometry_edges_are_what_their_names_say():
    by = {sp["name"]: sp for sp in Rf.EDGES}
    for exact in (True, False):
        case, R = _ref(by["wholly outside"], exact, F32)
        assert R.taps.shape[0] == 0 and not R.out.any() and not R.grad.any()
        case, R = _ref(by["no site inside the box"], exact, F32)
        assert R.taps.shape[0] == 0 and not R.out.any() and case["map"].n > 100
        case, R = _ref(by["z above the map"], exact, F32)
        assert R.btaps.shape[0] < R.taps.shape[0]                   # the forward clamps, the backward drops
    case, R = _ref(by["below one pixel"], False, F32)
    assert all((Rf.geometry(r, case["scale"], case["bins"], case["sr"])["raw"] < 1).all() for r in case["rois"])
    planes = {"cut by y = -1": (0, -1.0, -1), "cut by y = H": (0, Rf.SMALL[0], 1), "cut by x = -1": (1, -1.0, -1),
              "cut by x = W": (1, Rf.SMALL[1], 1), "cut by z = -1": (2, -1.0, -1)}
    for name, (ax, plane, side) in planes.items():
        for exact in (True, False):
            case, _ = _ref(by[name], exact, F32)
            cut = 0
            for r in case["rois"]:
                p = Rf.sample_positions(Rf.geometry(r, case["scale"], case["bins"], case["sr"]), case["bins"])[ax]
                cut += int(((p - plane) * side > 0).any() and ((p - plane) * side < 0).any())
            assert cut >= 1, (name, exact)
    case, _ = _ref(by["centre in the -1 .. 0 band"], False, F32)
    assert all((-1 <= c <= 0) for r in case["rois"] for c in Rf.geometry(r, case["scale"], case["bins"], 2)["c"])
    assert _ref(by["K = 0"], True, F32)[1].out.shape[0] == 0 and _ref(by["K = 1"], True, F32)[1].out.shape[0] == 1


def test_generators_terminate_with_full_lists_and_margins():
    n = 0
    for gname, specs in Rf.GROUPS.items():
        for sp in specs:
            for exact in Rf.kinds(sp):
                for typ in (F32, BF16):
                    case, R = _ref(sp, exact, typ)
                    n += 1
                    assert case["rois"].shape == (sp["K"], 8) and R.out.shape == (sp["K"], sp["C"]) + sp["bins"]
                    assert case["rois"].shape[0] == 0 or (0 <= case["rois"][:, 0].min()
                                                          and case["rois"][:, 0].max() < case["examples"])
                    assert case["map"].extent() == tuple(case["crop"])
                    if exact:
                        Rf.assert_exact_case(case["rois"], case["scale"], case["map"], case["crop"], case["bins"],
                                             case["sr"], top=case["top"])
                    else:
                        for r in case["rois"]:
                            assert Rf.discontinuity_margin(r, case["scale"], case["bins"], case["sr"], case["crop"]) >= Rf.MARGIN
                            assert -180.0 < r[7] <= 180.0
                        if typ == BF16:
                            assert Rf.same_bits(Rf.bf16_round(case["map"].feats), case["map"].feats)
                            assert Rf.same_bits(Rf.bf16_round(case["top"]), case["top"])
    assert n > 300
    far = _ref(Rf.LOOKUP_FAR[0], True, F32)[0]
    assert not Rf.dense_index_taken(far["map"].extent() + (1,)) and Rf.dense_index_taken(Rf.SMALL + (2,))
    assert {_ref(sp, True, F32)[0]["map"].n * sp["C"] % 4 for sp in Rf.CVT_TAILS} == {0, 1, 2, 3}
    for l in range(4):
        case = _ref(Rf.LEVEL_SPECS[l], True, F32)[0]
        assert case["crop"] == Rf.level_crop(Rf.SMALL, l) and case["map"].n > 8


def test_exact_precondition_refuses_what_is_not_exact():
    case = dict(_ref(Rf.BINS[2], True, F32)[0])
    rois = case["rois"].copy()
    rois[0, 7] = 30.0
    with pytest.raises(AssertionError):
        Rf.assert_exact_case(rois, case["scale"], case["map"], case["crop"], case["bins"], case["sr"])
    rois = case["rois"].copy()
    rois[0, 1] += 0.3
    with pytest.raises(AssertionError):
        Rf.assert_exact_case(rois, case["scale"], case["map"], case["crop"], case["bins"], case["sr"])
    with pytest.raises(AssertionError):
        Rf.assert_exact_case(case["rois"], case["scale"], case["map"], case["crop"], case["bins"], 3)


def test_position_bound_covers_the_model():
    """the derived 11 u M against the model's fp32 positions: the model measures 0.58 u M (ROI_POS_RATIO 0.0523 of the
    bound), M = scaled sizes + |scaled centres| of the RoI as in tests/roi_forms.py"""
    worst = 0.0
    for sp in Rf.SUBSAMPLES + Rf.LOOKUP_FAR + Rf.LEVEL_SPECS:
        case, R = _ref(sp, False, F32)
        for n in range(case["K"]):
            g = _geom32(case["rois"][n], case["scale"], case["bins"], case["sr"], None)
            geo = Rf.geometry(case["rois"][n], case["scale"], case["bins"], case["sr"])
            assert (g["gh"], g["gw"], g["gz"]) == tuple(int(v) for v in geo["g"])
            y64, x64, z64 = Rf.sample_positions(geo, case["bins"])
            got = positions32(g, case["bins"])
            err = max(np.abs(a.astype(np.float64) - b).max() for a, b in zip(got, (y64, x64, z64)))
            worst = max(worst, err / geo["pos"])
    assert 0 < worst < 1, worst
    print("\nROI_POS_RATIO", round(worst, 4))


def test_expect_roi_restates_the_constants():
    csrc = os.path.join(ROOT, "detection_3d_amd", "csrc")
    text = "".join(open(os.path.join(csrc, f)).read()
                   for f in ("roi_geometry.inc", "roi_forward.hip", "roi_backward.hip", "roi_backward_det.hip"))
    grid = open(os.path.join(csrc, "grid_views.hip")).read()

    def const(name, src=text):
        found = re.findall(r"constexpr \w+ " + name + r" = (\d+)", src)
        assert len(found) == 1, (name, found)                          # one definition across the files
        return int(found[0])
    assert (const("kRoiG"), const("kRoiCch"), const("kRoiWaves"), const("kRoiBwdCch"), const("kRoiDetChunk"),
            const("kRoiDetCpl"), const("kRoiMaxLevels")) == (Rf.ROI_G, Rf.ROI_CCH, Rf.ROI_WAVES, Rf.ROI_BWD_CCH,
                                                             Rf.DET_CHUNK, Rf.DET_CPL, Rf.MAX_LEVELS)
    assert re.search(r"kDenseMaxCells = 8L << 20", grid) and Rf.DENSE_MAX_CELLS == 8 << 20
    assert const("kRoiFormFields") == len(Rf.ROI_FIELDS)
    assert Rf.bwd_bins_ok((5, 3, 17)) and not Rf.bwd_bins_ok(Rf.REFUSED_BINS) and Rf.nb_of(Rf.REFUSED_BINS) == 256
    z = dict.fromkeys(Rf.ROI_FIELDS, 0)
    assert Rf.expect_roi(Rf.SPARSE, F32, 0, 8, (1, 1, 1)) == z and Rf.expect_roi(Rf.DET, F32, 3, 8, (1, 1, 1), 2) == z
    f = Rf.expect_roi(Rf.SPARSE, BF16, 7, 130, (6, 8, 4), 2, Rf.INDEX, Rf.DEVICE, 1)
    assert (f["grid_x"], f["grid_y"], f["grid_z"], f["block"], f["type"]) == (7, 2, 1, 256, BF16)
    f = Rf.expect_roi(Rf.DET, F32, 4, 257, (2, 2, 1), 2, n_rows=3870)
    assert (f["n_max"], f["n_chunks"], f["bits"], f["grid_x"]) == (4 * 4 * 8 * 8, 16, 12, 4)
    assert Rf.expect_roi(Rf.DET, F32, 4, 1, (1, 1, 1), 1, n_rows=1)["bits"] == 1
    f = Rf.expect_roi(Rf.SPARSE_BWD, BF16, 0, 1, (2, 2, 1), 2, n_rows=203)
    assert (f["cvt_wgs"], f["grid_x"], f["family"]) == (1, 0, Rf.SPARSE_BWD)
    assert Rf.expect_roi(Rf.DENSE, F32, 3, 5, (3, 2, 5))["grid_x"] == Rf.cdiv(3 * 5 * 30, 256)
    # channel counts against the chunk sizes they are there for
    assert [Rf.cdiv(s["C"], Rf.ROI_CCH) for s in Rf.FWD_CHANNELS] == [1, 1, 1, 1, 2, 2, 2]
    assert [Rf.cdiv(s["C"], Rf.ROI_BWD_CCH) for s in Rf.BWD_CHANNELS] == [1, 1, 1, 2, 3]
    assert [Rf.cdiv(s["C"], 64 * Rf.DET_CPL) for s in Rf.DET_CHANNELS] == [1, 1, 1, 2, 2]
    groups = [Rf.cdiv(Rf.nb_of(s["bins"]), Rf.ROI_G) for s in Rf.BINS]
    assert groups == [1, 1, 1, 2, 4, 5, 8, 48] and [Rf.nb_of(s["bins"]) % Rf.ROI_G for s in Rf.BINS] == [1, 3, 0, 1, 0, 1, 2, 0]
