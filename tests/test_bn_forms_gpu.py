"""Every BatchNorm launch form on the MI355X against fp64 results: the statistics (from a tensor and from a
convolution's column sums), the affine + activation pass, the backward pass, for fp32 and bf16 rows, and k_add.

Every case calls through the SCN wrappers, reads d3d_bn_last_form and asserts it equals tests.bn_forms.expect_bn (the
dispatch arithmetic of bn.hip / bn_backward.hip restated from the constants, itself checked in test_bn_forms_cpu.py), and
then compares what the kernels wrote with the fp64 reference of tests.bn_forms:

* exact cases -- rows of non-zero integers in +-{1..4}, saved mean a small integer, invstd and gamma powers of two
  times small integers, beta an integer, leak 0 or 0.25: column sums are exact in any order, so mean, d_bias and
  d_weight must match to the bit, variance / running statistics have 1 fp32 ulp, invstd 4, the apply pass is exact to
  the bit (bf16: its one rounding), dx has its rounding bound.  A lost or doubled row, or a lost slice, changes every
  column.
* rounding cases -- normal data with per-column mean / std of 0, 1 and 64, leak 0.333: per element and per column
  bounds from the arithmetic (mean 1 ulp; variance 2^-23 + (rows + 4) 2^-52 kappa; invstd 4 ulp; apply
  gamma_3 (|x w| + |mean w| + |beta|); backward sums 2 u of their magnitudes plus the final rounding; dx
  gamma_6 (|d'| + |gm| + |x - mean| |k|) |invstd w| plus gm's 1 u and k's 3 u, plus what gm and k inherit from the
  sums' own 2 u; bf16 one more rounding of the output).
  The last term is needed: against a reference with fp64 sums, "k good to 3 u" does not hold where dp cancels (its
  terms' magnitudes add up to rows, dp itself is of the order sqrt(rows)).  Without it the fp32 kernels, which are
  right, missed the dx bound in 7 of the 14 fp32 cases of test_backward on the MI355X, at worst by 3.4 x (C = 128:
  2.396e-08 against 6.962e-09; C = 768: 3.056e-09 against 1.028e-09; C = 4096: 4.143e-08 against 2.059e-08); with it
  the largest error is 0.57 of the bound, and a row lost from the sums still fails it (test_bn_forms_cpu.py).

form                                                        tests
==========================================================  ===========================================================
k_bn_stats<float>, butterfly (C 4 .. 128, LPR 1 .. 32)      test_statistics_from_a_tensor[4 .. 128]
k_bn_stats<float>, LDS row lanes (C 256 .. 4096, RL 16..1)  test_statistics_from_a_tensor[256 .. 4096]
k_bn_stats<bf16>, both layouts, modes 1 and 2               the same cases (st_type 2)
modes 0 / 1 / 2                                             batch_stats / BatchNormalization_updateOutput(train) /
                                                            batch_mean_invstd in every one of those cases
1 slice; 2 .. 16 slices in one group; 17 (group of 1);      the row counts of bn_forms.stats_row_counts: 1, 2, 3, RL-1,
128 slices with a short last slice; empty trailing slices   RL, RL+1, 4 RL (+1), 6 RL, 7 RL, T, T+1, 16 T, 16 T+1,
(C 4096, 1100 rows); 4-pass loop against 1, 2, 3 passes     127 T+1, 1100 -- all of them at C 4096, 1024, 128 and 32
rows = 1                                                    test_statistics_from_a_tensor (every class but C = 4)
tickets left zero, group counts in turn on one scratch      test_tickets_are_left_zero
k_bn_stats<double>: V 8 .. 1024 in one pass (SL 128 .. 1),  test_statistics_from_partials[4, 12, 128, 512]
2, 3 and 8 passes of 1024 values                            test_statistics_from_partials[1024, 1536, 4096]
partial rows 1, 8 SL, 8 SL+1, 16 * 8 SL+1, the 64-slice cap the same cases; both outputs (invstd, unbiased variance)
planes the finish does not serve (768, 516, 1280)           test_partials_refuse_what_the_finish_cannot_walk
k_bn_apply_rows<float / bf16>: RPI 256 .. 1, one workgroup, test_apply[4 .. 1024]; C 1024 at 2048, 2049, 6144, 6145,
the 2048-workgroup cap, the 4-rows-in-flight loop + tail    8193; C 256 and C 64 with 3 * 2048 RPI + RPI + 1 rows
k_bn_apply float4 path (C 2048, 4096)                       test_apply[2048, 4096]
k_bn_apply scalar path (C 1, 6, 9; rows C % 4 = 0 .. 3)     test_apply[1, 6, 9], through bn_apply and through
                                                            BatchNormalization_updateOutput in eval mode
weight / bias present and absent, leak 0 and 0.25 (0.333)   bn_forms.VARIANTS, cycled over the cases of test_apply
NaN, +-inf, -0 inputs                                       test_apply_non_finite
rows = 0: no launch                                         test_no_rows_no_launch
k_bn_bwd_partial4<float / bf16>, slices 1, 2, 7, 8, 9, 128  test_backward[4 .. 4096]
k_bn_bwd_partial (scalar): planes 1, 2; planes 768 (a loop  test_backward[1, 2, 768]; rows 1, 63, 64, 65, 8191, 8192
over channels); bf16 C = 4 on an 8-byte aligned view        test_backward_unaligned_rows
k_bn_bwd_finish: C < 32, C % 32 != 0, 1 .. 128 slices       the same cases
k_bn_bwd_apply_rows (two-row loop from 2049 rows at C 1024) test_backward[1024]: 2048, 2049, 4097
k_bn_bwd_apply4 (C 2048, 4096); k_bn_bwd_apply (scalar)     test_backward[2048, 4096]; the scalar cases above
weight absent, d_weight / d_bias NULL                       bn_forms.VARIANTS, cycled over the cases of test_backward
y = 0, y = -0, y = +-2^-100: the slope follows the sign     the exact cases of test_backward (hand-made y)
the module: saved statistics and the OUTPUT reach backward  test_module_train_path
k_add: n 1 .. 1027, 3072 .. 3075                            test_add

Not reached, and why:
* mode 0 on bf16 rows: d3d_bn_batch_stats takes fp32 rows only; the bf16 instantiation is launched in modes 1 and 2.
* the general apply kernels on bf16 rows: they do not exist -- d3d_bn_apply_dt refuses such planes (asserted), and
  with it d3d_bn_forward_dt: bf16 rows of 2048 and 4096 channels have their statistics in mode 2 only.
* slice caps other than the default of run_stats_partials: D3D_BN_SLICES is read once per process; the tests refuse to
  run with it set.
* row counts whose element index passes 2^31: the largest case here has 8.4 M values; the kernels index with size_t.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import bn_forms as B
from tests.bn_forms import BF16, EPS, F32

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_slices():
    assert "D3D_BN_SLICES" not in os.environ, \
        "D3D_BN_SLICES is set: expect_bn restates the default slice cap of run_stats_partials; unset it for these tests"


def _scn():
    from detection_3d_amd.sparseconvnet import SCN
    return SCN


def bn_last_form():
    from detection_3d_amd._lib import lib
    buf = (ctypes.c_int * len(B.BN_FIELDS))()
    n = lib().d3d_bn_last_form(buf, len(B.BN_FIELDS))
    assert n == len(B.BN_FIELDS)
    return dict(zip(B.BN_FIELDS, list(buf)))


def assert_form(tag, want):
    got = bn_last_form()
    assert got == want, f"{tag}: the launch form differs: " + ", ".join(
        f"{k} = {got[k]} (expected {want[k]})" for k in B.BN_FIELDS if got[k] != want[k])


def to_dev(a, dev, typ=F32):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    return t.bfloat16() if typ == BF16 else t        # the values are bf16 numbers already: no rounding here


def to_np(t):
    return t.detach().float().cpu().numpy()


def _rows_of(rng, rows, planes, exact_data, typ):
    return B.int_rows(rng, rows, planes) if exact_data else B.normal_rows(rng, rows, planes, typ == BF16)


# ------------------------------------------------------------------------------------- statistics from a tensor
def _run_statistics(dev, planes, rows, typ, exact_data):
    SCN = _scn()
    rng = np.random.RandomState(B.seed_of(planes, rows, typ, exact_data, 11))
    x = _rows_of(rng, rows, planes, exact_data, typ)
    if exact_data:
        B.assert_exact_rows(x)
        ref = B.stats_ref_exact(*B.col_sums(x), rows)
    else:
        ref = B.stats_ref(x)
    xt = to_dev(x, dev, typ)
    tag = f"C={planes} rows={rows} {'bf16' if typ == BF16 else 'fp32'}"
    bn_last_form()
    if typ == F32:
        mean, var = SCN.batch_stats(xt)
        assert_form(tag + " mode 0", B.expect_bn(rows, planes, typ, stats=("tensor", 0)))
        B.check_stats(tag + " mode 0", ref, 0, EPS, to_np(mean), to_np(var), exact_data)
    mean, invstd = SCN.batch_mean_invstd(xt, EPS)
    assert_form(tag + " mode 2", B.expect_bn(rows, planes, typ, stats=("tensor", 2)))
    B.check_stats(tag + " mode 2", ref, 2, EPS, to_np(mean), to_np(invstd), exact_data)
    if typ == BF16 and not B.apply_rows_kernel(planes):
        return          # d3d_bn_forward_dt has no apply kernel for such rows and refuses them: modes 0 / 2 only
    # mode 1 with the apply pass behind it; running statistics start away from 0 and 1
    if exact_data:
        rm, rv, mom = B.exact_running(rng, planes)
        _, _, gam, beta = B.exact_params(rng, planes)
        leak = 0.25
    else:
        rm, rv, mom = B.f32(rng.uniform(0.5, 1.5, planes)), B.f32(rng.uniform(0.5, 2.0, planes)), 0.9
        gam, beta, leak = B.f32(rng.uniform(0.5, 1.5, planes)), B.f32(rng.uniform(-0.5, 0.5, planes)), 0.333
    out = xt.new_empty(0)
    sm, si = torch.empty(planes, device=dev), torch.empty(planes, device=dev)
    rmt, rvt = to_dev(rm, dev), to_dev(rv, dev)
    SCN.BatchNormalization_updateOutput(xt, out, sm, si, rmt, rvt, to_dev(gam, dev), to_dev(beta, dev), EPS, mom, True, leak)
    assert_form(tag + " mode 1", B.expect_bn(rows, planes, typ, stats=("tensor", 1), apply=True))
    B.check_stats(tag + " mode 1", ref, 1, EPS, to_np(sm), to_np(si), exact_data, running=(rm, rv, mom, to_np(rmt), to_np(rvt)))
    # the output against fp64 of the fp32 statistics the apply pass was given
    B.check_apply(tag + " train", to_np(out), x, to_np(sm), to_np(si), gam, beta, leak, False, typ == BF16)
    if rows == 1:       # pinned as the code defines it today
        assert B.same_bits(to_np(sm), x[0]) and B.same_bits(to_np(mean), x[0])
        assert np.isnan(to_np(invstd)).all() and np.isnan(to_np(rvt)).all()
        B.within("stats invstd, one row", to_np(si), np.full(planes, float(np.float32(EPS)) ** -0.5), 4 * B.ulp32(100.0))
        if typ == F32:
            assert np.isnan(to_np(var)).all()


@pytest.mark.parametrize("planes", B.STATS_PLANES)
def test_statistics_from_a_tensor(dev, planes):
    for _, rows in B.stats_cases(planes):
        for typ in (F32, BF16):
            for exact_data in (True, False):
                _run_statistics(dev, planes, rows, typ, exact_data)


def test_row_counts_reach_what_they_are_there_for():
    for planes in B.FULL_CLASSES:
        forms = [B.expect_stats(r, planes, F32, 0) for _, r in B.stats_cases(planes)]
        shapes = {(f["st_slices"], f["st_groups"], f["st_last_group"]) for f in forms}
        assert {(1, 1, 1), (2, 1, 2), (16, 1, 16), (17, 2, 1), (128, 8, 16)} <= shapes
        rl = forms[0]["st_row_lanes"]
        one_slice = [r for _, r in B.stats_cases(planes) if r <= 8 * rl]
        assert {B.cdiv(r, rl) % 4 for r in one_slice if r >= 4 * rl} >= {0, 1, 2, 3}     # passes left after the 4-pass loop
    assert 0 in B.slice_rows(1100, B.expect_stats(1100, 4096, F32, 0)["st_slices"])


def test_tickets_are_left_zero(dev):
    """calls with 2, 1 and 8 first-level groups in turn on the one scratch: right each time, tickets zero after"""
    SCN = _scn()
    planes = 1024
    for rows in (513, 32, 4065, 33, 513):
        _run_statistics(dev, planes, rows, F32, True)
    scratch = SCN._bn_scratch(dev, 1)
    torch.cuda.synchronize()
    assert int(scratch[:B.TICKET_BYTES].to(torch.int64).abs().sum().item()) == 0


# -------------------------------------------------------------------------------------- statistics from partials
@pytest.mark.parametrize("planes", B.PARTIALS_PLANES)
def test_statistics_from_partials(dev, planes):
    SCN = _scn()
    for pr in B.partials_row_counts(planes):
        rng = np.random.RandomState(B.seed_of(planes, pr, 12))
        p, rows = B.make_partials(rng, pr, planes)
        tot = p.sum(0)
        ref = B.stats_ref_exact(tot[:planes], tot[planes:], rows)
        pt = torch.from_numpy(p).to(dev)
        assert pt.dtype == torch.float64 and rows != pr
        tag = f"partials C={planes} rows={pr}"
        bn_last_form()
        for want_invstd in (True, False):
            mode = 2 if want_invstd else 0
            mean, other = SCN.stats_from_partials(pt, pr, rows, EPS, want_invstd=want_invstd)
            assert_form(tag, B.expect_bn(rows, planes, F32, stats=("partials", mode, pr)))
            B.check_stats(tag, ref, mode, EPS, to_np(mean), to_np(other), True)
    scratch = SCN._bn_scratch(dev, 1)
    assert int(scratch[:B.TICKET_BYTES].to(torch.int64).abs().sum().item()) == 0


def test_partials_refuse_what_the_finish_cannot_walk(dev):
    """2 planes above 1024 and no multiple of it: the passes of 1024 threads would run past the vectors"""
    from detection_3d_amd._lib import D3DError
    SCN = _scn()
    for planes in B.PARTIALS_REFUSED:
        pt = torch.zeros((4, 2 * planes), dtype=torch.float64, device=dev)
        bn_last_form()
        with pytest.raises(D3DError, match="partials"):
            SCN.stats_from_partials(pt, 4, 13, EPS)
        assert bn_last_form() == dict.fromkeys(B.BN_FIELDS, 0)


# ---------------------------------------------------------------------------------------------------------- apply
APPLY_PLANES = sorted({c[0] for c in B.apply_cases()})


def _kinds(rows, planes):
    """exact data, then rounding data; shapes above 2^21 values make the exact check alone (the references are numpy
    passes over the tensor, and the form is pinned either way)"""
    return (True,) if rows * planes > 1 << 21 else (True, False)


@pytest.mark.parametrize("typ", [F32, BF16])
@pytest.mark.parametrize("planes", APPLY_PLANES)
def test_apply(dev, planes, typ):
    SCN = _scn()
    mine = [(i, rows) for i, (c, rows, t) in enumerate(B.apply_cases()) if c == planes and t == typ]
    if not mine:
        assert typ == BF16 and not B.apply_rows_kernel(planes)      # refused: test_bf16_rows_have_no_general_apply_kernel
        return
    for i, rows in mine:
        for j, exact_data in enumerate(_kinds(rows, planes)):
            variant = B.VARIANTS[(i + 3 * j) % len(B.VARIANTS)]
            x, mean, invstd, w, b, leak = B.make_apply_case(planes, rows, typ, variant, exact_data)
            if exact_data:
                B.assert_exact_apply(x, mean, invstd, w, b, leak)
            tag = f"apply C={planes} rows={rows} {'bf16' if typ == BF16 else 'fp32'} {variant}"
            xt = to_dev(x, dev, typ)
            bn_last_form()
            out = SCN.bn_apply(xt, to_dev(mean, dev), to_dev(invstd, dev), to_dev(w, dev), to_dev(b, dev), leak)
            assert_form(tag, B.expect_bn(rows, planes, typ, apply=True))
            assert out.dtype == xt.dtype
            B.check_apply(tag, to_np(out), x, mean, invstd, w, b, leak, exact_data, typ == BF16)
            if typ == F32 and not B.apply_rows_kernel(planes):
                # the same kernel through d3d_bn_forward_dt in eval mode: running statistics, invstd = powf(var + eps, -1/2)
                var = (invstd.astype(np.float64) ** -2).astype(np.float32)
                sm, si = torch.empty(planes, device=dev), torch.empty(planes, device=dev)
                out2 = xt.new_empty(0)
                SCN.BatchNormalization_updateOutput(xt, out2, sm, si, to_dev(mean, dev), to_dev(var, dev), to_dev(w, dev),
                                                    to_dev(b, dev), 0.0, 0.9, False, leak)
                assert_form(tag + " eval", B.expect_bn(rows, planes, typ, stats="running", apply=True))
                assert B.same_bits(to_np(sm), mean)
                want_si = B.invstd_of(var, 0.0)
                B.within("eval invstd", to_np(si), want_si, 4 * B.ulp32(want_si))
                same = B.same_bits(to_np(si), invstd)
                B.check_apply(tag + " eval", to_np(out2), x, mean, to_np(si), w, b, leak, exact_data and same, False)


def test_apply_forms_reached():
    forms = [B.expect_apply(r, c, t) for c, r, t in B.apply_cases()]
    assert {(f["ap_kernel"], f["ap_type"]) for f in forms} == {(B.ROWS, F32), (B.ROWS, BF16), (B.VEC4, F32), (B.SCALAR, F32)}
    for typ in (F32, BF16):
        multi = {c for (c, r, t), f in zip(B.apply_cases(), forms) if f["ap_multi"] and t == typ}
        assert multi == {64, 256, 1024}
    capped = [(r, f["ap_multi"]) for (c, r, t), f in zip(B.apply_cases(), forms) if c == 1024 and t == F32 and f["ap_wgs"] == 2048]
    assert capped == [(2048, 0), (2049, 0), (6144, 0), (6145, 1), (8193, 1)]


@pytest.mark.parametrize("planes,typ", [(64, F32), (64, BF16), (1024, BF16), (2048, F32), (9, F32)])
@pytest.mark.parametrize("leak", [0.0, 0.25])
def test_apply_non_finite(dev, planes, typ, leak):
    """leak 0: max(t, 0) sends NaN to 0; leak > 0: NaN stays NaN; -0 and the infinities follow the fp64 expression; every
    other element is untouched by its neighbours' values"""
    SCN = _scn()
    rows = 37
    rng = np.random.RandomState(B.seed_of(planes, typ, 13))
    x = B.int_rows(rng, rows, planes)
    mean, invstd, gam, beta = B.exact_params(rng, planes)
    special = (np.nan, np.inf, -np.inf, -0.0)
    where = rng.permutation(rows * planes)[:24]
    x.reshape(-1)[where] = np.resize(np.float32(special), 24)
    B.assert_exact_apply(x, mean, invstd, gam, beta, leak)
    bn_last_form()
    out = SCN.bn_apply(to_dev(x, dev, typ), to_dev(mean, dev), to_dev(invstd, dev), to_dev(gam, dev), to_dev(beta, dev), leak)
    assert_form("non-finite", B.expect_bn(rows, planes, typ, apply=True))
    got = to_np(out)
    B.check_apply("non-finite", got, x, mean, invstd, gam, beta, leak, True, typ == BF16)
    nan_in = np.isnan(x)
    assert nan_in.sum() == 6
    if leak == 0:
        assert np.isfinite(got[nan_in]).all() and (got[nan_in] == 0).all() and (got >= 0).all()
    else:
        assert np.isnan(got[nan_in]).all() and np.isnan(got).sum() == 6


def test_no_rows_no_launch(dev):
    SCN = _scn()
    for typ in (F32, BF16):
        dt = torch.bfloat16 if typ == BF16 else torch.float32
        x = torch.empty((0, 64), device=dev, dtype=dt)
        ones = torch.ones(64, device=dev)
        bn_last_form()
        assert SCN.bn_apply(x, ones, ones, None, None, 0.0).shape == (0, 64)
        sm, si = torch.full((64,), 7.0, device=dev), torch.full((64,), 7.0, device=dev)
        rm, rv = torch.full((64,), 3.0, device=dev), torch.full((64,), 5.0, device=dev)
        SCN.BatchNormalization_updateOutput(x, x.new_empty(0), sm, si, rm, rv, None, None, EPS, 0.9, True, 0.0)
        dw, db = torch.full((64,), 9.0, device=dev), torch.full((64,), 9.0, device=dev)
        SCN.BatchNormalization_backward(x, x.new_empty(0), x, x, sm, si, None, None, None, None, dw, db, 0.0)
        assert bn_last_form() == B.expect_bn(0, 64, typ, stats=("tensor", 1), apply=True, backward=True)
        for t, v in ((sm, 7.0), (si, 7.0), (rm, 3.0), (rv, 5.0), (dw, 9.0), (db, 9.0)):
            assert bool((t == v).all())


def test_bf16_rows_have_no_general_apply_kernel(dev):
    from detection_3d_amd._lib import D3DError
    SCN = _scn()
    x = torch.zeros((3, 2048), device=dev, dtype=torch.bfloat16)
    ones = torch.ones(2048, device=dev)
    bn_last_form()
    with pytest.raises(D3DError):
        SCN.bn_apply(x, ones, ones, None, None, 0.0)
    assert bn_last_form() == dict.fromkeys(B.BN_FIELDS, 0)


# ------------------------------------------------------------------------------------------------------- backward
def _run_backward(dev, planes, rows, typ, aligned16, variant, exact_data):
    SCN = _scn()
    x, y, dy, mean, invstd, w, leak = B.make_backward_case(planes, rows, typ, variant, exact_data)
    want_sums = variant[1]                       # d_weight / d_bias present, or NULL
    if exact_data:
        B.assert_exact_backward(x, y, dy, mean, invstd, leak)
    ref = B.backward_ref(x, y, dy, mean, invstd, w, leak)
    tag = f"backward C={planes} rows={rows} {'bf16' if typ == BF16 else 'fp32'} {variant} aligned={aligned16}"
    if aligned16:
        xt = to_dev(x, dev, typ)
    else:                                        # a row-sliced view: 8-byte aligned rows of 4 bf16 values
        base = torch.zeros((rows + 1, planes), device=dev, dtype=torch.bfloat16)
        base[1:] = to_dev(x, dev, typ)
        xt = base[1:]
        assert xt.is_contiguous() and xt.data_ptr() % 16 == 8
    yt, dyt = to_dev(y, dev, typ), to_dev(dy, dev, typ)
    d_in = xt.new_empty(0)
    dw = torch.full((planes,), 77.0, device=dev) if want_sums else None
    db = torch.full((planes,), 77.0, device=dev) if want_sums else None
    bn_last_form()
    SCN.BatchNormalization_backward(xt, d_in, yt, dyt, to_dev(mean, dev), to_dev(invstd, dev), None, None, to_dev(w, dev),
                                    None, dw, db, leak)
    assert_form(tag, B.expect_bn(rows, planes, typ, backward=True, aligned16=aligned16))
    assert d_in.shape == xt.shape and d_in.dtype == xt.dtype
    B.check_backward(tag, ref, to_np(d_in), to_np(dw) if want_sums else None, to_np(db) if want_sums else None,
                     exact_data, typ == BF16)


BACKWARD_PLANES = sorted({c[0] for c in B.backward_cases()})


@pytest.mark.parametrize("typ", [F32, BF16])
@pytest.mark.parametrize("planes", BACKWARD_PLANES)
def test_backward(dev, planes, typ):
    for i, (c, rows, t, aligned16) in enumerate(B.backward_cases()):
        if c != planes or t != typ or not aligned16:
            continue
        for j, exact_data in enumerate(_kinds(rows, planes)):
            _run_backward(dev, planes, rows, typ, True, B.VARIANTS[(i + 3 * j) % len(B.VARIANTS)], exact_data)


def test_backward_unaligned_rows(dev):
    """the alignment branch of `vec4`: bf16 rows of 4 channels starting 8 bytes past a 16-byte boundary"""
    cases = [c for c in B.backward_cases() if not c[3]]
    assert len(cases) == 6
    for i, (planes, rows, typ, _) in enumerate(cases):
        assert B.expect_backward(rows, planes, typ, True)["bw_partial"] == B.PARTIAL_VEC4
        for j, exact_data in enumerate((True, False)):
            _run_backward(dev, planes, rows, typ, False, B.VARIANTS[(i + 3 * j) % len(B.VARIANTS)], exact_data)


def test_backward_forms_reached():
    forms = [B.expect_backward(r, c, t, a) for c, r, t, a in B.backward_cases()]
    for typ in (F32, BF16):
        mine = [f for f in forms if f["bw_type"] == typ]
        assert {(f["bw_partial"], f["bw_apply"]) for f in mine} == \
            {(B.PARTIAL_VEC4, B.ROWS), (B.PARTIAL_VEC4, B.VEC4), (B.PARTIAL_SCALAR, B.SCALAR)}
        assert {1, 2, 7, 8, 9, 128} <= {f["bw_slices"] for f in mine if f["bw_partial"] == B.PARTIAL_VEC4}
        assert {1, 2, 128} <= {f["bw_slices"] for f in mine if f["bw_partial"] == B.PARTIAL_SCALAR}
        assert {0, 1} == {f["bw_multi"] for f in mine if f["bw_apply"] == B.ROWS}


@pytest.mark.parametrize("planes,rows,typ,leak", [(32, 1000, F32, 0.333), (128, 300, BF16, 0.333), (256, 77, F32, 0.0)])
def test_module_train_path(dev, planes, rows, typ, leak):
    """BatchNormLeakyReLU in train mode: its forward is the direct call to the bit, its backward gets the saved mean and
    invstd of that forward and the OUTPUT for the sign -- a reference that takes the sign from the input fails"""
    from detection_3d_amd import sparseconvnet as scn
    SCN = _scn()
    rng = np.random.RandomState(B.seed_of(planes, rows, typ, 14))
    x = B.normal_rows(rng, rows, planes, typ == BF16)
    g = rng.randn(rows, planes).astype(np.float32)
    if typ == BF16:
        g = B.bf16_round(g)
    gam, beta = B.f32(rng.uniform(0.5, 1.5, planes)), B.f32(rng.uniform(-0.5, 0.5, planes))
    rm, rv = B.f32(rng.uniform(0.5, 1.5, planes)), B.f32(rng.uniform(0.5, 2.0, planes))
    bn = scn.BatchNormLeakyReLU(planes, eps=EPS, momentum=0.9, leakiness=leak).to(dev).train()
    with torch.no_grad():
        bn.weight.copy_(to_dev(gam, dev))
        bn.bias.copy_(to_dev(beta, dev))
        bn.running_mean.copy_(to_dev(rm, dev))
        bn.running_var.copy_(to_dev(rv, dev))
    # the direct call on copies of the running statistics
    xd = to_dev(x, dev, typ)
    y_direct, sm, si = xd.new_empty(0), torch.empty(planes, device=dev), torch.empty(planes, device=dev)
    rmt, rvt = to_dev(rm, dev), to_dev(rv, dev)
    SCN.BatchNormalization_updateOutput(xd, y_direct, sm, si, rmt, rvt, to_dev(gam, dev), to_dev(beta, dev), EPS, 0.9, True, leak)
    xt = to_dev(x, dev, typ).requires_grad_(True)
    bn_last_form()
    y = bn(scn.SparseConvNetTensor(xt, None, torch.tensor([8, 8, 8]))).features
    assert_form("module forward", B.expect_bn(rows, planes, typ, stats=("tensor", 1), apply=True))
    assert torch.equal(y.detach(), y_direct) and torch.equal(bn.running_mean, rmt) and torch.equal(bn.running_var, rvt)
    ref_stats = B.stats_ref(x)
    B.check_stats("module", ref_stats, 1, EPS, to_np(sm), to_np(si), False,
                  running=(rm, rv, 0.9, to_np(bn.running_mean), to_np(bn.running_var)))
    # the record belongs to the thread that launched: autograd's worker here.  A hook on the input's gradient runs on
    # that thread right after the BatchNorm node
    seen = []
    xt.register_hook(lambda grad: seen.append(bn_last_form()))
    y.backward(to_dev(g, dev, typ))
    want = B.expect_bn(rows, planes, typ, backward=True)
    assert seen == [want], f"module backward: the launch form differs: {seen} (expected {want})"
    yn = to_np(y_direct)
    ref = B.backward_ref(x, yn, g, to_np(sm), to_np(si), gam, leak)
    got = (to_np(xt.grad), to_np(bn.weight.grad), to_np(bn.bias.grad))
    B.check_backward("module", ref, *got, False, typ == BF16)
    assert ((x > 0) != (yn > 0)).mean() > 0.2                  # the input's sign is another mask
    with pytest.raises(AssertionError):
        B.check_backward("sign from the input", B.backward_ref(x, x, g, to_np(sm), to_np(si), gam, leak), *got, False,
                         typ == BF16)
    with pytest.raises(AssertionError):                         # and the running statistics are other values
        B.check_backward("running statistics", B.backward_ref(x, yn, g, rm, B.f32(B.invstd_of(rv, EPS)), gam, leak),
                         *got, False, typ == BF16)


# ----------------------------------------------------------------------------------------------------------- k_add
def test_add(dev):
    """d3d_add: the exact fp32 sum, float4 body and scalar tail, nothing written past n"""
    from detection_3d_amd._lib import check, lib, ptr, stream_of
    rng = np.random.RandomState(15)
    for n in B.ADD_SIZES:
        a, b = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
        buf = torch.full((n + 8,), -123.0, device=dev)
        out = buf[4:4 + n]
        assert out.data_ptr() % 16 == 0
        at, bt = to_dev(a, dev), to_dev(b, dev)
        check(lib().d3d_add(ptr(at), ptr(bt), ptr(out), n, stream_of()))
        got = buf.cpu().numpy()
        assert B.same_bits(got[4:4 + n], a + b), n
        assert (got[:4] == -123.0).all() and (got[4 + n:] == -123.0).all(), n
    B.MARGINS.setdefault("add (bit for bit)", 0.0)


# ---------------------------------------------------------------------------------------------------------- record
def test_read_clears_the_record(dev):
    from detection_3d_amd._lib import lib
    SCN = _scn()
    x = torch.ones((5, 64), device=dev)
    SCN.batch_stats(x)
    assert bn_last_form()["st_src"] == B.TENSOR
    assert bn_last_form() == dict.fromkeys(B.BN_FIELDS, 0)
    assert lib().d3d_bn_last_form(None, 0) == len(B.BN_FIELDS)


def test_zz_margins(dev):
    """the largest error every check saw, as a fraction of its bound (printed for DESIGN.md; sets nothing)"""
    assert B.MARGINS and all(0 <= v <= 1 for v in B.MARGINS.values())
    print("\nBN_MARGINS " + json.dumps({k: round(v, 4) for k, v in sorted(B.MARGINS.items())}))
