"""The references, preconditions, comparators and expected-form arithmetic of test_bn_forms_gpu.py, checked without a
GPU: against the CPU oracle (fp32, SCN's own loops), against torch's fp64 autograd of the same expression, at the
documented thresholds, and by mutation -- a reference that lost a row, counted one twice, lost a slice's share or uses
y >= 0 must fail the comparator of its case, or the tolerances could not see the faults they are there for."""
import numpy as np
import pytest
import torch

import oracle
from tests import bn_forms as B
from tests.bn_forms import BF16, F32


def _rng(*key):
    return np.random.RandomState(B.seed_of(*key))


# ------------------------------------------------------------------------------------------------- the references
def test_statistics_equal_the_oracle_on_integer_rows():
    """64 rows (a power of two) of integers: the oracle's fp32 sums, its mean and its running mean are exact, the
    variances take one or two fp32 roundings, powf one more"""
    rng = _rng(1)
    x = B.int_rows(rng, 64, 24)
    B.assert_exact_rows(x)
    ref = B.stats_ref_exact(*B.col_sums(x), 64)
    two_pass = B.stats_ref(x)
    assert np.array_equal(ref["mean"], two_pass["mean"]) and np.allclose(ref["m2"], two_pass["m2"], rtol=1e-14, atol=0)
    rm, rv, mom = B.exact_running(rng, 24)
    _, sm, si, rm2, rv2 = oracle.bn_forward(x, rm, rv, None, None, B.EPS, mom, True, 0.0)
    B.check_stats("oracle", ref, 1, B.EPS, sm, si, True, running=(rm, rv, mom, rm2, rv2))
    assert B.same_bits(rm2, B.running_update(rm, ref["mean"], mom))
    # torch fp64 of the same columns
    xt = torch.from_numpy(x).double()
    assert np.array_equal(xt.mean(0).numpy(), ref["mean"])
    assert np.allclose(xt.var(0).numpy(), ref["var_u"], rtol=1e-14, atol=0)
    assert np.allclose(xt.var(0, unbiased=False).numpy(), ref["var_b"], rtol=1e-14, atol=0)


def test_statistics_against_the_oracle_on_normal_rows():
    """the oracle adds in fp32, one pass: mean within gamma_n sum|x| / n, m2 within gamma_(n+3) (q + mean^2 n)"""
    rng = _rng(2)
    n = 300
    x = B.normal_rows(rng, n, 12)
    ref = B.stats_ref(x)
    assert ref["kappa"][2] > 1000 > ref["kappa"][1] and ref["kappa"][0] < 1.5        # the ratio-64 column is the hard one
    _, sm, si, rm, rv = oracle.bn_forward(x, np.zeros(12), np.ones(12), None, None, B.EPS, 0.9, True, 0.0)
    amean = np.abs(x.astype(np.float64)).sum(0) / n
    B.within("oracle mean", sm, ref["mean"], B.gamma(n + 1) * amean)
    m2_err = B.gamma(n + 3) * (ref["q"] + ref["mean"] ** 2 * n) + 2 * n * np.abs(ref["mean"]) * B.gamma(n + 1) * amean
    want = B.invstd_of(ref["var_b"], B.EPS)
    B.within("oracle invstd", si, want, 4 * B.ulp32(want) + 0.5 * want * m2_err / ref["m2"])
    xt = torch.from_numpy(x).double()
    assert np.allclose(xt.var(0).numpy(), ref["var_u"], rtol=1e-12, atol=0)


def test_one_row():
    """rows = 1 as the code defines it: the mean is the row, the unbiased variance 0 / 0"""
    x = np.float32([[3, -1, 2, 4]])
    ref = B.stats_ref_exact(*B.col_sums(x), 1)
    assert np.array_equal(ref["mean"], x[0]) and np.isnan(ref["var_u"]).all() and (ref["var_b"] == 0).all()
    assert np.allclose(B.invstd_of(ref["var_b"], B.EPS), 100.0, rtol=1e-6)
    B.check_stats("one row", ref, 0, B.EPS, x[0], np.full(4, np.nan, np.float32), True)
    with pytest.raises(AssertionError):
        B.check_stats("one row", ref, 0, B.EPS, x[0], np.zeros(4, np.float32), True)


@pytest.mark.parametrize("leak", [0.0, 0.25])
def test_apply_equals_the_oracle_on_exact_data(leak):
    rng = _rng(3)
    x = B.int_rows(rng, 50, 24)
    mean, invstd, gam, beta = B.exact_params(rng, 24, pow2_invstd=True)
    B.assert_exact_apply(x, mean, invstd, gam, beta, leak)
    # eval mode with eps 0 and running variance invstd^-2: powf gives these powers of two back exactly
    out, sm, si, _, _ = oracle.bn_forward(x, mean, invstd.astype(np.float64) ** -2, gam, beta, 0.0, 0.9, False, leak)
    assert B.same_bits(sm, mean) and B.same_bits(si, invstd)
    want = B.apply_ref(x, mean, invstd, gam, beta, leak)[0]
    if leak:
        assert B.same_bits(out, want)
        B.check_apply("oracle", out, x, mean, invstd, gam, beta, leak, True, False)
    else:
        assert np.array_equal(out, want.astype(np.float32))          # t * 0 leaves -0 where max(t, 0) gives +0
    assert B.same_bits(B.bf16_round(want.astype(np.float32)), torch.from_numpy(want).float().bfloat16().float().numpy())


def test_apply_against_the_oracle_and_torch_on_normal_data():
    rng = _rng(4)
    x, mean, invstd, gam, beta, leak = B.make_apply_case(24, 200, F32, (True, True, 0.25), False)
    assert leak == 0.333
    out = oracle.bn_forward(x, mean, invstd.astype(np.float64) ** -2, gam, beta, 0.0, 0.9, False, leak)[0]
    si = oracle.bn_forward(x, mean, invstd.astype(np.float64) ** -2, gam, beta, 0.0, 0.9, False, leak)[2]
    B.check_apply("oracle", out, x, mean, si, gam, beta, leak, False, False)
    t = (torch.from_numpy(x).double() - torch.from_numpy(mean).double()) * torch.from_numpy(si).double() \
        * torch.from_numpy(gam).double() + torch.from_numpy(beta).double()
    y = torch.where(t > 0, t, t * float(np.float32(leak))).numpy()
    want, mag = B.apply_ref(x, mean, si, gam, beta, leak)
    assert (np.abs(y - want) <= 8 * 2.0 ** -53 * mag).all()


def test_non_finite_inputs_of_the_apply_reference():
    x = np.float32([[np.nan, np.inf, -np.inf, -0.0, 2.0, -2.0]])
    one, zero = np.ones(6, np.float32), np.zeros(6, np.float32)
    y0 = B.apply_ref(x, zero, one, None, None, 0.0)[0].astype(np.float32)
    assert B.same_bits(y0, np.float32([[0.0, np.inf, 0.0, 0.0, 2.0, 0.0]]))       # max(t, 0): NaN -> +0
    y1 = B.apply_ref(x, zero, one, None, None, 0.25)[0].astype(np.float32)
    assert B.same_bits(y1, np.float32([[np.nan, np.inf, -np.inf, 0.0, 2.0, -0.5]]))
    assert not B.same_bits(y0, y1)


def _torch_backward(x, dy, w, b, eps, leak):
    xt = torch.from_numpy(np.asarray(x, np.float64)).requires_grad_(True)
    wt = torch.from_numpy(np.asarray(w, np.float64)).requires_grad_(True)
    bt = torch.from_numpy(np.asarray(b, np.float64)).requires_grad_(True)
    mean, var = xt.mean(0), xt.var(0, unbiased=False)
    invstd = (var + eps) ** -0.5
    t = (xt - mean) * invstd * wt + bt
    y = torch.where(t > 0, t, t * leak)
    (y * torch.from_numpy(np.asarray(dy, np.float64))).sum().backward()
    return y.detach().numpy(), mean.detach().numpy(), invstd.detach().numpy(), xt.grad.numpy(), wt.grad.numpy(), bt.grad.numpy()


@pytest.mark.parametrize("exact_data", [True, False])
def test_backward_equals_torch_autograd(exact_data):
    """BatchNormalization.cpp:62-107 is the gradient through the batch statistics (biased variance)"""
    rng = _rng(5, exact_data)
    x = B.int_rows(rng, 64, 12) if exact_data else B.normal_rows(rng, 150, 12)
    dy = B.int_rows(rng, *x.shape) if exact_data else rng.randn(*x.shape).astype(np.float32)
    w, b = rng.uniform(0.5, 1.5, 12), rng.uniform(-0.5, 0.5, 12)
    leak = 0.25 if exact_data else float(np.float32(0.333))
    y, mean, invstd, dx, dw, db = _torch_backward(x, dy, w, b, B.EPS, leak)
    ref = B.backward_ref(x, y, dy, mean, invstd, w, leak)
    if exact_data:
        assert np.array_equal(db, ref["d_bias"])
    scale = ref["isw"] * (np.abs(ref["d"]) + np.abs(ref["gm"]) + np.abs(ref["xm"] * ref["k"]))
    assert (np.abs(dx - ref["dx"]) <= 1e-12 * scale + 1e-13).all()
    assert (np.abs(dw - ref["d_weight"]) <= 1e-12 * ref["a_dp"] * invstd).all()
    assert (np.abs(db - ref["d_bias"]) <= 1e-12 * ref["a_bias"]).all()


def test_backward_equals_the_oracle():
    """integer data, 64 rows: d_bias and d_weight to the bit, dx inside the comparator's bound; normal data: the
    oracle's fp32 sums within gamma_n of their magnitudes"""
    x, y, dy, mean, invstd, gam, leak = B.make_backward_case(24, 64, F32, (True, True, 0.25), True)
    ref = B.assert_exact_backward(x, y, dy, mean, invstd, leak)
    assert (y == 0).any() and np.signbit(y[y == 0]).any() and not np.signbit(y[y == 0]).all()
    ref = B.backward_ref(x, y, dy, mean, invstd, gam, leak)
    d_in, dw, db = oracle.bn_backward(x, y, dy, mean, invstd, gam, leak)
    B.check_backward("oracle", ref, d_in, dw, db, True, False)
    x, y, dy, mean, invstd, gam, leak = B.make_backward_case(12, 200, F32, (True, True, 0.25), False)
    ref = B.backward_ref(x, y, dy, mean, invstd, gam, leak)
    d_in, dw, db = oracle.bn_backward(x, y, dy, mean, invstd, gam, leak)
    B.within("oracle d_bias", db, ref["d_bias"], B.gamma(201) * ref["a_bias"])
    B.within("oracle d_weight", dw, ref["d_weight"], B.gamma(204) * ref["a_dp"] * invstd)


# ------------------------------------------------------------------------------------------------ the preconditions
def test_exactness_preconditions_hold_for_every_case():
    for planes in B.STATS_PLANES:
        for _, rows in B.stats_cases(planes):
            x = B.int_rows(_rng(planes, rows), rows, planes)
            B.assert_exact_rows(x)
            B.assert_exact_sums(*B.col_sums(x), rows)
    for planes in B.PARTIALS_PLANES:
        for pr in B.partials_row_counts(planes):
            p, rows = B.make_partials(_rng(planes, pr), pr, planes)
            s, q = p.sum(0)[:planes], p.sum(0)[planes:]
            B.assert_exact_sums(s, q, rows)
            assert rows != pr and (q * rows > s * s).all()
    for i, (planes, rows, typ) in enumerate(B.apply_cases()):
        if rows * planes > 1 << 20 and i % 7:
            continue                                    # the same generator: every seventh of the large ones
        x, mean, invstd, w, b, leak = B.make_apply_case(planes, rows, typ, B.VARIANTS[i % len(B.VARIANTS)], True)
        B.assert_exact_rows(x)
        B.assert_exact_apply(x, mean, invstd, w, b, leak)
    for i, (planes, rows, typ, _) in enumerate(B.backward_cases()):
        if rows * planes > 1 << 20 and i % 7:
            continue
        x, y, dy, mean, invstd, w, leak = B.make_backward_case(planes, rows, typ, B.VARIANTS[i % len(B.VARIANTS)], True)
        B.assert_exact_rows(x)
        B.assert_exact_rows(dy)
        assert B.is_bf16(y)
        B.assert_exact_backward(x, y, dy, mean, invstd, leak)
    # the largest backward case by its sums
    planes, rows = max(((p, r) for p, r, _, _ in B.backward_cases()), key=lambda c: c[1])
    assert 4 * 6 * 4 * rows < 2 ** 24


def test_exactness_preconditions_trip():
    x = B.int_rows(_rng(7), 10, 4)
    for bad in (0.0, 0.5, 5.0, 257.0):
        y = x.copy()
        y[3, 1] = bad
        with pytest.raises(AssertionError):
            B.assert_exact_rows(y)
    with pytest.raises(AssertionError):
        B.assert_exact_sums(np.float64([2.0 ** 27]), np.float64([2.0 ** 54]), 4)
    with pytest.raises(AssertionError):
        B.assert_exact_sums(np.float64([1.5]), np.float64([3.0]), 4)
    mean, invstd, gam, beta = B.exact_params(_rng(8), 4)
    B.assert_exact_apply(x, mean, invstd, gam, beta, 0.25)
    with pytest.raises(AssertionError):
        B.assert_exact_apply(x, mean, invstd * np.float32(1 / 3), gam, beta, 0.25)
    with pytest.raises(AssertionError):
        B.assert_exact_apply(x, mean, invstd, gam, beta, 0.333)
    xb, y, dy, mean, invstd, gam, leak = B.make_backward_case(4, 10, F32, (True, True, 0.25), True)
    B.assert_exact_backward(xb, y, dy, mean, invstd, leak)
    with pytest.raises(AssertionError):
        B.assert_exact_backward(xb, y, dy, mean + np.float32(1e-3), invstd, leak)
    with pytest.raises(AssertionError):
        B.assert_exact_backward(xb, y, dy, mean, invstd, 0.333)
    with pytest.raises(AssertionError):
        B.assert_exact_backward(np.tile(xb, (200000, 1)), np.tile(y, (200000, 1)), np.tile(dy, (200000, 1)), mean, invstd, leak)
    assert B.is_bf16(np.float32([1.0, -3.5, 2.0 ** -100])) and not B.is_bf16(np.float32([1.0 + 2.0 ** -9]))
    assert B.bf16_round(np.float32([1.0 + 2.0 ** -8]))[0] == 1.0 and B.bf16_round(np.float32([1.0 + 3 * 2.0 ** -8]))[0] == 1.015625


# ---------------------------------------------------------------------------------------------- the expected forms
def _st(f):
    return tuple(f[k] for k in ("st_lanes", "st_row_lanes", "st_slices", "st_groups", "st_last_group", "st_per"))


def test_expected_statistics_forms_at_the_thresholds():
    # channel classes: butterfly up to 128 (LPR 1 .. 32), LDS row lanes from 256 on (LPR 64 .. 1024), down to RL = 1
    assert [B.expect_stats(1, c, F32, 0)["st_lanes"] for c in (4, 8, 16, 32, 64, 128)] == [1, 2, 4, 8, 16, 32]
    assert [B.expect_stats(1, c, F32, 0)["st_row_lanes"] for c in (256, 512, 1024, 2048, 4096)] == [16, 8, 4, 2, 1]
    # C = 1024: RL 4, T = 32 rows per slice at the least
    assert _st(B.expect_stats(32, 1024, F32, 0)) == (256, 4, 1, 1, 1, 32)
    assert _st(B.expect_stats(33, 1024, F32, 0)) == (256, 4, 2, 1, 2, 17)
    assert _st(B.expect_stats(512, 1024, BF16, 2)) == (256, 4, 16, 1, 16, 32)
    assert _st(B.expect_stats(513, 1024, BF16, 2)) == (256, 4, 17, 2, 1, 31)
    assert _st(B.expect_stats(127 * 32 + 1, 1024, F32, 1)) == (256, 4, 128, 8, 16, 32)
    assert B.slice_rows(127 * 32 + 1, 128)[-2:] == [32, 1]
    assert _st(B.expect_stats(10 ** 6, 1024, F32, 1)) == (256, 4, 128, 8, 16, 7813)
    # C = 4096, 1100 rows: 128 slices of 9 rows, 123 .. 127 empty
    assert _st(B.expect_stats(1100, 4096, F32, 0)) == (1024, 1, 128, 8, 16, 9)
    shares = B.slice_rows(1100, 128)
    assert shares[:122] == [9] * 122 and shares[122:] == [2, 0, 0, 0, 0, 0] and sum(shares) == 1100
    # C = 4: one slice up to 8192 rows, two groups from 131073
    assert _st(B.expect_stats(8192, 4, F32, 0)) == (1, 1024, 1, 1, 1, 8192)
    assert _st(B.expect_stats(8193, 4, F32, 0)) == (1, 1024, 2, 1, 2, 4097)
    assert _st(B.expect_stats(131073, 4, F32, 0)) == (1, 1024, 17, 2, 1, 7711)
    assert B.stats_row_counts(4, False) == [8192, 8193, 131073]
    rc = B.stats_row_counts(1024, True)
    assert rc == [1, 2, 3, 4, 5, 16, 17, 24, 28, 32, 33, 512, 513, 4065]
    assert 1100 in B.stats_row_counts(4096, True)
    for planes in (768, 6, 0, 8192, 20):
        assert not B.stats_planes_ok(planes)
    f = B.expect_stats(33, 1024, BF16, 2)
    assert (f["st_src"], f["st_type"], f["st_mode"]) == (B.TENSOR, BF16, 2)


def test_expected_partials_forms_at_the_thresholds():
    assert _st(B.expect_stats_partials(1, 4, 2)) == (8, 128, 1, 1, 1, 1)
    assert _st(B.expect_stats_partials(1024, 4, 2)) == (8, 128, 1, 1, 1, 1024)
    assert _st(B.expect_stats_partials(1025, 4, 0)) == (8, 128, 2, 1, 2, 513)
    assert _st(B.expect_stats_partials(16 * 1024 + 1, 4, 0)) == (8, 128, 17, 2, 1, 964)
    assert _st(B.expect_stats_partials(64 * 1024 + 1, 4, 0)) == (8, 128, 64, 4, 16, 1025)      # the cap of 64 slices
    assert _st(B.expect_stats_partials(9, 512, 2)) == (1024, 1, 2, 1, 2, 5)
    assert _st(B.expect_stats_partials(513, 4096, 2)) == (1024, 1, 64, 4, 16, 9)
    assert _st(B.expect_stats_partials(9, 12, 2))[:2] == (24, 42)
    f = B.expect_stats_partials(9, 512, 2)
    assert (f["st_src"], f["st_type"], f["st_mode"]) == (B.PARTIALS, B.F64, 2)
    assert [B.partials_planes_ok(p) for p in (4, 12, 512, 516, 768, 1024, 1280, 1536, 2048, 4096)] == \
        [True, True, True, False, False, True, False, True, True, True]
    assert _st(B.expect_stats_partials(9, 1536, 0)) == (1024, 1, 2, 1, 2, 5)
    for planes in B.PARTIALS_REFUSED:
        assert not B.partials_planes_ok(planes) and planes % 4 == 0
        with pytest.raises(AssertionError):
            B.expect_stats_partials(8, planes, 2)


def _ap(f):
    return f["ap_kernel"], f["ap_wgs"], f["ap_multi"]


def test_expected_apply_forms_at_the_thresholds():
    # C = 1024: one row per workgroup iteration, 2048 workgroups at the most, the 4-row loop from 3 * 2048 + 1 rows
    assert [_ap(B.expect_apply(r, 1024, F32)) for r in (1, 2048, 2049, 6144, 6145, 8193)] == \
        [(B.ROWS, 1, 0), (B.ROWS, 2048, 0), (B.ROWS, 2048, 0), (B.ROWS, 2048, 0), (B.ROWS, 2048, 1), (B.ROWS, 2048, 1)]
    assert _ap(B.expect_apply(65, 16, BF16)) == (B.ROWS, 2, 0) and _ap(B.expect_apply(64, 16, BF16)) == (B.ROWS, 1, 0)
    assert _ap(B.expect_apply(3 * 8192 + 5, 256, F32)) == (B.ROWS, 2048, 1)
    assert _ap(B.expect_apply(3 * 8192, 256, F32)) == (B.ROWS, 2048, 0)
    assert _ap(B.expect_apply(3 * 32768 + 17, 64, BF16)) == (B.ROWS, 2048, 1)
    assert _ap(B.expect_apply(3, 2048, F32)) == (B.VEC4, 7, 0) and _ap(B.expect_apply(1, 4096, F32)) == (B.VEC4, 5, 0)
    assert _ap(B.expect_apply(1027, 1, F32)) == (B.SCALAR, 2, 0) and _ap(B.expect_apply(4, 9, F32)) == (B.SCALAR, 1, 0)
    assert _ap(B.expect_apply(5, 768, F32)) == (B.VEC4, 4, 0)          # C4 = 192 does not divide 256
    with pytest.raises(AssertionError):
        B.expect_apply(3, 2048, BF16)
    assert sorted({(r * c) % 4 for c, r, _ in B.apply_cases() if c in (1, 6, 9)}) == [0, 1, 2, 3]


def _bw(f):
    return f["bw_partial"], f["bw_slices"], f["bw_apply"], f["bw_wgs"], f["bw_multi"]


def test_expected_backward_forms_at_the_thresholds():
    V, S = B.PARTIAL_VEC4, B.PARTIAL_SCALAR
    # C = 1024: RL 4, 32 rows per slice, no grouping; the apply pass' two-row loop from 2049 rows
    assert [_bw(B.expect_backward(r, 1024, F32)) for r in (32, 33, 2048, 2049, 4097)] == \
        [(V, 1, B.ROWS, 32, 0), (V, 2, B.ROWS, 33, 0), (V, 64, B.ROWS, 2048, 0), (V, 65, B.ROWS, 2048, 1),
         (V, 128, B.ROWS, 2048, 1)]
    assert [B.expect_backward(r, 1024, BF16)["bw_slices"] for r in (193, 225, 257, 4065, 4097)] == [7, 8, 9, 128, 128]
    assert _bw(B.expect_backward(3, 2048, F32)) == (V, 1, B.VEC4, 6, 0)
    assert _bw(B.expect_backward(1100, 4096, BF16)) == (V, 128, B.VEC4, 4400, 0)
    # the scalar partial kernel: planes 1 and 2, planes 768 (192 does not divide 1024), unaligned rows
    assert [B.expect_backward(r, 1, F32)["bw_slices"] for r in (1, 63, 64, 65, 8191, 8192)] == [1, 1, 1, 2, 128, 128]
    assert _bw(B.expect_backward(65, 2, BF16)) == (S, 2, B.SCALAR, 1, 0)
    assert _bw(B.expect_backward(8191, 768, F32)) == (S, 128, B.SCALAR, 24573, 0)
    assert _bw(B.expect_backward(65, 4, BF16, aligned16=False)) == (S, 2, B.SCALAR, 2, 0)
    assert _bw(B.expect_backward(65, 4, BF16)) == (V, 1, B.ROWS, 1, 0)
    for planes in (3, 6, 9, 384):
        assert not B.backward_planes_ok(planes)
    reached = {B.expect_backward(r, p, t, a)["bw_slices"] for p, r, t, a in B.backward_cases()}
    assert {1, 2, 7, 8, 9, 128} <= reached


def test_expect_bn_composes_the_sections():
    f = B.expect_bn(513, 1024, BF16, stats=("tensor", 1), apply=True)
    assert f["st_slices"] == 17 and f["ap_wgs"] == 513 and f["bw_partial"] == 0 and set(f) == set(B.BN_FIELDS)
    f = B.expect_bn(40, 9, F32, stats="running", apply=True)
    assert (f["st_src"], f["st_slices"], f["ap_kernel"]) == (B.RUNNING, 0, B.SCALAR)
    f = B.expect_bn(100, 128, F32, stats=("partials", 2, 9))
    assert (f["st_src"], f["st_slices"], f["st_per"], f["ap_kernel"]) == (B.PARTIALS, 1, 9, 0)
    assert B.expect_bn(0, 64, F32, stats=("tensor", 1), apply=True, backward=True) == dict.fromkeys(B.BN_FIELDS, 0)
    assert B.expect_bn(65, 4, BF16, backward=True, aligned16=False)["bw_partial"] == B.PARTIAL_SCALAR
    assert len(B.BN_FIELDS) == 19


# ---------------------------------------------------------------------------------------------------- mutations
def _stats_outputs(x, rows, eps, mode):
    """what a statistics launch over x would return if it divided by `rows` (fp64 arithmetic, fp32 outputs)"""
    s, q = B.col_sums(x)
    mean, m2, var_u, var_b = B.stats_from_sums(s, q, rows)
    return B.f32(mean), B.f32(var_u if mode == 0 else B.invstd_of(var_b if mode == 1 else var_u, eps))


@pytest.mark.parametrize("exact_data", [True, False])
@pytest.mark.parametrize("planes,rows", [(4096, 1100), (32, 130049), (1024, 513)])
def test_statistics_comparator_sees_a_lost_row_a_doubled_row_and_a_lost_slice(planes, rows, exact_data):
    rng = _rng(planes, rows, exact_data)
    x = B.int_rows(rng, rows, planes) if exact_data else B.normal_rows(rng, rows, planes)
    ref = B.stats_ref_exact(*B.col_sums(x), rows) if exact_data else B.stats_ref(x)
    nblk = B.expect_stats(rows, planes, F32, 0)["st_slices"]
    per = B.cdiv(rows, nblk)
    last = max(b for b, n in enumerate(B.slice_rows(rows, nblk)) if n)
    mutants = {"none": x,
               "a row lost": np.delete(x, rows // 2, 0),
               "the last row lost": x[:-1],
               "a row doubled": np.concatenate([x, x[7:8]]),
               "the last slice's share lost": x[:last * per],
               "a middle slice's share lost": np.delete(x, np.s_[per:2 * per], 0)}
    for name, xm in mutants.items():
        for mode in (0, 1, 2):
            got = _stats_outputs(xm, rows, B.EPS, mode)
            if name == "none":
                B.check_stats(name, ref, mode, B.EPS, *got, exact_data)
                continue
            # the columns with mean / std 0 and 1 see a row in the mean; the ratio-64 columns see it too
            with pytest.raises(AssertionError):
                B.check_stats(name, ref, mode, B.EPS, *got, exact_data)
            if mode == 0:     # and each output on its own
                with pytest.raises(AssertionError):
                    B.check_stats(name, ref, mode, B.EPS, got[0], _stats_outputs(x, rows, B.EPS, 0)[1], exact_data)


@pytest.mark.parametrize("exact_data", [True, False])
def test_variance_comparator_sees_a_lost_row_with_the_mean_right(exact_data):
    """the sum of squares alone lost a row (the mean is from the whole tensor)"""
    rows, planes = 4065, 12
    rng = _rng(rows, exact_data, 2)
    x = B.int_rows(rng, rows, planes) if exact_data else B.normal_rows(rng, rows, planes)
    ref = B.stats_ref_exact(*B.col_sums(x), rows) if exact_data else B.stats_ref(x)
    s, q = B.col_sums(x)
    q_less = q - x[5].astype(np.float64) ** 2
    for mode in (0, 1, 2):
        mean, m2, var_u, var_b = B.stats_from_sums(s, q_less, rows)
        other = var_u if mode == 0 else B.invstd_of(var_b if mode == 1 else var_u, B.EPS)
        with pytest.raises(AssertionError):
            B.check_stats("q lost a row", ref, mode, B.EPS, B.f32(mean), B.f32(other), exact_data)


@pytest.mark.parametrize("exact_data", [True, False])
def test_running_statistics_comparator_sees_a_swapped_momentum(exact_data):
    rows, planes = 100, 12
    rng = _rng(rows, exact_data, 3)
    x = B.int_rows(rng, rows, planes) if exact_data else B.normal_rows(rng, rows, planes)
    ref = B.stats_ref_exact(*B.col_sums(x), rows) if exact_data else B.stats_ref(x)
    rm, rv, mom = B.exact_running(rng, planes)
    if not exact_data:
        mom = 0.9
    mean, invstd = _stats_outputs(x, rows, B.EPS, 1)
    good = (B.f32(B.running_update(rm, ref["mean"], mom)), B.f32(B.running_update(rv, ref["var_u"], mom)))
    B.check_stats("running", ref, 1, B.EPS, mean, invstd, exact_data, running=(rm, rv, mom) + good)
    swapped = (B.f32(B.running_update(rm, ref["mean"], 1 - mom)), B.f32(B.running_update(rv, ref["var_u"], 1 - mom)))
    biased = (good[0], B.f32(B.running_update(rv, ref["var_b"], mom)))
    for bad in (swapped, biased, (good[0], swapped[1]), (swapped[0], good[1])):
        with pytest.raises(AssertionError):
            B.check_stats("running", ref, 1, B.EPS, mean, invstd, exact_data, running=(rm, rv, mom) + bad)


@pytest.mark.parametrize("typ", [F32, BF16])
@pytest.mark.parametrize("exact_data", [True, False])
def test_apply_comparator_sees_a_wrong_element(exact_data, typ):
    x, mean, invstd, w, b, leak = B.make_apply_case(64, 33, typ, (True, True, 0.25), exact_data)
    y = B.apply_ref(x, mean, invstd, w, b, leak)[0].astype(np.float32)
    if typ == BF16:
        y = B.bf16_round(y)
    B.check_apply("none", y, x, mean, invstd, w, b, leak, exact_data, typ == BF16)
    for name, bad in (("a row not written", np.where(np.arange(33)[:, None] == 32, 0, y)),
                      ("the row above instead", np.roll(y, 1, 0)),
                      ("no bias", B.apply_ref(x, mean, invstd, w, None, leak)[0]),
                      ("the other slope", B.apply_ref(x, mean, invstd, w, b, 0.0)[0])):
        with pytest.raises(AssertionError):
            B.check_apply(name, B.f32(bad), x, mean, invstd, w, b, leak, exact_data, typ == BF16)
    if typ == BF16 and exact_data:      # truncation instead of round-to-nearest-even
        full = B.apply_ref(x, mean, invstd, w, b, leak)[0].astype(np.float32)
        trunc = (full.view(np.uint32) & 0xFFFF0000).view(np.float32)
        if not B.same_bits(trunc, y):
            with pytest.raises(AssertionError):
                B.check_apply("truncated", trunc, x, mean, invstd, w, b, leak, True, True)


@pytest.mark.parametrize("typ", [F32, BF16])
@pytest.mark.parametrize("exact_data", [True, False])
@pytest.mark.parametrize("planes,rows", [(1024, 257), (2, 8191), (32, 1025)])
def test_backward_comparator_sees_lost_rows_slices_and_the_sign_rule(planes, rows, exact_data, typ):
    x, y, dy, mean, invstd, w, leak = B.make_backward_case(planes, rows, typ, (True, True, 0.25), exact_data)
    ref = B.backward_ref(x, y, dy, mean, invstd, w, leak)
    bf = typ == BF16

    def outputs(r, n=rows):
        """what the kernels would write from the sums of r (fp64 arithmetic, fp32 / bf16 outputs), dividing by n"""
        gm, k = r["d_bias"] / n, r["dp"] * r["invstd"] ** 2 / n
        dx = B.f32((ref["d"] - gm - ref["xm"] * k) * ref["invstd"] * (1.0 if w is None else w.astype(np.float64)))
        return (B.bf16_round(dx) if bf else dx), B.f32(r["d_weight"]), B.f32(r["d_bias"])

    B.check_backward("none", ref, *outputs(ref), exact_data, bf)
    nblk = B.expect_backward(rows, planes, typ)["bw_slices"]
    per = B.cdiv(rows, nblk)
    keep_all = np.ones(rows, bool)

    def without(mask):
        return B.backward_ref(x[mask], y[mask], dy[mask], mean, invstd, w, leak)

    lost_row, lost_slice = keep_all.copy(), keep_all.copy()
    lost_row[rows // 3] = False
    lost_slice[(nblk - 1) * per:] = False
    twice = np.concatenate([np.arange(rows), [11]])
    mutants = {"a row lost": without(lost_row), "the last slice's share lost": without(lost_slice),
               "a row doubled": B.backward_ref(x[twice], y[twice], dy[twice], mean, invstd, w, leak)}
    for name, r in mutants.items():
        dx, dw, db = outputs(r)
        with pytest.raises(AssertionError):
            B.check_backward(name, ref, outputs(ref)[0], None, db, exact_data, bf)
        with pytest.raises(AssertionError):
            B.check_backward(name, ref, outputs(ref)[0], dw, None, exact_data, bf)
        if not bf:      # one row in `rows` moves gm and k by 1 / rows of the column's sum: above fp32 rounding,
            with pytest.raises(AssertionError):     # below bf16's -- there the sums above are what sees it
                B.check_backward(name, ref, dx, None, None, exact_data, bf)
    # the sign rule: y = 0 and y = -0 take the leak slope
    ge = B.backward_ref(x, y, dy, mean, invstd, w, leak, sign_ge=True)
    if exact_data:
        assert (y == 0).any()
        d_ge = ge["d"]
        dx_ge = B.f32((d_ge - ge["gm"] - ge["xm"] * ge["k"]) * ge["invstd"] * w.astype(np.float64))
        with pytest.raises(AssertionError):
            B.check_backward("y >= 0", ref, outputs(ref)[0], None, B.f32(ge["d_bias"]), True, bf)
        with pytest.raises(AssertionError):
            B.check_backward("y >= 0", ref, B.bf16_round(dx_ge) if bf else dx_ge, None, None, True, bf)
    else:
        assert not (y == 0).any() and np.array_equal(ge["d_bias"], ref["d_bias"])    # no zero output: the rules agree


def test_add_sizes():
    assert set(B.ADD_SIZES) >= {1, 3, 4, 5, 1023, 1024, 1025, 1024, 1025, 1026, 1027, 3072, 3075}
    assert {n % 4 for n in B.ADD_SIZES} == {0, 1, 2, 3}
