"""The reference and the expected-form arithmetic of test_dweight_forms_gpu.py, checked without a GPU."""
import numpy as np
import pytest

import oracle
from tests.dweight_forms import (ASYNC, BF16, CALLER, F32, LANE, assert_exact_precondition, dw64, expect_dw, gamma,
                                 rules_per_offset)
from tests.helpers import nbr_to_rules


def _small_scene(seed=0, n=300, side=9):
    rng = np.random.RandomState(seed)
    cells = rng.permutation(side ** 3)[:n]
    loc = np.stack([cells // (side * side), (cells // side) % side, cells % side, 0 * cells], 1).astype(np.int64)
    nbr, _ = oracle.subm_nbr(loc, [3, 3, 3])
    return loc, nbr_to_rules(nbr).astype(np.int64)


def test_dw64_equals_the_oracle():
    """the numpy dW of the GPU tests against oracle.rule_conv_backward (fp32 sums, rule by rule): integer data equal to
    the bit, normal data within gamma_n |x|^T |gout|; every offset has rules and they differ in number"""
    loc, rules = _small_scene()
    counts = rules_per_offset(rules, 27)
    assert counts.min() > 0 and counts[13] == len(loc) and len(set(counts.tolist())) > 3
    rng = np.random.RandomState(1)
    cin, cout = 9, 32
    w = np.zeros((27, cin, cout), np.float32)
    for exact in (True, False):
        x = rng.randint(-4, 5, (len(loc), cin)).astype(np.float64) if exact else rng.randn(len(loc), cin)
        g = rng.randint(-4, 5, (len(loc), cout)).astype(np.float64) if exact else rng.randn(len(loc), cout)
        x, g = x.astype(np.float32).astype(np.float64), g.astype(np.float32).astype(np.float64)
        want, a = dw64(x, g, rules, 27)
        _, ref = oracle.rule_conv_backward(x, w, rules, g)
        if exact:
            assert np.array_equal(ref.astype(np.float64), want)
        else:
            assert (np.abs(ref - want) <= gamma(int(counts.max()) + 1) * a).all()
    # one rule taken out moves the offset's result
    k = int(rules[5, 2])
    less, _ = dw64(x, g, np.delete(rules, 5, 0), 27)
    assert np.array_equal(less[np.arange(27) != k], want[np.arange(27) != k])
    assert np.allclose(want[k] - less[k], np.outer(x[rules[5, 0]], g[rules[5, 1]]), rtol=0, atol=1e-12)


def test_dw64_offsets_without_rules():
    loc, rules = _small_scene(2, 40, 12)          # sparse: some offsets have no rule
    counts = rules_per_offset(rules, 27)
    assert (counts == 0).any()
    rng = np.random.RandomState(3)
    x, g = rng.randint(-4, 5, (40, 20)).astype(np.float64), rng.randint(-4, 5, (40, 32)).astype(np.float64)
    want, a = dw64(x, g, rules, 27)
    assert (want[counts == 0] == 0).all() and (a[counts == 0] == 0).all()
    _, ref = oracle.rule_conv_backward(x, np.zeros((27, 20, 32), np.float32), rules, g)
    assert np.array_equal(ref.astype(np.float64), want)
    assert dw64(x, g, rules, 27, with_abs=False)[1] is None


def test_expected_forms_at_the_documented_boundaries():
    # run: ceil(n_blk K nz / 1024), at least 2; one chunk below 64
    f = expect_dw(F32, 64, 64, 64, 27, 188, False)
    assert (f["run"], f["chunk"], f["n_chunks"], f["gx"], f["gy"], f["gz"], f["G"], f["det"]) == (5, 5, 1, 38, 27, 1, 0, 0)
    assert expect_dw(F32, 64, 64, 64, 27, 41, False)["run"] == 2 and expect_dw(F32, 64, 64, 64, 1, 1, False)["run"] == 2
    # the chunked form: 607 blocks x 27 x nz 4 = 65556 >= 64 * 1024.  (The run length is rounded up, so the form is
    # taken from ceil(n_blk K nz / 1024) = 64 on, i.e. n_blk K nz > 63 * 1024: 598 blocks here, 2390 at 64 x 64.)
    f = expect_dw(F32, 256, 256, 256, 27, 607, False)
    assert (f["T"], f["nz"], f["run"], f["chunk"], f["n_chunks"], f["gx"], f["gz"]) == (64, 4, 64, 8, 8, 10, 32)
    assert expect_dw(F32, 256, 256, 256, 27, 598, False)["n_chunks"] == 8
    f = expect_dw(F32, 256, 256, 256, 27, 597, False)
    assert (f["run"], f["chunk"], f["n_chunks"], f["gx"], f["gz"]) == (63, 63, 1, 10, 4)
    f = expect_dw(BF16, 64, 64, 64, 27, 2428, False)
    assert (f["T"], f["nz"], f["run"], f["chunk"], f["n_chunks"], f["gx"], f["gz"]) == (4, 1, 64, 8, 8, 38, 8)
    assert expect_dw(BF16, 64, 64, 64, 27, 2390, False)["n_chunks"] == 8
    assert expect_dw(BF16, 64, 64, 64, 27, 2389, False)["run"] == 63
    # tiles: T, tiles per group 16, groups
    assert [expect_dw(F32, 32, 32, c, 27, 41, False)["T"] for c in (32, 64, 128, 256)] == [1, 2, 4, 8]
    assert expect_dw(F32, 128, 100, 256, 27, 41, False)["nz"] == 2 and expect_dw(F32, 256, 200, 128, 8, 41, True, LANE)["nz"] == 2
    assert expect_dw(BF16, 16, 9, 32, 27, 41, False)["T"] == 1 and expect_dw(BF16, 16, 9, 256, 27, 41, False)["T"] == 8
    # fixed order: G = min(runs of 64 blocks, 32, 64 MB / partial)
    assert [expect_dw(F32, 64, 64, 64, 27, nb, True, CALLER)["G"] for nb in (1, 64, 65, 2048, 2049, 5000)] == [1, 1, 2, 32, 32, 32]
    f = expect_dw(F32, 256, 256, 256, 27, 607, True, ASYNC)
    assert (f["G"], f["gx"], f["gy"], f["gz"], f["run"], f["n_chunks"], f["scratch"]) == (9, 9, 27, 4, 64, 1, ASYNC)
    assert expect_dw(F32, 256, 256, 256, 8, 5000, True, LANE)["G"] == 32       # 2 MB partials: not limited
    assert expect_dw(BF16, 256, 256, 256, 32, 5000, True, LANE)["G"] == 8      # [1, 1, 32]: 8 MB partials


def test_exactness_precondition():
    rules = np.zeros((2 ** 20 - 1, 3), np.int64)
    assert assert_exact_precondition(rules, 27) == 2 ** 20 - 1
    with pytest.raises(AssertionError):
        assert_exact_precondition(np.zeros((2 ** 20, 3), np.int64), 27)    # 16 * 2^20 = 2^24
    spread = np.zeros((2 ** 21, 3), np.int64)
    spread[:, 2] = np.arange(2 ** 21) % 27                                 # many rules, few per offset
    assert_exact_precondition(spread, 27)
