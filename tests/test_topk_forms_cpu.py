"""Keeps tests/topk_forms.py honest without a GPU: reference_topk against an independent formulation and against the
oracle port's stable argsort, the order of zeros and NaNs, and for every designed case the property it was built for,
recomputed from the key bits (test_topk_forms_gpu.py runs the kernel on the same objects)."""
import numpy as np
import pytest

from tests import topk_forms as F

CASES = F.cases_by_name()


def test_reference_equals_sorted_with_a_tuple_key_on_every_case():
    checked = 0
    for c in CASES.values():
        if c["n"] > 20000:
            continue
        for b in range(c["n_examples"]):
            rows = F.segment_rows(c, b)
            for g in range(c["n_groups"]):
                v = F.segment_values(c, g)
                idx, got, cnt = F.reference_topk(v, c["k"], rows, c["min_value"])
                assert idx.tolist() == F.reference_sorted(v, c["k"], rows), c["name"]
                assert np.array_equal(F.bits(got), F.bits(v[idx])) and len(idx) == min(c["k"], len(rows))
                if c["min_value"] is None:
                    assert cnt == len(idx)
                else:       # the kept values above the threshold are a prefix of the list: NaN is last and never above
                    above = [float(x) > float(np.float32(c["min_value"])) for x in got]
                    assert cnt == sum(above) and all(above[:cnt]) and not any(above[cnt:]), c["name"]
                checked += 1
    assert checked > 300


def test_reference_equals_the_oracle_ports_stable_argsort_on_finite_data():
    """oracle/detector_port.py (nms_clamped, rpn_select): np.argsort(-scores as fp64, kind='stable')[:k]"""
    n_cases = 0
    for c in CASES.values():
        for g in range(c["n_groups"]):
            v = F.segment_values(c, g)
            if c["n"] == 0 or not np.isfinite(v).all():
                continue
            want = np.argsort(-v.astype(np.float64), kind="stable")[:c["k"]]
            assert np.array_equal(F.reference_topk(v, c["k"])[0], want), c["name"]
            n_cases += 1
    assert n_cases > 200
    # ... and on the non-finite example of the defined order: inf, numbers, both zeros by index, -inf, NaN
    v = np.array([-0.0, 0.0, np.nan, 1.0, -np.inf, np.inf], np.float32)
    assert np.argsort(-v.astype(np.float64), kind="stable").tolist() == [5, 3, 0, 1, 4, 2]
    assert F.reference_topk(v, 6)[0].tolist() == [5, 3, 0, 1, 4, 2]


def test_reference_orders_zeros_by_index_and_puts_nan_last():
    v = np.array([-0.0, 0.0, -0.0, 0.0, 0.0, -0.0], np.float32)
    idx, got, cnt = F.reference_topk(v, 4)
    assert idx.tolist() == [0, 1, 2, 3] and F.bits(got).tolist() == [0x80000000, 0, 0x80000000, 0] and cnt == 4
    assert np.argsort(-F.raw_key_of(v).astype(np.int64), kind="stable")[:4].tolist() == [1, 3, 4, 0]   # the raw bits differ
    nan_pos, nan_neg = F.from_bits(np.array([0x7FC00000, 0xFFC00000], np.uint32))
    v = np.array([nan_pos, 1.0, np.inf, nan_neg, -np.inf, nan_pos], np.float32)
    assert F.reference_topk(v, 6)[0].tolist() == [2, 1, 4, 0, 3, 5]
    assert F.reference_topk(v, 6, min_value=float("-inf"))[2] == 2 and F.reference_topk(v, 6, min_value=2.0)[2] == 1
    assert F.reference_topk(v, 2, rows=[0, 3, 4, 5])[0].tolist() == [4, 0]
    assert np.argmax(F.raw_key_of(v)) == 0                                     # a sign-clear NaN above +inf in raw bits
    assert F.key_of(v).tolist() == [1, 0xBF800000, 0xFF800000, 1, 0x007FFFFF, 1]
    assert F.key_of(np.array([0.0, -0.0], np.float32)).tolist() == [0x80000000, 0x80000000]


def test_the_canonical_key_orders_like_the_reference():
    """sorting by (key descending, index ascending) is the defined order: on all 2^16 bit patterns with a zero low half and
    on random patterns"""
    rng = np.random.RandomState(0)
    pats = np.concatenate([np.arange(1 << 16, dtype=np.uint32) << 16, rng.randint(0, 1 << 32, 50000, dtype=np.uint64).astype(np.uint32),
                           np.array([0, 0x80000000, 1, 0x80000001, 0x7F800000, 0xFF800000, 0x7F800001, 0xFFFFFFFF], np.uint32)])
    pats = pats[rng.permutation(len(pats))]
    v = F.from_bits(pats)
    key = F.key_of(v).astype(np.int64)
    by_key = np.lexsort((np.arange(len(v)), -key))
    assert np.array_equal(by_key, F.reference_topk(v, len(v))[0])
    finite_or_inf = ~np.isnan(v)
    assert key[finite_or_inf].min() >= F.KEY_NEG_INF and key[~finite_or_inf].max() == 1 and (key != 0).all()
    assert not (key == 0x7FFFFFFF).any()


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["design"] and c["design"].get("level")])
def test_level_cases_decide_where_they_say(name):
    c = CASES[name]
    d, m = c["design"], F.segment_model(c)
    assert m["level"] == d["level"] and m["T"] == d["T"], (m, d)
    assert (m["n_eq"], m["need_eq"], m["all_ties"], m["P"]) == (d["n_eq"], d["need_eq"], d["all_ties"], d["P"])
    if d["above"] == "one_bin":
        assert m["above_bins"] == 1 and m["n_above"] >= 300
    if d["above"] == "one_per_bin":
        assert m["above_bins"] == m["n_above"] >= 300


def test_level_cases_cover_the_bins_and_threads():
    """the k-th key in the top reachable bin, the bottom one and bin 1023 / 511 of every level: thread 0, thread 1023 and
    thread 512 (the first lane of wave 8) of find_bin_from_top"""
    seen = {(c["design"]["level"], F.fields(c["design"]["T"])[c["design"]["level"] - 1])
            for c in CASES.values() if c["design"] and c["design"].get("level")}
    assert {(1, 0), (1, 3), (1, 2044), (1, 1023), (1, 1024)} <= seen
    assert {(2, 0), (2, 2047), (2, 1023), (3, 0), (3, 1023), (3, 511)} <= seen
    # bins 1, 2 and 2045 .. 2047 of level 1 hold no canonical key
    for b1 in (1, 2, 2045, 2046, 2047):
        with pytest.raises(AssertionError):
            F.from_keys(F.make_key([b1], [5], [5]))


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("ties_")])
def test_tie_cases_take_the_branch_they_say(name):
    c = CASES[name]
    d, m = c["design"], F.segment_model(c)
    assert (m["T"], m["n_eq"], m["need_eq"], m["all_ties"], m["P"]) == (d["T"], d["n_eq"], d["need_eq"], d["all_ties"], d["P"])


def test_tie_cases_cover_both_branches_and_the_range_edges():
    ties = {n: F.segment_model(c) for n, c in CASES.items() if n.startswith("ties_")}
    assert any(m["all_ties"] and m["n_eq"] > 1 for m in ties.values())
    assert any(not m["all_ties"] and m["need_eq"] == 1 for m in ties.values())
    assert any(not m["all_ties"] and m["need_eq"] == m["n_eq"] - 1 > 1 for m in ties.values())
    n, per = 5003, 5
    at = lambda name: np.nonzero(F.key_of(CASES[name]["vals"]) == ties[name]["T"])[0]
    assert (at("ties_last_range_only_need_1") // per == (n - 1) // per).all() and len(at("ties_last_range_only_need_1")) == 3
    assert len(set((at("ties_straddle_range_edge") // per).tolist())) == 2
    assert set((at("ties_straddle_wave_edge") // per // 64).tolist()) == {0, 1}
    assert ties["ties_everything_equal_n5003_k129"]["n_eq"] == 5003 and ties["ties_everything_equal_n70_k128"]["k_eff"] == 70


def test_pattern_cases_hold_the_lane_patterns():
    for name in F.PATTERNS:
        c = CASES[f"hist_{name}_level1_x1_n{17421 if name == 'run_across_pass' else 2381}_k1"]
        assert c["n"] % 64 != 0
        b = (F.key_of(c["vals"]) >> 21).astype(np.int64)
        waves = [b[i:i + 64] for i in range(0, c["n"] - 63, 64)]
        per_wave = [len(set(w.tolist())) for w in waves]
        if name == "one_bin":
            assert set(per_wave) == {1} and len(set(b.tolist())) == 1
        if name == "alternate":
            assert set(per_wave) == {2} and (b[0::2] == 1070).all() and (b[1::2] == 1930).all()
        if name == "new_bin_per_wave":
            assert set(per_wave) == {1} and all(waves[i][0] != waves[i + 1][0] for i in range(len(waves) - 1))
        if name == "distinct64":
            assert set(per_wave) == {64}
        if name == "ramp_up":
            assert (np.diff(b) >= 0).all() and b[-1] - b[0] > 900
        if name == "ramp_down":
            assert (np.diff(b) <= 0).all() and b[0] - b[-1] > 900
        if name == "run_across_pass":
            run = b[16384 - 40:16384 + 41]
            assert len(set(run.tolist())) == 1 and b[16384 - 41] != run[0] and b[16384 + 41] != run[0]
    b = (F.key_of(CASES["hist_run_across_pass_level1_x1_n2381_k700"]["vals"]) >> 21).astype(np.int64)
    assert len(set(b[1024 - 40:1024 + 41].tolist())) == 1 and len(set(b[2048 - 40:2048 + 41].tolist())) == 1
    # stretch 4: the lanes of a wave that holds four consecutive elements per thread see the stretch-1 pattern
    c1, c4 = CASES["hist_distinct64_level2_x1_n2381_k793"], CASES["hist_distinct64_level2_x4_n2381_k793"]
    f = lambda c: ((F.key_of(c["vals"]) >> 10) & 2047).astype(np.int64)
    assert np.array_equal(f(c4)[0::4], f(c1)[:len(f(c4)[0::4])])


def test_size_cases_cover_every_n_and_every_padded_size():
    sizes = [c for n, c in CASES.items() if n.startswith("size_")]
    assert {c["n"] for c in sizes} == set(F.SIZES) | {F.SIZE_ONCE}
    assert sum(c["n"] == F.SIZE_ONCE for c in sizes) == 1
    assert {c["k"] for c in sizes} >= set(F.KS)
    assert any(c["k"] > c["n"] for c in sizes)
    for c in sizes:
        assert F.segment_model(c)["P"] == c["design"]["P"]
    assert {c["design"]["P"] for c in sizes} == {128, 256, 512, 1024, 2048, 4096}
    for n in F.SIZES:
        if n >= 4096:
            assert {c["k"] for c in sizes if c["n"] == n} >= set(F.KS)
    assert 200 <= len(CASES) <= 600 and all(0 < c["k"] <= F.TOPK_MAX for c in CASES.values())


def test_value_and_layout_cases_hold_what_they_name():
    v = CASES["negatives_k1"]["vals"]
    assert (v < 0).all()
    z = CASES["zeros_k1"]["vals"]
    zb = F.bits(z)
    assert (zb == 0).sum() > 30 and (zb == 0x80000000).sum() > 30 and (zb == 1).any() and (zb == 0x80000001).any()
    first_zeros = F.reference_topk(z, int((z > 0).sum()) + 4)[0][-4:]
    assert len(set(zb[first_zeros].tolist())) == 2                       # the first zeros by index are of both signs
    d = CASES["denormals_k1"]["vals"]
    assert (np.abs(d) < np.float32(1.1754944e-38)).all() and (d > 0).any() and (d < 0).any()
    nan = CASES["nan_k1"]["vals"]
    nb = F.bits(nan)[np.isnan(nan)]
    assert (nb >> 31 == 0).any() and (nb >> 31 == 1).any() and np.isposinf(nan).any() and np.isneginf(nan).any()
    assert np.isnan(CASES["nan_everywhere"]["vals"]).all()
    assert CASES[F.NAN_MIN_VALUE_REPEAT]["min_value"] == 0.0 and CASES[F.NAN_MIN_VALUE_REPEAT]["k"] == 301
    lay = [c for n, c in CASES.items() if n.startswith("layout_")]
    assert {(c["elem_stride"], c["group_stride"], c["n_groups"]) for c in lay} >= {(1, 0, 1), (1, 1, 1), (3, 1, 3), (1, 1301, 4)}
    assert {c["n_examples"] for c in lay} == {1, 2, 3}
    counts = {tuple(len(F.segment_rows(c, b)) for b in range(c["n_examples"])) for c in lay if c["n_examples"] > 1}
    assert any(0 in t for t in counts) and any(5 in t for t in counts)
    tail = CASES["layout_flat_B2_tail_k40"]["example"]
    assert (np.diff(tail) < 0).any()                                     # not contiguous per example
    for fam in F.SIGMOID_FAMILIES:
        assert F.sigmoid_logits(fam).dtype == np.float32
    x = F.sigmoid_logits("denormal").astype(np.float64)
    s = 1.0 / (1.0 + np.exp(-x))
    assert (s < 2.0 ** -126).mean() > 0.9 and (s > 2.0 ** -149).all()
    b = F.separated_boxes(9001)
    assert len({(float(r[0]), float(r[1])) for r in b}) == 9001          # distinct centres 4 apart, extents 1
