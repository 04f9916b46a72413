"""What the top-k selection tests share and a machine without a GPU can check (test_topk_forms_cpu.py): the defined order
in plain numpy, a model of the select's decisions on key bits, and cases built FROM key bits so that each states where the
k-th decision falls.  Imports neither torch nor the library.

ORDER.  Descending score, equal scores by the lower index: the stable argsort of -scores (oracle/detector_port.py:
nms_clamped, rpn_select).  Under it -0.0 == +0.0 (the index decides) and a NaN of either sign comes last, behind -inf.
reference_topk sorts by (is-NaN, -value compared as a float, index).

KEY.  csrc/topk.hip selects on a 32-bit key: the order-preserving image of the fp32 bits (sign set: ~bits, else
bits | 0x80000000), canonical for the two places where the order does not follow the bits -- every zero has +0.0's key
0x80000000 and every NaN has key 1.  -inf is 0x007fffff, +inf is 0xff800000; keys in between are the finite values, and
0x7fffffff (the raw image of -0.0) never occurs.  The radix select fixes bits 31..21, 20..10 and 9..0 (levels 1, 2, 3 with
2048, 2048 and 1024 bins); find_bin_from_top gives thread t the bins 2047 - 2t, 2046 - 2t (1023 - t at level 3).  Of level 1
the canonical key reaches bin 0 (NaN), 3 (-inf alone), 4 .. 2043 and 2044 (+inf alone).

A case is a dict: vals (the fp32 storage), n, elem_stride, group_stride, n_groups, example (int32 [n] or None), n_examples,
k, min_value (None or a float) and, for designed cases, `design` = the properties the builder aimed at (select_model
recomputes them from the key bits)."""
import math

import numpy as np

F32 = np.float32
TOPK_MAX = 4096
THREADS = 1024
LEVELS = ((21, 11), (10, 11), (0, 10))          # (shift, bits) of the three radix levels
KEY_NAN, KEY_ZERO, KEY_NEG_INF, KEY_POS_INF = 1, 0x80000000, 0x007FFFFF, 0xFF800000
SIZES = (1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 32769)
SIZE_ONCE = 70001
KS = (1, 127, 128, 129, 2048, 2049, 4095, 4096)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def from_bits(b):
    return np.ascontiguousarray(b, np.uint32).view(F32)


# --------------------------------------------------------------------------------------------------------- the order
def reference_topk(vals, k, rows=None, min_value=None):
    """vals: fp32 [n]; rows: the element indices of the segment (None: all).  -> (indices int64 [m], values fp32 [m],
    count) with m = min(k, elements); count = m, or with min_value the number of kept values > min_value"""
    vals = np.ascontiguousarray(vals, F32)
    rows = np.arange(vals.shape[0], dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    with np.errstate(invalid="ignore"):              # (signalling NaNs among the inputs)
        v = vals[rows].astype(np.float64)
    nan = np.isnan(v)
    order = np.lexsort((rows, np.where(nan, 0.0, -v), nan))
    idx = rows[order][:max(int(k), 0)]
    got = vals[idx]
    count = len(idx) if min_value is None else int((got > F32(min_value)).sum())
    return idx, got, count


def reference_sorted(vals, k, rows=None):
    """the same order through Python's sorted and a tuple key (independent of numpy's sorts)"""
    vals = [float(x) for x in np.ascontiguousarray(vals, F32)]
    rows = range(len(vals)) if rows is None else [int(r) for r in rows]
    return sorted(rows, key=lambda i: (True, 0.0, i) if math.isnan(vals[i]) else (False, -vals[i], i))[:max(int(k), 0)]


# ----------------------------------------------------------------------------------------------------------- key bits
def key_of(vals):
    """the canonical selection key of every value, uint32"""
    b = bits(vals)
    mag = b & np.uint32(0x7FFFFFFF)
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    key = np.where(mag == 0, np.uint32(KEY_ZERO), key)
    return np.where(mag > 0x7F800000, np.uint32(KEY_NAN), key).astype(np.uint32)


def raw_key_of(vals):
    """the image without the two canonical rules (what the order of the raw bits would be)"""
    b = bits(vals)
    return np.maximum(np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32), np.uint32(1))


def from_keys(keys):
    """fp32 values whose canonical keys are `keys` (key 1 -> a NaN; the builders assert the round trip)"""
    keys = np.ascontiguousarray(keys, np.uint32)
    b = np.where(keys & np.uint32(0x80000000), keys & np.uint32(0x7FFFFFFF), ~keys).astype(np.uint32)
    b = np.where(keys == KEY_NAN, np.uint32(0x7FC00000), b).astype(np.uint32)
    v = from_bits(b)
    assert np.array_equal(key_of(v), keys), "not a canonical key"
    return v


def make_key(b1, b2, b3):
    return (np.asarray(b1, np.uint64) << 21 | np.asarray(b2, np.uint64) << 10 | np.asarray(b3, np.uint64)).astype(np.uint32)


def fields(key):
    key = int(key)
    return key >> 21, (key >> 10) & 2047, key & 1023


def padded(k_eff):
    P = 128
    while P < k_eff:
        P <<= 1
    return P


def select_model(keys, k):
    """The decisions of the radix select on the keys of ONE segment's elements (in index order), from the bits alone.
    level: the first level after which the bin of the k-th key holds copies of it only (the later levels decide nothing).
    bins: the bin of the k-th key at each level.  per_level_want: `want` as each level receives it."""
    keys = np.ascontiguousarray(keys, np.uint32).astype(np.int64)
    n = keys.shape[0]
    k_eff = min(int(k), n)
    if k_eff == 0:
        return dict(k_eff=0)
    T = int(np.sort(keys)[::-1][k_eff - 1])
    n_eq, n_above = int((keys == T).sum()), int((keys > T).sum())
    level, wants, want = None, [], k_eff
    for lv, (shift, _) in enumerate(LEVELS, 1):
        wants.append(want)
        want = k_eff - int(((keys >> shift) > (T >> shift)).sum())       # the bins above T's, through this level
        if level is None and int(((keys >> shift) == (T >> shift)).sum()) == n_eq:
            level = lv
    need_eq = k_eff - n_above
    assert want == need_eq and 1 <= need_eq <= n_eq
    return dict(k_eff=k_eff, T=T, n_eq=n_eq, need_eq=need_eq, n_above=n_above, all_ties=n_eq == need_eq, level=level,
                bins=fields(T), per_level_want=tuple(wants), P=padded(k_eff),
                above_bins=len(set((keys[keys > T] >> 21).tolist())))


# -------------------------------------------------------------------------------------------------------------- cases
def case(name, vals, k, n=None, elem_stride=1, group_stride=0, n_groups=1, example=None, n_examples=1, min_value=None,
         design=None):
    vals = np.ascontiguousarray(vals, F32)
    n = vals.shape[0] if n is None else int(n)
    if example is not None:
        example = np.ascontiguousarray(example, np.int32)
        assert example.shape == (n,)
    assert vals.ndim == 1 and (n == 0 or (n_groups - 1) * group_stride + (n - 1) * elem_stride < vals.shape[0])
    return dict(name=name, vals=vals, n=n, elem_stride=int(elem_stride), group_stride=int(group_stride),
                n_groups=int(n_groups), example=example, n_examples=int(n_examples), k=int(k), min_value=min_value,
                design=design)


def segment_rows(c, b):
    """element indices of example b"""
    if c["example"] is None or c["n_examples"] == 1:
        return np.arange(c["n"], dtype=np.int64)
    return np.nonzero(c["example"] == b)[0].astype(np.int64)


def segment_values(c, g):
    """fp32 [n]: the values of group g by element index"""
    return c["vals"][g * c["group_stride"] + np.arange(c["n"], dtype=np.int64) * c["elem_stride"]]


def reference_case(c, values_of=None):
    """-> list over segments s = b * n_groups + g of (indices, values, count, elements).  values_of(g): the values to
    order by instead of the stored ones (the sigmoid form orders by the device's own sigmoid bits)"""
    out = []
    for b in range(c["n_examples"]):
        rows = segment_rows(c, b)
        for g in range(c["n_groups"]):
            v = segment_values(c, g) if values_of is None else values_of(g)
            idx, got, cnt = reference_topk(v, c["k"], rows, c["min_value"])
            out.append((idx, got, cnt, min(c["k"], len(rows))))
    return out


def segment_model(c, s=0):
    b, g = divmod(s, c["n_groups"])
    return select_model(key_of(segment_values(c, g)[segment_rows(c, b)]), c["k"])


# ---- radix levels: the k-th decision at a chosen level, in a chosen bin
MID1 = 1500                                         # a level-1 bin of ordinary positive values (about 0.004 .. 0.008)
LEVEL_T = {                                         # (level, where) -> the k-th key
    (1, "nan"): KEY_NAN, (1, "neg_inf"): KEY_NEG_INF, (1, "pos_inf"): KEY_POS_INF,
    (1, "bin1023"): int(make_key(1023, 77, 5)), (1, "bin1024"): int(make_key(1024, 77, 5)),
    (2, "bin0"): int(make_key(MID1, 0, 513)), (2, "bin2047"): int(make_key(MID1, 2047, 513)),
    (2, "bin1023"): int(make_key(MID1, 1023, 513)),
    (3, "bin0"): int(make_key(MID1, 900, 0)), (3, "bin1023"): int(make_key(MID1, 900, 1023)),
    (3, "bin511"): int(make_key(MID1, 900, 511)),
}


def _other_keys(rng, T, count, above, share):
    """`count` distinct keys above / below T that share `share` leading levels with it and differ at the next one (all
    that fit, then keys of other level-1 bins)"""
    f = list(fields(T))
    out = set()
    if share > 0 and T not in (KEY_NAN, KEY_NEG_INF, KEY_POS_INF):
        width = (2048, 2048, 1024)[share]
        cand = range(f[share] + 1, width) if above else range(0, f[share])
        cand = list(cand)
        rng.shuffle(cand)
        for x in cand[:max(count // 2, min(count, 1))]:
            g = f[:share] + [x] + [int(rng.randint(0, 2048)) for _ in range(2 - share)]
            g[2] &= 1023
            out.add(int(make_key(*g)))
    lo, hi = (f[0] + 1, 2043) if above else (4, f[0] - 1)
    lo, hi = max(lo, 4), min(hi, 2043)
    while len(out) < count:
        assert lo <= hi, "no room on that side of T"
        key = int(make_key(rng.randint(lo, hi + 1), rng.randint(0, 2048), rng.randint(0, 1024)))
        if key != 0x7FFFFFFF:
            out.add(key)
    return sorted(out)


def level_case(level, where, n=2381, n_above=300, n_eq=1, need_eq=1, above="spread", seed=0):
    """the k-th key is LEVEL_T[level, where]; other keys share level - 1 leading levels with it, so that the decision
    falls at `level`.  above: 'spread' (many level-1 bins), 'one_bin' (every key above T in ONE level-1 bin) or
    'one_per_bin' (each in a level-1 bin of its own)"""
    rng = np.random.RandomState(1000 * level + seed + sum(map(ord, where)))
    T = LEVEL_T[level, where]
    if T == KEY_POS_INF:
        n_above = 0
    n_below = n - n_above - n_eq
    if T == KEY_NAN:
        n_below = 0
        n_above = n - n_eq
    t1 = fields(T)[0]
    if above == "one_bin" and n_above:
        b1 = t1 + 1 if T != KEY_NAN else 1800
        low = rng.permutation(1 << 21)[:n_above]
        up = [int(b1 << 21 | int(x)) for x in low]
    elif above == "one_per_bin" and n_above:
        lo = max(t1 + 1, 4)
        assert n_above <= 2043 - lo + 1
        b1s = lo + rng.permutation(2043 - lo + 1)[:n_above]
        up = [int(make_key(b, rng.randint(0, 2048), rng.randint(0, 1024))) for b in b1s]
    else:
        up = _other_keys(rng, T, n_above, True, level - 1)
    # (below -inf there are only NaNs)
    down = [KEY_NAN] * n_below if T == KEY_NEG_INF else _other_keys(rng, T, n_below, False, level - 1)
    keys = np.array(up + [T] * n_eq + down, np.uint32)
    keys = keys[rng.permutation(n)]
    vals = from_keys(keys)
    at = np.nonzero(keys == KEY_NAN)[0]            # NaNs of both signs and several payloads: all one key
    b = bits(vals).copy()
    b[at] = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32)[np.arange(len(at)) % 4]
    vals = from_bits(b)
    assert np.array_equal(key_of(vals), keys)
    k = n_above + need_eq
    return case(f"level{level}_{where}_{above}_eq{n_eq}_need{need_eq}", vals, k,
                design=dict(level=level, T=T, n_eq=n_eq, need_eq=need_eq, all_ties=n_eq == need_eq, P=padded(k),
                            above=above))


def level_cases():
    out = []
    for (level, where) in LEVEL_T:
        out.append(level_case(level, where))
        out.append(level_case(level, where, n_eq=7, need_eq=3, seed=1))
    for above in ("one_bin", "one_per_bin"):
        out.append(level_case(2, "bin1023", above=above, seed=2))
        out.append(level_case(1, "bin1024", above=above, n_eq=5, need_eq=5, seed=3))
    return out


# ---- run-length histogram: lane patterns of hist_add (wbin / wcnt), at lengths that are no multiple of 64
def _pattern_bins(name, i, n):
    if name == "one_bin":
        return np.full_like(i, 40)
    if name == "alternate":
        return np.where(i % 2 == 0, 40, 900)
    if name == "new_bin_per_wave":
        return 10 + (i // 64) % 300
    if name == "distinct64":
        return 100 + (i % 64) * 3
    if name == "ramp_up":
        return i * 1000 // n
    if name == "ramp_down":
        return (n - 1 - i) * 1000 // n
    if name == "run_across_pass":                  # one bin from 40 elements before a pass edge to 40 behind it
        near = np.minimum(i % 1024, 1024 - i % 1024) if n < 16384 else np.abs(i - 16384)
        return np.where((near <= 40) & (i >= 512), 77, 200 + i % 7)
    raise KeyError(name)


PATTERNS = ("one_bin", "alternate", "new_bin_per_wave", "distinct64", "ramp_up", "ramp_down", "run_across_pass")


def pattern_case(name, level, stretch, n, k):
    """the lane pattern in the bins of `level` (higher fields fixed, lower ones hashed from the index).  stretch 4
    repeats each pattern element four times: with key scratch a thread holds four consecutive elements, so a wave's
    64 lanes see the pattern as the form without scratch sees it at stretch 1"""
    i = np.arange(n, dtype=np.int64)
    p = _pattern_bins(name, i // stretch, (n + stretch - 1) // stretch)
    h = (i * 2654435761) & 0xFFFFFFFF
    if level == 1:
        f = (1030 + p, (h >> 5) & 2047, (h >> 17) & 1023)
    elif level == 2:
        f = (np.full_like(i, MID1), p + 1, (h >> 7) & 1023)
    else:
        f = (np.full_like(i, MID1), np.full_like(i, 900), p % 1024)
    return case(f"hist_{name}_level{level}_x{stretch}_n{n}_k{k}", from_keys(make_key(*f)), k,
                design=dict(level=None, pattern=name))


def pattern_cases():
    out = []
    for name in PATTERNS:
        n = 17421 if name == "run_across_pass" else 2381
        for level in (1, 2, 3):
            for stretch in (1, 4):
                for k in (1, min(n // 3, 2000), min(n - 1, TOPK_MAX)):
                    if level == 1 or k != 1:
                        out.append(pattern_case(name, level, stretch, n, k))
    out.append(pattern_case("run_across_pass", 1, 1, 2381, 700))
    return out


# ---- ties at the threshold
def tie_case(name, n, at, need_eq, n_above, seed=0):
    """the threshold value 0.5 at the indices `at`; n_above distinct values above it elsewhere, the rest below"""
    rng = np.random.RandomState(seed + n)
    at = np.asarray(sorted(at), np.int64)
    assert len(set(at.tolist())) == len(at) and at.min() >= 0 and at.max() < n and 1 <= need_eq <= len(at)
    rest = np.setdiff1d(np.arange(n), at)
    n_above = min(n_above, len(rest))
    pool = rng.permutation(1 << 20)[:len(rest)].astype(np.int64)
    keys = np.empty(n, np.uint32)
    T = int(key_of(np.array([0.5], F32))[0])
    up = rng.permutation(len(rest))
    keys[rest[up[:n_above]]] = T + 1 + pool[:n_above]
    keys[rest[up[n_above:]]] = T - 1 - pool[n_above:]
    keys[at] = T
    k = n_above + need_eq
    return case(f"ties_{name}", from_keys(keys), k,
                design=dict(level=None, T=T, n_eq=len(at), need_eq=need_eq, all_ties=len(at) == need_eq, P=padded(k)))


def tie_cases():
    n = 5003                                        # per = ceil(5003 / 1024) = 5: thread t owns [5 t, 5 t + 5)
    per = (n + THREADS - 1) // THREADS
    last = ((n - 1) // per) * per                   # first index of the last non-empty range (5000: three elements)
    spread = list(range(7, n, 251))
    out = [
        tie_case("all_taken", n, spread, len(spread), 100),
        tie_case("need_1", n, spread, 1, 100),
        tie_case("need_all_but_one", n, spread, len(spread) - 1, 100),
        tie_case("need_half", n, spread, len(spread) // 2, 3000),
        tie_case("last_range_only_need_1", n, range(last, n), 1, 50),
        tie_case("last_range_only_need_2", n, range(last, n), 2, 50),
        tie_case("straddle_range_edge", n, range(per * 300 - 2, per * 300 + 3), 3, 50),
        tie_case("straddle_wave_edge", n, range(per * 64 - 3, per * 64 + 4), 4, 50),          # threads 63 | 64
        tie_case("straddle_wave_edge_need_1_behind", n, [3] + list(range(per * 64, per * 64 + 4)), 2, 50),
        tie_case("first_and_last_element", n, [0, n - 1], 1, 200),
        tie_case("long_run_need_1000", n, range(1000, 4000), 1000, 500),
        tie_case("small_n_per_1", 700, range(100, 140), 17, 30),
        tie_case("n_1025_per_2", 1025, [1022, 1023, 1024], 2, 10),
    ]
    for n_all, k in ((5003, 1), (5003, 129), (5003, 4096), (70, 69), (70, 70), (70, 128), (1, 1), (16385, 2049)):
        c = tie_case(f"everything_equal_n{n_all}_k{k}", n_all, range(n_all), min(k, n_all), 0)
        c["k"] = k
        c["design"]["P"] = padded(min(k, n_all))
        out.append(c)
    return out


# ---- value families
def _nan(sign, payload):
    return from_bits(np.array([(0x80000000 if sign else 0) | 0x7F800000 | payload], np.uint32))[0]


def value_cases():
    rng = np.random.RandomState(5)
    n = 301
    out = []
    neg = -np.abs(rng.randn(n)).astype(F32) - F32(0.25)
    neg[::9] = F32(-2.5)
    out += [case(f"negatives_k{k}", neg, k) for k in (1, 50, n, n + 9)]
    # zeros of both signs in an order that their bits would sort differently, among small values of both signs
    z = np.zeros(n, F32)
    z[0::2] = F32(-0.0)
    z[5::7] = F32(1e-30)
    z[6::11] = F32(-1e-30)
    z[3::13] = from_bits(np.array([1], np.uint32))[0]                   # the smallest denormal, above every zero
    z[4::17] = from_bits(np.array([0x80000001], np.uint32))[0]          # its negative, below every zero
    n_pos = int((z > 0).sum())
    n_zero = int((z == 0).sum())
    out += [case(f"zeros_k{k}", z, k) for k in (1, n_pos, n_pos + 1, n_pos + 2, n_pos + n_zero // 2, n_pos + n_zero - 1,
                                                n_pos + n_zero, n_pos + n_zero + 1, n)]
    out.append(case("zeros_minus_first", np.array([-0.0, 0.0, -0.0, 0.0, 0.0, -0.0], F32), 3))
    out.append(case("zeros_only_min_value", np.array([0.0, -0.0] * 40, F32), 33, min_value=-0.0))
    out.append(case("zeros_below_min_value", np.concatenate([z, [F32(1.0)]]), n, min_value=-1e-31))
    inf = rng.randn(n).astype(F32)
    inf[::6] = F32(np.inf)
    inf[1::6] = F32(-np.inf)
    n_inf = int(np.isposinf(inf).sum())
    out += [case(f"inf_k{k}", inf, k) for k in (1, n_inf - 1, n_inf, n_inf + 1, n - n_inf, n - n_inf + 1, n)]
    out.append(case("inf_min_value_is_inf", inf, n, min_value=float("inf")))
    out.append(case("inf_min_value_is_minus_inf", inf, n, min_value=float("-inf")))
    den = from_bits(rng.randint(1, 0x00800000, n).astype(np.uint32) | (rng.randint(0, 2, n).astype(np.uint32) << 31))
    den[::10] = F32(0.0)
    den[1::10] = F32(-0.0)
    den[2::10] = den[2]
    out += [case(f"denormals_k{k}", den, k) for k in (1, 100, 150, 200, n)]
    out.append(case("denormals_min_value_0", den, n, min_value=0.0))
    # NaN of both signs: at the top of the raw bit order, at the threshold, everywhere
    nan = rng.randn(n).astype(F32)
    nan[::8] = _nan(0, 0x400000)
    nan[3::8] = _nan(1, 0x400000)
    nan[5::16] = _nan(0, 1)
    nan[9::16] = _nan(1, 0x7FFFFF)
    nan[2] = F32(np.inf)
    nan[4] = F32(-np.inf)
    n_num = int((~np.isnan(nan)).sum())
    out += [case(f"nan_k{k}", nan, k) for k in (1, 5, n_num - 1, n_num, n_num + 1, n_num + 2, n - 1, n, n + 5)]
    out += [case(f"nan_min_value_{str(mv).replace('.', 'p').replace('-', 'm')}_k{k}", nan, k, min_value=mv)
            for mv in (0.0, -3.0e38, float("-inf")) for k in (n_num // 2, n_num + 2, n)]
    out.append(case("nan_everywhere", from_bits(np.where(np.arange(n) % 2 == 0, 0x7FC00000, 0xFFC00000).astype(np.uint32)
                                                 + (np.arange(n) % 5).astype(np.uint32)), 128))
    out.append(case("nan_everywhere_min_value", from_bits(np.full(n, 0x7FC00000, np.uint32)), n, min_value=0.0))
    out.append(case("nan_first_numbers_last", np.concatenate([np.full(200, np.nan, F32), rng.randn(101).astype(F32)]), 150))
    return out


NAN_MIN_VALUE_REPEAT = "nan_min_value_0p0_k301"


# ---- sizes
def _size_values(n, seed):
    """random values from few levels, so that the threshold falls into a run of equal values, with zeros of both signs"""
    rng = np.random.RandomState(seed)
    v = (rng.randint(-40, 40, n) * 0.125).astype(F32) if n < 1000 else np.round(rng.randn(n) * 64).astype(F32) / F32(64)
    v[rng.rand(n) < 0.05] = F32(-0.0)
    return v


def size_cases():
    out = []
    for n in SIZES:
        seen = set()                                 # each n with the k that change P, k_eff or "k > n"
        for k in sorted(set(KS + ((n,) if n <= TOPK_MAX else ()))):
            sig = (padded(min(k, n)), min(k, n), k > n)
            if sig not in seen:
                seen.add(sig)
                out.append(case(f"size_n{n}_k{k}", _size_values(n, n), k, design=dict(level=None, P=sig[0])))
    for k in (256, 257, 512, 513, 1024, 1025):       # the padded sizes the listed k leave out (512, 1024) and their edges
        out.append(case(f"size_n4097_k{k}", _size_values(4097, 4097), k, design=dict(level=None, P=padded(k))))
    out.append(case(f"size_n{SIZE_ONCE}_k1000", _size_values(SIZE_ONCE, 7), 1000, design=dict(level=None, P=1024)))
    return out


# ---- layouts
def layout_cases():
    rng = np.random.RandomState(21)
    out = []

    def vals(m):
        v = (rng.randint(-30, 30, m) * 0.25).astype(F32)
        v[rng.rand(m) < 0.03] = F32(np.nan)
        v[rng.rand(m) < 0.05] = F32(-0.0)
        return v

    def examples(n, B, kind):
        if B == 1:
            return None
        if kind == "interleaved":
            return (np.arange(n) % B).astype(np.int32)
        ex = np.sort(rng.randint(0, B, n)).astype(np.int32)
        if kind == "tail":
            ex[-7:] = 0                              # not contiguous per example
        if kind == "none_first":                     # example 0 has no element
            ex[:] = 1
        if kind == "few_last":                       # the last example has 5 elements, fewer than k
            ex[:] = 0
            ex[[3, 500, 501, 900, n - 1]] = B - 1
        if kind == "few_and_none":                   # example 0 has 5 elements, example 1 none
            ex[:] = 2
            ex[[0, 64, 1023, 1024, n - 1]] = 0
        return ex

    n = 1301
    for B in (1, 2, 3):
        for kind in {1: ("none",), 2: ("interleaved", "tail", "none_first", "few_last"),
                     3: ("interleaved", "tail", "few_and_none")}[B]:
            for k in (40, 700):
                ex = examples(n, B, kind)
                tag = f"B{B}_{kind}_k{k}"
                out.append(case(f"layout_flat_{tag}", vals(n), k, example=ex, n_examples=B))
                for G in (1, 3):
                    out.append(case(f"layout_columns_G{G}_{tag}", vals(n * G), k, n=n, elem_stride=G, group_stride=1,
                                    n_groups=G, example=ex, n_examples=B))
                K, nseg = n, 4
                out.append(case(f"layout_rows_{tag}", vals(K * nseg), k, n=K, elem_stride=1, group_stride=K, n_groups=nseg,
                                example=ex, n_examples=B, min_value=0.0 if k == 40 else None))
    # the box head's layout: columns 1 .. nc - 1 of a [K, nc] matrix, the storage starting at column 1
    K, nc = 997, 4
    out.append(case("layout_box_head_columns", vals(K * nc)[1:], K, n=K, elem_stride=nc, group_stride=1, n_groups=nc - 1,
                    min_value=0.05))
    return out


def all_cases():
    return level_cases() + pattern_cases() + tie_cases() + value_cases() + size_cases() + layout_cases()


_CACHE = {}


def cases_by_name():
    """every case once per process (the references of the GPU tests are computed from these and left unchanged)"""
    if not _CACHE:
        for c in all_cases():
            assert c["name"] not in _CACHE, c["name"]
            c["vals"].setflags(write=False)
            _CACHE[c["name"]] = c
    return _CACHE


# ---- sigmoid form: logits whose sigmoid saturates to 1.0, underflows to 0.0 or is denormal
def sigmoid_logits(family, n=1500, seed=3):
    rng = np.random.RandomState(seed)
    if family == "ordinary":
        x = (rng.randn(n) * 4).astype(F32)
        x[rng.rand(n) < 0.3] = F32(0.37)
    elif family == "saturated":                    # exactly 1.0 above about 16.64 (exp(-x) < 2^-24), exactly 0.0 below
                                                   # about -88.73 (exp(-x) overflows to inf)
        x = (rng.randn(n) * 4).astype(F32)
        x[0::5] = F32(40.0)
        x[1::5] = (17.0 + rng.rand(len(x[1::5])) * 5).astype(F32)
        x[2::5] = F32(-110.0)
        x[3::7] = F32(-200.0)
        x[4::11] = F32(np.inf)
        x[5::13] = F32(-np.inf)
        x[6::17] = F32(np.nan)
    elif family == "denormal":                     # 1 / (1 + exp(-x)) below 2^-126 and above 0: x in about
        x = (-87.3 - rng.rand(n) * 1.5).astype(F32)   # (-88.73, -87.34); both edges are inside the sampled interval
        x[::9] = F32(-88.0)
    else:
        raise KeyError(family)
    return x


SIGMOID_FAMILIES = ("ordinary", "saturated", "denormal")


# ---- well-separated boxes for d3d_rotate_nms_3d: nothing is suppressed, the keep list is the selection
def separated_boxes(n):
    i = np.arange(n)
    b = np.zeros((n, 7), F32)
    b[:, 0] = (i % 100) * 4.0
    b[:, 1] = (i // 100) * 4.0
    b[:, 3:6] = 1.0
    b[:, 6] = (i % 7) * 0.3
    return b


def nms_scores(kind, n, seed=2):
    rng = np.random.RandomState(seed)
    s = rng.rand(n).astype(F32)
    if kind == "tied":
        s = (rng.randint(0, 12, n) / 16.0).astype(F32)
    elif kind == "zeros":
        s = np.where(rng.rand(n) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
        s[::9] = F32(0.5)
        s[4::9] = F32(-0.5)
    elif kind == "nan":
        s[::4] = F32(np.nan)
        s[1::8] = from_bits(np.array([0xFFC00000], np.uint32))[0]
        s[2::16] = F32(0.25)
    return s


NMS_SCORE_KINDS = ("random", "tied", "zeros", "nan")
