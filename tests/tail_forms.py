"""References and designed cases of the detector tail (csrc/rpn_head.hip; csrc/box_tail.hip from k_post_scores down;
box_decode_one of d3d_internal.h).  Plain numpy, no GPU: tests/test_tail_forms_cpu.py keeps what is asserted about the
cases here honest, tests/test_tail_forms_gpu.py runs them.

Heads.  t = relu(x W1^T + b1), out = t W2^T + b2 in fp64 (head_reference); the launch form is restated from the kernel
(out_tiles, slices); the operand packing is written here from the kernel's comment (pack_f32 / pack_bf16), apart from
detector.RPNHead._packed and detector._pack_linear, which the tests compare with it.  Every head case has two data sets:
  exact     small integers, dense (no zero weight): every product and partial sum is an integer below 2^24, so fp32
            gives the fp64 result in any order and a dropped slice, a swapped half-wave, a wrong row or a lost bias moves
            an element by >= 1 (exact_headroom is asserted < 2^24 on the CPU)
  rounding  |x|, |w| uniform in [0.5, 2] with a random sign; the per-element bound of rounding_bound (standard
            gamma_n = n u / (1 - n u) forward error of an n-term fp32 sum, u = 2^-24)
Box decode: the cases only (the reference is oracle.box_decode).  Final selection: select_reference and friends."""
import numpy as np

U = 2.0 ** -24
RPN_MAX_SLICES = 8          # kRpnMaxSlices


# ----------------------------------------------------------------------------------------------------------------------
# launch forms of k_rpn_head / k_rpn_head_bf16, restated
def out_tiles(a):
    return (8 * a + 31) // 32


def slices(C, a):
    """S of stage 2: the W = C / 32 waves split (output tile, channel slice); a power of two, at most RPN_MAX_SLICES"""
    W, T = C // 32, out_tiles(a)
    S = 1
    while 2 * S * T <= W and 2 * S <= RPN_MAX_SLICES:
        S *= 2
    return S


def all_forms(C):
    """every (out_tiles, S) the kernel's loop can produce at C channels"""
    return sorted({(out_tiles(a), slices(C, a)) for a in range(1, C // 8 + 1)})


def all_ws():
    """every (W, S) pair over the three channel counts"""
    return sorted({(C // 32, s) for C in (128, 256, 512) for _, s in all_forms(C)})


# ----------------------------------------------------------------------------------------------------------------------
# bf16 as the kernels see it
def bf16_bits(x):
    """float32 -> bf16 bit pattern (uint16), round to nearest even: what `(__bf16)v` of st1(unsigned short *, float) and
    torch's .to(bfloat16) do; a NaN stays a (quiet) NaN"""
    x = np.ascontiguousarray(x, np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(x)
    r[nan] = ((b[nan] >> 16) | 0x40).astype(np.uint16)
    return r


def bf16_value(bits16):
    return (np.ascontiguousarray(bits16, np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    return bf16_value(bf16_bits(x))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 2: np.uint16}[a.dtype.itemsize])


# ----------------------------------------------------------------------------------------------------------------------
# operand packing, from the kernel's comment: packed[g][co][j] = W[co][G g + j], columns padded with zeros to whole tiles
def _pack(w, G):
    cout, c = w.shape
    cp = (cout + 31) // 32 * 32
    wp = np.zeros((cp, c), w.dtype)
    wp[:cout] = w
    g, co, j = np.ogrid[0:c // G, 0:cp, 0:G]
    return np.ascontiguousarray(wp[co, G * g + j])


def pack_f32(w):
    """[cout, C] fp32 -> [C/4, cout32, 4]"""
    return _pack(np.asarray(w, np.float32), 4)


def pack_bf16(w):
    """[cout, C] (values bf16 holds) -> [C/8, cout32, 8] bf16 bit patterns"""
    return _pack(bf16_bits(np.asarray(w, np.float32)), 8)


# ----------------------------------------------------------------------------------------------------------------------
# head data and references
def _signed(rng, shape, lo, hi):
    """integers of magnitude lo..hi with a random sign (never 0)"""
    return (rng.randint(lo, hi + 1, shape) * (2 * rng.randint(0, 2, shape) - 1)).astype(np.float32)


EXACT_RANGE = {128: (4, 4, 4), 256: (3, 3, 3), 512: (2, 3, 2)}   # C -> largest |x|, |w1|, |w2| (narrower as C grows)


def head_data(C, a, n, exact, seed, bf16=False):
    """-> dict x [n, C], w1 [C, C], b1 [C], w2 [8a, C] (objectness rows first), b2 [8a], all float32"""
    rng = np.random.RandomState(seed)
    if exact:
        mx, m1, m2 = EXACT_RANGE[C]
        d = dict(x=_signed(rng, (n, C), 1, mx), w1=_signed(rng, (C, C), 1, m1), b1=_signed(rng, (C,), 1, 8),
                 w2=_signed(rng, (8 * a, C), 1, m2), b2=_signed(rng, (8 * a,), 1, 8))
    else:
        def u(shape):
            return ((0.5 + 1.5 * rng.rand(*shape)) * (2 * rng.randint(0, 2, shape) - 1)).astype(np.float32)
        d = dict(x=u((n, C)), w1=u((C, C)), b1=u((C,)), w2=u((8 * a, C)), b2=u((8 * a,)))
        if bf16:
            d["x"], d["w1"], d["w2"] = bf16_round(d["x"]), bf16_round(d["w1"]), bf16_round(d["w2"])
    return d


def head_reference(d, relu_in=False, bf16=False, stages=3):
    """fp64: -> t [n, C] (bf16: rounded once, as st1 rounds it), out [n, 8a].  stages = 2: x is t."""
    x = d["x"].astype(np.float64)
    if relu_in:
        x = np.where(x < 0, 0.0, x)
    if stages & 1:
        t = x @ d["w1"].astype(np.float64).T + d["b1"].astype(np.float64)
        t = np.where(t < 0, 0.0, t)
        if bf16:
            t = bf16_round(t.astype(np.float32)).astype(np.float64)
    else:
        t = x
    out = t @ d["w2"].astype(np.float64).T + d["b2"].astype(np.float64) if stages & 2 else None
    return t, out


def _mags(d, relu_in, bf16, stages):
    x = np.abs(d["x"].astype(np.float64))
    if relu_in:
        x = np.where(d["x"] < 0, 0.0, x)
    m1 = x @ np.abs(d["w1"]).astype(np.float64).T + np.abs(d["b1"]).astype(np.float64) if stages & 1 else None
    t, _ = head_reference(d, relu_in, bf16, stages)
    m2 = np.abs(t) @ np.abs(d["w2"]).astype(np.float64).T + np.abs(d["b2"]).astype(np.float64) if stages & 2 else None
    return m1, np.abs(t), m2


def exact_headroom(d, relu_in=False, bf16=False, stages=3):
    """the largest sum_k |x_k| |w1_k| + |b1| and sum_k |t_k| |w2_k| + |b2| over the elements: below 2^24, every partial
    sum of either stage is an integer fp32 holds"""
    m1, _, m2 = _mags(d, relu_in, bf16, stages)
    return max(0.0 if m1 is None else m1.max(initial=0.0), 0.0 if m2 is None else m2.max(initial=0.0))


def gamma(n):
    return n * U / (1.0 - n * U)


def rounding_bound(d, C, a, relu_in=False, bf16=False, stages=3):
    """-> (bound on t [n, C] or None, bound on out [n, 8a] or None) per element, from the fp64 magnitudes:
    e1 = gamma_{C+1} (|x||W1|^T + |b1|); out: e1 |W2|^T + gamma_{C+S+1} (|t||W2|^T + |b2|); bf16 adds the rounding of t
    at 2^-8 of every |t||w2| term (the operands are bf16 values already)"""
    m1, t, m2 = _mags(d, relu_in, bf16, stages)
    e1 = gamma(C + 1) * m1 if stages & 1 else np.zeros_like(t)
    if not stages & 2:
        return e1, None
    w2 = np.abs(d["w2"]).astype(np.float64)
    bound = e1 @ w2.T + gamma(C + slices(C, a) + 1) * m2
    if bf16:
        bound = bound + 2.0 ** -8 * (t @ w2.T)
    return (e1 if stages & 1 else None), bound


def largest_products(d, relu_in=False, bf16=False, stages=3):
    """per element the largest |term| of its reference sum: (of t [n, C] or None, of out [n, 8a] or None)"""
    x = d["x"].astype(np.float64)
    if relu_in:
        x = np.where(x < 0, 0.0, x)
    def largest(rows, w):                                   # a row at a time: [cout, C] products
        w = np.abs(w.astype(np.float64))
        return np.stack([(np.abs(r)[None, :] * w).max(1) for r in rows]) if len(rows) else np.zeros((0, w.shape[0]))

    p1 = largest(x, d["w1"]) if stages & 1 else None
    t, _ = head_reference(d, relu_in, bf16, stages)
    p2 = largest(t, d["w2"]) if stages & 2 else None
    return p1, p2


# rows of every map; totals 1, 31, 32, 33, 65; 1, 2 and 6 maps; a boundary inside a 32-row block ([20, 13], [5, 0, 27 ..])
# and on a block edge ([32, 33], [.. 32]); an empty map first, in the middle, last; nothing at all
LAYOUTS = ([1], [31], [32], [33], [65], [20, 13], [32, 33], [0, 31], [17, 0, 15], [32, 0], [5, 0, 27, 1, 0, 32],
           [0], [0, 0, 0])
# a per channel count: every out_tiles / S named for W = 4, 8, 16; 8a % 32 != 0 (1, 3, 5, 13, 17, 33); the gate 8a == C
A_VALUES = {128: (1, 4, 5, 8, 12, 13, 16), 256: (1, 3, 8, 12, 17, 32), 512: (1, 5, 8, 12, 17, 33, 64)}
MLP_ROWS = (1, 31, 32, 33, 65)


def rpn_cases():
    """(C, a, rows): every a with one layout each (in rotation), every layout with one a"""
    out = []
    for C in (128, 256):
        live = [l for l in LAYOUTS if sum(l)]
        for i, a in enumerate(A_VALUES[C]):
            out.append((C, a, tuple(live[(3 * i + 4) % len(live)])))
        for l in LAYOUTS:
            out.append((C, 4 if C == 128 else 3, tuple(l)))
    return list(dict.fromkeys(out))


def mlp_cases():
    """(C, a, rows, relu_in): every a, every row count, both relu_in at every C"""
    out = []
    for C in (128, 256, 512):
        for i, a in enumerate(A_VALUES[C]):
            out.append((C, a, MLP_ROWS[i % len(MLP_ROWS)], i % 2))
        for i, n in enumerate(MLP_ROWS):
            out.append((C, A_VALUES[C][1], n, (i + 1) % 2))
    return sorted(set(out))


# ----------------------------------------------------------------------------------------------------------------------
# box decode cases
CLIPS = (float(np.float32(np.log(1000.0))), 10000.0)
WEIGHTS = ((1.0,) * 7, (10.0, 10.0, 10.0, 5.0, 5.0, 5.0, 1.0), (0.5, 2.0, 3.0, 0.25, 4.0, 0.5, 0.1))
PI32 = np.float32(3.14159265358979323846)


def decode_rows(n, seed):
    """ordinary rows: enc [n, 7] (no zero entry), anchors [n, 7] with positive sizes"""
    rng = np.random.RandomState(seed)
    enc = ((0.05 + rng.rand(n, 7)) * (2 * rng.randint(0, 2, (n, 7)) - 1) * 0.7).astype(np.float32)
    anchors = np.concatenate([rng.rand(n, 3) * 20 - 5, 0.2 + rng.rand(n, 3) * 3, (rng.rand(n, 1) - 0.5) * 3], 1)
    return enc, anchors.astype(np.float32)


SPECIALS = (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf))
# outputs that depend on: encoding slot k -> {k}; anchor slot: xa ya za -> the centre, wa la -> the diagonal (x, y) and
# their own size, ha -> z and its size, ra -> the yaw
_ENC_DEP = {k: (k,) for k in range(7)}
_ANC_DEP = {0: (0,), 1: (1,), 2: (2,), 3: (0, 1, 3), 4: (0, 1, 4), 5: (2, 5), 6: (6,)}


def nonfinite_cases(seed=11):
    """one special value at a time in every encoding slot and every anchor slot, each in a row of its own between
    ordinary rows.  -> enc, anchors, expect [n, 7] bool: the outputs that are not finite.  A +inf size delta is
    clamped to the clip and stays finite; a NaN one stays a NaN (torch.clamp)."""
    rows = [(which, k, v) for which in ("enc", "anc") for k in range(7) for v in SPECIALS]
    n = 2 * len(rows) + 1
    enc, anchors = decode_rows(n, seed)
    expect = np.zeros((n, 7), bool)
    for i, (which, k, v) in enumerate(rows):
        r = 2 * i + 1
        if which == "enc":
            enc[r, k] = v
            if not (3 <= k < 6 and v == np.inf):
                expect[r, list(_ENC_DEP[k])] = True
        else:
            anchors[r, k] = v
            expect[r, list(_ANC_DEP[k])] = True
    return enc, anchors, expect


def clip_cases(clip, weights=(1.0,) * 7):
    """size deltas that divide to exactly `clip`, one ulp below and one ulp above, in each size slot (size weights that
    are powers of two: the division is exact)"""
    c = np.float32(clip)
    vals = [np.nextafter(c, np.float32(0)), c, np.nextafter(c, np.float32(np.inf))]
    enc, anchors = decode_rows(9, 5)
    for i in range(9):
        enc[i, 3 + i // 3] = vals[i % 3] * np.float32(weights[3 + i // 3])
    return enc, anchors, np.array([v for _ in range(3) for v in vals], np.float32)


def yaw_cases():
    """t6 + ra exactly on odd multiples of fl32(pi) / 2 (the wrap's floor argument k + 0.5 + 0.5 sits on an integer up
    to rounding), given whole, as halves and from the anchor alone; |yaw| around 1e6"""
    odd = np.array([1, -1, 3, -3, 5, 7, -9, 101, -1001], np.float32)
    target = odd * (PI32 / np.float32(2))
    t6 = np.concatenate([target, np.zeros_like(target), target / 2, np.float32(1e6) + np.arange(9, dtype=np.float32) / 16,
                         -np.float32(1e6) - np.arange(9, dtype=np.float32) / 16])
    ra = np.concatenate([np.zeros_like(target), target, target / 2, np.linspace(-1.5, 1.5, 9).astype(np.float32),
                         np.linspace(1.5, -1.5, 9).astype(np.float32)])
    enc, anchors = decode_rows(t6.shape[0], 9)
    enc[:, 6], anchors[:, 6] = t6, ra
    return enc, anchors, np.tile(target, 3)


# ----------------------------------------------------------------------------------------------------------------------
# final selection
def f32_key(s):
    """the integer image k_post_select orders by: larger float <=> larger key; -0.0 is 0.0, every NaN is the top key"""
    s = np.ascontiguousarray(s, np.float32) + np.float32(0)
    b = s.view(np.uint32)
    k = np.where(b & 0x80000000, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(s)] = 0xffffffff
    return k


def candidates(keep, nk, n_max, prob_flat):
    """-> flat [N] int64 (0 for padding), s [N] float32 (-1 for padding): what d3d_post_gather writes"""
    nseg = nk.shape[0]
    t = np.arange(nseg * n_max)
    valid = (t % max(n_max, 1)) < nk[t // max(n_max, 1)] if t.size else np.zeros(0, bool)
    flat = np.where(valid, keep.reshape(-1)[:t.size], 0).astype(np.int64)
    s = np.where(valid, prob_flat[flat], np.float32(-1)).astype(np.float32)
    return flat, s


def dth_largest(s, D):
    """entry D - 1 of torch.sort(s, descending=True): NaN of either sign ranks above +inf"""
    nan = int(np.isnan(s).sum())
    if D - 1 < nan:
        return np.float32(np.nan)
    return np.sort(s[~np.isnan(s)], kind="stable")[::-1][D - 1 - nan]


def select_reference(keep, nk, n_max, prob_flat, boxes, nc, D):
    """inference.py:140-148 as PostProcessor.forward's tensor ending states it: the D-th largest candidate score
    (0 < D < N), clamp_min(0), s >= thresh (nothing when thresh is a NaN; -0.0 >= 0 stays), selection in t order.
    -> (boxes [m, 7], scores [m], labels [m] int64)"""
    flat, s = candidates(keep, nk, n_max, prob_flat)
    if 0 < D < s.shape[0]:
        th = dth_largest(s, D)
        th = th if np.isnan(th) else max(th, np.float32(0))
        with np.errstate(invalid="ignore"):
            sel = s >= th
    else:
        with np.errstate(invalid="ignore"):
            sel = s >= np.float32(0)
    f = flat[sel]
    return boxes[f], prob_flat[f], (f % nc).astype(np.int64)


def decided_pass(s, D):
    """the radix pass (1..4, most significant byte first) of k_post_select after which the D-th largest key is alone
    with its equals among the keys that still match its prefix"""
    k = f32_key(s).astype(np.uint64)
    kd = np.sort(k)[::-1][D - 1]
    for p in range(1, 5):
        sh = 32 - 8 * p
        if ((k >> sh) == (kd >> sh)).sum() == (k == kd).sum():
            return p
    return 4


def dth_bin(s, D, p):
    """the 8-bit digit of the D-th largest key in pass p"""
    kd = np.sort(f32_key(s).astype(np.uint64))[::-1][D - 1]
    return int((kd >> (32 - 8 * p)) & 255)


def _sel_case(name, nseg, n_max, D, scores, nc=3, nk=None, seed=0):
    """scores: [N] candidate scores in t order (before n_keep cuts them); stored through a shuffled keep"""
    rng = np.random.RandomState(seed + nseg * 131 + n_max)
    N = nseg * n_max
    scores = np.asarray(scores, np.float32)
    assert scores.shape == (N,)
    P = N + 5
    where = rng.permutation(P)[:N]                       # candidate t lives at flat box index where[t]
    prob = np.full(P, 0.75, np.float32)
    prob[where] = scores
    boxes = rng.randn(P, 7).astype(np.float32)
    nk = np.full(nseg, n_max, np.int32) if nk is None else np.asarray(nk, np.int32)
    return dict(name=name, nseg=nseg, n_max=n_max, D=D, nc=nc, keep=where.astype(np.int32).reshape(nseg, n_max), nk=nk,
                prob=prob, boxes=boxes)


def _from_bits(b):
    return np.asarray(b, np.uint32).view(np.float32)


def select_cases():
    out = []
    rng = np.random.RandomState(3)
    # sizes: 1 -> 2 -> 8 candidates per thread, the last thread's short range; every D edge
    for nseg, n_max in ((1, 1), (1, 1023), (3, 341), (2, 512), (1, 1025), (5, 205), (1, 2049), (8, 1024), (4, 2048)):
        N = nseg * n_max
        grid = (np.round(rng.rand(N) * 40) / 40 + 0.0125).astype(np.float32)
        nk = rng.randint(0, n_max + 1, nseg)
        for D in sorted({0, 1, N - 1, N, N + 1, 200}):
            out.append(_sel_case(f"size_{nseg}x{n_max}_D{D}", nseg, n_max, D, grid, nc=nseg + 1, nk=nk))
        out.append(_sel_case(f"size_{nseg}x{n_max}_full_D{max(N // 2, 1)}", nseg, n_max, max(N // 2, 1), grid, nc=nseg + 1))
    # fewer survivors than D: the threshold is a padding entry
    out.append(_sel_case("few_survivors", 2, 50, 60, 0.1 + 0.8 * rng.rand(100), nk=[30, 20]))
    # the D-th key decided in pass 1 .. 4: scores that differ in one byte only
    for p in (1, 2, 3, 4):
        sh = 32 - 8 * p
        n = 600
        if p == 1:
            b = (np.uint32(0x30) + rng.randint(0, 16, n).astype(np.uint32)) << np.uint32(24) | np.uint32(0x00123456)
        else:
            b = np.uint32(0x3f000000) | (rng.randint(0, 100, n).astype(np.uint32) << np.uint32(sh))
            if p < 4:
                b |= np.uint32(0x5a) >> np.uint32(8 - min(8, sh))     # equal low bits below the deciding byte
        out.append(_sel_case(f"pass{p}", 1, n, 97, _from_bits(b), nc=2))
        out.append(_sel_case(f"pass{p}_segments", 3, 200, 301, _from_bits(b), nc=9, nk=[200, 150, 200]))
    # the D-th key in bin 0 of a pass: pass 1 (-inf: key 0x007fffff), passes 2..4 (+0.0: key 0x80000000)
    s = 0.5 + rng.rand(300).astype(np.float32)
    s[:40] = -np.inf
    out.append(_sel_case("bin0_pass1_neg_inf", 1, 300, 280, s))
    s = 0.5 + rng.rand(300).astype(np.float32)
    s[10:60] = 0.0
    out.append(_sel_case("bin0_zero", 1, 300, 270, s))
    # everything equal: all stay, more than D rows come back
    out.append(_sel_case("all_equal", 2, 700, 5, np.full(1400, 0.3125, np.float32)))
    out.append(_sel_case("all_equal_cut", 2, 700, 5, np.full(1400, 0.3125, np.float32), nk=[13, 0]))
    # n_keep 0 / n_max / nothing anywhere; labels with nc = 2 and 9
    g = (np.round(rng.rand(1200) * 40) / 40 + 0.0125).astype(np.float32)
    out.append(_sel_case("nk_zero_and_full", 4, 300, 100, g, nc=9, nk=[0, 300, 0, 300]))
    out.append(_sel_case("nk_all_zero", 4, 300, 100, g, nc=2, nk=[0, 0, 0, 0]))
    out.append(_sel_case("nc2", 1, 1200, 100, g, nc=2))
    out.append(_sel_case("nc9", 8, 150, 100, g, nc=9, nk=[150, 3, 77, 0, 150, 1, 149, 20]))
    # zeros of both signs and NaN: -0.0 stays (s >= 0), a NaN ranks first and is never selected
    z = 0.25 + rng.rand(400).astype(np.float32)
    z[::7] = -0.0
    z[3::11] = 0.0
    out.append(_sel_case("zeros_all_stay", 1, 400, 0, z))
    out.append(_sel_case("zeros_D_above_positive", 1, 400, 390, z))          # the D-th is a zero: both signs stay
    out.append(_sel_case("zeros_padding_thresh", 2, 200, 390, z, nk=[150, 200]))
    z2 = z.copy()
    z2[1::13] = -0.125                                                       # below zero: never stays
    out.append(_sel_case("negative_scores_D0", 1, 400, 0, z2))
    out.append(_sel_case("negative_scores_thresh", 1, 400, 399, z2))
    q = 0.25 + rng.rand(400).astype(np.float32)
    q[5::40] = np.nan
    q[6::80] = _from_bits([0xffc00001])[0]                                   # a NaN with the sign bit
    nn = int(np.isnan(q).sum())
    out.append(_sel_case("nan_D0", 1, 400, 0, q))
    out.append(_sel_case("nan_below_D", 1, 400, nn + 20, q))                 # 20 finite scores stay
    out.append(_sel_case("nan_is_dth", 1, 400, nn, q))                       # thresh is a NaN: nothing
    out.append(_sel_case("nan_is_first", 1, 400, 1, q))
    out.append(_sel_case("nan_D_N", 2, 200, 400, q))
    out.append(_sel_case("nan_all", 1, 64, 10, np.full(64, np.nan, np.float32)))
    qi = q.copy()
    qi[7::50] = np.inf
    out.append(_sel_case("nan_and_inf", 1, 400, nn + 3, qi))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def cases_by_name():
    return {c["name"]: c for c in select_cases()}


def post_scores_reference(prob, thresh):
    """k_post_scores: sc [nc-1, K] = prob[:, j+1] where > thresh else -1 (prob == thresh and NaN: -1), counts"""
    with np.errstate(invalid="ignore"):
        c = prob[:, 1:].T > np.float32(thresh)
    return np.where(c, prob[:, 1:].T, np.float32(-1)).astype(np.float32), c.sum(1).astype(np.int32)


def post_scores_case(K, nc, seed=0):
    rng = np.random.RandomState(seed + 17 * K + nc)
    thresh = np.float32(0.05)
    prob = (rng.rand(K, nc) * 0.2).astype(np.float32)
    flat = prob.reshape(-1)
    flat[::3] = thresh                                   # excluded
    flat[1::7] = np.nextafter(thresh, np.float32(1))     # the first value that counts
    flat[2::11] = np.nan
    return prob, float(thresh)


def post_order_reference(idx, nc):
    """order[j][i] = idx[j][i] * nc + j + 1: box index of (RoI idx[j][i], class j + 1) in the [K, nc] layout"""
    return (idx * nc + np.arange(1, idx.shape[0] + 1)[:, None]).astype(np.int32)


def gather_kept_reference(boxes, scores, keep, n_keep, P, min_size):
    """k_gather_kept: row i < n_keep is candidate keep[i], the others candidate 0; sizes `v < min_size ? min_size : v`
    (torch.clamp(min=): a NaN stays; -0.0 is not below 0.0)"""
    j = np.where(np.arange(P) < n_keep, keep[:P], 0)
    b = boxes[j].copy()
    with np.errstate(invalid="ignore"):
        b[:, 3:6] = np.where(b[:, 3:6] < np.float32(min_size), np.float32(min_size), b[:, 3:6])
    return b, scores[j]
