"""What the BatchNorm tests share and a machine without a GPU can check (test_bn_forms_cpu.py): the fp64 references of
the statistics, the affine + activation pass and the backward pass, the generators of exact-arithmetic and of rounding
data with their preconditions, the comparators with their bounds, and the dispatch arithmetic of bn.hip / bn_backward.hip
restated (run_stats, run_stats_partials, launch_bn_apply, d3d_bn_apply_dt, bn_backward_t) -- the record
d3d_bn_last_form must give for (rows, planes, storage type, alignment).  expect_bn assumes D3D_BN_SLICES is unset."""
import numpy as np

# ---------------------------------------------------------------------------------------------------- the record
BN_FIELDS = ("st_src", "st_type", "st_mode", "st_lanes", "st_row_lanes", "st_slices", "st_groups", "st_last_group",
             "st_per", "ap_kernel", "ap_type", "ap_wgs", "ap_multi", "bw_partial", "bw_slices", "bw_apply", "bw_wgs",
             "bw_multi", "bw_type")
TENSOR, PARTIALS, RUNNING = 1, 2, 3          # st_src
F32, BF16, F64 = 1, 2, 3                     # st_type / ap_type / bw_type
ROWS, VEC4, SCALAR = 1, 2, 3                 # ap_kernel / bw_apply; bw_partial: VEC4 -> 1, SCALAR -> 2
PARTIAL_VEC4, PARTIAL_SCALAR = 1, 2

STAT_THREADS = 1024                          # kStatThreads
STAT_BLOCKS = 128                            # kStatBlocks: row slices of k_bn_stats
STAT_GROUP = 16                              # kStatGroup: slices per first-level group
STAT_PASSES = 8                              # a slice is at least 8 passes of the row lanes
PARTIALS_SLICE_CAP = 64                      # run_stats_partials without D3D_BN_SLICES
TICKET_BYTES = 256                           # kTicketBytes
APPLY_THREADS = 256
APPLY_WG_CAP = 2048                          # 256 * 8 workgroups of the row-walking kernels
BWD_BLOCKS = 128                             # kBnBwdBlocks
BWD_SCALAR_ROWS = 64                         # rows per slice of the scalar partial kernel below 128 * 64 rows

U32 = 2.0 ** -24                             # unit roundoff of fp32
UBF = 2.0 ** -8                              # unit roundoff of bf16 (8 significand bits, the leading one implied)


def cdiv(a, b):
    return -(-a // b)


def _zero():
    return dict.fromkeys(BN_FIELDS, 0)


def stats_planes_ok(planes):
    return 0 < planes <= 4096 and planes % 4 == 0 and STAT_THREADS % (planes // 4) == 0


def partials_planes_ok(planes):
    """run_stats_partials: stat_reduce_rows walks the 2 C values in whole passes of 1024 threads"""
    return 0 < planes <= 4096 and planes % 4 == 0 and (2 * planes <= STAT_THREADS or 2 * planes % STAT_THREADS == 0)


def _groups(f, nblk, n):
    f["st_slices"] = nblk
    f["st_groups"] = cdiv(nblk, STAT_GROUP)
    f["st_last_group"] = nblk - (f["st_groups"] - 1) * STAT_GROUP
    f["st_per"] = cdiv(n, nblk)


def expect_stats(rows, planes, typ, mode):
    """run_stats: k_bn_stats<float / bf16> over the tensor"""
    assert stats_planes_ok(planes) and rows > 0 and typ in (F32, BF16) and mode in (0, 1, 2)
    lpr = planes // 4
    rl = STAT_THREADS // lpr
    nblk = max(1, min(STAT_BLOCKS, cdiv(rows, STAT_PASSES * rl)))
    f = dict(st_src=TENSOR, st_type=typ, st_mode=mode, st_lanes=lpr, st_row_lanes=rl)
    _groups(f, nblk, rows)
    return f


def expect_stats_partials(partial_rows, planes, mode):
    """run_stats_partials: k_bn_stats<double> over partial_rows rows of [2 planes] column sums"""
    assert partials_planes_ok(planes) and partial_rows > 0 and mode in (0, 2)
    v = 2 * planes
    vp = min(v, STAT_THREADS)
    sl = STAT_THREADS // vp
    nblk = max(1, min(cdiv(partial_rows, STAT_PASSES * sl), PARTIALS_SLICE_CAP, STAT_BLOCKS))
    f = dict(st_src=PARTIALS, st_type=F64, st_mode=mode, st_lanes=vp, st_row_lanes=sl)
    _groups(f, nblk, partial_rows)
    return f


def apply_rows_kernel(planes):
    c4 = planes // 4
    return planes % 4 == 0 and 1 <= c4 <= APPLY_THREADS and APPLY_THREADS % c4 == 0


def expect_apply(rows, planes, typ):
    """launch_bn_apply (fp32) / d3d_bn_apply_dt (bf16: the row-walking kernel only)"""
    assert rows > 0 and typ in (F32, BF16)
    if apply_rows_kernel(planes):
        rpi = APPLY_THREADS // (planes // 4)
        wgs = max(1, min(cdiv(rows, rpi), APPLY_WG_CAP))
        return dict(ap_kernel=ROWS, ap_type=typ, ap_wgs=wgs, ap_multi=int(rows > 3 * wgs * rpi))
    assert typ == F32, "bf16 rows have the row-walking kernel only"
    total = rows * planes
    return dict(ap_kernel=VEC4 if planes % 4 == 0 else SCALAR, ap_type=F32, ap_wgs=(total // 4 + 256) // 256, ap_multi=0)


def backward_planes_ok(planes):
    return planes > 0 and (planes % 256 == 0 if planes >= 256 else 256 % planes == 0)


def expect_backward(rows, planes, typ, aligned16=True):
    """bn_backward_t.  aligned16: all four feature pointers are 16-byte aligned"""
    assert backward_planes_ok(planes) and rows > 0 and typ in (F32, BF16)
    vec4 = planes % 4 == 0 and STAT_THREADS % (planes // 4) == 0 and aligned16
    if vec4:
        rl = STAT_THREADS // (planes // 4)
        nblk = max(1, min(BWD_BLOCKS, cdiv(rows, STAT_PASSES * rl)))
    else:
        nblk = BWD_BLOCKS if rows >= BWD_BLOCKS * BWD_SCALAR_ROWS else max(1, cdiv(rows, BWD_SCALAR_ROWS))
    f = dict(bw_partial=PARTIAL_VEC4 if vec4 else PARTIAL_SCALAR, bw_slices=nblk, bw_type=typ, bw_multi=0)
    total = rows * planes
    if vec4 and apply_rows_kernel(planes):
        rpi = APPLY_THREADS // (planes // 4)
        wgs = max(1, min(cdiv(rows, rpi), APPLY_WG_CAP))
        f.update(bw_apply=ROWS, bw_wgs=wgs, bw_multi=int(rows > wgs * rpi))
    elif vec4:
        f.update(bw_apply=VEC4, bw_wgs=cdiv(total // 4, 256))
    else:
        f.update(bw_apply=SCALAR, bw_wgs=cdiv(total, 256))
    return f


def expect_bn(rows, planes, typ, stats=None, apply=False, backward=False, aligned16=True):
    """The whole record after one call.  stats: None, ("tensor", mode), ("partials", mode, partial_rows) or "running"
    (eval mode of d3d_bn_forward_dt: running statistics, nothing else recorded); apply / backward: that stage ran."""
    f = _zero()
    if rows == 0:
        return f                              # every entry point returns before its first launch
    if stats == "running":
        f["st_src"] = RUNNING
    elif stats is not None and stats[0] == "tensor":
        f.update(expect_stats(rows, planes, typ, stats[1]))
    elif stats is not None:
        assert stats[0] == "partials"
        f.update(expect_stats_partials(stats[2], planes, stats[1]))
    if apply:
        f.update(expect_apply(rows, planes, typ))
    if backward:
        f.update(expect_backward(rows, planes, typ, aligned16))
    return f


def slice_rows(n, nblk):
    """rows of every slice: per = ceil(n / nblk), the trailing slices may be short or empty"""
    per = cdiv(n, nblk)
    return [max(0, min(n, (b + 1) * per) - min(n, b * per)) for b in range(nblk)]


def stats_row_counts(planes, full):
    """the row counts of the statistics (and vec4 backward) cases of a channel class, from the constants above"""
    rl = STAT_THREADS // (planes // 4)
    t = STAT_PASSES * rl
    if planes == 4:                            # T = 8192: the one-slice and two-group forms only
        return [t, t + 1, STAT_GROUP * t + 1]
    if not full:
        return sorted({1, rl + 1, 4 * rl + 1, t + 1, STAT_GROUP * t + 1})
    n = {1, 2, 3, rl - 1, rl, rl + 1,
         4 * rl, 4 * rl + 1, 6 * rl, 7 * rl,               # the 4-pass loop alone, then tails of 1, 2 and 3 passes
         t, t + 1, STAT_GROUP * t, STAT_GROUP * t + 1,
         (STAT_BLOCKS - 1) * t + 1}                        # 128 slices, the last one short
    if planes == 4096:
        n.add(1100)                                         # 128 slices of 9 rows: 123 .. 127 are empty
    return sorted(r for r in n if r > 0)


# ------------------------------------------------------------------------------------------------- number formats
def f32(a):
    return np.asarray(a, dtype=np.float32)


def is_f32(a):
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(over="ignore"):
        return bool(np.array_equal(a.astype(np.float32).astype(np.float64), a))


def ulp32(v):
    """the spacing of fp32 numbers at |v| (normal range)"""
    v = np.abs(np.asarray(v, dtype=np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        return 2.0 ** (np.floor(np.log2(np.maximum(v, 2.0 ** -126))) - 23)


def gamma(n):
    return n * U32 / (1 - n * U32)


def bf16_round(a):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32; NaN stays NaN"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(a), a, r).astype(np.float32)


def is_bf16(a):
    a = f32(a)
    return bool(np.array_equal(bf16_round(a).view(np.uint32), a.view(np.uint32)))


def same_bits(got, want):
    """equal to the bit; a NaN equals any NaN"""
    got, want = f32(got), f32(want)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


MARGINS = {}    # check -> largest error seen as a fraction of its bound (recorded for DESIGN.md, never used to set one)


def within(name, got, want, bound):
    """|got - want| <= bound element by element (NaN must meet NaN); records the largest fraction of the bound used"""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    assert got.shape == want.shape, f"{name}: shape {got.shape} != {want.shape}"
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{name}: NaN where the reference has none, or none where it has one"
    bound = np.broadcast_to(bound, want.shape)
    inf = np.isinf(want) & ~nan
    assert np.array_equal(got[inf], want[inf]), f"{name}: infinities differ"
    ok = ~nan & ~inf
    err = np.abs(got[ok] - want[ok])
    b = bound[ok]
    bad = err > b
    if bad.any():
        i = int(np.argmax(np.where(b > 0, err / np.where(b > 0, b, 1), np.where(err > 0, np.inf, 0))))
        raise AssertionError(f"{name}: {int(bad.sum())} of {err.size} outside the bound; worst error {err[i]:.3e} against "
                             f"{b[i]:.3e} (got {got[ok][i]!r}, want {want[ok][i]!r})")
    if err.size:
        frac = float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1), 0.0)))
        MARGINS[name] = max(MARGINS.get(name, 0.0), frac)


def exact(name, got, want, tag=""):
    assert same_bits(got, want), f"{name} {tag}: not equal to the bit ({int((f32(got) != f32(want)).sum())} values differ)"
    MARGINS.setdefault(name + " (bit for bit)", 0.0)


# ------------------------------------------------------------------------------------------------------ generators
def int_rows(rng, rows, planes, lo=1, hi=4):
    """non-zero integers in +-{lo..hi}: a lost or doubled row changes every column sum"""
    return (rng.randint(lo, hi + 1, (rows, planes)) * rng.choice((-1, 1), (rows, planes))).astype(np.float32)


RATIOS = (0.0, 1.0, 64.0)       # mean / std of the rounding data, by column: 64 is the hard column of a one-pass variance


def normal_rows(rng, rows, planes, bf16=False):
    """normal data with per-column mean / std of 0, 1 and 64 (column c has RATIOS[c % 3]); bf16: rounded to bf16"""
    x = rng.randn(rows, planes) + np.asarray(RATIOS)[np.arange(planes) % 3]
    x = x.astype(np.float32)
    return bf16_round(x) if bf16 else x


def exact_params(rng, planes, pow2_invstd=False):
    """saved mean a small integer, invstd and gamma powers of two times small integers, beta an integer"""
    mean = rng.randint(-2, 3, planes).astype(np.float32)
    invstd = (2.0 ** rng.randint(-2, 2, planes) * (1 if pow2_invstd else rng.choice((1, 3), planes))).astype(np.float32)
    gam = (2.0 ** rng.randint(-1, 2, planes) * rng.choice((1, 3, 5), planes) * rng.choice((-1, 1), planes)).astype(np.float32)
    beta = rng.randint(-3, 4, planes).astype(np.float32)
    return mean, invstd, gam, beta


# --------------------------------------------------------------------------------------------------- the statistics
def col_sums(x):
    """fp64 column sum and sum of squares"""
    x = np.asarray(x, dtype=np.float64)
    return x.sum(0), (x * x).sum(0)


def stats_from_sums(s, q, rows, m2=None):
    """mean, sum of squared deviations, unbiased and biased variance; rows = 1: unbiased variance NaN (0 / 0)"""
    s, q = np.asarray(s, np.float64), np.asarray(q, np.float64)
    mean = s / rows
    if m2 is None:
        m2 = np.maximum((q * rows - s * s) / rows, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        var_u = m2 / (rows - 1) if rows > 1 else np.full_like(m2, np.nan)
    return mean, m2, var_u, m2 / rows


def stats_ref(x):
    """two-pass fp64 statistics of x and kappa = sum x^2 / sum (x - mean)^2 per column"""
    x = np.asarray(x, dtype=np.float64)
    rows = x.shape[0]
    s, q = col_sums(x)
    mean = s / rows
    m2 = ((x - mean) ** 2).sum(0)
    _, _, var_u, var_b = stats_from_sums(s, q, rows, m2)
    with np.errstate(invalid="ignore", divide="ignore"):
        kappa = np.where(m2 > 0, q / np.where(m2 > 0, m2, 1), 1.0)
    return dict(rows=rows, s=s, q=q, mean=mean, m2=m2, var_u=var_u, var_b=var_b, kappa=kappa)


def stats_ref_exact(s, q, rows):
    """the statistics from exact integer sums (s, q below 2^53, and so is q * rows - s^2: asserted)"""
    s, q = np.asarray(s, np.float64), np.asarray(q, np.float64)
    assert_exact_sums(s, q, rows)
    mean, m2, var_u, var_b = stats_from_sums(s, q, rows)
    return dict(rows=rows, s=s, q=q, mean=mean, m2=m2, var_u=var_u, var_b=var_b, kappa=np.ones_like(s))


def assert_exact_sums(s, q, rows):
    """every sum the kernel forms is an integer below 2^53 in any order, and the reference's q rows - s^2 too"""
    s, q = np.asarray(s, np.float64), np.asarray(q, np.float64)
    assert np.array_equal(s, np.rint(s)) and np.array_equal(q, np.rint(q)), "sums of integer data must be integers"
    assert (q >= np.abs(s)).all(), "sum of squares below |sum|: not the sums of integer rows"
    assert float(q.max(initial=0)) * rows < 2.0 ** 53, "q * rows is not an exact fp64 integer"
    assert float(np.abs(s).max(initial=0)) ** 2 < 2.0 ** 53, "s^2 is not an exact fp64 integer"


def assert_exact_rows(x, amax=4):
    """x holds non-zero integers of magnitude <= amax: fp32 and bf16 hold them exactly, squares and sums of up to 2^48
    of them are exact in fp64"""
    x = np.asarray(x, dtype=np.float64)
    assert np.array_equal(x, np.rint(x)) and (x != 0).all() and np.abs(x).max(initial=1) <= amax, \
        f"rows must be non-zero integers of magnitude <= {amax}"
    assert x.shape[0] * amax * amax < 2 ** 48
    assert is_bf16(x)


def invstd_of(var, eps):
    """(var + eps)^-1/2 in fp64, eps the fp32 value the kernel is given"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return (np.asarray(var, np.float64) + float(np.float32(eps))) ** -0.5


def running_update(old, new, momentum):
    """retention momentum: momentum * old + (1 - momentum) * new, with the fp32 values of momentum and 1 - momentum"""
    m = np.float32(momentum)
    return float(m) * np.asarray(old, np.float64) + float(np.float32(1) - m) * np.asarray(new, np.float64)


def var_bound(ref, var):
    """relative 2^-23 + (rows + 4) 2^-52 kappa: the final fp32 rounding (twice half an ulp of reserve) and the one-pass
    fp64 formula sum x^2 - mean^2 rows, whose cancellation loses a factor kappa"""
    return (2.0 ** -23 + (ref["rows"] + 4) * 2.0 ** -52 * ref["kappa"]) * np.abs(var)


def check_stats(tag, ref, mode, eps, got_mean, got_other, exact_data, running=None):
    """the outputs of one statistics launch against `ref` (stats_ref or stats_ref_exact).
    mode 0: other = unbiased variance; 1: other = invstd of the biased variance, running = (old mean, old var, momentum,
    got mean, got var); 2: other = invstd of the unbiased variance.
    exact_data: the sums are exact, so the mean is float32(S / rows) to the bit and what follows has 1 ulp."""
    kind = "exact" if exact_data else "rounding"
    if exact_data:
        exact(f"stats mean [{kind}]", got_mean, f32(ref["mean"]), tag)
    else:
        within(f"stats mean [{kind}]", got_mean, ref["mean"], ulp32(ref["mean"]))
    var = ref["var_b"] if mode == 1 else ref["var_u"]
    if mode == 0:
        within(f"stats variance [{kind}]", got_other, var, ulp32(var) if exact_data else var_bound(ref, var))
    else:
        want = invstd_of(var, eps)
        within(f"stats invstd [{kind}]", got_other, want, 4 * ulp32(want))
    if running is not None:
        old_mean, old_var, momentum, new_mean, new_var = running
        wm, wv = running_update(old_mean, ref["mean"], momentum), running_update(old_var, ref["var_u"], momentum)
        if exact_data:
            bm, bv = ulp32(wm), ulp32(wv)
        else:   # three fp32 roundings of the update, on a new value with the error allowed above
            one = float(np.float32(1) - np.float32(momentum))
            am = float(np.float32(momentum)) * np.abs(old_mean) + one * np.abs(ref["mean"])
            av = float(np.float32(momentum)) * np.abs(old_var) + one * np.abs(ref["var_u"])
            bm = gamma(3) * am + one * ulp32(ref["mean"])
            bv = gamma(3) * av + one * var_bound(ref, ref["var_u"])
        within(f"running mean [{kind}]", new_mean, wm, bm)
        within(f"running variance [{kind}]", new_var, wv, bv)


def exact_running(rng, planes):
    """running statistics 8 .. 12 with momentum 0.75: 0.75 old and 0.25 new are exact in fp32 and the sum is at least 5,
    so its one rounding and a quarter of the new value's error stay inside 1 ulp"""
    return rng.randint(8, 13, planes).astype(np.float32), rng.randint(8, 13, planes).astype(np.float32), 0.75


# ----------------------------------------------------------------------------------------------------------- apply
def apply_ref(x, mean, invstd, weight, bias, leak):
    """y = leaky(x w + b), w = invstd gamma, b = -mean w + beta in fp64; -> y and |x w| + |mean w| + |beta|.
    leak 0 is max(t, 0), which sends NaN to +0; leak > 0 keeps NaN."""
    x = np.asarray(x, np.float64)
    w = np.asarray(invstd, np.float64) * (1.0 if weight is None else np.asarray(weight, np.float64))
    beta = 0.0 if bias is None else np.asarray(bias, np.float64)
    b = -np.asarray(mean, np.float64) * w + beta
    with np.errstate(invalid="ignore", over="ignore"):
        t = x * w + b
        y = np.where(t > 0, t, 0.0 if leak == 0 else t * float(np.float32(leak)))
        mag = np.abs(x * w) + np.abs(np.asarray(mean, np.float64) * w) + np.abs(beta)
    return y, mag


def assert_exact_apply(x, mean, invstd, weight, bias, leak):
    """every product, sum and the leak product the kernel forms is an fp32 number"""
    fin = np.isfinite(np.asarray(x, np.float64))
    xf = np.where(fin, np.asarray(x, np.float64), 1.0)
    w = np.asarray(invstd, np.float64) * (1.0 if weight is None else np.asarray(weight, np.float64))
    mw = np.asarray(mean, np.float64) * w
    b = -mw + (0.0 if bias is None else np.asarray(bias, np.float64))
    t = xf * w + b
    lk = float(np.float32(leak))
    assert is_f32(w) and is_f32(mw) and is_f32(b) and is_f32(xf * w) and is_f32(t) and is_f32(t * lk), \
        "the apply pass would round: not an exact case"


def check_apply(tag, got, x, mean, invstd, weight, bias, leak, exact_data, bf16):
    """got: fp32 values of the output (bf16 storage widened)"""
    y, mag = apply_ref(x, mean, invstd, weight, bias, leak)
    if exact_data:
        want = y.astype(np.float32)
        exact(f"apply [exact{', bf16' if bf16 else ''}]", got, bf16_round(want) if bf16 else want, tag)
        return
    bound = gamma(3) * mag
    if bf16:
        bound = bound + UBF * (np.abs(y) + bound)
    within(f"apply [rounding{', bf16' if bf16 else ''}]", got, y, bound)


# -------------------------------------------------------------------------------------------------------- backward
def backward_ref(x, y, dy, mean, invstd, weight, leak, sign_ge=False):
    """BatchNormalization.cpp:62-107 in fp64 with d' = dy (y > 0 ? 1 : leak): d_bias = sum d', dp = sum (x - mean) d',
    d_weight = dp invstd, gm = d_bias / rows, k = dp invstd^2 / rows, dx = (d' - gm - (x - mean) k) invstd w.
    sign_ge: the mutated rule y >= 0 (for the mutation check)."""
    x, y, dy = (np.asarray(a, np.float64) for a in (x, y, dy))
    mean, invstd = np.asarray(mean, np.float64), np.asarray(invstd, np.float64)
    w = 1.0 if weight is None else np.asarray(weight, np.float64)
    rows = x.shape[0]
    pos = (y >= 0) if sign_ge else (y > 0)
    d = dy * np.where(pos, 1.0, float(np.float32(leak)))
    xm = x - mean
    d_bias, dp = d.sum(0), (xm * d).sum(0)
    gm, k = d_bias / rows, dp * invstd * invstd / rows
    dx = (d - gm - xm * k) * invstd * w
    return dict(rows=rows, d=d, xm=xm, d_bias=d_bias, dp=dp, d_weight=dp * invstd, gm=gm, k=k, dx=dx,
                a_bias=np.abs(d).sum(0), a_dp=(np.abs(xm) * np.abs(d)).sum(0), isw=np.abs(invstd * w),
                invstd=invstd)


def assert_exact_backward(x, y, dy, mean, invstd, leak):
    """d', x - mean and their product are fp32 numbers, the sums fp64 integers (in units of the leak's 1/4) that fp32
    holds, and d_weight = float(dp) invstd is one too"""
    r = backward_ref(x, y, dy, mean, invstd, None, leak)
    assert float(np.float32(leak)) in (0.0, 0.25)
    assert is_f32(r["d"]) and is_f32(r["xm"]) and is_f32(r["xm"] * r["d"]), "the backward products would round"
    assert np.array_equal(4 * r["d"], np.rint(4 * r["d"])) and np.array_equal(r["xm"], np.rint(r["xm"]))
    assert 4 * float(r["a_dp"].max()) < 2 ** 24 and 4 * float(r["a_bias"].max()) < 2 ** 24, \
        "a column sum does not fit fp32 exactly"
    assert is_f32(r["d_weight"]), "d_weight = dp invstd would round"
    return r


def check_backward(tag, ref, got_dx, got_dw, got_db, exact_data, bf16):
    """got_dx: fp32 values (bf16 storage widened); got_dw / got_db: None when the call passed NULL"""
    kind = "exact" if exact_data else "rounding"
    if exact_data:
        if got_db is not None:
            exact("d_bias [exact]", got_db, f32(ref["d_bias"]), tag)
        if got_dw is not None:
            exact("d_weight [exact]", got_dw, f32(ref["d_weight"]), tag)
    else:
        # the fp32 terms of a sum: 2 u of their magnitudes; then the final rounding -- one conversion for d_bias, a
        # conversion and a product for d_weight
        if got_db is not None:
            within("d_bias [rounding]", got_db, ref["d_bias"], 2 * U32 * ref["a_bias"] + U32 * np.abs(ref["d_bias"]))
        if got_dw is not None:
            within("d_weight [rounding]", got_dw, ref["d_weight"],
                   2 * U32 * ref["a_dp"] * ref["invstd"] + gamma(2) * np.abs(ref["d_weight"]))
    # dx: six fp32 operations on fp32 operands, with gm good to 1 u and k to 3 u (dp's conversion, two products, one
    # division) GIVEN the sums.  In the rounding cases the sums themselves carry the error bounded above, 2 u of their
    # terms' magnitudes, and gm = sum / rows and k = dp invstd^2 / rows inherit it as an absolute error: where a sum
    # cancels (dp is of the order sqrt(rows), its terms' magnitudes add up to rows) that is far more than 3 u of k.
    agm, ak = np.abs(ref["gm"]), np.abs(ref["xm"]) * np.abs(ref["k"])
    bound = gamma(6) * (np.abs(ref["d"]) + agm + ak) + U32 * agm + 3 * U32 * ak
    if not exact_data:
        rows = ref["rows"]
        bound = bound + 2 * U32 * ref["a_bias"] / rows + np.abs(ref["xm"]) * (2 * U32 * ref["a_dp"] * ref["invstd"] ** 2 / rows)
    bound = bound * ref["isw"]
    if bf16:
        bound = bound + UBF * (np.abs(ref["dx"]) + bound)
    within(f"dx [{kind}{', bf16' if bf16 else ''}]", got_dx, ref["dx"], bound)


# ------------------------------------------------------------------------------------------------------- the cases
FULL_CLASSES = (4096, 1024, 128, 32)                    # every row-count class
OTHER_CLASSES = (2048, 512, 256, 64, 16, 8)             # the channel class itself, at a reduced list
STATS_PLANES = (4,) + tuple(sorted(FULL_CLASSES + OTHER_CLASSES))
EPS = 1e-4


def seed_of(*key):
    return (sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) + 17) % (2 ** 31 - 1)


def stats_cases(planes):
    return [(planes, rows) for rows in stats_row_counts(planes, planes in FULL_CLASSES)]


PARTIALS_PLANES = (4, 12, 128, 512, 1024, 1536, 4096)   # V = 8 (SL 128), 24 (no divisor of 1024), 256, 1024 (SL 1), then
                                                        # two, three and eight passes over the values
PARTIALS_REFUSED = (768, 516, 1280)                     # 2 C above 1024 and no multiple of it: an error, not a launch


def partials_row_counts(planes):
    sl = STAT_THREADS // min(2 * planes, STAT_THREADS)
    t = STAT_PASSES * sl
    return sorted({1, t, t + 1, STAT_GROUP * t + 1, PARTIALS_SLICE_CAP * t + 1})


def make_partials(rng, partial_rows, planes):
    """hand-made fp64 integer rows [partial_rows, 2 planes]: sums in +-{1..4}, sums of squares 16 .. 20, standing for a
    tensor of rows = 3 partial_rows + 1 rows (so that sum^2 / rows stays below the sum of squares)"""
    s = rng.randint(1, 5, (partial_rows, planes)) * rng.choice((-1, 1), (partial_rows, planes))
    q = rng.randint(16, 21, (partial_rows, planes))
    return np.concatenate([s, q], 1).astype(np.float64), 3 * partial_rows + 1


VARIANTS = ((True, True, 0.0), (True, True, 0.25), (False, True, 0.0), (True, False, 0.25), (False, False, 0.25),
            (False, False, 0.0))                        # weight present, bias present, leak


def apply_cases():
    """(planes, rows, storage) of the apply pass"""
    cases = []
    for planes in (4, 16, 64, 256, 1024):
        rpi = APPLY_THREADS // (planes // 4)
        rows = {1, rpi - 1, rpi, rpi + 1} - {0}
        if planes == 1024:
            cap = APPLY_WG_CAP * rpi
            rows |= {cap, cap + 1, 3 * cap, 3 * cap + 1, 4 * cap + 1}      # the workgroup cap, then the 4-row loop
        if planes in (256, 64):
            rows.add(3 * APPLY_WG_CAP * rpi + rpi + 1)                     # the 4-row loop for some, a tail for all
        cases += [(planes, r, t) for r in sorted(rows) for t in (F32, BF16)]
    cases += [(planes, r, F32) for planes in (2048, 4096) for r in (1, 3, 130)]
    cases += [(1, r, F32) for r in (1, 4, 5, 6, 7, 1027)]
    cases += [(6, r, F32) for r in (1, 2, 683)]
    cases += [(9, r, F32) for r in (1, 2, 3, 4, 1001)]
    return cases


def backward_cases():
    """(planes, rows, storage, aligned16) of the backward pass"""
    cases = []
    for planes in STATS_PLANES:
        rl = STAT_THREADS // (planes // 4)
        t = STAT_PASSES * rl
        if planes == 4:
            rows = {t, t + 1, 8 * t + 1}
        elif planes in FULL_CLASSES:    # slices 1, 2, 7, 8, 9, 128 (k_bn_bwd_finish adds them in 8 lanes), 128 short
            rows = {1, 2, 3, rl - 1, rl, rl + 1, t, t + 1, 6 * t + 1, 7 * t + 1, 8 * t + 1, 127 * t + 1, 128 * t + 1} - {0}
            if planes == 4096:
                rows.add(1100)
            if planes == 1024:
                rows |= {2048, 2049, 4097}                                  # the apply pass' two-row loop and its tail
        else:
            rows = {1, rl + 1, t + 1}
        cases += [(planes, r, ty, True) for r in sorted(rows) for ty in (F32, BF16)]
    scalar_rows = (1, 63, 64, 65, 8191, 8192)
    cases += [(planes, r, ty, True) for planes in (1, 2, 768) for r in scalar_rows for ty in (F32, BF16)]
    cases += [(4, r, BF16, False) for r in scalar_rows]
    return cases


def make_apply_case(planes, rows, typ, variant, exact_data):
    """-> x (fp32 values the storage type holds), mean, invstd, weight or None, bias or None, leak"""
    rng = np.random.RandomState(seed_of(planes, rows, typ, exact_data))
    has_w, has_b, leak = variant
    if exact_data:
        x = int_rows(rng, rows, planes)
        mean, invstd, gam, beta = exact_params(rng, planes)
    else:
        leak = 0.333 if leak else 0.0
        x = normal_rows(rng, rows, planes, typ == BF16)
        r = stats_ref(x) if rows > 1 else None
        mean = f32(r["mean"]) if r else f32(rng.randn(planes))
        invstd = f32(invstd_of(r["var_b"], EPS)) if r else f32(rng.uniform(0.5, 2, planes))
        gam, beta = f32(rng.uniform(0.5, 1.5, planes)), f32(rng.uniform(-0.5, 0.5, planes))
    return x, mean, invstd, (gam if has_w else None), (beta if has_b else None), leak


def make_backward_case(planes, rows, typ, variant, exact_data):
    """-> x, y, dy (fp32 values the storage type holds), mean, invstd, weight or None, leak.  y is hand-made in the exact
    cases (signs of its own, zeros of both signs); in the rounding cases it is the stored output of the forward pass."""
    rng = np.random.RandomState(seed_of(planes, rows, typ, exact_data, 3))
    has_w, _, leak = variant
    if exact_data:
        leak = 0.25 if leak else 0.0
        x, dy = int_rows(rng, rows, planes), int_rows(rng, rows, planes)
        y = rng.randint(-2, 3, (rows, planes)).astype(np.float32)
        y[(y == 0) & (rng.rand(rows, planes) < 0.5)] = -0.0
        tiny = rng.rand(rows, planes) < 0.05                   # the sign alone decides, whatever the magnitude
        y[tiny] = np.where(rng.rand(int(tiny.sum())) < 0.5, 1, -1) * np.float32(2.0 ** -100)
        mean, invstd, gam, _ = exact_params(rng, planes, pow2_invstd=True)
    else:
        leak = 0.333 if leak else 0.0
        bf = typ == BF16
        x = normal_rows(rng, rows, planes, bf)
        r = stats_ref(x)
        mean = f32(r["mean"])
        invstd = f32(invstd_of(r["var_b"], EPS)) if rows > 1 else f32(rng.uniform(0.5, 2, planes))
        gam, beta = f32(rng.uniform(0.5, 1.5, planes)), f32(rng.uniform(-0.5, 0.5, planes))
        y = apply_ref(x, mean, invstd, gam if has_w else None, beta, leak)[0].astype(np.float32)
        dy = rng.randn(rows, planes).astype(np.float32)
        if bf:
            y, dy = bf16_round(y), bf16_round(dy)
    return x, y, dy, mean, invstd, (gam if has_w else None), leak


ADD_SIZES = (1, 3, 4, 5, 1023, 1024, 1025) + tuple(4 * 256 * k + r for k in (1, 3) for r in range(4))
