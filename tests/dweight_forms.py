"""What the dWeight tests share and a machine without a GPU can check (test_dweight_forms_cpu.py): the fp64 reference of
dW over a rulebook, the precondition of the exact-arithmetic check, and the dispatcher's arithmetic restated
(conv_dw.hip launch_dw_with) -- the form d3d_conv_dw_last_form must report for a plan and a layer."""
import numpy as np

F32, BF16 = 1, 2                       # family
NONE, CALLER, LANE, ASYNC = 0, 1, 2, 3  # scratch of the fixed-order partials
DW_FIELDS = ("family", "cw", "cout", "cin", "T", "nz", "run", "chunk", "n_chunks", "gx", "gy", "gz", "det", "G", "scratch",
             "n_blk", "K")
BLOCKS_PER_WG = 64                     # kDwBlocksPerWg: one ballot covers the longest run
TARGET_WGS = 1024                      # kDwTargetWgs
MAX_CHUNK = 8                          # kDwMaxChunk
DET_PARTIALS = 32                      # kDwDetPartials
DET_BUDGET = 64 << 20                  # kDwDetBudget, bytes
CPS = (32, 64, 128, 256)               # CP of k_conv_dw
CSS = (16, 32, 64, 128, 256)           # CS of k_conv_dw_bf16
COUTS = (32, 64, 128, 256)
U32 = 2.0 ** -24


def dw64(x, gout, rules, fv, with_abs=True):
    """fp64 dW[k] = x[in_k]^T gout[out_k] over the rules (in, out, k) of offset k, and a[k] = |x|^T |gout|"""
    want = np.zeros((fv, x.shape[1], gout.shape[1]))
    a = np.zeros_like(want) if with_abs else None
    order = np.argsort(rules[:, 2], kind="stable")
    ks = rules[order, 2]
    lo, hi = np.searchsorted(ks, np.arange(fv)), np.searchsorted(ks, np.arange(fv), side="right")
    for k in range(fv):
        r = rules[order[lo[k]:hi[k]]]
        if len(r) == 0:
            continue
        xi, go = x[r[:, 0]], gout[r[:, 1]]
        want[k] = xi.T @ go
        if with_abs:
            a[k] = np.abs(xi).T @ np.abs(go)
    return want, a


def rules_per_offset(rules, fv):
    return np.bincount(rules[:, 2], minlength=fv)


def assert_exact_precondition(rules, fv, amax=4):
    """operands are integers of magnitude <= amax: every partial sum of an offset's products, in any order and grouping,
    is an integer below 2^24 and so exact in fp32 while amax^2 * rules_of_offset < 2^24"""
    most = int(rules_per_offset(rules, fv).max()) if len(rules) else 0
    assert amax * amax * most < 2 ** 24, f"{most} rules at one offset: sums of products up to {amax * amax} are not exact in fp32"
    return most


def gamma(n):
    return n * U32 / (1 - n * U32)


def expect_dw(family, cw, cin, cout, K, n_blk, det, scratch=NONE):
    """the form of one dW launch.  cw: CP (fp32: the padded class of cin) or CS (bf16: the stored width)"""
    assert cw in (CPS if family == F32 else CSS) and cin <= cw and cout in COUTS
    T = max(cw // 32, 1) * (cout // 32)
    tpg = min(T, 16)
    nz = -(-T // tpg)
    f = dict(family=family, cw=cw, cout=cout, cin=cin, T=T, nz=nz, n_blk=n_blk, K=K)
    if det:
        run = BLOCKS_PER_WG
        n_runs = -(-n_blk // run)
        n = K * cin * cout
        G = min(min(n_runs, DET_PARTIALS), max(1, DET_BUDGET // (4 * n)))
        assert scratch in (CALLER, LANE, ASYNC)
        f.update(run=run, chunk=run, n_chunks=1, gx=G, gy=K, gz=nz, det=1, G=G, scratch=scratch)
        return f
    run = -(-n_blk * K * nz // TARGET_WGS)
    if run >= BLOCKS_PER_WG:
        run, chunk = BLOCKS_PER_WG, MAX_CHUNK
    else:
        run = max(2, run)
        chunk = run
    n_chunks = -(-run // chunk)
    f.update(run=run, chunk=chunk, n_chunks=n_chunks, gx=-(-n_blk // run), gy=K, gz=nz * n_chunks, det=0, G=0, scratch=NONE)
    return f


def cp_of(cin):
    return next(c for c in CPS if cin <= c)
