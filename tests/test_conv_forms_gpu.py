"""Every launch form of the sparse convolution dispatchers against an fp64 result of the same operation.

Reference: fp64 numpy on the rulebooks of the CPU oracle (oracle.subm_nbr, oracle.conv_rules, identity for 1x1x1), over
the rows and sites the library reports.  Two checks per case:

- exact arithmetic: integer features and weights in [-4, 4] (and a BatchNorm prologue of small integers and powers of
  two) keep every product and every partial sum exact in fp32 (|sum| <= 16 * 27 * 256 < 2^24), whatever the summation
  order.  fp32 outputs must equal the fp64 result bit for bit, bf16 outputs its single round-to-nearest-even, and the
  column statistics the fused epilogue leaves the fp64 column sums and sums of squares.  bf16x3 outputs stay within
  2^-22 sum |x||w| of it: the rows' integers have a zero lo part, but the packing gives a weight that bf16 holds
  exactly the lo part hi * 2^-24 (conv_bf16.hip split_weight_x3, kept so that an Inf row never meets a zero weight
  plane), i.e. 2^-24 of every product.  A wrong row mapping, a dropped or doubled offset or a lost channel moves a
  result by at least 1/16 and fails this in any row, however small the row's values are next to the map's largest.
- rounding: normal data; per element |got - y| <= gamma_n sum |x||w| (n = fv Cin + 2 terms: products, residual,
  u = 2^-24); bf16 storage against the fp64 products of the bf16-rounded operands plus one bf16 output rounding;
  bf16x3 the HARD bound of test_conv_precision_gpu.py.  And max |err| / ||x o w||_2 <= TAU, which one product taken
  out of the reference breaks (asserted in every case).

The form a launch ran is read back with d3d_conv_last_form and asserted in every case; the geometry is forced with
d3d_conv_split_mode (1 never split, 2 split wherever the form allows), or left automatic at its threshold.

Forms the dispatchers can select (conv.hip launch_conv / launch_c / launch_t, conv_ws.hip launch_conv_ws,
conv_bf16.hip launch_conv_bf16 / launch_cb / launch_tb / conv_x3_serves) and the tests that reach them:

======================================================  =======================================================
form                                                    tests
======================================================  =======================================================
k_conv<CT,1,COUT,1,BPW,true,LATE> CT 16 / 32 / 64 /    test_fp32_forms[cin-cout-split-late] (every padded Cin
128, k_conv<128,2,..> (Cin 256); COUT 32 (BPW 4, never  and Cout, LATE on / off -- LATE is never taken at CT
split) / 64 / 128 / 256 (BPW 1); unsplit, and           16), test_row_structure, test_fp32_auto_threshold,
offset-split + k_conv_reduce (+ column statistics)      test_stages, test_dinput_exact
k_conv<..., VEC = false, LATE = false>                  test_fp32_unpadded_cin (Cin 9 / 20 / 48 / 100 / 200)
dWeight, atomic and fixed-order (conv_dw.hip)           test_dweight; every launch form of it in
                                                        test_dweight_forms_gpu.py (d3d_conv_dw_last_form)
k_conv_ws<64,64,64,4>, k_conv_ws<128,128,32,4>          test_fp32_ws (d3d_conv_ws_mode 2, unsplit only: the
                                                        split form never takes it)
k_conv_bf16<CT,NCT,COUT,BPW,RB> RB 1 / 2 / 4            test_bf16_forms[cin-cout-rb-split] (RB 4 falls back to
(RB 2 at Cout 256, RB 4 at Cout 64 / 128) unsplit       2 at Cout 256; Cout 32 is always RB 1, BPW 4),
and split + k_conv_reduce_bf16                          test_row_structure, test_bf16_auto_threshold,
                                                        test_stages, test_dinput_exact
k_conv_bf16<..., float> (bf16x3) RB 1 / 2, unsplit      test_x3_forms (every class conv_x3_serves accepts, and
and split + k_conv_reduce                               the classes it declines run k_conv), test_stages,
                                                        test_bf16_auto_threshold[x3], test_dinput_exact
======================================================  =======================================================

Every forward and dInput launch is asserted through d3d_conv_last_form (family, CT, NCT, COUT, BPW, RB, VEC, LATE,
n_split, statistics, row blocks, filter volume).
Not reached: the unsplit fallback of a split launch whose partial sums do not fit the feature arena (it takes GiBs of
partials; d3d_conv_last_form would report it as n_split 1), and the 4 GiB gather-offset limit (D3D_REQUIRE).  Every
test that changes a mode restores it in `finally`."""
import contextlib
import ctypes
import itertools

import numpy as np
import pytest
import torch

import oracle
from tests.helpers import nbr_to_rules, precision

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
U16 = 2.0 ** -8          # bf16: 8 significant bits, round to nearest even
HARD_X3 = 2.5e-4         # test_conv_precision_gpu.py
TAU = {"f32": 1e-4, "bf16": 1e-4, "x3": 1e-3}
FIELDS = ("family", "ct", "nct", "cout", "bpw", "rb", "vec", "late", "n_split", "stats", "n_blk", "K")
CONV, WS, BF16, X3 = 1, 2, 3, 4
SUB3, SUB1, DOWN, UP, PROJ = "subm3", "subm1", "down2", "up2", "proj32"
OPS = (SUB3, SUB1, DOWN, UP, PROJ)
SPLIT_TARGET = 4096      # kSplitTargetWaves / kSplitTargetWavesB
CINS = (16, 32, 64, 128, 256)
COUTS = (32, 64, 128, 256)


def _lib():
    from detection_3d_amd._lib import lib
    return lib()


def last_form():
    buf = (ctypes.c_int * len(FIELDS))()
    n = _lib().d3d_conv_last_form(buf, len(FIELDS))
    assert n == len(FIELDS)
    return dict(zip(FIELDS, list(buf)))


@contextlib.contextmanager
def modes(split=None, late=None, ws=None, rb=None, rb_min_waves=0):
    """the dispatch switches for the block, restored afterwards"""
    from detection_3d_amd._lib import check
    L = _lib()
    was = L.d3d_conv_split_mode(-1), L.d3d_conv_late_mode(-1), L.d3d_conv_ws_mode(-1)
    try:
        if split is not None:
            L.d3d_conv_split_mode(split)
        if late is not None:
            L.d3d_conv_late_mode(late)
        if ws is not None:
            L.d3d_conv_ws_mode(ws)
        if rb is not None:
            check(L.d3d_conv_bf16_tuning(rb, rb_min_waves))
        yield
    finally:
        L.d3d_conv_split_mode(was[0])
        L.d3d_conv_late_mode(was[1])
        L.d3d_conv_ws_mode(was[2])
        if rb is not None:
            check(L.d3d_conv_bf16_tuning(2, -1))


# ---------------------------------------------------------------------------------------------------------- scenes
def _structured_coords(n, seed, size=(64, 64, 32)):
    """n unique sites in `size`: a dense 6^3 block (rows with all 27 offsets), 2x2x2 cubes (corners with exactly 8),
    2x2 squares (4), 3-site lines (2-3), and isolated sites (1) up to n.  Structures sit in their own 8^3 cells, two
    voxels or more apart, so no two of them touch."""
    rng = np.random.RandomState(seed)
    cells = [np.array(c) for c in itertools.product(*(range(0, s, 8) for s in size))]
    order = rng.permutation(len(cells))
    cells = [cells[i] for i in order]
    pts = [cells[0] + d for d in itertools.product(range(6), repeat=3)]
    for c in cells[1:6]:                                       # 40 cubes of 2^3
        for o in itertools.product((0, 4), repeat=3):
            pts += [c + np.array(o) + d for d in itertools.product((0, 1), repeat=3)]
    for c in cells[6:8]:                                       # 16 squares of 2^2 (in x, y)
        for o in itertools.product((0, 4), repeat=3):
            pts += [c + np.array(o) + (i, j, 0) for i in (0, 1) for j in (0, 1)]
    for o in itertools.product((0, 4), (0, 2, 4, 6), (0, 2, 4, 6)):   # 32 lines of 3 along x
        pts += [cells[8] + np.array(o) + (i, 0, 0) for i in range(3)]
    assert len(pts) <= n
    taken = {tuple(p) for p in pts}
    free = cells[9:]
    while len(pts) < n:         # isolated: no site within Chebyshev distance 1, any parity
        c = free[rng.randint(len(free))] + rng.randint(0, 8, 3)
        if any((c[0] + a, c[1] + b, c[2] + d) in taken for a, b, d in itertools.product((-1, 0, 1), repeat=3)):
            continue
        taken.add(tuple(c))
        pts.append(c)
    return np.array(pts, np.int64), size


def _isolated_coords(n, size=(512, 256, 32)):
    """n isolated sites (one active offset each) on the even points of `size`"""
    g = np.stack(np.meshgrid(*(np.arange(0, s, 2) for s in size), indexing="ij"), -1).reshape(-1, 3)
    assert n <= len(g)
    return g[:n].astype(np.int64), size


def _match_rows(got_loc, want_loc):
    """index into want_loc of every row of got_loc (both the same set of sites)"""
    def key(a):
        a = np.asarray(a, np.int64)
        return ((a[:, 3] * 8192 + a[:, 0]) * 8192 + a[:, 1]) * 8192 + a[:, 2]
    kg, kw = key(got_loc), key(want_loc)
    assert kg.size == kw.size
    ow = np.argsort(kw)
    idx = ow[np.clip(np.searchsorted(kw[ow], kg), 0, kw.size - 1)]
    assert (kw[idx] == kg).all()
    return idx


class Geometry:
    def __init__(self, in_size, out_size, filt, stride, rules, n_in, n_out):
        self.in_size, self.out_size, self.filt, self.stride = in_size, out_size, filt, stride
        self.rules, self.n_in, self.n_out = rules, n_in, n_out
        self.fv = int(np.prod(filt))


class Scene:
    """an input layer over `coords` and the rulebooks of every operation, in the rows the library uses"""

    def __init__(self, dev, coords, size):
        from detection_3d_amd import sparseconvnet as scn
        self.dev, self.size = dev, tuple(size)
        self.t = scn.InputLayer(3, list(size), mode=4)([torch.from_numpy(coords), torch.zeros(len(coords), 1, device=dev)])
        self.m = self.t.metadata
        self.loc = self.m.getSpatialLocations(self.size).cpu().numpy()
        self.n = self.loc.shape[0]
        assert self.n == len(coords)
        self._geo = {}

    def _strided(self, filt, stride):
        from detection_3d_amd.sparseconvnet import SCN
        out_size = tuple((s - f) // st + 1 for s, f, st in zip(self.size, filt, stride))
        SCN.Convolution_prepare(self.size, out_size, tuple(filt), tuple(stride), self.m)
        got_lo = self.m.getSpatialLocations(out_size).cpu().numpy()
        lo, ru = oracle.conv_rules(self.loc, list(filt), list(stride), list(out_size))
        inv = np.empty(lo.shape[0], np.int64)
        inv[_match_rows(got_lo, lo)] = np.arange(lo.shape[0])
        ru = ru.astype(np.int64)
        ru[:, 1] = inv[ru[:, 1]]
        return out_size, ru, lo.shape[0]

    def geometry(self, op):
        g = self._geo.get(op)
        if g is not None:
            return g
        if op == SUB3:
            nbr, _ = oracle.subm_nbr(self.loc, [3, 3, 3])
            g = Geometry(self.size, self.size, (3, 3, 3), None, nbr_to_rules(nbr).astype(np.int64), self.n, self.n)
        elif op == SUB1:
            r = np.arange(self.n)
            g = Geometry(self.size, self.size, (1, 1, 1), None, np.stack([r, r, 0 * r], 1), self.n, self.n)
        elif op == DOWN:
            out_size, ru, n_out = self._strided((2, 2, 2), (2, 2, 2))
            g = Geometry(self.size, out_size, (2, 2, 2), (2, 2, 2), ru, self.n, n_out)
        elif op == UP:
            d = self.geometry(DOWN)
            g = Geometry(d.out_size, self.size, (2, 2, 2), (2, 2, 2), d.rules[:, [1, 0, 2]], d.n_out, self.n)
        elif op == PROJ:
            z = self.size[2]
            out_size, ru, n_out = self._strided((1, 1, z), (1, 1, 1))
            g = Geometry(self.size, out_size, (1, 1, z), (1, 1, 1), ru, self.n, n_out)
        self._geo[op] = g
        return g


_SCENES = {}


def scene(dev, kind, n):
    key = (kind, n)
    if key not in _SCENES:
        coords, size = _structured_coords(n, seed=n) if kind == "mixed" else _isolated_coords(n)
        if len(_SCENES) > 6:
            _SCENES.clear()
        _SCENES[key] = Scene(dev, coords, size)
    return _SCENES[key]


N_MAIN = 32 * 40 + 1     # 41 row blocks, the last one with a single row: odd for RB 2 / 4 and BPW 4


# ------------------------------------------------------------------------------------------------------- launches
def launch(sc, op, x, w, residual=None, bn=None, stats=False):
    """one convolution of `op` over x (device rows of the op's input) with w [fv, Cin, Cout] (fp32, device) ->
    (output rows, fp64 [2 Cout] column sums / sums of squares from the fused epilogue or None, form)"""
    from detection_3d_amd.sparseconvnet import SCN
    g = sc.geometry(op)
    w4 = w.reshape(g.fv, 1, w.shape[1], w.shape[2]).contiguous()
    out = x.new_empty(0)
    st = [] if stats else None
    last_form()
    if op in (SUB3, SUB1):
        SCN.SubmanifoldConvolution_updateOutput(g.in_size, g.filt, sc.m, x, out, w4, None, residual=residual, bn=bn,
                                                stats=st)
    elif op in (DOWN, PROJ):
        assert residual is None
        SCN.Convolution_updateOutput(g.in_size, g.out_size, g.filt, g.stride, sc.m, x, out, w4, None, bn=bn, stats=st)
    else:
        SCN.Deconvolution_updateOutput(g.in_size, g.out_size, g.filt, g.stride, sc.m, x, out, w4, None,
                                       residual=residual, bn=bn, stats=st)
    form = last_form()
    col = None
    if stats and st and st[1].value > 0:
        col = st[0][: st[1].value].sum(0).cpu().numpy()
    torch.cuda.synchronize()
    return out, col, form


def conv64(x, w, rules, n_out):
    """fp64 y = sum over rules (in, out, k) of x[in] @ w[k], and sum |x||w|, ||x o w||_2"""
    y, a, s2 = (np.zeros((n_out, w.shape[2])) for _ in range(3))
    for k in range(w.shape[0]):
        sel = rules[:, 2] == k
        i, o = rules[sel, 0], rules[sel, 1]
        assert np.unique(o).size == o.size
        y[o] += x[i] @ w[k]
        a[o] += np.abs(x[i]) @ np.abs(w[k])
        s2[o] += (x[i] ** 2) @ (w[k] ** 2)
    return y, a, np.sqrt(s2)


def bf16(a):
    """fp64 array -> its values rounded to bf16 (to nearest even; exact through fp32 for the magnitudes here)"""
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).double().numpy()


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ expected forms
def _cp(cin):
    return next(c for c in CINS if cin <= c)


def _n_split(split, allowed, K, waves):
    if not allowed or K <= 1 or split == 1:
        return 1
    n = min(K, -(-SPLIT_TARGET // waves))
    return max(n, 2) if split == 2 else (n if waves < SPLIT_TARGET else 1)


def expect_f32(cin, cout, fv, n_blk, split, late=True, ws=0):
    cp = _cp(cin)
    ct, nct = (cp, 1) if cp <= 128 else (128, 2)
    bpw = 4 if cout == 32 else 1
    n_split = _n_split(split, bpw == 1, fv, n_blk * (cout // 32))
    vec = cin == cp
    if ws and vec and n_split == 1 and fv > 1 and (cin, cout) in ((64, 64), (128, 128)) and (ws == 2 or n_blk >= 2048):
        ct, nct = (64, 1) if cin == 64 else (32, 4)
        return dict(family=WS, ct=ct, nct=nct, cout=cout, bpw=4, rb=1, vec=1, late=0, n_split=1)
    return dict(family=CONV, ct=ct, nct=nct, cout=cout, bpw=bpw, rb=1, vec=int(vec), late=int(vec and late and ct >= 32),
                n_split=n_split)


def expect_bf16(cin, cout, fv, n_blk, split, rb, x3=False, rb_min_waves=0):
    ct, nct = {16: (16, 1), 32: (32, 1), 64: (64, 1), 128: (64, 2) if x3 else (128, 1), 256: (128, 2)}[cin]
    r = min(rb, 2) if x3 else rb
    if r >= 2 and cout >= 64 and n_blk * (cout // 32) >= rb_min_waves * r:
        r = 4 if (r == 4 and cout in (64, 128)) else 2
    else:
        r = 1
    bpw = 4 if cout == 32 else 1
    waves = -(-n_blk // r) * (cout // 32)
    return dict(family=X3 if x3 else BF16, ct=ct, nct=nct, cout=cout, bpw=bpw, rb=r, vec=1, late=0,
                n_split=_n_split(split, bpw == 1, fv, waves))


def x3_serves(fv, cin, cout):
    return cin in (32, 64, 128, 256) and cout in (32, 64, 128) and not (fv == 8 and cin >= 128)


def assert_form(form, want, fv, n_blk):
    got = {k: form[k] for k in want}
    assert got == want, (got, want)
    assert form["K"] == fv and form["n_blk"] == n_blk, form


# ----------------------------------------------------------------------------------------------------- checks
def check_exact(got, want, kind, a=None):
    """kind 'f32': fp32 rows equal to the fp64 result; 'bf16': its round to nearest even; 'x3': within 2^-22 sum |x||w|
    (the bf16x3 packing gives a weight that bf16 holds exactly the lo part hi * 2^-24, conv_bf16.hip split_weight_x3,
    so integer data are off by 2^-24 per product -- while a dropped or doubled product moves a result by >= 1/16)"""
    g = got.double().cpu().numpy()
    if kind == "x3":
        err = np.abs(g - want)
        assert (err <= 2.0 ** -22 * a).all(), float(err.max())
        assert float(err.max()) < 1.0 / 64
        return
    w = bf16(want) if kind == "bf16" else want
    bad = np.argwhere(g != w)
    assert bad.size == 0, (f"{len(bad)} of {g.size} differ; first (row, col) {bad[:4].tolist()}: got "
                           f"{g[tuple(bad[0])]} want {w[tuple(bad[0])]}")


def _round_err(g, y, kind):
    """|got - y| less the output rounding bf16 storage allows"""
    err = np.abs(g - y)
    return np.maximum(err - U16 * np.abs(g), 0.0) if kind == "bf16" else err


def check_rounding(got, y, a, norm, n_terms, kind, drop=None):
    """the per-element bound and max |err| / ||x o w|| <= TAU; `drop` = (row, col, product) of one product: taking it
    out of the reference must break TAU"""
    g = got.double().cpu().numpy()
    assert np.isfinite(g).all()
    if kind == "x3":
        bound = HARD_X3 * a
    else:
        gam = n_terms * U32 / (1 - n_terms * U32)
        bound = gam * a if kind == "f32" else gam * a * (1 + U16) + U16 * np.abs(y)
    err = np.abs(g - y)
    assert (err <= bound + 1e-300).all(), float((err - bound).max())
    live = norm > 0
    stat = float((_round_err(g, y, kind)[live] / norm[live]).max())
    assert stat <= TAU[kind], stat
    if drop is not None:
        r, c, p = drop
        y2 = y[r, c] - p
        broken = float(_round_err(g[r, c], y2, kind) / norm[r, c])
        assert broken > TAU[kind], (broken, p, norm[r, c])
    return stat


def largest_product(x, w, rules):
    """(out row, column, value) of the largest single product x[i][ci] w[k][ci][c] of a few rules"""
    best = (0, 0, 0.0)
    for j in np.linspace(0, len(rules) - 1, 7).astype(int):
        i, o, k = rules[j]
        p = x[i][:, None] * w[k]
        ci, c = np.unravel_index(np.argmax(np.abs(p)), p.shape)
        if abs(p[ci, c]) > abs(best[2]):
            best = (o, c, p[ci, c])
    return best


def _ints(rng, shape, lo=-4, hi=4):
    return rng.randint(lo, hi + 1, shape).astype(np.float64)


def _to_dev(a, dev, kind):
    t = torch.from_numpy(np.asarray(a, np.float32)).to(dev)
    return t.to(torch.bfloat16) if kind == "bf16" else t


def run_case(sc, op, cin, cout, kind, want, seed, residual=False, bn=None, stats=False, rounding=True, tf32=False):
    """exact-arithmetic and rounding checks of one operation; want: the form d3d_conv_last_form must report.
    bn: None or the leakiness of a fused BatchNorm prologue (exact data only with 0 or a power of two).  tf32: run under
    torch's TF32 opt-in (always for kind 'x3'; for 'f32' the classes bf16x3 declines)"""
    g = sc.geometry(op)
    rng = np.random.RandomState(seed)
    exact_bn = bn is None or bn in (0.0, 0.25, 0.5)
    with precision("tf32" if (kind == "x3" or tf32) else "ieee"):
        for exact in (True, False) if rounding else (True,):
            x = _ints(rng, (g.n_in, cin)) if exact else rng.randn(g.n_in, cin)
            w = _ints(rng, (g.fv, cin, cout)) if exact else rng.randn(g.fv, cin, cout)
            r = (_ints(rng, (g.n_out, cout), -8, 8) if exact else rng.randn(g.n_out, cout)) if residual else None
            if kind == "bf16":
                x, r = bf16(x), (None if r is None else bf16(r))
            elif not exact:
                x, w, r = f32(x), f32(w), (None if r is None else f32(r))
            bn_dev, z = None, x
            if bn is not None:
                mean = rng.randint(-1, 2, cin).astype(np.float32)
                invstd = rng.choice([0.5, 1.0, 2.0], cin).astype(np.float32)
                gamma = rng.choice([0.5, 1.0], cin).astype(np.float32)
                beta = rng.randint(-1, 2, cin).astype(np.float32)
                bn_dev = tuple(torch.from_numpy(v).to(sc.dev) for v in (mean, invstd, gamma, beta)) + (bn,)
                sc32 = f32(invstd * gamma)
                sh32 = f32(np.float32(-mean * (invstd * gamma)) + beta)
                t = f32(x * sc32 + sh32)                       # fmaf (exact here, or one rounding)
                z = f32(np.where(t > 0, t, f32(t * np.float32(bn))))
                if kind == "bf16":
                    z = bf16(z)
            wk = bf16(w) if kind == "bf16" else w
            y, a, norm = conv64(z, wk, g.rules, g.n_out)
            if r is not None:
                y, a = y + r, a + np.abs(r)
            out, col, form = launch(sc, op, _to_dev(x, sc.dev, kind), torch.from_numpy(np.asarray(w, np.float32)).to(sc.dev),
                                    residual=None if r is None else _to_dev(r, sc.dev, kind), bn=bn_dev, stats=stats)
            assert_form(form, want, g.fv, -(-g.n_out // 32))
            assert out.shape == (g.n_out, cout)
            if exact and exact_bn:
                check_exact(out, y, kind, a)
            else:       # (integer data through leaky(0.333 x) are no longer exact: the bounds instead)
                check_rounding(out, y, a, norm, g.fv * cin + 2, kind, drop=largest_product(z, wk, g.rules))
            if stats:   # the sums of the rows as stored: exact sums of integers, else fp64 sums of the output
                assert form["stats"] == 1 and col is not None
                yy = y if (exact and exact_bn) else out.double().cpu().numpy()
                want_col = np.concatenate([yy.sum(0), (yy * yy).sum(0)])
                if exact and exact_bn:
                    assert np.array_equal(col, want_col), "column statistics"
                else:
                    assert np.allclose(col, want_col, rtol=1e-12, atol=1e-9), "column statistics"


# --------------------------------------------------------------------------------------------------------- fp32
@pytest.mark.parametrize("late", [1, 0])
@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("cin", CINS)
def test_fp32_forms(dev, cin, cout, split, late):
    """k_conv over every padded Cin x Cout, split and unsplit, LATE on and off: submanifold 3^3 and 1x1x1, strided 2^3/2,
    its deconvolution and the [1, 1, 32] projection"""
    sc = scene(dev, "mixed", N_MAIN)
    with modes(split=split, late=late, ws=0):
        for j, op in enumerate(o for o in OPS if o != UP or cin >= 32):
            ci, co = (cout, cin) if op == UP else (cin, cout)
            g = sc.geometry(op)
            run_case(sc, op, ci, co, "f32", expect_f32(ci, co, g.fv, -(-g.n_out // 32), split, late), seed=j)


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("cin", [9, 20, 48, 100, 200])
def test_fp32_unpadded_cin(dev, cin, split):
    """k_conv<..., VEC = false>: rows that are no whole number of 16-byte pieces"""
    sc = scene(dev, "mixed", N_MAIN)
    with modes(split=split):
        for cout in (32, 128):
            for j, op in enumerate((SUB3, SUB1, DOWN, PROJ)):
                g = sc.geometry(op)
                run_case(sc, op, cin, cout, "f32", expect_f32(cin, cout, g.fv, -(-g.n_out // 32), split), seed=j)


@pytest.mark.parametrize("c", [64, 128])
def test_fp32_ws(dev, c):
    """the weight-sharing kernel (d3d_conv_ws_mode 2) on the unsplit geometry; the split one keeps k_conv"""
    sc = scene(dev, "mixed", N_MAIN)
    for split in (1, 2):
        with modes(split=split, ws=2):
            for j, op in enumerate((SUB3, DOWN, UP, PROJ, SUB1)):
                g = sc.geometry(op)
                want = expect_f32(c, c, g.fv, -(-g.n_out // 32), split, ws=2)
                assert want["family"] == (WS if split == 1 and g.fv > 1 else CONV)
                run_case(sc, op, c, c, "f32", want, seed=j, residual=op in (SUB3, UP), stats=True)


# --------------------------------------------------------------------------------------------------------- bf16
@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("rb", [1, 2, 4])
@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("cin", CINS)
def test_bf16_forms(dev, cin, cout, rb, split):
    """k_conv_bf16 over every stored Cin x Cout x RB (forced for every launch size), split and unsplit"""
    sc = scene(dev, "mixed", N_MAIN)
    with modes(split=split, rb=rb):
        for j, op in enumerate(o for o in OPS if o != UP or cin >= 32):
            ci, co = (cout, cin) if op == UP else (cin, cout)
            g = sc.geometry(op)
            run_case(sc, op, ci, co, "bf16", expect_bf16(ci, co, g.fv, -(-g.n_out // 32), split, rb), seed=j,
                     rounding=op in (SUB3, DOWN))


# ---------------------------------------------------------------------------------------------------------- x3
X3_CLASSES = [(cin, cout) for cin in (32, 64, 128, 256) for cout in (32, 64, 128)]


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("rb", [1, 2])
@pytest.mark.parametrize("cin,cout", X3_CLASSES + [(64, 256), (256, 256)])
def test_x3_forms(dev, cin, cout, rb, split):
    """bf16x3 (fp32 rows, torch's TF32 opt-in) over every class conv_x3_serves accepts; the classes it declines
    (Cout 256, 2^3 with Cin >= 128) run k_conv and give the exact result"""
    sc = scene(dev, "mixed", N_MAIN)
    with modes(split=split, rb=rb):
        for j, op in enumerate((SUB3, SUB1, DOWN, PROJ)):
            g = sc.geometry(op)
            nb = -(-g.n_out // 32)
            if x3_serves(g.fv, cin, cout):
                want = expect_bf16(cin, cout, g.fv, nb, split, rb, x3=True)
            else:
                want = expect_f32(cin, cout, g.fv, nb, split)
            run_case(sc, op, cin, cout, "x3" if want["family"] == X3 else "f32", want, seed=j, tf32=True)


# -------------------------------------------------------------------------------------------------------- stages
@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("kind", ["f32", "bf16", "x3"])
@pytest.mark.parametrize("leak", [0.0, 0.25, 0.333])
def test_stages(dev, kind, leak, split):
    """fused BatchNorm prologue (leakiness 0 and a power of two exact, 0.333 within the bounds), residual, and the
    column-statistics epilogue of k_conv, in both geometries"""
    sc = scene(dev, "mixed", N_MAIN)
    with modes(split=split, rb=2):
        for j, (op, cin, cout) in enumerate([(SUB3, 64, 64), (SUB3, 256, 128), (DOWN, 32, 64), (UP, 64, 32),
                                             (PROJ, 128, 128), (SUB1, 128, 64)]):
            g = sc.geometry(op)
            nb = -(-g.n_out // 32)
            k = kind
            if kind == "f32":
                want = expect_f32(cin, cout, g.fv, nb, split)
            elif kind == "bf16":
                want = expect_bf16(cin, cout, g.fv, nb, split, 2)
            elif x3_serves(g.fv, cin, cout):
                want = expect_bf16(cin, cout, g.fv, nb, split, 2, x3=True)
            else:
                want, k = expect_f32(cin, cout, g.fv, nb, split), "f32"
            if k == "bf16" and leak == 0.333:
                continue   # bf16 rows of leaky(0.333 x) are rounded twice; the bounds above do not model that
            run_case(sc, op, cin, cout, k, want, seed=j, residual=op in (SUB3, UP, SUB1), bn=leak,
                     stats=k == "f32", tf32=kind == "x3")


# --------------------------------------------------------------------------------------------------- row structure
@pytest.mark.parametrize("n", [32 * 41 + 1, 32 * 42 - 1, 32 * 43, 32 * 45 - 7])
def test_row_structure(dev, n):
    """row counts = 1, 31, 0 (mod 32) and last RB 2 / 4 groups or BPW 4 workgroups partly empty"""
    sc = scene(dev, "mixed", n)
    nb = -(-n // 32)
    for split in (1, 2):
        with modes(split=split, rb=4):
            for j, cout in enumerate((32, 64, 128)):
                run_case(sc, SUB3, 64, cout, "f32", expect_f32(64, cout, 27, nb, split), seed=j, residual=True,
                         stats=True)
                run_case(sc, SUB3, 32, cout, "bf16", expect_bf16(32, cout, 27, nb, split, 4), seed=j, residual=True)
                run_case(sc, SUB1, 128, cout, "bf16", expect_bf16(128, cout, 1, nb, split, 4), seed=j)
        with modes(split=split, rb=2):
            run_case(sc, SUB3, 64, 64, "bf16", expect_bf16(64, 64, 27, nb, split, 2), seed=5)
            run_case(sc, SUB3, 64, 128, "x3", expect_bf16(64, 128, 27, nb, split, 2, x3=True), seed=6)


# ------------------------------------------------------------------------------------------------ automatic geometry
def _threshold_blocks(cout, rb=1):
    """the smallest row-block count whose launch has SPLIT_TARGET waves (unsplit)"""
    return (-(-SPLIT_TARGET // (cout // 32)) - 1) * rb + 1


@pytest.mark.parametrize("cout", [32, 64, 128, 256])
def test_fp32_auto_threshold(dev, cout):
    """split mode 0: offset-split one row block below the threshold, unsplit at it (Cout 32, BPW 4: never split)"""
    nb_hi = _threshold_blocks(max(cout, 64))
    for nb in (nb_hi - 1, nb_hi):
        sc = scene(dev, "iso", nb * 32)
        want = expect_f32(32, cout, 27, nb, 0)
        assert want["n_split"] == (1 if cout == 32 or nb == nb_hi else want["n_split"])
        assert cout == 32 or (want["n_split"] > 1) == (nb < nb_hi)
        run_case(sc, SUB3, 32, cout, "f32", want, seed=1, rounding=False, stats=True)


@pytest.mark.parametrize("kind", ["bf16", "x3"])
def test_bf16_auto_threshold(dev, kind):
    """split mode 0 and the default row-block tuning: RB 1 below 2 * 8192 waves, split below 4096 waves; RB 2 at
    8192 blocks (Cout 64); with RB 2 forced the split threshold moves to twice the blocks"""
    x3 = kind == "x3"
    cin, cout = 32, 64
    nb_hi = _threshold_blocks(cout)
    default_min = 2 * SPLIT_TARGET
    for nb in (nb_hi - 1, nb_hi, 8191, 8192):
        sc = scene(dev, "iso", nb * 32)
        want = expect_bf16(cin, cout, 27, nb, 0, 2, x3=x3, rb_min_waves=default_min)
        assert want["rb"] == (2 if nb >= 8192 else 1) and (want["n_split"] > 1) == (nb < nb_hi)
        with modes(split=0):
            run_case(sc, SUB3, cin, cout, kind, want, seed=2, rounding=False)
    nb_hi2 = _threshold_blocks(cout, 2)
    for nb in (nb_hi2 - 2, nb_hi2):
        sc = scene(dev, "iso", nb * 32)
        want = expect_bf16(cin, cout, 27, nb, 0, 2, x3=x3)
        assert want["rb"] == 2 and (want["n_split"] > 1) == (nb < nb_hi2)
        with modes(split=0, rb=2):
            run_case(sc, SUB3, cin, cout, kind, want, seed=3, rounding=False)


# ---------------------------------------------------------------------------------------------- dInput, dWeight
def _backward(sc, op, x, w, gout, want_d_input=True):
    from detection_3d_amd.sparseconvnet import SCN
    g = sc.geometry(op)
    w4 = w.reshape(g.fv, 1, w.shape[1], w.shape[2]).contiguous()
    d_in, d_w = x.new_empty(0), torch.zeros_like(w4)
    last_form()
    if op == SUB3:
        SCN.SubmanifoldConvolution_backward(g.in_size, g.filt, sc.m, x, d_in, gout, w4, d_w, None,
                                            want_d_input=want_d_input)
    elif op == DOWN:
        SCN.Convolution_backward(g.in_size, g.out_size, g.filt, g.stride, sc.m, x, d_in, gout, w4, d_w, None,
                                 want_d_input=want_d_input)
    form = last_form()
    torch.cuda.synchronize()
    return d_in, d_w.reshape(w.shape), form


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("kind", ["f32", "bf16", "x3"])
@pytest.mark.parametrize("op", [SUB3, DOWN])
def test_dinput_exact(dev, op, kind, split):
    """dInput = the forward kernel on W^T over the transposed rulebook: exact-arithmetic result and its form"""
    sc = scene(dev, "mixed", N_MAIN)
    g = sc.geometry(op)
    cin, cout = 64, 128
    rng = np.random.RandomState(7)
    x, w, gout = _ints(rng, (g.n_in, cin)), _ints(rng, (g.fv, cin, cout)), _ints(rng, (g.n_out, cout))
    # dX[in] = sum over rules g[out] @ W[k]^T
    want_dx, a, _ = conv64(gout, np.ascontiguousarray(w.transpose(0, 2, 1)), g.rules[:, [1, 0, 2]], g.n_in)
    nb_t = -(-g.n_in // 32)
    fv = g.fv
    with modes(split=split, rb=2), precision("tf32" if kind == "x3" else "ieee"):
        if kind == "f32" or (kind == "x3" and not x3_serves(fv, cout, cin)):
            want = expect_f32(cout, cin, fv, nb_t, split)
        else:
            want = expect_bf16(cout, cin, fv, nb_t, split, 2, x3=kind == "x3")
        d_in, _, form = _backward(sc, op, _to_dev(x, dev, kind), torch.from_numpy(w.astype(np.float32)).to(dev),
                                  _to_dev(gout, dev, kind))
    assert_form(form, want, fv, nb_t)
    check_exact(d_in, want_dx, {CONV: "f32", BF16: "bf16", X3: "x3"}[want["family"]], a)


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("op", [SUB3, DOWN])
def test_dweight(dev, op, kind, deterministic):
    """dWeight in its atomic and its fixed-order form (torch.use_deterministic_algorithms): exact with integer data,
    within gamma_n of fp64 with normal data"""
    sc = scene(dev, "mixed", N_MAIN)
    g = sc.geometry(op)
    cin, cout = 32, 64
    rng = np.random.RandomState(8)
    counts = np.bincount(g.rules[:, 2], minlength=g.fv)
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(deterministic)
    try:
        for exact in (True, False):
            x = _ints(rng, (g.n_in, cin)) if exact else rng.randn(g.n_in, cin)
            gout = _ints(rng, (g.n_out, cout)) if exact else rng.randn(g.n_out, cout)
            x, gout = (bf16(x), bf16(gout)) if kind == "bf16" else (f32(x), f32(gout))
            w = rng.randn(g.fv, cin, cout)
            _, d_w, _ = _backward(sc, op, _to_dev(x, dev, kind), torch.from_numpy(w.astype(np.float32)).to(dev),
                                  _to_dev(gout, dev, kind), want_d_input=False)
            want, a = np.zeros((g.fv, cin, cout)), np.zeros((g.fv, cin, cout))
            for k in range(g.fv):
                sel = g.rules[:, 2] == k
                i, o = g.rules[sel, 0], g.rules[sel, 1]
                want[k] = x[i].T @ gout[o]
                a[k] = np.abs(x[i]).T @ np.abs(gout[o])
            got = d_w.double().cpu().numpy()
            if exact:
                check_exact(d_w, want, "f32")
            else:
                n = int(counts.max()) + 1
                assert (np.abs(got - want) <= n * U32 / (1 - n * U32) * a + 1e-300).all()
    finally:
        torch.use_deterministic_algorithms(was)


def test_split_mode_and_form_record_restore(dev):
    """the switches report and restore their settings; the record is cleared by reading it"""
    L = _lib()
    was = L.d3d_conv_split_mode(-1)
    try:
        assert L.d3d_conv_split_mode(2) == was
        assert L.d3d_conv_split_mode(-1) == 2
        assert L.d3d_conv_split_mode(7) == 2 and L.d3d_conv_split_mode(-1) == 2   # out of range: ignored
    finally:
        L.d3d_conv_split_mode(was)
    last_form()
    assert last_form()["family"] == 0
