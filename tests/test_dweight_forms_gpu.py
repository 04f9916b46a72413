"""Every launch form of the dWeight dispatcher (conv_dw.hip launch_dw_with) against an fp64 result of the same sum.

Reference: fp64 numpy on the rulebooks of the CPU oracle (tests.dweight_forms.dw64: dW[k] = x[in_k]^T gout[out_k] and
a[k] = |x|^T |gout|; checked against oracle.rule_conv_backward in test_dweight_forms_cpu.py).  Two checks per case:

- exact arithmetic: integer operands in [-4, 4].  Every partial sum of an offset's products is an integer below 2^24
  while 16 * rules_of_offset < 2^24 (asserted), so the fp32 dW of the atomic and of the fixed-order form equals the fp64
  result bit for bit, whatever the grouping into blocks, runs, chunks and partials; bf16 rows hold the same integers
  and dW is fp32, so it is exact too.  A block skipped or taken twice, a tile written to another tile's place, a
  partial left out or a row ci >= cin written moves an element by an integer and fails in that element, however small
  it is next to the layer's largest.
- rounding: normal data; per element |got - want| <= gamma_n a with n = the most rules of an offset + 1; bf16 against
  the products of the bf16-rounded operands.  Where `teeth` is set, one rule taken out of the reference must break the
  bound in some element of its offset.  In the fixed-order form two launches must give the same bits.

dW always lies inside a larger buffer with sentinel values on both sides, which must survive every launch.  The form a
launch ran is read back with d3d_conv_dw_last_form and compared, field by field, with tests.dweight_forms.expect_dw,
which restates the dispatcher's arithmetic from n_blk, K, Cin and Cout.

======================================================  =======================================================
form                                                    tests
======================================================  =======================================================
k_conv_dw<CP, COUT, DET>, k_conv_dw_bf16<CS, COUT,      test_every_class (every CP / CS x COUT, atomic and fixed
DET>: T 1 .. 64, tiles per wave 1 / 2 / 4, waves        order, run < 64, one chunk; CS 16 stores Cin 9)
without a tile, nz 1 / 2 / 4
vec == false (Cin no multiple of the class)             test_unpadded_cin (9 / 20 / 48 / 100 / 200)
K 27 / 1 / 8 / 8 (deconvolution plan) / 32 (bit 31 of   test_every_operation
blkmask, blockIdx.y 31)
one block, one run of 64 exactly, a ragged second run   test_row_structure (n_runs 1 / 1 / 2 in fixed order)
run 64, chunk 8, 8 chunks (blockIdx.z / nz > 0)         test_chunked_atomic (256 x 256 at 607 blocks, all 27
                                                        offsets dense; 64 x 64 at 2428 blocks of isolated sites)
G = n_runs < 32; G = 32 < n_runs (a workgroup walks     test_row_structure, test_fixed_order_partials (64 x 64
several runs); G = 9 by the 64 MB budget; zero          at 2049 blocks; 256 x 256 at 607 blocks; isolated sites:
partials; the caller's buffer / the feature lane / a    26 offsets without a rule), test_small_arena_takes_a_
stream-ordered allocation                               stream_ordered_buffer
dW is added to; a plan without rows launches nothing    test_accumulates_into_dw, test_empty_plan
======================================================  =======================================================

test_zz_coverage asserts that the forms the tests above assert contain every (family, CP / CS, COUT, DET)
instantiation, n_chunks > 1, the three kinds of G, the three scratch paths and K 1 / 8 / 27 / 32; it runs whichever of
them this process has not run yet.  Every test that sets a switch restores it in `finally`.

The costly reference is the one of 256 x 256 at 19424 sites: 27 fp64 products [256 x n_k] [n_k x 256] -- numpy, 0.8 s
for the integer data on 8 CPUs (1.0 s with |x|^T |gout| for the normal data), computed once per kind of data and shared
by the tests; the tests that use it take under a second each on the GPU machine's 16 CPUs."""
import contextlib
import ctypes
import zlib

import numpy as np
import pytest
import torch

from tests.dweight_forms import (ASYNC, BF16, CALLER, COUTS, CPS, CSS, DW_FIELDS, F32, LANE, NONE, assert_exact_precondition,
                                 cp_of, dw64, expect_dw, gamma, rules_per_offset)
from tests.test_conv_forms_gpu import (DOWN, N_MAIN, OPS, PROJ, SUB1, SUB3, UP, Scene, _ints, _isolated_coords,  # noqa: F401
                                       _structured_coords, _to_dev, bf16, check_exact, f32, scene)

pytestmark = pytest.mark.gpu

SENTINEL = 12345.5
PAD = 256                 # floats of sentinel on either side of dW
SEEN = []                 # every form a test asserted
_RAN = set()              # case groups this process has run (test_zz_coverage runs the others)
ATOMIC, FLAG, SWITCH = "atomic", "flag", "switch"   # fp32 atomics / torch.use_deterministic_algorithms / d3d_conv_dw_deterministic
SCRATCH_OF = {ATOMIC: NONE, FLAG: CALLER, SWITCH: LANE}


def _lib():
    from detection_3d_amd._lib import lib
    return lib()


def dw_last_form():
    buf = (ctypes.c_int * len(DW_FIELDS))()
    n = _lib().d3d_conv_dw_last_form(buf, len(DW_FIELDS))
    assert n == len(DW_FIELDS)
    return dict(zip(DW_FIELDS, list(buf)))


@contextlib.contextmanager
def dw_mode(mode):
    """the accumulation form for the block: both switches set, both restored"""
    was_flag = torch.are_deterministic_algorithms_enabled()
    was_switch = _lib().d3d_conv_dw_deterministic(-1)
    try:
        torch.use_deterministic_algorithms(mode == FLAG)
        _lib().d3d_conv_dw_deterministic(1 if mode == SWITCH else 0)
        yield
    finally:
        torch.use_deterministic_algorithms(was_flag)
        _lib().d3d_conv_dw_deterministic(was_switch)


# ---------------------------------------------------------------------------------------------------------- scenes
def _compact_coords(n, seed, size=(64, 64, 32)):
    """n distinct sites drawn from a box that they fill to about 40 % (more where the box meets `size`): every one of
    the 27 offsets has rules in nearly every row block"""
    side = max(2, int(np.ceil((n * 2.5) ** (1 / 3))))
    box = [min(side, s) for s in size]
    assert n <= np.prod(box)
    cells = np.random.RandomState(seed).permutation(int(np.prod(box)))[:n]
    return np.stack([cells // (box[1] * box[2]), (cells // box[2]) % box[1], cells % box[2]], 1).astype(np.int64), size


_COMPACT = {}
N_CHUNKED = 32 * 607      # 256 x 256: 607 blocks x 27 offsets x 4 tile groups >= 64 * 1024 -> run 64, chunks of 8
N_CHUNKED_64 = 32 * 2428  # 64 x 64: 2428 x 27 x 1 >= 64 * 1024
N_WALK = 32 * 2048 + 1    # 2049 blocks: 33 runs of 64 for 32 partials; the last run has one block with one row


def compact_scene(dev, n):
    if n not in _COMPACT:
        if len(_COMPACT) > 2:
            _COMPACT.clear()
        _COMPACT[n] = Scene(dev, *_compact_coords(n, seed=n))
    sc = _COMPACT[n]
    sc.tag = ("compact", n)
    return sc


def tagged(dev, kind, n):
    sc = scene(dev, kind, n)
    sc.tag = (kind, n)
    return sc


# ------------------------------------------------------------------------------------------------- data, reference
_DATA = {}


def case_data(sc, op, cols, cin, cout, flavour):
    """(x [n_in, cols], gout [n_out, cout], want, a) of a layer on a scene; flavour 'int' (integers, shared by both
    families; a is None), 'f32' or 'bf16' (normal data rounded to that type).  Columns cin .. cols-1 of x (bf16 rows
    stored wider than Cin) carry data too: dW has no such rows.  Computed once."""
    key = (sc.tag, op, cols, cin, cout, flavour)
    if key not in _DATA:
        g = sc.geometry(op)
        rng = np.random.RandomState(zlib.crc32(repr((op, cols, cout, flavour)).encode()))
        if flavour == "int":
            x, gout = _ints(rng, (g.n_in, cols)), _ints(rng, (g.n_out, cout))
        else:
            rnd = bf16 if flavour == "bf16" else f32
            x, gout = rnd(rng.randn(g.n_in, cols)), rnd(rng.randn(g.n_out, cout))
        want, a = dw64(x[:, :cin], gout, g.rules, g.fv, with_abs=flavour != "int")
        if len(_DATA) > 24:
            _DATA.clear()
        _DATA[key] = (x, gout, want, a)
    return _DATA[key]


# --------------------------------------------------------------------------------------------------------- launch
def launch_dw(sc, op, x, gout, cin, cout, prefill=None):
    """dW of `op` through the library's backward entry point (no dInput) -> (dW [fv, cin, cout] fp32, recorded form).
    dW lies between two sentinel pads, which must come back untouched."""
    from detection_3d_amd.sparseconvnet import SCN
    g = sc.geometry(op)
    n = g.fv * cin * cout
    buf = torch.full((PAD + n + PAD,), SENTINEL, device=x.device)
    d_w = buf[PAD:PAD + n].view(g.fv, 1, cin, cout)
    if prefill is None:
        d_w.zero_()
    else:
        d_w.copy_(prefill.view(g.fv, 1, cin, cout))
    w4 = torch.zeros((g.fv, 1, cin, cout), device=x.device)
    d_in = x.new_empty(0)
    dw_last_form()
    if op in (SUB3, SUB1):
        SCN.SubmanifoldConvolution_backward(g.in_size, g.filt, sc.m, x, d_in, gout, w4, d_w, None, want_d_input=False)
    elif op in (DOWN, PROJ):
        SCN.Convolution_backward(g.in_size, g.out_size, g.filt, g.stride, sc.m, x, d_in, gout, w4, d_w, None,
                                 want_d_input=False)
    else:
        SCN.Deconvolution_backward(g.in_size, g.out_size, g.filt, g.stride, sc.m, x, d_in, gout, w4, d_w, None,
                                   want_d_input=False)
    form = dw_last_form()
    torch.cuda.synchronize()
    return buf, form


def _split(buf, fv, cin, cout):
    n = fv * cin * cout
    pads = torch.cat([buf[:PAD], buf[PAD + n:]])
    assert bool((pads == SENTINEL).all()), "a launch wrote outside dW"
    return buf[PAD:PAD + n].view(fv, cin, cout)


def run_dw(sc, op, kind, cin, cout, mode, cs=None, rounding=True, teeth=False, scratch=None, prefill=False):
    """exact-arithmetic and rounding check of one dW launch form; -> the recorded form"""
    g = sc.geometry(op)
    fam = F32 if kind == "f32" else BF16
    cols = cin if kind == "f32" else (cs or cin)
    cw = cp_of(cin) if kind == "f32" else cols
    n_blk = -(-g.n_out // 32)
    det = mode != ATOMIC
    want_form = expect_dw(fam, cw, cin, cout, g.fv, n_blk, det, scratch if scratch is not None else SCRATCH_OF[mode])
    counts = rules_per_offset(g.rules, g.fv)
    assert_exact_precondition(g.rules, g.fv, amax=4)
    form = None
    for exact in (True, False) if rounding else (True,):
        x, gout, want, a = case_data(sc, op, cols, cin, cout, "int" if exact else kind)
        xd, gd = _to_dev(x, sc.dev, kind), _to_dev(gout, sc.dev, kind)
        pre = None
        if prefill and exact:
            pre_np = _ints(np.random.RandomState(5), want.shape, -8, 8)
            pre, want = torch.from_numpy(pre_np.astype(np.float32)).to(sc.dev), want + pre_np
        with dw_mode(mode):
            buf, form = launch_dw(sc, op, xd, gd, cin, cout, prefill=pre)
            again = launch_dw(sc, op, xd, gd, cin, cout, prefill=pre)[0] if (det and not exact) else None
        assert form == want_form, (form, want_form)
        d_w = _split(buf, g.fv, cin, cout)
        if exact:
            check_exact(d_w, want, "f32")
            continue
        if again is not None:
            assert torch.equal(buf, again), "the fixed-order form gave other bits in a second launch"
        got = d_w.double().cpu().numpy()
        gam = gamma(int(counts.max()) + 1)
        assert np.isfinite(got).all()
        assert (np.abs(got - want) <= gam * a + 1e-300).all(), float((np.abs(got - want) - gam * a).max())
        if teeth:   # the reference without one rule: its offset must miss the bound somewhere
            for j in (0, len(g.rules) // 2, len(g.rules) - 1):
                i, o, k = g.rules[j]
                w2 = want[k] - np.outer(x[i, :cin], gout[o])
                a2 = a[k] - np.outer(np.abs(x[i, :cin]), np.abs(gout[o]))
                assert (np.abs(got[k] - w2) > gam * a2).any(), (j, k)
    SEEN.append(form)
    return form


def _once(fn, *args):
    key = (fn.__name__,) + args
    if key not in _RAN:
        fn(*args)
        _RAN.add(key)


# ---------------------------------------------------------------------------------------- 1. every class, small plan
CLASSES = [("f32", c, co) for c in CPS for co in COUTS] + [("bf16", c, co) for c in CSS for co in COUTS]


def _every_class(dev, kind, cw, cout):
    sc = tagged(dev, "mixed", N_MAIN)
    cin = 9 if cw == 16 else cw
    for mode in (ATOMIC, FLAG):
        f = run_dw(sc, SUB3, kind, cin, cout, mode, cs=cw, teeth=(cw, cout) in ((64, 64), (16, 32), (256, 256)))
        assert f["run"] == (64 if f["det"] else 5 if f["T"] == 64 else 3 if f["T"] == 32 else 2)
        assert f["n_chunks"] == 1 and f["n_blk"] == 41 and f["G"] == f["det"]


@pytest.mark.parametrize("kind,cw,cout", CLASSES)
def test_every_class(dev, kind, cw, cout):
    """every instantiation on 41 row blocks (the last with one row), submanifold 3^3: atomic with run 2 (3 at T = 32, 5
    at T = 64) and fixed order with one partial"""
    _once(_every_class, dev, kind, cw, cout)


# ------------------------------------------------------------------------------------------------- 2. unpadded Cin
@pytest.mark.parametrize("cin", [9, 20, 48, 100, 200])
def test_unpadded_cin(dev, cin):
    """fp32 rows that are no whole number of 16-byte pieces (vec == false), and the ci < cin guard of the stores: the
    sentinel behind dW is where row ci = cin of the last offset would go"""
    sc = tagged(dev, "mixed", N_MAIN)
    for cout in (32, 128):
        for mode in (ATOMIC, SWITCH):
            for op in (SUB3, DOWN):
                f = run_dw(sc, op, "f32", cin, cout, mode, rounding=op == SUB3)
                assert f["cw"] > f["cin"] == cin


# ----------------------------------------------------------------------------------------------- 3. every operation
def _every_operation(dev, kind, op):
    sc = tagged(dev, "mixed", N_MAIN)
    for mode in (ATOMIC, FLAG, SWITCH):
        f = run_dw(sc, op, kind, 64, 64, mode, teeth=True)
        assert f["K"] == {SUB3: 27, SUB1: 1, DOWN: 8, UP: 8, PROJ: 32}[op] == f["gy"]


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_every_operation(dev, kind, op):
    """submanifold 3^3 and 1x1x1 (identity plan), strided 2^3 / 2, its deconvolution (dW over the deconvolution plan) and
    the [1, 1, 32] projection, whose offset 31 is bit 31 of the block masks"""
    _once(_every_operation, dev, kind, op)


# ------------------------------------------------------------------------------------------------ 4. row structure
ROWS = [1, 31, 32, 33, 32 * 64 - 1, 32 * 64, 32 * 64 + 1]


def _row_structure(dev, n):
    sc = compact_scene(dev, n)
    n_runs = -(-(-(-n // 32)) // 64)
    assert n_runs == (2 if n > 32 * 64 else 1)
    for kind in ("f32", "bf16"):
        run_dw(sc, SUB3, kind, 64, 64, ATOMIC)
        for mode in (FLAG, SWITCH):
            f = run_dw(sc, SUB3, kind, 64, 64, mode)
            assert f["G"] == n_runs == f["gx"]


@pytest.mark.parametrize("n", ROWS)
def test_row_structure(dev, n):
    """one row, one block less a row, one block, one block and a row; one run of 64 blocks less a row, exactly, and a
    second run of one block with one row (fixed order: G = n_runs = 1 / 1 / 2)"""
    _once(_row_structure, dev, n)


# ------------------------------------------------------------------------------------------- 5. chunked atomic form
def _chunked(dev, kind, c):
    sc = compact_scene(dev, N_CHUNKED) if c == 256 else tagged(dev, "iso", N_CHUNKED_64)
    g = sc.geometry(SUB3)
    counts = rules_per_offset(g.rules, 27)
    if c == 256:
        assert counts.min() > 32 * 64          # dense: every chunk of every run carries blocks at every offset
    else:
        assert counts[13] == sc.n and counts.sum() == sc.n   # the centre only: 26 offsets' workgroups leave dW alone
    f = run_dw(sc, SUB3, kind, c, c, ATOMIC)
    assert (f["run"], f["chunk"], f["n_chunks"]) == (64, 8, 8) and f["gz"] == 8 * f["nz"] and f["n_chunks"] > 1


@pytest.mark.parametrize("c", [256, 64])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_chunked_atomic(dev, kind, c):
    """run 64 dealt out in 8 chunks of 8 active blocks: 256 x 256 (4 tile groups) on 607 blocks of a compact scene, and
    64 x 64 on 2428 blocks of isolated sites"""
    _once(_chunked, dev, kind, c)


# ------------------------------------------------------------------------------------------ 6. fixed-order partials
PARTIALS = [(64, N_WALK), (256, N_CHUNKED), (64, N_CHUNKED_64)]


def _partials(dev, kind, c, n):
    sc = tagged(dev, "iso", n) if n == N_CHUNKED_64 else compact_scene(dev, n)
    n_runs = -(-(-(-n // 32)) // 64)
    for mode in (FLAG, SWITCH):
        f = run_dw(sc, SUB3, kind, c, c, mode, rounding=mode == FLAG)
        assert f["G"] == (9 if c == 256 else 32) < n_runs and f["scratch"] == SCRATCH_OF[mode]
    if n == N_WALK:
        assert run_dw(sc, SUB3, kind, c, c, ATOMIC, rounding=False)["run"] == 55


@pytest.mark.parametrize("c,n", PARTIALS)
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_fixed_order_partials(dev, kind, c, n):
    """more runs than partials, so that a workgroup walks several: 32 partials for 33 runs (the last of one block) and
    for 38 runs of isolated sites (26 of 27 offsets store zeros), 9 partials for 10 runs where 27 x 256 x 256 floats
    meet the 64 MB budget; in the caller's buffer and in the feature lane"""
    _once(_partials, dev, kind, c, n)


def _small_arena(dev, monkeypatch_setattr):
    from detection_3d_amd.sparseconvnet import SCN
    big = compact_scene(dev, N_CHUNKED)
    monkeypatch_setattr(SCN, "arena_bytes_for", lambda n_points: 96 << 20)
    sc = Scene(dev, *_compact_coords(N_CHUNKED, seed=N_CHUNKED))
    # the same sites; where the rows are the same too, the reference of compact_scene(N_CHUNKED) serves
    sc.tag = big.tag if np.array_equal(sc.loc, big.loc) else ("compact, small arena", N_CHUNKED)
    assert 9 * 27 * 256 * 256 * 4 > (96 << 20) // 3
    for kind in ("f32", "bf16"):
        f = run_dw(sc, SUB3, kind, 256, 256, SWITCH, scratch=ASYNC)
        assert f["G"] == 9 and f["scratch"] == ASYNC
        f = run_dw(sc, SUB3, kind, 256, 256, FLAG, rounding=False)
        assert f["scratch"] == CALLER


def test_small_arena_takes_a_stream_ordered_buffer(dev, monkeypatch):
    """metadata whose feature lane (a third of 96 MB) cannot hold the 9 partials of a 256 x 256 layer (7 MB each): the
    process-wide switch takes a stream-ordered allocation, the torch flag still the caller's buffer"""
    if "small_arena" not in _RAN:
        _small_arena(dev, monkeypatch.setattr)
        _RAN.add("small_arena")


# ------------------------------------------------------------------------------ 7. accumulation contract, empty plan
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_accumulates_into_dw(dev, kind):
    """both forms add to what dW holds: integers in [-8, 8] before the launch, prefill + dW after it"""
    sc = tagged(dev, "mixed", N_MAIN)
    for mode in (ATOMIC, FLAG, SWITCH):
        for op, cin, cout in ((SUB3, 64, 64), (DOWN, 32, 128)):
            run_dw(sc, op, kind, cin, cout, mode, rounding=False, prefill=True)


def test_empty_plan(dev):
    """a scene without points: D3D_OK from the C entry points, no launch recorded, dW and its surroundings untouched"""
    from detection_3d_amd import sparseconvnet as scn
    from detection_3d_amd._lib import ints, ptr, stream_of
    from detection_3d_amd.sparseconvnet.SCN import BF16 as DT_BF16
    size = (64, 64, 32)
    t = scn.InputLayer(3, list(size), mode=4)([torch.zeros((0, 3), dtype=torch.int64), torch.zeros((0, 1), device=dev)])
    assert t.features.shape[0] == 0
    L = _lib()
    for mode in (ATOMIC, SWITCH):
        for filt in ((3, 3, 3), (1, 1, 1)):
            fv = int(np.prod(filt))
            buf = torch.full((PAD + fv * 64 * 64 + PAD,), SENTINEL, device=dev)
            x32, g32 = torch.zeros((0, 64), device=dev), torch.zeros((0, 64), device=dev)
            dw_last_form()
            with dw_mode(mode):
                rc = L.d3d_subm_conv_backward_dt(t.metadata._h, ints(size), ints(filt), ptr(x32), 64, 64, None, 64, ptr(g32),
                                                 None, ctypes.c_void_p(buf.data_ptr() + 4 * PAD), 0, stream_of())
                rc16 = L.d3d_subm_conv_backward_dt(t.metadata._h, ints(size), ints(filt), ptr(x32.bfloat16()), 64, 64, None,
                                                   64, ptr(g32.bfloat16()), None,
                                                   ctypes.c_void_p(buf.data_ptr() + 4 * PAD), DT_BF16, stream_of())
            torch.cuda.synchronize()
            assert rc == 0 and rc16 == 0
            assert dw_last_form()["family"] == 0
            assert bool((buf == SENTINEL).all())


def test_form_record_is_cleared_by_reading(dev):
    sc = tagged(dev, "mixed", N_MAIN)
    x, gout, _, _ = case_data(sc, SUB1, 32, 32, 32, "int")
    with dw_mode(ATOMIC):
        _, form = launch_dw(sc, SUB1, _to_dev(x, dev, "f32"), _to_dev(gout, dev, "f32"), 32, 32)
    assert form["family"] == F32 and form["K"] == 1
    assert dw_last_form() == dict.fromkeys(DW_FIELDS, 0)
    assert _lib().d3d_conv_dw_last_form(None, 0) == len(DW_FIELDS)


# ------------------------------------------------------------------------------------------------------- coverage
def test_zz_coverage(dev, monkeypatch):
    """the asserted forms contain every instantiation and every host-side choice the dispatcher can make (groups of
    cases this process has not run yet are run first)"""
    for kind, cw, cout in CLASSES:
        _once(_every_class, dev, kind, cw, cout)
    for kind in ("f32", "bf16"):
        for op in OPS:
            _once(_every_operation, dev, kind, op)
        for c in (256, 64):
            _once(_chunked, dev, kind, c)
        for c, n in PARTIALS:
            _once(_partials, dev, kind, c, n)
    for n in (33, 32 * 64 + 1):
        _once(_row_structure, dev, n)
    if "small_arena" not in _RAN:
        _small_arena(dev, monkeypatch.setattr)
        _RAN.add("small_arena")
    inst = {(f["family"], f["cw"], f["cout"], f["det"]) for f in SEEN}
    want = {(F32, c, co, d) for c in CPS for co in COUTS for d in (0, 1)}
    want |= {(BF16, c, co, d) for c in CSS for co in COUTS for d in (0, 1)}
    assert want <= inst, sorted(want - inst)
    for fam in (F32, BF16):
        mine = [f for f in SEEN if f["family"] == fam]
        assert any(f["n_chunks"] > 1 and f["nz"] > 1 for f in mine) and any(f["n_chunks"] > 1 and f["nz"] == 1 for f in mine)
        runs = lambda f: -(-f["n_blk"] // 64)
        assert any(f["det"] and 1 < f["G"] == runs(f) < 32 for f in mine)
        assert any(f["det"] and f["G"] == 32 < runs(f) for f in mine)
        assert any(f["det"] and f["G"] == 9 < min(runs(f), 32) for f in mine)
        assert {f["scratch"] for f in mine} == {NONE, CALLER, LANE, ASYNC}
        assert {f["K"] for f in mine} == {1, 8, 27, 32}
        assert {f["nz"] for f in mine} == {1, 2, 4} and {1, 2, 4, 8, 16, 32, 64} <= {f["T"] for f in mine}
