"""k_roi_sparse against the fp32 emulation of tests/roi_merge_ref.py, to the bit.

Geometry is the exact class of tests/roi_forms.py (yaw 0, samples on the 1/8-pixel lattice, NS a power of two): every tap
weight and every sum of tap weights is an fp32 number whatever the reduction tree.  The feature values are arbitrary fp32
(or bf16) numbers, so the bits of a result are decided by the order of a bin's list of merged cells and by the order of
the accumulation down the list -- both are pinned here: fp32 rows must equal the emulation bit for bit, bf16 rows its
round-to-nearest-even.

What is not observable here: the SHAPE of the tree that sums a cell's tap weights (levels 32, 16, 8, 4, 2, 1 of the xor
butterfly).  On exact weights every tree gives the same number.  The shape is pinned by construction (roi_cells4_sum in
csrc/roi_forward.hip adds lane i to lane i ^ d at every level) and by the paired comparison of DESIGN.md section 5e: on
seeded cases of arbitrary yaw the pooled tensor is byte-identical to that of the serial butterfly it replaced.

Cases (tests/roi_merge_ref.py; test_roi_merge_cpu.py asserts that they reach what they are named for):
  lengths        merged lists of 0, 1, B - 1, B, B + 1 and 64 cells per bin (B = 8 cells per batch of weight sums), groups
                 such as (0, 64, 1, B + 1) whose batches straddle bins, a full step of 4 x 64 cells
  one cell       all 64 taps in one cell (a box below one pixel, clamped at the far corner); 1 x 1 x 1 bins: a ragged group
  ragged 6x8x3   groups that straddle (ph, pw) cells; PZ = 5: a ragged last group of two bins
  NS = 32        four steps per group, the lists rewritten per step
  store paths    layout 1 with PZ = 4 at C = 128, 130 (second chunk: one channel pair) and 127 (odd C: scalar loads and
                 stores), PZ = 3 and 5, layout 0, a result whose data pointer is not 16-byte (fp32) / 8-byte (bf16)
                 aligned, rows of level -1 left untouched
Every case runs through both lookups (hash table with the caller's crop, dense index with the extent read on the device)
and both layouts."""
import ctypes

import numpy as np
import pytest
import torch

from tests import roi_forms as Rf
from tests import roi_merge_ref as M
from tests.roi_forms import BF16, F32

pytestmark = pytest.mark.gpu

TYPES = [F32, BF16]
_TENSORS = {}


def _ops():
    from detection_3d_amd import roi_align_rotated_3d as ops
    return ops


def _last_form():
    from detection_3d_amd._lib import lib
    buf = (ctypes.c_int * len(Rf.ROI_FIELDS))()
    assert lib().d3d_roi_last_form(buf, len(Rf.ROI_FIELDS)) == len(Rf.ROI_FIELDS)
    return dict(zip(Rf.ROI_FIELDS, list(buf)))


def _tensor(dev, case, typ):
    """the case's map as a SparseConvNetTensor (rows in the grid's order), built once per case and storage type"""
    key = (case["name"], typ)
    if key not in _TENSORS:
        from detection_3d_amd import sparseconvnet as scn
        m = case["map"]
        t = scn.InputLayer(3, case["size"], mode=4)([torch.from_numpy(m.sites.copy()), torch.ones((m.n, 1), device=dev)])
        loc = t.get_spatial_locations().cpu().numpy()
        perm = m.find(loc[:, 3], loc[:, 0], loc[:, 1], loc[:, 2])
        assert loc.shape[0] == m.n and (perm >= 0).all()
        feats = torch.from_numpy(np.ascontiguousarray(np.asarray(m.feats, np.float32)[perm])).to(dev)
        feats = feats.bfloat16() if typ == BF16 else feats          # bf16 cases hold bf16 numbers: no rounding here
        _TENSORS[key] = scn.SparseConvNetTensor(feats, t.metadata, t.spatial_size)
    return _TENSORS[key]


def _want(emulated, typ):
    return Rf.bf16_round(emulated) if typ == BF16 else emulated


def _pool(dev, case, typ, layout1, hashed, out=None, roi_levels=None):
    """-> the pooled tensor as fp32 [K, C, PH, PW, PZ] (and the tensor written)"""
    t = _tensor(dev, case, typ)
    K, C, bins = case["K"], case["C"], case["bins"]
    shape = (K, bins[0], bins[1], C, bins[2]) if layout1 else (K, C) + bins
    if out is None:
        out = torch.full(shape, float("nan"), dtype=t.features.dtype, device=dev)
    _last_form()
    _ops().roi_align_rotated_3d_sparse_into(out, t, torch.from_numpy(case["rois"]).to(dev), case["scale"], case["sr"],
                                            crop=list(case["crop"]) if hashed else None, roi_levels=roi_levels, level=0,
                                            channels_inner=layout1)
    form = _last_form()
    assert form["family"] == Rf.SPARSE and form["lookup"] == (Rf.HASH if hashed else Rf.INDEX), form
    got = out.permute(0, 3, 1, 2, 4) if layout1 else out
    return np.ascontiguousarray(got.detach().float().cpu().numpy()), out


def _check_all_forms(dev, name, typ):
    cs, emu = M.cached(typ == BF16)
    case, want = cs[name], _want(emu[name][0], typ)
    for layout1 in (True, False):
        for hashed in (True, False):
            got, _ = _pool(dev, case, typ, layout1, hashed)
            bad = got.view(np.uint32) != want.view(np.uint32)
            assert not bad.any(), (f"{name}, layout {int(layout1)}, {'hash' if hashed else 'index'}: {bad.sum()} of "
                                   f"{bad.size} elements differ from the emulation, first at {np.argwhere(bad)[0]}")


@pytest.mark.parametrize("typ", TYPES)
@pytest.mark.parametrize("name", ["lengths", "one cell", "ragged 6x8x3", "NS = 32"])
def test_lists(dev, name, typ):
    _check_all_forms(dev, name, typ)


@pytest.mark.parametrize("typ", TYPES)
@pytest.mark.parametrize("name", ["PZ = 4, C = 128", "PZ = 4, C = 130", "PZ = 4, C = 127", "PZ = 3", "PZ = 5"])
def test_store_paths(dev, name, typ):
    _check_all_forms(dev, name, typ)


@pytest.mark.parametrize("typ", TYPES)
@pytest.mark.parametrize("name", ["PZ = 4, C = 128", "PZ = 4, C = 130"])
def test_unaligned_result(dev, name, typ):
    """layout 1, PZ = 4, the result one element past an aligned address: the scalar stores, nothing written outside"""
    cs, emu = M.cached(typ == BF16)
    case, want = cs[name], _want(emu[name][0], typ)
    K, C, bins = case["K"], case["C"], case["bins"]
    shape = (K, bins[0], bins[1], C, bins[2])
    numel = int(np.prod(shape))
    buf = torch.full((numel + 16,), float("nan"), dtype=torch.bfloat16 if typ == BF16 else torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + numel].view(shape)
    assert out.is_contiguous() and out.data_ptr() % (8 if typ == BF16 else 16) != 0
    got, _ = _pool(dev, case, typ, True, False, out=out)
    assert Rf.same_bits(got, want)
    assert torch.isnan(buf[:1]).all() and torch.isnan(buf[1 + numel:]).all()


@pytest.mark.parametrize("typ", TYPES)
@pytest.mark.parametrize("layout1", [True, False])
def test_rows_of_level_minus_one_untouched(dev, layout1, typ):
    cs, emu = M.cached(typ == BF16)
    name = "PZ = 4, C = 128"
    case, want = cs[name], _want(emu[name][0], typ)
    levels = np.zeros(case["K"], np.int32)
    levels[[1, 3]] = -1
    got, out = _pool(dev, case, typ, layout1, False, roi_levels=torch.from_numpy(levels).to(dev))
    keep = levels == 0
    assert Rf.same_bits(got[keep], want[keep])
    assert np.isnan(got[~keep]).all() and torch.isnan(out[torch.from_numpy(~keep).to(dev)]).all()
