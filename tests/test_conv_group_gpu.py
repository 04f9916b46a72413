"""Grouped sparse convolutions (d3d_conv_group_forward, scn.modules.conv_group) against the same convolutions called one
by one: every output, and every column-statistics row a member leaves, must be bit-identical (torch.equal), whatever the
order of the members.

One scene carries every member: sites are drawn inside 33 of the 64 cells of 16^3 voxels of a 64^3 grid, so the pyramid
of 2x2x2 / stride 2 grids has a few thousand sites at level 0, exactly 33 at the 4^3 level (one full 32-row block and one
row of the next) and at most 8 at the 2^3 level (one row block).  A grid without sites exists only in a scene without
points, where every grid is empty: the zero-row member is checked there, in a group of its own."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FIELDS = ("family", "ct", "nct", "cout", "bpw", "rb", "vec", "late", "n_split", "stats", "n_blk", "K")
CAP = 8                     # kGroupCap of conv.hip: members per grouped launch
SIZES = [[64 >> k] * 3 for k in range(6)]      # 64, 32, 16, 8, 4, 2


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _last_form():
    from detection_3d_amd._lib import lib
    buf = (ctypes.c_int * len(FIELDS))()
    lib().d3d_conv_last_form(buf, len(FIELDS))
    return dict(zip(FIELDS, list(buf)))


def _scene(dev, empty=False):
    """-> (metadata, site count per level) with the grids of SIZES built"""
    from detection_3d_amd import sparseconvnet as scn
    rng = np.random.RandomState(5)
    cells = rng.permutation(64)[:33]
    pts = []
    for c in cells:
        base = np.array([c // 16, (c // 4) % 4, c % 4]) * 16
        pts.append(base + rng.randint(0, 16, (110, 3)))
        pts.append(base[None] + [[0, 0, 0], [15, 15, 15]])      # the cell's two 8^3 corner cells: both children exist
    coords = np.unique(np.concatenate(pts), axis=0)
    if empty:
        coords = coords[:0]
    feats = torch.zeros((coords.shape[0], 1), device=dev)
    t = scn.InputLayer(3, SIZES[0], mode=4)([torch.from_numpy(coords.astype(np.int64)), feats])
    md = t.metadata
    counts = [md.getNActive(SIZES[0])]
    for a, b in zip(SIZES[:-1], SIZES[1:]):
        counts.append(scn.SCN.Convolution_prepare(a, b, [2] * 3, [2] * 3, md))
    return md, counts


class _Calls(object):
    """the members: (module, input, residual) triples on one metadata, with seeded weights and rows"""

    def __init__(self, dev, md, counts):
        from detection_3d_amd import sparseconvnet as scn
        from detection_3d_amd.sparseconvnet.modules import SparseConvNetTensor, _PendingBN
        self.dev, self.md, self.counts = dev, md, counts
        g = torch.Generator(device="cpu").manual_seed(17)
        self.g = g

        def rows(level, c):
            return torch.randn((counts[level], c), generator=g).to(dev)

        def tensor(level, c):
            return SparseConvNetTensor(rows(level, c), md, torch.tensor(SIZES[level]))

        def module(cls, *args):
            m = cls(3, *args)
            m.weight.data.copy_(torch.randn(m.weight.shape, generator=g) * 0.1)
            return m.to(dev)

        sub, conv, dec = scn.SubmanifoldConvolution, scn.Convolution, scn.Deconvolution
        bn = (torch.randn(128, generator=g).to(dev), (torch.rand(128, generator=g) + 0.5).to(dev),
              torch.randn(128, generator=g).to(dev), torch.randn(128, generator=g).to(dev), 0.333)
        self.named = {
            # (a) 1x1x1, one row block
            "a": (module(sub, 128, 128, 1, False), tensor(5, 128), None),
            # (b) 3x3x3, 33 rows: crosses the 32-row block edge
            "b": (module(sub, 128, 128, 3, False), tensor(4, 128), None),
            # (c) 3x3x3 with few rows: offset-split, with a residual
            "c": (module(sub, 128, 128, 3, False), tensor(3, 128), tensor(3, 128)),
            # (e) another channel instantiation, many row blocks, unsplit (one offset)
            "e": (module(sub, 256, 128, 1, False), tensor(0, 256), None),
            # (f) fused BatchNorm prologue
            "f": (module(sub, 128, 128, 3, False),
                  _PendingBN(rows(0, 128), bn, md, torch.tensor(SIZES[0])), None),
            # strided convolution and deconvolution (with residual) through the same entry point
            "down": (module(conv, 128, 128, 2, 2, False), tensor(2, 128), None),
            "up": (module(dec, 128, 128, 2, 2, False), tensor(4, 128), tensor(3, 128)),
            # a third instantiation, BPW = 4 (never split)
            "n32": (module(sub, 64, 32, 3, False), tensor(1, 64), None),
        }

    def one_by_one(self, names):
        out = {}
        for n in names:
            mod, inp, res = self.named[n]
            y = mod(inp) if res is None else mod(inp, residual=res)
            out[n] = (y, _last_form())
        return out


def _same(got, want):
    assert got.features.shape == want.features.shape
    assert torch.equal(got.features, want.features)
    assert got.spatial_size.tolist() == want.spatial_size.tolist()
    cw, cg = getattr(want, "col_partials", None), getattr(got, "col_partials", None)
    assert (cw is None) == (cg is None)
    if cw is not None:
        assert cw[1] == cg[1] and torch.equal(cw[0][:cw[1]], cg[0][:cg[1]])


@pytest.fixture(scope="module")
def calls(dev):
    with torch.no_grad():
        md, counts = _scene(dev)
        assert counts[4] == 33 and counts[5] <= 8 and 2000 <= counts[0] <= 5000, counts
        c = _Calls(dev, md, counts)
        c.ref = c.one_by_one(list(c.named))
    return c


ORDER = ["a", "b", "c", "e", "f", "down", "up", "n32"]


@pytest.mark.parametrize("reverse", [False, True])
def test_group_equals_one_by_one(calls, reverse):
    from detection_3d_amd.sparseconvnet.modules import conv_group
    names = ORDER[::-1] if reverse else ORDER
    forms = []
    outs = conv_group([calls.named[n] for n in names], forms=forms)
    assert len(outs) == len(names) == len(forms)
    for n, y, form in zip(names, outs, forms):
        want, want_form = calls.ref[n]
        _same(y, want)
        assert dict(zip(FIELDS, form)) == want_form, n          # each member keeps the form of its own call
    assert calls.ref["c"][1]["n_split"] > 1 and calls.ref["b"][1]["n_split"] > 1
    assert calls.ref["e"][1]["n_split"] == 1 and calls.ref["e"][1]["n_blk"] > 32
    assert calls.ref["b"][1]["n_blk"] == 2 and calls.ref["a"][1]["n_blk"] == 1
    assert calls.ref["e"][1]["nct"] == 2 and calls.ref["n32"][1]["bpw"] == 4     # three instantiations in the group
    assert calls.ref["f"][1]["stats"] == 1


@pytest.mark.parametrize("name", ["a", "c", "e"])
def test_group_of_one(calls, name):
    from detection_3d_amd.sparseconvnet.modules import conv_group
    (y,) = conv_group([calls.named[name]])
    _same(y, calls.ref[name][0])


def test_group_longer_than_the_table(calls):
    """CAP + 3 members of one instantiation, all of them offset-split but one: two k_conv_group launches and two
    reduction launches"""
    from detection_3d_amd.sparseconvnet.modules import conv_group
    names = (["b", "c", "f", "down", "up"] * 3)[:CAP + 2] + ["a"]
    outs = conv_group([calls.named[n] for n in names])
    for n, y in zip(names, outs):
        _same(y, calls.ref[n][0])
    assert sum(calls.ref[n][1]["n_split"] > 1 for n in names) > CAP


def test_group_without_statistics(calls):
    from detection_3d_amd.sparseconvnet.modules import conv_group
    outs = conv_group([calls.named[n] for n in ORDER], want_stats=False)
    for n, y in zip(ORDER, outs):
        assert torch.equal(y.features, calls.ref[n][0].features)
        assert not hasattr(y, "col_partials")


def test_members_without_rows(dev):
    """(d) a scene without points: every member has zero active rows, nothing is launched"""
    from detection_3d_amd.sparseconvnet.modules import conv_group
    md, counts = _scene(dev, empty=True)
    assert counts == [0] * len(SIZES)
    c = _Calls(dev, md, counts)
    forms = []
    outs = conv_group([c.named[n] for n in ORDER], forms=forms)
    for n, y in zip(ORDER, outs):
        assert y.features.shape == (0, c.named[n][0].nOut)
    assert all(not any(f) for f in forms)
    torch.cuda.synchronize()
