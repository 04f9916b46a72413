"""An fp32 emulation of k_roi_sparse's arithmetic for the exact geometry class of tests.roi_forms (yaw 0, a power-of-two
scale, samples on the 1/8-pixel lattice, NS a power of two), and the cases of test_roi_merge_cpu.py / test_roi_merge_gpu.py.

With that geometry every tap weight and every sum of tap weights is an fp32 number whatever the order of the additions,
so the weight of a merged cell does not depend on the reduction tree.  The feature values are arbitrary fp32 numbers:
what decides the bits of a result is the order of a bin's list of merged cells (ascending first lane of the cell) and
the order of the accumulation acc = fl(acc + fl(w v)) down that list, step after step, then one division by NS.

Lanes of a step: lane = 8 (sub-sample - first sub-sample of the step) + corner, sub-sample = (iy g_x + ix) g_z + iz,
corner = 4 zb + 2 yb + xb -- the order of tests.roi_forms.taps_of."""
import numpy as np

from tests import roi_forms as Rf

B = 8                           # kRoiB: cells per batch of weight sums in k_roi_sparse
SCALE = 0.25


def tree_sum(v):
    """the xor butterfly over 64 lanes, levels 32 ... 1, in fp32 (last axis: lanes); what lane 0 holds at the end"""
    v = np.asarray(v, np.float32).copy()
    idx = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., idx ^ d]).astype(np.float32)
    return v[..., 0]


def bin_lists(site, w):
    """site, w [NS, 8] of one bin -> per step of 8 sub-samples the list [(site, fp32 weight)] in order of first lane"""
    NS = site.shape[0]
    out = []
    for s0 in range(0, NS, 8):
        ls = np.full(64, -1, np.int64)
        lw = np.zeros(64, np.float32)
        n = min(8, NS - s0) * 8
        ls[:n] = site[s0:s0 + 8].reshape(-1)
        w32 = w[s0:s0 + 8].reshape(-1).astype(np.float32)
        assert np.array_equal(w32.astype(np.float64), w[s0:s0 + 8].reshape(-1)), "a tap weight is no fp32 number"
        lw[:n] = w32
        cells, first = np.unique(ls[ls >= 0], return_index=True)
        cells = cells[np.argsort(first, kind="stable")]
        if cells.size:
            wsum = tree_sum(np.where(ls[None, :] == cells[:, None], lw[None, :], np.float32(0)))
        else:
            wsum = np.zeros(0, np.float32)
        out.append((cells, wsum))
    return out


def emulate(rois, scale, m, crop, bins, sr):
    """-> out fp32 [K, C, PH, PW, PZ], lengths (the merged-list length of every (RoI, bin, step), in that order)"""
    rois = Rf.f32(rois).reshape(-1, 8)
    K, NB = rois.shape[0], Rf.nb_of(bins)
    F = np.asarray(m.feats, np.float32)
    C = F.shape[1]
    out = np.zeros((K, C, NB), np.float32)
    lengths = []
    for n in range(K):
        geo = Rf.geometry(rois[n], scale, bins, sr)
        y, x, z = Rf.sample_positions(geo, bins)
        NS = y.shape[1]
        site, w = Rf.taps_of(m, geo["b"], y, x, z, crop, False)
        for b in range(NB):
            acc = np.zeros(C, np.float32)
            for cells, wsum in bin_lists(site[b], w[b]):
                lengths.append(cells.size)
                for c, ww in zip(cells, wsum):
                    acc = (acc + (ww * F[c]).astype(np.float32)).astype(np.float32)
            out[n, :, b] = acc / np.float32(NS)
    return out.reshape((K, C) + tuple(bins)), np.array(lengths, np.int64)


# --------------------------------------------------------------------------------------------------------- cases
SIZE = (32, 32, 16)             # spatial size of every scene; the site (31, 31, 15) of example 0 makes it the extent


def _roi(by, bx, bz, bins, cells=4, example=0):
    """a box whose bins are `cells` pixels wide and start half a pixel below pixel (cells by, cells bx, cells bz): with
    sampling ratio 2 the two sub-samples of a bin per axis sit at +0.5 and +2.5 pixels (cells = 4), so the 64 taps of
    a bin are the 64 cells of its own 4 x 4 x 4 block"""
    r = np.zeros(8, np.float32)
    r[0] = example
    for col_c, col_s, b0, P in ((2, 5, by, bins[0]), (1, 4, bx, bins[1]), (3, 6, bz, bins[2])):
        r[col_s] = P * cells / SCALE
        r[col_c] = (cells * b0 - 0.5 + P * cells / 2.0) / SCALE
    return r


def _values(rng, rows, C, bf16):
    v = rng.randn(rows, C).astype(np.float32) * np.float32(3)
    return Rf.bf16_round(v) if bf16 else v


def _case(name, sites, rois, bins, sr, C, bf16, examples=1):
    sites = np.asarray(sites, np.int64).reshape(-1, 4)
    far = np.array([[SIZE[0] - 1, SIZE[1] - 1, SIZE[2] - 1, 0]])
    sites = np.unique(np.concatenate([sites, far]), axis=0)
    rng = np.random.RandomState(Rf.seed_of(name, C, bf16))
    sites = sites[rng.permutation(sites.shape[0])]
    m = Rf.SparseMap(sites, _values(rng, sites.shape[0], C, bf16))
    rois = np.asarray(rois, np.float32).reshape(-1, 8)
    assert rois.shape[0] <= 8
    return dict(name=name, map=m, rois=rois, crop=SIZE, size=SIZE, bins=tuple(bins), sr=sr, C=C, K=rois.shape[0],
                scale=SCALE, examples=examples, bf16=bf16)


GROUP_LENGTHS = [[(0, 64, 1, B + 1), (B - 1, B, B + 1, 64)],            # RoI 0: its two groups (pw = 0, 1)
                 [(64, 64, 64, 64), (1, 1, 0, 0)],                        # RoI 1: a full list of 256 cells
                 [(B, B, B, B), (3, 5, B - 1, 2)],
                 [(B + 1, 0, 0, B - 1), (64, 0, 64, 1)]]


def lengths_case(C, bf16):
    """bins 1 x 2 x 4 of 4-pixel bins; the occupancy of every bin's block is drawn to the list length wanted"""
    rng = np.random.RandomState(5)
    bins = (1, 2, 4)
    sites, rois = [], []
    for n, groups in enumerate(GROUP_LENGTHS):
        by, bx = n, 2 * (n % 3)
        rois.append(_roi(by, bx, 0, bins))
        for pw, lens in enumerate(groups):
            for pz, L in enumerate(lens):
                pick = rng.permutation(64)[:L]
                dy, dx, dz = np.unravel_index(pick, (4, 4, 4))
                sites.append(np.stack([4 * by + dy, 4 * (bx + pw) + dx, 4 * pz + dz, np.zeros(L, np.int64)], 1))
    return _case("lengths", np.concatenate(sites), rois, bins, 2, C, bf16)


def expected_lengths():
    return [L for groups in GROUP_LENGTHS for lens in groups for L in lens]


def one_cell_case(C, bf16):
    """1 x 1 x 1 bins (a ragged single group).  RoI 0: a box below one pixel beyond the far corner of the map: every
    coordinate is clamped, all 64 taps are the corner cell.  RoI 1: a one-pixel box inside: 8 cells of 8 taps.  RoI 2:
    the same box where only one of its 8 cells is a site."""
    bins = (1, 1, 1)
    r0 = np.zeros(8, np.float32)
    r0[1:4] = [(SIZE[1] - 0.5) / SCALE, (SIZE[0] - 0.5) / SCALE, (SIZE[2] - 0.5) / SCALE]
    r0[4:7] = 0.5 / SCALE
    r1 = np.zeros(8, np.float32)
    r1[1:4] = [5.5 / SCALE, 9.5 / SCALE, 3.5 / SCALE]
    r1[4:7] = 1.0 / SCALE
    r2 = r1.copy()
    r2[1:4] = [21.5 / SCALE, 9.5 / SCALE, 7.5 / SCALE]
    y, x, z = np.meshgrid([9, 10], [5, 6], [3, 4], indexing="ij")
    sites = np.stack([y.ravel(), x.ravel(), z.ravel(), np.zeros(8, np.int64)], 1)
    sites = np.concatenate([sites, [[10, 21, 7, 0]]])
    return _case("one cell", sites, [r0, r1, r2], bins, 2, C, bf16)


def random_case(name, C, bins, sr, K, bf16, g=None, occupancy=0.4):
    """a scene of tests.roi_forms (about 40 % of the cells of 24 x 20 x 10, two examples) and its exact-class boxes"""
    rng = np.random.RandomState(Rf.seed_of("merge", name, C, bins, sr))
    sites = Rf.small_sites(rng, occupancy=occupancy)
    gg = g if sr <= 0 else (sr,) * 3
    rois = Rf.exact_rois(rng, K, bins, gg, Rf.SMALL, 2, centre="adaptive" if sr <= 0 else None, scale=SCALE)
    return _case(name, sites, rois, bins, sr, C, bf16, examples=2)


def cases(bf16):
    """name -> case: the list-length cases and the store-path cases of the issue"""
    out = [lengths_case(6, bf16), one_cell_case(5, bf16),
           random_case("ragged 6x8x3", 4, (6, 8, 3), 2, 3, bf16),
           random_case("NS = 32", 6, (2, 2, 1), 0, 4, bf16, g=(4, 4, 2)),
           random_case("PZ = 3", 6, (2, 2, 3), 2, 4, bf16),
           random_case("PZ = 5", 6, (2, 1, 5), 2, 4, bf16)]
    out += [random_case(f"PZ = 4, C = {c}", c, (2, 2, 4), 2, 5, bf16) for c in (128, 130, 127)]
    return {c["name"]: c for c in out}


_CACHE = {}


def cached(bf16):
    """(cases, name -> (fp32 emulation, list lengths)), built once per storage type and never modified"""
    if bf16 not in _CACHE:
        cs = cases(bf16)
        _CACHE[bf16] = (cs, {k: emulate(c["rois"], c["scale"], c["map"], c["crop"], c["bins"], c["sr"])
                             for k, c in cs.items()})
    return _CACHE[bf16]
