"""What the rotated-RoIAlign tests share and a machine without a GPU can check (test_roi_forms_cpu.py): the fp64 reference
of the operation on a sparse map (forward, gradient of the feature rows, magnitude and slope terms, the tap list), the
generators of exact-arithmetic and of rounding cases with their preconditions and discontinuity margins, the comparators
with their bounds, and the dispatch arithmetic of the roi_*.hip files restated -- the record d3d_roi_last_form must give.

The operation (ROIAlignRotated3D): a RoI row is (example, centre x, centre y, centre z, size x, size y, size z, yaw in
degrees) in pixels of the full-resolution grid; y runs over the map's first spatial axis (H), x over the second (W).
Centre and sizes are multiplied by the spatial scale, sizes are clamped to one pixel, the box is cut into PH x PW x PZ
bins, every bin is sampled at g_y x g_x x g_z points (g = sampling_ratio, or ceil(size / bins) per axis), the points are
rotated about the centre by the yaw, a point outside [-1, H] x [-1, W] x [-1, inf) is empty (the forward has no upper z
bound -- the `zsize > zsize` comparison of the reference operation, kept by the kernels; the backward drops z > Z),
coordinates are clamped to the crop, the map is interpolated trilinearly (absent sites are zeros) and the bin's value is
the mean over all NS = g_y g_x g_z points, empty ones included.

Bounds of the rounding class (u = 2^-24).  Nothing here is fitted to a kernel's output.

* position: the kernels evaluate the sample positions in fp32.  roi_geom rounds centre and size once each (u), the bin
  size once; sample_pos rounds ph * b, its sum with the start, (i + .5) * b, the division by g and the last sum: with
  the size's own rounding 7 roundings of quantities no larger than the size s of that axis, |d yy| <= 7 u s.  The yaw is
  rounded to fp32 radians (u |theta| <= u pi) and cos / sin once more (u), the two products and their sum round once
  each at magnitudes <= (s_x + s_y) / 2, the sum with the centre rounds at |x| <= |c| + (s_x + s_y) / 2 and the centre
  carries its own u |c|:  |d x| <= u [7 (s_x + s_y) + (pi + 3) (s_x + s_y) / 2 + (s_x + s_y) / 2 + 2 |c|]
  < 11 u M with M = s_x + s_y + s_z + |c_x| + |c_y| + |c_z|.  A fused multiply-add removes a rounding and adds none.
  pos_bound(M) = gamma_11 M serves the three axes.  (The fp32 model of test_roi_forms_cpu.py measures 0.58 u M with this M.)
* forward, position term: the trilinear interpolant of a channel is continuous, and along an axis its slope is a convex
  combination of differences of adjacent cells, so it is Lipschitz with the largest adjacent difference G of that channel
  in that example (absent neighbours are zeros); clamping to the crop is 1-Lipschitz.  A mean over samples that each move
  by at most pos_bound per axis changes by at most 3 G pos_bound.
* forward, accumulation term: gamma_n sum |w v| / NS with n = 12 + 8 NS: the corner weight (1 - l, two products; l = y -
  floor y is exact) 4, the butterfly merge 6, the product with the value 1, at most 8 NS additions, the division 1.
* backward: the weight of a site as a function of the sample position is a product of three hat functions, each
  1-Lipschitz with values in [0, 1], so a record's weight moves by at most 3 pos_bound; the slope term of a feature row
  sums 3 pos_bound |top| / NS over the samples within pos_bound of the site's support.  Accumulation: gamma_n sum |w top|
  / NS with n = 16 + R + R / 64 (weight 4, merge 6, product, division, rounding of the record's weight, at most R
  additions for the row's R taps, the chunk partials of the fixed-order form).
* bf16 results add half a bf16 ulp of |reference| + bound.

The operation is discontinuous at the bound tests, the one-pixel clamp and the ceil of the adaptive grid; the rounding
generator keeps every fp64 sample 2^10 pos_bound away from the planes y = -1, y = H, x = -1, x = W, z = -1 and z = Z,
every scaled size that far from 1 and, for adaptive sampling (the only place it matters), size / bins that far from an
integer, redrawing from the same seeded stream.  No element is left out of a comparison."""
import math

import numpy as np

# ---------------------------------------------------------------------------------------------------- the record
ROI_FIELDS = ("family", "type", "lookup", "extent", "grid_x", "grid_y", "grid_z", "block", "levels", "cvt_wgs", "n_max",
              "n_chunks", "bits")
DENSE, SPARSE, DENSE_BWD, SPARSE_BWD, DET = 1, 2, 3, 4, 5      # family
F32, BF16 = 1, 2                                                # type
HASH, INDEX = 1, 2                                              # lookup (bits)
CROP, DEVICE = 1, 2                                             # extent (bits)

ROI_G = 4                      # kRoiG: bins per group of k_roi_sparse
ROI_WAVES = 4                  # kRoiWaves
ROI_CCH = 128                  # kRoiCch
ROI_BWD_CCH = 64               # kRoiBwdCch
DET_CHUNK = 64                 # kRoiDetChunk
DET_CPL = 4                    # kRoiDetCpl
MAX_LEVELS = 4                 # kRoiMaxLevels
DENSE_MAX_CELLS = 8 << 20      # kDenseMaxCells (grid_views.hip)
LDS_BYTES = 64 * 1024

U32 = 2.0 ** -24
POS_K = 11                     # roundings of a sample position, see the module docstring
MARGIN = 2.0 ** 10             # discontinuity margin in position bounds


def cdiv(a, b):
    return -(-a // b)


def gamma(n):
    return n * U32 / (1 - n * U32)


def nb_of(bins):
    return bins[0] * bins[1] * bins[2]


def bwd_bins_ok(bins):
    """the backward's tile [kRoiBwdCch][NB + 1] of floats must fit the 64 KB of LDS: NB <= 255"""
    return ROI_BWD_CCH * (nb_of(bins) + 1) * 4 <= LDS_BYTES


def dense_index_taken(hext):
    """grid_extent: hext = 1 + largest (x, y, z, example) of the grid's sites"""
    return 0 < hext[0] * hext[1] * hext[2] * hext[3] <= DENSE_MAX_CELLS


def expect_roi(family, typ, K, C, bins, sr=0, lookup=0, extent=0, levels=0, n_rows=0):
    """The whole record after one call (zeros: nothing launched)."""
    f = dict.fromkeys(ROI_FIELDS, 0)
    NB = nb_of(bins)
    if family in (DENSE, DENSE_BWD):
        assert typ == F32
        if K:
            f.update(family=family, type=F32, grid_x=cdiv(K * C * NB, 256), grid_y=1, grid_z=1, block=256)
    elif family == SPARSE:
        if K:
            f.update(family=SPARSE, type=typ, lookup=lookup, extent=extent, grid_x=K, grid_y=cdiv(C, ROI_CCH), grid_z=1,
                     block=ROI_WAVES * 64, levels=levels)
    elif family == SPARSE_BWD:
        assert bwd_bins_ok(bins)
        if typ == BF16 and n_rows:          # the rounding pass runs for K = 0 too: every row is written
            f.update(family=SPARSE_BWD, type=BF16, lookup=HASH, extent=CROP, block=256, levels=1,
                     cvt_wgs=cdiv(n_rows * C, 1024))
            if K:
                f.update(grid_x=K, grid_y=cdiv(C, ROI_BWD_CCH), grid_z=1)
        elif typ == F32 and K:
            f.update(family=SPARSE_BWD, type=F32, lookup=HASH, extent=CROP, grid_x=K, grid_y=cdiv(C, ROI_BWD_CCH),
                     grid_z=1, block=256, levels=1)
    else:
        assert family == DET and sr > 0
        if K and n_rows:
            n_max = K * NB * sr ** 3 * 8
            n_chunks = cdiv(n_max, DET_CHUNK)
            bits = 1
            while bits < 31 and (1 << bits) < n_rows:
                bits += 1
            f.update(family=DET, type=typ, lookup=HASH, extent=CROP, grid_x=cdiv(n_chunks, 4), grid_y=1, grid_z=1,
                     block=256, levels=1, n_max=n_max, n_chunks=n_chunks, bits=bits)
    return f


# ------------------------------------------------------------------------------------------------ number formats
def f32(a):
    return np.asarray(a, dtype=np.float32)


def bf16_round(a):
    """round to nearest even to bf16, as fp32 values (finite inputs)"""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def half_ulp_bf16(x):
    """half the spacing of bf16 numbers at magnitude x (8 significand bits)"""
    x = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return 0.5 * 2.0 ** (np.floor(np.log2(x)) - 7)


# ------------------------------------------------------------------------------------------------------ the map
class SparseMap:
    """sites int64 [n, 4] = (y, x, z, example) -- the columns of get_spatial_locations -- and their feature rows"""

    def __init__(self, sites, feats):
        self.sites = np.asarray(sites, np.int64).reshape(-1, 4)
        self.feats = np.asarray(feats)
        assert self.feats.shape[0] == self.sites.shape[0]
        k = self._key(self.sites[:, 3], self.sites[:, 0], self.sites[:, 1], self.sites[:, 2])
        self._order = np.argsort(k, kind="stable")
        self._keys = k[self._order]
        assert np.unique(k).size == k.size, "duplicate sites"

    @staticmethod
    def _key(b, y, x, z):
        return ((np.asarray(b, np.int64) << 48) | (np.asarray(y, np.int64) << 32) | (np.asarray(x, np.int64) << 16)
                | np.asarray(z, np.int64))

    @property
    def n(self):
        return self.sites.shape[0]

    def extent(self):
        return tuple(int(v) + 1 for v in self.sites[:, :3].max(0))

    def find(self, b, y, x, z):
        """site id per cell, -1 where the cell is empty (coordinates >= 0)"""
        k = self._key(b, y, x, z)
        if self._keys.size == 0:
            return np.full(k.shape, -1, np.int64)
        p = np.minimum(np.searchsorted(self._keys, k), self._keys.size - 1)
        return np.where(self._keys[p] == k, self._order[p], -1)


def dense_as_map(dense):
    """a dense map [B, C, H, W, Z] in which every cell is a site (site id = the cell's flat index)"""
    B, C, H, W, Z = dense.shape
    b, y, x, z = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), np.arange(Z), indexing="ij")
    sites = np.stack([y.ravel(), x.ravel(), z.ravel(), b.ravel()], 1)
    return SparseMap(sites, np.moveaxis(dense, 1, -1).reshape(-1, C))


def adjacent_slope(m, n_examples):
    """G [example, C]: the largest difference of a channel between cells adjacent along an axis (absent cells are zeros)"""
    F = np.abs(np.asarray(m.feats, np.float64))
    C = F.shape[1]
    G = np.zeros((n_examples, C))
    if m.n == 0:
        return G
    v = np.asarray(m.feats, np.float64)
    pad = np.vstack([v, np.zeros((1, C))])
    s = m.sites
    worst = F.copy()
    for ax in range(3):
        for d in (-1, 1):
            q = s[:, :3].copy()
            q[:, ax] += d
            ok = q[:, ax] >= 0
            nb = m.find(s[:, 3], np.maximum(q[:, 0], 0), np.maximum(q[:, 1], 0), np.maximum(q[:, 2], 0))
            nb = np.where(ok & (nb >= 0), nb, m.n)
            worst = np.maximum(worst, np.abs(v - pad[nb]))
    for b in range(n_examples):
        sel = s[:, 3] == b
        if sel.any():
            G[b] = worst[sel].max(0)
    return G


# ------------------------------------------------------------------------------------------------- the geometry
def geometry(roi, scale, bins, sr):
    """fp64, from the fp32 RoI row and the fp32 spatial scale"""
    r = f32(roi).astype(np.float64)
    s = float(np.float32(scale))
    c = np.array([r[2], r[1], r[3]]) * s                         # centre (y, x, z)
    size = np.maximum(np.array([r[5], r[4], r[6]]) * s, 1.0)     # size (y, x, z) after the one-pixel clamp
    raw = np.array([r[5], r[4], r[6]]) * s
    P = np.array(bins, np.float64)
    g = np.array([sr] * 3) if sr > 0 else np.ceil(size / P).astype(np.int64)
    M = float(size.sum() + np.abs(c).sum())
    return dict(b=int(r[0]), c=c, size=size, raw=raw, bin=size / P, g=g, theta=r[7] * math.pi / 180.0, M=M,
                pos=gamma(POS_K) * M)


def sample_positions(geo, bins):
    """y, x, z [NB, NS]: bin = (ph PW + pw) PZ + pz, sub-sample = (iy g_x + ix) g_z + iz"""
    PH, PW, PZ = bins
    gh, gw, gz = (int(v) for v in geo["g"])
    loc = []
    for ax, (P, g) in enumerate(((PH, gh), (PW, gw), (PZ, gz))):
        p = np.arange(P, dtype=np.float64)[:, None]
        i = np.arange(g, dtype=np.float64)[None, :]
        loc.append(-geo["size"][ax] / 2 + p * geo["bin"][ax] + (i + 0.5) * geo["bin"][ax] / g)
    ph, pw, pz = np.unravel_index(np.arange(PH * PW * PZ), (PH, PW, PZ))
    iy, ix, iz = np.unravel_index(np.arange(gh * gw * gz), (gh, gw, gz))
    yy = loc[0][ph[:, None], iy[None, :]]
    xx = loc[1][pw[:, None], ix[None, :]]
    zz = loc[2][pz[:, None], iz[None, :]]
    ct, st = math.cos(geo["theta"]), math.sin(geo["theta"])
    return yy * ct - xx * st + geo["c"][0], xx * ct + yy * st + geo["c"][1], zz + geo["c"][2]


def _axis(v, n, tau=0.0):
    """clamp to the crop; cells and weights along one axis; with tau > 0 the three candidate cells within tau"""
    v = np.maximum(v, 0.0)
    lo = np.floor(v).astype(np.int64)
    top = lo >= n - 1
    lo = np.where(top, n - 1, lo)
    hi = np.where(top, n - 1, lo + 1)
    v = np.where(top, lo.astype(np.float64), v)
    l = v - lo
    if tau == 0.0:
        return lo, hi, 1.0 - l, l
    a = np.clip(v - tau, 0, n - 1)
    b = np.clip(v + tau, 0, n - 1)
    c0 = np.floor(a).astype(np.int64)
    c1 = np.minimum(c0 + 1, n - 1)
    c2 = np.minimum(np.floor(b).astype(np.int64) + 1, n - 1)
    return c0, c1, c2


def inside(y, x, z, crop, backward):
    H, W, Z = crop
    ok = ~((y < -1.0) | (y > H) | (x < -1.0) | (x > W) | (z < -1.0))
    return ok & ~(z > Z) if backward else ok


def taps_of(m, b, y, x, z, crop, backward):
    """site [NB, NS, 8] (-1: the sample is empty or the cell has no site) and weight [NB, NS, 8]; corner = 4 zb + 2 yb + xb"""
    H, W, Z = crop
    ok = inside(y, x, z, crop, backward)
    yl, yh, hy, ly = _axis(y, H)
    xl, xh, hx, lx = _axis(x, W)
    zl, zh, hz, lz = _axis(z, Z)
    site = np.empty(y.shape + (8,), np.int64)
    w = np.empty(y.shape + (8,), np.float64)
    for q in range(8):
        zb, yb, xb = q >> 2, (q >> 1) & 1, q & 1
        site[..., q] = m.find(b, yh if yb else yl, xh if xb else xl, zh if zb else zl)
        w[..., q] = (ly if yb else hy) * (lx if xb else hx) * (lz if zb else hz)
    site = np.where(ok[..., None], site, -1)
    return site, np.where(site >= 0, w, 0.0)


def near_sites(m, b, y, x, z, crop, backward, tau):
    """site [NB, NS, 27]: every site whose support comes within tau of the sample (-1: none); the third candidate of an
    axis is masked where it repeats the second"""
    H, W, Z = crop
    ok = inside(y, x, z, crop, backward)
    cy, cx, cz = _axis(y, H, tau), _axis(x, W, tau), _axis(z, Z, tau)
    out = np.empty(y.shape + (27,), np.int64)
    for i in range(3):
        for j in range(3):
            for k in range(3):
                s = m.find(b, cy[i], cx[j], cz[k])
                dup = np.zeros(y.shape, bool)
                if i == 2:
                    dup |= cy[2] == cy[1]
                if j == 2:
                    dup |= cx[2] == cx[1]
                if k == 2:
                    dup |= cz[2] == cz[1]
                out[..., (i * 3 + j) * 3 + k] = np.where(dup | ~ok, -1, s)
    return out


# ------------------------------------------------------------------------------------------------ the reference
class Ref:
    pass


def roi_ref(rois, scale, m, crop, bins, sr, top=None, n_examples=None, slopes=True):
    """The fp64 reference.  rois fp32 [K, 8]; m a SparseMap; crop (H, W, Z).  Returns an object with
      out [K, C, PH, PW, PZ], mag (sum |w v| / NS), slope (3 G per element), pos [K] (position bound of the RoI), ns [K];
      with top [K, C, PH, PW, PZ]: grad [n, C], gmag (sum |w top| / NS), gslope (sum 3 pos |top| / NS), recs [n] (merged
      records of a row), ntaps [n] (its taps before merging);
      taps: int64 [T, 4] rows (site, RoI, bin, step) -- one per merged cell of a step of 8 sub-samples, sorted by
      (RoI, bin, step); steps [K]: the number of steps per bin.
    The forward quantities use the forward's bound test, the gradient ones the backward's."""
    rois = f32(rois).reshape(-1, 8)
    K, NB = rois.shape[0], nb_of(bins)
    C = m.feats.shape[1]
    F = np.vstack([np.asarray(m.feats, np.float64), np.zeros((1, C))])
    n_examples = n_examples or (int(m.sites[:, 3].max()) + 1 if m.n else 1)
    G = adjacent_slope(m, n_examples) if slopes else np.zeros((n_examples, C))
    R = Ref()
    R.out, R.mag, R.slope = np.zeros((K, C, NB)), np.zeros((K, C, NB)), np.zeros((K, C, NB))
    R.pos, R.ns, R.steps = np.zeros(K), np.zeros(K, np.int64), np.zeros(K, np.int64)
    R.M = np.zeros(K)
    taps, btaps = [], []
    if top is not None:
        top = np.asarray(top, np.float64).reshape(K, C, NB)
        R.grad, R.gmag, R.gslope = np.zeros((m.n + 1, C)), np.zeros((m.n + 1, C)), np.zeros((m.n + 1, C))
        R.recs, R.ntaps = np.zeros(m.n + 1, np.int64), np.zeros(m.n + 1, np.int64)
    for n in range(K):
        geo = geometry(rois[n], scale, bins, sr)
        y, x, z = sample_positions(geo, bins)
        NS = y.shape[1]
        R.pos[n], R.ns[n], R.steps[n], R.M[n] = geo["pos"], NS, cdiv(NS, 8), geo["M"]
        R.slope[n] = 3.0 * G[geo["b"]][:, None]
        for backward in ((False, True) if top is not None else (False,)):
            site, w = taps_of(m, geo["b"], y, x, z, crop, backward)
            flat = site.reshape(NB, -1)
            touched, inv = np.unique(np.where(flat >= 0, flat, m.n), return_inverse=True)
            Wm = np.zeros((touched.size, NB))
            np.add.at(Wm, (inv.reshape(-1), np.repeat(np.arange(NB), flat.shape[1])), w.reshape(-1))
            # merged cells per (bin, step)
            step = np.broadcast_to((np.arange(NS) // 8)[None, :, None], site.shape)
            binx = np.broadcast_to(np.arange(NB)[:, None, None], site.shape)
            have = site >= 0
            key = np.unique((binx[have] * R.steps[n] + step[have]) * (m.n + 1) + site[have])
            rows = np.stack([key % (m.n + 1), np.full(key.size, n), key // (m.n + 1) // R.steps[n],
                             key // (m.n + 1) % R.steps[n]], 1) if key.size else np.zeros((0, 4), np.int64)
            if not backward:
                R.out[n] = (Wm.T @ F[touched]).T / NS
                R.mag[n] = (Wm.T @ np.abs(F[touched])).T / NS
                taps.append(rows)
            else:
                R.grad[touched] += Wm @ top[n].T / NS
                R.gmag[touched] += Wm @ np.abs(top[n]).T / NS
                np.add.at(R.recs, rows[:, 0], 1)
                np.add.at(R.ntaps, flat[flat >= 0], 1)
                btaps.append(rows)
                if slopes:
                    near = near_sites(m, geo["b"], y, x, z, crop, True, geo["pos"]).reshape(NB, -1)
                    t2, inv2 = np.unique(np.where(near >= 0, near, m.n), return_inverse=True)
                    E = np.zeros((t2.size, NB))
                    np.add.at(E, (inv2.reshape(-1), np.repeat(np.arange(NB), near.shape[1])), 1.0)
                    R.gslope[t2] += 3.0 * geo["pos"] * (E @ np.abs(top[n]).T) / NS
    shape = (K, C) + tuple(bins)
    R.out, R.mag, R.slope = R.out.reshape(shape), R.mag.reshape(shape), R.slope.reshape(shape)
    R.taps = np.concatenate(taps) if taps else np.zeros((0, 4), np.int64)
    if top is not None:
        R.grad, R.gmag, R.gslope, R.recs, R.ntaps = R.grad[:-1], R.gmag[:-1], R.gslope[:-1], R.recs[:-1], R.ntaps[:-1]
        R.btaps = np.concatenate(btaps) if btaps else np.zeros((0, 4), np.int64)
    return R


def list_lengths(taps, K, NB, steps):
    """merged-cell list length of every (RoI, bin, step), zeros included"""
    out = []
    for n in range(K):
        t = taps[taps[:, 1] == n]
        out.append(np.bincount(t[:, 2] * steps[n] + t[:, 3], minlength=NB * steps[n]))
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def record_lists(btaps, n_rows):
    """the fixed-order backward's inverted index: records sorted stably by site; begin / end of every site's list"""
    order = np.argsort(btaps[:, 0], kind="stable")
    skey = btaps[order, 0]
    beg = np.searchsorted(skey, np.arange(n_rows), "left")
    end = np.searchsorted(skey, np.arange(n_rows), "right")
    return order, beg, end


# ------------------------------------------------------------------------------------------------- comparators
MARGINS = {}          # check -> the largest error / bound it saw
WORST = {}            # check -> the case that gave it


def _note(name, ratio, tag=""):
    if name not in MARGINS or float(ratio) > MARGINS[name]:
        MARGINS[name], WORST[name] = float(ratio), tag


def forward_bound(R, bf16):
    n_ops = 12 + 8 * R.ns
    b = R.pos[:, None, None, None, None] * R.slope + gamma(n_ops)[:, None, None, None, None] * R.mag
    return b + half_ulp_bf16(np.abs(R.out) + b) if bf16 else b


def backward_bound(R, bf16):
    n_ops = 16 + R.ntaps + R.ntaps // DET_CHUNK      # taps, not merged records: the dense backward adds every tap
    b = R.gslope + gamma(n_ops)[:, None] * R.gmag
    return b + half_ulp_bf16(np.abs(R.grad) + b) if bf16 else b


def check(tag, name, got, want, bound, exact, bf16):
    """exact: the bits of the fp64 result (bf16: rounded to nearest even once); else every element within its bound"""
    got = np.asarray(got)
    assert got.shape == want.shape, f"{tag}: shape {got.shape} != {want.shape}"
    assert np.isfinite(got).all(), f"{tag}: {int((~np.isfinite(got)).sum())} non-finite values"
    if exact:
        w32 = want.astype(np.float32)
        assert np.array_equal(w32.astype(np.float64), want), f"{tag}: the exact result is no fp32 number"
        target = bf16_round(w32) if bf16 else w32
        bad = f32(got).view(np.uint32) != np.ascontiguousarray(target).view(np.uint32)
        # -0 cannot arise (sums start from +0); +0 == +0 bitwise
        assert not bad.any(), (f"{tag}: {int(bad.sum())} of {bad.size} elements differ in bits, first at "
                               f"{tuple(np.argwhere(bad)[0])}: {f32(got)[bad][0]!r} != {target[bad][0]!r}")
        _note(name + " (bit for bit)", 0.0, tag)
        return
    err = np.abs(got.astype(np.float64) - want)
    over = err > bound
    ratio = (err / np.maximum(bound, 1e-300))
    if over.any():
        i = tuple(np.argwhere(over)[np.argmax(ratio[over])])
        raise AssertionError(f"{tag}: {int(over.sum())} of {over.size} elements past their bound, worst at {i}: "
                             f"got {got[i]!r}, reference {want[i]!r}, error {err[i]:.3e}, bound {bound[i]:.3e}")
    _note(name, ratio[bound > 0].max() if (bound > 0).any() else 0.0, tag)


def check_forward(tag, got, R, exact, bf16):
    check(tag, "forward bf16" if bf16 else "forward fp32", got, R.out, None if exact else forward_bound(R, bf16), exact, bf16)


def check_backward(tag, got, R, exact, bf16, base=None):
    """base: what d_feats held before the call (the fp32 fixed-order form adds to it)"""
    want = R.grad if base is None else R.grad + np.asarray(base, np.float64)
    b = None
    if not exact:
        b = backward_bound(R, bf16)
        if base is not None:
            b = b + U32 * np.abs(want)         # the one addition to the buffer's value
    name = "backward bf16" if bf16 else "backward fp32"
    check(tag, name if base is None else name + ", added to a buffer", got, want, b, exact, bf16)


# -------------------------------------------------------------------------------------------------- generators
def seed_of(*parts):
    h = 2166136261
    for p in parts:
        for ch in repr(p).encode():
            h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


SMALL = (24, 20, 10)            # crop (H, W, Z) of the small scene
SMALL_SIZE = (32, 32, 16)       # its spatial size
FAR_SIZE = (4096, 4096, 512)
SCALE = 0.25


def small_sites(rng, n_examples=2, occupancy=0.4, crop=SMALL):
    """about 40 % of the cells per example, a different set in each; the far corner of example 0 is always a site, so
    the occupied extent is the crop"""
    H, W, Z = crop
    out = []
    for b in range(n_examples):
        occ = rng.rand(H, W, Z) < occupancy
        if b == 0:
            occ[H - 1, W - 1, Z - 1] = True
        y, x, z = np.nonzero(occ)
        out.append(np.stack([y, x, z, np.full(y.size, b)], 1))
    s = np.concatenate(out)
    return s[rng.permutation(s.shape[0])]


def far_sites(rng):
    """two clusters far enough apart on the 4096 x 4096 x 512 lattice that the dense index is declined"""
    a = np.stack(np.meshgrid(np.arange(6, 18), np.arange(6, 18), np.arange(3, 11), indexing="ij"), -1).reshape(-1, 3)
    a = a[rng.rand(a.shape[0]) < 0.4]
    b = a + np.array([3000, 3000, 400])
    s = np.concatenate([a, b, np.array([[4000, 4000, 500]])])
    s = np.concatenate([s, np.zeros((s.shape[0], 1), np.int64)], 1)
    assert not dense_index_taken(tuple(int(v) + 1 for v in s.max(0)))
    return s[rng.permutation(s.shape[0])]


def exact_values(rng, shape):
    """non-zero integers in +-{1..4}: fp32 and bf16 numbers"""
    return (rng.randint(1, 5, shape) * rng.choice([-1, 1], shape)).astype(np.float32)


CHANNEL_SCALES = (1.0, 1.0 / 64, 64.0)


def rounding_values(rng, rows, C, bf16):
    v = rng.randn(rows, C) * np.resize(np.array(CHANNEL_SCALES), C)[None, :]
    return bf16_round(v) if bf16 else v.astype(np.float32)


def exact_rois(rng, K, bins, g, crop, n_examples, centre=None, scale=SCALE):
    """yaw 0, spatial scale a power of two, bin size b = g m / 4 per axis with integer m (adaptive sampling: sampling_ratio 0 and
    m = 4, so that ceil(b) = g), centres on the 1/8-pixel lattice of the map: every sample coordinate
    is a multiple of 1/8 pixel.  g: sub-samples per axis (y, x, z), each a power of two."""
    rois = np.zeros((K, 8), np.float32)
    for n in range(K):
        rois[n, 0] = n % n_examples
        for ax, col_c, col_s in ((0, 2, 5), (1, 1, 4), (2, 3, 6)):
            P, gg = bins[ax], g[ax]
            m_min = max(1, cdiv(4, P * gg))
            mm = 4 if centre == "adaptive" else rng.randint(m_min, m_min + 5)
            b = gg * mm / 4.0
            rois[n, col_s] = P * b / scale
            lo, hi = (0, crop[ax]) if centre is None or centre == "adaptive" else centre[ax]
            rois[n, col_c] = rng.randint(int(lo * 8), int(hi * 8) + 1) / 8.0 / scale
    return rois


def assert_exact_case(rois, scale, m, crop, bins, sr, top=None):
    """the preconditions of the exact class: dyadic geometry, NS a power of two, every partial sum within 24 bits"""
    R = roi_ref(rois, scale, m, crop, bins, sr, top=top, slopes=False)
    assert math.log2(float(np.float32(scale))).is_integer()
    for n in range(f32(rois).reshape(-1, 8).shape[0]):
        geo = geometry(rois[n], scale, bins, sr)
        assert geo["theta"] == 0.0
        for v in sample_positions(geo, bins):
            assert np.array_equal(v * 8, np.round(v * 8)) and np.abs(v).max() < 2 ** 20
        assert R.ns[n] & (R.ns[n] - 1) == 0
    v = np.asarray(m.feats, np.float64)
    assert np.array_equal(v, np.round(v)) and (np.abs(v) >= 1).all() and (np.abs(v) <= 4).all()
    ns = R.ns[:, None, None, None, None] if R.ns.size else 1
    assert (R.mag * ns * 512 < 2 ** 24).all()       # weights are multiples of 1/512, values integers
    if top is not None:
        t = np.asarray(top, np.float64)
        assert np.array_equal(t, np.round(t)) and (np.abs(t) >= 1).all() and (np.abs(t) <= 4).all()
        assert (R.gmag * 512 * (int(R.ns.max()) if R.ns.size else 1) < 2 ** 24).all()
    return R


def discontinuity_margin(roi, scale, bins, sr, crop):
    """the smallest distance of the RoI from a discontinuity of the operation, in units of its position bound"""
    geo = geometry(roi, scale, bins, sr)
    y, x, z = sample_positions(geo, bins)
    H, W, Z = crop
    d = min(np.abs(y + 1).min(), np.abs(y - H).min(), np.abs(x + 1).min(), np.abs(x - W).min(), np.abs(z + 1).min(),
            np.abs(z - Z).min(), np.abs(geo["raw"] - 1.0).min())
    if sr <= 0:
        q = geo["size"] / np.array(bins, np.float64)
        d = min(d, np.abs(q - np.round(q)).min())
    return d / geo["pos"]


def rounding_rois(rng, K, bins, sr, crop, n_examples, size=(0.3, 14.0), centre=None, g=None, scale=SCALE,
                  max_draws=10000):
    """arbitrary yaw in (-180, 180], centres and sizes on no lattice; g (adaptive sampling only): the sub-sample counts
    per axis (y, x, z) the sizes are drawn for.  A box closer than 2^10 position bounds to a discontinuity is redrawn."""
    rois = np.zeros((K, 8), np.float32)
    draws = 0
    for n in range(K):
        while True:
            draws += 1
            assert draws <= max_draws, "the generator does not terminate"
            r = np.zeros(8, np.float32)
            r[0] = n % n_examples
            for ax, col_c, col_s in ((0, 2, 5), (1, 1, 4), (2, 3, 6)):
                lo, hi = (-1.0, crop[ax] + 1.0) if centre is None else centre[ax]
                r[col_c] = rng.uniform(lo, hi) / scale
                if g is not None:
                    r[col_s] = bins[ax] * rng.uniform(g[ax] - 0.9, g[ax] - 0.1) / scale
                else:
                    s_lo, s_hi = size if np.isscalar(size[0]) else size[ax]
                    r[col_s] = rng.uniform(s_lo, s_hi) / scale
            r[7] = 180.0 - rng.uniform(0.0, 360.0)
            if discontinuity_margin(r, scale, bins, sr, crop) >= MARGIN:
                rois[n] = r
                break
    return rois



# -------------------------------------------------------------------------------------------------------- cases
def spec(name, C, bins, sr, K, scene="small", g=None, centre=None, size=(0.3, 14.0), scale=SCALE, n_sites=None,
         exact=True, rounding=True):
    return dict(name=name, C=C, bins=tuple(bins), sr=sr, K=K, scene=scene, g=g, centre=centre, size=size, scale=scale,
                n_sites=n_sites, exact=exact, rounding=rounding)


def _pow2(g):
    return all(v & (v - 1) == 0 for v in g)


FWD_CHANNELS = [spec(f"C={c}", c, (3, 2, 5), 2, 4) for c in (1, 2, 37, 128, 130, 255, 256)]
BWD_CHANNELS = [spec(f"C={c}", c, (3, 2, 5), 2, 4) for c in (1, 63, 64, 65, 130)]
DET_CHANNELS = [spec(f"C={c}", c, (2, 2, 1), 2, 4) for c in (1, 37, 256, 257, 320)]
BINS = [spec("bins=%dx%dx%d" % b, 6, b, 2, 4) for b in
        ((1, 1, 1), (1, 3, 1), (2, 2, 1), (1, 5, 1), (4, 2, 2), (17, 1, 1), (3, 2, 5), (6, 8, 4))]
BWD_ONLY_BINS = [spec("bins=5x3x17", 3, (5, 3, 17), 1, 2)]
REFUSED_BINS = (4, 8, 8)
SUBSAMPLES = [spec("sr=1", 5, (3, 2, 2), 1, 6), spec("sr=2", 5, (3, 2, 2), 2, 6),
              spec("sr=3", 5, (3, 2, 2), 3, 6, exact=False),
              spec("adaptive 1x2x3", 5, (2, 2, 1), 0, 5, g=(1, 2, 3), exact=False),
              spec("adaptive 4x4x2", 5, (2, 2, 1), 0, 5, g=(4, 4, 2)),
              spec("adaptive 5x3x2", 5, (2, 2, 1), 0, 5, g=(5, 3, 2), exact=False),
              spec("adaptive 1x2x2", 5, (3, 2, 2), 0, 5, g=(1, 2, 2)),
              spec("small boxes", 5, (1, 3, 1), 2, 8, size=(0.3, 1.6))]
FAR_A, FAR_B = ((8.0, 16.0), (8.0, 16.0), (5.0, 9.0)), ((3002.0, 3016.0), (3002.0, 3016.0), (402.0, 409.0))
LOOKUP_FAR = [spec("far, near cluster", 4, (2, 2, 1), 2, 4, scene="far", centre=FAR_A, size=(2.5, 6.0)),
              spec("far, far cluster", 4, (2, 2, 1), 2, 4, scene="far", centre=FAR_B, size=(2.5, 6.0))]
H_, W_, Z_ = SMALL
_MID = ((6.0, 18.0), (6.0, 14.0), (3.0, 7.0))


def _edge(name, centre, size=(2.0, 6.0), scene="small", K=3, **kw):
    return spec(name, 3, (2, 2, 1), 2, K, scene=scene, centre=centre, size=size, **kw)


EDGES = [_edge("below one pixel", _MID, size=(0.05, 0.6), exact=False),
         _edge("wholly outside", ((H_ + 20.0, H_ + 30.0), _MID[1], _MID[2])),
         _edge("cut by y = -1", ((-1.0, 1.0), _MID[1], _MID[2])),
         _edge("cut by y = H", ((H_ - 1.0, H_ + 1.0), _MID[1], _MID[2])),
         _edge("cut by x = -1", (_MID[0], (-1.0, 1.0), _MID[2])),
         _edge("cut by x = W", (_MID[0], (W_ - 1.0, W_ + 1.0), _MID[2])),
         _edge("cut by z = -1", (_MID[0], _MID[1], (-1.2, -0.8))),
         _edge("z above the map", (_MID[0], _MID[1], (Z_ - 1.0, Z_ + 3.0))),
         _edge("centre in the -1 .. 0 band", ((-1.0, 0.0), (-1.0, 0.0), (-1.0, 0.0)), size=(0.3, 3.0)),
         _edge("K = 0", _MID, K=0),
         _edge("K = 1", _MID, K=1),
         _edge("no site inside the box", ((12.0, 18.0), _MID[1], _MID[2]), size=(1.2, 3.0), scene="corner")]
_HOT = ((10.2, 10.8), (8.2, 8.8), (4.2, 4.8))
DET_LISTS = [spec("hot site", 5, (2, 2, 1), 1, 64, scene="hot", centre=_HOT, size=(0.3, 0.9), exact=False),
             spec("hot site, exact", 5, (2, 2, 1), 1, 64, scene="hot", centre=_HOT, rounding=False),
             spec("many rows", 70, (3, 2, 5), 2, 6)]
CVT_TAILS = [spec(f"n_rows = {r} mod 4", 3, (2, 2, 1), 2, 4, n_sites=r) for r in (0, 1, 2, 3)]   # n_rows C = 0, 3, 2, 1 mod 4
LEVEL_SPECS = [spec(f"level {l}", 6, (3, 2, 2), 2, 9, scene=f"level{l}", scale=SCALE / 2 ** l) for l in range(4)]
DENSE_SPECS = [dict(s, C=c, scene="dense", name=f"dense C={c} {s['name']}") for c in (1, 5) for s in BINS + SUBSAMPLES]

GROUPS = dict(fwd_channels=FWD_CHANNELS, bwd_channels=BWD_CHANNELS, det_channels=DET_CHANNELS, bins=BINS,
              bwd_only_bins=BWD_ONLY_BINS, subsamples=SUBSAMPLES, lookup_far=LOOKUP_FAR, edges=EDGES, det_lists=DET_LISTS,
              cvt_tails=CVT_TAILS, levels=LEVEL_SPECS, dense=DENSE_SPECS)


def level_sites(sites, l):
    """the sites of pyramid level l: what a chain of l size-2 stride-2 convolutions leaves"""
    s = sites.copy()
    s[:, :3] >>= l
    return np.unique(s, axis=0)


def level_crop(crop, l):
    return tuple(((c - 1) >> l) + 1 for c in crop)


def scene_of(sp, rng):
    """-> sites, crop (= the occupied extent), spatial size, examples"""
    name = sp["scene"]
    if name == "far":
        s = far_sites(rng)
        return s, tuple(int(v) + 1 for v in s[:, :3].max(0)), FAR_SIZE, 1
    if name.startswith("level"):
        l = int(name[5:])
        s = level_sites(small_sites(np.random.RandomState(77)), l)
        return s[rng.permutation(s.shape[0])], level_crop(SMALL, l), tuple(v >> l for v in (64, 64, 32)), 2
    if name == "dense":
        crop = (9, 8, 6)
        b, y, x, z = np.meshgrid(np.arange(2), np.arange(crop[0]), np.arange(crop[1]), np.arange(crop[2]), indexing="ij")
        return np.stack([y.ravel(), x.ravel(), z.ravel(), b.ravel()], 1), crop, crop, 2
    s = small_sites(rng)
    if name == "corner":
        s = s[(s[:, 0] < 4) | ((s[:, 0] == H_ - 1) & (s[:, 1] == W_ - 1) & (s[:, 2] == Z_ - 1))]
    if name == "hot":
        hot = np.array([[10, 8, 4, 0], [11, 8, 4, 0], [10, 9, 5, 0]])
        s = np.unique(np.concatenate([s, hot]), axis=0)
        s = s[rng.permutation(s.shape[0])]
    if sp["n_sites"] is not None:
        keep = (s[:, 0] == H_ - 1) & (s[:, 1] == W_ - 1) & (s[:, 2] == Z_ - 1) & (s[:, 3] == 0)
        s = np.concatenate([s[keep], s[~keep]])
        n = 200 + sp["n_sites"]
        s = s[:n]
        assert s.shape[0] % 4 == sp["n_sites"]
    return s, SMALL, SMALL_SIZE, 2


def build_case(sp, exact, bf16, with_top=True):
    """-> dict(rois, map, crop, size, top, examples); the values of a rounding case in bf16 storage are bf16 numbers"""
    rng = np.random.RandomState(seed_of(sp["name"], sp["C"], sp["bins"], sp["sr"], sp["scene"], exact, bf16))
    sites, crop, size, nex = scene_of(sp, rng)
    C, K, bins = sp["C"], sp["K"], sp["bins"]
    scale, centre = sp["scale"], sp["centre"]
    if exact:
        g = sp["g"] if sp["sr"] <= 0 else (sp["sr"],) * 3
        assert _pow2(g)
        assert sp["sr"] > 0 or centre is None, "adaptive exact cases draw their centres over the map"
        rois = exact_rois(rng, K, bins, g, crop, nex, centre="adaptive" if sp["sr"] <= 0 else centre, scale=scale)
        feats = exact_values(rng, (sites.shape[0], C))
        top = exact_values(rng, (K, C) + bins) if with_top else None
    else:
        rois = rounding_rois(rng, K, bins, sp["sr"], crop, nex, size=sp["size"], centre=centre, g=sp["g"], scale=scale)
        feats = rounding_values(rng, sites.shape[0], C, bf16)
        top = rounding_values(rng, K * nb_of(bins), C, bf16).reshape((K,) + bins + (C,)) if with_top else None
        if top is not None:
            top = np.ascontiguousarray(np.moveaxis(top, -1, 1))
    return dict(rois=rois, map=SparseMap(sites, feats), crop=crop, size=size, top=top, examples=nex, scale=scale,
                bins=bins, sr=sp["sr"], C=C, K=K, name=sp["name"], exact=exact, bf16=bf16)


_CASES = {}


def cached_case(sp, exact, typ):
    """(case, reference) of a spec, built once and shared by the tests (never modified); the exact class holds the same
    numbers for both storage types"""
    key = (sp["name"], sp["C"], sp["bins"], sp["sr"], sp["scene"], exact, F32 if exact else typ)
    if key not in _CASES:
        case = build_case(sp, exact, typ == BF16)
        _CASES[key] = (case, reference(case))
    return _CASES[key]


def kinds(sp):
    return [e for e in (True, False) if sp["exact" if e else "rounding"]]


def reference(case, with_top=True):
    top = case["top"] if with_top else None
    return roi_ref(case["rois"], case["scale"], case["map"], case["crop"], case["bins"], case["sr"], top=top,
                   n_examples=case["examples"])
