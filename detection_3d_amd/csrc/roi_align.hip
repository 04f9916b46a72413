// a21. RoIAlignRotated3D forward (maskrcnn_benchmark/csrc/cuda/ROIAlignRotated3D_cuda.cu:15-177).
//  * dense variant: same contract as _C.roi_align_rotated_3d_forward (input [B,C,H,W,Z]);
//  * sparse variant: samples the SparseConvNetTensor through its hash grid, so the 1.07 GB dense
//    map of sparse_3d_to_dense_2d (sparseconvnet/tools_3d_2d.py:7-48) is never materialised.
// Both keep the reference's `zsize > zsize` bound quirk (:27): z above the map is clamped.
#include <algorithm>

#include "d3d_internal.h"

namespace d3d {

struct RoiGeom {
  int b;
  float cw, ch, cz, bh, bw, bz, sh, sw, sz, cosT, sinT;
  int gh, gw, gz;
};
__device__ __forceinline__ RoiGeom roi_geom(const float *r, float spatial_scale, int PH, int PW, int PZ,
                                            int sampling_ratio) {
  RoiGeom g;
  g.b = (int)r[0];
  g.cw = r[1] * spatial_scale;
  g.ch = r[2] * spatial_scale;
  g.cz = r[3] * spatial_scale;
  float rw = r[4] * spatial_scale, rh = r[5] * spatial_scale, rz = r[6] * spatial_scale;
  const float theta = (float)((double)r[7] * 3.14159265358979323846 / 180.0);
  rw = fmaxf(rw, 1.f);
  rh = fmaxf(rh, 1.f);
  rz = fmaxf(rz, 1.f);
  g.bh = rh / (float)PH;
  g.bw = rw / (float)PW;
  g.bz = rz / (float)PZ;
  g.gh = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rh / PH);
  g.gw = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rw / PW);
  g.gz = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rz / PZ);
  g.sh = (float)(-rh / 2.0);
  g.sw = (float)(-rw / 2.0);
  g.sz = (float)(-rz / 2.0);
  g.cosT = (float)cos((double)theta);
  g.sinT = (float)sin((double)theta);
  return g;
}
// sample position of (bin, sub-sample) in map coordinates (:150-163)
__device__ __forceinline__ void sample_pos(const RoiGeom &g, int ph, int pw, int pz, int iy, int ix,
                                           int iz, float &y, float &x, float &z) {
  const float yy = g.sh + ph * g.bh + (float)(iy + .5f) * g.bh / (float)g.gh;
  const float xx = g.sw + pw * g.bw + (float)(ix + .5f) * g.bw / (float)g.gw;
  const float zz = g.sz + pz * g.bz + (float)(iz + .5f) * g.bz / (float)g.gz;
  x = xx * g.cosT + yy * g.sinT + g.cw;
  y = yy * g.cosT - xx * g.sinT + g.ch;
  z = zz + g.cz;
}
// interpolation set-up of bilinear_interpolate (:15-62): returns false for an empty sample
struct Tri {
  int yl, yh, xl, xh, zl, zh;
  float ly, lx, lz, hy, hx, hz;
};
__device__ __forceinline__ bool tri_setup(float y, float x, float z, int H, int W, int Z, Tri &t) {
  if (y < -1.0 || y > H || x < -1.0 || x > W || z < -1.0) return false;
  if (y <= 0) y = 0;
  if (x <= 0) x = 0;
  if (z <= 0) z = 0;
  t.yl = (int)y;
  t.xl = (int)x;
  t.zl = (int)z;
  if (t.yl >= H - 1) { t.yh = t.yl = H - 1; y = (float)t.yl; } else t.yh = t.yl + 1;
  if (t.xl >= W - 1) { t.xh = t.xl = W - 1; x = (float)t.xl; } else t.xh = t.xl + 1;
  if (t.zl >= Z - 1) { t.zh = t.zl = Z - 1; z = (float)t.zl; } else t.zh = t.zl + 1;
  t.ly = y - t.yl;
  t.lx = x - t.xl;
  t.lz = z - t.zl;
  t.hy = 1. - t.ly;
  t.hx = 1. - t.lx;
  t.hz = 1. - t.lz;
  return true;
}

__global__ __launch_bounds__(256) void k_roi_dense(const float *__restrict__ input, int C, int H,
                                                   int W, int Z, const float *__restrict__ rois,
                                                   long nthreads, float spatial_scale, int PH, int PW,
                                                   int PZ, int sampling_ratio, float *__restrict__ out) {
  long index = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (index >= nthreads) return;
  const int pz = index % PZ;
  const int pw = (index / PZ) % PW;
  const int ph = (index / PZ / PW) % PH;
  const int c = (index / PZ / PW / PH) % C;
  const int n = index / PZ / PW / PH / C;
  const RoiGeom g = roi_geom(rois + (size_t)n * 8, spatial_scale, PH, PW, PZ, sampling_ratio);
  const float *d = input + ((size_t)g.b * C + c) * H * W * Z;
  const float count = (float)(g.gh * g.gw * g.gz);
  float acc = 0.f;
  for (int iy = 0; iy < g.gh; iy++)
    for (int ix = 0; ix < g.gw; ix++)
      for (int iz = 0; iz < g.gz; iz++) {
        float y, x, z;
        sample_pos(g, ph, pw, pz, iy, ix, iz, y, x, z);
        Tri t;
        if (!tri_setup(y, x, z, H, W, Z, t)) continue;
        const float v1 = d[(t.yl * W + t.xl) * Z + t.zl], v2 = d[(t.yl * W + t.xh) * Z + t.zl];
        const float v3 = d[(t.yh * W + t.xl) * Z + t.zl], v4 = d[(t.yh * W + t.xh) * Z + t.zl];
        const float v5 = d[(t.yl * W + t.xl) * Z + t.zh], v6 = d[(t.yl * W + t.xh) * Z + t.zh];
        const float v7 = d[(t.yh * W + t.xl) * Z + t.zh], v8 = d[(t.yh * W + t.xh) * Z + t.zh];
        const float w1 = t.hy * t.hx * t.hz, w2 = t.hy * t.lx * t.hz, w3 = t.ly * t.hx * t.hz, w4 = t.ly * t.lx * t.hz;
        const float w5 = t.hy * t.hx * t.lz, w6 = t.hy * t.lx * t.lz, w7 = t.ly * t.hx * t.lz, w8 = t.ly * t.lx * t.lz;
        acc += (w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4 + w5 * v5 + w6 * v6 + w7 * v7 + w8 * v8);
      }
  out[index] = acc / count;
}

// Sparse variant.  Block = one RoI x one chunk of 128 channels (lane = 2 adjacent channels); a wave owns
// groups of kRoiG consecutive bins.  Per group and per step of 8 sub-samples the 64 lanes first resolve
// (sub-sample, corner) -> (row, weight) through the hash grid for all kRoiG bins at once (kRoiG independent
// probes in flight per lane), merge the taps that fall into one cell into a per-bin list in LDS (cells in
// order of their first lane; the cells are found with v_readlane, their weights summed in batches of kRoiB
// independent register-only butterflies, roi_cells4_sum), and then every lane accumulates its two channels
// over the lists with 8 independent feature-row loads in flight (each a coalesced 512-B read of the wave).
// Everything is latency-bound L2 traffic: the feature map of a pyramid level is a few MB; what matters is the
// number of loads in flight, not bytes.
// layout 0: out[n][c][ph][pw][pz] (the reference's); layout 1: out[n][ph][pw][c][pz] (rows of the box head's
// [1,1,pz] convolution seen as a GEMM).  roi_levels (optional): only RoIs with roi_levels[i] == level are pooled.
// kRoiG: 4 bins per group and 4 waves per SIMD (128 VGPRs, 4 spilled).  Measured on the bench's 1000 RoIs (4.98 merged
// cells per bin and step on average, 231 ... 1952 per RoI): the launch takes 0.64 of the cycles it took
// with the merge as one loop per cell of seven dependent ds_bpermute round trips (about 70 cycles each, a third of a
// wave's life).  What is left: a wave waits 39 % of its cycles (probes, row loads) and issues VALU instructions in
// 27 %, and the launch lasts twice the mean life of its waves -- a single round of workgroups over RoIs of unequal
// size.
static constexpr int kRoiG = 4;
static constexpr int kRoiCch = 128;
__device__ __forceinline__ void roi_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
static constexpr int kRoiWaves = 4;  // waves per RoI (8 measured the same; what helps is waves per SIMD, see kRoiG)
static constexpr int kRoiB = 8;      // merged cells whose weight sums run as independent chains (two roi_cells4_sum)

// The wave-wide sums of four lane vectors a, b, c, d, each added in the pairing of the xor butterfly
// `for (d = 32; d >= 1; d >>= 1) w += __shfl_xor(w, d)` (lane i with lane i ^ 32, then ^ 16, ... ^ 1; fp32 addition is
// commutative, so the pairing alone fixes the bits), without LDS and with one chain for the four:
//  * level 32: v_permlane32_swap exchanges the upper half of a with the lower half of b, so the sum of the two results
//    holds a's level in lanes 0-31 and b's in lanes 32-63 (a lane's partner at this level holds the same number);
//  * level 16: v_permlane16_swap exchanges the odd rows (of 16 lanes) of the first operand with the even rows of the
//    second: the sum holds a, c, b, d in rows 0, 1, 2, 3;
//  * levels 8, 4, 2, 1 stay inside a row: DPP row_ror:8 is lane ^ 8, row_half_mirror (lane ^ 7) followed by quad_perm
//    [3,2,1,0] (lane ^ 3) is lane ^ 4, quad_perm [2,3,0,1] and [1,0,3,2] are lane ^ 2 and lane ^ 1.
// Every lane of row 0 returns the sum of a, of row 1 that of c, of row 2 that of b, of row 3 that of d.  All 64 lanes
// must be active.
template <int CTRL>
__device__ __forceinline__ float roi_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float roi_pack32(float a, float b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float roi_pack16(float p, float q) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(p), __float_as_uint(q), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float roi_cells4_sum(float a, float b, float c, float d) {
  float v = roi_pack16(roi_pack32(a, b), roi_pack32(c, d));
  v += roi_dpp<0x128>(v);                  // row_ror:8
  v += roi_dpp<0x1B>(roi_dpp<0x141>(v));   // row_half_mirror, then quad_perm [3,2,1,0]
  v += roi_dpp<0x4E>(v);                   // quad_perm [2,3,0,1]
  v += roi_dpp<0xB1>(v);                   // quad_perm [1,0,3,2]
  return v;
}
// One launch serves every pyramid level: a RoI's workgroup picks the map of roi_levels[n] (a launch per level leaves
// the workgroups of the other levels' RoIs to exit at once -- with two levels each launch fills half the wave slots).
struct RoiLevel {
  const HashEntry *tab;   // null: this level is not pooled by the launch
  const void *feats;      // rows of the launch's storage type T
  const int32_t *extent;  // occupied extent of the grid on the device, or null: H, W, Z below
  const int32_t *dense;   // null, or the dense index of the grid's bounding box [b][e0][e1][e2] (1 + site id, 0 = empty)
  int cap, H, W, Z;
  int e0, e1, e2;
  float scale;
};
static constexpr int kRoiMaxLevels = 4;
struct RoiLevels {
  RoiLevel v[kRoiMaxLevels];
};
// T = storage type of the feature rows and of the output: float, or unsigned short (bf16 bits: the rows are widened as
// they are read, the taps are summed in fp32 in the same order, and the bin's mean is rounded once at the store, so the
// result is the fp32 kernel's on the widened map, rounded to bf16).
template <typename T>
__global__ __launch_bounds__(kRoiWaves * 64) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_roi_sparse(
    RoiLevels lv, int C, const float *__restrict__ rois, const int32_t *__restrict__ roi_levels,
    int PH, int PW, int PZ, int sampling_ratio, int layout, T *__restrict__ out) {
  const int n = blockIdx.x, cc = blockIdx.y;
  const int l = roi_levels ? __builtin_amdgcn_readfirstlane(roi_levels[n]) : 0;
  if (l < 0 || l >= kRoiMaxLevels) return;   // -1: a padding row (d3d_roi_prepare_counted)
  RoiLevel L = lv.v[0];                       // selects, not an indexed copy of the argument block
  if (l == 1) L = lv.v[1];
  if (l == 2) L = lv.v[2];
  if (l == 3) L = lv.v[3];
  if (!L.tab) return;                         // pooled from another pyramid level (by another launch)
  const HashEntry *__restrict__ tab = L.tab;
  const int32_t *__restrict__ dense = L.dense;
  const T *__restrict__ feats = (const T *)L.feats;
  const int cap = L.cap;
  const float spatial_scale = L.scale;
  int H = L.H, W = L.W, Z = L.Z;
  if (L.extent) {  // crop = occupied extent of the grid, read on the device (no host round trip)
    H = L.extent[0];
    W = L.extent[1];
    Z = L.extent[2];
  }
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  __shared__ int2 list[kRoiWaves][kRoiG * 64];  // (row, weight bits) of a step's merged cells, bin after bin
  const int NB = PH * PW * PZ;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const RoiGeom g = roi_geom(rois + (size_t)n * 8, spatial_scale, PH, PW, PZ, sampling_ratio);
  const int NS = g.gh * g.gw * g.gz;
  const float count = (float)NS;
  const int c0 = cc * kRoiCch + 2 * lane;
  const bool ok0 = c0 < C, ok1 = c0 + 1 < C;
  const bool pair = ok1 && (C % 2 == 0);  // 8-byte aligned pair load
  const size_t n_out = (size_t)n;
  auto load2 = [&](int row) -> f32x2 {
    const T *p = feats + (size_t)row * C + c0;
    f32x2 v = {0.f, 0.f};
    if (pair) {
      if constexpr (sizeof(T) == 4) {
        v = *(const f32x2 *)p;
      } else {
        const unsigned u = *(const unsigned *)p;   // two bf16 channels: 4-byte aligned (C even)
        v[0] = __uint_as_float(u << 16);
        v[1] = __uint_as_float(u & 0xffff0000u);
      }
    } else {
      if (ok0) v[0] = ld1(p);
      if (ok1) v[1] = ld1(p + 1);
    }
    return v;
  };
  // layout 1 with PZ == kRoiG, a whole chunk of channels and an aligned result: a lane's kRoiG bins of a channel are
  // consecutive, 16 bytes of fp32 or 8 of bf16 (the offset of a group is a multiple of that: kRoiG elements per channel)
  static_assert(kRoiG == 4, "the wide store writes four bins per channel");
  const bool wide = layout == 1 && PZ == kRoiG && (cc + 1) * kRoiCch <= C &&
                    ((uintptr_t)out & (kRoiG * sizeof(T) - 1)) == 0;
  const int ngroups = (NB + kRoiG - 1) / kRoiG;
  for (int grp = wave; grp < ngroups; grp += kRoiWaves) {
    const int b0 = grp * kRoiG;
    f32x2 acc[kRoiG];
#pragma unroll
    for (int gi = 0; gi < kRoiG; gi++) acc[gi] = {0.f, 0.f};
    for (int s0 = 0; s0 < NS; s0 += 8) {
      // ---- lanes = (sub-sample s0 + lane/8, corner lane%8), kRoiG bins at once ----
      const int s = s0 + (lane >> 3), corner = lane & 7;
      const int iz = s % g.gz, ix = (s / g.gz) % g.gw, iy = s / (g.gz * g.gw);
      const int zb = corner >> 2, yb = (corner >> 1) & 1, xb = corner & 1;
      int row[kRoiG];
      float wgt[kRoiG];
      // the probes of a lane four bins at a time in lockstep (hash_find_n: their round trips overlap; all kRoiG at
      // once costs a wave of occupancy in registers)
      static_assert(kRoiG % 4 == 0, "probe groups of four");
#pragma unroll
      for (int g0 = 0; g0 < kRoiG; g0 += 4) {
        uint64_t key[4];
        bool want[4];
        int r4[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int bin = b0 + g0 + j;
          wgt[g0 + j] = 0.f;
          key[j] = 0;
          want[j] = false;
          if (s < NS && bin < NB) {
            const int pz = bin % PZ, pw = (bin / PZ) % PW, ph = bin / (PZ * PW);
            float y, x, z;
            sample_pos(g, ph, pw, pz, iy, ix, iz, y, x, z);
            Tri t;
            if (tri_setup(y, x, z, H, W, Z, t)) {
              wgt[g0 + j] = (yb ? t.ly : t.hy) * (xb ? t.lx : t.hx) * (zb ? t.lz : t.hz);
              // dense index [y][x][z]: y runs over the tensor's 1st spatial axis, x over the 2nd
              key[j] = pack_key(g.b, yb ? t.yh : t.yl, xb ? t.xh : t.xl, zb ? t.zh : t.zl);
              want[j] = true;
            }
          }
        }
        if (dense) {       // one load per corner: the cell of the grid's dense index (coordinates are inside the box:
                           // tri_setup clamps them to the occupied extent, which the box contains)
          int v4[4];
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const uint64_t kk = key[j];
            const size_t cell = ((((size_t)(kk >> 48) * L.e0 + (size_t)((kk >> 32) & 0xffff)) * L.e1 +
                                  (size_t)((kk >> 16) & 0xffff)) * L.e2 + (size_t)(kk & 0xffff));
            v4[j] = want[j] ? dense[cell] : 0;
          }
#pragma unroll
          for (int j = 0; j < 4; j++) r4[j] = v4[j] - 1;
        } else {
          hash_find_n<4>(tab, cap, key, want, r4);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) row[g0 + j] = r4[j];
      }
      // the 64 taps of a bin fall into a handful of cells (its sub-samples are a fraction of a cell apart): merge
      // the taps of one cell (weights summed in the pairing of a wave butterfly) so that each feature row is fetched
      // once per bin and step.
      // Leader pass (no LDS): the cells of a bin in order of their first lane.  The leader's row comes through a
      // scalar-indexed v_readlane; every lane learns the index of its cell in the step's list (the kRoiG bins' cells
      // one after another: bin gi owns [base[gi], base[gi] + cnt[gi])), lane j of cellrow[gi] the row of the bin's cell j.
      int2 *lst = list[wave];
      int cnt[kRoiG], base[kRoiG], flat[kRoiG];
      int total = 0;
#pragma unroll
      for (int gi = 0; gi < kRoiG; gi++) {
        unsigned long long m = __ballot(row[gi] >= 0);
        int c = 0, fl = -1, cellrow = 0;
        while (m) {
          const int rl = __builtin_amdgcn_readlane(row[gi], __builtin_ctzll(m));   // wave-uniform cell
          const bool mine = row[gi] == rl;
          fl = mine ? total + c : fl;
          cellrow = lane == c ? rl : cellrow;
          c++;
          m &= ~__ballot(mine);
        }
        if (lane < c) lst[total + lane].x = cellrow;
        flat[gi] = fl;
        base[gi] = total;
        cnt[gi] = c;
        total += c;
      }
      // Weight sums, kRoiB cells of the list per batch: every cell's sum is the xor butterfly of the serial form (levels
      // 32 ... 1 over `mine ? wgt : 0`), but the chains of a batch are independent and none of them goes through LDS
      // (roi_cells4_sum).  A batch may straddle bins; only the bins it touches are looked at.
      for (int f0 = 0; f0 < total; f0 += kRoiB) {
        float sm[kRoiB];
#pragma unroll
        for (int k = 0; k < kRoiB; k++) sm[k] = 0.f;
#pragma unroll
        for (int gi = 0; gi < kRoiG; gi++) {
          if (base[gi] < f0 + kRoiB && base[gi] + cnt[gi] > f0) {   // wave-uniform
            const int e = flat[gi] - f0;
#pragma unroll
            for (int k = 0; k < kRoiB; k++) sm[k] = e == k ? wgt[gi] : sm[k];
          }
        }
#pragma unroll
        for (int h = 0; h < kRoiB; h += 4) {
          const float w = roi_cells4_sum(sm[h], sm[h + 1], sm[h + 2], sm[h + 3]);
          const int q = lane >> 4;                                  // rows of 16 lanes hold cells h + 0, 2, 1, 3
          const int f = f0 + h + (((q & 1) << 1) | (q >> 1));
          if ((lane & 15) == 0 && f < total) lst[f].y = __float_as_int(w);
        }
      }
      roi_wave_sync();
      // ---- lanes = channel pairs: one entry per cell, batches of independent row loads ----
#pragma unroll
      for (int gi = 0; gi < kRoiG; gi++) {
        const int2 *L = lst + base[gi];
        const int nc = cnt[gi];
        int i = 0;
        for (; i + 8 <= nc; i += 8) {
          int2 e[8];
          f32x2 v[8];
#pragma unroll
          for (int j = 0; j < 8; j++) e[j] = L[i + j];
#pragma unroll
          for (int j = 0; j < 8; j++) v[j] = load2(e[j].x);
#pragma unroll
          for (int j = 0; j < 8; j++) acc[gi] += __int_as_float(e[j].y) * v[j];
        }
        if (i + 4 <= nc) {
          int2 e[4];
          f32x2 v[4];
#pragma unroll
          for (int j = 0; j < 4; j++) e[j] = L[i + j];
#pragma unroll
          for (int j = 0; j < 4; j++) v[j] = load2(e[j].x);
#pragma unroll
          for (int j = 0; j < 4; j++) acc[gi] += __int_as_float(e[j].y) * v[j];
          i += 4;
        }
        if (i + 2 <= nc) {
          const int2 e0 = L[i], e1 = L[i + 1];
          const f32x2 v0 = load2(e0.x), v1 = load2(e1.x);
          acc[gi] += __int_as_float(e0.y) * v0;
          acc[gi] += __int_as_float(e1.y) * v1;
          i += 2;
        }
        if (i < nc) {
          const int2 e0 = L[i];
          acc[gi] += __int_as_float(e0.y) * load2(e0.x);
        }
      }
      roi_wave_sync();  // the lists are rewritten by the next step
    }
    if (wide) {   // the group is the pz run of one (ph, pw) cell: kRoiG consecutive outputs per channel, one store each
      f32x2 r[kRoiG];
#pragma unroll
      for (int gi = 0; gi < kRoiG; gi++) r[gi] = acc[gi] / count;
      T *o = out + ((n_out * (size_t)(PH * PW) + grp) * C + c0) * kRoiG;
#pragma unroll
      for (int ch = 0; ch < 2; ch++) {
        if constexpr (sizeof(T) == 4) {
          const d3d_f32x4 v = {r[0][ch], r[1][ch], r[2][ch], r[3][ch]};
          *(d3d_f32x4 *)(o + ch * kRoiG) = v;
        } else {
          unsigned short h[kRoiG];
#pragma unroll
          for (int gi = 0; gi < kRoiG; gi++) st1(&h[gi], r[gi][ch]);
          *(uint2 *)(o + ch * kRoiG) = make_uint2(h[0] | (unsigned)h[1] << 16, h[2] | (unsigned)h[3] << 16);
        }
      }
      continue;
    }
#pragma unroll
    for (int gi = 0; gi < kRoiG; gi++) {
      const int bin = b0 + gi;
      if (bin >= NB) break;
      const f32x2 r = acc[gi] / count;
      if (layout == 0) {
        T *o = out + (n_out * C + c0) * NB + bin;
        if (ok0) st1(o, r[0]);
        if (ok1) st1(o + NB, r[1]);
      } else {
        const int pz = bin % PZ, cell = bin / PZ;
        T *o = out + ((n_out * (size_t)(PH * PW) + cell) * C + c0) * PZ + pz;
        if (ok0) st1(o, r[0]);
        if (ok1) st1(o + PZ, r[1]);
      }
    }
  }
}

// Dense backward, _C.roi_align_rotated_3d_backward (ROIAlignRotated3D_cuda.cu:238-354): one thread per
// pooled element, 8 fp32 atomics per sub-sample into the zeroed dense gradient.
__global__ __launch_bounds__(256) void k_roi_dense_bwd(const float *__restrict__ top_diff, int C, int H, int W,
                                                       int Z, const float *__restrict__ rois, long nthreads,
                                                       float spatial_scale, int PH, int PW, int PZ,
                                                       int sampling_ratio, float *__restrict__ bottom_diff) {
  long index = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (index >= nthreads) return;
  const int pz = index % PZ;
  const int pw = (index / PZ) % PW;
  const int ph = (index / PZ / PW) % PH;
  const int c = (index / PZ / PW / PH) % C;
  const int n = index / PZ / PW / PH / C;
  const RoiGeom g = roi_geom(rois + (size_t)n * 8, spatial_scale, PH, PW, PZ, sampling_ratio);
  float *d = bottom_diff + ((size_t)g.b * C + c) * H * W * Z;
  const float count = (float)(g.gh * g.gw * g.gz);
  const float top = top_diff[index];
  for (int iy = 0; iy < g.gh; iy++)
    for (int ix = 0; ix < g.gw; ix++)
      for (int iz = 0; iz < g.gz; iz++) {
        float y, x, z;
        sample_pos(g, ph, pw, pz, iy, ix, iz, y, x, z);
        Tri t;
        if (z > Z || !tri_setup(y, x, z, H, W, Z, t)) continue;   // backward bound test (:190)
        const float w[8] = {t.hy * t.hx * t.hz, t.hy * t.lx * t.hz, t.ly * t.hx * t.hz, t.ly * t.lx * t.hz,
                            t.hy * t.hx * t.lz, t.hy * t.lx * t.lz, t.ly * t.hx * t.lz, t.ly * t.lx * t.lz};
#pragma unroll
        for (int q = 0; q < 8; q++) {
          const int yy = (q >> 1) & 1 ? t.yh : t.yl, xx = q & 1 ? t.xh : t.xl, zz = q >> 2 ? t.zh : t.zl;
          atomicAdd(d + ((size_t)yy * W + xx) * Z + zz, top * w[q] / count);
        }
      }
}

// Backward of the sparse variant: the dense gradient of RoIAlignRotated3DBackwardFeature (:238-354)
// restricted to the active sites (what SparseToDense_updateGradInput would gather back).  Keeps the
// backward's own bound test `z > zsize` (:190).  fp32 atomics, like the reference.  TT = storage type of top_diff
// (float, or bf16 bits widened as they are read); d_feats is fp32 either way.
static constexpr int kRoiBwdCch = 64;
template <typename TT>
__global__ __launch_bounds__(256) void k_roi_sparse_bwd(
    const HashEntry *__restrict__ tab, int cap, int C, int H, int W, int Z, const float *__restrict__ rois,
    float spatial_scale, int PH, int PW, int PZ, int sampling_ratio, const TT *__restrict__ top_diff,
    float *__restrict__ d_feats) {
  extern __shared__ float tile[];  // [kRoiBwdCch][NB + 1]
  const int n = blockIdx.x, cc = blockIdx.y;
  const int NB = PH * PW * PZ, LD = NB + 1;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nch = min(kRoiBwdCch, C - cc * kRoiBwdCch);
  const TT *g0 = top_diff + ((size_t)n * C + (size_t)cc * kRoiBwdCch) * NB;
  for (int idx = threadIdx.x; idx < nch * NB; idx += 256) tile[(idx / NB) * LD + idx % NB] = ld1(g0 + idx);
  __syncthreads();
  const RoiGeom g = roi_geom(rois + (size_t)n * 8, spatial_scale, PH, PW, PZ, sampling_ratio);
  const int NS = g.gh * g.gw * g.gz;
  const float count = (float)NS;
  const int c = cc * kRoiBwdCch + lane;
  const bool cok = c < C;
  for (int bin = wave; bin < NB; bin += 4) {
    const int pz = bin % PZ, pw = (bin / PZ) % PW, ph = bin / (PZ * PW);
    const float top = cok ? tile[lane * LD + bin] : 0.f;
    for (int s0 = 0; s0 < NS; s0 += 8) {
      const int s = s0 + (lane >> 3), corner = lane & 7;
      int row = -1;
      float wgt = 0.f;
      if (s < NS) {
        const int iz = s % g.gz, ix = (s / g.gz) % g.gw, iy = s / (g.gz * g.gw);
        float y, x, z;
        sample_pos(g, ph, pw, pz, iy, ix, iz, y, x, z);
        Tri t;
        if (!(z > Z) && tri_setup(y, x, z, H, W, Z, t)) {
          const int zb = corner >> 2, yb = (corner >> 1) & 1, xb = corner & 1;
          wgt = (yb ? t.ly : t.hy) * (xb ? t.lx : t.hx) * (zb ? t.lz : t.hz);
          row = hash_find(tab, cap, pack_key(g.b, yb ? t.yh : t.yl, xb ? t.xh : t.xl, zb ? t.zh : t.zl));
        }
      }
      // the 64 taps of a step fall into a handful of cells: one atomic per (cell, channel) with the taps' weights summed
      // by a wave butterfly (as the forward does) instead of one per tap -- 5x fewer atomics on the hot rows
      unsigned long long m = __ballot(row >= 0);
      while (m) {
        const int rr = __shfl(row, __builtin_ctzll(m), 64);   // wave-uniform cell
        const bool mine = row == rr;
        float ww = mine ? wgt : 0.f;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) ww += __shfl_xor(ww, d, 64);
        if (cok) atomicAdd(d_feats + (size_t)rr * C + c, top * ww / count);
        m &= ~__ballot(mine);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// Fixed-order form of the sparse backward (d3d_roi_align_rotated_3d_sparse_backward_deterministic): no float atomics.
//  1. taps -> records.  k_roi_det_taps walks the taps exactly as k_roi_sparse_bwd does and merges the taps of one step
//     (8 sub-samples x 8 corners) that land in one cell by the same wave butterfly; every merged cell is one record
//     (destination row, source (RoI, bin), weight / count).  A counting pass and a scan place the records (record order
//     = (RoI, bin, step, first lane of the cell)); a second pass writes them.
//  2. inverted index: a stable radix sort of the records by destination row (sort_pairs_u32), so the records of a row
//     keep their order; k_roi_det_bounds marks where each row's list begins and ends.
//  3. sum: the sorted list is cut into chunks of kRoiDetChunk records at fixed positions; one wave sums a chunk over all
//     channels in list order (top_diff transposed to [K, NB, C] first, so a record's channels are one contiguous row).
//     A row wholly inside its chunk is added to d_feats at once; the (at most two) rows a chunk shares with its
//     neighbours leave a partial, and k_roi_det_join adds a long row's partials in chunk order.  The summation order
//     is a function of the records alone: not of the grid size, the wave schedule or the number of CUs.
static constexpr int kRoiDetChunk = 64;   // records per chunk = lanes of a wave (one cooperative load of the chunk)
static constexpr int kRoiDetCpl = 4;      // channels per lane in one pass over a chunk (256 channels)

// [K][C][NB] -> [K][NB][C] through a 32 x 33 tile (TT: float, or bf16 bits widened to fp32)
template <typename TT>
__global__ __launch_bounds__(256) void k_roi_det_transpose(const TT *__restrict__ in, int C, int NB,
                                                           float *__restrict__ out) {
  __shared__ float t[32][33];
  const int n = blockIdx.x, b0 = blockIdx.y * 32, c0 = blockIdx.z * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const TT *src = in + (size_t)n * C * NB;
  for (int j = ty; j < 32; j += 8) {
    const int c = c0 + j, b = b0 + tx;
    t[j][tx] = (c < C && b < NB) ? ld1(src + (size_t)c * NB + b) : 0.f;
  }
  __syncthreads();
  float *dst = out + (size_t)n * NB * C;
  for (int j = ty; j < 32; j += 8) {
    const int b = b0 + j, c = c0 + tx;
    if (c < C && b < NB) dst[(size_t)b * C + c] = t[tx][j];
  }
}

// WRITE = false: cnt[n * NB + bin] = records of (n, bin).  WRITE = true: the records at offs[n * NB + bin] ...
// Rows outside [0, n_rows) are not taps (they cannot occur: the grid numbers its n_rows sites).
template <bool WRITE>
__global__ __launch_bounds__(256) void k_roi_det_taps(
    const HashEntry *__restrict__ tab, int cap, int H, int W, int Z, const float *__restrict__ rois,
    float spatial_scale, int PH, int PW, int PZ, int sampling_ratio, int n_rows, int32_t *__restrict__ cnt,
    const int32_t *__restrict__ offs, uint32_t *__restrict__ rec_key, int32_t *__restrict__ rec_val,
    int32_t *__restrict__ rec_src, float *__restrict__ rec_w) {
  const int n = blockIdx.x;
  const int NB = PH * PW * PZ;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const RoiGeom g = roi_geom(rois + (size_t)n * 8, spatial_scale, PH, PW, PZ, sampling_ratio);
  const int NS = g.gh * g.gw * g.gz;
  const float count = (float)NS;
  for (int bin = wave; bin < NB; bin += 4) {
    const int pz = bin % PZ, pw = (bin / PZ) % PW, ph = bin / (PZ * PW);
    const int src = n * NB + bin;
    int pos = WRITE ? offs[src] : 0;
    for (int s0 = 0; s0 < NS; s0 += 8) {
      const int s = s0 + (lane >> 3), corner = lane & 7;
      int row = -1;
      float wgt = 0.f;
      if (s < NS) {
        const int iz = s % g.gz, ix = (s / g.gz) % g.gw, iy = s / (g.gz * g.gw);
        float y, x, z;
        sample_pos(g, ph, pw, pz, iy, ix, iz, y, x, z);
        Tri t;
        if (!(z > Z) && tri_setup(y, x, z, H, W, Z, t)) {
          const int zb = corner >> 2, yb = (corner >> 1) & 1, xb = corner & 1;
          wgt = (yb ? t.ly : t.hy) * (xb ? t.lx : t.hx) * (zb ? t.lz : t.hz);
          row = hash_find(tab, cap, pack_key(g.b, yb ? t.yh : t.yl, xb ? t.xh : t.xl, zb ? t.zh : t.zl));
          if (row >= n_rows) row = -1;
        }
      }
      unsigned long long m = __ballot(row >= 0);
      while (m) {
        const int rr = __shfl(row, __builtin_ctzll(m), 64);   // wave-uniform cell, cells in order of their first lane
        const bool mine = row == rr;
        if (WRITE) {
          float ww = mine ? wgt : 0.f;
#pragma unroll
          for (int d = 32; d >= 1; d >>= 1) ww += __shfl_xor(ww, d, 64);
          if (lane == 0) {
            rec_key[pos] = (uint32_t)rr;
            rec_val[pos] = pos;
            rec_src[pos] = src;
            rec_w[pos] = ww / count;
          }
        }
        pos++;
        m &= ~__ballot(mine);
      }
    }
    if (!WRITE && lane == 0) cnt[src] = pos;
  }
}

// rbeg[row] / rend[row]: the row's list in the sorted records (rows without records keep 0 / 0)
__global__ __launch_bounds__(256) void k_roi_det_bounds(const uint32_t *__restrict__ skey, int n_max,
                                                        const int32_t *__restrict__ total, int32_t *__restrict__ rbeg,
                                                        int32_t *__restrict__ rend) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int n = *total;
  if (i >= n || i >= n_max) return;
  const uint32_t k = skey[i];
  if (i == 0 || skey[i - 1] != k) rbeg[k] = i;
  if (i == n - 1 || skey[i + 1] != k) rend[k] = i + 1;
}

// one wave per chunk [a, a + kRoiDetChunk) of the sorted records: lane j loads record a + j, then the wave walks the
// chunk in order, all channels at once (lane = channels lane, lane + 64, ...).  A run of one row that is the whole of
// the row's list goes to d_feats; otherwise it is the chunk's first run (slot 0) or last run (slot 1) and goes to
// part[chunk][slot].  TO = float: d_feats is added to; TO = bf16 bits: the row's sum is rounded and written (the row was
// zeroed: 0 + sum is the sum itself, as a sum that starts from +0 is never -0).
template <typename TO>
__global__ __launch_bounds__(256) void k_roi_det_sum(const uint32_t *__restrict__ skey, const int32_t *__restrict__ sval,
                                                     const int32_t *__restrict__ rec_src, const float *__restrict__ rec_w,
                                                     int n_max, const int32_t *__restrict__ total,
                                                     const int32_t *__restrict__ rbeg, const int32_t *__restrict__ rend,
                                                     const float *__restrict__ topT, int C, float *__restrict__ part,
                                                     TO *__restrict__ d_feats) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + wave;
  const int a = chunk * kRoiDetChunk;
  const int n = min(*total, n_max);
  if (a >= n) return;
  const int len = min(kRoiDetChunk, n - a);
  int my_key = -1, my_src = 0;
  float my_w = 0.f;
  if (lane < len) {
    my_key = (int)skey[a + lane];
    const int v = sval[a + lane];
    my_src = rec_src[v];
    my_w = rec_w[v];
  }
  for (int cb = 0; cb < C; cb += 64 * kRoiDetCpl) {
    float acc[kRoiDetCpl];
#pragma unroll
    for (int j = 0; j < kRoiDetCpl; j++) acc[j] = 0.f;
    int cur = __shfl(my_key, 0, 64), seg = 0;
    auto flush = [&](int row, int sa, int sb) {
      const bool whole = rbeg[row] == a + sa && rend[row] == a + sb;
      if (whole) {
        TO *dst = d_feats + (size_t)row * C;
#pragma unroll
        for (int j = 0; j < kRoiDetCpl; j++) {
          const int c = cb + lane + 64 * j;
          if (c < C) {
            if constexpr (sizeof(TO) == 4) dst[c] = dst[c] + acc[j];
            else st1(dst + c, acc[j]);
          }
          acc[j] = 0.f;
        }
      } else {
        float *dst = part + ((size_t)chunk * 2 + (sa == 0 ? 0 : 1)) * C;
#pragma unroll
        for (int j = 0; j < kRoiDetCpl; j++) {
          const int c = cb + lane + 64 * j;
          if (c < C) dst[c] = acc[j];
          acc[j] = 0.f;
        }
      }
    };
    for (int p0 = 0; p0 < len; p0 += 4) {
      int key[4], src[4];
      float w[4], v[4][kRoiDetCpl];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        key[q] = __shfl(my_key, p0 + q, 64);
        src[q] = __shfl(my_src, p0 + q, 64);
        w[q] = __shfl(my_w, p0 + q, 64);
      }
#pragma unroll
      for (int q = 0; q < 4; q++)
#pragma unroll
        for (int j = 0; j < kRoiDetCpl; j++) {
          const int c = cb + lane + 64 * j;
          v[q][j] = (p0 + q < len && c < C) ? topT[(size_t)src[q] * C + c] : 0.f;
        }
#pragma unroll
      for (int q = 0; q < 4; q++) {
        if (p0 + q >= len) break;
        if (key[q] != cur) {
          flush(cur, seg, p0 + q);
          cur = key[q];
          seg = p0 + q;
        }
#pragma unroll
        for (int j = 0; j < kRoiDetCpl; j++) acc[j] += w[q] * v[q][j];
      }
    }
    flush(cur, seg, len);
  }
}

// one wave per row whose list spans several chunks: d_feats[row] += its chunk partials, in chunk order (TO as in
// k_roi_det_sum)
template <typename TO>
__global__ __launch_bounds__(256) void k_roi_det_join(const int32_t *__restrict__ rbeg, const int32_t *__restrict__ rend,
                                                      int n_rows, const float *__restrict__ part, int C,
                                                      TO *__restrict__ d_feats) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n_rows) return;
  const int rb = rbeg[row], re = rend[row];
  if (re <= rb) return;
  const int c0 = rb / kRoiDetChunk, c1 = (re - 1) / kRoiDetChunk;
  if (c0 == c1) return;
  for (int c = lane; c < C; c += 64) {
    float acc = 0.f;
    for (int k = c0; k <= c1; k++) {
      const int slot = (k == c0 && rb != k * kRoiDetChunk) ? 1 : 0;
      acc += part[((size_t)k * 2 + slot) * C + c];
    }
    if constexpr (sizeof(TO) == 4) d_feats[(size_t)row * C + c] += acc;
    else st1(d_feats + (size_t)row * C + c, acc);
  }
}

// fp32 -> bf16 (round to nearest even), n elements; in 16-byte and out 8-byte aligned (checked by the caller)
__global__ __launch_bounds__(256) void k_roi_f32_to_bf16(const float *__restrict__ in, long n,
                                                         unsigned short *__restrict__ out) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i + 4 <= n)
    store4(out + i, load4<float>(in + i));
  else
    for (long j = i; j < n; j++) st1(out + j, in[j]);
}

// scratch layout of the fixed-order backward (offsets from a 256-aligned base)
struct RoiDetLayout {
  size_t cnt, offs, total, scan, rkey, rval, rsrc, rw, skey, sval, sort, rbeg, rend, topT, part, bytes;
  size_t scan_bytes, sort_bytes;
  long n_max, n_src, n_chunks;
  int bits;
};
static bool roi_det_layout(int K, int C, int ph, int pw, int pz, int sampling_ratio, int n_rows, RoiDetLayout &L) {
  if (K < 0 || C <= 0 || ph <= 0 || pw <= 0 || pz <= 0 || sampling_ratio <= 0 || n_rows < 0) return false;
  const long NB = (long)ph * pw * pz, NS = (long)sampling_ratio * sampling_ratio * sampling_ratio;
  L.n_src = (long)K * NB;
  L.n_max = L.n_src * NS * 8;   // a record holds at least one of the 8 NS taps of its bin
  if (L.n_max >= (1L << 31) - kRoiDetChunk) return false;
  L.n_chunks = (L.n_max + kRoiDetChunk - 1) / kRoiDetChunk;
  L.bits = 1;
  while (L.bits < 31 && (1L << L.bits) < (long)n_rows) L.bits++;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o = (o + bytes + 255) & ~size_t(255);
    return at;
  };
  L.cnt = take(4 * L.n_src);
  L.offs = take(4 * L.n_src);
  L.total = take(4);
  L.scan_bytes = 4 * ((L.n_src + 2047) / 2048 + 1) + 256;
  L.scan = take(L.scan_bytes);
  L.rkey = take(4 * L.n_max);
  L.rval = take(4 * L.n_max);
  L.rsrc = take(4 * L.n_max);
  L.rw = take(4 * L.n_max);
  L.skey = take(4 * L.n_max);
  L.sval = take(4 * L.n_max);
  L.sort_bytes = sort_scratch_bytes((int)std::max(L.n_max, 1L), L.bits);
  L.sort = take(L.sort_bytes);
  L.rbeg = take(4 * (size_t)n_rows);
  L.rend = take(4 * (size_t)n_rows);
  L.topT = take(4 * (size_t)L.n_src * C);
  L.part = take(4 * (size_t)L.n_chunks * 2 * C);
  L.bytes = o + 256;   // + alignment of the caller's base
  return true;
}

// d3d_roi_last_form: what the calling thread's last RoIAlign call launched (host stores only).  family (1 k_roi_dense,
// 2 k_roi_sparse, 3 k_roi_dense_bwd, 4 k_roi_sparse_bwd, 5 the fixed-order backward), storage type (1 fp32, 2 bf16),
// lookup (bit 0: a level probes the hash table, bit 1: a level reads the dense index; 0 for the dense kernels), extent
// (1 the caller's crop, 2 read on the device, 0 for the dense kernels), grid x / y / z and workgroup size of the family's
// main kernel (5: k_roi_det_sum), levels with a table, workgroups of k_roi_f32_to_bf16 (4 on bf16 rows), and for 5
// n_max, n_chunks and the sort's key bits.  A call that launches nothing leaves the record as it is.
static constexpr int kRoiFormFields = 13;
static thread_local int t_roi_last_form[kRoiFormFields] = {};
enum RoiFamily { kRoiFamDense = 1, kRoiFamSparse = 2, kRoiFamDenseBwd = 3, kRoiFamSparseBwd = 4, kRoiFamDet = 5 };
static void roi_record(int family, size_t type_bytes, int lookup, int extent, dim3 grid, int block, int levels, long cvt = 0,
                       long n_max = 0, long n_chunks = 0, int bits = 0) {
  const int f[kRoiFormFields] = {family, type_bytes == 4 ? 1 : 2, lookup, extent, (int)grid.x, (int)grid.y, (int)grid.z,
                                 block, levels, (int)cvt, (int)n_max, (int)n_chunks, bits};
  std::copy(f, f + kRoiFormFields, t_roi_last_form);
}
// the lookup and extent fields of a forward launch over the levels of lv
static void roi_record_sparse(const RoiLevels &lv, size_t type_bytes, dim3 grid) {
  int lookup = 0, extent = 0, levels = 0;
  for (int l = 0; l < kRoiMaxLevels; l++) {
    if (!lv.v[l].tab) continue;
    levels++;
    lookup |= lv.v[l].dense ? 2 : 1;
    extent |= lv.v[l].extent ? 2 : 1;
  }
  roi_record(kRoiFamSparse, type_bytes, lookup, extent, grid, kRoiWaves * 64, levels);
}

}  // namespace d3d

using namespace d3d;

// Pooler pre-processing in one launch (what the reference spreads over ~25 tensor ops): metric yx_zb proposals ->
// the op's RoI rows (batch id, centre x, centre y, centre z, size x, size y, size z, yaw in degrees, in pixels of the
// full-resolution grid) and the FPN level of every RoI.  The arithmetic is the reference's, operation by operation in
// fp32 (a division by a constant is the product with its fp32 reciprocal, as the tensor library evaluates it), so
// that the result equals the host-side chain bit for bit (tests/test_boxes_gpu.py).
struct RoiPrepScales {
  float v[8];
};
__global__ __launch_bounds__(256) void k_roi_prepare(const float *__restrict__ boxes, int n, float voxel_scale,
                                                     RoiPrepScales scales, int n_levels, float inv_canonical,
                                                     float *__restrict__ rois, int32_t *__restrict__ levels,
                                                     const int32_t *__restrict__ batch_ids,
                                                     const int32_t *__restrict__ count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (count && i >= *count) {   // padding row of a list whose length is still on the device: no level pools it
    float *r = rois + (size_t)i * 8;
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = 0.f;
    if (levels) levels[i] = -1;
    return;
  }
  float b[7];
#pragma unroll
  for (int j = 0; j < 7; j++) b[j] = boxes[(size_t)i * 7 + j];
#pragma unroll
  for (int j = 0; j < 6; j++) b[j] *= voxel_scale;                  // convert_metric_to_pixel
  const float kHalfPi = (float)(3.14159265358979323846 * 0.5), kPi = (float)3.14159265358979323846;
  const float kInvPi = 1.f / kPi, kDeg = (float)(180.0 / 3.14159265358979323846);
  float yaw = b[6] + kHalfPi;                                        // yx_zb -> standard (bounding_box_3d.py:221-242)
  yaw = yaw - floorf(yaw * kInvPi + 0.f) * kPi;                      // limit_period(yaw, 0, pi)
  float *r = rois + (size_t)i * 8;
  r[0] = batch_ids ? (float)batch_ids[i] : 0.f;        // example index of the RoI (poolers_3d.py:112-118)
  r[1] = b[1];
  r[2] = b[0];
  r[3] = b[2] + b[5] * 0.5f;
  r[4] = b[3];
  r[5] = b[4];
  r[6] = b[5];
  r[7] = yaw * kDeg;
  if (levels) {                                                      // poolers_3d.py LevelMapper
    const float rate = sqrtf(fmaxf(b[3], b[4])) * inv_canonical;
    int best = 0;
    float bd = fabsf(scales.v[0] - rate);
    for (int l = 1; l < n_levels; l++) {
      const float d = fabsf(scales.v[l] - rate);
      if (d < bd) {
        bd = d;
        best = l;
      }
    }
    levels[i] = best;
  }
}

extern "C" {

int d3d_roi_prepare(const float *boxes_metric, int n, float voxel_scale, const float *scales_host, int n_levels,
                    float canonical_size, const int32_t *batch_ids, float *rois, int32_t *levels, void *stream) {
  return d3d_roi_prepare_counted(boxes_metric, n, nullptr, voxel_scale, scales_host, n_levels, canonical_size, batch_ids,
                                 rois, levels, stream);
}

int d3d_roi_prepare_counted(const float *boxes_metric, int n, const int32_t *count_dev, float voxel_scale,
                            const float *scales_host, int n_levels, float canonical_size, const int32_t *batch_ids,
                            float *rois, int32_t *levels, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(n >= 0 && n_levels >= 0 && n_levels <= 8, "roi_prepare: bad arguments (at most 8 levels)");
  if (n == 0) return D3D_OK;
  D3D_REQUIRE(boxes_metric && rois && (n_levels == 0 || scales_host), "roi_prepare: null pointer");
  RoiPrepScales sc = {};
  for (int l = 0; l < n_levels; l++) sc.v[l] = scales_host[l];
  hipLaunchKernelGGL(k_roi_prepare, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, boxes_metric, n, voxel_scale, sc,
                     n_levels, 1.f / canonical_size, rois, n_levels > 1 ? levels : nullptr, batch_ids, count_dev);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

int d3d_roi_align_rotated_3d_forward(const float *input, int B, int C, int H, int W, int Z,
                                     const float *rois, int K, float spatial_scale, int ph, int pw,
                                     int pz, int sampling_ratio, float *out, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && Z > 0 && K >= 0 && ph > 0 && pw > 0 && pz > 0, "roi_align: bad shape");
  if (K == 0) return D3D_OK;
  D3D_REQUIRE(input && rois && out, "roi_align: null pointer");
  long nthreads = (long)K * C * ph * pw * pz;
  hipLaunchKernelGGL(k_roi_dense, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, s, input, C, H, W, Z, rois, nthreads, spatial_scale, ph, pw, pz, sampling_ratio, out);
  D3D_LAUNCH_CHECK();
  roi_record(kRoiFamDense, 4, 0, 0, dim3((unsigned)((nthreads + 255) / 256)), 256, 0);
  return D3D_OK;
}

// fills lv (one pyramid level of a pooling launch) from the grid of spatial size `size`
static int roi_level_of(d3d_meta *m, const int *size, const void *feats, const int *crop, float spatial_scale,
                        hipStream_t s, RoiLevel *lv) {
  std::map<Size3, Grid>::iterator it;
  bool have_grid;
  {
    D3D_LOCK(m);
    it = m->grids.find(Size3{size[0], size[1], size[2]});
    have_grid = it != m->grids.end();
  }
  if (!have_grid) {
    set_error("roi_align_sparse: no grid of spatial size [%d,%d,%d]", size[0], size[1], size[2]);
    return D3D_ERR_STATE;
  }
  Grid &g = it->second;
  const int32_t *extent = nullptr;
  if (!crop) {  // NULL crop: the grid's own occupied extent, computed once on the device
    int rc = grid_extent(m, g, s);
    if (rc) return rc;
    extent = g.extent;
  }
  *lv = {g.tab, feats, extent, crop ? nullptr : g.dense, g.cap, crop ? crop[0] : 0, crop ? crop[1] : 0, crop ? crop[2] : 0,
         g.hext[0], g.hext[1], g.hext[2], spatial_scale};
  return D3D_OK;
}

}  // extern "C"

template <typename T>
static int roi_sparse_forward(d3d_meta *m, const int *size, const T *feats, int C, const int *crop, const float *rois, int K,
                              float spatial_scale, int ph, int pw, int pz, int sampling_ratio, const int *roi_levels,
                              int level, int layout, T *out, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && size && C > 0 && K >= 0 && ph > 0 && pw > 0 && pz > 0, "roi_align_sparse: bad arguments");
  D3D_REQUIRE(!roi_levels || (level >= 0 && level < kRoiMaxLevels), "roi_align_sparse: level %d (< %d)", level, kRoiMaxLevels);
  D3D_REQUIRE(sizeof(T) == 4 || ((uintptr_t)feats & 3) == 0, "roi_align_sparse: bf16 rows not 4-byte aligned");
  RoiLevels lv = {};
  if (int rc = roi_level_of(m, size, feats, crop, spatial_scale, s, &lv.v[roi_levels ? level : 0])) return rc;
  if (K == 0) return D3D_OK;
  D3D_REQUIRE(feats && rois && out, "roi_align_sparse: null pointer");
  D3D_REQUIRE(layout == 0 || layout == 1, "roi_align_sparse: layout must be 0 ([K,C,ph,pw,pz]) or 1 ([K,ph,pw,C,pz])");
  hipLaunchKernelGGL(k_roi_sparse<T>, dim3(K, (C + kRoiCch - 1) / kRoiCch), dim3(kRoiWaves * 64), 0, s, lv, C, rois,
                     roi_levels, ph, pw, pz, sampling_ratio, layout, out);
  D3D_LAUNCH_CHECK();
  roi_record_sparse(lv, sizeof(T), dim3(K, (C + kRoiCch - 1) / kRoiCch));
  return D3D_OK;
}

template <typename T>
static int roi_sparse_forward_levels(d3d_meta *m, int n_levels, const int *sizes_host, const T *const *feats_host, int C,
                                     const float *scales_host, const float *rois, int K, int ph, int pw, int pz,
                                     int sampling_ratio, const int *roi_levels, int layout, T *out, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && sizes_host && feats_host && scales_host && n_levels >= 1 && n_levels <= kRoiMaxLevels,
              "roi_align_sparse_levels: 1..%d levels", kRoiMaxLevels);
  D3D_REQUIRE(C > 0 && K >= 0 && ph > 0 && pw > 0 && pz > 0 && (roi_levels || n_levels == 1),
              "roi_align_sparse_levels: bad arguments");
  D3D_REQUIRE(layout == 0 || layout == 1, "roi_align_sparse: layout must be 0 ([K,C,ph,pw,pz]) or 1 ([K,ph,pw,C,pz])");
  RoiLevels lv = {};
  for (int l = 0; l < n_levels; l++) {
    D3D_REQUIRE(feats_host[l], "roi_align_sparse_levels: null feature pointer of level %d", l);
    D3D_REQUIRE(sizeof(T) == 4 || ((uintptr_t)feats_host[l] & 3) == 0, "roi_align_sparse_levels: bf16 rows not 4-byte aligned");
    if (int rc = roi_level_of(m, sizes_host + 3 * l, feats_host[l], nullptr, scales_host[l], s, &lv.v[l])) return rc;
  }
  if (K == 0) return D3D_OK;
  D3D_REQUIRE(rois && out, "roi_align_sparse_levels: null pointer");
  hipLaunchKernelGGL(k_roi_sparse<T>, dim3(K, (C + kRoiCch - 1) / kRoiCch), dim3(kRoiWaves * 64), 0, s, lv, C, rois,
                     roi_levels, ph, pw, pz, sampling_ratio, layout, out);
  D3D_LAUNCH_CHECK();
  roi_record_sparse(lv, sizeof(T), dim3(K, (C + kRoiCch - 1) / kRoiCch));
  return D3D_OK;
}

extern "C" {

int d3d_roi_align_rotated_3d_sparse_forward(d3d_meta *m, const int *size, const float *feats, int C,
                                            const int *crop, const float *rois, int K,
                                            float spatial_scale, int ph, int pw, int pz,
                                            int sampling_ratio, const int *roi_levels, int level, int layout,
                                            float *out, void *stream) {
  return roi_sparse_forward<float>(m, size, feats, C, crop, rois, K, spatial_scale, ph, pw, pz, sampling_ratio, roi_levels,
                                   level, layout, out, stream);
}

int d3d_roi_align_rotated_3d_sparse_forward_bf16(d3d_meta *m, const int *size, const void *feats, int C, const int *crop,
                                                 const float *rois, int K, float spatial_scale, int ph, int pw, int pz,
                                                 int sampling_ratio, const int *roi_levels, int level, int layout,
                                                 void *out, void *stream) {
  return roi_sparse_forward<unsigned short>(m, size, (const unsigned short *)feats, C, crop, rois, K, spatial_scale, ph,
                                            pw, pz, sampling_ratio, roi_levels, level, layout, (unsigned short *)out,
                                            stream);
}

int d3d_roi_align_rotated_3d_sparse_forward_levels(d3d_meta *m, int n_levels, const int *sizes_host,
                                                   const float *const *feats_host, int C, const float *scales_host,
                                                   const float *rois, int K, int ph, int pw, int pz, int sampling_ratio,
                                                   const int *roi_levels, int layout, float *out, void *stream) {
  return roi_sparse_forward_levels<float>(m, n_levels, sizes_host, feats_host, C, scales_host, rois, K, ph, pw, pz,
                                          sampling_ratio, roi_levels, layout, out, stream);
}

int d3d_roi_align_rotated_3d_sparse_forward_levels_bf16(d3d_meta *m, int n_levels, const int *sizes_host,
                                                        const void *const *feats_host, int C, const float *scales_host,
                                                        const float *rois, int K, int ph, int pw, int pz,
                                                        int sampling_ratio, const int *roi_levels, int layout, void *out,
                                                        void *stream) {
  return roi_sparse_forward_levels<unsigned short>(m, n_levels, sizes_host, (const unsigned short *const *)feats_host, C,
                                                   scales_host, rois, K, ph, pw, pz, sampling_ratio, roi_levels, layout,
                                                   (unsigned short *)out, stream);
}

int d3d_roi_align_rotated_3d_backward(const float *top_diff, int B, int C, int H, int W, int Z,
                                      const float *rois, int K, float spatial_scale, int ph, int pw, int pz,
                                      int sampling_ratio, float *bottom_diff, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && Z > 0 && K >= 0 && ph > 0 && pw > 0 && pz > 0 && bottom_diff,
              "roi_align_backward: bad arguments");
  D3D_HIP_CHECK(hipMemsetAsync(bottom_diff, 0, sizeof(float) * (size_t)B * C * H * W * Z, s));
  if (K == 0) return D3D_OK;
  D3D_REQUIRE(top_diff && rois, "roi_align_backward: null pointer");
  long nthreads = (long)K * C * ph * pw * pz;
  hipLaunchKernelGGL(k_roi_dense_bwd, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, s, top_diff, C, H, W, Z,
                     rois, nthreads, spatial_scale, ph, pw, pz, sampling_ratio, bottom_diff);
  D3D_LAUNCH_CHECK();
  roi_record(kRoiFamDenseBwd, 4, 0, 0, dim3((unsigned)((nthreads + 255) / 256)), 256, 0);
  return D3D_OK;
}

// the grid of spatial size `size`, or D3D_ERR_STATE
static int roi_grid_of(d3d_meta *m, const int *size, const char *what, const Grid **out) {
  std::map<Size3, Grid>::iterator it;
  bool have_grid;
  {
    D3D_LOCK(m);
    it = m->grids.find(Size3{size[0], size[1], size[2]});
    have_grid = it != m->grids.end();
  }
  if (!have_grid) {
    set_error("%s: no grid of spatial size [%d,%d,%d]", what, size[0], size[1], size[2]);
    return D3D_ERR_STATE;
  }
  *out = &it->second;
  return D3D_OK;
}

// d_feats [n_active, C] is accumulated into (zero it first)
int d3d_roi_align_rotated_3d_sparse_backward(d3d_meta *m, const int *size, const float *top_diff, int C,
                                             const int *crop, const float *rois, int K, float spatial_scale,
                                             int ph, int pw, int pz, int sampling_ratio, float *d_feats,
                                             void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && size && crop && C > 0 && K >= 0 && ph > 0 && pw > 0 && pz > 0, "roi_align_sparse_backward: bad arguments");
  const Grid *gp;
  if (int rc = roi_grid_of(m, size, "roi_align_sparse_backward", &gp)) return rc;
  if (K == 0) return D3D_OK;
  D3D_REQUIRE(top_diff && rois && d_feats, "roi_align_sparse_backward: null pointer");
  const Grid &g = *gp;
  const int NB = ph * pw * pz;
  size_t lds = (size_t)kRoiBwdCch * (NB + 1) * sizeof(float);
  D3D_REQUIRE(lds <= 64 * 1024, "roi_align_sparse_backward: pooled volume %d too large", NB);
  hipLaunchKernelGGL(k_roi_sparse_bwd<float>, dim3(K, (C + kRoiBwdCch - 1) / kRoiBwdCch), dim3(256), lds, s, g.tab, g.cap,
                     C, crop[0], crop[1], crop[2], rois, spatial_scale, ph, pw, pz, sampling_ratio, top_diff, d_feats);
  D3D_LAUNCH_CHECK();
  roi_record(kRoiFamSparseBwd, 4, 1, 1, dim3(K, (C + kRoiBwdCch - 1) / kRoiBwdCch), 256, 1);
  return D3D_OK;
}

size_t d3d_roi_align_rotated_3d_sparse_backward_bf16_scratch_bytes(int C, int n_rows) {
  if (C <= 0 || n_rows < 0) return 0;
  return (size_t)n_rows * C * sizeof(float) + 256;   // + alignment of the caller's base
}

int d3d_roi_align_rotated_3d_sparse_backward_bf16(d3d_meta *m, const int *size, const void *top_diff, int C,
                                                  const int *crop, const float *rois, int K, float spatial_scale, int ph,
                                                  int pw, int pz, int sampling_ratio, void *d_feats, int n_rows,
                                                  void *scratch, size_t scratch_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && size && crop && C > 0 && K >= 0 && ph > 0 && pw > 0 && pz > 0 && n_rows >= 0,
              "roi_align_sparse_backward_bf16: bad arguments");
  const int NB = ph * pw * pz;
  const size_t lds = (size_t)kRoiBwdCch * (NB + 1) * sizeof(float);
  D3D_REQUIRE(lds <= 64 * 1024, "roi_align_sparse_backward_bf16: pooled volume %d too large", NB);
  const size_t need = d3d_roi_align_rotated_3d_sparse_backward_bf16_scratch_bytes(C, n_rows);
  D3D_REQUIRE(scratch_bytes >= need, "roi_align_sparse_backward_bf16: scratch %zu < %zu bytes", scratch_bytes, need);
  const Grid *gp;
  if (int rc = roi_grid_of(m, size, "roi_align_sparse_backward_bf16", &gp)) return rc;
  D3D_REQUIRE(n_rows == gp->n, "roi_align_sparse_backward_bf16: n_rows %d != %d active sites", n_rows, gp->n);
  if (n_rows == 0) return D3D_OK;
  D3D_REQUIRE(d_feats && scratch && (K == 0 || (top_diff && rois)), "roi_align_sparse_backward_bf16: null pointer");
  D3D_REQUIRE(((uintptr_t)d_feats & 7) == 0, "roi_align_sparse_backward_bf16: d_feats not 8-byte aligned");
  float *acc = (float *)(((uintptr_t)scratch + 255) & ~(uintptr_t)255);
  const long total = (long)n_rows * C;
  D3D_HIP_CHECK(hipMemsetAsync(acc, 0, sizeof(float) * (size_t)total, s));
  if (K > 0) {
    const Grid &g = *gp;
    hipLaunchKernelGGL(k_roi_sparse_bwd<unsigned short>, dim3(K, (C + kRoiBwdCch - 1) / kRoiBwdCch), dim3(256), lds, s,
                       g.tab, g.cap, C, crop[0], crop[1], crop[2], rois, spatial_scale, ph, pw, pz, sampling_ratio,
                       (const unsigned short *)top_diff, acc);
  }
  hipLaunchKernelGGL(k_roi_f32_to_bf16, dim3((unsigned)((total + 1023) / 1024)), dim3(256), 0, s, acc, total,
                     (unsigned short *)d_feats);
  D3D_LAUNCH_CHECK();
  roi_record(kRoiFamSparseBwd, 2, 1, 1, K > 0 ? dim3(K, (C + kRoiBwdCch - 1) / kRoiBwdCch) : dim3(0, 0, 0), 256, 1,
             (total + 1023) / 1024);
  return D3D_OK;
}

size_t d3d_roi_align_rotated_3d_sparse_backward_deterministic_scratch_bytes(int K, int C, int ph, int pw, int pz,
                                                                           int sampling_ratio, int n_rows) {
  RoiDetLayout L;
  return roi_det_layout(K, C, ph, pw, pz, sampling_ratio, n_rows, L) ? L.bytes : 0;
}

size_t d3d_roi_align_rotated_3d_sparse_backward_deterministic_bf16_scratch_bytes(int K, int C, int ph, int pw, int pz,
                                                                                int sampling_ratio, int n_rows) {
  return d3d_roi_align_rotated_3d_sparse_backward_deterministic_scratch_bytes(K, C, ph, pw, pz, sampling_ratio, n_rows);
}

}  // extern "C"

// the launches of the fixed-order backward (arguments checked by the caller): TT = storage type of top_diff, TO of d_feats
template <typename TT, typename TO>
static int roi_det_run(const Grid &g, const int *crop, const TT *top_diff, int C, const float *rois, int K,
                       float spatial_scale, int ph, int pw, int pz, int sampling_ratio, TO *d_feats, int n_rows,
                       const RoiDetLayout &L, void *scratch, hipStream_t s) {
  char *base = (char *)(((uintptr_t)scratch + 255) & ~(uintptr_t)255);
  int32_t *cnt = (int32_t *)(base + L.cnt), *offs = (int32_t *)(base + L.offs), *total = (int32_t *)(base + L.total);
  uint32_t *rkey = (uint32_t *)(base + L.rkey), *skey = (uint32_t *)(base + L.skey);
  int32_t *rval = (int32_t *)(base + L.rval), *sval = (int32_t *)(base + L.sval), *rsrc = (int32_t *)(base + L.rsrc);
  float *rw = (float *)(base + L.rw), *topT = (float *)(base + L.topT), *part = (float *)(base + L.part);
  int32_t *rbeg = (int32_t *)(base + L.rbeg), *rend = (int32_t *)(base + L.rend);
  const int NB = ph * pw * pz;
  hipLaunchKernelGGL(k_roi_det_transpose<TT>, dim3(K, (NB + 31) / 32, (C + 31) / 32), dim3(256), 0, s, top_diff, C, NB,
                     topT);
  hipLaunchKernelGGL((k_roi_det_taps<false>), dim3(K), dim3(256), 0, s, g.tab, g.cap, crop[0], crop[1], crop[2], rois,
                     spatial_scale, ph, pw, pz, sampling_ratio, n_rows, cnt, nullptr, nullptr, nullptr, nullptr, nullptr);
  D3D_LAUNCH_CHECK();
  Arena scan_arena;
  scan_arena.base = base + L.scan;
  scan_arena.cap = L.scan_bytes;
  if (int rc = scan_exclusive_i32(cnt, offs, (int)L.n_src, total, scan_arena, s)) return rc;
  hipLaunchKernelGGL((k_roi_det_taps<true>), dim3(K), dim3(256), 0, s, g.tab, g.cap, crop[0], crop[1], crop[2], rois,
                     spatial_scale, ph, pw, pz, sampling_ratio, n_rows, nullptr, offs, rkey, rval, rsrc, rw);
  D3D_LAUNCH_CHECK();
  Arena sort_arena;
  sort_arena.base = base + L.sort;
  sort_arena.cap = L.sort_bytes;
  if (int rc = sort_pairs_u32(rkey, skey, rval, sval, (int)L.n_max, L.bits, sort_arena, s, false, total)) return rc;
  D3D_HIP_CHECK(hipMemsetAsync(rbeg, 0, 4 * (size_t)n_rows, s));
  D3D_HIP_CHECK(hipMemsetAsync(rend, 0, 4 * (size_t)n_rows, s));
  hipLaunchKernelGGL(k_roi_det_bounds, dim3((unsigned)((L.n_max + 255) / 256)), dim3(256), 0, s, skey, (int)L.n_max,
                     total, rbeg, rend);
  hipLaunchKernelGGL(k_roi_det_sum<TO>, dim3((unsigned)((L.n_chunks + 3) / 4)), dim3(256), 0, s, skey, sval, rsrc, rw,
                     (int)L.n_max, total, rbeg, rend, topT, C, part, d_feats);
  hipLaunchKernelGGL(k_roi_det_join<TO>, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, s, rbeg, rend, n_rows, part, C,
                     d_feats);
  D3D_LAUNCH_CHECK();
  roi_record(kRoiFamDet, sizeof(TO), 1, 1, dim3((unsigned)((L.n_chunks + 3) / 4)), 256, 1, 0, L.n_max, L.n_chunks, L.bits);
  return D3D_OK;
}

extern "C" {

int d3d_roi_last_form(int *out, int n) {
  for (int i = 0; out && i < n && i < kRoiFormFields; i++) out[i] = t_roi_last_form[i];
  std::fill(t_roi_last_form, t_roi_last_form + kRoiFormFields, 0);
  return kRoiFormFields;
}

int d3d_roi_align_rotated_3d_sparse_backward_deterministic(d3d_meta *m, const int *size, const float *top_diff, int C,
                                                           const int *crop, const float *rois, int K,
                                                           float spatial_scale, int ph, int pw, int pz,
                                                           int sampling_ratio, float *d_feats, int n_rows,
                                                           void *scratch, size_t scratch_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && size && crop && C > 0 && K >= 0 && ph > 0 && pw > 0 && pz > 0 && n_rows >= 0,
              "roi_align_sparse_backward_deterministic: bad arguments");
  D3D_REQUIRE(sampling_ratio > 0,
              "roi_align_sparse_backward_deterministic: sampling_ratio %d (adaptive sampling has no record bound before "
              "the launch)", sampling_ratio);
  const Grid *gp;
  if (int rc = roi_grid_of(m, size, "roi_align_sparse_backward_deterministic", &gp)) return rc;
  if (K == 0 || n_rows == 0) return D3D_OK;
  D3D_REQUIRE(top_diff && rois && d_feats && scratch, "roi_align_sparse_backward_deterministic: null pointer");
  RoiDetLayout L;
  D3D_REQUIRE(roi_det_layout(K, C, ph, pw, pz, sampling_ratio, n_rows, L),
              "roi_align_sparse_backward_deterministic: %d RoIs x %d bins x %d samples is too many records", K,
              ph * pw * pz, sampling_ratio * sampling_ratio * sampling_ratio);
  D3D_REQUIRE(scratch_bytes >= L.bytes, "roi_align_sparse_backward_deterministic: scratch %zu < %zu bytes", scratch_bytes,
              L.bytes);
  return roi_det_run<float, float>(*gp, crop, top_diff, C, rois, K, spatial_scale, ph, pw, pz, sampling_ratio, d_feats,
                                   n_rows, L, scratch, s);
}

int d3d_roi_align_rotated_3d_sparse_backward_deterministic_bf16(d3d_meta *m, const int *size, const void *top_diff, int C,
                                                                const int *crop, const float *rois, int K,
                                                                float spatial_scale, int ph, int pw, int pz,
                                                                int sampling_ratio, void *d_feats, int n_rows,
                                                                void *scratch, size_t scratch_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && size && crop && C > 0 && K >= 0 && ph > 0 && pw > 0 && pz > 0 && n_rows >= 0,
              "roi_align_sparse_backward_deterministic_bf16: bad arguments");
  D3D_REQUIRE(sampling_ratio > 0,
              "roi_align_sparse_backward_deterministic_bf16: sampling_ratio %d (adaptive sampling has no record bound "
              "before the launch)", sampling_ratio);
  RoiDetLayout L;
  D3D_REQUIRE(roi_det_layout(K, C, ph, pw, pz, sampling_ratio, n_rows, L),
              "roi_align_sparse_backward_deterministic_bf16: %d RoIs x %d bins x %d samples is too many records", K,
              ph * pw * pz, sampling_ratio * sampling_ratio * sampling_ratio);
  D3D_REQUIRE(K == 0 || scratch_bytes >= L.bytes, "roi_align_sparse_backward_deterministic_bf16: scratch %zu < %zu bytes",
              scratch_bytes, L.bytes);
  const Grid *gp;
  if (int rc = roi_grid_of(m, size, "roi_align_sparse_backward_deterministic_bf16", &gp)) return rc;
  D3D_REQUIRE(n_rows == gp->n, "roi_align_sparse_backward_deterministic_bf16: n_rows %d != %d active sites", n_rows,
              gp->n);
  if (n_rows == 0) return D3D_OK;
  D3D_REQUIRE(d_feats && (K == 0 || (top_diff && rois && scratch)),
              "roi_align_sparse_backward_deterministic_bf16: null pointer");
  D3D_HIP_CHECK(hipMemsetAsync(d_feats, 0, sizeof(unsigned short) * (size_t)n_rows * C, s));   // rows with no record
  if (K == 0) return D3D_OK;
  return roi_det_run<unsigned short, unsigned short>(*gp, crop, (const unsigned short *)top_diff, C, rois, K, spatial_scale,
                                                     ph, pw, pz, sampling_ratio, (unsigned short *)d_feats, n_rows, L,
                                                     scratch, s);
}

}  // extern "C"
