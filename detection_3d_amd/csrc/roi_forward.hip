// a21. RoIAlignRotated3D forward (maskrcnn_benchmark/csrc/cuda/ROIAlignRotated3D_cuda.cu:15-177).
//  * dense variant: same contract as _C.roi_align_rotated_3d_forward (input [B,C,H,W,Z]);
//  * sparse variant: samples the SparseConvNetTensor through its hash grid, so the 1.07 GB dense
//    map of sparse_3d_to_dense_2d (sparseconvnet/tools_3d_2d.py:7-48) is never materialised.
// Both keep the reference's `zsize > zsize` bound quirk (:27): z above the map is clamped.
// Also the pooler's pre-processing (k_roi_prepare) and the one definition of the form record that roi_backward.hip and
// roi_backward_det.hip write too.
#include "grid_internal.h"

namespace d3d {

#include "roi_geometry.inc"

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

thread_local int t_roi_last_form[kRoiFormFields] = {};
void roi_record(int family, size_t type_bytes, int lookup, int extent, dim3 grid, int block, int levels, long cvt,
                long n_max, long n_chunks, int bits) {
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
  Grid *gp = find_grid(m, size);
  if (!gp) {
    set_error("roi_align_sparse: no grid of spatial size [%d,%d,%d]", size[0], size[1], size[2]);
    return D3D_ERR_STATE;
  }
  Grid &g = *gp;
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

int d3d_roi_last_form(int *out, int n) {
  for (int i = 0; out && i < n && i < kRoiFormFields; i++) out[i] = t_roi_last_form[i];
  std::fill(t_roi_last_form, t_roi_last_form + kRoiFormFields, 0);
  return kRoiFormFields;
}

}  // extern "C"
