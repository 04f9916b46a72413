// a21. RoIAlignRotated3D backward over the hash grid without float atomics; the atomic form is roi_backward.hip.
#include "grid_internal.h"

namespace d3d {

#include "roi_geometry.inc"

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

// what follows from the arguments alone: (RoI, bin) sources, the bound on the records, their chunks, the sort's key bits
struct RoiDetDims {
  long n_src, n_max, n_chunks;
  int bits;
};
static bool roi_det_dims(int K, int C, int ph, int pw, int pz, int sampling_ratio, int n_rows, RoiDetDims &D) {
  if (K < 0 || C <= 0 || ph <= 0 || pw <= 0 || pz <= 0 || sampling_ratio <= 0 || n_rows < 0) return false;
  const long NB = (long)ph * pw * pz, NS = (long)sampling_ratio * sampling_ratio * sampling_ratio;
  D.n_src = (long)K * NB;
  D.n_max = D.n_src * NS * 8;   // a record holds at least one of the 8 NS taps of its bin
  if (D.n_max >= (1L << 31) - kRoiDetChunk) return false;
  D.n_chunks = (D.n_max + kRoiDetChunk - 1) / kRoiDetChunk;
  D.bits = 1;
  while (D.bits < 31 && (1L << D.bits) < (long)n_rows) D.bits++;
  return true;
}

// the scratch of the fixed-order backward, carved from a 256-aligned base by the entry points and by their size query
struct RoiDetLayout {
  int32_t *cnt, *offs, *total;   // [n_src] records per (RoI, bin), their scan; the number of records
  char *scan, *sort;             // scan_exclusive_i32's and sort_pairs_u32's own scratch, of scan_bytes and sort_bytes
  uint32_t *rkey, *skey;         // [n_max] destination rows in tap order; sorted
  int32_t *rval, *sval, *rsrc;   // [n_max] record index in tap order; in sorted order; source (RoI, bin)
  float *rw, *topT, *part;       // [n_max] weight / count; top_diff as [K, NB, C]; [n_chunks][2][C] partial sums
  int32_t *rbeg, *rend;          // [n_rows] a row's list in the sorted records
  size_t scan_bytes, sort_bytes;
};
static int roi_det_carve(Arena &A, const RoiDetDims &D, int C, int n_rows, RoiDetLayout &L) {
  const size_t scan_bytes = 4 * ((D.n_src + kScanTile - 1) / kScanTile + 1) + 256;
  const size_t sort_bytes = sort_scratch_bytes((int)std::max(D.n_max, 1L), D.bits);
  D3D_ALLOC(cnt, int32_t, A, D.n_src);
  D3D_ALLOC(offs, int32_t, A, D.n_src);
  D3D_ALLOC(total, int32_t, A, 1);
  D3D_ALLOC(scan, char, A, scan_bytes);
  D3D_ALLOC(rkey, uint32_t, A, D.n_max);
  D3D_ALLOC(rval, int32_t, A, D.n_max);
  D3D_ALLOC(rsrc, int32_t, A, D.n_max);
  D3D_ALLOC(rw, float, A, D.n_max);
  D3D_ALLOC(skey, uint32_t, A, D.n_max);
  D3D_ALLOC(sval, int32_t, A, D.n_max);
  D3D_ALLOC(sort, char, A, sort_bytes);
  D3D_ALLOC(rbeg, int32_t, A, n_rows);
  D3D_ALLOC(rend, int32_t, A, n_rows);
  D3D_ALLOC(topT, float, A, (size_t)D.n_src * C);
  D3D_ALLOC(part, float, A, (size_t)D.n_chunks * 2 * C);
  L = RoiDetLayout{cnt, offs, total, scan, sort, rkey, skey, rval, sval, rsrc, rw, topT, part, rbeg, rend, scan_bytes, sort_bytes};
  return D3D_OK;
}
// what the carve takes, and 255 bytes for a caller's `scratch` that is not 256-aligned
static size_t roi_det_bytes(const RoiDetDims &D, int C, int n_rows) {
  Arena A = sizing_arena();
  RoiDetLayout L;
  (void)roi_det_carve(A, D, C, n_rows, L);
  return A.used + 255;
}

// the launches of the fixed-order backward (arguments and scratch size checked by the caller): TT = storage type of
// top_diff, TO of d_feats.  `scratch` need not be aligned: the carve starts at the next multiple of 256.
template <typename TT, typename TO>
static int roi_det_run(const Grid &g, const int *crop, const TT *top_diff, int C, const float *rois, int K,
                       float spatial_scale, int ph, int pw, int pz, int sampling_ratio, TO *d_feats, int n_rows,
                       const RoiDetDims &D, void *scratch, size_t scratch_bytes, hipStream_t s) {
  const size_t pad = (size_t)(-(uintptr_t)scratch & 255);
  Arena A = scratch_arena((char *)scratch + pad, scratch_bytes - pad);
  RoiDetLayout L;
  if (int rc = roi_det_carve(A, D, C, n_rows, L)) return rc;
  const int NB = ph * pw * pz;
  hipLaunchKernelGGL(k_roi_det_transpose<TT>, dim3(K, (NB + 31) / 32, (C + 31) / 32), dim3(256), 0, s, top_diff, C, NB,
                     L.topT);
  hipLaunchKernelGGL((k_roi_det_taps<false>), dim3(K), dim3(256), 0, s, g.tab, g.cap, crop[0], crop[1], crop[2], rois,
                     spatial_scale, ph, pw, pz, sampling_ratio, n_rows, L.cnt, nullptr, nullptr, nullptr, nullptr, nullptr);
  D3D_LAUNCH_CHECK();
  Arena scan_arena = scratch_arena(L.scan, L.scan_bytes);
  if (int rc = scan_exclusive_i32(L.cnt, L.offs, (int)D.n_src, L.total, scan_arena, s)) return rc;
  hipLaunchKernelGGL((k_roi_det_taps<true>), dim3(K), dim3(256), 0, s, g.tab, g.cap, crop[0], crop[1], crop[2], rois,
                     spatial_scale, ph, pw, pz, sampling_ratio, n_rows, nullptr, L.offs, L.rkey, L.rval, L.rsrc, L.rw);
  D3D_LAUNCH_CHECK();
  Arena sort_arena = scratch_arena(L.sort, L.sort_bytes);
  if (int rc = sort_pairs_u32(L.rkey, L.skey, L.rval, L.sval, (int)D.n_max, D.bits, sort_arena, s, false, L.total)) return rc;
  D3D_HIP_CHECK(hipMemsetAsync(L.rbeg, 0, 4 * (size_t)n_rows, s));
  D3D_HIP_CHECK(hipMemsetAsync(L.rend, 0, 4 * (size_t)n_rows, s));
  hipLaunchKernelGGL(k_roi_det_bounds, dim3((unsigned)((D.n_max + 255) / 256)), dim3(256), 0, s, L.skey, (int)D.n_max,
                     L.total, L.rbeg, L.rend);
  hipLaunchKernelGGL(k_roi_det_sum<TO>, dim3((unsigned)((D.n_chunks + 3) / 4)), dim3(256), 0, s, L.skey, L.sval, L.rsrc, L.rw,
                     (int)D.n_max, L.total, L.rbeg, L.rend, L.topT, C, L.part, d_feats);
  hipLaunchKernelGGL(k_roi_det_join<TO>, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, s, L.rbeg, L.rend, n_rows, L.part,
                     C, d_feats);
  D3D_LAUNCH_CHECK();
  roi_record(kRoiFamDet, sizeof(TO), 1, 1, dim3((unsigned)((D.n_chunks + 3) / 4)), 256, 1, 0, D.n_max, D.n_chunks, D.bits);
  return D3D_OK;
}

}  // namespace d3d

using namespace d3d;

extern "C" {

// 0: the arguments are refused
size_t d3d_roi_align_rotated_3d_sparse_backward_deterministic_scratch_bytes(int K, int C, int ph, int pw, int pz,
                                                                           int sampling_ratio, int n_rows) {
  RoiDetDims D;
  return roi_det_dims(K, C, ph, pw, pz, sampling_ratio, n_rows, D) ? roi_det_bytes(D, C, n_rows) : 0;
}

size_t d3d_roi_align_rotated_3d_sparse_backward_deterministic_bf16_scratch_bytes(int K, int C, int ph, int pw, int pz,
                                                                                int sampling_ratio, int n_rows) {
  return d3d_roi_align_rotated_3d_sparse_backward_deterministic_scratch_bytes(K, C, ph, pw, pz, sampling_ratio, n_rows);
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
  RoiDetDims D;
  D3D_REQUIRE(roi_det_dims(K, C, ph, pw, pz, sampling_ratio, n_rows, D),
              "roi_align_sparse_backward_deterministic: %d RoIs x %d bins x %d samples is too many records", K,
              ph * pw * pz, sampling_ratio * sampling_ratio * sampling_ratio);
  const size_t need = roi_det_bytes(D, C, n_rows);
  D3D_REQUIRE(scratch_bytes >= need, "roi_align_sparse_backward_deterministic: scratch %zu < %zu bytes", scratch_bytes,
              need);
  return roi_det_run<float, float>(*gp, crop, top_diff, C, rois, K, spatial_scale, ph, pw, pz, sampling_ratio, d_feats,
                                   n_rows, D, scratch, scratch_bytes, s);
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
  RoiDetDims D;
  D3D_REQUIRE(roi_det_dims(K, C, ph, pw, pz, sampling_ratio, n_rows, D),
              "roi_align_sparse_backward_deterministic_bf16: %d RoIs x %d bins x %d samples is too many records", K,
              ph * pw * pz, sampling_ratio * sampling_ratio * sampling_ratio);
  const size_t need = roi_det_bytes(D, C, n_rows);
  D3D_REQUIRE(K == 0 || scratch_bytes >= need, "roi_align_sparse_backward_deterministic_bf16: scratch %zu < %zu bytes",
              scratch_bytes, need);
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
                                                     ph, pw, pz, sampling_ratio, (unsigned short *)d_feats, n_rows, D,
                                                     scratch, scratch_bytes, s);
}

}  // extern "C"
