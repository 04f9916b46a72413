// Voxel down-sampling and a point cap for raw scans: steps 2 and 4 of the reference's data preparation
// (data3d/suncg_utils/suncg_preprocess.py:748-767, open3d.voxel_down_sample(pcd, voxel_size=0.02);
// data3d/indoor_data_util.py:59-71, random_sample_pcl(..., only_reduce=True)).  The definitions are written out in
// include/d3d_hip.h; they restate open3d's VoxelDownSample and are not pinned against open3d itself.
//
// Down-sampling, passes: per-axis min / max of the kept rows -> cell coordinates in fp64 -> three stable radix sorts
// (z, y, x; a dropped row carries bit 21 of x and sorts behind every voxel) -> 63-bit keys of the sorted positions ->
// segment heads; a head's point is the voxel's first occurrence, and a scan of those flags over the POINT indices is the
// output row -> segment starts and the 512-row chunks of the segments longer than 64 rows -> one read-back (voxels,
// overflow, chunks).  Then: one wave per chunk sums its rows in fp64 (k_ds_partial), one lane per voxel sums a short
// segment's rows or a long one's partial sums in chunk order, divides and writes the output row once (k_ds_rows).  No
// float atomics; every order is fixed by the data, so the same input gives the same bits.
//
// Cap: the k-th smallest 32-bit row key by four 8-bit radix histogram passes over many workgroups (the keys are
// recomputed from the row index, never stored), flags, a scan, and a compaction in ascending row order.
#include "d3d_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace d3d {

namespace {

constexpr int kCellBits = 21;                      // per axis: 3 x 21 bits in a 64-bit key
constexpr uint32_t kCellMax = (1u << kCellBits) - 1u;
constexpr uint32_t kDropX = 1u << kCellBits;       // x digit of a dropped row: behind every cell in the x sort
constexpr uint64_t kNoKey = ~uint64_t(0);
constexpr int kShort = 64;                         // segments up to here: one lane sums the rows
constexpr int kChunk = 512;                        // longer ones: chunks of this many rows, one wave each
constexpr int kMaxCols = 16;
constexpr int kMaxPoints = 1 << 28;

inline unsigned reduce_blocks(int n) { return std::max(1u, std::min(1024u, (unsigned)((n + 255) / 256))); }

__device__ __forceinline__ bool finite3(const float *p) {
  return fabsf(p[0]) < INFINITY && fabsf(p[1]) < INFINITY && fabsf(p[2]) < INFINITY;   // false for NaN
}

// info (device int32[16]): 0 voxels, 1 overflow flag, 2 chunks of long segments, 3 voxels again (scan over the points);
// 8..10 per-axis min and 11..13 max of the kept rows as order-preserving integers
enum { kInfoM = 0, kInfoOverflow = 1, kInfoChunks = 2, kInfoM2 = 3, kInfoMin = 8, kInfoMax = 11 };

// integer min / max of the order-preserving image: commutative, so the result does not depend on scheduling
__global__ __launch_bounds__(256) void k_ds_minmax(const float *__restrict__ pcl, int n, int C, uint32_t *info) {
  uint32_t lo[3] = {~0u, ~0u, ~0u}, hi[3] = {0u, 0u, 0u};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float *p = pcl + (size_t)i * C;
    if (!finite3(p)) continue;
    for (int d = 0; d < 3; d++) {
      const uint32_t u = f32_ordered(p[d]);
      lo[d] = min(lo[d], u);
      hi[d] = max(hi[d], u);
    }
  }
  for (int d = 0; d < 3; d++) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      lo[d] = min(lo[d], (uint32_t)__shfl_xor((int)lo[d], s, 64));
      hi[d] = max(hi[d], (uint32_t)__shfl_xor((int)hi[d], s, 64));
    }
  }
  if ((threadIdx.x & 63) == 0)
    for (int d = 0; d < 3; d++) {
      if (lo[d] != ~0u) atomicMin(&info[kInfoMin + d], lo[d]);
      if (hi[d] != 0u) atomicMax(&info[kInfoMax + d], hi[d]);
    }
}

// cell = floor((double(p) - lo) / voxel), lo = double(min) - 0.5 voxel: fp64 subtraction and IEEE division, no
// contraction (the build's -ffp-contract=off), no reciprocal.  p >= min, so the quotient is at least 0.5.
__global__ void k_ds_cells(const float *__restrict__ pcl, int n, int C, const uint32_t *info_u, double voxel,
                           uint32_t *cx, uint32_t *cy, uint32_t *cz, int32_t *iota, int32_t *info) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float *p = pcl + (size_t)i * C;
  uint32_t c[3] = {kDropX, 0u, 0u};
  if (finite3(p)) {
    bool over = false;
    for (int d = 0; d < 3; d++) {
      const double lo = (double)ordered_to_f32(info_u[kInfoMin + d]) - 0.5 * voxel;
      const double q = floor(((double)p[d] - lo) / voxel);
      over = over || !(q <= (double)kCellMax);
      c[d] = q >= 0.0 ? (q < (double)kCellMax ? (uint32_t)q : kCellMax) : 0u;
    }
    if (over) info[kInfoOverflow] = 1;     // every writer stores the same value
  }
  cx[i] = c[0];
  cy[i] = c[1];
  cz[i] = c[2];
  iota[i] = i;
}

__global__ void k_ds_keys(const int32_t *__restrict__ perm, const uint32_t *__restrict__ cx,
                          const uint32_t *__restrict__ cy, const uint32_t *__restrict__ cz, int n, uint64_t *key) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int i = perm[k];
  const uint32_t x = cx[i];
  key[k] = x >= kDropX ? kNoKey : ((uint64_t)x << (2 * kCellBits)) | ((uint64_t)cy[i] << kCellBits) | (uint64_t)cz[i];
}

// hflag[k]: sorted position k opens a voxel; isfirst[i]: point i is the first of its voxel (perm is a permutation, so
// every entry of both arrays is written exactly once)
__global__ void k_ds_heads(const uint64_t *__restrict__ key, const int32_t *__restrict__ perm, int n, int32_t *hflag,
                           int32_t *isfirst) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint64_t c = key[k];
  const int head = (c != kNoKey && (k == 0 || key[k - 1] != c)) ? 1 : 0;
  hflag[k] = head;
  isfirst[perm[k]] = head;
}

// segstart[s] = first sorted position of voxel s (in key order), segstart[M] = the number of kept rows
__global__ void k_ds_segs(const uint64_t *__restrict__ key, const int32_t *__restrict__ hflag,
                          const int32_t *__restrict__ hscan, int n, int32_t *segstart) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n || key[k] == kNoKey) return;
  const int s = hscan[k] + hflag[k] - 1;
  if (hflag[k]) segstart[s] = k;
  if (k == n - 1 || key[k + 1] == kNoKey) segstart[s + 1] = k + 1;
}

__device__ __forceinline__ int chunks_of(int len) { return len > kShort ? (len + kChunk - 1) / kChunk : 0; }

__global__ void k_ds_nch(const int32_t *__restrict__ segstart, const int32_t *__restrict__ info, int n, int32_t *nch) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  nch[s] = s < info[kInfoM] ? chunks_of(segstart[s + 1] - segstart[s]) : 0;
}

// One wave per 512-row chunk of a long segment: lane l sums rows l, l + 64, ... of the chunk in that order, the lanes
// are added by a fixed butterfly.  partial[t][c], t in chunk order over the segments.
__global__ __launch_bounds__(256) void k_ds_partial(const float *__restrict__ pcl, int n, int C,
                                                    const int32_t *__restrict__ perm,
                                                    const int32_t *__restrict__ segstart,
                                                    const int32_t *__restrict__ choff,
                                                    const int32_t *__restrict__ info, int m_host, int t_host,
                                                    double *partial) {
  const int M = min(m_host, info[kInfoM]), T = min(t_host, info[kInfoChunks]);
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= T || M <= 0) return;
  int lo = 0, hi = M - 1;                  // the last segment whose first chunk is not after t
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (choff[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  const int s = lo;
  const int b = segstart[s] + (t - choff[s]) * kChunk;
  const int e = min(min(b + kChunk, segstart[s + 1]), n);
  double acc[kMaxCols];
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) acc[c] = 0.0;
  for (int k = max(b, 0) + lane; k < e; k += 64) {
    const float *row = pcl + (size_t)perm[k] * C;
#pragma unroll
    for (int c = 0; c < kMaxCols; c++)
      if (c < C) acc[c] += (double)row[c];
  }
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    if (c < C) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 64);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < kMaxCols; c++)
      if (c < C) partial[(size_t)t * C + c] = acc[c];
  }
}

// One lane per voxel: the fp64 sum (rows in index order, or the chunk sums in chunk order), one division by the count,
// the normal scaled to unit length in fp64, one rounding to fp32; every output row is written once.
__global__ __launch_bounds__(256) void k_ds_rows(const float *__restrict__ pcl, int n, int C, int nc,
                                                 const int32_t *__restrict__ perm,
                                                 const int32_t *__restrict__ segstart,
                                                 const int32_t *__restrict__ choff, const double *__restrict__ partial,
                                                 const int32_t *__restrict__ rowof, const int32_t *__restrict__ info,
                                                 int m_host, int t_host, float *out, int32_t *counts) {
  const int M = min(m_host, info[kInfoM]), T = min(t_host, info[kInfoChunks]);
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= M) return;
  const int b = max(segstart[s], 0), e = min(segstart[s + 1], n), len = e - b;
  if (len <= 0) return;
  double acc[kMaxCols];
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) acc[c] = 0.0;
  if (len <= kShort) {
    for (int k = b; k < e; k++) {
      const float *row = pcl + (size_t)perm[k] * C;
#pragma unroll
      for (int c = 0; c < kMaxCols; c++)
        if (c < C) acc[c] += (double)row[c];
    }
  } else {
    const int t0 = choff[s], nchunks = chunks_of(len);
    for (int j = 0; j < nchunks && t0 + j < T; j++) {
#pragma unroll
      for (int c = 0; c < kMaxCols; c++)
        if (c < C) acc[c] += partial[(size_t)(t0 + j) * C + c];
    }
  }
  const double cnt = (double)len;
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) acc[c] = acc[c] / cnt;
  if (nc >= 0 && len > 1) {            // a point alone in its voxel stays as it is, bit for bit
    double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < kMaxCols; c++)
      if (c >= nc && c < nc + 3) v[c - nc] = acc[c];
    const double len2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    const double nl = sqrt(len2);
    if (nl > 0.0) {
#pragma unroll
      for (int c = 0; c < kMaxCols; c++)
        if (c >= nc && c < nc + 3) acc[c] = acc[c] / nl;
    }
  }
  const int r = rowof[perm[b]];
  if ((unsigned)r >= (unsigned)M) return;
  float *o = out + (size_t)r * C;
#pragma unroll
  for (int c = 0; c < kMaxCols; c++)
    if (c < C) o[c] = (float)acc[c];
  if (counts) counts[r] = len;
}

__global__ void k_ds_inverse(const uint64_t *__restrict__ key, const int32_t *__restrict__ perm,
                             const int32_t *__restrict__ hflag, const int32_t *__restrict__ hscan,
                             const int32_t *__restrict__ segstart, const int32_t *__restrict__ rowof, int n,
                             int32_t *inverse) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int i = perm[k];
  int r = -1;
  if (key[k] != kNoKey) {
    const int s = hscan[k] + hflag[k] - 1;
    const int b = segstart[s];
    if ((unsigned)b < (unsigned)n) r = rowof[perm[b]];
  }
  inverse[i] = r;
}

struct Layout {
  int32_t *info;
  uint32_t *cx, *cy, *cz, *ktmp;
  int32_t *perm_a, *perm_b, *segstart, *choff;
  uint64_t *key;
  double *partial;
  // what the arrays above become once the keys are built
  int32_t *hflag() const { return (int32_t *)cx; }
  int32_t *hscan() const { return (int32_t *)cy; }
  int32_t *isfirst() const { return (int32_t *)cz; }
  int32_t *rowof() const { return (int32_t *)ktmp; }
  int32_t *nch() const { return perm_a; }
};

size_t max_chunks(int n) { return (size_t)n / (kShort + 1) + 1; }   // a long segment has > 64 rows and <= len / 65 chunks

int carve(Arena &A, int n, int ncols, Layout &L) {
  const size_t N = (size_t)n + 2;
  D3D_ALLOC(info, int32_t, A, 64);
  D3D_ALLOC(cx, uint32_t, A, N);
  D3D_ALLOC(cy, uint32_t, A, N);
  D3D_ALLOC(cz, uint32_t, A, N);
  D3D_ALLOC(ktmp, uint32_t, A, N);
  D3D_ALLOC(perm_a, int32_t, A, N);
  D3D_ALLOC(perm_b, int32_t, A, N);
  D3D_ALLOC(segstart, int32_t, A, N);
  D3D_ALLOC(choff, int32_t, A, N);
  D3D_ALLOC(key, uint64_t, A, N);
  D3D_ALLOC(partial, double, A, max_chunks(n) * (size_t)ncols);
  L = Layout{info, cx, cy, cz, ktmp, perm_a, perm_b, segstart, choff, key, partial};
  return D3D_OK;
}

bool shape_ok(int n, int ncols) { return n >= 0 && n <= kMaxPoints && ncols >= 3 && ncols <= kMaxCols; }

// ---- cap ----
__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}
__host__ __device__ __forceinline__ uint32_t row_key(uint32_t i, uint32_t s0, uint32_t s1) {
  return mix32(mix32(i ^ s0) + s1);
}

// pass p: histogram of bits [24 - 8 p, 32 - 8 p) of the keys whose higher bits equal the prefix found so far
__global__ __launch_bounds__(256) void k_cap_hist(int n, uint32_t s0, uint32_t s1, int pass,
                                                  const uint32_t *__restrict__ sel, uint32_t *hist) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const uint32_t prefix = pass ? sel[0] : 0u;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t key = row_key((uint32_t)i, s0, s1);
    const uint32_t above = pass ? key >> (shift + 8) : 0u;
    if (above == prefix) atomicAdd(&h[(key >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[pass * 256 + threadIdx.x], h[threadIdx.x]);
}

// the digit in which the k-th smallest key lies; sel[0] = prefix so far, sel[1] = rank left among the keys under it
__global__ void k_cap_pick(const uint32_t *__restrict__ hist, int pass, int k, uint32_t *sel) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint32_t left = pass ? sel[1] : (uint32_t)k, prefix = pass ? sel[0] : 0u, cum = 0;
  int d = 0;
  for (; d < 255; d++) {
    const uint32_t c = hist[pass * 256 + d];
    if (cum + c >= left) break;
    cum += c;
  }
  sel[0] = (prefix << 8) | (uint32_t)d;
  sel[1] = left - cum;
}

__global__ void k_cap_flag(int n, uint32_t s0, uint32_t s1, const uint32_t *__restrict__ sel, int32_t *flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flag[i] = row_key((uint32_t)i, s0, s1) <= sel[0] ? 1 : 0;
}

__global__ void k_cap_write(int n, int k, const int32_t *__restrict__ flag, const int32_t *__restrict__ rank,
                            int32_t *rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const int r = rank[i];
  if ((unsigned)r < (unsigned)k) rows[r] = i;
}

__global__ void k_cap_iota(int32_t *p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = i;
}

}  // namespace
}  // namespace d3d

using namespace d3d;

size_t d3d_voxel_downsample_scratch_bytes(int n, int ncols) {
  const size_t N = (size_t)std::max(0, std::min(n, kMaxPoints)) + 2;
  const size_t C = (size_t)std::max(3, std::min(ncols, kMaxCols));
  return 512 + 8 * (N * 4 + 256) + (N * 8 + 256) + (max_chunks((int)N) * C * 8 + 256) +
         sort_scratch_bytes((int)N, kCellBits + 1) + 4096;
}

int d3d_voxel_downsample_cells(const float *pcl, int n, int ncols, double voxel, void *scratch, size_t scratch_bytes,
                               int *info_host, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(info_host, "d3d_voxel_downsample_cells: null pointer");
  info_host[0] = info_host[1] = 0;
  D3D_REQUIRE(shape_ok(n, ncols), "d3d_voxel_downsample_cells: %d rows of %d columns (at most 2^28 rows, 3 to 16 columns)",
              n, ncols);
  D3D_REQUIRE(voxel > 0.0 && voxel < (double)INFINITY, "d3d_voxel_downsample_cells: voxel %g must be positive and finite",
              voxel);
  if (n == 0) return D3D_OK;
  D3D_REQUIRE(pcl && scratch, "d3d_voxel_downsample_cells: null pointer");
  D3D_REQUIRE(scratch_bytes >= d3d_voxel_downsample_scratch_bytes(n, ncols), "d3d_voxel_downsample_cells: scratch too small");
  Arena A = scratch_arena(scratch, scratch_bytes);
  Layout L;
  int rc = carve(A, n, ncols, L);
  if (rc) return rc;
  const size_t mark = A.used;
  uint32_t *info_u = (uint32_t *)L.info;
  D3D_HIP_CHECK(hipMemsetAsync(L.info, 0, 64 * sizeof(int32_t), s));
  D3D_HIP_CHECK(hipMemsetAsync(L.info + kInfoMin, 0xFF, 3 * sizeof(int32_t), s));
  hipLaunchKernelGGL(k_ds_minmax, dim3(reduce_blocks(n)), dim3(256), 0, s, pcl, n, ncols, info_u);
  hipLaunchKernelGGL(k_ds_cells, grid1d(n), dim3(256), 0, s, pcl, n, ncols, (const uint32_t *)info_u, voxel, L.cx, L.cy,
                     L.cz, L.perm_a, L.info);
  D3D_LAUNCH_CHECK();
  // the order (x, y, z, index) into perm_b; the x digit is one bit wider: a dropped row carries kDropX
  rc = sort_cells_zyx(L.cx, L.cy, L.cz, L.perm_a, L.perm_b, L.ktmp, n, kCellBits, kCellBits + 1, A, s);
  if (rc) return rc;
  hipLaunchKernelGGL(k_ds_keys, grid1d(n), dim3(256), 0, s, (const int32_t *)L.perm_b, (const uint32_t *)L.cx,
                     (const uint32_t *)L.cy, (const uint32_t *)L.cz, n, L.key);
  // cx, cy, cz, ktmp and perm_a are free from here on
  hipLaunchKernelGGL(k_ds_heads, grid1d(n), dim3(256), 0, s, (const uint64_t *)L.key, (const int32_t *)L.perm_b, n,
                     L.hflag(), L.isfirst());
  D3D_LAUNCH_CHECK();
  rc = scan_exclusive_i32(L.hflag(), L.hscan(), n, L.info + kInfoM, A, s);
  if (rc) return rc;
  A.used = mark;
  rc = scan_exclusive_i32(L.isfirst(), L.rowof(), n, L.info + kInfoM2, A, s);
  if (rc) return rc;
  A.used = mark;
  hipLaunchKernelGGL(k_ds_segs, grid1d(n), dim3(256), 0, s, (const uint64_t *)L.key, (const int32_t *)L.hflag(),
                     (const int32_t *)L.hscan(), n, L.segstart);
  hipLaunchKernelGGL(k_ds_nch, grid1d(n), dim3(256), 0, s, (const int32_t *)L.segstart, (const int32_t *)L.info, n,
                     L.nch());
  D3D_LAUNCH_CHECK();
  rc = scan_exclusive_i32(L.nch(), L.choff, n, L.info + kInfoChunks, A, s);
  if (rc) return rc;
  A.used = mark;
  int32_t host[16];
  rc = readback_publish(L.info, 16, s);
  if (rc) return rc;
  rc = readback_wait(host, 16);
  if (rc) return rc;
  if (host[kInfoOverflow]) {
    double ext[3];
    for (int d = 0; d < 3; d++)
      ext[d] = (double)ordered_to_f32((uint32_t)host[kInfoMax + d]) - (double)ordered_to_f32((uint32_t)host[kInfoMin + d]);
    set_error("d3d_voxel_downsample: the cloud spans %.9g x %.9g x %.9g m, more than the limit of 2^21 = 2097152 cells of "
              "%.9g m per axis (%.9g m)", ext[0], ext[1], ext[2], voxel, voxel * 2097152.0);
    return D3D_ERR_ARG;
  }
  info_host[0] = host[kInfoM];
  info_host[1] = host[kInfoChunks];
  return D3D_OK;
}

int d3d_voxel_downsample_rows(const float *pcl, int n, int ncols, int normal_col, const int *info_host,
                              const void *scratch, size_t scratch_bytes, float *out, int32_t *inverse, int32_t *counts,
                              void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(info_host, "d3d_voxel_downsample_rows: null pointer");
  D3D_REQUIRE(shape_ok(n, ncols), "d3d_voxel_downsample_rows: %d rows of %d columns (at most 2^28 rows, 3 to 16 columns)", n,
              ncols);
  D3D_REQUIRE(normal_col == -1 || (normal_col >= 0 && normal_col + 3 <= ncols),
              "d3d_voxel_downsample_rows: normal column %d of %d columns", normal_col, ncols);
  if (n == 0) return D3D_OK;
  const int M = info_host[0], T = info_host[1];
  D3D_REQUIRE(M >= 0 && M <= n && T >= 0 && (size_t)T <= max_chunks(n), "d3d_voxel_downsample_rows: bad counts %d, %d", M, T);
  D3D_REQUIRE(pcl && scratch && (out || M == 0), "d3d_voxel_downsample_rows: null pointer");
  D3D_REQUIRE(scratch_bytes >= d3d_voxel_downsample_scratch_bytes(n, ncols), "d3d_voxel_downsample_rows: scratch too small");
  Arena A = scratch_arena(scratch, scratch_bytes);
  Layout L;
  const int rc = carve(A, n, ncols, L);
  if (rc) return rc;
  if (M > 0 && T > 0)
    hipLaunchKernelGGL(k_ds_partial, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, s, pcl, n, ncols,
                       (const int32_t *)L.perm_b, (const int32_t *)L.segstart, (const int32_t *)L.choff,
                       (const int32_t *)L.info, M, T, L.partial);
  if (M > 0)
    hipLaunchKernelGGL(k_ds_rows, grid1d(M), dim3(256), 0, s, pcl, n, ncols, normal_col, (const int32_t *)L.perm_b,
                       (const int32_t *)L.segstart, (const int32_t *)L.choff, (const double *)L.partial,
                       (const int32_t *)L.rowof(), (const int32_t *)L.info, M, T, out, counts);
  if (inverse)
    hipLaunchKernelGGL(k_ds_inverse, grid1d(n), dim3(256), 0, s, (const uint64_t *)L.key, (const int32_t *)L.perm_b,
                       (const int32_t *)L.hflag(), (const int32_t *)L.hscan(), (const int32_t *)L.segstart,
                       (const int32_t *)L.rowof(), n, inverse);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

size_t d3d_sample_rows_scratch_bytes(int n) {
  const size_t N = (size_t)std::max(n, 1);
  return 4 * 256 * 4 + 256 + 2 * (N * 4 + 256) + ((N + 2047) / 2048) * 4 + 4096;
}

int d3d_sample_rows(int n, int k, uint64_t seed, int32_t *rows, void *scratch, size_t scratch_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(n >= 0 && k >= 0, "d3d_sample_rows: n %d, k %d", n, k);
  if (n == 0 || k == 0) return D3D_OK;
  D3D_REQUIRE(rows, "d3d_sample_rows: null pointer");
  if (k >= n) {
    hipLaunchKernelGGL(k_cap_iota, grid1d(n), dim3(256), 0, s, rows, n);
    D3D_LAUNCH_CHECK();
    return D3D_OK;
  }
  D3D_REQUIRE(scratch && scratch_bytes >= d3d_sample_rows_scratch_bytes(n), "d3d_sample_rows: scratch too small");
  Arena A = scratch_arena(scratch, scratch_bytes);
  D3D_ALLOC(hist, uint32_t, A, 4 * 256 + 16);
  uint32_t *sel = hist + 4 * 256;
  D3D_ALLOC(flag, int32_t, A, n);
  D3D_ALLOC(rank, int32_t, A, n);
  const uint32_t s0 = mix32((uint32_t)seed + 0x9e3779b9U), s1 = mix32((uint32_t)(seed >> 32) ^ s0);
  D3D_HIP_CHECK(hipMemsetAsync(hist, 0, (4 * 256 + 16) * sizeof(uint32_t), s));
  for (int pass = 0; pass < 4; pass++) {
    hipLaunchKernelGGL(k_cap_hist, dim3(reduce_blocks(n)), dim3(256), 0, s, n, s0, s1, pass, (const uint32_t *)sel, hist);
    hipLaunchKernelGGL(k_cap_pick, dim3(1), dim3(64), 0, s, (const uint32_t *)hist, pass, k, sel);
  }
  hipLaunchKernelGGL(k_cap_flag, grid1d(n), dim3(256), 0, s, n, s0, s1, (const uint32_t *)sel, flag);
  D3D_LAUNCH_CHECK();
  const int rc = scan_exclusive_i32(flag, rank, n, nullptr, A, s);
  if (rc) return rc;
  hipLaunchKernelGGL(k_cap_write, grid1d(n), dim3(256), 0, s, n, k, (const int32_t *)flag, (const int32_t *)rank, rows);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}
