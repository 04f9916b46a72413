// Cleaning a raw scan before it is voxelised: the neighbour count of every point, its mean distance to its k nearest
// neighbours with the cloud's mean and deviation of those, and the connected components of the "within r" graph.  The
// three of open3d's remove_radius_outlier, remove_statistical_outlier (on a hybrid search) and a clustering pass that
// the reference's users run on the CPU; restatements, not pinned against open3d.
//
// All three are consumers of the cell list (celllist::build, celllist.hip) and queries of the one walk over it
// (cell_walk.inc): one workgroup per kSpan sorted queries, the span cell by cell, the 27 neighbour cells staged into
// LDS when they hold at most kBudget points and read from global memory otherwise, one query per lane group of 8.  The
// union-find and its labelling tail: union_find.inc, shared with planes.hip.
// Distances are dist2_bits': d2 = (dx dx + dy dy) + dz dz in fp32 from the fp32 offset, d2 <= r2 by bit comparison.
// No float atomics, every sum in an order fixed by the data: the same input gives the same bits.
#include "d3d_internal.h"

#include <algorithm>

namespace d3d {

namespace {

using namespace celllist;
#include "cell_walk.inc"
#include "union_find.inc"

constexpr int kStatRows = 1024;                   // rows per block of the statistics' first launch
constexpr int kStatThreads = 256;

// count[i] = the points within r of point i, itself included
struct CountQuery {
  uint32_t r2_bits;
  int32_t *count;
  template <bool STAGED>
  __device__ __forceinline__ void run(const float4 *__restrict__ pts, const float4 *cand, const Ranges &R, int q, float4 P,
                                      int gl) const {
    int c = 0;
    // d2 <= r2 <=> bits(d2) <= bits(r2); a NaN distance has larger bits than any finite r2 and is never counted
    for_candidates<STAGED>(pts, cand, R, gl, [&](float4 C, int) { c += dist2_bits(C, P) <= r2_bits ? 1 : 0; });
    c = group_sum(c);
    if (gl == 0) count[__float_as_int(P.w)] = c;
  }
};

// mean[i] = (sum of sqrt(double(d2)) over the k + 1 nearest candidates by (d2, j), the point itself among them) / k,
// found[i] = the kept candidates - 1; found < k: mean = +inf.  The cut is nearest_cut's (cell_walk.inc), want = k + 1.
struct KnnQuery {
  uint32_t r2_bits;
  int k, n;
  double *mean;
  int32_t *found;
  template <bool STAGED>
  __device__ __forceinline__ void run(const float4 *__restrict__ pts, const float4 *cand, const Ranges &R, int q, float4 P,
                                      int gl) const {
    uint32_t T = r2_bits;
    int J;
    const int m = nearest_cut<STAGED>(pts, cand, R, P, gl, k + 1, n, T, J);
    double s = 0.0;                     // lane order, then the lanes pairwise: fixed by the data
    for_candidates<STAGED>(pts, cand, R, gl, [&](float4 C, int) {
      const uint32_t u = dist2_bits(C, P);
      if (u < T || (u == T && __float_as_int(C.w) <= J)) s += sqrt((double)__uint_as_float(u));
    });
#pragma unroll
    for (int o = kGroup / 2; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (gl != 0) return;
    const int i = __float_as_int(P.w);
    found[i] = m - 1;
    mean[i] = m - 1 < k ? (double)INFINITY : s / (double)k;
  }
};

// every point links to its neighbours of lower sorted position
struct LinkQuery {
  uint32_t r2_bits;
  int32_t *par;
  template <bool STAGED>
  __device__ __forceinline__ void run(const float4 *__restrict__ pts, const float4 *cand, const Ranges &R, int q, float4 P,
                                      int gl) const {
    for_candidates<STAGED>(pts, cand, R, gl, [&](float4 C, int pos) {
      if (pos < q && dist2_bits(C, P) <= r2_bits) uf_unite(par, q, pos);
    });
  }
};

// ---- mean and deviation of the finite means, fp64, fixed order, no atomics ----
// A block's sum: lanes pairwise, then the waves in order.  Every thread gets the result.
__device__ __forceinline__ double block_sum(double v, double *lds /* [blockDim / 64] */) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  __syncthreads();                    // the previous use of lds is over
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < (int)(blockDim.x >> 6); w++) t += lds[w];
  return t;
}

struct StatPartial {
  double count, sum, m2;              // of the finite means of kStatRows rows: how many, their sum, and the sum of their
};                                    // squared deviations from the block's own mean

// first launch: block b takes rows [b kStatRows, (b + 1) kStatRows), thread t rows t, t + 256, ... of them
__global__ __launch_bounds__(kStatThreads) void k_cln_stat_partial(const double *__restrict__ mean, int n, StatPartial *part) {
  __shared__ double lds[kStatThreads / 64];
  const int base = blockIdx.x * kStatRows;
  double v[kStatRows / kStatThreads];
  double c = 0.0, s = 0.0;
#pragma unroll
  for (int j = 0; j < kStatRows / kStatThreads; j++) {
    const int i = base + j * kStatThreads + threadIdx.x;
    v[j] = i < n ? mean[i] : (double)INFINITY;
    if (v[j] < (double)INFINITY) {
      c += 1.0;
      s += v[j];
    }
  }
  c = block_sum(c, lds);
  s = block_sum(s, lds);
  const double mu = c > 0.0 ? s / c : 0.0;
  double q = 0.0;
#pragma unroll
  for (int j = 0; j < kStatRows / kStatThreads; j++)
    if (v[j] < (double)INFINITY) q += (v[j] - mu) * (v[j] - mu);
  q = block_sum(q, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = StatPartial{c, s, q};
}

// second launch, one block: the first pass over the partials gives the mean, the second the squared deviations about
// it (a block's own plus count (block mean - mean)^2), divided by (count - 1).  stats = (mean, deviation); no finite
// mean at all: (0, 0); a single one: deviation 0.
__global__ __launch_bounds__(1024) void k_cln_stat_finish(const StatPartial *__restrict__ part, int nb, double *stats) {
  __shared__ double lds[16];
  double c = 0.0, s = 0.0;
  for (int b = threadIdx.x; b < nb; b += blockDim.x) {
    c += part[b].count;
    s += part[b].sum;
  }
  c = block_sum(c, lds);
  s = block_sum(s, lds);
  const double mu = c > 0.0 ? s / c : 0.0;
  double q = 0.0;
  for (int b = threadIdx.x; b < nb; b += blockDim.x) {
    const StatPartial p = part[b];
    if (p.count > 0.0) {
      const double d = p.sum / p.count - mu;
      q += p.m2 + p.count * (d * d);
    }
  }
  q = block_sum(q, lds);
  if (threadIdx.x == 0) {
    stats[0] = mu;
    stats[1] = c > 1.0 ? sqrt(q / (c - 1.0)) : 0.0;
  }
}

__global__ void k_cln_stat_keep(const double *__restrict__ mean, int n, const double *__restrict__ stats, double ratio,
                                uint8_t *keep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double m = mean[i];
  keep[i] = (m < (double)INFINITY && m <= stats[0] + ratio * stats[1]) ? 1 : 0;
}

// ---- host side ----
int stat_blocks(int n) { return (int)(((long)std::max(n, 1) + kStatRows - 1) / kStatRows); }

}  // namespace
}  // namespace d3d

using namespace d3d;

size_t d3d_radius_neighbors_scratch_bytes(int n) {
  if (n <= 0) return 256;
  return celllist::scratch_bytes(n);
}

int d3d_radius_neighbors(const float *xyz, int n, int row_stride_floats, float radius, int32_t *count, void *scratch,
                         size_t scratch_bytes, void *stream, float *phase_ms_host) {
  D3D_REQUIRE(args_ok(n, row_stride_floats, radius), "d3d_radius_neighbors: bad point count, row stride or radius");
  if (n == 0) {
    zero_phases(phase_ms_host);
    return D3D_OK;
  }
  D3D_REQUIRE(xyz && count && scratch, "d3d_radius_neighbors: null pointer");
  D3D_REQUIRE(scratch_bytes >= d3d_radius_neighbors_scratch_bytes(n), "d3d_radius_neighbors: scratch too small");
  hipStream_t s = (hipStream_t)stream;
  Timer T;
  CLN_TRY(T.start(phase_ms_host != nullptr, kPhases + 1));
  Arena A = scratch_arena(scratch, scratch_bytes);
  celllist::CellList L;
  CLN_TRY(celllist::build(xyz, n, row_stride_floats, radius, A, s, &L, T.events()));
  CLN_TRY(launch_walk(L, n, CountQuery{r2_bits(radius), count}, s));
  CLN_TRY(T.mark(4, s));
  CLN_TRY(T.mark(5, s));
  return T.finish(phase_ms_host);
}

size_t d3d_knn_mean_distance_scratch_bytes(int n) {
  if (n <= 0) return 256;
  const int N = std::min(n, celllist::kMaxPoints);
  return celllist::scratch_bytes(N) + (size_t)stat_blocks(N) * sizeof(StatPartial) + 256;
}

int d3d_knn_mean_distance(const float *xyz, int n, int row_stride_floats, float radius, int k, double std_ratio,
                          double *mean, int32_t *found, double *stats, uint8_t *keep, void *scratch,
                          size_t scratch_bytes, void *stream, float *phase_ms_host) {
  D3D_REQUIRE(args_ok(n, row_stride_floats, radius), "d3d_knn_mean_distance: bad point count, row stride or radius");
  D3D_REQUIRE(k >= 1 && k < celllist::kMaxPoints, "d3d_knn_mean_distance: k < 1");
  D3D_REQUIRE(stats, "d3d_knn_mean_distance: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    D3D_HIP_CHECK(hipMemsetAsync(stats, 0, 2 * sizeof(double), s));
    zero_phases(phase_ms_host);
    return D3D_OK;
  }
  D3D_REQUIRE(xyz && mean && found && scratch, "d3d_knn_mean_distance: null pointer");
  D3D_REQUIRE(scratch_bytes >= d3d_knn_mean_distance_scratch_bytes(n), "d3d_knn_mean_distance: scratch too small");
  Timer T;
  CLN_TRY(T.start(phase_ms_host != nullptr, kPhases + 1));
  Arena A = scratch_arena(scratch, scratch_bytes);
  const int nb = stat_blocks(n);
  D3D_ALLOC(part, StatPartial, A, nb);
  celllist::CellList L;
  CLN_TRY(celllist::build(xyz, n, row_stride_floats, radius, A, s, &L, T.events()));
  CLN_TRY(launch_walk(L, n, KnnQuery{r2_bits(radius), k, n, mean, found}, s));
  CLN_TRY(T.mark(4, s));
  hipLaunchKernelGGL(k_cln_stat_partial, dim3((unsigned)nb), dim3(kStatThreads), 0, s, (const double *)mean, n, part);
  hipLaunchKernelGGL(k_cln_stat_finish, dim3(1), dim3(1024), 0, s, (const StatPartial *)part, nb, stats);
  if (keep)
    hipLaunchKernelGGL(k_cln_stat_keep, grid1d(n), dim3(256), 0, s, (const double *)mean, n, (const double *)stats, std_ratio,
                       keep);
  D3D_LAUNCH_CHECK();
  CLN_TRY(T.mark(5, s));
  return T.finish(phase_ms_host);
}

size_t d3d_connected_components_scratch_bytes(int n) {
  if (n <= 0) return 256;
  const size_t N = (size_t)std::min(n, celllist::kMaxPoints);
  return celllist::scratch_bytes((int)N) + 4 * (N * 4 + 256);
}

int d3d_connected_components(const float *xyz, int n, int row_stride_floats, float radius, int32_t *label, int32_t *size,
                             void *scratch, size_t scratch_bytes, void *stream, float *phase_ms_host) {
  D3D_REQUIRE(args_ok(n, row_stride_floats, radius), "d3d_connected_components: bad point count, row stride or radius");
  if (n == 0) {
    zero_phases(phase_ms_host);
    return D3D_OK;
  }
  D3D_REQUIRE(xyz && label && size && scratch, "d3d_connected_components: null pointer");
  D3D_REQUIRE(scratch_bytes >= d3d_connected_components_scratch_bytes(n), "d3d_connected_components: scratch too small");
  hipStream_t s = (hipStream_t)stream;
  Timer T;
  CLN_TRY(T.start(phase_ms_host != nullptr, kPhases + 1));
  Arena A = scratch_arena(scratch, scratch_bytes);
  D3D_ALLOC(par, int32_t, A, n);
  D3D_ALLOC(root, int32_t, A, n);
  D3D_ALLOC(min_index, int32_t, A, n);
  D3D_ALLOC(csize, int32_t, A, n);
  celllist::CellList L;
  CLN_TRY(celllist::build(xyz, n, row_stride_floats, radius, A, s, &L, T.events()));
  hipLaunchKernelGGL(k_cln_iota, grid1d(n), dim3(256), 0, s, par, n);
  D3D_HIP_CHECK(hipMemsetAsync(min_index, 0x7F, (size_t)n * 4, s));      // above every index
  D3D_HIP_CHECK(hipMemsetAsync(csize, 0, (size_t)n * 4, s));
  CLN_TRY(launch_walk(L, n, LinkQuery{r2_bits(radius), par}, s));
  CLN_TRY(T.mark(4, s));
  hipLaunchKernelGGL(k_cln_roots, grid1d(n), dim3(256), 0, s, (const int32_t *)par, L.pts, n, root, min_index, csize);
  hipLaunchKernelGGL(k_cln_labels, grid1d(n), dim3(256), 0, s, (const int32_t *)root, L.pts, n, (const int32_t *)min_index,
                     (const int32_t *)csize, label, size);
  D3D_LAUNCH_CHECK();
  CLN_TRY(T.mark(5, s));
  return T.finish(phase_ms_host);
}
