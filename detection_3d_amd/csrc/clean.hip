// Cleaning a raw scan before it is voxelised: the neighbour count of every point, its mean distance to its k nearest
// neighbours with the cloud's mean and deviation of those, and the connected components of the "within r" graph.  The
// three of open3d's remove_radius_outlier, remove_statistical_outlier (on a hybrid search) and a clustering pass that
// the reference's users run on the CPU; restatements, not pinned against open3d.
//
// All three are consumers of the cell list of normals.hip (celllist::build, d3d_internal.h) and walk it as
// k_nrm_search does: one workgroup per kSpan sorted queries, the span cell by cell, the 27 neighbour cells staged into
// LDS when they hold at most kBudget points and read from global memory otherwise, one query per lane group of 8.
// Distances are one_query's: d2 = (dx dx + dy dy) + dz dz in fp32 from the fp32 offset, d2 <= r2 by bit comparison.
// No float atomics, every sum in an order fixed by the data: the same input gives the same bits.
#include "d3d_internal.h"

#include <algorithm>

namespace d3d {

namespace {

using namespace celllist;
constexpr int kThreads = 128;                     // 16 lane groups of 8, one query per group at a time
constexpr int kGroup = 8;
constexpr int kGroups = kThreads / kGroup;
constexpr int kSpan = 64;                         // sorted queries per workgroup
constexpr int kBudget = 1024;                     // staged candidates (16 KiB of LDS); beyond: read from global memory
constexpr int kStatRows = 1024;                   // rows per block of the statistics' first launch
constexpr int kStatThreads = 256;

struct Ranges {     // the 27 neighbour cells' candidates: positions in `pts` and, when staged, in the LDS copy
  int gb[27], ge[27], lb[27];
};

// f(C, pos) for the candidates of one query that lane gl of its group takes: l, l + 8, ... of every cell, cells in a
// fixed order; pos is the candidate's sorted position
template <bool STAGED, class F>
__device__ __forceinline__ void for_candidates(const float4 *__restrict__ pts, const float4 *cand, const Ranges &R, int gl,
                                               F f) {
#pragma unroll 1                      // unrolled 27-fold, the count query took 255 registers and one wave per SIMD
  for (int r = 0; r < 27; r++) {
    const int len = R.ge[r] - R.gb[r];
    for (int t = gl; t < len; t += kGroup) {
      const float4 C = STAGED ? cand[R.lb[r] + t] : pts[R.gb[r] + t];
      f(C, R.gb[r] + t);
    }
  }
}

__device__ __forceinline__ uint32_t dist2_bits(float4 C, float4 P) {
  const float dx = C.x - P.x, dy = C.y - P.y, dz = C.z - P.z;
  return __float_as_uint((dx * dx + dy * dy) + dz * dz);
}

__device__ __forceinline__ int group_sum(int c) {
#pragma unroll
  for (int o = kGroup / 2; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
  return c;
}

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
// found[i] = the kept candidates - 1; found < k: mean = +inf.  The cut is one_query's (normals.hip):
//   keep(d2, j) = d2 < T or (d2 == T and j <= J): T the (k+1)-th smallest d2, J the cut among the candidates tied at T.
struct KnnQuery {
  uint32_t r2_bits;
  int k, n;
  double *mean;
  int32_t *found;
  template <bool STAGED>
  __device__ __forceinline__ void run(const float4 *__restrict__ pts, const float4 *cand, const Ranges &R, int q, float4 P,
                                      int gl) const {
    auto count_kept = [&](uint32_t T, int J) {
      int c = 0;
      for_candidates<STAGED>(pts, cand, R, gl, [&](float4 C, int) {
        const uint32_t u = dist2_bits(C, P);
        c += (u < T || (u == T && __float_as_int(C.w) <= J)) ? 1 : 0;
      });
      return group_sum(c);
    };
    const int want = k + 1;
    uint32_t T = r2_bits;
    int J = 0x7fffffff;
    int m = count_kept(T, J);
    if (m > want) {
      uint32_t lo = 0, hi = T;          // invariant: count(d2 <= hi) = m_hi >= want
      int m_hi = m;
      while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const int c = count_kept(mid, J);
        if (c >= want) {
          hi = mid;
          m_hi = c;
        } else {
          lo = mid + 1;
        }
      }
      T = hi;
      if (m_hi > want) {                // ties at T: the smallest J with count(.., J) >= want, then exactly `want`
        int jl = 0, jh = n - 1;
        while (jl < jh) {
          const int mid = jl + (jh - jl) / 2;
          if (count_kept(T, mid) >= want) jh = mid;
          else jl = mid + 1;
        }
        J = jh;
      }
      m = want;
    }
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

// Lock-free union-find over the sorted positions.  par[x] <= x always and only ever decreases, every value it takes is a
// member of x's component, and every access inside the linking kernel is a device-scope atomic, so that no CU works on
// a cached copy.  Nothing here waits for another thread's store: a failed compare-and-swap returns the value that beat
// it, and the loop goes on from that value, strictly downwards.
__device__ __forceinline__ int uf_load(int32_t *par, int x) {
  return __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int uf_find(int32_t *par, int x) {
  while (true) {                        // path halving; x strictly decreases
    const int p = uf_load(par, x);
    if (p == x) return x;
    const int g = uf_load(par, p);
    if (g == p) return p;
    atomicMin(par + x, g);
    x = g;
  }
}
__device__ __forceinline__ void uf_unite(int32_t *par, int a, int b) {
  while (true) {                        // a + b strictly decreases
    a = uf_find(par, a);
    b = uf_find(par, b);
    if (a == b) return;
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicCAS(par + hi, hi, lo);      // hook a root under the lower id
    if (old == hi) return;
    a = old;                            // hi had been hooked meanwhile: go on from its parent
    b = lo;
  }
}

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

// k_nrm_search's walk with the query left open.  One workgroup per kSpan sorted queries.  The span is walked cell by
// cell: the 27 neighbour cells' ranges come from the table, their points are staged into LDS once (when they fit) and
// every query of the cell in the span reuses them.
template <class Q>
__global__ __launch_bounds__(kThreads) void k_cln_walk(const float4 *__restrict__ pts, const uint64_t *__restrict__ key,
                                                       int n, const HashEntry *__restrict__ tab, int cap, Q query) {
  __shared__ float4 cand[kBudget];
  __shared__ Ranges R;
  __shared__ int s_next, s_total;
  const int tid = threadIdx.x, grp = tid / kGroup, gl = tid % kGroup;
  int k = blockIdx.x * kSpan;
  const int kend = min(n, k + kSpan);
  while (k < kend) {                  // uniform over the workgroup
    const uint64_t ck = key[k];
    if (tid == 0) s_next = kend;
    __syncthreads();
    for (int t = k + 1 + tid; t < kend; t += kThreads)
      if (key[t] != ck) {
        atomicMin(&s_next, t);
        break;
      }
    if (tid < 27) {
      const int cx = (int)(ck >> (2 * kCellBits)) + tid / 9 - 1;
      const int cy = (int)((ck >> kCellBits) & kCellMax) + (tid / 3) % 3 - 1;
      const int cz = (int)(ck & kCellMax) + tid % 3 - 1;
      int2 g = make_int2(0, 0);
      if (cx >= 0 && cx <= kCellMax && cy >= 0 && cy <= kCellMax && cz >= 0 && cz <= kCellMax)
        g = cell_range(tab, cap, cell_key((uint32_t)cx, (uint32_t)cy, (uint32_t)cz));
      g.x = max(0, min(g.x, n));      // whatever the table holds, no range leaves the sorted points
      g.y = max(g.x, min(g.y, n));
      R.gb[tid] = g.x;
      R.ge[tid] = g.y;
    }
    __syncthreads();
    if (tid == 0) {
      int tot = 0;
      for (int r = 0; r < 27; r++) {
        R.lb[r] = tot;
        tot += R.ge[r] - R.gb[r];
      }
      s_total = tot;
    }
    __syncthreads();
    const int e = s_next;
    const bool staged = s_total <= kBudget;
    if (staged) {
      for (int r = grp; r < 27; r += kGroups) {
        const int len = R.ge[r] - R.gb[r];
        for (int t = gl; t < len; t += kGroup) cand[R.lb[r] + t] = pts[R.gb[r] + t];
      }
    }
    __syncthreads();
    for (int q = k + grp; q < e; q += kGroups) {
      if (staged) query.template run<true>(pts, cand, R, q, pts[q], gl);
      else query.template run<false>(pts, cand, R, q, pts[q], gl);
    }
    __syncthreads();
    k = e;
  }
}

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

// ---- connected components: after the linking ----
__global__ void k_cln_iota(int32_t *par, int n) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) par[k] = k;
}

// root of every sorted position (par is only read here), and per root the smallest original index and the point count:
// integer min and add, which commute.  A wave first gathers the lanes that share a root, so that a component of a
// whole building does not send one atomic per point to one address.
__global__ __launch_bounds__(256) void k_cln_roots(const int32_t *__restrict__ par, const float4 *__restrict__ pts, int n,
                                                   int32_t *root, int32_t *min_index, int32_t *size) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool active = k < n;
  int r = -1, idx = 0x7fffffff;
  if (active) {
    r = k;
    while (true) {
      const int p = par[r];
      if (p == r) break;
      r = p;
    }
    root[k] = r;
    idx = __float_as_int(pts[k].w);
  }
  unsigned long long todo = __ballot(active);
  while (todo) {                      // uniform over the wave; every round retires at least its leader
    const int leader = __ffsll((long long)todo) - 1;
    const int lr = __shfl(r, leader, 64);
    const bool same = active && r == lr;
    const unsigned long long m = __ballot(same);
    int v = same ? idx : 0x7fffffff;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = min(v, __shfl_xor(v, s, 64));
    if (lane == leader) {
      atomicAdd(size + lr, __popcll(m));
      atomicMin(min_index + lr, v);
    }
    todo &= ~m;
    active = active && !same;
  }
}

__global__ void k_cln_labels(const int32_t *__restrict__ root, const float4 *__restrict__ pts, int n,
                             const int32_t *__restrict__ min_index, const int32_t *__restrict__ csize, int32_t *label,
                             int32_t *size) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int i = __float_as_int(pts[k].w), r = root[k];
  label[i] = min_index[r];
  size[i] = csize[r];
}

// ---- host side ----
constexpr int kPhases = 5;            // cells, sort, table, search, tail

struct Timer {                        // events around the phases when the caller asked for their times
  hipEvent_t ev[kPhases + 1] = {};
  bool on = false;
  int start(bool want) {
    on = want;
    if (on)
      for (int k = 0; k <= kPhases; k++) D3D_HIP_CHECK(hipEventCreate(&ev[k]));
    return D3D_OK;
  }
  int mark(int k, hipStream_t s) {
    if (on) D3D_HIP_CHECK(hipEventRecord(ev[k], s));
    return D3D_OK;
  }
  int finish(float *ms) {
    if (!on) return D3D_OK;
    D3D_HIP_CHECK(hipEventSynchronize(ev[kPhases]));
    for (int k = 0; k < kPhases; k++) D3D_HIP_CHECK(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
    for (int k = 0; k <= kPhases; k++) (void)hipEventDestroy(ev[k]);
    return D3D_OK;
  }
};

bool args_ok(int n, int stride, float radius) {
  return n >= 0 && n <= kMaxPoints && stride >= 3 && radius > 0.f && radius < INFINITY;
}

// the bits of the fp32 product r r: the kernels compare distances as integers
uint32_t r2_bits(float radius) { return __builtin_bit_cast(uint32_t, radius * radius); }

void zero_phases(float *ms) {
  if (ms)
    for (int k = 0; k < kPhases; k++) ms[k] = 0.f;
}

int stat_blocks(int n) { return (int)(((long)std::max(n, 1) + kStatRows - 1) / kStatRows); }

template <class Q>
int launch_walk(const CellList &L, int n, Q q, hipStream_t s) {
  hipLaunchKernelGGL(k_cln_walk<Q>, dim3((unsigned)((n + kSpan - 1) / kSpan)), dim3(kThreads), 0, s, L.pts, L.key, n, L.tab,
                     L.cap, q);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

#define CLN_TRY(expr)        \
  do {                       \
    const int rc_ = (expr);  \
    if (rc_) return rc_;     \
  } while (0)

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
  CLN_TRY(T.start(phase_ms_host != nullptr));
  Arena A = scratch_arena(scratch, scratch_bytes);
  celllist::CellList L;
  CLN_TRY(celllist::build(xyz, n, row_stride_floats, radius, A, s, &L, T.on ? T.ev : nullptr));
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
  CLN_TRY(T.start(phase_ms_host != nullptr));
  Arena A = scratch_arena(scratch, scratch_bytes);
  const int nb = stat_blocks(n);
  D3D_ALLOC(part, StatPartial, A, nb);
  celllist::CellList L;
  CLN_TRY(celllist::build(xyz, n, row_stride_floats, radius, A, s, &L, T.on ? T.ev : nullptr));
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
  CLN_TRY(T.start(phase_ms_host != nullptr));
  Arena A = scratch_arena(scratch, scratch_bytes);
  D3D_ALLOC(par, int32_t, A, n);
  D3D_ALLOC(root, int32_t, A, n);
  D3D_ALLOC(min_index, int32_t, A, n);
  D3D_ALLOC(csize, int32_t, A, n);
  celllist::CellList L;
  CLN_TRY(celllist::build(xyz, n, row_stride_floats, radius, A, s, &L, T.on ? T.ev : nullptr));
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
