// Point normals for clouds that come without them (data3d/indoor_data_util.py:73-76, add_norm: open3d's hybrid search of
// radius r and at most max_nn neighbours, then the smallest eigenvector of the neighbours' covariance).
//
// Semantics (a restatement of the hybrid search, not pinned against open3d): the candidates of point i are
// all j, i included, with d2 = (dx dx + dy dy) + dz dz <= r r, everything in fp32 from the fp32 offset p_j - p_i; more
// than max_nn of them are cut to the max_nn smallest by (d2, j); count < 3 or coincident points give (0, 0, 1);
// otherwise the unit eigenvector of the smallest eigenvalue of the kept points' covariance, signed so that its largest
// component is positive (or so that it faces a viewpoint).  No float atomics and a fixed summation order: the same
// input gives the same bits.
//
// Passes: per-axis min -> cell coordinates (cells of edge 1.0001 r, so that a neighbour is never two cells away) ->
// three stable radix sorts (z, y, x: z is the fastest digit of the order) -> sorted points and their 60-bit cell keys
// -> open-addressing table cell -> [first, last) -> k_nrm_search.
#include "d3d_internal.h"

#include <algorithm>

namespace d3d {

namespace {

using namespace celllist;                         // kCellBits, kCellMax, cell_key, cell_range, table_cap (d3d_internal.h)
constexpr int kThreads = 128;                     // k_nrm_search: 16 lane groups of 8, one query per group at a time
constexpr int kGroup = 8;
constexpr int kGroups = kThreads / kGroup;
constexpr int kSpan = 64;                         // sorted queries per workgroup
constexpr int kBudget = 1024;                     // staged candidates (16 KiB of LDS); beyond: read from global memory
#include "eigen3.inc"

// per-axis min: grid-stride, wave shuffle, LDS, one integer atomic per block and axis -- order-independent
__global__ __launch_bounds__(256) void k_nrm_min(const float *__restrict__ xyz, int n, int stride, uint32_t *red) {
  __shared__ float lds[4][3];
  float v[3] = {INFINITY, INFINITY, INFINITY};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    for (int d = 0; d < 3; d++) v[d] = fminf(v[d], xyz[(size_t)i * stride + d]);
  for (int d = 0; d < 3; d++) {
    float x = v[d];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x = fminf(x, __shfl_xor(x, s, 64));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6][d] = x;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int d = threadIdx.x;
    const float x = fminf(fminf(lds[0][d], lds[1][d]), fminf(lds[2][d], lds[3][d]));
    atomicMin(&red[d], f32_ordered(x));
  }
}

// cell coordinate floor((p - min) / h) per axis in fp64 (p - min is exact there), clamped; anything unordered -> 0
__global__ void k_nrm_cells(const float *__restrict__ xyz, int n, int stride, const uint32_t *__restrict__ red, double h,
                            uint32_t *cx, uint32_t *cy, uint32_t *cz, int32_t *iota) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t c[3];
  for (int d = 0; d < 3; d++) {
    const double q = floor(((double)xyz[(size_t)i * stride + d] - (double)ordered_to_f32(red[d])) / h);
    c[d] = q >= 0.0 ? (q < (double)kCellMax ? (uint32_t)q : (uint32_t)kCellMax) : 0u;
  }
  cx[i] = c[0];
  cy[i] = c[1];
  cz[i] = c[2];
  iota[i] = i;
}

__global__ void k_nrm_gather(const uint32_t *__restrict__ src, const int32_t *__restrict__ perm, int n, uint32_t *dst) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) dst[k] = src[perm[k]];
}

// the points in cell order: (x, y, z, original index) and the cell key of every sorted position
__global__ void k_nrm_sorted(const float *__restrict__ xyz, int n, int stride, const int32_t *__restrict__ perm,
                             const uint32_t *__restrict__ cx, const uint32_t *__restrict__ cy,
                             const uint32_t *__restrict__ cz, float4 *pts, uint64_t *key) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int i = perm[k];
  const float *p = xyz + (size_t)i * stride;
  pts[k] = make_float4(p[0], p[1], p[2], __int_as_float(i));
  key[k] = cell_key(cx[i], cy[i], cz[i]);
}

// cell -> [val, first) of the sorted positions: the first position of a cell stores val, the last one first; one
// thread each, so no two threads write the same word
__global__ void k_nrm_table(const uint64_t *__restrict__ key, int n, HashEntry *tab, int cap) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint64_t c = key[k];
  const bool head = k == 0 || key[k - 1] != c, tail = k == n - 1 || key[k + 1] != c;
  if (!head && !tail) return;
  const int slot = cell_insert(tab, cap, c);
  if (head) tab[slot].val = k;
  if (tail) tab[slot].first = (uint32_t)(k + 1);
}

struct Ranges {     // the 27 neighbour cells' candidates: positions in `pts` and, when staged, in the LDS copy
  int gb[27], ge[27], lb[27];
};

// One query by one lane group.  Lane l of the group takes candidates l, l + 8, ... of every cell, cells in a fixed
// order: the kept set, the counts and the order of every sum do not depend on scheduling.
//   keep(d2, j) = d2 < T or (d2 == T and j <= J): T the max_nn-th smallest d2 (bits of a non-negative float order like
//   the float), J the cut among the candidates tied at T.
template <bool STAGED>
__device__ __forceinline__ void one_query(const float4 *__restrict__ pts, const float4 *cand, const Ranges &R, float4 P,
                                          int n, float r2, int max_nn, bool has_vp, float vx, float vy, float vz,
                                          float *normals, int32_t *counts, int gl) {
  auto count_kept = [&](uint32_t T, int J) {
    int c = 0;
    for (int r = 0; r < 27; r++) {
      const int b = STAGED ? R.lb[r] : R.gb[r], e = b + (R.ge[r] - R.gb[r]);
      for (int t = b + gl; t < e; t += kGroup) {
        const float4 C = STAGED ? cand[t] : pts[t];
        const float dx = C.x - P.x, dy = C.y - P.y, dz = C.z - P.z;
        const uint32_t u = __float_as_uint((dx * dx + dy * dy) + dz * dz);
        c += (u < T || (u == T && __float_as_int(C.w) <= J)) ? 1 : 0;
      }
    }
#pragma unroll
    for (int o = kGroup / 2; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
    return c;
  };
  // d2 <= r2 <=> bits(d2) <= bits(r2); a NaN distance has larger bits than any finite r2 and is never kept
  uint32_t T = __float_as_uint(r2);
  int J = 0x7fffffff;
  int m = count_kept(T, J);
  if (m > max_nn) {
    uint32_t lo = 0, hi = T;          // invariant: count(d2 <= hi) = m_hi >= max_nn
    int m_hi = m;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      const int c = count_kept(mid, J);
      if (c >= max_nn) {
        hi = mid;
        m_hi = c;
      } else {
        lo = mid + 1;
      }
    }
    T = hi;
    if (m_hi > max_nn) {              // ties at T: the smallest J with count(.., J) >= max_nn, then exactly max_nn
      int jl = 0, jh = n - 1;
      while (jl < jh) {
        const int mid = jl + (jh - jl) / 2;
        if (count_kept(T, mid) >= max_nn) jh = mid;
        else jl = mid + 1;
      }
      J = jh;
    }
    m = max_nn;
  }
  float s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // sum q, sum q q^T (xx xy xz yy yz zz), q = p_j - p_i
  for (int r = 0; r < 27; r++) {
    const int b = STAGED ? R.lb[r] : R.gb[r], e = b + (R.ge[r] - R.gb[r]);
    for (int t = b + gl; t < e; t += kGroup) {
      const float4 C = STAGED ? cand[t] : pts[t];
      const float dx = C.x - P.x, dy = C.y - P.y, dz = C.z - P.z;
      const uint32_t u = __float_as_uint((dx * dx + dy * dy) + dz * dz);
      if (u < T || (u == T && __float_as_int(C.w) <= J)) {
        s[0] += dx;
        s[1] += dy;
        s[2] += dz;
        s[3] += dx * dx;
        s[4] += dx * dy;
        s[5] += dx * dz;
        s[6] += dy * dy;
        s[7] += dy * dz;
        s[8] += dz * dz;
      }
    }
  }
  double S[9];
#pragma unroll
  for (int k = 0; k < 9; k++) {
    S[k] = (double)s[k];
#pragma unroll
    for (int o = kGroup / 2; o >= 1; o >>= 1) S[k] += __shfl_xor(S[k], o, 64);
  }
  if (gl != 0) return;
  const int i = __float_as_int(P.w);
  float nx = 0.f, ny = 0.f, nz = 1.f;
  if (m >= 3) {
    const double inv = 1.0 / (double)m;
    const double mx = S[0] * inv, my = S[1] * inv, mz = S[2] * inv;
    const double c[6] = {S[3] * inv - mx * mx, S[4] * inv - mx * my, S[5] * inv - mx * mz,
                         S[6] * inv - my * my, S[7] * inv - my * mz, S[8] * inv - mz * mz};
    double v[3];
    if (smallest_eigenvector(c, v)) {
      nx = (float)v[0];
      ny = (float)v[1];
      nz = (float)v[2];
      bool flip;
      if (has_vp) {
        const double d = ((double)nx * ((double)vx - (double)P.x) + (double)ny * ((double)vy - (double)P.y)) +
                         (double)nz * ((double)vz - (double)P.z);
        flip = d < 0.0;
      } else {
        const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
        flip = (ax >= ay && ax >= az) ? nx < 0.f : (ay >= az ? ny < 0.f : nz < 0.f);
      }
      if (flip) {
        nx = -nx;
        ny = -ny;
        nz = -nz;
      }
    }
  }
  normals[(size_t)i * 3 + 0] = nx;
  normals[(size_t)i * 3 + 1] = ny;
  normals[(size_t)i * 3 + 2] = nz;
  if (counts) counts[i] = m;
}

// One workgroup per kSpan sorted queries.  The span is walked cell by cell: the 27 neighbour cells' ranges come from
// the table, their points are staged into LDS once (when they fit) and every query of the cell in the span reuses them.
__global__ __launch_bounds__(kThreads) void k_nrm_search(const float4 *__restrict__ pts, const uint64_t *__restrict__ key,
                                                         int n, const HashEntry *__restrict__ tab, int cap, float r2,
                                                         int max_nn, int has_vp, float vx, float vy, float vz,
                                                         float *normals, int32_t *counts) {
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
      if (staged)
        one_query<true>(pts, cand, R, pts[q], n, r2, max_nn, has_vp != 0, vx, vy, vz, normals, counts, gl);
      else
        one_query<false>(pts, cand, R, pts[q], n, r2, max_nn, has_vp != 0, vx, vy, vz, normals, counts, gl);
    }
    __syncthreads();
    k = e;
  }
}

int estimate(const float *xyz, int n, int stride, float radius, int max_nn, const float *vp, float *normals,
             int32_t *counts, void *scratch, size_t scratch_bytes, hipStream_t s, float *phase_ms) {
  D3D_REQUIRE(n >= 0 && n <= kMaxPoints && stride >= 3, "d3d_estimate_normals: bad point count or row stride");
  D3D_REQUIRE(radius > 0.f && radius < INFINITY && max_nn >= 3, "d3d_estimate_normals: radius <= 0 or max_nn < 3");
  if (n == 0) {
    if (phase_ms) phase_ms[0] = phase_ms[1] = phase_ms[2] = phase_ms[3] = 0.f;
    return D3D_OK;
  }
  D3D_REQUIRE(xyz && normals && scratch, "d3d_estimate_normals: null pointer");
  D3D_REQUIRE(scratch_bytes >= d3d_estimate_normals_scratch_bytes(n, max_nn), "d3d_estimate_normals: scratch too small");
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  if (phase_ms)
    for (int k = 0; k < 5; k++) D3D_HIP_CHECK(hipEventCreate(&ev[k]));
  Arena A = scratch_arena(scratch, scratch_bytes);
  CellList L;
  const int rc = celllist::build(xyz, n, stride, radius, A, s, &L, phase_ms ? ev : nullptr);
  if (rc) return rc;
  hipLaunchKernelGGL(k_nrm_search, dim3((unsigned)((n + kSpan - 1) / kSpan)), dim3(kThreads), 0, s, L.pts, L.key, n, L.tab,
                     L.cap, radius * radius, max_nn, vp ? 1 : 0, vp ? vp[0] : 0.f, vp ? vp[1] : 0.f, vp ? vp[2] : 0.f,
                     normals, counts);
  D3D_LAUNCH_CHECK();
  if (phase_ms) {
    D3D_HIP_CHECK(hipEventRecord(ev[4], s));
    D3D_HIP_CHECK(hipEventSynchronize(ev[4]));
    for (int k = 0; k < 4; k++) D3D_HIP_CHECK(hipEventElapsedTime(&phase_ms[k], ev[k], ev[k + 1]));
    for (int k = 0; k < 5; k++) (void)hipEventDestroy(ev[k]);
  }
  return D3D_OK;
}

}  // namespace

namespace celllist {

int table_cap(int n) {
  long c = 1024;
  while (c < 2l * n) c <<= 1;
  return (int)c;
}

size_t scratch_bytes(int n) {
  const size_t N = (size_t)std::max(1, std::min(n, kMaxPoints));
  // the arrays of build() (256-byte aligned each), the table and one sort's temporaries
  return 6 * (N * 4 + 256) + (N * 16 + 256) + (N * 8 + 256) + ((size_t)table_cap((int)N) * sizeof(HashEntry) + 256) +
         sort_scratch_bytes((int)N, kCellBits) + 1024;
}

int build(const float *xyz, int n, int stride, float radius, Arena &A, hipStream_t s, CellList *out, hipEvent_t *ev) {
  D3D_REQUIRE(n >= 1 && n <= kMaxPoints && stride >= 3 && xyz && out, "cell list: bad point count, row stride or pointer");
#define NRM_MARK(k) \
  if (ev) D3D_HIP_CHECK(hipEventRecord(ev[k], s))
  const int cap = table_cap(n);
  D3D_ALLOC(red, uint32_t, A, 4);
  D3D_ALLOC(cx, uint32_t, A, n);
  D3D_ALLOC(cy, uint32_t, A, n);
  D3D_ALLOC(cz, uint32_t, A, n);
  D3D_ALLOC(perm_a, int32_t, A, n);
  D3D_ALLOC(perm_b, int32_t, A, n);
  D3D_ALLOC(ktmp, uint32_t, A, n);
  D3D_ALLOC(pts, float4, A, n);
  D3D_ALLOC(key, uint64_t, A, n);
  D3D_ALLOC(tab, HashEntry, A, cap);
  const size_t mark = A.used;
  NRM_MARK(0);
  D3D_HIP_CHECK(hipMemsetAsync(red, 0xFF, 16, s));
  hipLaunchKernelGGL(k_nrm_min, dim3(std::max(1u, std::min(1024u, grid1d(n).x))), dim3(256), 0, s, xyz, n, stride, red);
  hipLaunchKernelGGL(k_nrm_cells, grid1d(n), dim3(256), 0, s, xyz, n, stride, (const uint32_t *)red,
                     (double)radius * 1.0001, cx, cy, cz, perm_a);
  D3D_LAUNCH_CHECK();
  NRM_MARK(1);
  // least significant digit first; every sort is stable, so the final order is (x, y, z, original index)
  int rc = sort_pairs_u32(cz, nullptr, perm_a, perm_b, n, kCellBits, A, s, false);
  if (rc) return rc;
  A.used = mark;
  hipLaunchKernelGGL(k_nrm_gather, grid1d(n), dim3(256), 0, s, (const uint32_t *)cy, (const int32_t *)perm_b, n, ktmp);
  rc = sort_pairs_u32(ktmp, nullptr, perm_b, perm_a, n, kCellBits, A, s, false);
  if (rc) return rc;
  A.used = mark;
  hipLaunchKernelGGL(k_nrm_gather, grid1d(n), dim3(256), 0, s, (const uint32_t *)cx, (const int32_t *)perm_a, n, ktmp);
  rc = sort_pairs_u32(ktmp, nullptr, perm_a, perm_b, n, kCellBits, A, s, false);
  if (rc) return rc;
  A.used = mark;
  hipLaunchKernelGGL(k_nrm_sorted, grid1d(n), dim3(256), 0, s, xyz, n, stride, (const int32_t *)perm_b,
                     (const uint32_t *)cx, (const uint32_t *)cy, (const uint32_t *)cz, pts, key);
  D3D_LAUNCH_CHECK();
  NRM_MARK(2);
  D3D_HIP_CHECK(hipMemsetAsync(tab, 0xFF, (size_t)cap * sizeof(HashEntry), s));
  hipLaunchKernelGGL(k_nrm_table, grid1d(n), dim3(256), 0, s, (const uint64_t *)key, n, tab, cap);
  D3D_LAUNCH_CHECK();
  NRM_MARK(3);
#undef NRM_MARK
  out->pts = pts;
  out->key = key;
  out->tab = tab;
  out->cap = cap;
  out->red = red;
  out->h = (double)radius * 1.0001;
  return D3D_OK;
}

}  // namespace celllist
}  // namespace d3d

using namespace d3d;

size_t d3d_estimate_normals_scratch_bytes(int n, int max_nn) {
  (void)max_nn;   // the cut needs no per-query storage
  if (n <= 0) return 256;
  return celllist::scratch_bytes(n);
}

int d3d_estimate_normals(const float *xyz, int n, int row_stride_floats, float radius, int max_nn,
                         const float *viewpoint_host, float *normals, int32_t *counts, void *scratch,
                         size_t scratch_bytes, void *stream) {
  return estimate(xyz, n, row_stride_floats, radius, max_nn, viewpoint_host, normals, counts, scratch, scratch_bytes,
                  (hipStream_t)stream, nullptr);
}

int d3d_estimate_normals_phases(const float *xyz, int n, int row_stride_floats, float radius, int max_nn,
                                const float *viewpoint_host, float *normals, int32_t *counts, void *scratch,
                                size_t scratch_bytes, void *stream, float *phase_ms_host) {
  D3D_REQUIRE(phase_ms_host, "d3d_estimate_normals_phases: null pointer");
  return estimate(xyz, n, row_stride_floats, radius, max_nn, viewpoint_host, normals, counts, scratch, scratch_bytes,
                  (hipStream_t)stream, phase_ms_host);
}
