// Planar patches of a cloud that carries normals, and the plane of every patch (include/d3d_hip.h).
//
// d3d_segment_planes is d3d_connected_components (clean.hip) with a narrower edge: the same cell list, the same walk
// (cell_walk.inc) and the same lock-free union-find (union_find.inc), but two points within r are joined only when their normals agree
// and each lies in the other's tangent plane.  Pairwise region growing, not RANSAC: a smoothly curved surface chains into
// one patch.  The three tests are bitwise symmetric in the two points (products commute, C - P = -(P - C) exactly,
// the absolute values are equal), so linking only towards lower sorted positions gives the components of an undirected
// graph.  Each is written as "passes if": a NaN anywhere fails it and leaves the point a singleton.
//
// The normals are gathered to the sorted positions once (float4 per position) and the query reads a candidate's normal
// from that array only after the candidate passed the position and distance tests; the walk's LDS holds the positions
// alone, as in clean.hip.
//
// d3d_fit_planes: fp64 moments about the patch's first row.  The rows of a patch are cut into chunks of kChunk; a
// workgroup takes one chunk of one patch, thread t adds rows t, t + 256, ... in that order, the block adds its lanes
// pairwise and its waves in order; one thread per patch then adds the chunks in order and solves the 3x3 (eigen3.inc).
// No float atomics: the same input gives the same bits.
#include "d3d_internal.h"

#include <algorithm>

namespace d3d {

namespace {

using namespace celllist;
#include "cell_walk.inc"
#include "union_find.inc"
#include "eigen3.inc"

constexpr int kMaxPlanes = 4096;      // box_fit.hip's kMaxBoxes: label_planes hands the patches to d3d_fit_boxes
constexpr int kChunk = 1024;          // rows of one workgroup of k_pln_moments
constexpr int kFitThreads = 256;
constexpr int kMoments = 10;          // count, sum q (3), sum q q^T (xx xy xz yy yz zz)

// the normal of every sorted position, indexed by the original row pts[k].w
__global__ void k_pln_gather(const float4 *__restrict__ pts, const float *__restrict__ normals, int n, float4 *nrm) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const float *v = normals + (size_t)__float_as_int(pts[k].w) * 3;
  nrm[k] = make_float4(v[0], v[1], v[2], 0.f);
}

// every point links to its neighbours of lower sorted position that pass all three tests, d = C - P:
//   bits((dx dx + dy dy) + dz dz) <= bits(r2);  |(nPx nCx + nPy nCy) + nPz nCz| >= cos_min;
//   |(nPx dx + nPy dy) + nPz dz| <= offset and the same with nC (for ordered values: fmax of the two <= offset;
//   two comparisons, so that a NaN on either side fails where fmax would drop it)
struct PlaneLinkQuery {
  uint32_t r2_bits;
  float cos_min, offset;
  const float4 *nrm;
  int32_t *par;
  template <bool STAGED>
  __device__ __forceinline__ void run(const float4 *__restrict__ pts, const float4 *cand, const Ranges &R, int q, float4 P,
                                      int gl) const {
    const float4 nP = nrm[q];
    for_candidates<STAGED>(pts, cand, R, gl, [&](float4 C, int pos) {
      if (!(pos < q && dist2_bits(C, P) <= r2_bits)) return;
      const float dx = C.x - P.x, dy = C.y - P.y, dz = C.z - P.z;
      const float4 nC = nrm[pos];
      const float c = (nP.x * nC.x + nP.y * nC.y) + nP.z * nC.z;
      if (!(fabsf(c) >= cos_min)) return;
      const float eP = fabsf((nP.x * dx + nP.y * dy) + nP.z * dz);
      const float eC = fabsf((nC.x * dx + nC.y * dy) + nC.z * dz);
      if (eP <= offset && eC <= offset) uf_unite(par, q, pos);
    });
  }
};

// ---- planes of the patches ----
// first chunk of every plane: cstart[g] = sum over g' < g of ceil(len(g') / kChunk), cstart[k] the total; one block,
// thread t takes planes 4 t .. 4 t + 3.  [lo, hi) of plane g is its offsets clamped into [0, n] and made ordered.
__device__ __forceinline__ int2 plane_rows(const int32_t *__restrict__ offsets, int g, int n) {
  const int lo = max(0, min(offsets[g], n));
  return make_int2(lo, max(lo, min(offsets[g + 1], n)));
}

__global__ __launch_bounds__(1024) void k_pln_chunks(const int32_t *__restrict__ offsets, int k, int n, int32_t *cstart) {
  __shared__ int s[1024];
  const int t = threadIdx.x;
  int c[kMaxPlanes / 1024], tot = 0;
#pragma unroll
  for (int j = 0; j < kMaxPlanes / 1024; j++) {
    const int g = t * (kMaxPlanes / 1024) + j;
    c[j] = 0;
    if (g < k) {
      const int2 r = plane_rows(offsets, g, n);
      c[j] = (r.y - r.x + kChunk - 1) / kChunk;
    }
    tot += c[j];
  }
  s[t] = tot;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {        // inclusive scan of the threads' totals
    const int v = t >= d ? s[t - d] : 0;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  int run = s[t] - tot;
#pragma unroll
  for (int j = 0; j < kMaxPlanes / 1024; j++) {
    const int g = t * (kMaxPlanes / 1024) + j;
    if (g < k) cstart[g] = run;
    run += c[j];
  }
  if (t == 1023) cstart[k] = s[t];
}

// block b: the plane g with cstart[g] <= b < cstart[g + 1] and its chunk b - cstart[g] -> part[b][kMoments]
__global__ __launch_bounds__(kFitThreads) void k_pln_moments(const float *__restrict__ xyz, int n, int stride,
                                                               const int32_t *__restrict__ plane_of_point,
                                                               const int32_t *__restrict__ order,
                                                               const int32_t *__restrict__ offsets, int k,
                                                               const int32_t *__restrict__ cstart, double *part) {
  __shared__ double lds[kFitThreads / 64][kMoments];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= cstart[k]) return;                 // uniform over the block
  int lo = 0, hi = k - 1;                     // the last g with cstart[g] <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (cstart[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  const int g = lo;
  const int2 rows = plane_rows(offsets, g, n);
  const int first = order[rows.x];
  double o[3] = {0.0, 0.0, 0.0};
  if ((unsigned)first < (unsigned)n)
    for (int d = 0; d < 3; d++) o[d] = (double)xyz[(size_t)first * stride + d];
  const int begin = rows.x + (b - cstart[g]) * kChunk, end = min(rows.y, begin + kChunk);
  double s[kMoments] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int p = begin + tid; p < end; p += kFitThreads) {
    const int row = order[p];
    if ((unsigned)row >= (unsigned)n || plane_of_point[row] != g) continue;      // not a row of this plane: skipped
    const float *v = xyz + (size_t)row * stride;
    const double x = (double)v[0] - o[0], y = (double)v[1] - o[1], z = (double)v[2] - o[2];
    s[0] += 1.0;
    s[1] += x;
    s[2] += y;
    s[3] += z;
    s[4] += x * x;
    s[5] += x * y;
    s[6] += x * z;
    s[7] += y * y;
    s[8] += y * z;
    s[9] += z * z;
  }
#pragma unroll
  for (int j = 0; j < kMoments; j++) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s[j] += __shfl_xor(s[j], d, 64);
    if ((tid & 63) == 0) lds[tid >> 6][j] = s[j];
  }
  __syncthreads();
  if (tid < kMoments) {
    double t = 0.0;
    for (int w = 0; w < kFitThreads / 64; w++) t += lds[w][tid];
    part[(size_t)b * kMoments + tid] = t;
  }
}

// one thread per plane: its chunks in order, the centroid, the covariance and its eigen-decomposition
__global__ __launch_bounds__(64) void k_pln_solve(const float *__restrict__ xyz, int n, int stride,
                                                   const int32_t *__restrict__ order, const int32_t *__restrict__ offsets,
                                                   int k, const int32_t *__restrict__ cstart, int nchunks,
                                                   const double *__restrict__ part, double *normal, double *dist,
                                                   double *centroid, int32_t *count, double *rms, double *eig) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= k) return;
  double s[kMoments] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int c0 = min(cstart[g], nchunks), c1 = min(cstart[g + 1], nchunks);
  for (int c = c0; c < c1; c++)
    for (int j = 0; j < kMoments; j++) s[j] += part[(size_t)c * kMoments + j];
  double nv[3] = {0.0, 0.0, 0.0}, ce[3] = {0.0, 0.0, 0.0}, ev[3] = {0.0, 0.0, 0.0}, dd = 0.0, rr = 0.0;
  const double m = s[0];
  if (m > 0.0) {
    const int2 rows = plane_rows(offsets, g, n);
    const int first = order[rows.x];
    double o[3] = {0.0, 0.0, 0.0};
    if ((unsigned)first < (unsigned)n)
      for (int d = 0; d < 3; d++) o[d] = (double)xyz[(size_t)first * stride + d];
    const double mx = s[1] / m, my = s[2] / m, mz = s[3] / m;
    ce[0] = o[0] + mx, ce[1] = o[1] + my, ce[2] = o[2] + mz;
    const double C[6] = {s[4] / m - mx * mx, s[5] / m - mx * my, s[6] / m - mx * mz,
                         s[7] / m - my * my, s[8] / m - my * mz, s[9] / m - mz * mz};
    double v[3];
    if (smallest_eigenvector(C, v)) {
      const double ax = fabs(v[0]), ay = fabs(v[1]), az = fabs(v[2]);
      const bool flip = (ax >= ay && ax >= az) ? v[0] < 0.0 : (ay >= az ? v[1] < 0.0 : v[2] < 0.0);
      for (int d = 0; d < 3; d++) nv[d] = flip ? -v[d] : v[d];
      dd = (nv[0] * ce[0] + nv[1] * ce[1]) + nv[2] * ce[2];
      // eigenvalues: the Rayleigh quotient of v, and the 2x2 of C on the plane across v (u from the axis v leans on
      // least, w = v x u)
      const int a = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);
      double u[3] = {-v[a] * v[0], -v[a] * v[1], -v[a] * v[2]};
      u[a] += 1.0;
      const double ul = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
      for (int d = 0; d < 3; d++) u[d] /= ul;
      const double w[3] = {v[1] * u[2] - v[2] * u[1], v[2] * u[0] - v[0] * u[2], v[0] * u[1] - v[1] * u[0]};
      auto form = [&](const double *p, const double *q) {
        const double cq0 = (C[0] * q[0] + C[1] * q[1]) + C[2] * q[2];
        const double cq1 = (C[1] * q[0] + C[3] * q[1]) + C[4] * q[2];
        const double cq2 = (C[2] * q[0] + C[4] * q[1]) + C[5] * q[2];
        return (p[0] * cq0 + p[1] * cq1) + p[2] * cq2;
      };
      const double l0 = form(v, v), buu = form(u, u), buw = form(u, w), bww = form(w, w);
      const double half = 0.5 * (buu - bww), mid = 0.5 * (buu + bww), root = sqrt(half * half + buw * buw);
      double e0 = l0, e1 = mid - root, e2 = mid + root;
      if (e1 < e0) {
        const double t = e0;
        e0 = e1, e1 = t;
      }
      ev[0] = e0, ev[1] = e1, ev[2] = e2;
      rr = sqrt(fmax(e0, 0.0));
    }
  }
  for (int d = 0; d < 3; d++) {
    normal[(size_t)g * 3 + d] = nv[d];
    centroid[(size_t)g * 3 + d] = ce[d];
    eig[(size_t)g * 3 + d] = ev[d];
  }
  dist[g] = dd;
  rms[g] = rr;
  count[g] = (int32_t)m;
}

int fit_chunks(int n, int k) { return (int)(((long)std::max(n, 0) + kChunk - 1) / kChunk) + std::max(k, 0); }

size_t fit_scratch_bytes(int n, int k) {
  return (size_t)fit_chunks(n, k) * kMoments * sizeof(double) + 256 + ((size_t)std::max(k, 0) + 1) * sizeof(int32_t) + 256;
}

}  // namespace
}  // namespace d3d

using namespace d3d;

size_t d3d_segment_planes_scratch_bytes(int n) {
  if (n <= 0) return 256;
  const size_t N = (size_t)std::min(n, celllist::kMaxPoints);
  return celllist::scratch_bytes((int)N) + 4 * (N * 4 + 256) + (N * 16 + 256);
}

int d3d_segment_planes(const float *xyz, int n, int row_stride_floats, const float *normals, float radius, float cos_min,
                       float offset, int32_t *label, int32_t *size, void *scratch, size_t scratch_bytes, void *stream,
                       float *phase_ms_host) {
  D3D_REQUIRE(args_ok(n, row_stride_floats, radius), "d3d_segment_planes: bad point count, row stride or radius");
  D3D_REQUIRE(cos_min >= 0.f && cos_min <= 1.f, "d3d_segment_planes: cos_min %g outside [0, 1]", (double)cos_min);
  D3D_REQUIRE(offset >= 0.f && offset < INFINITY, "d3d_segment_planes: offset %g negative or not finite", (double)offset);
  if (n == 0) {
    zero_phases(phase_ms_host);
    return D3D_OK;
  }
  D3D_REQUIRE(xyz && normals && label && size && scratch, "d3d_segment_planes: null pointer");
  D3D_REQUIRE(scratch_bytes >= d3d_segment_planes_scratch_bytes(n), "d3d_segment_planes: scratch too small");
  hipStream_t s = (hipStream_t)stream;
  Timer T;
  CLN_TRY(T.start(phase_ms_host != nullptr, kPhases + 1));
  Arena A = scratch_arena(scratch, scratch_bytes);
  D3D_ALLOC(par, int32_t, A, n);
  D3D_ALLOC(root, int32_t, A, n);
  D3D_ALLOC(min_index, int32_t, A, n);
  D3D_ALLOC(csize, int32_t, A, n);
  D3D_ALLOC(nrm, float4, A, n);
  celllist::CellList L;
  CLN_TRY(celllist::build(xyz, n, row_stride_floats, radius, A, s, &L, T.events()));
  hipLaunchKernelGGL(k_pln_gather, grid1d(n), dim3(256), 0, s, L.pts, normals, n, nrm);
  hipLaunchKernelGGL(k_cln_iota, grid1d(n), dim3(256), 0, s, par, n);
  D3D_HIP_CHECK(hipMemsetAsync(min_index, 0x7F, (size_t)n * 4, s));      // above every index
  D3D_HIP_CHECK(hipMemsetAsync(csize, 0, (size_t)n * 4, s));
  CLN_TRY(launch_walk(L, n, PlaneLinkQuery{r2_bits(radius), cos_min, offset, (const float4 *)nrm, par}, s));
  CLN_TRY(T.mark(4, s));
  hipLaunchKernelGGL(k_cln_roots, grid1d(n), dim3(256), 0, s, (const int32_t *)par, L.pts, n, root, min_index, csize);
  hipLaunchKernelGGL(k_cln_labels, grid1d(n), dim3(256), 0, s, (const int32_t *)root, L.pts, n, (const int32_t *)min_index,
                     (const int32_t *)csize, label, size);
  D3D_LAUNCH_CHECK();
  CLN_TRY(T.mark(5, s));
  return T.finish(phase_ms_host);
}

size_t d3d_fit_planes_scratch_bytes(int n, int k) {
  return n < 0 || n > celllist::kMaxPoints || k < 0 || k > kMaxPlanes ? 0 : fit_scratch_bytes(n, k);
}

int d3d_fit_planes(const float *xyz, int n, int row_stride_floats, const int32_t *plane_of_point, const int32_t *order,
                   const int32_t *offsets, int k, double *normal, double *d, double *centroid, int32_t *count, double *rms,
                   double *eigenvalues, void *scratch, size_t scratch_bytes, void *stream, float *phase_ms_host) {
  D3D_REQUIRE(n >= 0 && n <= celllist::kMaxPoints && k >= 0, "d3d_fit_planes: n %d, k %d out of range", n, k);
  D3D_REQUIRE(k <= kMaxPlanes, "d3d_fit_planes: %d planes, at most %d", k, kMaxPlanes);
  if (phase_ms_host) phase_ms_host[0] = phase_ms_host[1] = 0.f;
  if (k == 0) return D3D_OK;
  D3D_REQUIRE(row_stride_floats >= 3, "d3d_fit_planes: row stride %d < 3 floats", row_stride_floats);
  D3D_REQUIRE(n == 0 || (xyz && plane_of_point && order), "d3d_fit_planes: null pointer (xyz, plane_of_point, order)");
  D3D_REQUIRE(offsets && normal && d && centroid && count && rms && eigenvalues, "d3d_fit_planes: null pointer");
  D3D_REQUIRE(scratch && scratch_bytes >= fit_scratch_bytes(n, k), "d3d_fit_planes: scratch of %zu bytes, need %zu",
              scratch_bytes, fit_scratch_bytes(n, k));
  hipStream_t s = (hipStream_t)stream;
  Arena A = scratch_arena(scratch, scratch_bytes);
  const int nchunks = fit_chunks(n, k);
  D3D_ALLOC(part, double, A, (size_t)nchunks * kMoments);
  D3D_ALLOC(cstart, int32_t, A, k + 1);
  Timer T;                            // moments, solve
  CLN_TRY(T.start(phase_ms_host != nullptr, 3));
  CLN_TRY(T.mark(0, s));
  hipLaunchKernelGGL(k_pln_chunks, dim3(1), dim3(1024), 0, s, offsets, k, n, cstart);
  hipLaunchKernelGGL(k_pln_moments, dim3((unsigned)nchunks), dim3(kFitThreads), 0, s, xyz, n, row_stride_floats,
                     plane_of_point, order, offsets, k, (const int32_t *)cstart, part);
  CLN_TRY(T.mark(1, s));
  hipLaunchKernelGGL(k_pln_solve, grid1d(k, 64), dim3(64), 0, s, xyz, n, row_stride_floats, order, offsets, k,
                     (const int32_t *)cstart, nchunks, (const double *)part, normal, d, centroid, count, rms, eigenvalues);
  D3D_LAUNCH_CHECK();
  CLN_TRY(T.mark(2, s));
  return T.finish(phase_ms_host);
}
