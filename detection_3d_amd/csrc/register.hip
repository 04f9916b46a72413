// Aligning overlapping scans: the nearest point of one cloud for every point of another, and ICP as a loop around it
// (what the reference's users do with open3d's compute_point_cloud_distance and registration_icp on the CPU;
// restatements that are not pinned against open3d itself).
//
// k_reg_nearest queries a cloud's cell list (celllist::build, celllist.hip) by the points of ANOTHER cloud, in the
// queries' own order: the query's cell is floor((q - min) / h) per axis in fp64, the build's arithmetic, clamped to
// [-1, kCellMax]; the 27 cells around it hold every cloud point within the radius.  Distances are dist2_bits':
// d2 = (dx dx + dy dy) + dz dz in fp32 from the fp32 offset C - Q, compared as unsigned integers; the minimum is taken
// over (bits of d2, original row), so a tie goes to the lowest row and the order of the candidates does not show.
//
// ICP: per step k_reg_transform (the queries fp32(R p + t)), k_reg_nearest, k_reg_accumulate (29 fp64 sums of the
// normal equations per block of kAccRows rows: thread order, lanes pairwise, waves in order) and k_reg_solve (the
// partials in block order, a 6 x 6 Cholesky solve, the pose update, the step's record).  Nothing is read back between
// the steps: once the status word is non-zero the remaining steps' kernels return at once.  No float atomics.
#include "d3d_internal.h"

#include <algorithm>

namespace d3d {

namespace {

using namespace celllist;
#include "cell_walk.inc"

constexpr int kQSpan = 64;                        // query rows per workgroup of k_reg_nearest: 4 per lane group
constexpr int kAccThreads = 256;
constexpr int kAccRows = 4096;                    // source rows per workgroup of k_reg_accumulate
constexpr int kSys = 29;                          // A (21, upper triangle by rows), b (6), e, c
constexpr int kHistory = 20;                      // pose (16), c, e, |w|, |v|
constexpr int kIcpPhases = 7;                     // cells, sort, table, transform, nearest, accumulate, solve
constexpr int kMaxIterations = 10000;

// the build's cell coordinate of a foreign point, clamped to [-1, kCellMax]; anything unordered -> -1
__device__ __forceinline__ int query_cell(float q, float lo, double h) {
  const double c = floor(((double)q - (double)lo) / h);
  return c >= 0.0 ? (c < (double)kCellMax ? (int)c : kCellMax) : -1;
}

__global__ void k_reg_fill(int m, int32_t *index, float *dist2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  index[i] = -1;
  if (dist2) dist2[i] = INFINITY;
}

// index[q] = the original row of the cloud point nearest to query q by (bits of d2, row) among those with d2 <= r2, or
// -1; dist2[q] = that d2, or +inf.  One lane group per query, kQSpan consecutive queries per workgroup.  Every lane
// stays in the loops (a dead query has empty ranges), so that the group's shuffles always find their partners.
// state: null, or the ICP's (steps, status): a non-zero status ends the launch at once.
__global__ __launch_bounds__(kThreads) void k_reg_nearest(const float4 *__restrict__ pts, int n,
                                                          const HashEntry *__restrict__ tab, int cap,
                                                          const uint32_t *__restrict__ red, double h,
                                                          const float *__restrict__ query, int m, int qstride,
                                                          uint32_t r2b, int32_t *index, float *dist2,
                                                          const int32_t *__restrict__ state) {
  if (state && state[1] != 0) return;
  const int tid = threadIdx.x, grp = tid / kGroup, gl = tid % kGroup;
  const float lo0 = ordered_to_f32(red[0]), lo1 = ordered_to_f32(red[1]), lo2 = ordered_to_f32(red[2]);
  const long base = (long)blockIdx.x * kQSpan;
  for (int it = 0; it < kQSpan / kGroups; it++) {
    const long q = base + it * kGroups + grp;
    const bool live = q < m;
    float4 Q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
      const float *p = query + (size_t)q * qstride;
      Q = make_float4(p[0], p[1], p[2], 0.f);
    }
    const bool ok = live && isfinite(Q.x) && isfinite(Q.y) && isfinite(Q.z);
    const int c0 = query_cell(Q.x, lo0, h), c1 = query_cell(Q.y, lo1, h), c2 = query_cell(Q.z, lo2, h);
    int cb[4], ce[4];                 // the ranges of this lane's cells gl, gl + 8, gl + 16, gl + 24 (cells 27.. : empty)
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const int r = gl + kGroup * s;
      int2 g = make_int2(0, 0);
      if (ok && r < 27) {
        const int cx = c0 + r / 9 - 1, cy = c1 + (r / 3) % 3 - 1, cz = c2 + r % 3 - 1;
        if (cx >= 0 && cx <= kCellMax && cy >= 0 && cy <= kCellMax && cz >= 0 && cz <= kCellMax)
          g = cell_range(tab, cap, cell_key((uint32_t)cx, (uint32_t)cy, (uint32_t)cz));
      }
      g.x = max(0, min(g.x, n));      // whatever the table holds, no range leaves the sorted points
      g.y = max(g.x, min(g.y, n));
      cb[s] = g.x;
      ce[s] = g.y;
    }
    uint32_t bb = 0xFFFFFFFFu, bi = 0xFFFFFFFFu;     // best (bits of d2, row) of this lane: none yet
#pragma unroll
    for (int s = 0; s < 4; s++) {
#pragma unroll 1
      for (int o = 0; o < kGroup; o++) {
        const int b = __shfl(cb[s], o, kGroup), e = __shfl(ce[s], o, kGroup);
        for (int t = b + gl; t < e; t += kGroup) {
          const float4 C = pts[t];
          const uint32_t u = dist2_bits(C, Q), j = __float_as_uint(C.w);
          // a NaN distance has larger bits than any finite r2 and never competes
          if (u <= r2b && (u < bb || (u == bb && j < bi))) {
            bb = u;
            bi = j;
          }
        }
      }
    }
#pragma unroll
    for (int o = kGroup / 2; o >= 1; o >>= 1) {      // min over (bits, row): the order of the lanes does not show
      const uint32_t ob = __shfl_xor(bb, o, 64), oi = __shfl_xor(bi, o, 64);
      if (ob < bb || (ob == bb && oi < bi)) {
        bb = ob;
        bi = oi;
      }
    }
    if (gl == 0 && live) {
      const bool found = bi != 0xFFFFFFFFu;
      index[q] = found ? (int32_t)bi : -1;
      if (dist2) dist2[q] = found ? __uint_as_float(bb) : INFINITY;
    }
  }
}

// p' = R p + t in fp64 from the fp32 row widened, T the first three rows of the row-major 4 x 4 pose
__device__ __forceinline__ void moved(const double *T, const float *p, double *o) {
  const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
#pragma unroll
  for (int k = 0; k < 3; k++) o[k] = ((T[4 * k] * x + T[4 * k + 1] * y) + T[4 * k + 2] * z) + T[4 * k + 3];
}

// the step's queries: fp32(p'), rounded to nearest, rows of 3 floats
__global__ void k_reg_transform(const float *__restrict__ src, int m, int sstride, const double *__restrict__ pose,
                                const int32_t *__restrict__ state, float *query) {
  if (state[1] != 0) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  double T[12], o[3];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = pose[k];
  moved(T, src + (size_t)i * sstride, o);
  query[(size_t)i * 3 + 0] = (float)o[0];
  query[(size_t)i * 3 + 1] = (float)o[1];
  query[(size_t)i * 3 + 2] = (float)o[2];
}

// acc += (J^T J, J^T r, r r) of one residual with the Jacobian row J
__device__ __forceinline__ void add_row(double (&acc)[kSys], const double (&J)[6], double r) {
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int b = a; b < 6; b++) acc[k++] += J[a] * J[b];
#pragma unroll
  for (int a = 0; a < 6; a++) acc[21 + a] += J[a] * r;
  acc[27] += r * r;
}

// One partial record per block of kAccRows source rows: thread t adds rows t, t + 256, ... of the block in that order,
// the lanes are added pairwise, the waves in order.  METHOD 0: point to plane, r = (p' - q) . n, J = (p' x n, n); a
// target normal that is not finite or is zero contributes nothing.  METHOD 1: point to point, the three residuals
// p' - q with the rows (-[p']x, I).
template <int METHOD>
__global__ __launch_bounds__(kAccThreads) void k_reg_accumulate(const float *__restrict__ src, int m, int sstride,
                                                                const float *__restrict__ target, int n, int tstride,
                                                                const float *__restrict__ normals, int nstride,
                                                                const double *__restrict__ pose,
                                                                const int32_t *__restrict__ index,
                                                                const int32_t *__restrict__ state, double *part) {
  if (state[1] != 0) return;
  __shared__ double lds[kAccThreads / 64][kSys];
  double T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = pose[k];
  double acc[kSys];
#pragma unroll
  for (int k = 0; k < kSys; k++) acc[k] = 0.0;
  const long base = (long)blockIdx.x * kAccRows;
#pragma unroll 1
  for (int j = 0; j < kAccRows / kAccThreads; j++) {
    const long i = base + j * kAccThreads + threadIdx.x;
    if (i >= m) continue;
    const int t = index[i];
    if (t < 0 || t >= n) continue;
    double p[3];
    moved(T, src + (size_t)i * sstride, p);
    const float *qf = target + (size_t)t * tstride;
    const double d0 = p[0] - (double)qf[0], d1 = p[1] - (double)qf[1], d2 = p[2] - (double)qf[2];
    if (METHOD == 0) {
      const float *nf = normals + (size_t)t * nstride;
      const float f0 = nf[0], f1 = nf[1], f2 = nf[2];
      if (!(isfinite(f0) && isfinite(f1) && isfinite(f2)) || (f0 == 0.f && f1 == 0.f && f2 == 0.f)) continue;
      const double n0 = (double)f0, n1 = (double)f1, n2 = (double)f2;
      const double r = (d0 * n0 + d1 * n1) + d2 * n2;
      const double J[6] = {p[1] * n2 - p[2] * n1, p[2] * n0 - p[0] * n2, p[0] * n1 - p[1] * n0, n0, n1, n2};
      add_row(acc, J, r);
    } else {
      const double J0[6] = {0.0, p[2], -p[1], 1.0, 0.0, 0.0};
      const double J1[6] = {-p[2], 0.0, p[0], 0.0, 1.0, 0.0};
      const double J2[6] = {p[1], -p[0], 0.0, 0.0, 0.0, 1.0};
      add_row(acc, J0, d0);
      add_row(acc, J1, d1);
      add_row(acc, J2, d2);
    }
    acc[28] += 1.0;
  }
#pragma unroll
  for (int k = 0; k < kSys; k++) {
    double v = acc[k];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kSys) {
    double s = lds[0][threadIdx.x];
    for (int w = 1; w < kAccThreads / 64; w++) s += lds[w][threadIdx.x];
    part[(size_t)blockIdx.x * kSys + threadIdx.x] = s;
  }
}

// One workgroup: the partials in block order, then thread 0 solves A x = -b by Cholesky, x = (w, v), and updates the
// pose: dR = Rodrigues(w), R <- dR R, t <- dR t + v.  Degenerate (c < 6, or a pivot <= 1e-12 of A's largest diagonal
// entry): the pose stays and status = 2.  |w| <= tol and |v| <= tol: status = 1.  The step's record goes to row
// state[0] of history: the pose after the step, c, e, |w|, |v| (0, 0 for a degenerate step).
__global__ __launch_bounds__(64) void k_reg_solve(const double *__restrict__ part, int nb, double tol, int max_steps,
                                                  double *pose, double *history, int32_t *state, double *last_system) {
  __shared__ double S[kSys];
  const int status = state[1], step = state[0];
  if (status != 0) return;            // uniform: every thread has read the word before thread 0 writes it below
  if (threadIdx.x < kSys) {
    double s = 0.0;
    for (int b = 0; b < nb; b++) s += part[(size_t)b * kSys + threadIdx.x];
    S[threadIdx.x] = s;
    if (last_system) last_system[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double A[6][6], g[6], L[6][6], y[6], x[6];
  int k = 0;
  for (int a = 0; a < 6; a++)
    for (int b = a; b < 6; b++) {
      A[a][b] = S[k];
      A[b][a] = S[k++];
    }
  for (int a = 0; a < 6; a++) g[a] = S[21 + a];
  const double e = S[27], c = S[28];
  double top = A[0][0];
  for (int a = 1; a < 6; a++) top = fmax(top, A[a][a]);
  bool degenerate = !(c >= 6.0);
  for (int a = 0; a < 6; a++)
    for (int b = 0; b < 6; b++) L[a][b] = 0.0;
  for (int a = 0; a < 6 && !degenerate; a++) {
    double d = A[a][a];
    for (int j = 0; j < a; j++) d -= L[a][j] * L[a][j];
    if (!(d > 1e-12 * top)) {         // also a NaN
      degenerate = true;
      break;
    }
    L[a][a] = sqrt(d);
    for (int i = a + 1; i < 6; i++) {
      double s = A[i][a];
      for (int j = 0; j < a; j++) s -= L[i][j] * L[a][j];
      L[i][a] = s / L[a][a];
    }
  }
  double wn = 0.0, vn = 0.0;
  bool converged = false;
  if (!degenerate) {
    for (int i = 0; i < 6; i++) {
      double s = -g[i];
      for (int j = 0; j < i; j++) s -= L[i][j] * y[j];
      y[i] = s / L[i][i];
    }
    for (int i = 5; i >= 0; i--) {
      double s = y[i];
      for (int j = i + 1; j < 6; j++) s -= L[j][i] * x[j];
      x[i] = s / L[i][i];
    }
    const double th2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
    wn = sqrt(th2);
    vn = sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]);
    if (isfinite(wn) && isfinite(vn)) {
      double ca, cb;                  // dR = I + ca K + cb K K, K = [w]x
      if (th2 < 1e-16) {
        ca = 1.0 - th2 / 6.0;
        cb = 0.5 - th2 / 24.0;
      } else {
        const double sh = sin(0.5 * wn);
        ca = sin(wn) / wn;
        cb = 2.0 * sh * sh / th2;
      }
      const double K[3][3] = {{0.0, -x[2], x[1]}, {x[2], 0.0, -x[0]}, {-x[1], x[0], 0.0}};
      double dR[3][3], P[3][4];
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
          dR[i][j] = ((i == j ? 1.0 : 0.0) + ca * K[i][j]) + cb * (x[i] * x[j] - (i == j ? th2 : 0.0));
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++)
          P[i][j] = ((dR[i][0] * pose[j] + dR[i][1] * pose[4 + j]) + dR[i][2] * pose[8 + j]) + (j == 3 ? x[3 + i] : 0.0);
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) pose[4 * i + j] = P[i][j];
      converged = wn <= tol && vn <= tol;
    } else {                          // a solution that is not finite: as a vanished pivot
      degenerate = true;
      wn = vn = 0.0;
    }
  }
  if (step < max_steps) {
    double *row = history + (size_t)step * kHistory;
    for (int j = 0; j < 16; j++) row[j] = pose[j];
    row[16] = c;
    row[17] = e;
    row[18] = wn;
    row[19] = vn;
  }
  state[0] = step + 1;
  state[1] = degenerate ? 2 : (converged ? 1 : 0);
}

int acc_blocks(int m) { return (int)(((long)std::max(m, 1) + kAccRows - 1) / kAccRows); }

int launch_nearest(const CellList &L, int n, const float *query, int m, int qstride, float radius, int32_t *index,
                   float *dist2, const int32_t *state, hipStream_t s) {
  hipLaunchKernelGGL(k_reg_nearest, dim3((unsigned)(((long)m + kQSpan - 1) / kQSpan)), dim3(kThreads), 0, s, L.pts, n, L.tab,
                     L.cap, L.red, L.h, query, m, qstride, r2_bits(radius), index, dist2, state);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

}  // namespace
}  // namespace d3d

using namespace d3d;

size_t d3d_nearest_scratch_bytes(int n_cloud, int n_query) {
  (void)n_query;                      // a query needs no storage of its own
  if (n_cloud <= 0) return 256;
  return celllist::scratch_bytes(n_cloud);
}

int d3d_nearest(const float *cloud, int n, int row_stride_floats, const float *query, int m, int query_stride_floats,
                float radius, int32_t *index, float *dist2, void *scratch, size_t scratch_bytes, void *stream,
                float *phase_ms_host) {
  D3D_REQUIRE(args_ok(n, row_stride_floats, radius), "d3d_nearest: bad point count, row stride or radius");
  D3D_REQUIRE(m >= 0 && m <= celllist::kMaxPoints && query_stride_floats >= 3, "d3d_nearest: bad query count or row stride");
  hipStream_t s = (hipStream_t)stream;
  if (m == 0) {
    zero_phases(phase_ms_host);
    return D3D_OK;
  }
  D3D_REQUIRE(query && index, "d3d_nearest: null pointer");
  if (n == 0) {                       // nothing to find, and no table to read
    hipLaunchKernelGGL(k_reg_fill, grid1d(m), dim3(256), 0, s, m, index, dist2);
    D3D_LAUNCH_CHECK();
    zero_phases(phase_ms_host);
    return D3D_OK;
  }
  D3D_REQUIRE(cloud && scratch, "d3d_nearest: null pointer");
  D3D_REQUIRE(scratch_bytes >= d3d_nearest_scratch_bytes(n, m), "d3d_nearest: scratch too small");
  Timer T;
  CLN_TRY(T.start(phase_ms_host != nullptr, kPhases + 1));
  Arena A = scratch_arena(scratch, scratch_bytes);
  celllist::CellList L;
  CLN_TRY(celllist::build(cloud, n, row_stride_floats, radius, A, s, &L, T.events()));
  CLN_TRY(launch_nearest(L, n, query, m, query_stride_floats, radius, index, dist2, nullptr, s));
  CLN_TRY(T.mark(4, s));
  CLN_TRY(T.mark(5, s));
  return T.finish(phase_ms_host);
}

size_t d3d_icp_scratch_bytes(int n_target, int n_source) {
  const size_t N = (size_t)std::max(1, std::min(n_target, celllist::kMaxPoints));
  const size_t M = (size_t)std::max(1, std::min(n_source, celllist::kMaxPoints));
  return celllist::scratch_bytes((int)N) + (M * 12 + 256) + (M * 4 + 256) + ((size_t)acc_blocks((int)M) * kSys * 8 + 256) + 1024;
}

int d3d_icp(const float *source, int m, int source_stride_floats, const float *target, int n, int target_stride_floats,
            const float *target_normals, int normal_stride_floats, float max_dist, int method, int iterations, double tol,
            double *pose_inout_dev, double *history_dev, int32_t *state_dev, int32_t *last_index, double *last_system,
            void *scratch, size_t scratch_bytes, void *stream, float *phase_ms_host) {
  D3D_REQUIRE(args_ok(n, target_stride_floats, max_dist), "d3d_icp: bad target count, row stride or max_dist");
  D3D_REQUIRE(m >= 0 && m <= celllist::kMaxPoints && source_stride_floats >= 3, "d3d_icp: bad source count or row stride");
  D3D_REQUIRE(method == 0 || method == 1, "d3d_icp: method is 0 (point to plane) or 1 (point to point)");
  D3D_REQUIRE(iterations >= 0 && iterations <= kMaxIterations, "d3d_icp: iterations outside [0, 10000]");
  D3D_REQUIRE(tol >= 0.0 && tol < (double)INFINITY, "d3d_icp: tol is negative or not finite");
  D3D_REQUIRE(pose_inout_dev && state_dev && scratch, "d3d_icp: null pointer");
  D3D_REQUIRE(iterations == 0 || history_dev, "d3d_icp: null pointer");
  D3D_REQUIRE(m == 0 || source, "d3d_icp: null pointer");
  D3D_REQUIRE(n == 0 || target, "d3d_icp: null pointer");
  D3D_REQUIRE(method != 0 || n == 0 || (target_normals && normal_stride_floats >= 3), "d3d_icp: point to plane needs the target's normals");
  D3D_REQUIRE(scratch_bytes >= d3d_icp_scratch_bytes(n, m), "d3d_icp: scratch too small");
  hipStream_t s = (hipStream_t)stream;
  Timer T;                            // timed: 4 events around the build, then one behind every kernel of every step
  CLN_TRY(T.start(phase_ms_host != nullptr, 4 + 4 * (size_t)iterations));
  Arena A = scratch_arena(scratch, scratch_bytes);
  const int nb = acc_blocks(m);
  D3D_ALLOC(qbuf, float, A, (size_t)std::max(m, 1) * 3);
  D3D_ALLOC(own_index, int32_t, A, std::max(m, 1));
  D3D_ALLOC(part, double, A, (size_t)nb * kSys);
  int32_t *index = last_index ? last_index : own_index;
  D3D_HIP_CHECK(hipMemsetAsync(state_dev, 0, 2 * sizeof(int32_t), s));
  celllist::CellList L;
  if (n > 0) {
    CLN_TRY(celllist::build(target, n, target_stride_floats, max_dist, A, s, &L, T.events()));
  } else {
    for (int k = 0; k < 4; k++) CLN_TRY(T.mark(k, s));
    if (m > 0) hipLaunchKernelGGL(k_reg_fill, grid1d(m), dim3(256), 0, s, m, index, (float *)nullptr);
    D3D_LAUNCH_CHECK();
  }
  for (int it = 0; it < iterations; it++) {
    const size_t e = 4 + 4 * (size_t)it;
    if (n > 0 && m > 0) {
      hipLaunchKernelGGL(k_reg_transform, grid1d(m), dim3(256), 0, s, source, m, source_stride_floats,
                         (const double *)pose_inout_dev, (const int32_t *)state_dev, qbuf);
      D3D_LAUNCH_CHECK();
    }
    CLN_TRY(T.mark(e, s));
    if (n > 0 && m > 0) CLN_TRY(launch_nearest(L, n, qbuf, m, 3, max_dist, index, nullptr, state_dev, s));
    CLN_TRY(T.mark(e + 1, s));
    if (method == 0)
      hipLaunchKernelGGL(k_reg_accumulate<0>, dim3((unsigned)nb), dim3(kAccThreads), 0, s, source, m, source_stride_floats,
                         target, n, target_stride_floats, target_normals, normal_stride_floats,
                         (const double *)pose_inout_dev, (const int32_t *)index, (const int32_t *)state_dev, part);
    else
      hipLaunchKernelGGL(k_reg_accumulate<1>, dim3((unsigned)nb), dim3(kAccThreads), 0, s, source, m, source_stride_floats,
                         target, n, target_stride_floats, target_normals, normal_stride_floats,
                         (const double *)pose_inout_dev, (const int32_t *)index, (const int32_t *)state_dev, part);
    D3D_LAUNCH_CHECK();
    CLN_TRY(T.mark(e + 2, s));
    hipLaunchKernelGGL(k_reg_solve, dim3(1), dim3(64), 0, s, (const double *)part, nb, tol, iterations, pose_inout_dev,
                       history_dev, state_dev, last_system);
    D3D_LAUNCH_CHECK();
    CLN_TRY(T.mark(e + 3, s));
  }
  for (int k = 0; T.on && k < kIcpPhases; k++) phase_ms_host[k] = 0.f;
  // the build's three phases, then the four kernels of a step summed over the steps
  return T.finish(phase_ms_host, [](size_t k) { return k < 3 ? k : 3 + (k - 3) % 4; });
}
