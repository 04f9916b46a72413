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
// The cell list is celllist.hip's, the walk and the nearest-max_nn cut are cell_walk.inc's; NormalQuery is what one
// lane group does with the kept candidates of one point.
#include "d3d_internal.h"

namespace d3d {

namespace {

using namespace celllist;
#include "cell_walk.inc"
#include "eigen3.inc"

// One query by one lane group.  Lane l of the group takes candidates l, l + 8, ... of every cell, cells in a fixed
// order: the kept set, the counts and the order of every sum do not depend on scheduling.
struct NormalQuery {
  uint32_t r2_bits;
  int max_nn, n;
  bool has_vp;
  float vx, vy, vz;
  float *normals;
  int32_t *counts;
  template <bool STAGED>
  __device__ __forceinline__ void run(const float4 *__restrict__ pts, const float4 *cand, const Ranges &R, int q, float4 P,
                                      int gl) const {
    uint32_t T = r2_bits;
    int J;
    const int m = nearest_cut<STAGED>(pts, cand, R, P, gl, max_nn, n, T, J);
    float s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // sum q, sum q q^T (xx xy xz yy yz zz), q = p_j - p_i
    for_candidates<STAGED>(pts, cand, R, gl, [&](float4 C, int) {
      const float dx = C.x - P.x, dy = C.y - P.y, dz = C.z - P.z;
      const uint32_t u = dist2_bits(C, P);
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
    });
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
};

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
  Timer T;
  CLN_TRY(T.start(phase_ms != nullptr, kPhases + 1));
  Arena A = scratch_arena(scratch, scratch_bytes);
  CellList L;
  CLN_TRY(celllist::build(xyz, n, stride, radius, A, s, &L, T.events()));
  CLN_TRY(launch_walk(L, n, NormalQuery{r2_bits(radius), max_nn, n, vp != nullptr, vp ? vp[0] : 0.f, vp ? vp[1] : 0.f,
                                        vp ? vp[2] : 0.f, normals, counts}, s));
  CLN_TRY(T.mark(4, s));
  CLN_TRY(T.mark(5, s));
  float ms[kPhases];                  // the timer's five; the caller's array holds cells, sort, table, search
  CLN_TRY(T.finish(ms));
  if (phase_ms)
    for (int k = 0; k < 4; k++) phase_ms[k] = ms[k];
  return D3D_OK;
}

}  // namespace
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
