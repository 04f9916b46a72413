// Posed depth frames -> one cloud, with image-space normals: the reference's depth_2_pcl
// (data3d/suncg_utils/suncg_preprocess.py:790-832, numpy fp64, one frame at a time on the CPU) for a whole batch of
// frames in two launches.  The arithmetic contract is written out in include/d3d_hip.h; it restates the
// reference and is not pinned against a run of it.
//
// Ordered compaction without an F H W sized array: workgroup g owns the pixels [g kRun, (g + 1) kRun) of the row-major
// index (f H + v) W + u.  k_up_count writes one count per workgroup (wave64 ballot + popcount), scan_exclusive_i32 turns
// the counts into bases and the total, the host reads the total back once and allocates the rows.  k_up_rows finds the
// kept pixels again from the depth, ranks the lanes of a wave with mbcnt over the ballot, and the waves and the 256-pixel
// steps of the run by a running count: the rows come out in ascending pixel index and no atomic is involved.
//
// Bytes, counted for a kept pixel with uint16 depth, uint8 colour and nine columns (the accounting of DESIGN 6g): 2 of
// depth and 3 of colour read, 36 written, so the depth is 2 of 41 bytes.  The left / right neighbours of the normals
// are in the lines the wave loads anyway; the rows above and below a run belong to the neighbouring workgroups' runs
// and are read from global memory: 2 W of kRun = 2048 pixels again, at W = 640 62 % of the depth = 1.25 of those 41
// bytes, 3 %, which the L2 and the Infinity Cache serve while the neighbours are in flight.  A staged halo would save
// those 3 % at the price of a second code path, so there is none.
//
// Stores: lane i of a step holds row (base + rank i), ncols floats; written directly, one store instruction would
// touch 64 addresses 12, 24 or 36 bytes apart.  The rows of a step are packed into LDS at their local rank instead and
// the workgroup copies the packed floats out with consecutive lanes on consecutive dwords: full lines.
#include "d3d_internal.h"

#include <algorithm>
#include <cmath>

namespace d3d {

namespace {

constexpr int kThreads = 256;
constexpr int kSteps = 8;
constexpr int kRun = kThreads * kSteps;      // pixels of one workgroup

#include "depth_frames.inc"   // DepthView, depth_at, valid_z, kept_at, Camera, cam_point, frames_view

__global__ __launch_bounds__(kThreads) void k_up_count(DepthView V, int32_t *__restrict__ counts) {
  __shared__ int wave_cnt[kThreads / 64];
  const int tid = threadIdx.x;
  int cnt = 0;                               // the same in every lane of a wave
  for (int it = 0; it < kSteps; it++) {
    const long p = (long)blockIdx.x * kRun + it * kThreads + tid;
    int f, v, u;
    double z;
    cnt += __popcll(__ballot(kept_at(V, p, f, v, u, z)));
  }
  if ((tid & 63) == 0) wave_cnt[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) counts[blockIdx.x] = (wave_cnt[0] + wave_cnt[1]) + (wave_cnt[2] + wave_cnt[3]);
}

// the camera-frame point of the neighbour (u + du, v + dv) of a pixel of depth z, when it is usable
__device__ __forceinline__ bool neighbour(const DepthView &V, const Camera &K, long p, int u, int v, double z, int du,
                                          int dv, double edge, double (&C)[3]) {
  const int uu = u + du, vv = v + dv;
  if (uu < 0 || uu >= V.W || vv < 0 || vv >= V.H) return false;
  const double zq = depth_at(V, p + du + (long)dv * V.W);
  if (!valid_z(V, zq) || !(fabs(zq - z) <= edge * z)) return false;
  cam_point(K, uu, vv, zq, C);
  return true;
}

// one-sided or central difference along one image axis; false: neither neighbour is usable
__device__ __forceinline__ bool difference(bool has_hi, const double (&hi)[3], bool has_lo, const double (&lo)[3],
                                           const double (&C)[3], double (&d)[3]) {
  if (!has_hi && !has_lo) return false;
#pragma unroll
  for (int k = 0; k < 3; k++) d[k] = (has_hi ? hi[k] : C[k]) - (has_lo ? lo[k] : C[k]);
  return true;
}

template <int NC>
__global__ __launch_bounds__(kThreads) void k_up_rows(DepthView V, const void *__restrict__ color, int color_u8,
                                                      double color_div, const double *__restrict__ intr,
                                                      const double *__restrict__ extr, double edge,
                                                      const int32_t *__restrict__ bases, int n_rows,
                                                      float *__restrict__ out, int32_t *__restrict__ pixel_of_point) {
  __shared__ float stage[kThreads * NC];
  __shared__ int wave_cnt[2][kThreads / 64];   // two sets: a wave may be one step ahead of another
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long row0 = bases[blockIdx.x];               // output row of this step's first kept pixel
  for (int it = 0; it < kSteps; it++) {
    const long p = (long)blockIdx.x * kRun + it * kThreads + tid;
    int f = 0, v = 0, u = 0;
    double z = 0.0;
    const bool keep = kept_at(V, p, f, v, u, z);
    const unsigned long long b = __ballot(keep);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
    if (lane == 0) wave_cnt[it & 1][wave] = __popcll(b);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; w++) {
      const int c = wave_cnt[it & 1][w];
      before += w < wave ? c : 0;
      total += c;
    }
    if (total == 0) continue;                  // the same in every thread
    if (keep) {
      const int local = before + rank;
      Camera K;
      load_camera(intr, extr, f, K);
      double C[3];
      cam_point(K, u, v, z, C);
      float *s = stage + local * NC;
#pragma unroll
      for (int k = 0; k < 3; k++) s[k] = (float)(((K.R[k][0] * C[0] + K.R[k][1] * C[1]) + K.R[k][2] * C[2]) + K.t[k]);
      if (NC >= 6) {
        if (!color) {
          s[3] = s[4] = s[5] = 0.f;
        } else if (color_u8) {
          const uint8_t *c = (const uint8_t *)color + 3 * p;
#pragma unroll
          for (int k = 0; k < 3; k++) s[3 + k] = (float)((double)c[k] / color_div);
        } else {
          const uint32_t *c = (const uint32_t *)color + 3 * p;
#pragma unroll
          for (int k = 0; k < 3; k++) s[3 + k] = __uint_as_float(c[k]);
        }
      }
      if (NC >= 9) {
        double hi[3], lo[3], a[3], d[3], n[3] = {0.0, 0.0, 0.0};
        bool has_hi = neighbour(V, K, p, u, v, z, 1, 0, edge, hi);
        bool has_lo = neighbour(V, K, p, u, v, z, -1, 0, edge, lo);
        bool ok = difference(has_hi, hi, has_lo, lo, C, a);
        has_hi = neighbour(V, K, p, u, v, z, 0, 1, edge, hi);
        has_lo = neighbour(V, K, p, u, v, z, 0, -1, edge, lo);
        ok = difference(has_hi, hi, has_lo, lo, C, d) && ok;
        if (ok) {
          double m[3] = {a[1] * d[2] - a[2] * d[1], a[2] * d[0] - a[0] * d[2], a[0] * d[1] - a[1] * d[0]};
          const double l2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
          if (l2 > 0.0) {
            if ((m[0] * C[0] + m[1] * C[1]) + m[2] * C[2] > 0.0) {
#pragma unroll
              for (int k = 0; k < 3; k++) m[k] = -m[k];
            }
            const double len = sqrt(l2);
#pragma unroll
            for (int k = 0; k < 3; k++) m[k] = m[k] / len;
#pragma unroll
            for (int k = 0; k < 3; k++) n[k] = (K.R[k][0] * m[0] + K.R[k][1] * m[1]) + K.R[k][2] * m[2];
          }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) s[6 + k] = (float)n[k];
      }
      if (pixel_of_point && row0 + local < n_rows) pixel_of_point[row0 + local] = (int32_t)p;
    }
    __syncthreads();
    // never past the rows the caller allocated, whatever the depth holds by now
    const int rows = (int)std::min<long>(total, std::max<long>((long)n_rows - row0, 0));
    float *o = out + row0 * NC;
    for (int k = tid; k < rows * NC; k += kThreads) o[k] = stage[k];
    row0 += total;
  }
}

inline long n_groups(long P) { return (P + kRun - 1) / kRun; }

struct Layout {
  int32_t *total, *counts, *bases;
};

int carve(Arena &A, long P, Layout &L) {
  const size_t G = (size_t)n_groups(P) + 2;
  D3D_ALLOC(total, int32_t, A, 64);
  D3D_ALLOC(counts, int32_t, A, G);
  D3D_ALLOC(bases, int32_t, A, G);
  L = Layout{total, counts, bases};
  return D3D_OK;
}

}  // namespace
}  // namespace d3d

using namespace d3d;

size_t d3d_unproject_scratch_bytes(int frames, int height, int width, int step) {
  (void)step;                                  // the runs are laid over all pixels, on the lattice or not
  const size_t P = (size_t)std::max(frames, 0) * (size_t)std::max(height, 0) * (size_t)std::max(width, 0);
  const size_t G = (size_t)n_groups((long)P) + 2;
  return 512 + 2 * (G * 4 + 256) + (G / 2048 + 1) * 4 + 4096;
}

int d3d_unproject_count(const d3d_depth_frames *frames, int step, double min_depth, double max_depth, void *scratch,
                        size_t scratch_bytes, int *info_host, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(info_host, "d3d_unproject_count: null pointer");
  info_host[0] = 0;
  DepthView V;
  int rc = frames_view("d3d_unproject_count", frames, step, min_depth, max_depth, kFramesDepth, V);
  if (rc) return rc;
  if (V.P == 0) return D3D_OK;
  D3D_REQUIRE(scratch, "d3d_unproject_count: null pointer");
  D3D_REQUIRE(scratch_bytes >= d3d_unproject_scratch_bytes(frames->frames, V.H, V.W, step),
              "d3d_unproject_count: scratch too small");
  Arena A = scratch_arena(scratch, scratch_bytes);
  Layout L;
  rc = carve(A, V.P, L);
  if (rc) return rc;
  const int G = (int)n_groups(V.P);
  hipLaunchKernelGGL(k_up_count, dim3((unsigned)G), dim3(kThreads), 0, s, V, L.counts);
  D3D_LAUNCH_CHECK();
  rc = scan_exclusive_i32(L.counts, L.bases, G, L.total, A, s);
  if (rc) return rc;
  rc = readback_publish(L.total, 1, s);
  if (rc) return rc;
  return readback_wait(info_host, 1);
}

int d3d_unproject_rows(const d3d_depth_frames *frames, int step, double min_depth, double max_depth, double color_div,
                       double edge, int ncols, const int *info_host, const void *scratch, size_t scratch_bytes, float *out,
                       int32_t *pixel_of_point, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(info_host && frames, "d3d_unproject_rows: null pointer");
  D3D_REQUIRE(ncols == 3 || ncols == 6 || ncols == 9, "d3d_unproject_rows: %d columns (3, 6 or 9)", ncols);
  D3D_REQUIRE(edge >= 0.0, "d3d_unproject_rows: edge %g must not be negative", edge);
  const void *color = frames->color;
  const int u8 = frames->color_is_u8 ? 1 : 0;
  D3D_REQUIRE(!(color && u8) || (color_div > 0.0 && color_div < (double)INFINITY),
              "d3d_unproject_rows: color_div %g must be positive and finite", color_div);
  DepthView V;
  int rc = frames_view("d3d_unproject_rows", frames, step, min_depth, max_depth, kFramesDepth | kFramesCameras, V);
  if (rc) return rc;
  const int N = info_host[0];
  D3D_REQUIRE(N >= 0 && (long)N <= V.P, "d3d_unproject_rows: %d rows of %ld pixels", N, V.P);
  if (V.P == 0 || N == 0) return D3D_OK;
  D3D_REQUIRE(scratch && out, "d3d_unproject_rows: null pointer");
  D3D_REQUIRE(scratch_bytes >= d3d_unproject_scratch_bytes(frames->frames, V.H, V.W, step),
              "d3d_unproject_rows: scratch too small");
  Arena A = scratch_arena(scratch, scratch_bytes);
  Layout L;
  rc = carve(A, V.P, L);
  if (rc) return rc;
  const dim3 grid((unsigned)n_groups(V.P)), block(kThreads);
#define D3D_UP_ROWS(NC)                                                                                                \
  hipLaunchKernelGGL(k_up_rows<NC>, grid, block, 0, s, V, color, u8, color_div, frames->intrinsics, frames->extrinsics, \
                     edge, (const int32_t *)L.bases, N, out, pixel_of_point)
  if (ncols == 3) D3D_UP_ROWS(3);
  else if (ncols == 6) D3D_UP_ROWS(6);
  else D3D_UP_ROWS(9);
#undef D3D_UP_ROWS
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}
