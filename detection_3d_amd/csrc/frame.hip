// The Manhattan frame of a scan from its normals (include/d3d_hip.h, d3d_manhattan_frame): the rotation that levels the
// cloud and squares it to its walls, by the route of box_fit.hip.  Candidate directions come from host tables, a thread
// is a candidate, the rows are staged in LDS and the scores are 64-bit integer sums, so that no order can show.
//
// Five passes of 256 candidates: three of tilt (a 16 x 16 lattice of up directions around the frame so far, each an
// eighth as wide as the one before) and two of heading (a quarter turn coarse, then fine, over the rows the final up
// direction calls walls).  A workgroup takes kChunk rows at a time and stages per row (n0, n1, n2, m) and the factor
// that turns its vote into an integer (tilt), or (p, q, factor) (heading).  A row that does not vote is staged as zeros
// with the factor 0: its vote would be s2 under the plain expression (a zero normal is within every tolerance), times 0
// it is exactly 0, and the walk needs no branch.  All 256 threads walk the same staged rows, one LDS address for the
// whole wave per read (a broadcast), keep their sum in registers over a grid-stride loop of chunks and add it to
// acc[256] with one 64-bit integer atomic each.  One wave then picks the winner, the lowest index among equals, and
// composes the next pass's frame in fp64; nothing is read back.  No device sin / cos / sqrt / divide.
#include "d3d_internal.h"

namespace d3d {
namespace {

constexpr int kThreads = 256;          // = candidates of a pass
constexpr int kChunk = 1024;           // rows a workgroup stages at a time (frame.FRAME_CHUNK)
constexpr int kPerThread = kChunk / kThreads;
constexpr int kMaxGrid = 2048;         // workgroups of a sweep; more chunks than that are taken in a grid-stride loop
constexpr int kPasses = 5;
constexpr float kVoteScale = 1073741824.f;   // 2^30
enum { kTilt = 0, kHeadCoarse = 1, kHeadFine = 2 };

struct Mat3 {
  double v[9];
};

// element (r, c) of B M, both row-major 3 x 3: (B[r,0] M[0,c] + B[r,1] M[1,c]) + B[r,2] M[2,c], no contraction
__device__ __forceinline__ double mul_rc(const double *B, const double *M, int r, int c) {
  const double p0 = B[3 * r] * M[c], p1 = B[3 * r + 1] * M[3 + c], p2 = B[3 * r + 2] * M[6 + c];
  return (p0 + p1) + p2;
}

// fp64 (C, S) of the coarse direction turned by the fine one: products and sums separate operations
__device__ __forceinline__ void compose(double ca, double sa, double fc, double fs, double &c, double &s) {
  const double p0 = ca * fc, p1 = sa * fs, p2 = sa * fc, p3 = ca * fs;
  c = p0 - p1;
  s = p2 + p3;
}

__device__ __forceinline__ float dot3(float n0, float n1, float n2, float u0, float u1, float u2) {
  const float a = n0 * u0, b = n1 * u1, c = n2 * u2;
  return (a + b) + c;
}

// accumulators of all passes, the frame B_0, and the outputs of a call in which no pass finds a vote
__global__ void k_frame_begin(Mat3 b0, unsigned long long *acc, double *B, int32_t *choice, long long *score,
                              int32_t *support) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < kPasses * kThreads) acc[i] = 0ull;
  if (i < 9) B[i] = b0.v[i];
  if (i < kPasses) choice[i] = i < 3 ? 136 : (i == 3 ? 0 : 128), score[i] = 0;
  if (i < 2) support[i] = 0;
}

// the vote of a staged tilt row e = (n0, n1, n2, m) with factor w for the direction u
__device__ __forceinline__ int vote_tilt(float4 e, float w, float u0, float u1, float u2, float s2) {
  const float d = dot3(e.x, e.y, e.z, u0, u1, u2);
  const float a2 = d * d;
  const float r = __builtin_fminf(a2, __builtin_fmaxf(e.w - a2, 0.f));
  const float v = __builtin_fmaxf(s2 - r, 0.f);
  return (int)(v * w);
}

// the vote of a staged heading row e = (p, q, factor, .) for the direction (c, s)
__device__ __forceinline__ int vote_head(float4 e, float c, float s, float s2) {
  const float cp = c * e.x, sq = s * e.y, cq = c * e.y, sp = s * e.x;
  const float d1 = cp + sq, d2 = cq - sp;
  const float r = __builtin_fminf(d1 * d1, d2 * d2);
  const float v = __builtin_fmaxf(s2 - r, 0.f);
  return (int)(v * e.z);
}

// kTilt: thread t sweeps the up direction of B M[t] over the voting rows.  kHeadCoarse / kHeadFine: thread t sweeps
// coarse heading t / (choice[3], t) over the wall rows of the final frame B; kHeadCoarse also counts support.
template <int KIND>
__global__ __launch_bounds__(kThreads) void k_frame_sweep(const float *__restrict__ nrm, int n, int stride,
                                                           const double *__restrict__ B, const double *__restrict__ table,
                                                           const double *__restrict__ fine,
                                                           const int32_t *__restrict__ choice, float s2,
                                                           unsigned long long *__restrict__ acc,
                                                           int32_t *__restrict__ support) {
  __shared__ float4 row4[kChunk];
  __shared__ float wgt[KIND == kTilt ? kChunk : 1];
  const int tid = threadIdx.x;
  float u0, u1, u2;                                      // tilt: the candidate; heading: the final up direction
  float x0 = 0.f, x1 = 0.f, x2 = 0.f, y0 = 0.f, y1 = 0.f, y2 = 0.f, c = 0.f, s = 0.f;
  if (KIND == kTilt) {
    const double *M = table + (size_t)tid * 9;
    u0 = (float)mul_rc(B, M, 0, 2), u1 = (float)mul_rc(B, M, 1, 2), u2 = (float)mul_rc(B, M, 2, 2);
  } else {
    x0 = (float)B[0], x1 = (float)B[3], x2 = (float)B[6];
    y0 = (float)B[1], y1 = (float)B[4], y2 = (float)B[7];
    u0 = (float)B[2], u1 = (float)B[5], u2 = (float)B[8];
    if (KIND == kHeadCoarse) {
      c = (float)table[2 * tid], s = (float)table[2 * tid + 1];
    } else {
      const int a = choice[3] & 255;
      double cd, sd;
      compose(table[2 * a], table[2 * a + 1], fine[2 * tid], fine[2 * tid + 1], cd, sd);
      c = (float)cd, s = (float)sd;
    }
  }
  unsigned long long sum = 0ull;
  int n_valid = 0, n_wall = 0;
  const long chunks = ((long)n + kChunk - 1) / kChunk;
  for (long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    const long base = chunk * kChunk;
    const int cnt = (int)min((long)kChunk, (long)n - base);
#pragma unroll
    for (int j = 0; j < kPerThread; j++) {
      const int l = j * kThreads + tid;
      float n0 = 0.f, n1 = 0.f, n2 = 0.f, m = 0.f;
      bool valid = false;
      if (l < cnt) {
        const float *p = nrm + (size_t)(base + l) * (size_t)stride;
        n0 = p[0], n1 = p[1], n2 = p[2];
        m = dot3(n0, n1, n2, n0, n1, n2);
        valid = m >= 0.5f && m <= 2.f;                   // NaN, infinite and zero rows fail
      }
      if (KIND == kTilt) {
        row4[l] = valid ? make_float4(n0, n1, n2, m) : make_float4(0.f, 0.f, 0.f, 0.f);
        wgt[l] = valid ? kVoteScale : 0.f;
      } else {
        bool wall = false;
        float p_ = 0.f, q_ = 0.f;
        if (valid) {
          const float d = dot3(n0, n1, n2, u0, u1, u2);
          wall = d * d <= s2;
          p_ = dot3(n0, n1, n2, x0, x1, x2), q_ = dot3(n0, n1, n2, y0, y1, y2);
        }
        row4[l] = wall ? make_float4(p_, q_, kVoteScale, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
        n_valid += valid, n_wall += wall;
      }
    }
    __syncthreads();
    const int cnt4 = (cnt + 3) & ~3;                     // rows past cnt are staged as rows that do not vote
    for (int q = 0; q < cnt4; q += 4) {
      int part = 0;                                      // four votes < 2^27 each
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (KIND == kTilt) part += vote_tilt(row4[q + k], wgt[q + k], u0, u1, u2, s2);
        else part += vote_head(row4[q + k], c, s, s2);
      }
      sum += (unsigned long long)(unsigned)part;
    }
    __syncthreads();
  }
  if (sum) atomicAdd(acc + tid, sum);
  if (KIND == kHeadCoarse) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n_valid += __shfl_xor(n_valid, d, 64), n_wall += __shfl_xor(n_wall, d, 64);
    if ((tid & 63) == 0 && n_valid) atomicAdd(support, n_valid), atomicAdd(support + 1, n_wall);
  }
}

// One wave: the candidate of the highest score, the lowest index among equals, `none` when no row voted.  kTilt
// composes B <- B M[winner]; kHeadFine writes the pose.
template <int KIND>
__global__ __launch_bounds__(64) void k_frame_pick(int pass, const unsigned long long *__restrict__ acc,
                                                    const double *__restrict__ table, const double *__restrict__ fine,
                                                    double *__restrict__ B, int32_t *__restrict__ choice,
                                                    long long *__restrict__ score, double *__restrict__ pose) {
  const int lane = threadIdx.x;
  long long best = -1;
  int at = 0;
#pragma unroll
  for (int j = 0; j < kThreads / 64; j++) {
    const int d = j * 64 + lane;
    const long long sc = (long long)acc[d];
    if (sc > best) best = sc, at = d;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const long long ob = __shfl_xor(best, d, 64);
    const int oa = __shfl_xor(at, d, 64);
    if (ob > best || (ob == best && oa < at)) best = ob, at = oa;
  }
  if (lane != 0) return;
  if (best <= 0) at = KIND == kTilt ? 136 : (KIND == kHeadCoarse ? 0 : 128);
  choice[pass] = at;
  score[pass] = best;
  if (KIND == kTilt) {
    const double *M = table + (size_t)at * 9;
    double nb[9];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) nb[3 * r + c] = mul_rc(B, M, r, c);
    for (int i = 0; i < 9; i++) B[i] = nb[i];
  }
  if (KIND == kHeadFine) {
    const int ia = choice[3] & 255;
    double C, S;
    compose(table[2 * ia], table[2 * ia + 1], fine[2 * at], fine[2 * at + 1], C, S);
    if (128 * ia + at - 128 >= 16384) {                  // of the four equal headings the one within 45 degrees
      const double t = C;
      C = S, S = -t;
    }
    const double Rz[9] = {C, -S, 0.0, S, C, 0.0, 0.0, 0.0, 1.0};
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) pose[4 * c + r] = mul_rc(B, Rz, r, c);      // the transpose: aligned <- scan
    pose[3] = pose[7] = pose[11] = 0.0;
    pose[12] = pose[13] = pose[14] = 0.0, pose[15] = 1.0;
  }
}

size_t frame_scratch_bytes() { return (size_t)kPasses * kThreads * sizeof(unsigned long long) + 256 + 9 * sizeof(double) + 256; }

}  // namespace
}  // namespace d3d

using namespace d3d;

size_t d3d_manhattan_frame_scratch_bytes() { return frame_scratch_bytes(); }

int d3d_manhattan_frame(const float *normals, int n, int row_stride_floats, const double *tilt_tables_dev,
                        const double *b0_host, const float *s2_host, const double *coarse_dev, const double *fine_dev,
                        double *pose, int32_t *choice, int64_t *score, int32_t *support, void *scratch,
                        size_t scratch_bytes, void *stream, float *phase_ms_host) {
  D3D_REQUIRE(n >= 0, "d3d_manhattan_frame: n %d must not be negative", n);
  D3D_REQUIRE(n == 0 || normals, "d3d_manhattan_frame: null pointer (normals)");
  D3D_REQUIRE(n <= 1 || row_stride_floats >= 3, "d3d_manhattan_frame: row stride %d < 3 floats", row_stride_floats);
  D3D_REQUIRE(s2_host && coarse_dev && fine_dev, "d3d_manhattan_frame: null pointer (s2, coarse, fine)");
  D3D_REQUIRE(pose && choice && score && support, "d3d_manhattan_frame: null pointer (pose, choice, score, support)");
  for (int k = 0; k < 4; k++)
    D3D_REQUIRE(s2_host[k] > 0.f && s2_host[k] <= 0.125f, "d3d_manhattan_frame: s2[%d] = %g outside (0, 0.125]", k,
                (double)s2_host[k]);
  D3D_REQUIRE(scratch && scratch_bytes >= frame_scratch_bytes(), "d3d_manhattan_frame: scratch of %zu bytes, need %zu",
              scratch_bytes, frame_scratch_bytes());
  if (phase_ms_host)
    for (int k = 0; k < kPasses; k++) phase_ms_host[k] = 0.f;
  hipStream_t s = (hipStream_t)stream;
  Arena A = scratch_arena(scratch, scratch_bytes);
  D3D_ALLOC(acc, unsigned long long, A, (size_t)kPasses * kThreads);
  D3D_ALLOC(B, double, A, 9);
  Mat3 b0 = {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}};
  if (b0_host)
    for (int i = 0; i < 9; i++) b0.v[i] = b0_host[i];
  long long *score_ll = reinterpret_cast<long long *>(score);
  const long chunks = ((long)n + kChunk - 1) / kChunk;
  const dim3 grid((unsigned)(chunks < kMaxGrid ? chunks : kMaxGrid)), block(kThreads);
  Timer T;                            // one phase per pass: its sweep and its pick
  if (int rc = T.start(phase_ms_host != nullptr, kPasses + 1)) return rc;
  hipLaunchKernelGGL(k_frame_begin, grid1d(kPasses * kThreads), dim3(256), 0, s, b0, acc, B, choice, score_ll, support);
  for (int k = 0; k < 3; k++) {
    if (int rc = T.mark(k, s)) return rc;
    if (!tilt_tables_dev) continue;   // max_tilt 0: B_3 = B_0, the choices stay 136 and the scores 0
    const double *M = tilt_tables_dev + (size_t)k * kThreads * 9;
    if (n > 0)
      hipLaunchKernelGGL(k_frame_sweep<kTilt>, grid, block, 0, s, normals, n, row_stride_floats, B, M,
                         (const double *)nullptr, choice, s2_host[k], acc + k * kThreads, support);
    hipLaunchKernelGGL(k_frame_pick<kTilt>, dim3(1), dim3(64), 0, s, k, acc + k * kThreads, M, (const double *)nullptr,
                       B, choice, score_ll, pose);
  }
  if (int rc = T.mark(3, s)) return rc;
  if (n > 0)
    hipLaunchKernelGGL(k_frame_sweep<kHeadCoarse>, grid, block, 0, s, normals, n, row_stride_floats, B, coarse_dev,
                       fine_dev, choice, s2_host[3], acc + 3 * kThreads, support);
  hipLaunchKernelGGL(k_frame_pick<kHeadCoarse>, dim3(1), dim3(64), 0, s, 3, acc + 3 * kThreads, coarse_dev, fine_dev, B,
                     choice, score_ll, pose);
  if (int rc = T.mark(4, s)) return rc;
  if (n > 0)
    hipLaunchKernelGGL(k_frame_sweep<kHeadFine>, grid, block, 0, s, normals, n, row_stride_floats, B, coarse_dev,
                       fine_dev, choice, s2_host[3], acc + 4 * kThreads, support);
  hipLaunchKernelGGL(k_frame_pick<kHeadFine>, dim3(1), dim3(64), 0, s, 4, acc + 4 * kThreads, coarse_dev, fine_dev, B,
                     choice, score_ll, pose);
  D3D_LAUNCH_CHECK();
  if (int rc = T.mark(5, s)) return rc;
  return T.finish(phase_ms_host);
}
