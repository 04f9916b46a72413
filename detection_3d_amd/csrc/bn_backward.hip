// a7. BatchNorm backward (SCN/CPU/BatchNormalization.cpp:62-107): partial sums of d' = dOut * relu' and
// (x - mean) d', fixed-order reduction, then the elementwise pass.  The forward half and the form record (t_bn_form)
// are bn.hip's.
#include <algorithm>

#include "d3d_internal.h"

namespace d3d {

typedef float f32x4 __attribute__((ext_vector_type(4)));

static constexpr int kBnBwdBlocks = 128;
template <typename T>
__global__ __launch_bounds__(256) void k_bn_bwd_partial(const T *__restrict__ x, const T *__restrict__ y,
                                                        const T *__restrict__ dy, int rows, int C,
                                                        const float *__restrict__ mean, float leak,
                                                        double *__restrict__ partial) {
  extern __shared__ double red[];
  const int tid = threadIdx.x;
  const int lpr = C < 256 ? C : 256, row_lanes = 256 / lpr;
  const int rl = tid / lpr, cl = tid % lpr;
  const int per = (rows + gridDim.x - 1) / gridDim.x;
  const int r0 = blockIdx.x * per, r1 = min(rows, r0 + per);
  for (int c = cl; c < C; c += lpr) {
    double s = 0, dp = 0;
    const float mu = mean[c];
    for (int r = r0 + rl; r < r1; r += row_lanes) {
      const size_t i = (size_t)r * C + c;
      const float d = ld1(dy + i) * ((ld1(y + i) > 0) ? 1.f : leak);
      s += (double)d;
      dp += (double)((ld1(x + i) - mu) * d);
    }
    red[tid * 2] = s;
    red[tid * 2 + 1] = dp;
    __syncthreads();
    if (rl == 0) {
      for (int j = 1; j < row_lanes; j++) {
        s += red[(j * lpr + cl) * 2];
        dp += red[(j * lpr + cl) * 2 + 1];
      }
      partial[(size_t)blockIdx.x * 2 * C + c] = s;
      partial[(size_t)blockIdx.x * 2 * C + C + c] = dp;
    }
    __syncthreads();
  }
}
// Same sums with 16-byte loads: threads = float4 channel groups x concurrent rows (1024 per workgroup), butterfly
// inside the wave, one LDS entry per wave -- the layout of k_bn_stats (bn.hip).  planes % 4 == 0, planes/4 | 1024.
template <typename T>
__global__ __launch_bounds__(1024) void k_bn_bwd_partial4(const T *__restrict__ x, const T *__restrict__ y,
                                                          const T *__restrict__ dy, int rows, int C,
                                                          const float *__restrict__ mean, float leak,
                                                          double *__restrict__ partial) {
  __shared__ double red[4][1024];
  const int tid = threadIdx.x;
  const int C4 = C >> 2;
  const int LPR = C4 < 1024 ? C4 : 1024;
  const int RL = 1024 / LPR;
  const int rl = tid / LPR, cl = tid - rl * LPR;
  const int per = (rows + gridDim.x - 1) / gridDim.x;
  const int r0 = blockIdx.x * per, r1 = min(rows, r0 + per);
  for (int g4 = cl; g4 < C4; g4 += LPR) {
    const f32x4 mu = *(const f32x4 *)(mean + g4 * 4);
    double s[4] = {0, 0, 0, 0}, dp[4] = {0, 0, 0, 0};
    for (int r = r0 + rl; r < r1; r += RL) {
      const size_t i = (size_t)r * C + g4 * 4;
      const f32x4 vx = load4<T>(x + i), vy = load4<T>(y + i), vd = load4<T>(dy + i);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float d = vd[j] * ((vy[j] > 0) ? 1.f : leak);
        s[j] += (double)d;
        dp[j] += (double)((vx[j] - mu[j]) * d);
      }
    }
    if (LPR < 64)
      for (int d = LPR; d < 64; d <<= 1)
#pragma unroll
        for (int j = 0; j < 4; j++) {
          s[j] += __shfl_xor(s[j], d, 64);
          dp[j] += __shfl_xor(dp[j], d, 64);
        }
    const int NE = LPR < 64 ? 16 : RL;
    const int e = LPR < 64 ? (tid >> 6) : rl;
    const bool holder = LPR < 64 ? (tid & 63) < LPR : true;
#pragma unroll
    for (int half = 0; half < 2; half++) {
      double *vals = half ? dp : s;
      if (holder)
#pragma unroll
        for (int j = 0; j < 4; j++) red[j][e * LPR + cl] = vals[j];
      __syncthreads();
      if (e == 0 && holder)
        for (int q = 1; q < NE; q++)
#pragma unroll
          for (int j = 0; j < 4; j++) vals[j] += red[j][q * LPR + cl];
      __syncthreads();
    }
    if (e == 0 && holder) {
      double *pp = partial + (size_t)blockIdx.x * 2 * C;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        pp[g4 * 4 + j] = s[j];
        pp[C + g4 * 4 + j] = dp[j];
      }
    }
  }
}
// dx for 4 channels per thread
template <typename T>
__global__ __launch_bounds__(256) void k_bn_bwd_apply4(const T *__restrict__ x, const T *__restrict__ y,
                                                       const T *__restrict__ dy, T *__restrict__ dx,
                                                       size_t total4, int C, const float *__restrict__ mean,
                                                       const float *__restrict__ invstd,
                                                       const float *__restrict__ weight,
                                                       const float *__restrict__ grad_mean,
                                                       const float *__restrict__ kcoef, float leak) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total4) return;
  const size_t i = t * 4;
  const int c = (int)(i % C);
  const f32x4 vx = load4<T>(x + i), vy = load4<T>(y + i), vd = load4<T>(dy + i);
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const float d = vd[j] * ((vy[j] > 0) ? 1.f : leak);
    o[j] = (d - grad_mean[c + j] - (vx[j] - mean[c + j]) * kcoef[c + j]) * invstd[c + j] * (weight ? weight[c + j] : 1.f);
  }
  store4(dx + i, o);
}
// the same arithmetic with one 4-channel group per thread walking rows (parameters read once per thread, see
// k_bn_apply_rows in bn.hip); C4 = C / 4 divides 256
template <typename T>
__global__ __launch_bounds__(256) void k_bn_bwd_apply_rows(const T *__restrict__ x, const T *__restrict__ y,
                                                           const T *__restrict__ dy, T *__restrict__ dx,
                                                           int rows, int C, const float *__restrict__ mean,
                                                           const float *__restrict__ invstd,
                                                           const float *__restrict__ weight,
                                                           const float *__restrict__ grad_mean,
                                                           const float *__restrict__ kcoef, float leak) {
  const int C4 = C >> 2, RPI = 256 / C4;
  const int cg = threadIdx.x % C4, rl = threadIdx.x / C4;
  const int c = cg * 4;
  f32x4 gm, mu, kc, is, wt;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    gm[j] = grad_mean[c + j];
    mu[j] = mean[c + j];
    kc[j] = kcoef[c + j];
    is[j] = invstd[c + j];
    wt[j] = weight ? weight[c + j] : 1.f;
  }
  const size_t step = (size_t)gridDim.x * RPI;
  auto one = [&](f32x4 vx, f32x4 vy, f32x4 vd) {
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float d = vd[j] * ((vy[j] > 0) ? 1.f : leak);
      o[j] = (d - gm[j] - (vx[j] - mu[j]) * kc[j]) * is[j] * wt[j];
    }
    return o;
  };
  size_t r = (size_t)blockIdx.x * RPI + rl;
  for (; r + step < (size_t)rows; r += 2 * step) {   // 2 rows = 6 loads in flight
    const size_t i0 = r * C + c, i1 = (r + step) * C + c;
    const f32x4 x0 = load4<T>(x + i0), y0 = load4<T>(y + i0), d0 = load4<T>(dy + i0);
    const f32x4 x1 = load4<T>(x + i1), y1 = load4<T>(y + i1), d1 = load4<T>(dy + i1);
    store4(dx + i0, one(x0, y0, d0));
    store4(dx + i1, one(x1, y1, d1));
  }
  for (; r < (size_t)rows; r += step) {
    const size_t i0 = r * C + c;
    store4(dx + i0, one(load4<T>(x + i0), load4<T>(y + i0), load4<T>(dy + i0)));
  }
}
__global__ __launch_bounds__(256) void k_bn_bwd_finish(const double *__restrict__ partial, int nblk, int rows,
                                                       int C, const float *__restrict__ invstd,
                                                       float *grad_mean, float *kcoef, float *d_weight,
                                                       float *d_bias) {
  __shared__ double red[256][2];
  const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  double s = 0, dp = 0;
  if (c < C)
    for (int b = sl; b < nblk; b += 8) {
      s += partial[(size_t)b * 2 * C + c];
      dp += partial[(size_t)b * 2 * C + C + c];
    }
  red[threadIdx.x][0] = s;
  red[threadIdx.x][1] = dp;
  __syncthreads();
  if (sl != 0 || c >= C) return;
  for (int j = 1; j < 8; j++) {
    s += red[j * 32 + cl][0];
    dp += red[j * 32 + cl][1];
  }
  const float is = invstd[c];
  if (d_bias) d_bias[c] = (float)s;
  if (d_weight) d_weight[c] = (float)dp * is;
  grad_mean[c] = (float)(s / rows);
  kcoef[c] = (float)dp * is * is / rows;
}
template <typename T>
__global__ __launch_bounds__(256) void k_bn_bwd_apply(const T *__restrict__ x, const T *__restrict__ y,
                                                      const T *__restrict__ dy, T *__restrict__ dx,
                                                      size_t total, int C, const float *__restrict__ mean,
                                                      const float *__restrict__ invstd,
                                                      const float *__restrict__ weight,
                                                      const float *__restrict__ grad_mean,
                                                      const float *__restrict__ kcoef, float leak) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const float d = ld1(dy + i) * ((ld1(y + i) > 0) ? 1.f : leak);
  st1(dx + i, (d - grad_mean[c] - (ld1(x + i) - mean[c]) * kcoef[c]) * invstd[c] * (weight ? weight[c] : 1.f));
}

// the scratch of a call, carved by bn_backward_t and by d3d_bn_backward_scratch_bytes
struct BnBwdLayout {
  double *partial;            // [kBnBwdBlocks][2][planes], whatever the number of slices launched
  float *grad_mean, *kcoef;   // [planes] each, one block: kcoef directly behind grad_mean
};
static int bn_bwd_carve(Arena &A, int planes, BnBwdLayout &L) {
  D3D_ALLOC(partial, double, A, (size_t)kBnBwdBlocks * 2 * planes);
  D3D_ALLOC(coef, float, A, 2 * (size_t)planes);
  L = BnBwdLayout{partial, coef, coef + planes};
  return D3D_OK;
}

// d3d_bn_backward_dt for storage type T (float, or bf16 as raw 16-bit words): fp32 arithmetic, fp64 partial sums
template <typename T>
static int bn_backward_t(const T *in, const T *out, const T *d_out, T *d_in, int rows, int planes, const float *save_mean,
                         const float *save_invstd, const float *weight, float *d_weight, float *d_bias, float leakiness,
                         void *scratch, size_t scratch_bytes, hipStream_t s) {
  D3D_REQUIRE(planes > 0 && rows >= 0 && save_mean && save_invstd, "bn_backward: bad arguments");
  if (rows == 0) return D3D_OK;
  D3D_REQUIRE(in && out && d_out && d_in, "bn_backward: null features");
  D3D_REQUIRE(planes >= 256 ? (planes % 256 == 0) : (256 % planes == 0), "bn_backward: planes=%d unsupported", planes);
  D3D_REQUIRE(scratch && scratch_bytes >= d3d_bn_backward_scratch_bytes(planes), "bn_backward: scratch too small");
  int nblk = kBnBwdBlocks;
  if (rows < nblk * 64) nblk = std::max(1, (rows + 63) / 64);
  Arena A = scratch_arena(scratch, scratch_bytes);
  BnBwdLayout L;
  if (int rc = bn_bwd_carve(A, planes, L)) return rc;
  double *partial = L.partial;
  float *grad_mean = L.grad_mean, *kcoef = L.kcoef;
  const bool vec4 = planes % 4 == 0 && 1024 % (planes / 4) == 0 && (((uintptr_t)in | (uintptr_t)out | (uintptr_t)d_out | (uintptr_t)d_in) & 15) == 0;
  if (vec4) {
    const int RL = 1024 / (planes / 4);
    nblk = std::max(1, std::min(kBnBwdBlocks, (rows + 8 * RL - 1) / (8 * RL)));
    hipLaunchKernelGGL(k_bn_bwd_partial4<T>, dim3(nblk), dim3(1024), 0, s, in, out, d_out, rows, planes, save_mean, leakiness,
                       partial);
  } else {
    hipLaunchKernelGGL(k_bn_bwd_partial<T>, dim3(nblk), dim3(256), 256 * 2 * sizeof(double), s, in, out, d_out, rows, planes,
                       save_mean, leakiness, partial);
  }
  hipLaunchKernelGGL(k_bn_bwd_finish, dim3((planes + 31) / 32), dim3(256), 0, s, partial, nblk, rows, planes,
                     save_invstd, grad_mean, kcoef, d_weight, d_bias);
  size_t total = (size_t)rows * planes;
  int apply_kernel = kBnApplyScalar;
  unsigned apply_wgs = (unsigned)((total + 255) / 256);
  bool apply_multi = false;
  if (vec4 && planes / 4 <= 256 && 256 % (planes / 4) == 0) {
    const int rpi = 256 / (planes / 4);
    const long need = ((long)rows + rpi - 1) / rpi;
    const unsigned blocks = (unsigned)std::max<long>(1, std::min<long>(need, 256 * 8));
    apply_kernel = kBnApplyRows, apply_wgs = blocks, apply_multi = (long)rows > (long)blocks * rpi;
    hipLaunchKernelGGL(k_bn_bwd_apply_rows<T>, dim3(blocks), dim3(256), 0, s, in, out, d_out, d_in, rows, planes, save_mean,
                       save_invstd, weight, grad_mean, kcoef, leakiness);
  } else if (vec4) {
    apply_kernel = kBnApplyVec4, apply_wgs = (unsigned)((total / 4 + 255) / 256);
    hipLaunchKernelGGL(k_bn_bwd_apply4<T>, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, s, in, out, d_out, d_in,
                       total / 4, planes, save_mean, save_invstd, weight, grad_mean, kcoef, leakiness);
  } else
    hipLaunchKernelGGL(k_bn_bwd_apply<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, out, d_out, d_in, total,
                       planes, save_mean, save_invstd, weight, grad_mean, kcoef, leakiness);
  int *f = t_bn_form;
  f[kBnBwPartial] = vec4 ? 1 : 2, f[kBnBwSlices] = nblk, f[kBnBwApply] = apply_kernel, f[kBnBwWgs] = (int)apply_wgs;
  f[kBnBwMulti] = apply_multi ? 1 : 0, f[kBnBwType] = bn_form_type<T>();
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

}  // namespace d3d

using namespace d3d;

extern "C" {

size_t d3d_bn_backward_scratch_bytes(int planes) {
  Arena A = sizing_arena();
  BnBwdLayout L;
  (void)bn_bwd_carve(A, planes, L);
  return A.used;
}

int d3d_bn_backward_dt(const void *in, const void *out, const void *d_out, void *d_in, int rows, int planes,
                       const float *save_mean, const float *save_invstd, const float *weight, float *d_weight,
                       float *d_bias, float leakiness, void *scratch, size_t scratch_bytes, int dtype, void *stream) {
  if (dtype == D3D_F32)
    return bn_backward_t((const float *)in, (const float *)out, (const float *)d_out, (float *)d_in, rows, planes,
                         save_mean, save_invstd, weight, d_weight, d_bias, leakiness, scratch, scratch_bytes,
                         (hipStream_t)stream);
  D3D_REQUIRE(dtype == D3D_BF16, "bn_backward_dt: dtype %d is neither D3D_F32 nor D3D_BF16", dtype);
  typedef unsigned short bf16_t;
  return bn_backward_t((const bf16_t *)in, (const bf16_t *)out, (const bf16_t *)d_out, (bf16_t *)d_in, rows, planes,
                       save_mean, save_invstd, weight, d_weight, d_bias, leakiness, scratch, scratch_bytes,
                       (hipStream_t)stream);
}

}  // extern "C"
