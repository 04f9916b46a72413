// Rotated boxes fitted to labelled points (include/d3d_hip.h, d3d_fit_boxes): per instance the candidate direction, out
// of 256 coarse and then 256 fine ones, whose axis-aligned extents of the rotated points enclose the smallest area.  The
// inverse of points_in_boxes.hip, with the same fp32 rotation u = c x - s y, v = s x + c y.
//
// The caller hands over the rows sorted by instance.  A workgroup takes kChunk consecutive sorted rows and stages their
// (x, y) once in LDS.  A thread is a candidate direction: all 256 threads walk the same staged points, two per 16-byte
// LDS read at one address for the whole wave (a broadcast, no bank conflict), and keep their four extents in registers;
// nothing is reduced across lanes.  A chunk holds pieces of one or of many instances: at the end of every run of equal
// ids a thread folds its four values into the [k, 256, 4] accumulator with unsigned atomic min / max of the order-
// preserving image of the floats.  Min and max commute, so neither the order of the rows nor of the atomics can show.
// z needs no direction: the staging takes its minimum and maximum (pass 1 only), one pair of atomics per wave where the
// wave's 64 rows belong to one instance.  A wave per instance then picks the direction of the smallest fp64 area, lowest
// index first; pass 2 repeats the sweep with the directions composed from the instance's coarse choice and the fine
// table, and its pick writes the box.  No device cos / sin: both tables come from the host.
#include "d3d_internal.h"

namespace d3d {
namespace {

constexpr int kThreads = 256;          // = candidate directions of a pass
constexpr int kChunk = 1024;           // sorted rows of one workgroup (primitives.FIT_CHUNK)
constexpr int kPerThread = kChunk / kThreads;
constexpr int kMaxBoxes = 4096;
constexpr double kPi = 3.14159265358979323846;

// accumulators of one pass: (umin, umax, vmin, vmax) images per instance and direction; z images per instance
__global__ void k_fit_begin(int k, uint4 *acc, uint32_t *zlo, uint32_t *zhi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k * kThreads) return;
  const uint32_t lo = f32_ordered(__builtin_inff()), hi = f32_ordered(-__builtin_inff());
  acc[i] = make_uint4(lo, hi, lo, hi);
  if (zlo && i < k) zlo[i] = lo, zhi[i] = hi;
}

// the fp32 direction (a, i): the coarse one turned by the fine one, products and sums in fp64 without contraction
__device__ __forceinline__ void compose(double ca, double sa, double fc, double fs, float &c, float &s) {
  const double p0 = ca * fc, p1 = sa * fs, p2 = sa * fc, p3 = ca * fs;
  c = (float)(p0 - p1);
  s = (float)(p2 + p3);
}

struct Ext {
  float un, ux, vn, vx;
  __device__ __forceinline__ void take(float c, float s, float x, float y) {
    const float cx = c * x, sy = s * y, sx = s * x, cy = c * y;
    const float u = cx - sy, v = sx + cy;
    un = __builtin_fminf(un, u), ux = __builtin_fmaxf(ux, u);
    vn = __builtin_fminf(vn, v), vx = __builtin_fmaxf(vx, v);
  }
};

// PASS 1: thread t sweeps coarse direction t and the staging takes z.  PASS 2: thread t sweeps (choice[g].a, t).
template <int PASS>
__global__ __launch_bounds__(kThreads) void k_fit_sweep(const float *__restrict__ xyz, int n, int stride,
                                                         const double *__restrict__ origin,
                                                         const int32_t *__restrict__ order,
                                                         const int32_t *__restrict__ sorted_id,
                                                         const int32_t *__restrict__ offsets, int k,
                                                         const double *__restrict__ coarse, const double *__restrict__ fine,
                                                         const int32_t *__restrict__ choice, uint32_t *__restrict__ acc,
                                                         uint32_t *__restrict__ zlo, uint32_t *__restrict__ zhi) {
  __shared__ float4 xy4[kChunk / 2];                     // (x, y) of two staged rows per 16-byte read
  float2 *xy = reinterpret_cast<float2 *>(xy4);
  __shared__ int32_t ids[kChunk];
  const int tid = threadIdx.x;
  const int m = min(offsets[k], n);                      // the sorted rows that belong to an instance
  const long base = (long)blockIdx.x * kChunk;
  if (base >= m) return;
  const int cnt = (int)min((long)kChunk, m - base);
  double o0 = 0.0, o1 = 0.0, o2 = 0.0;
  if (origin) o0 = origin[0], o1 = origin[1], o2 = origin[2];
#pragma unroll
  for (int j = 0; j < kPerThread; j++) {
    const int l = j * kThreads + tid;
    int g = -1;
    float x = 0.f, y = 0.f, z = 0.f;
    if (l < cnt) {
      const int row = order[base + l];
      g = sorted_id[base + l];
      if ((unsigned)row < (unsigned)n && (unsigned)g < (unsigned)k) {
        const float *p = xyz + (size_t)row * (size_t)stride;
        x = p[0], y = p[1], z = p[2];
        if (origin) {
          x = (float)((double)x - o0);
          y = (float)((double)y - o1);
          z = (float)((double)z - o2);
        }
      } else {
        g = -1;                                          // not a row of the caller's lists: skipped by the walk
      }
    }
    xy[l] = make_float2(x, y);
    ids[l] = g;
    if (PASS == 1) {
      const bool live = g >= 0;
      const int g0 = __builtin_amdgcn_readfirstlane(g);
      if (__ballot(live && g == g0) == ~0ull) {          // the wave's 64 rows are one instance's
        float lo = z, hi = z;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
          lo = __builtin_fminf(lo, __shfl_xor(lo, d, 64));
          hi = __builtin_fmaxf(hi, __shfl_xor(hi, d, 64));
        }
        if ((tid & 63) == 0) atomicMin(zlo + g0, f32_ordered(lo + 0.f)), atomicMax(zhi + g0, f32_ordered(hi + 0.f));
      } else if (live) {
        atomicMin(zlo + g, f32_ordered(z + 0.f)), atomicMax(zhi + g, f32_ordered(z + 0.f));
      }
    }
  }
  float c = 0.f, s = 0.f;
  double fc = 0.0, fs = 0.0;
  if (PASS == 1) {
    c = (float)coarse[2 * tid], s = (float)coarse[2 * tid + 1];
  } else {
    fc = fine[2 * tid], fs = fine[2 * tid + 1];
  }
  __syncthreads();

  int p = 0;
  while (p < cnt) {                                      // p, g, end are the same in every thread
    const int g = __builtin_amdgcn_readfirstlane(ids[p]);
    if (g < 0) {
      p++;
      continue;
    }
    int end = (int)min((long)cnt, (long)offsets[g + 1] - base);
    end = max(end, p + 1);
    if (PASS == 2) {
      const int a = choice[2 * g] & 255;
      compose(coarse[2 * a], coarse[2 * a + 1], fc, fs, c, s);
    }
    Ext e = {__builtin_inff(), -__builtin_inff(), __builtin_inff(), -__builtin_inff()};
    int q = p;
    if (q & 1) {
      const float2 t = xy[q];
      e.take(c, s, t.x, t.y);
      q++;
    }
#pragma unroll 2
    for (; q + 1 < end; q += 2) {
      const float4 t = xy4[q >> 1];
      e.take(c, s, t.x, t.y);
      e.take(c, s, t.z, t.w);
    }
    if (q < end) {
      const float2 t = xy[q];
      e.take(c, s, t.x, t.y);
    }
    // + 0: a -0 becomes +0, so that the extents do not depend on how a zero came about
    uint32_t *a4 = acc + ((size_t)g * kThreads + tid) * 4;
    atomicMin(a4 + 0, f32_ordered(e.un + 0.f)), atomicMax(a4 + 1, f32_ordered(e.ux + 0.f));
    atomicMin(a4 + 2, f32_ordered(e.vn + 0.f)), atomicMax(a4 + 3, f32_ordered(e.vx + 0.f));
    p = end;
  }
}

// One wave per instance: the direction of the smallest area, the lowest index among equals.  PASS 1 leaves the coarse
// index in choice[g][0]; PASS 2 leaves the fine one in choice[g][1] and writes the instance's row of every output.
template <int PASS>
__global__ __launch_bounds__(64) void k_fit_pick(int k, const uint4 *__restrict__ acc, const uint32_t *__restrict__ zlo,
                                                  const uint32_t *__restrict__ zhi, const int32_t *__restrict__ offsets,
                                                  const uint8_t *__restrict__ yaw_free, const double *__restrict__ coarse,
                                                  const double *__restrict__ fine, float *__restrict__ boxes,
                                                  int32_t *__restrict__ count, int32_t *__restrict__ choice,
                                                  float *__restrict__ extent) {
  const int g = blockIdx.x, lane = threadIdx.x;
  if (g >= k) return;
  const int cnt = offsets[g + 1] - offsets[g];
  const bool free_yaw = yaw_free ? yaw_free[g] != 0 : true;
  if (cnt <= 0) {
    if (lane == 0) {
      choice[2 * g + PASS - 1] = -1;
      if (PASS == 2) {
        count[g] = 0;
        for (int j = 0; j < 7; j++) boxes[(size_t)g * 7 + j] = 0.f;
        for (int j = 0; j < 6; j++) extent[(size_t)g * 6 + j] = (j & 1) ? -__builtin_inff() : __builtin_inff();
      }
    }
    return;
  }
  double best = 0.0;
  int at = -1;
#pragma unroll
  for (int j = 0; j < kThreads / 64; j++) {
    const int d = j * 64 + lane;
    const uint4 w = acc[(size_t)g * kThreads + d];
    const double eu = (double)ordered_to_f32(w.y) - (double)ordered_to_f32(w.x);
    const double ev = (double)ordered_to_f32(w.w) - (double)ordered_to_f32(w.z);
    const double area = eu * ev;
    if (at < 0 || area < best) best = area, at = d;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double ob = __shfl_xor(best, d, 64);
    const int oa = __shfl_xor(at, d, 64);
    if (ob < best || (ob == best && oa < at)) best = ob, at = oa;
  }
  if (lane != 0) return;
  if (!free_yaw) at = PASS == 1 ? 0 : 128;
  choice[2 * g + PASS - 1] = at;
  if (PASS == 1) return;

  const int a = choice[2 * g] & 255, i = at;
  float c, s;
  compose(coarse[2 * a], coarse[2 * a + 1], fine[2 * i], fine[2 * i + 1], c, s);
  const uint4 w = acc[(size_t)g * kThreads + i];
  const float umin = ordered_to_f32(w.x), umax = ordered_to_f32(w.y), vmin = ordered_to_f32(w.z), vmax = ordered_to_f32(w.w);
  const float zmin = ordered_to_f32(zlo[g]), zmax = ordered_to_f32(zhi[g]);
  const double theta = (double)(a * 128 + (i - 128)) * (kPi / 65536.0);
  const double eu = (double)umax - (double)umin, ev = (double)vmax - (double)vmin;
  const double mu = ((double)umin + (double)umax) * 0.5, mv = ((double)vmin + (double)vmax) * 0.5;
  const double cd = (double)c, sd = (double)s;
  const double x0 = cd * mu, x1 = sd * mv, y0 = -sd * mu, y1 = cd * mv;
  double d3 = eu, d4 = ev, yaw = theta;
  if (free_yaw && eu > ev) d3 = ev, d4 = eu, yaw = theta + kPi / 2;
  if (yaw >= kPi / 2) yaw -= kPi;
  float *b = boxes + (size_t)g * 7;
  b[0] = (float)(x0 + x1), b[1] = (float)(y0 + y1), b[2] = zmin;
  b[3] = (float)d3, b[4] = (float)d4, b[5] = (float)((double)zmax - (double)zmin), b[6] = (float)yaw;
  count[g] = cnt;
  float *e = extent + (size_t)g * 6;
  e[0] = umin, e[1] = umax, e[2] = vmin, e[3] = vmax, e[4] = zmin, e[5] = zmax;
}

size_t fit_scratch_bytes(int k) {
  const size_t kk = (size_t)max(k, 1);
  return kk * kThreads * sizeof(uint4) + 256 + 2 * (kk * sizeof(uint32_t) + 256);
}

}  // namespace
}  // namespace d3d

using namespace d3d;

size_t d3d_fit_boxes_scratch_bytes(int k) { return k < 0 || k > kMaxBoxes ? 0 : fit_scratch_bytes(k); }

int d3d_fit_boxes(const float *xyz, int n, int row_stride_floats, const double *origin_dev, const int32_t *order,
                  const int32_t *sorted_id, const int32_t *offsets, int k, const uint8_t *yaw_free,
                  const double *coarse_dev, const double *fine_dev, float *boxes, int32_t *count, int32_t *choice,
                  float *extent, void *scratch, size_t scratch_bytes, void *stream, float *phase_ms_host) {
  D3D_REQUIRE(n >= 0 && k >= 0, "d3d_fit_boxes: n %d, k %d must not be negative", n, k);
  D3D_REQUIRE(k <= kMaxBoxes, "d3d_fit_boxes: %d instances, at most %d", k, kMaxBoxes);
  if (phase_ms_host) phase_ms_host[0] = phase_ms_host[1] = 0.f;
  if (k == 0) return D3D_OK;
  D3D_REQUIRE(row_stride_floats >= 3, "d3d_fit_boxes: row stride %d < 3 floats", row_stride_floats);
  D3D_REQUIRE(n == 0 || (xyz && order && sorted_id), "d3d_fit_boxes: null pointer (xyz, order, sorted_id)");
  D3D_REQUIRE(offsets && coarse_dev && fine_dev, "d3d_fit_boxes: null pointer (offsets, coarse, fine)");
  D3D_REQUIRE(boxes && count && choice && extent, "d3d_fit_boxes: null pointer (boxes, count, choice, extent)");
  D3D_REQUIRE(scratch && scratch_bytes >= fit_scratch_bytes(k), "d3d_fit_boxes: scratch of %zu bytes, need %zu",
              scratch_bytes, fit_scratch_bytes(k));
  hipStream_t s = (hipStream_t)stream;
  Arena A = scratch_arena(scratch, scratch_bytes);
  D3D_ALLOC(acc, uint4, A, (size_t)k * kThreads);
  D3D_ALLOC(zlo, uint32_t, A, k);
  D3D_ALLOC(zhi, uint32_t, A, k);
  uint32_t *acc_u = reinterpret_cast<uint32_t *>(acc);
  const dim3 cells = grid1d((long)k * kThreads), chunks = grid1d(n, kChunk);
  Timer T;                            // coarse pass, fine pass
  if (int rc = T.start(phase_ms_host != nullptr, 3)) return rc;
  if (int rc = T.mark(0, s)) return rc;
  hipLaunchKernelGGL(k_fit_begin, cells, dim3(256), 0, s, k, acc, zlo, zhi);
  if (n > 0)
    hipLaunchKernelGGL(k_fit_sweep<1>, chunks, dim3(kThreads), 0, s, xyz, n, row_stride_floats, origin_dev, order,
                       sorted_id, offsets, k, coarse_dev, fine_dev, choice, acc_u, zlo, zhi);
  hipLaunchKernelGGL(k_fit_pick<1>, dim3(k), dim3(64), 0, s, k, acc, zlo, zhi, offsets, yaw_free, coarse_dev, fine_dev,
                     boxes, count, choice, extent);
  if (int rc = T.mark(1, s)) return rc;
  hipLaunchKernelGGL(k_fit_begin, cells, dim3(256), 0, s, k, acc, (uint32_t *)nullptr, (uint32_t *)nullptr);
  if (n > 0)
    hipLaunchKernelGGL(k_fit_sweep<2>, chunks, dim3(kThreads), 0, s, xyz, n, row_stride_floats, origin_dev, order,
                       sorted_id, offsets, k, coarse_dev, fine_dev, choice, acc_u, zlo, zhi);
  hipLaunchKernelGGL(k_fit_pick<2>, dim3(k), dim3(64), 0, s, k, acc, zlo, zhi, offsets, yaw_free, coarse_dev, fine_dev,
                     boxes, count, choice, extent);
  D3D_LAUNCH_CHECK();
  if (int rc = T.mark(2, s)) return rc;
  return T.finish(phase_ms_host);
}
