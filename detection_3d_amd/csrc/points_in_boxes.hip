// Points of each rotated box (include/d3d_hip.h, d3d_points_in_boxes): membership of every point in every box, the
// lowest box that holds each point, and per box the member count and the extent of its members in the box frame -- what
// Bbox3D.points_in_bbox (utils3d/bbox3d_ops.py:731-755), split_bbox's counts (data3d/indoor_data_util.py:244-254) and
// crop_bbox_by_points' minima and maxima (bbox3d_ops.py:873-878) compute from an [N, K] mask, without that mask.
//
// Lanes own points (kPointsPerLane each, in registers) and sweep the boxes, which the workgroup stages in LDS a tile of
// kTile at a time: centre, cos, sin (fp64, rounded to fp32 -- rbbox_to_corners of the IoU path), half sizes and height
// after `grow`.  A box that no lane of the wave hits costs one ballot.  For one that is hit, the count and the six
// extents are reduced across the wave, then into the tile's LDS accumulators, and after the sweep every box the
// workgroup touched gets one global atomic per quantity: an integer add, and unsigned min / max of the order-preserving
// image of the floats.  Integer add, min and max commute, so the results do not depend on the order of the atomics.
#include "d3d_internal.h"

namespace d3d {
namespace {

constexpr int kThreads = 256;
constexpr int kPointsPerLane = 4;
constexpr int kSpan = kThreads * kPointsPerLane;   // points of one workgroup
constexpr int kTile = 256;                         // boxes staged at a time
constexpr int kMaxBoxes = 4096;

// count = 0, lo = image(+inf), hi = image(-inf): the accumulators the sweep's atomics start from
__global__ void k_pib_begin(int k, int32_t *count, uint32_t *lo, uint32_t *hi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * k) return;
  if (i < k) count[i] = 0;
  lo[i] = f32_ordered(__builtin_inff());
  hi[i] = f32_ordered(-__builtin_inff());
}

// the images back to floats, in place
__global__ void k_pib_end(int k, uint32_t *lo, uint32_t *hi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * k) return;
  reinterpret_cast<float *>(lo)[i] = ordered_to_f32(lo[i]);
  reinterpret_cast<float *>(hi)[i] = ordered_to_f32(hi[i]);
}

struct BoxTile {
  float xc[kTile], yc[kTile], zb[kTile], c[kTile], s[kTile], hx[kTile], hy[kTile], hz[kTile];
  int32_t count[kTile];
  uint32_t lo[3][kTile], hi[3][kTile];
};

__global__ __launch_bounds__(kThreads) void k_pib_sweep(const float *__restrict__ xyz, int n, int stride,
                                                         const double *__restrict__ origin,
                                                         const float *__restrict__ boxes, int k, float grow_yx,
                                                         float grow_z, int32_t *__restrict__ owner,
                                                         int32_t *__restrict__ count, uint32_t *__restrict__ lo,
                                                         uint32_t *__restrict__ hi) {
  __shared__ BoxTile T;
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * kSpan;
  float px[kPointsPerLane], py[kPointsPerLane], pz[kPointsPerLane];
  int32_t own[kPointsPerLane];
  double o0 = 0.0, o1 = 0.0, o2 = 0.0;
  if (origin) o0 = origin[0], o1 = origin[1], o2 = origin[2];
#pragma unroll
  for (int j = 0; j < kPointsPerLane; j++) {
    const size_t i = base + (size_t)j * kThreads + tid;
    own[j] = -1;
    if (i < (size_t)n) {
      const float *p = xyz + i * (size_t)stride;
      px[j] = p[0], py[j] = p[1], pz[j] = p[2];
      if (origin) {
        px[j] = (float)((double)px[j] - o0);
        py[j] = (float)((double)py[j] - o1);
        pz[j] = (float)((double)pz[j] - o2);
      }
    } else {
      px[j] = py[j] = pz[j] = __builtin_nanf("");      // a member of nothing
    }
  }

  for (int t0 = 0; t0 < k; t0 += kTile) {
    const int nb = min(kTile, k - t0);
    if (tid < nb) {                                    // entry tid is this thread's alone between the two barriers below
      const float *b = boxes + (size_t)(t0 + tid) * 7;
      const double yaw = (double)b[6];
      T.xc[tid] = b[0], T.yc[tid] = b[1], T.zb[tid] = b[2];
      T.c[tid] = (float)cos(yaw), T.s[tid] = (float)sin(yaw);
      T.hx[tid] = fmaxf(b[3], grow_yx) * 0.5f;
      T.hy[tid] = fmaxf(b[4], grow_yx) * 0.5f;
      T.hz[tid] = fmaxf(b[5], grow_z);
      T.count[tid] = 0;
#pragma unroll
      for (int d = 0; d < 3; d++) T.lo[d][tid] = 0xFFFFFFFFu, T.hi[d][tid] = 0u;
    }
    __syncthreads();
    for (int bi = 0; bi < nb; bi++) {
      const float xc = T.xc[bi], yc = T.yc[bi], zb = T.zb[bi], c = T.c[bi], s = T.s[bi];
      const float hx = T.hx[bi], hy = T.hy[bi], hz = T.hz[bi];
      int hits = 0;
      float mn0 = __builtin_inff(), mn1 = mn0, mn2 = mn0, mx0 = -mn0, mx1 = mx0, mx2 = mx0;
#pragma unroll
      for (int j = 0; j < kPointsPerLane; j++) {
        const float dx = px[j] - xc, dy = py[j] - yc;
        const float lx = c * dx - s * dy, ly = s * dx + c * dy, lz = pz[j] - zb;
        const bool in = fabsf(lx) <= hx && fabsf(ly) <= hy && lz >= 0.f && lz <= hz;      // NaN: false
        if (in) {
          hits++;
          if (own[j] < 0) own[j] = t0 + bi;
          // + 0: a -0 becomes +0, so that the extents do not depend on how a zero came about
          mn0 = fminf(mn0, lx + 0.f), mx0 = fmaxf(mx0, lx + 0.f);
          mn1 = fminf(mn1, ly + 0.f), mx1 = fmaxf(mx1, ly + 0.f);
          mn2 = fminf(mn2, lz + 0.f), mx2 = fmaxf(mx2, lz + 0.f);
        }
      }
      if (__ballot(hits != 0) == 0ull) continue;       // wave-uniform
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        hits += __shfl_xor(hits, d, 64);
        mn0 = fminf(mn0, __shfl_xor(mn0, d, 64)), mx0 = fmaxf(mx0, __shfl_xor(mx0, d, 64));
        mn1 = fminf(mn1, __shfl_xor(mn1, d, 64)), mx1 = fmaxf(mx1, __shfl_xor(mx1, d, 64));
        mn2 = fminf(mn2, __shfl_xor(mn2, d, 64)), mx2 = fmaxf(mx2, __shfl_xor(mx2, d, 64));
      }
      if ((tid & 63) == 0) {
        atomicAdd(&T.count[bi], hits);
        atomicMin(&T.lo[0][bi], f32_ordered(mn0)), atomicMax(&T.hi[0][bi], f32_ordered(mx0));
        atomicMin(&T.lo[1][bi], f32_ordered(mn1)), atomicMax(&T.hi[1][bi], f32_ordered(mx1));
        atomicMin(&T.lo[2][bi], f32_ordered(mn2)), atomicMax(&T.hi[2][bi], f32_ordered(mx2));
      }
    }
    __syncthreads();
    if (tid < nb && T.count[tid] > 0) {
      const size_t g = (size_t)(t0 + tid);
      atomicAdd(count + g, T.count[tid]);
#pragma unroll
      for (int d = 0; d < 3; d++) {
        atomicMin(lo + g * 3 + d, T.lo[d][tid]);
        atomicMax(hi + g * 3 + d, T.hi[d][tid]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kPointsPerLane; j++) {
    const size_t i = base + (size_t)j * kThreads + tid;
    if (i < (size_t)n) owner[i] = own[j];
  }
}

}  // namespace
}  // namespace d3d

using namespace d3d;

int d3d_points_in_boxes(const float *xyz, int n, int row_stride_floats, const double *origin_dev, const float *boxes,
                        int k, float grow_yx, float grow_z, int32_t *owner, int32_t *count, float *lo, float *hi,
                        void *stream) {
  D3D_REQUIRE(n >= 0 && k >= 0, "d3d_points_in_boxes: n %d, k %d must not be negative", n, k);
  D3D_REQUIRE(k <= kMaxBoxes, "d3d_points_in_boxes: %d boxes, at most %d", k, kMaxBoxes);
  D3D_REQUIRE(row_stride_floats >= 3, "d3d_points_in_boxes: row stride %d < 3 floats", row_stride_floats);
  D3D_REQUIRE(grow_yx >= 0.f && grow_z >= 0.f, "d3d_points_in_boxes: grow (%g, %g) must not be negative",
              (double)grow_yx, (double)grow_z);
  D3D_REQUIRE(n == 0 || (xyz && owner), "d3d_points_in_boxes: null pointer (xyz, owner)");
  D3D_REQUIRE(k == 0 || (boxes && count && lo && hi), "d3d_points_in_boxes: null pointer (boxes, count, lo, hi)");
  hipStream_t s = (hipStream_t)stream;
  const dim3 per_box((unsigned)((3 * k + 255) / 256));
  uint32_t *lo_u = reinterpret_cast<uint32_t *>(lo), *hi_u = reinterpret_cast<uint32_t *>(hi);
  if (k > 0) hipLaunchKernelGGL(k_pib_begin, per_box, dim3(256), 0, s, k, count, lo_u, hi_u);
  if (n > 0)
    hipLaunchKernelGGL(k_pib_sweep, dim3((unsigned)(((size_t)n + kSpan - 1) / kSpan)), dim3(kThreads), 0, s, xyz, n,
                       row_stride_floats, origin_dev, boxes, k, grow_yx, grow_z, owner, count, lo_u, hi_u);
  if (k > 0) hipLaunchKernelGGL(k_pib_end, per_box, dim3(256), 0, s, k, lo_u, hi_u);
  if (n > 0 || k > 0) D3D_LAUNCH_CHECK();
  return D3D_OK;
}
