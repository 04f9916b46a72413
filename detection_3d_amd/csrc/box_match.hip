// The IoU matrix (rotate_iou_gpu_eval, boxes_iou_3d) and training label assignment on the geometry of box_geometry.inc.
#include "d3d_internal.h"

namespace d3d {

#include "box_geometry.inc"

// ------------------------------------------------------------------------------------------
// IoU matrix: 64 x 64 tile per 256-thread block; lane = column (coalesced stores).
__global__ __launch_bounds__(256) void k_iou_matrix(IouArgs a) {
  __shared__ BoxRec srow[64], scol[64];
  const int tid = threadIdx.x;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  if (tid < 64) {
    if (r0 + tid < a.N) load_box(a, a.rows, r0 + tid, true, srow[tid]);
  } else if (tid < 128) {
    const int t = tid - 64;
    if (c0 + t < a.K) load_box(a, a.cols, c0 + t, false, scol[t]);
  }
  __syncthreads();
  const int c = tid & 63, rg = tid >> 6;
  if (c0 + c >= a.K) return;
  const BoxRec &cb = scol[c];
  for (int i = 0; i < 16; i++) {
    const int rr = rg * 16 + i;
    if (r0 + rr >= a.N) break;
    a.out[(size_t)(r0 + rr) * a.K + c0 + c] = iou_pair(a, srow[rr], cb);
  }
}

// ------------------------------------------------------------------------------------------
// Label assignment of several segments (examples, or (example, class group) pairs) in one launch set: every prediction
// (anchor or proposal) is matched against the GT rows of ITS segment only.  IoU = iou_pair with GT as rows (the values
// of d3d_boxes_iou_3d), the Matcher of matcher.py:13-177 and box_encode (box_coder_3d.py:31-36) fused; no [M, N] matrix.
//   pass 1: thread = prediction; the GT rows of the block's segments are staged in LDS chunks; best value + argmax per
//           prediction, per-GT maxima (low-quality rule) as an order-preserving integer max (LDS, then one global
//           atomic per GT and block: integer max is exact and order-independent, so the result is deterministic)
//   pass 2 (low-quality rule only): the IoUs are evaluated again where they can decide (q == highest, q > ignore
//           threshold), cheaper than storing them: most pairs take the bounding-box early-out
static constexpr int kMatchThreads = 256, kMatchChunk = 256, kMatchMaxSeg = 256;
struct MatchArgs {
  IouArgs a;                  // mode 1: rows = GT [M, 7], cols = predictions [N, 7]
  const int32_t *pred_seg;
  int S, N, use_yaw, low_quality;
  float yaw_thr, high, low;
  float w[7];
  int32_t *matched;
  float *reg;
  float *best;
  int32_t *arg;
  unsigned *highest;          // f32_ordered_nan_top of the per-GT maxima: a NaN of either sign is the top value (q.max(1)
                              // is NaN if any quality of the row is), which ordered_to_f32 gives back as a NaN
  int off[kMatchMaxSeg + 1];  // GT rows of segment s: [off[s], off[s + 1])
};

// limit_period(v, offset, pi) as the tensor library evaluates it: v / pi is the product with the fp32 reciprocal
__device__ __forceinline__ float limit_period_pi(float v, float offset) {
  const float kPi = (float)3.14159265358979323846, kInvPi = 1.f / kPi;
  return v - floorf(v * kInvPi + offset) * kPi;
}

// Matcher's quality: IoU x (|limit_period(yaw_gt - yaw_pred)| < YAW_THRESHOLD) (matcher.py:50-55; a masked negative
// IoU becomes -0.0, as in the tensor form)
__device__ __forceinline__ float match_quality(const MatchArgs &m, const BoxRec &g, const BoxRec &p) {
  float v = iou_pair(m.a, g, p);
  if (m.use_yaw) {
    const float d = fabsf(limit_period_pi(g.raw[4] - p.raw[4], 0.5f));
    v = v * (d < m.yaw_thr ? 1.f : 0.f);
  }
  return v;
}

// BoxCoder3D.encode (smooth_dim), operation by operation as the tensor form (training.box_encode) evaluates it
__device__ __forceinline__ void box_encode_one(const float *g, const float *a, const float *w, float *o) {
  const float diag = sqrtf(a[4] * a[4] + a[3] * a[3]);
  float e[7];
  e[0] = (g[0] - a[0]) / diag;
  e[1] = (g[1] - a[1]) / diag;
  e[2] = (g[2] - a[2]) / a[5];
  e[3] = g[3] / a[3] - 1.f;
  e[4] = g[4] / a[4] - 1.f;
  e[5] = g[5] / a[5] - 1.f;
  e[6] = limit_period_pi(g[6] - a[6], 0.5f);
#pragma unroll
  for (int k = 0; k < 7; k++) o[k] = e[k] * w[k];
}

// matched[p] and the regression target of row gt[max(matched, first row of the segment)] (gt_boxes[matched.clamp(min=0)]);
// a segment without GT: -1 and zeros (the empty-GT branches of prepare_targets / subsample)
__device__ __forceinline__ void match_store(const MatchArgs &m, int p, int lo, int hi, int matched) {
  m.matched[p] = matched;
  if (!m.reg) return;
  float *o = m.reg + (size_t)p * 7;
  if (hi <= lo) {
#pragma unroll
    for (int k = 0; k < 7; k++) o[k] = 0.f;
    return;
  }
  box_encode_one(m.a.rows + (size_t)(matched >= 0 ? matched : lo) * 7, m.a.cols + (size_t)p * 7, m.w, o);
}

// below the low threshold -1, between -2, else the argmax (a NaN maximum is neither, as in the tensor form)
__device__ __forceinline__ int match_thresholds(const MatchArgs &m, float best, int arg) {
  if (best < m.low) return -1;
  if (best < m.high) return -2;
  return arg;
}

// the segment of row p (out-of-range ids: no GT) and the union of the GT ranges the block's rows need
__device__ __forceinline__ void match_rows(const MatchArgs &m, int p, bool want, int &lo, int &hi, int *s_range) {
  int seg = p < m.N ? m.pred_seg[p] : -1;
  if (seg < 0 || seg >= m.S) seg = -1;
  lo = seg >= 0 ? m.off[seg] : 0;
  hi = seg >= 0 ? m.off[seg + 1] : 0;
  if (threadIdx.x == 0) {
    s_range[0] = 0x7fffffff;
    s_range[1] = 0;
  }
  __syncthreads();
  if (want && hi > lo) {
    atomicMin(&s_range[0], lo);
    atomicMax(&s_range[1], hi);
  }
  __syncthreads();
}

__global__ __launch_bounds__(kMatchThreads) void k_match_pass1(MatchArgs m) {
  __shared__ BoxRec sg[kMatchChunk];
  __shared__ unsigned shi[kMatchChunk];
  __shared__ int s_range[2];
  const int tid = threadIdx.x, p = blockIdx.x * kMatchThreads + tid;
  int lo, hi;
  match_rows(m, p, true, lo, hi, s_range);
  const int blo = s_range[0], bhi = s_range[1];
  BoxRec pb;
  if (hi > lo) load_box(m.a, m.a.cols, p, false, pb);
  float best = 0.f;
  int arg = -1;
  for (int c0 = blo; c0 < bhi; c0 += kMatchChunk) {     // block-uniform loop
    const int cn = min(kMatchChunk, bhi - c0);
    if (tid < cn) {
      load_box(m.a, m.a.rows, c0 + tid, true, sg[tid]);
      shi[tid] = 0u;
    }
    __syncthreads();
    const int r1 = min(hi, c0 + cn);
    for (int r = max(lo, c0); r < r1; r++) {
      const float v = match_quality(m, sg[r - c0], pb);
      // q.max(dim=0): first maximum (lowest GT row); a NaN wins and stays
      if (arg < 0 || v > best || (v != v && best == best)) {
        best = v;
        arg = r;
      }
      if (m.low_quality) atomicMax(&shi[r - c0], f32_ordered_nan_top(v));
    }
    __syncthreads();
    if (m.low_quality && tid < cn && shi[tid] != 0u) atomicMax(&m.highest[c0 + tid], shi[tid]);
    __syncthreads();                                     // sg / shi are restaged by the next chunk
  }
  if (p >= m.N) return;
  if (m.low_quality) {
    m.best[p] = best;
    m.arg[p] = arg;
  } else {
    match_store(m, p, lo, hi, hi > lo ? match_thresholds(m, best, arg) : -1);
  }
}

// allow_low_quality_matches (matcher.py:105-177): every GT keeps its best prediction(s) (q == highest, ties included);
// predictions that would be negatives and have q > max(0.02, highest - 0.05) for some GT are ignored (-2)
__global__ __launch_bounds__(kMatchThreads) void k_match_pass2(MatchArgs m) {
  __shared__ BoxRec sg[kMatchChunk];
  __shared__ float shv[kMatchChunk], sthr[kMatchChunk];
  __shared__ int s_range[2];
  const int tid = threadIdx.x, p = blockIdx.x * kMatchThreads + tid;
  const float best = p < m.N ? m.best[p] : 0.f;
  const int arg = p < m.N ? m.arg[p] : -1;
  // best >= high (or NaN): restoring gives the argmax back and the ignore rule needs -1 -> nothing can change
  const bool need = p < m.N && arg >= 0 && best < m.high;
  int lo, hi;
  match_rows(m, p, need, lo, hi, s_range);
  const int blo = s_range[0], bhi = s_range[1];
  BoxRec pb;
  if (need) load_box(m.a, m.a.cols, p, false, pb);
  bool restore = false, ignore = false;
  for (int c0 = blo; c0 < bhi; c0 += kMatchChunk) {
    const int cn = min(kMatchChunk, bhi - c0);
    if (tid < cn) {
      load_box(m.a, m.a.rows, c0 + tid, true, sg[tid]);
      const float h = ordered_to_f32(m.highest[c0 + tid]);
      const float t = h - 0.05f;
      shv[tid] = h;
      sthr[tid] = t != t ? t : fmaxf(0.02f, t);          // torch.max(0.02, highest - 0.05): a NaN propagates
    }
    __syncthreads();
    if (need) {
      const int r1 = min(hi, c0 + cn);
      for (int r = max(lo, c0); r < r1; r++) {
        const float h = shv[r - c0], t = sthr[r - c0];
        // q <= best: below min(highest, threshold) the pair decides nothing (a NaN highest never matches)
        if (h != h || best < fminf(h, t)) continue;
        const float q = match_quality(m, sg[r - c0], pb);
        restore = restore || q == h;
        ignore = ignore || q > t;
      }
    }
    __syncthreads();
  }
  if (p >= m.N) return;
  if (arg < 0) {          // no GT in the segment
    match_store(m, p, lo, hi, -1);
    return;
  }
  int mt = match_thresholds(m, best, arg);
  if (restore) mt = arg;
  if (ignore && mt == -1) mt = -2;
  match_store(m, p, lo, hi, mt);
}

namespace {

struct Layout {
  float *best;          // [N] pass 1's maximum per prediction
  int32_t *arg;         // [N] ... and its GT row
  unsigned *highest;    // [M] per-GT maxima
};

int carve(Arena &A, int M, int N, Layout &L) {
  D3D_ALLOC(best, float, A, N);
  D3D_ALLOC(arg, int32_t, A, N);
  D3D_ALLOC(highest, unsigned, A, M);
  L = Layout{best, arg, highest};
  return D3D_OK;
}

}  // namespace
}  // namespace d3d

using namespace d3d;

extern "C" {

int d3d_rotate_iou_eval(const float *boxes, int N, const float *query, int K, int criterion,
                        float *out, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(N >= 0 && K >= 0, "rotate_iou_eval: negative size");
  if (N == 0 || K == 0) return D3D_OK;
  D3D_REQUIRE(boxes && query && out, "rotate_iou_eval: null pointer");
  IouArgs a;
  a.rows = boxes; a.cols = query; a.N = N; a.K = K; a.mode = 0; a.criterion = criterion; a.only_xy = 1;
  a.aug[0] = a.aug[1] = a.aug[2] = a.aug[3] = 0.f;
  a.out = out;
  hipLaunchKernelGGL(k_iou_matrix, dim3((K + 63) / 64, (N + 63) / 64), dim3(256), 0, s, a);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

int d3d_boxes_iou_3d(const float *targets, int M, const float *anchors, int N, const float *aug_host,
                     int criterion, int only_xy, float *out, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(M >= 0 && N >= 0, "boxes_iou_3d: negative size");
  if (M == 0 || N == 0) return D3D_OK;
  D3D_REQUIRE(targets && anchors && out, "boxes_iou_3d: null pointer");
  IouArgs a;
  a.rows = targets; a.cols = anchors; a.N = M; a.K = N; a.mode = 1; a.criterion = criterion; a.only_xy = only_xy;
  for (int i = 0; i < 4; i++) a.aug[i] = aug_host ? aug_host[i] : 0.f;
  a.out = out;
  hipLaunchKernelGGL(k_iou_matrix, dim3((N + 63) / 64, (M + 63) / 64), dim3(256), 0, s, a);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

size_t d3d_match_segments_scratch_bytes(int M, int N) {
  Arena A = sizing_arena();
  Layout L;
  (void)carve(A, M > 0 ? M : 0, N > 0 ? N : 0, L);
  return A.used ? A.used : 256;   // never 0: a caller may allocate it as it is
}

int d3d_match_segments(const float *gt, const int *gt_off_host, int S, const float *pred, int N, const int32_t *pred_seg,
                       const float *aug_host, int criterion, float yaw_threshold, float high, float low,
                       int allow_low_quality, const float *encode_weights_host, int32_t *matched, float *reg_targets,
                       void *scratch, size_t scratch_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(N >= 0 && S >= 0 && S <= kMatchMaxSeg, "match_segments: N=%d or S=%d out of range (S <= %d)", N, S,
              kMatchMaxSeg);
  D3D_REQUIRE(S == 0 || gt_off_host, "match_segments: null GT offsets");
  D3D_REQUIRE(S == 0 || gt_off_host[0] == 0, "match_segments: GT offsets must start at 0");
  for (int i = 0; i < S; i++)
    D3D_REQUIRE(gt_off_host[i + 1] >= gt_off_host[i], "match_segments: GT offsets decrease at segment %d", i);
  const int M = S ? gt_off_host[S] : 0;
  D3D_REQUIRE(criterion >= -1 && criterion <= 2, "match_segments: criterion %d", criterion);
  D3D_REQUIRE(low <= high, "match_segments: low threshold above the high one");
  if (N == 0) return D3D_OK;
  D3D_REQUIRE(pred && pred_seg && matched && (M == 0 || gt), "match_segments: null pointer");
  D3D_REQUIRE(scratch && scratch_bytes >= d3d_match_segments_scratch_bytes(M, N), "match_segments: scratch too small");
  Arena A = scratch_arena(scratch, scratch_bytes);
  Layout L;
  const int rc = carve(A, M, N, L);
  if (rc) return rc;
  MatchArgs m;
  m.a.rows = gt; m.a.cols = pred; m.a.N = M; m.a.K = N; m.a.mode = 1; m.a.criterion = criterion; m.a.only_xy = 0;
  for (int i = 0; i < 4; i++) m.a.aug[i] = aug_host ? aug_host[i] : 0.f;
  m.a.out = nullptr;
  m.pred_seg = pred_seg;
  m.S = S; m.N = N;
  m.use_yaw = !(yaw_threshold > 1.58f);
  m.low_quality = allow_low_quality ? 1 : 0;
  m.yaw_thr = yaw_threshold; m.high = high; m.low = low;
  for (int k = 0; k < 7; k++) m.w[k] = encode_weights_host ? encode_weights_host[k] : 1.f;
  m.matched = matched; m.reg = reg_targets;
  m.best = L.best; m.arg = L.arg; m.highest = L.highest;
  for (int i = 0; i <= kMatchMaxSeg; i++) m.off[i] = i <= S ? gt_off_host[i] : M;
  const dim3 grid((N + kMatchThreads - 1) / kMatchThreads);
  if (m.low_quality && M > 0) D3D_HIP_CHECK(hipMemsetAsync(m.highest, 0, (size_t)M * 4, s));   // below every value
  hipLaunchKernelGGL(k_match_pass1, grid, dim3(kMatchThreads), 0, s, m);
  if (m.low_quality) hipLaunchKernelGGL(k_match_pass2, grid, dim3(kMatchThreads), 0, s, m);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

}  // extern "C"
