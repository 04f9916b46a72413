// a14. The inference tail around the NMS: box decode, the RPN's survivor gather and the box head's post-processing.
#include "d3d_internal.h"

namespace d3d {

// a14. BoxCoder3D.decode
__global__ void k_box_decode(const float *__restrict__ enc, const float *__restrict__ anchors, int n,
                             float w0, float w1, float w2, float w3, float w4, float w5, float w6,
                             float clip, float *__restrict__ out, const int64_t *__restrict__ rows, int nc) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t src = rows ? (size_t)rows[i] : (size_t)i;   // rows: the top-k selection, gathered here
  // nc > 1: enc holds nc class-wise encodings per anchor row (box_coder_3d.py decode of [n, 7 nc])
  const float *e = enc + src * 7, *a = anchors + (src / (size_t)nc) * 7;
  const float w[7] = {w0, w1, w2, w3, w4, w5, w6};
  box_decode_one(e, a, w, clip, out + (size_t)i * 7);
}

// survivors of the RPN's NMS into a list padded to P rows: out row i < *n_keep is box / score keep[i] with its sizes
// clamped from below (BoxList3D.clamp_size), the other rows repeat row 0 of the candidates (never pooled)
__global__ void k_gather_kept(const float *__restrict__ boxes, const float *__restrict__ scores,
                              const int32_t *__restrict__ keep, const int32_t *__restrict__ n_keep, int P,
                              float min_size, float *__restrict__ out_boxes, float *__restrict__ out_scores,
                              int32_t *__restrict__ count_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  // the count, for the host: a store to pinned host memory that an event recorded behind this launch makes visible --
  // no copy engine and no second stream between the NMS and the host
  if (i == 0 && count_out) __hip_atomic_store(count_out, *n_keep, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  if (i >= P) return;
  const int j = i < *n_keep ? keep[i] : 0;
  const float *b = boxes + (size_t)j * 7;
  float *o = out_boxes + (size_t)i * 7;
#pragma unroll
  for (int k = 0; k < 7; k++) {
    float v = b[k];
    if (k >= 3 && k < 6) v = v < min_size ? min_size : v;   // torch.clamp(min=): a NaN stays
    o[k] = v;
  }
  out_scores[i] = scores[j];
}

}  // namespace d3d

using namespace d3d;

extern "C" {

// ---- box-head post-processing glue (inference.py:113-148), three launches instead of ~20 tensor ops ----
// masked class scores, class-major: sc[j][i] = prob[i][j+1] if > thresh else -1; counts[j] = candidates of class j+1
__global__ __launch_bounds__(256) void k_post_scores(const float *__restrict__ prob, int K, int nc, float thresh,
                                                     float *__restrict__ sc, int32_t *__restrict__ counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  bool c = false;
  if (i < K) {
    const float v = prob[(size_t)i * nc + j + 1];
    c = v > thresh;
    sc[(size_t)j * K + i] = c ? v : -1.f;
  }
  const unsigned long long bal = __ballot(c);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(counts + j, __popcll(bal));
}
// order[j][i] = box index (RoI idx[j][i], class j+1) in the [K, nc] layout of the decoded boxes
__global__ __launch_bounds__(256) void k_post_order(const int64_t *__restrict__ idx, int K, int nc, int nseg,
                                                    int32_t *__restrict__ order) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)nseg * K) return;
  order[t] = (int32_t)(idx[t] * nc + (int64_t)(t / K) + 1);
}
// survivors of the batched NMS, class-major in selection order: flat box index + score, padding = (0, -1)
__global__ __launch_bounds__(256) void k_post_gather(const int32_t *__restrict__ keep, const int32_t *__restrict__ nk,
                                                     int nseg, int n_max, const float *__restrict__ prob_flat,
                                                     float *__restrict__ s_all, int64_t *__restrict__ flat_all) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nseg * n_max) return;
  const bool valid = (t % n_max) < nk[t / n_max];
  const int f = valid ? keep[t] : 0;
  flat_all[t] = f;
  s_all[t] = valid ? prob_flat[f] : -1.f;
}

// The cut to detections_per_img and the final gathers of inference.py:140-148 in ONE single-workgroup launch (what
// followed d3d_post_gather as ~12 tensor-library launches: top-k, compare, nonzero, three index ops, remainder).
// Candidates t = 0 .. segments * n_max - 1 (class-major, selection order): score s[t] = prob_flat[keep[t]] for
// t % n_max < n_keep[t / n_max], else -1.  thresh = the D-th largest s (D > 0 and D < #candidates; a padding -1 when
// fewer than D survive) clamped to >= 0; the selected set is { t : s[t] >= thresh } IN t ORDER -- like the reference's
// `keep = cls_scores >= image_thresh`, ties at the threshold all stay.  For every selected t: the box, the score and
// the label (box index % nc).  The D-th largest is found by a 4 x 8-bit radix select on the order-preserving integer
// image of the floats (exact), the compaction by a workgroup scan.
// The keys follow the tensor spelling of the same cut (torch.sort, clamp_min(0), >=) on every float: -0.0 ranks and
// compares as 0.0 (it stays), a NaN of either sign ranks above +inf and is never selected, and when the D-th largest is a
// NaN nothing is (`s >= NaN`).
static constexpr int kSelMax = 8192, kSelThreads = 1024;
static constexpr uint32_t kSelNanKey = 0xffffffffu;   // f32_ordered_nan_top of a NaN
__device__ __forceinline__ uint32_t post_key(float v) { return f32_ordered_nan_top(v + 0.f); }
__global__ __launch_bounds__(kSelThreads) void k_post_select(const int32_t *__restrict__ keep,
                                                             const int32_t *__restrict__ nk, int nseg, int n_max,
                                                             const float *__restrict__ prob_flat,
                                                             const float *__restrict__ boxes, int nc, int D,
                                                             float *__restrict__ out_boxes, float *__restrict__ out_scores,
                                                             int64_t *__restrict__ out_labels, int32_t *__restrict__ out_n) {
  __shared__ uint32_t key[kSelMax];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t wsum[kSelThreads / 64];
  __shared__ uint32_t sel_prefix, sel_rank;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = nseg * n_max;
  for (int t = tid; t < N; t += kSelThreads) {
    const bool valid = (t % n_max) < nk[t / n_max];
    key[t] = post_key(valid ? prob_flat[keep[t]] : -1.f);
  }
  uint32_t thresh_key = f32_ordered(0.f);     // s >= 0: every survivor
  if (D > 0 && D < N) {
    // radix select of the D-th largest key: fix 8 bits per pass, most significant first
    uint32_t prefix = 0, want = (uint32_t)D;   // `want`-th largest among the keys that match `prefix` on the fixed bits
    for (int pass = 0; pass < 4; pass++) {
      const int shift = 24 - 8 * pass;
      const uint32_t fixed_mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for (int t = tid; t < N; t += kSelThreads) {
        const uint32_t k = key[t];
        if ((k & fixed_mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        uint32_t acc = 0;
        int b = 255;
        for (; b > 0; b--) {
          if (acc + hist[b] >= want) break;
          acc += hist[b];
        }
        sel_prefix = prefix | ((uint32_t)b << shift);
        sel_rank = want - acc;
      }
      __syncthreads();
      prefix = sel_prefix;
      want = sel_rank;
      __syncthreads();
    }
    thresh_key = max(prefix, thresh_key);      // thresh.clamp_min(0)
  }
  __syncthreads();
  // ordered compaction: thread t owns the contiguous candidates [per * t, per * t + per)
  const int per = (N + kSelThreads - 1) / kSelThreads;
  const int t0 = min(N, tid * per), t1 = min(N, t0 + per);
  uint32_t mine = 0;
  for (int t = t0; t < t1; t++) mine += key[t] >= thresh_key && key[t] != kSelNanKey;
  uint32_t incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t pos = incl - mine;
  for (int w = 0; w < wave; w++) pos += wsum[w];
  if (tid == kSelThreads - 1)   // out_n may be a pinned host word: system-scope release, like k_gather_kept's count
    __hip_atomic_store(out_n, (int32_t)(pos + mine), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  for (int t = t0; t < t1; t++) {
    if (key[t] < thresh_key || key[t] == kSelNanKey) continue;
    const int f = keep[t];
#pragma unroll
    for (int j = 0; j < 7; j++) out_boxes[(size_t)pos * 7 + j] = boxes[(size_t)f * 7 + j];
    out_scores[pos] = prob_flat[f];
    out_labels[pos] = (int64_t)(f % nc);
    pos++;
  }
}

int d3d_post_scores(const float *prob, int K, int nc, float thresh, float *sc, int32_t *counts, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(K >= 0 && nc >= 2, "post_scores: bad shape");
  D3D_REQUIRE(counts, "post_scores: null pointer");
  D3D_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int32_t) * (nc - 1), s));
  if (K == 0) return D3D_OK;
  D3D_REQUIRE(prob && sc, "post_scores: null pointer");
  hipLaunchKernelGGL(k_post_scores, dim3((K + 255) / 256, nc - 1), dim3(256), 0, s, prob, K, nc, thresh, sc, counts);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}
int d3d_post_order(const int64_t *idx, int K, int nc, int32_t *order, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(K >= 0 && nc >= 2, "post_order: bad shape");
  if (K == 0) return D3D_OK;
  D3D_REQUIRE(idx && order, "post_order: null pointer");
  const long total = (long)(nc - 1) * K;
  hipLaunchKernelGGL(k_post_order, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, idx, K, nc, nc - 1, order);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}
int d3d_post_gather(const int32_t *keep, const int32_t *n_keep, int segments, int n_max, const float *prob_flat,
                    float *scores, int64_t *flat, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(segments >= 0 && n_max >= 0, "post_gather: bad shape");
  if (segments == 0 || n_max == 0) return D3D_OK;
  D3D_REQUIRE(keep && n_keep && prob_flat && scores && flat, "post_gather: null pointer");
  hipLaunchKernelGGL(k_post_gather, dim3((segments * n_max + 255) / 256), dim3(256), 0, s, keep, n_keep, segments, n_max,
                     prob_flat, scores, flat);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

int d3d_post_select_max(void) { return kSelMax; }
int d3d_post_select(const int32_t *keep, const int32_t *n_keep, int segments, int n_max, const float *prob_flat,
                    const float *boxes, int nc, int detections, float *out_boxes, float *out_scores, int64_t *out_labels,
                    int32_t *out_n, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(segments >= 0 && n_max >= 0 && nc >= 1 && out_n, "post_select: bad arguments");
  const long N = (long)segments * n_max;
  D3D_REQUIRE(N <= kSelMax, "post_select: %ld candidates exceed the %d of the single-workgroup selection", N, kSelMax);
  if (N == 0) {
    D3D_HIP_CHECK(hipMemsetAsync(out_n, 0, sizeof(int32_t), s));
    return D3D_OK;
  }
  D3D_REQUIRE(keep && n_keep && prob_flat && boxes && out_boxes && out_scores && out_labels, "post_select: null pointer");
  hipLaunchKernelGGL(k_post_select, dim3(1), dim3(kSelThreads), 0, s, keep, n_keep, segments, n_max, prob_flat, boxes, nc,
                     detections, out_boxes, out_scores, out_labels, out_n);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

int d3d_box_decode(const float *enc, const float *anchors, int n, const float *weights_host,
                   float clip, float *out, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return D3D_OK;
  D3D_REQUIRE(enc && anchors && out && weights_host && n > 0, "box_decode: bad arguments");
  const float *w = weights_host;
  hipLaunchKernelGGL(k_box_decode, dim3((n + 255) / 256), dim3(256), 0, s, enc, anchors, n, w[0], w[1], w[2], w[3], w[4], w[5], w[6], clip, out,
                     (const int64_t *)nullptr, 1);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

int d3d_box_decode_rows(const float *enc, const float *anchors, const int64_t *rows, int n, const float *weights_host,
                        float clip, float *out, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return D3D_OK;
  D3D_REQUIRE(enc && anchors && rows && out && weights_host && n > 0, "box_decode_rows: bad arguments");
  const float *w = weights_host;
  hipLaunchKernelGGL(k_box_decode, dim3((n + 255) / 256), dim3(256), 0, s, enc, anchors, n, w[0], w[1], w[2], w[3], w[4], w[5], w[6], clip, out,
                     rows, 1);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

int d3d_box_decode_classes(const float *enc, const float *anchors, int n, int nc, const float *weights_host, float clip,
                           float *out, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return D3D_OK;
  D3D_REQUIRE(enc && anchors && out && weights_host && n > 0 && nc >= 1, "box_decode_classes: bad arguments");
  const float *w = weights_host;
  const long total = (long)n * nc;
  D3D_REQUIRE(total < (1L << 31), "box_decode_classes: %ld boxes", total);
  hipLaunchKernelGGL(k_box_decode, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, enc, anchors, (int)total, w[0], w[1], w[2], w[3],
                     w[4], w[5], w[6], clip, out, (const int64_t *)nullptr, nc);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

int d3d_gather_kept(const float *boxes, const float *scores, const int32_t *keep, const int32_t *n_keep_dev, int P,
                    float min_size, float *out_boxes, float *out_scores, int32_t *count_out, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (P == 0) return D3D_OK;
  D3D_REQUIRE(boxes && scores && keep && n_keep_dev && out_boxes && out_scores && P > 0, "gather_kept: bad arguments");
  hipLaunchKernelGGL(k_gather_kept, dim3((P + 255) / 256), dim3(256), 0, s, boxes, scores, keep, n_keep_dev, P, min_size,
                     out_boxes, out_scores, count_out);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

}  // extern "C"
