// a15-a18. Greedy rotated NMS on the geometry of box_geometry.inc -- all on device.
// The reference bounces GPU -> numpy -> numba-CUDA -> numpy -> spconv C++ -> GPU
// (utils3d/rotate_nms_3d_torch.py:64-83, second/core/non_max_suppression/nms_cpu.py:35-43).
#include "d3d_internal.h"

#include <algorithm>
#include <cstdlib>

namespace d3d {

#include "box_geometry.inc"

// ------------------------------------------------------------------------------------------
// NMS suppression masks: one wave per 64 x 64 tile; lanes = candidate boxes j; __ballot packs the
// 64 decisions "i suppresses j" of row i into one 64-bit word (wave64).
struct NmsBox {
  Quad q;
  float d0, d1, z0, z1, raw[5];
  float radius;  // BEV circumscribed circle, for the exact far-apart early-out
  double area;
};

// Conservative separating-axis test of two quads (rectangles): true only if they are separated by
// more than `margin` along one of the 4 edge directions -> they cannot touch, intersection area 0.
__device__ __forceinline__ bool quads_separated(const float *a, const float *b, float margin) {
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const float *p = q ? b : a;
#pragma unroll
    for (int e = 0; e < 2; e++) {
      float nx = p[2 * e + 3] - p[2 * e + 1], ny = -(p[2 * e + 2] - p[2 * e]);  // normal of edge e
      const float len = sqrtf(nx * nx + ny * ny);
      if (!(len > 0.f)) continue;
      nx /= len;
      ny /= len;
      float amin = 1e30f, amax = -1e30f, bmin = 1e30f, bmax = -1e30f;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const float pa = a[2 * i] * nx + a[2 * i + 1] * ny, pb = b[2 * i] * nx + b[2 * i + 1] * ny;
        amin = fminf(amin, pa); amax = fmaxf(amax, pa);
        bmin = fminf(bmin, pb); bmax = fmaxf(bmax, pb);
      }
      if (amin > bmax + margin || bmin > amax + margin) return true;
    }
  }
  return false;
}
// A batch of independent candidate lists ("segments", e.g. the classes of the box head): candidate i of
// segment b is box order[b*stride + i] (b*stride + i without `order`), i < counts[b] (n_max without `counts`),
// already in descending score order.
struct NmsSegs {
  const int32_t *order;
  const int32_t *counts;
  int stride, n_max;
};
__device__ __forceinline__ int seg_count(const NmsSegs &g, int b) { return g.counts ? min(g.counts[b], g.n_max) : g.n_max; }
__device__ __forceinline__ int seg_box(const NmsSegs &g, int b, int i) {
  return g.order ? g.order[(size_t)b * g.stride + i] : b * g.stride + i;
}
// min_yx / min_z: the NMS_AUG_THICKNESS clamp of boxlist_nms_3d (dy, dx >= min_yx, dz >= min_z, IoU only)
__global__ void k_nms_prep(const float *__restrict__ boxes, NmsSegs g, float min_yx, float min_z,
                           NmsBox *__restrict__ rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, sb = blockIdx.y;
  if (i >= seg_count(g, sb)) return;
  const float *b = boxes + (size_t)seg_box(g, sb, i) * 7;
  // torch.clamp(min=) of boxlist_nms_3d: a NaN size stays NaN (fmaxf would replace it by the bound)
  const float d0 = b[3] < min_yx ? min_yx : b[3], d1 = b[4] < min_yx ? min_yx : b[4], dz = b[5] < min_z ? min_z : b[5];
  NmsBox r;
  r.d0 = d0; r.d1 = d1;
  r.z0 = b[2]; r.z1 = b[2] + dz;
  r.raw[0] = b[0]; r.raw[1] = b[1]; r.raw[2] = d0; r.raw[3] = d1; r.raw[4] = b[6];
  r.q = make_quad(b[0], b[1], d0, d1, b[6]);
  r.radius = 0.5f * sqrtf(d0 * d0 + d1 * d1);
  r.area = quad_area_f64(r.q.p);
  rec[(size_t)sb * g.n_max + i] = r;
}
// overlap of the z intervals as iou_one_dim's torch.min / torch.max give it (rotate_nms_3d_torch.py:18): a NaN bound makes it
// NaN (fminf / fmaxf would drop the NaN).  z0 = NaN or dz = NaN both leave z1 = NaN, so testing z1 covers the box.
__device__ __forceinline__ float nms_z_overlap(const NmsBox &cb, const NmsBox &rb) {
  const float overlap = fminf(cb.z1, rb.z1) - fmaxf(cb.z0, rb.z0);
  return (cb.z1 != cb.z1 || rb.z1 != rb.z1) ? __builtin_nanf("") : overlap;
}
// Suppression masks in two passes so that the expensive geometry runs with full lanes:
//  k_nms_pairs  -- 256 threads per 64 x 64 tile (wave w: rows 16w..16w+15, lanes = candidate boxes j):
//                  cheap exact early-outs, survivors appended to a pair list (wave64 ballot + one atomic
//                  per wave).  The early-outs cannot change the decision:
//                   * z intervals do not overlap and their hull is finite and not a point -> iou_z = overlap / common
//                     <= 0 -> the gate skips the pair.  A NaN iou_z (a NaN bound, 0 / 0 of two equal point intervals,
//                     inf / inf) is NOT skipped: the gate of spconv's rotate_non_max_suppression_cpu is
//                     `iou3d <= 0 -> skip`, which a NaN passes -- k_nms_eval then decides on the polygon alone;
//                   * BEV circumscribed circles disjoint, or rectangles separated along an edge normal (margin
//                     ~1e-3 of the box size, far above fp32 rounding of metre-sized boxes) -> no corner inside
//                     the other box, no edges cross -> area 0 -> gate false.
//  k_nms_eval   -- one thread per listed pair: gate (fp32 IoU of nms_gpu.py x z IoU) and fp64 polygon IoU
//                  >= thresh; sets bit j of word [i][j/64] (atomicOr, order independent).
static constexpr int kNmsIdxBits = 12;  // candidates per segment <= 4096
__global__ __launch_bounds__(256) void k_nms_pairs(const NmsBox *__restrict__ rec, NmsSegs g, int2 *__restrict__ pairs,
                                                   unsigned int *__restrict__ n_pairs) {
  const int rt = blockIdx.y, ct = blockIdx.x, sb = blockIdx.z;
  const int n = seg_count(g, sb);
  if (ct < rt || ct * 64 >= n) return;
  rec += (size_t)sb * g.n_max;
  __shared__ NmsBox srow[64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < 64 && rt * 64 + threadIdx.x < n) srow[threadIdx.x] = rec[rt * 64 + threadIdx.x];
  const int j = ct * 64 + lane;
  NmsBox cb;
  if (j < n) cb = rec[j];
  __syncthreads();
  const int nrow = min(64, n - rt * 64);
  // the wave's 16 rows first (ballots stay in registers), then ONE counter atomic per wave: the pair counter is
  // a single address, and one atomic per (wave, row) serialises the whole grid on it
  unsigned long long bal[16];
  unsigned int total = 0;
#pragma unroll
  for (int u = 0; u < 16; u++) {
    const int ii = wave * 16 + u;
    const int i = rt * 64 + ii;
    bool cand = false;
    if (ii < nrow && j < n && j > i) {
      const NmsBox &rb = srow[ii];
      const float overlap = nms_z_overlap(cb, rb);
      const float common = fmaxf(cb.z1, rb.z1) - fminf(cb.z0, rb.z0);
      const bool z_apart = overlap <= 0.f && common > 0.f && common < __builtin_inff();   // -> iou_z <= 0, whatever it rounds to
      const float dx = cb.raw[0] - rb.raw[0], dy = cb.raw[1] - rb.raw[1];
      const float rr = (cb.radius + rb.radius) * 1.001f + 1e-4f;
      cand = !z_apart && dx * dx + dy * dy <= rr * rr &&
             !quads_separated(rb.q.p, cb.q.p, 1e-3f * (1.f + cb.radius + rb.radius));
    }
    bal[u] = __ballot(cand);
    total += (unsigned int)__popcll(bal[u]);
  }
  if (total == 0) return;
  unsigned int base = 0;
  if (lane == 0) base = atomicAdd(n_pairs, total);
  base = __shfl(base, 0, 64);
  const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
  for (int u = 0; u < 16; u++) {
    if ((bal[u] >> lane) & 1ull)
      pairs[base + __popcll(bal[u] & lt)] = make_int2((sb << kNmsIdxBits) | (rt * 64 + wave * 16 + u), j);
    base += (unsigned int)__popcll(bal[u]);
  }
}
static constexpr int kEvalThreads = 128;   // x 32 doubles of LDS per thread (the clip's two vertex lists) = 32 KB
__global__ __launch_bounds__(kEvalThreads) void k_nms_eval(const NmsBox *__restrict__ rec, const int2 *__restrict__ pairs,
                                                           const unsigned int *__restrict__ n_pairs, int n_max, int ncb,
                                                           float thresh, unsigned long long *__restrict__ mask) {
  // one column per lane, in a region per WAVE: the fp32 gate's point list (72 floats), then the fp64 clip's two vertex
  // lists (32 doubles) reuse it.  The two layouts overlap in memory, which is safe only inside a wave (its lanes run
  // the gate of a pair together, then some of them the clip); another wave may be in the other phase.
  constexpr int kColBytes = kLdsPtsFloats * 4 > 256 ? kLdsPtsFloats * 4 : 256;
  __shared__ __attribute__((aligned(16))) char sm[kEvalThreads * kColBytes];
  char *region = sm + (threadIdx.x >> 6) * (64 * kColBytes);
  const int lane = threadIdx.x & 63;
  double *clip = reinterpret_cast<double *>(region) + lane;
  const LdsPts pts = {reinterpret_cast<float *>(region) + lane, 64};
  const unsigned int total = *n_pairs;
  for (unsigned int p = blockIdx.x * blockDim.x + threadIdx.x; p < total; p += gridDim.x * blockDim.x) {
    int2 ij = pairs[p];
    const size_t seg0 = (size_t)(ij.x >> kNmsIdxBits) * n_max;  // first record / mask row of the segment
    ij.x &= (1 << kNmsIdxBits) - 1;
    const NmsBox rb = rec[seg0 + ij.x], cb = rec[seg0 + ij.y];
    // gate = boxes_iou_3d(dets, dets)[i, j] > 0 (nms_cpu.py:35, spconv nms.h)
    float v = iou_eval(cb.q, cb.d0, cb.d1, rb.q, rb.d0, rb.d1, -1, pts);
    bool same = true;
#pragma unroll
    for (int d = 0; d < 5; d++) same = same && (fabsf(rb.raw[d] - cb.raw[d]) < (float)1e-6);
    if (same) v = 1.f;
    const float overlap = nms_z_overlap(cb, rb);
    const float common = fmaxf(cb.z1, rb.z1) - fminf(cb.z0, rb.z0);
    v = v * (overlap / common);
    if (v <= 0.0f) continue;   // a NaN gate goes on to the polygon test, as in the reference
    const double ia = quad_inter_f64(rb.q.p, cb.q.p, clip, 64);
    if (!(ia > 0)) continue;
    const double ua = rb.area + cb.area - ia;
    if (ua > 0 && ia / ua >= (double)thresh) {
      atomicOr(&mask[(seg0 + ij.x) * ncb + (ij.y >> 6)], 1ull << (ij.y & 63));
      // inside a 64-box chunk also the mirrored bit: a row's diagonal word then lists the EARLIER boxes of the chunk that
      // suppress it too, which lets the sweep resolve a chunk by fixed-point iteration over all lanes (k_nms_sweep_lds)
      if ((ij.x >> 6) == (ij.y >> 6)) atomicOr(&mask[(seg0 + ij.y) * ncb + (ij.x >> 6)], 1ull << (ij.x & 63));
    }
  }
}
// Greedy sweep by ONE wave: lane w owns word w of the "removed" bit vector.  Per 64-box chunk the
// intra-chunk chain is resolved on the diagonal words with v_readlane; the chunk's 64 mask rows are
// loaded unconditionally in one batch (independent loads) and OR-ed in for the kept boxes; the next
// chunk's diagonal word is fetched one chunk ahead.
__global__ __launch_bounds__(64) void k_nms_sweep(const unsigned long long *__restrict__ mask, NmsSegs g, int ncb,
                                                  int max_keep, int32_t *__restrict__ keep,
                                                  int32_t *__restrict__ n_keep) {
  const int lane = threadIdx.x, sb = blockIdx.x;
  const int n = __builtin_amdgcn_readfirstlane(seg_count(g, sb));  // wave-uniform: keep it (and all row pointers) in SGPRs
  mask += (size_t)sb * g.n_max * ncb;  // rows of ncb words; this segment uses the first ceil(n/64)
  keep += (size_t)sb * g.n_max;
  n_keep += sb;
  const int ncw = (n + 63) / 64;
  const unsigned long long lt = (1ull << lane) - 1ull;
  unsigned long long removed = 0;  // word `lane`
  int cnt = 0;
  // rows of chunk c, word `lane`.  Unconditional loads from a wave-uniform row pointer + the lane's word offset
  // (lanes past the row end re-read its last word, rows past the chunk end re-read its last row): neither is ever
  // used -- words left of the diagonal / beyond ncw are not read again, kept has no bit for a missing row -- and
  // the loads stay free of per-lane predication and 64-bit vector address arithmetic (the sweep is one wave:
  // every instruction is on the critical path)
  const unsigned int lane_off = (unsigned int)min(lane, max(ncb - 1, 0)) * 8u;  // byte offset of this lane's word
  auto load_rows = [&](int c, unsigned long long *w) {
    if (c >= ncw) return;
    const int base = c * 64;
    const int nrow = min(64, n - base);
    const unsigned long long *rowp = mask + (size_t)base * ncb;
#pragma unroll
    for (int b = 0; b < 64; b++) {
      const char *rp = (const char *)(rowp + (size_t)min(b, nrow - 1) * ncb);  // wave-uniform (SGPR pair)
      w[b] = *(const unsigned long long *)(rp + lane_off);
    }
  };
  auto load_diag = [&](int c) -> unsigned long long {
    const int base = c * 64;
    return (c < ncw && lane < min(64, n - base)) ? mask[(size_t)(base + lane) * ncb + c] : 0ull;
  };
  // one chunk: `w` holds its rows, `diag` its diagonal word; the rows of the chunk AFTER NEXT and the next diagonal
  // are requested before the dependent chain, so that a batch of 64 row loads has two chains to arrive under (one
  // chain is shorter than the batch's latency; the wave is alone on its SIMD and may use all 512 VGPRs)
  auto step = [&](int c, const unsigned long long *w, unsigned long long *w_fill, unsigned long long &diag) {
    const int base = c * 64;
    const int nrow = min(64, n - base);
    load_rows(c + 2, w_fill);
    const unsigned long long diag_next = load_diag(c + 1);
    // (requested before the chain: read through `order`, it is a global load the survivors' store would wait for)
    const int my_box = lane < nrow ? seg_box(g, sb, base + lane) : 0;
    // word c of the removed set, read into SGPRs: alive / kept / cnt and with them the whole chain stay scalar
    unsigned long long alive =
        ~(((unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)(removed >> 32), c) << 32) |
          (unsigned int)__builtin_amdgcn_readlane((int)removed, c));
    if (nrow < 64) alive &= (1ull << nrow) - 1ull;
    unsigned long long kept = 0;
    const unsigned int dlo = (unsigned int)diag, dhi = (unsigned int)(diag >> 32);
    // The dependent chain over the chunk's 64 boxes, a quarter of a chunk at a time: first the 16 diagonal words are moved
    // into scalar registers (independent v_readlane pairs, they pipeline), then the chain itself is pure scalar ALU --
    // test bit b of `alive`, clear the boxes that box b suppresses -- instead of two v_readlane round trips inside
    // every dependent step.  Rows past the segment's end have a zero word and no `alive` bit.
#pragma unroll
    for (int part = 0; part < 4; part++) {
      unsigned long long d[16];
#pragma unroll
      for (int b = 0; b < 16; b++)
        d[b] = ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)dhi, part * 16 + b) << 32) |
               (unsigned int)__builtin_amdgcn_readlane((int)dlo, part * 16 + b);
#pragma unroll
      for (int b = 0; b < 16; b++) {
        const unsigned long long bit = 1ull << (part * 16 + b);
        const bool on = (alive & bit) != 0;
        kept |= on ? bit : 0ull;
        alive &= on ? ~d[b] : ~0ull;
      }
    }
#pragma unroll
    for (int b = 0; b < 64; b++)
      if ((kept >> b) & 1ull) removed |= w[b];
    // survivors of the chunk, all lanes at once
    if ((kept >> lane) & 1ull) {
      const int pos = cnt + __popcll(kept & lt);
      if (pos < g.n_max) keep[pos] = my_box;
    }
    cnt += __popcll(kept);
    diag = diag_next;
  };
  unsigned long long wa[64], wb[64], wc[64];
  unsigned long long diag = load_diag(0);
  load_rows(0, wa);
  load_rows(1, wb);
  for (int c = 0; c < ncw && cnt < max_keep; c += 3) {   // the caller keeps at most max_keep survivors
    step(c, wa, wc, diag);
    if (c + 1 < ncw && cnt < max_keep) step(c + 1, wb, wa, diag);
    if (c + 2 < ncw && cnt < max_keep) step(c + 2, wc, wb, diag);
  }
  if (lane == 0) *n_keep = min(cnt, max_keep);  // the last chunk may overshoot the cap
}

// The same sweep with the mask rows staged through LDS by loader waves.  k_nms_sweep keeps three chunks of 64 rows in
// registers (384 VGPRs; the compiler moves them through the accumulation registers and scratch) and spends ~3.4 us per
// 64-box chunk, almost all of it waiting: the dependent chain itself is ~0.15 us.  Here the workgroup is one sweeper wave
// and kSwLoaders loader waves: a loader thread holds its 16-byte pieces of the next kSwStages chunks in registers (loads
// issued that many iterations ahead, so their latency is covered) and drops the oldest into one of two LDS slots while the
// sweeper works on the other; one workgroup barrier per chunk hands the slots over.  The sweeper reads its 64 diagonal
// words and, for the update of the removed set, the rows of the chunk from LDS (static offsets, conflict-free row
// stride of ncb + 1 words).  Same decisions in the same order: identical survivor lists.
static constexpr int kSwLoaders = 4, kSwStages = 4;
static constexpr int kSwThreads = 64 * (1 + kSwLoaders);
template <int NCBMAX>   // words per mask row <= NCBMAX (16: n <= 1024, 32: n <= 2048, 64: n <= 4096)
__global__ __launch_bounds__(kSwThreads) void k_nms_sweep_lds(const unsigned long long *__restrict__ mask, NmsSegs g,
                                                              int ncb, int max_keep, int32_t *__restrict__ keep,
                                                              int32_t *__restrict__ n_keep) {
  constexpr int NP = NCBMAX * 32 / (64 * kSwLoaders);      // 16-byte pieces of a chunk per loader thread
  static_assert(NP >= 1, "a chunk must give every loader thread a piece");
  extern __shared__ unsigned long long slots[];             // 2 x 64 rows x (ncb + 1) words
  __shared__ int stop_s;
  const int sb = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = seg_count(g, sb);
  mask += (size_t)sb * g.n_max * ncb;
  keep += (size_t)sb * g.n_max;
  n_keep += sb;
  const int ncw = (n + 63) / 64;
  const int rs = ncb + 1;                                    // LDS row stride in words
  const int slot_words = 64 * rs;
  if (threadIdx.x == 0) stop_s = 0;
  if (ncw == 0) {
    if (threadIdx.x == 0) *n_keep = 0;
    return;
  }
  const int half = ncb / 2 + (ncb & 1);                      // 16-byte pieces per row (the last may be half used)
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  // ---- loader side: piece p of thread tl covers words [2 q % half .., +2) of row q / half, q = tl + 64 kSwLoaders p
  const int tl = (int)threadIdx.x - 64;
  u64x2 st[kSwStages][NP];
  auto issue = [&](int c, u64x2 *dst) {                      // global loads of chunk c -> registers
    if (c >= ncw) return;
#pragma unroll
    for (int p = 0; p < NP; p++) {
      const int q = tl + 64 * kSwLoaders * p;
      const int row = q / half, w2 = (q - row * half) * 2;
      u64x2 v = {0ull, 0ull};
      if (row < 64) {
        const unsigned long long *src = mask + (size_t)min(c * 64 + row, n - 1) * ncb + w2;
        v[0] = src[0];
        if (w2 + 1 < ncb) v[1] = src[1];
      }
      dst[p] = v;
    }
  };
  auto drop = [&](int c, const u64x2 *src) {                 // registers -> LDS slot c & 1
    if (c >= ncw) return;
    unsigned long long *slot = slots + (size_t)(c & 1) * slot_words;
#pragma unroll
    for (int p = 0; p < NP; p++) {
      const int q = tl + 64 * kSwLoaders * p;
      const int row = q / half, w2 = (q - row * half) * 2;
      if (row < 64) {
        slot[row * rs + w2] = src[p][0];
        if (w2 + 1 < ncb) slot[row * rs + w2 + 1] = src[p][1];
      }
    }
  };
  // ---- sweeper state
  const unsigned long long lt = (1ull << lane) - 1ull;
  unsigned long long removed = 0;                            // word `lane` of the removed set
  int cnt = 0;
  if (wave > 0) {
#pragma unroll
    for (int j = 0; j < kSwStages; j++) issue(j, st[j]);
    drop(0, st[0]);
    issue(kSwStages, st[0]);
  }
  __syncthreads();
  for (int c0 = 0; c0 < ncw; c0 += kSwStages) {
    bool stop = false;
#pragma unroll
    for (int u = 0; u < kSwStages; u++) {
      const int c = c0 + u;
      if (c >= ncw) break;                                   // uniform
      if (wave > 0) {
        // chunk c + 1 (loaded kSwStages - 1 iterations ago) goes to the other slot; its stage is refilled
        drop(c + 1, st[(u + 1) % kSwStages]);
        issue(c + 1 + kSwStages, st[(u + 1) % kSwStages]);
      } else {
        const unsigned long long *slot = slots + (size_t)(c & 1) * slot_words;
        const int base = c * 64;
        const int nrow = min(64, n - base);
        const int my_box = lane < nrow ? seg_box(g, sb, base + lane) : 0;
        const unsigned long long diag = lane < nrow ? slot[lane * rs + c] : 0ull;
        unsigned long long alive =
            ~(((unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)(removed >> 32), c) << 32) |
              (unsigned int)__builtin_amdgcn_readlane((int)removed, c));
        if (nrow < 64) alive &= (1ull << nrow) - 1ull;
        // The chunk's greedy decision by fixed-point iteration over all lanes: box b is kept iff it is alive and no KEPT
        // earlier box of the chunk suppresses it.  K <- { b alive : (sup[b] & K) == 0 } starting from K = alive settles
        // box 0 after one step, box b once every earlier box is settled -- at most 64 steps, in practice the depth of
        // the longest suppression chain (a few) -- and its only fixed point is the greedy set.  One ballot per step
        // instead of a 64-step scalar chain fed by 128 lane reads.
        const unsigned long long sup = diag & lt;                 // earlier boxes of the chunk that suppress box `lane`
        const bool my_alive = (alive >> lane) & 1ull;
        unsigned long long kept = alive;
        for (int it = 0; it < 65; it++) {
          const unsigned long long knew = __ballot(my_alive && (sup & kept) == 0ull);
          if (knew == kept) break;
          kept = knew;
        }
        // removed |= rows of the kept boxes (word `lane`): 16 LDS reads in flight at a time
        const unsigned long long *col = slot + min(lane, ncb - 1);
#pragma unroll
        for (int part = 0; part < 4; part++) {
          unsigned long long w[16];
#pragma unroll
          for (int b = 0; b < 16; b++) w[b] = col[(part * 16 + b) * rs];
#pragma unroll
          for (int b = 0; b < 16; b++)
            if ((kept >> (part * 16 + b)) & 1ull) removed |= w[b];
        }
        if ((kept >> lane) & 1ull) {
          const int pos = cnt + __popcll(kept & lt);
          if (pos < g.n_max) keep[pos] = my_box;
        }
        cnt += __popcll(kept);
        if (cnt >= max_keep && lane == 0) stop_s = 1;
      }
      __syncthreads();
      // stop_s is one word for all chunks: the sweeper may set it for chunk c + 1 before a slow loader wave has read it
      // for chunk c.  That loader then leaves one chunk early.  The result does not depend on it: keep, cnt and n_keep are
      // the sweeper's alone, and the sweeper itself stops behind the barrier of chunk c + 1, so the slot the early leaver
      // did not fill (chunk c + 2) is never read.  The barrier count does not either: a wave that has ended no longer
      // counts towards the workgroup barrier, so the waves still at the barrier of chunk c + 1 are released by the rest.
      if (stop_s) {
        stop = true;
        break;
      }
    }
    if (stop) break;
  }
  if (threadIdx.x == 0) *n_keep = min(cnt, max_keep);
}

namespace {

struct Layout {
  unsigned long long *mask;   // [B n] rows of ncb words
  unsigned int *n_pairs;      // the pair counter: 256 bytes directly behind the mask, so that one memset clears both
  NmsBox *rec;                // [B n]
  int2 *pairs;                // every (i, j > i) of a segment may be listed
};

int carve(Arena &A, int B, int n, Layout &L) {
  const size_t rows = (size_t)B * n, ncb = ((size_t)n + 63) / 64;
  D3D_ALLOC(mask, unsigned long long, A, rows * ncb);
  D3D_ALLOC(n_pairs, unsigned int, A, 64);
  D3D_ALLOC(rec, NmsBox, A, rows);
  D3D_ALLOC(pairs, int2, A, rows * n / 2 + 64);
  L = Layout{mask, n_pairs, rec, pairs};
  return D3D_OK;
}

}  // namespace
}  // namespace d3d

using namespace d3d;

extern "C" {

// d3d_nms_sweep_mode: 0 default (the LDS form), 1 the single-wave register form, 2 the LDS form.  Starts from
// D3D_NMS_SWEEP (r...: the register form), so that A/B runs of a whole process keep working.
static int g_nms_sweep = -1;
static int nms_sweep_mode() {
  if (g_nms_sweep < 0) {
    const char *e = getenv("D3D_NMS_SWEEP");
    g_nms_sweep = (e && e[0] == 'r') ? 1 : 0;
  }
  return g_nms_sweep;
}
int d3d_nms_sweep_mode(int mode) {
  const int was = nms_sweep_mode();
  if (mode >= 0 && mode <= 2) g_nms_sweep = mode;
  return was;
}
// d3d_nms_last_form: what the calling thread's last d3d_rotate_nms_3d_batched launch chose (host stores only): sweep
// family (1 k_nms_sweep, 2 k_nms_sweep_lds), NCBMAX (0 for the register form), ncb, segments, n_max, the resolved
// max_keep, dynamic LDS bytes.  A call that launches nothing (no segments, n_max 0) leaves the record as it is.
static constexpr int kNmsFormFields = 7;
static thread_local int t_nms_last_form[kNmsFormFields] = {};
static void nms_record(int family, int ncbmax, int ncb, int segments, int n_max, int max_keep, int lds) {
  const int f[kNmsFormFields] = {family, ncbmax, ncb, segments, n_max, max_keep, lds};
  std::copy(f, f + kNmsFormFields, t_nms_last_form);
}
int d3d_nms_last_form(int *out, int n) {
  for (int i = 0; out && i < n && i < kNmsFormFields; i++) out[i] = t_nms_last_form[i];
  std::fill(t_nms_last_form, t_nms_last_form + kNmsFormFields, 0);
  return kNmsFormFields;
}

size_t d3d_nms_batched_scratch_bytes(int segments, int n_max) {
  Arena A = sizing_arena();
  Layout L;
  (void)carve(A, segments > 0 ? segments : 0, n_max > 0 ? n_max : 0, L);
  return A.used;
}
size_t d3d_nms_scratch_bytes(int n) { return d3d_nms_batched_scratch_bytes(1, n); }

int d3d_rotate_nms_3d_batched(const float *boxes, const int32_t *order, int stride, const int32_t *counts,
                              int segments, int n_max, float thresh, float min_yx, float min_z, int max_keep,
                              int32_t *keep, int32_t *n_keep, void *scratch, size_t scratch_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const int B = segments, n = n_max;
  D3D_REQUIRE(n >= 0 && n <= (1 << kNmsIdxBits), "rotate_nms_3d: n_max=%d out of range (<= 4096)", n);
  D3D_REQUIRE(B >= 0 && B <= 4096 && n_keep, "rotate_nms_3d: bad segment count %d or null n_keep", B);
  if (B == 0) return D3D_OK;
  if (n == 0) {
    D3D_HIP_CHECK(hipMemsetAsync(n_keep, 0, sizeof(int32_t) * B, s));
    return D3D_OK;
  }
  D3D_REQUIRE(boxes && keep && scratch && scratch_bytes >= d3d_nms_batched_scratch_bytes(B, n), "rotate_nms_3d: bad buffers");
  D3D_REQUIRE(B == 1 || order || stride >= n, "rotate_nms_3d: overlapping segments (stride %d < n_max %d)", stride, n);
  const int ncb = (n + 63) / 64;
  Arena A = scratch_arena(scratch, scratch_bytes);
  Layout L;
  const int rc = carve(A, B, n, L);
  if (rc) return rc;
  const NmsSegs g = {order, counts, stride, n};
  D3D_HIP_CHECK(hipMemsetAsync(L.mask, 0, (size_t)((char *)L.n_pairs - (char *)L.mask) + 256, s));  // masks + pair counter
  hipLaunchKernelGGL(k_nms_prep, dim3((n + 127) / 128, B), dim3(128), 0, s, boxes, g, min_yx, min_z, L.rec);
  hipLaunchKernelGGL(k_nms_pairs, dim3(ncb, ncb, B), dim3(256), 0, s, L.rec, g, L.pairs, L.n_pairs);
  hipLaunchKernelGGL(k_nms_eval, dim3(1024), dim3(kEvalThreads), 0, s, L.rec, L.pairs, L.n_pairs, n, ncb, thresh, L.mask);
  const int mk = max_keep > 0 ? max_keep : n;
  const bool lds_sweep = nms_sweep_mode() != 1;
  if (lds_sweep) {
    const size_t lds = (size_t)2 * 64 * (ncb + 1) * sizeof(unsigned long long);
    const int ncbmax = ncb <= 16 ? 16 : ncb <= 32 ? 32 : 64;
    if (ncb <= 16) {
      hipLaunchKernelGGL(k_nms_sweep_lds<16>, dim3(B), dim3(kSwThreads), lds, s, L.mask, g, ncb, mk, keep, n_keep);
    } else if (ncb <= 32) {
      hipLaunchKernelGGL(k_nms_sweep_lds<32>, dim3(B), dim3(kSwThreads), lds, s, L.mask, g, ncb, mk, keep, n_keep);
    } else {
      // 4033..4096 candidates: two slots of 64 rows x 65 words are 66,560 B, above 64 KiB.  A gfx950 workgroup may use
      // 160 KiB and the launch is accepted as it is (tests/test_nms_forms_gpu.py, n = 4033 and 4096)
      hipLaunchKernelGGL(k_nms_sweep_lds<64>, dim3(B), dim3(kSwThreads), lds, s, L.mask, g, ncb, mk, keep, n_keep);
    }
    nms_record(2, ncbmax, ncb, B, n, mk, (int)lds);
  } else {
    hipLaunchKernelGGL(k_nms_sweep, dim3(B), dim3(64), 0, s, L.mask, g, ncb, mk, keep, n_keep);
    nms_record(1, 0, ncb, B, n, mk, 0);
  }
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

int d3d_rotate_nms_3d_sorted(const float *boxes, int n, float thresh, int max_keep, int32_t *keep,
                             int32_t *n_keep, void *scratch, size_t scratch_bytes, void *stream) {
  return d3d_rotate_nms_3d_batched(boxes, nullptr, 0, nullptr, 1, n, thresh, 0.f, 0.f, max_keep, keep, n_keep, scratch,
                                   scratch_bytes, stream);
}

}  // extern "C"
