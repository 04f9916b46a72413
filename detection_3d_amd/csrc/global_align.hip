// The coarse pose between two levelled and squared scans (include/d3d_hip.h, d3d_global_align): one of four quarter
// turns, an integer shift on a lattice of `bin` and a z shift, by the route of box_fit.hip and frame.hip: integer votes,
// a thread per candidate, tables and peaks defined exactly, so that numpy reproduces every bit and no order can show.
//
//   rows       per cloud: class and cell of every row; three histograms in LDS, flushed with integer adds; the wall
//              classes' bird's-eye bitmaps with integer ors (a bit that is set already is not written again);
//              the target's bitmaps are then dilated 3 x 3 word by word;
//   cells      the set bits of the source's bitmaps as ascending lists of (y << 16 | x): popcounts per 1024 words, a
//              block scan, no sort, the counts stay on the device;
//   correlate  a thread per shift, both histograms in LDS (the source's turned, the target's smoothed), 64-bit sums;
//   peaks      a workgroup per correlation: the peaks go to a list, each takes the rank of its (value, shift) by counting;
//   verify     a thread per candidate (q, i, j), lanes along i: the lanes of a wave probe one bitmap row at the x shifts of
//              the peak table, one or two cache lines a probe.  The grid's second dimension cuts each list into equal
//              slices, a slice is staged in LDS by chunks of 1024, the counts go out with one integer add per thread;
//   pick       one workgroup: the best candidate, the best of each heading, the runner-up, and the pose in fp64.
#include "d3d_internal.h"

namespace d3d {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 1024;           // rows a workgroup of the row pass takes at a time; cells staged by the verification
constexpr int kMaxL = 4096;            // lattice length per axis
constexpr int kMaxK = 64;              // peaks per axis
constexpr int kMaxSep = 64;
constexpr int kMaxGrid = 1024;         // workgroups of the row pass
constexpr int kMaxSlices = 32;         // second grid dimension of the verification
constexpr int kWordsPerBlock = 4 * kThreads;
constexpr int kPhases = 6;

struct Lattice {
  int L, Lz;                           // Lx == Ly == L
  int LT;                              // 2 L + Lz: the three histograms of a cloud, x, y, z
  int W;                               // L L / 32: the words of a bitmap
  int NS;                              // 2 max(L, Lz) - 1: the row length of the correlations
};

__device__ __forceinline__ bool finite3(float a, float b, float c) {
  return fabsf(a) <= 3.402823466e38f && fabsf(b) <= 3.402823466e38f && fabsf(c) <= 3.402823466e38f;   // NaN fails
}

// class and cells of every row of one cloud; hist [LT] and bits [2][W] of this cloud, support (used, dropped)
__global__ __launch_bounds__(kThreads) void k_ga_rows(const float *__restrict__ xyz, int stride,
                                                       const float *__restrict__ nrm, int nstride, int n,
                                                       const double *__restrict__ origin, double bin, Lattice lat, float c2,
                                                       int32_t *__restrict__ hist, uint32_t *__restrict__ bits,
                                                       int32_t *__restrict__ support) {
  extern __shared__ int lh[];          // [LT]
  const int tid = threadIdx.x;
  for (int i = tid; i < lat.LT; i += kThreads) lh[i] = 0;
  __syncthreads();
  const double o0 = origin[0], o1 = origin[1], o2 = origin[2];
  int used = 0, dropped = 0;
  const long chunks = ((long)n + kChunk - 1) / kChunk;
  for (long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    for (int j = 0; j < kChunk / kThreads; j++) {
      const long row = chunk * kChunk + j * kThreads + tid;
      if (row >= n) break;
      const float *q = nrm + (size_t)row * (size_t)nstride;
      const float *p = xyz + (size_t)row * (size_t)stride;
      const float n0 = q[0], n1 = q[1], n2 = q[2], p0 = p[0], p1 = p[1], p2 = p[2];
      const float a0 = n0 * n0, a1 = n1 * n1, a2 = n2 * n2;
      const float m = (a0 + a1) + a2;
      if (!(m >= 0.5f && m <= 2.f) || !finite3(p0, p1, p2)) continue;
      const double f0 = floor(((double)p0 - o0) / bin), f1 = floor(((double)p1 - o1) / bin),
                   f2 = floor(((double)p2 - o2) / bin);
      if (!(f0 >= 0.0 && f0 < (double)lat.L && f1 >= 0.0 && f1 < (double)lat.L && f2 >= 0.0 && f2 < (double)lat.Lz)) {
        dropped++;
        continue;
      }
      used++;
      const int cx = (int)f0, cy = (int)f1, cz = (int)f2;
      const float t = c2 * m;
      const int cls = a0 >= t ? 0 : (a1 >= t ? 1 : (a2 >= t ? 2 : -1));
      if (cls < 0) continue;
      atomicAdd(&lh[cls == 0 ? cx : (cls == 1 ? lat.L + cy : 2 * lat.L + cz)], 1);
      if (cls < 2) {
        const unsigned idx = (unsigned)cy * (unsigned)lat.L + (unsigned)cx;
        uint32_t *w = bits + (size_t)cls * lat.W + (idx >> 5);
        const uint32_t b = 1u << (idx & 31);
        if (!(*w & b)) atomicOr(w, b);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < lat.LT; i += kThreads)
    if (lh[i]) atomicAdd(hist + i, lh[i]);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) used += __shfl_xor(used, d, 64), dropped += __shfl_xor(dropped, d, 64);
  if ((tid & 63) == 0) {
    if (used) atomicAdd(support, used);
    if (dropped) atomicAdd(support + 1, dropped);
  }
}

// raw [2][W] -> out [2][W]: every bit with its eight neighbours, clipped at the lattice edge; bit b of word k of row y is x = 32 k + b
__global__ void k_ga_dilate(const uint32_t *__restrict__ raw, uint32_t *__restrict__ out, Lattice lat) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= lat.W) return;
  const int wpr = lat.L >> 5, y = w / wpr, k = w - y * wpr;
  const uint32_t *r = raw + (size_t)blockIdx.y * lat.W;
  uint32_t acc = 0;
  for (int dy = -1; dy <= 1; dy++) {
    const int yy = y + dy;
    if (yy < 0 || yy >= lat.L) continue;
    const uint32_t *rr = r + (size_t)yy * wpr;
    const uint32_t v = rr[k], left = k > 0 ? rr[k - 1] : 0u, right = k < wpr - 1 ? rr[k + 1] : 0u;
    acc |= v | (v << 1) | (v >> 1) | (left >> 31) | (right << 31);
  }
  out[(size_t)blockIdx.y * lat.W + w] = acc;
}

// exclusive scan of one int per thread over the workgroup of kThreads; total: the sum
__device__ __forceinline__ int block_scan_excl(int v, int &total) {
  __shared__ int wsum[kThreads / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; w++) {
    if (w < wv) base += wsum[w];
    total += wsum[w];
  }
  __syncthreads();
  return base + inc - v;
}

// the set bits of every kWordsPerBlock words of a source bitmap: blocksum [2][nb]
__global__ __launch_bounds__(kThreads) void k_ga_popc(const uint32_t *__restrict__ bits, Lattice lat, int nb,
                                                       int32_t *__restrict__ blocksum) {
  const uint32_t *b = bits + (size_t)blockIdx.y * lat.W;
  const int w0 = blockIdx.x * kWordsPerBlock + 4 * threadIdx.x;
  int c = 0;
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (w0 + k < lat.W) c += __popc(b[w0 + k]);
  int total;
  block_scan_excl(c, total);
  if (threadIdx.x == 0) blocksum[blockIdx.y * nb + blockIdx.x] = total;
}

// ... and the bits as cells (y << 16 | x) in ascending order: cells [2][cap], count [2]
__global__ __launch_bounds__(kThreads) void k_ga_compact(const uint32_t *__restrict__ bits, Lattice lat, int nb,
                                                          const int32_t *__restrict__ blocksum, int32_t *__restrict__ cells,
                                                          int cap, int32_t *__restrict__ count) {
  const uint32_t *b = bits + (size_t)blockIdx.y * lat.W;
  int before = 0;
  for (int k = threadIdx.x; k < (int)blockIdx.x; k += kThreads) before += blocksum[blockIdx.y * nb + k];
  int prefix;
  block_scan_excl(before, prefix);
  const int w0 = blockIdx.x * kWordsPerBlock + 4 * threadIdx.x;
  uint32_t word[4];
  int c = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    word[k] = w0 + k < lat.W ? b[w0 + k] : 0u;
    c += __popc(word[k]);
  }
  int total;
  int pos = prefix + block_scan_excl(c, total);
  int32_t *out = cells + (size_t)blockIdx.y * cap;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    uint32_t v = word[k];
    const int first = (w0 + k) << 5, y = first / lat.L, x0 = first - y * lat.L;
    while (v) {
      const int bit = __ffs(v) - 1;
      v &= v - 1;
      if (pos < cap) out[pos] = (y << 16) | (x0 + bit);     // (the count cannot pass cap: a bit has a row of the source)
      pos++;
    }
  }
  if (blockIdx.x == (unsigned)nb - 1 && threadIdx.x == 0) count[blockIdx.y] = prefix + total;
}

// correlation k = 2 q + axis (axis 0: x, 1: y) for k < 8, k = 8: z.  hist [2][LT]: source, target.  corr [9][NS], entry
// s + La - 1 of a row the shift s; the entries past 2 La - 1 are zero.
__global__ __launch_bounds__(kThreads) void k_ga_correlate(const int32_t *__restrict__ hist, Lattice lat,
                                                            long long *__restrict__ corr) {
  __shared__ int hs[kMaxL], ht[kMaxL];
  const int k = blockIdx.y, tid = threadIdx.x;
  const int La = k < 8 ? lat.L : lat.Lz;
  const int32_t *src, *tgt = hist + lat.LT;
  bool rev = false;
  if (k < 8) {
    const int q = k >> 1, ax = k & 1;
    const int from = (ax ^ q) & 1;                       // the source class that the turn makes class ax
    src = hist + from * lat.L;
    rev = ax == 0 ? (q == 1 || q == 2) : (q == 2 || q == 3);
    tgt += ax * lat.L;
  } else {
    src = hist + 2 * lat.L;
    tgt += 2 * lat.L;
  }
  for (int c = tid; c < La; c += kThreads) {
    hs[c] = src[rev ? La - 1 - c : c];
    ht[c] = 2 * tgt[c] + (c > 0 ? tgt[c - 1] : 0) + (c < La - 1 ? tgt[c + 1] : 0);
  }
  __syncthreads();
  const int at = blockIdx.x * kThreads + tid;
  if (at >= lat.NS) return;
  long long sum = 0;
  if (at < 2 * La - 1) {
    const int s = at - (La - 1);
    for (int c = 0; c < La; c++) {
      const int h = hs[c];                               // one address for the wave
      if (h == 0) continue;
      const int t = c + s;
      if ((unsigned)t < (unsigned)La) sum += (long long)h * (long long)ht[t];
    }
  }
  corr[(size_t)k * lat.NS + at] = sum;
}

// one workgroup per correlation: peak_value / peak_shift [9][K]; list_value / list_shift [9][NS] take the peaks unordered
__global__ __launch_bounds__(kThreads) void k_ga_peaks(const long long *__restrict__ corr, Lattice lat, int K, int sep,
                                                        long long *list_value, int32_t *list_shift,
                                                        long long *__restrict__ peak_value,
                                                        int32_t *__restrict__ peak_shift) {
  __shared__ int cnt;
  const int k = blockIdx.x, tid = threadIdx.x;
  const int La = k < 8 ? lat.L : lat.Lz, ns = 2 * La - 1;
  const long long *C = corr + (size_t)k * lat.NS;
  long long *lv = list_value + (size_t)k * lat.NS;
  int32_t *ls = list_shift + (size_t)k * lat.NS;
  if (tid == 0) cnt = 0;
  __syncthreads();
  for (int at = tid; at < ns; at += kThreads) {
    const long long v = C[at];
    bool peak = v > 0;
    for (int d = 1; peak && d <= sep; d++) {
      if (at - d >= 0 && C[at - d] >= v) peak = false;
      if (at + d < ns && C[at + d] > v) peak = false;
    }
    if (peak) {
      const int slot = atomicAdd(&cnt, 1);
      lv[slot] = v;
      ls[slot] = at - (La - 1);
    }
  }
  __syncthreads();
  const int P = cnt;
  for (int p = tid; p < P; p += kThreads) {
    const long long v = lv[p];
    const int s = ls[p];
    int rank = 0;
    for (int j = 0; j < P; j++) {
      const long long vj = lv[j];
      rank += vj > v || (vj == v && ls[j] < s);
    }
    if (rank < K) peak_value[k * K + rank] = v, peak_shift[k * K + rank] = s;
  }
  for (int r = (P < K ? P : K) + tid; r < K; r += kThreads) peak_value[k * K + r] = -1, peak_shift[k * K + r] = 0;
}

// scores [4][K][K]: 0 for a candidate of two valid peaks, -1 otherwise
__global__ void k_ga_scores_begin(const long long *__restrict__ peak_value, int K, int32_t *__restrict__ scores) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 4 * K * K) return;
  const int q = t / (K * K), r = t - q * K * K, i = r / K, j = r - i * K;
  scores[t] = peak_value[(2 * q) * K + i] > 0 && peak_value[(2 * q + 1) * K + j] > 0 ? 0 : -1;
}

// thread blockIdx.x * 256 + tid = (q K + j) K + i: the candidate (q, i, j), the lanes of a wave along i.  cells [2][cap] and
// count [2] of the source's classes x and y, tbits [2][W] the target's dilated bitmaps.
__global__ __launch_bounds__(kThreads) void k_ga_verify(const int32_t *__restrict__ cells, int cap,
                                                         const int32_t *__restrict__ count,
                                                         const uint32_t *__restrict__ tbits, Lattice lat, int K,
                                                         const long long *__restrict__ peak_value,
                                                         const int32_t *__restrict__ peak_shift,
                                                         int32_t *__restrict__ scores) {
  __shared__ int stage[kChunk];
  const int tid = threadIdx.x, t = blockIdx.x * kThreads + tid, L = lat.L;
  bool live = t < 4 * K * K;
  int q = 0, i = 0, j = 0;
  if (live) {
    q = t / (K * K);
    const int r = t - q * K * K;
    j = r / K, i = r - j * K;
    live = peak_value[(2 * q) * K + i] > 0 && peak_value[(2 * q + 1) * K + j] > 0;
  }
  const int sx = live ? peak_shift[(2 * q) * K + i] : 0, sy = live ? peak_shift[(2 * q + 1) * K + j] : 0;
  // turned cell + shift: tx = axx cx + axy cy + bx, ty = ayx cx + ayy cy + by
  const int axx = q == 0 ? 1 : (q == 2 ? -1 : 0), axy = q == 1 ? -1 : (q == 3 ? 1 : 0);
  const int ayx = q == 1 ? 1 : (q == 3 ? -1 : 0), ayy = q == 0 ? 1 : (q == 2 ? -1 : 0);
  const int bx = sx + ((q == 1 || q == 2) ? L - 1 : 0), by = sy + ((q == 2 || q == 3) ? L - 1 : 0);
  int sum = 0;
  for (int cls = 0; cls < 2; cls++) {
    const int cnt = min(count[cls], cap);
    const uint32_t *tb = tbits + (size_t)(cls ^ (q & 1)) * lat.W;   // an odd turn swaps the wall classes
    const int32_t *list = cells + (size_t)cls * cap;
    const int per = (cnt + (int)gridDim.y - 1) / (int)gridDim.y;      // the list in equal slices: its length is known here only
    const int last = min(cnt, ((int)blockIdx.y + 1) * per);
    for (int base = blockIdx.y * per; base < last; base += kChunk) {
      const int here = min(kChunk, last - base);
      for (int l = tid; l < here; l += kThreads) stage[l] = list[base + l];
      __syncthreads();
      if (live) {
        for (int e = 0; e < here; e++) {
          const int c = stage[e], cx = c & 0xffff, cy = c >> 16;
          const int tx = axx * cx + axy * cy + bx, ty = ayx * cx + ayy * cy + by;
          if ((unsigned)tx < (unsigned)L && (unsigned)ty < (unsigned)L) {
            const unsigned idx = (unsigned)ty * (unsigned)L + (unsigned)tx;
            sum += (tb[idx >> 5] >> (idx & 31)) & 1u;
          }
        }
      }
      __syncthreads();
    }
  }
  if (live && sum) atomicAdd(scores + (q * K + i) * K + j, sum);
}

// one workgroup: the best candidate (the lowest (q, i, j) among equals), the best of every heading, the runner-up, the pose
__global__ __launch_bounds__(kThreads) void k_ga_pick(const int32_t *__restrict__ scores, int K, Lattice lat, double bin,
                                                       const long long *__restrict__ peak_value,
                                                       const int32_t *__restrict__ peak_shift,
                                                       const double *__restrict__ os, const double *__restrict__ ot,
                                                       double *__restrict__ pose, int32_t *__restrict__ choice,
                                                       long long *__restrict__ score, int32_t *__restrict__ status) {
  __shared__ unsigned long long best_key;
  __shared__ unsigned head[4], second;
  const int tid = threadIdx.x, total = 4 * K * K;
  if (tid == 0) best_key = 0ull, second = 0u;
  if (tid < 4) head[tid] = 0u;
  __syncthreads();
  // key: (score + 1) above, the index counted down below, so that the largest key is the highest score at the lowest index
  unsigned long long mine = 0ull;
  for (int t = tid; t < total; t += kThreads) {
    const unsigned v = (unsigned)(scores[t] + 1);
    const unsigned long long key = ((unsigned long long)v << 32) | (unsigned)(total - t);
    if (key > mine) mine = key;
    atomicMax(&head[t / (K * K)], v);
  }
  atomicMax(&best_key, mine);
  __syncthreads();
  const int at = total - (int)(unsigned)(best_key & 0xffffffffull);
  unsigned other = 0u;
  for (int t = tid; t < total; t += kThreads)
    if (t != at) other = max(other, (unsigned)(scores[t] + 1));
  atomicMax(&second, other);
  __syncthreads();
  if (tid != 0) return;
  const long long best = (long long)(best_key >> 32) - 1;
  for (int h = 0; h < 4; h++) score[h] = (long long)head[h] - 1;
  score[4] = best;
  score[5] = (long long)second - 1;
  for (int r = 0; r < 16; r++) pose[r] = (r % 5 == 0) ? 1.0 : 0.0;
  if (best <= 0) {                                      // no wall met a wall: the origins' shift alone
    status[0] = 1;
    choice[0] = choice[1] = choice[2] = choice[3] = 0;
    for (int a = 0; a < 3; a++) pose[4 * a + 3] = ot[a] - os[a];
    return;
  }
  const int q = at / (K * K), r = at - q * K * K, i = r / K, j = r - i * K;
  const int sx = peak_shift[(2 * q) * K + i], sy = peak_shift[(2 * q + 1) * K + j];
  const int sz = peak_value[8 * K] > 0 ? peak_shift[8 * K] : 0;
  status[0] = 0;
  choice[0] = q, choice[1] = sx, choice[2] = sy, choice[3] = sz;
  const int half = lat.L / 2;
  const double hb = bin * (double)half;
  const double ux = os[0] + hb, uy = os[1] + hb, uz = os[2];
  const double vx = ot[0] + bin * (double)(sx + half), vy = ot[1] + bin * (double)(sy + half), vz = ot[2] + bin * (double)sz;
  // Rz(q) u, its entries 0 and +-1: selections and sign changes, no product
  const double wx = q == 0 ? ux : (q == 1 ? -uy : (q == 2 ? -ux : uy));
  const double wy = q == 0 ? uy : (q == 1 ? ux : (q == 2 ? -uy : -ux));
  const double c = q == 0 ? 1.0 : (q == 2 ? -1.0 : 0.0), s = q == 1 ? 1.0 : (q == 3 ? -1.0 : 0.0);
  pose[0] = c, pose[1] = s == 0.0 ? 0.0 : -s, pose[4] = s, pose[5] = c;
  pose[3] = vx - wx, pose[7] = vy - wy, pose[11] = vz - uz;
}

bool lattice_of(const int *lattice, Lattice &lat) {
  if (!lattice) return false;
  const int L = lattice[0], Lz = lattice[2];
  if (L != lattice[1] || L < 32 || L > kMaxL || (L & 31) || Lz < 1 || Lz > kMaxL) return false;
  lat.L = L, lat.Lz = Lz, lat.LT = 2 * L + Lz, lat.W = L * L / 32;
  lat.NS = 2 * (L > Lz ? L : Lz) - 1;
  return true;
}

int cells_cap(int n_source, const Lattice &lat) {
  const long c = (long)lat.L * lat.L < (long)n_source ? (long)lat.L * lat.L : (long)n_source;
  return (int)(c < 1 ? 1 : c);
}

int popc_blocks(const Lattice &lat) { return (lat.W + kWordsPerBlock - 1) / kWordsPerBlock; }

// the words of the region that a call zeroes first: hist [2][LT], support [4], count [2] and 2 spare, bitmaps source [2][W] and target raw [2][W]
size_t zero_words(const Lattice &lat) { return (size_t)2 * lat.LT + 8 + (size_t)4 * lat.W; }

size_t global_scratch_bytes(int n_source, const Lattice &lat, int K) {
  size_t b = 0;
  auto add = [&](size_t bytes) { b += ((bytes + 255) & ~size_t(255)) + 256; };
  add(zero_words(lat) * 4);
  add((size_t)2 * lat.W * 4);                           // dilated
  add((size_t)2 * cells_cap(n_source, lat) * 4);
  add((size_t)2 * popc_blocks(lat) * 4);
  add((size_t)9 * lat.NS * 8);                          // corr
  add((size_t)9 * lat.NS * 8);                          // list_value
  add((size_t)9 * lat.NS * 4);                          // list_shift
  add((size_t)9 * K * 8);
  add((size_t)9 * K * 4);
  add((size_t)4 * K * K * 4);
  return b;
}

}  // namespace
}  // namespace d3d

using namespace d3d;

size_t d3d_global_align_scratch_bytes(int n_source, const int *lattice, int peaks) {
  Lattice lat;
  if (n_source < 0 || peaks < 1 || peaks > kMaxK || !lattice_of(lattice, lat)) return 0;
  return global_scratch_bytes(n_source, lat, peaks);
}

int d3d_global_align(const float *source, int m, int source_stride_floats, const float *source_normals,
                     int source_normal_stride_floats, const double *source_origin_dev, const float *target, int n,
                     int target_stride_floats, const float *target_normals, int target_normal_stride_floats,
                     const double *target_origin_dev, double bin, const int *lattice, float c2, int peaks, int sep,
                     double *pose, int32_t *choice, int64_t *score, int32_t *support, int32_t *status,
                     const d3d_global_align_details *details, void *scratch, size_t scratch_bytes, void *stream,
                     float *phase_ms_host) {
  Lattice lat;
  D3D_REQUIRE(m >= 0 && n >= 0 && m <= (1 << 28) && n <= (1 << 28), "d3d_global_align: %d and %d rows outside [0, 2^28]", m, n);
  D3D_REQUIRE(lattice_of(lattice, lat),
              "d3d_global_align: lattice must be (L, L, Lz) with L a multiple of 32 in [32, %d] and Lz in [1, %d]", kMaxL, kMaxL);
  D3D_REQUIRE(m == 0 || (source && source_normals), "d3d_global_align: null pointer (source, source_normals)");
  D3D_REQUIRE(n == 0 || (target && target_normals), "d3d_global_align: null pointer (target, target_normals)");
  D3D_REQUIRE(m <= 1 || (source_stride_floats >= 3 && source_normal_stride_floats >= 3),
              "d3d_global_align: source row strides %d, %d < 3 floats", source_stride_floats, source_normal_stride_floats);
  D3D_REQUIRE(n <= 1 || (target_stride_floats >= 3 && target_normal_stride_floats >= 3),
              "d3d_global_align: target row strides %d, %d < 3 floats", target_stride_floats, target_normal_stride_floats);
  D3D_REQUIRE(source_origin_dev && target_origin_dev, "d3d_global_align: null pointer (origins)");
  D3D_REQUIRE(bin > 0.0 && bin <= 1e6, "d3d_global_align: bin %g must be positive and finite", bin);
  D3D_REQUIRE(c2 >= 0.88f && c2 < 1.f, "d3d_global_align: c2 = %g is not the squared cosine of an angle in (0, 20] degrees", (double)c2);
  D3D_REQUIRE(peaks >= 1 && peaks <= kMaxK, "d3d_global_align: peaks %d outside [1, %d]", peaks, kMaxK);
  D3D_REQUIRE(sep >= 0 && sep <= kMaxSep, "d3d_global_align: sep %d outside [0, %d]", sep, kMaxSep);
  D3D_REQUIRE(pose && choice && score && support && status, "d3d_global_align: null pointer (pose, choice, score, support, status)");
  const size_t need = global_scratch_bytes(m, lat, peaks);
  D3D_REQUIRE(scratch && scratch_bytes >= need, "d3d_global_align: scratch of %zu bytes, need %zu", scratch_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  const int K = peaks, cap = cells_cap(m, lat), nb = popc_blocks(lat);
  Arena A = scratch_arena(scratch, scratch_bytes);
  D3D_ALLOC(zero, int32_t, A, zero_words(lat));
  int32_t *hist = zero, *sup = zero + 2 * lat.LT, *count = sup + 4;
  uint32_t *sbits = reinterpret_cast<uint32_t *>(count + 4), *traw = sbits + (size_t)2 * lat.W;
  D3D_ALLOC(tbits, uint32_t, A, (size_t)2 * lat.W);
  D3D_ALLOC(cells, int32_t, A, (size_t)2 * cap);
  D3D_ALLOC(blocksum, int32_t, A, (size_t)2 * nb);
  D3D_ALLOC(corr, long long, A, (size_t)9 * lat.NS);
  D3D_ALLOC(list_value, long long, A, (size_t)9 * lat.NS);
  D3D_ALLOC(list_shift, int32_t, A, (size_t)9 * lat.NS);
  D3D_ALLOC(peak_value, long long, A, (size_t)9 * K);
  D3D_ALLOC(peak_shift, int32_t, A, (size_t)9 * K);
  D3D_ALLOC(scores, int32_t, A, (size_t)4 * K * K);
  Timer T;
  if (int rc = T.start(phase_ms_host != nullptr, kPhases + 1)) return rc;
  if (int rc = T.mark(0, s)) return rc;
  D3D_HIP_CHECK(hipMemsetAsync(zero, 0, zero_words(lat) * 4, s));
  const size_t lds = (size_t)lat.LT * sizeof(int);
  if (m > 0) {
    const long chunks = ((long)m + kChunk - 1) / kChunk;
    hipLaunchKernelGGL(k_ga_rows, dim3((unsigned)(chunks < kMaxGrid ? chunks : kMaxGrid)), dim3(kThreads), lds, s, source,
                       source_stride_floats, source_normals, source_normal_stride_floats, m, source_origin_dev, bin, lat, c2,
                       hist, sbits, sup);
  }
  if (n > 0) {
    const long chunks = ((long)n + kChunk - 1) / kChunk;
    hipLaunchKernelGGL(k_ga_rows, dim3((unsigned)(chunks < kMaxGrid ? chunks : kMaxGrid)), dim3(kThreads), lds, s, target,
                       target_stride_floats, target_normals, target_normal_stride_floats, n, target_origin_dev, bin, lat, c2,
                       hist + lat.LT, traw, sup + 2);
  }
  hipLaunchKernelGGL(k_ga_dilate, dim3(grid1d(lat.W).x, 2), dim3(256), 0, s, traw, tbits, lat);
  if (int rc = T.mark(1, s)) return rc;
  hipLaunchKernelGGL(k_ga_popc, dim3(nb, 2), dim3(kThreads), 0, s, sbits, lat, nb, blocksum);
  hipLaunchKernelGGL(k_ga_compact, dim3(nb, 2), dim3(kThreads), 0, s, sbits, lat, nb, blocksum, cells, cap, count);
  if (int rc = T.mark(2, s)) return rc;
  hipLaunchKernelGGL(k_ga_correlate, dim3(grid1d(lat.NS, kThreads).x, 9), dim3(kThreads), 0, s, hist, lat, corr);
  if (int rc = T.mark(3, s)) return rc;
  hipLaunchKernelGGL(k_ga_peaks, dim3(9), dim3(kThreads), 0, s, corr, lat, K, sep, list_value, list_shift, peak_value,
                     peak_shift);
  hipLaunchKernelGGL(k_ga_scores_begin, grid1d(4 * K * K), dim3(256), 0, s, peak_value, K, scores);
  if (int rc = T.mark(4, s)) return rc;
  const int slices = (cap + kChunk - 1) / kChunk;
  hipLaunchKernelGGL(k_ga_verify, dim3(grid1d(4 * K * K, kThreads).x, slices < kMaxSlices ? slices : kMaxSlices),
                     dim3(kThreads), 0, s, cells, cap, count, tbits, lat, K, peak_value, peak_shift, scores);
  if (int rc = T.mark(5, s)) return rc;
  hipLaunchKernelGGL(k_ga_pick, dim3(1), dim3(kThreads), 0, s, scores, K, lat, bin, peak_value, peak_shift,
                     source_origin_dev, target_origin_dev, pose, choice, reinterpret_cast<long long *>(score), status);
  D3D_LAUNCH_CHECK();
  D3D_HIP_CHECK(hipMemcpyAsync(support, sup, 4 * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (details) {
    const hipMemcpyKind dd = hipMemcpyDeviceToDevice;
    if (details->hist) D3D_HIP_CHECK(hipMemcpyAsync(details->hist, hist, (size_t)2 * lat.LT * 4, dd, s));
    if (details->cells) D3D_HIP_CHECK(hipMemcpyAsync(details->cells, cells, (size_t)2 * cap * 4, dd, s));
    if (details->cell_count) D3D_HIP_CHECK(hipMemcpyAsync(details->cell_count, count, 2 * 4, dd, s));
    if (details->target_bits) D3D_HIP_CHECK(hipMemcpyAsync(details->target_bits, tbits, (size_t)2 * lat.W * 4, dd, s));
    if (details->corr) D3D_HIP_CHECK(hipMemcpyAsync(details->corr, corr, (size_t)9 * lat.NS * 8, dd, s));
    if (details->peak_value) D3D_HIP_CHECK(hipMemcpyAsync(details->peak_value, peak_value, (size_t)9 * K * 8, dd, s));
    if (details->peak_shift) D3D_HIP_CHECK(hipMemcpyAsync(details->peak_shift, peak_shift, (size_t)9 * K * 4, dd, s));
    if (details->scores) D3D_HIP_CHECK(hipMemcpyAsync(details->scores, scores, (size_t)4 * K * K * 4, dd, s));
  }
  if (int rc = T.mark(6, s)) return rc;
  return T.finish(phase_ms_host);
}
