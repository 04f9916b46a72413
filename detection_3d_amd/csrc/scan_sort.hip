// Exclusive int32 scan, the stable radix sort of (key, value) pairs and the 0xFF fill: what every builder of the
// library sorts, ranks and clears with.
#include "grid_internal.h"

namespace d3d {

// ------------------------------------------------------------------------------------------
// Exclusive scan of int32: wave64 shuffle scan -> block scan -> block-sum scan -> add.
__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    int t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

__global__ __launch_bounds__(kScanThreads) void k_scan_tiles(const int32_t *__restrict__ in,
                                                             int32_t *__restrict__ out, int n,
                                                             int32_t *__restrict__ tile_sums) {
  D3D_SIDE_PRIO();
  __shared__ int wave_tot[kScanThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long base = (long)blockIdx.x * kScanTile + (long)tid * kScanItems;
  int v[kScanItems];
  int sum = 0;
#pragma unroll
  for (int i = 0; i < kScanItems; i++) {
    v[i] = (base + i < n) ? in[base + i] : 0;
    sum += v[i];
  }
  int incl = wave_inclusive_scan(sum, lane);
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  int wave_off = 0;
  for (int w = 0; w < wave; w++) wave_off += wave_tot[w];
  int run = wave_off + incl - sum;
#pragma unroll
  for (int i = 0; i < kScanItems; i++) {
    if (base + i < n) out[base + i] = run;
    run += v[i];
  }
  if (tid == kScanThreads - 1) tile_sums[blockIdx.x] = run;
}

// (one workgroup of 4 waves: it finds a free slot beside the convolutions of another stream at once -- as 16 waves it
//  waited ~0.1 ms per call for a CU to drain in the 4 x 1 M-point step)
static constexpr int kSumThreads = 256;
__global__ __launch_bounds__(kSumThreads) void k_scan_sums(int32_t *__restrict__ sums, int nb,
                                                           int32_t *__restrict__ total) {
  D3D_SIDE_PRIO();
  __shared__ int wave_tot[kSumThreads / 64];
  __shared__ int carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += kSumThreads) {
    int i = base + tid;
    int v = i < nb ? sums[i] : 0;
    int incl = wave_inclusive_scan(v, lane);
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int off = carry_s;
    for (int w = 0; w < wave; w++) off += wave_tot[w];
    if (i < nb) sums[i] = off + incl - v;
    __syncthreads();
    if (tid == kSumThreads - 1) carry_s = off + incl;
    __syncthreads();
  }
  if (tid == 0 && total) *total = carry_s;
}

__global__ __launch_bounds__(kScanThreads) void k_scan_add(int32_t *__restrict__ out, int n,
                                                           const int32_t *__restrict__ sums) {
  D3D_SIDE_PRIO();
  const long base = (long)blockIdx.x * kScanTile + (long)threadIdx.x * kScanItems;
  const int add = sums[blockIdx.x];
#pragma unroll
  for (int i = 0; i < kScanItems; i++)
    if (base + i < n) out[base + i] += add;
}

int scan_exclusive_i32(const int32_t *in, int32_t *out, int n, int32_t *total_dev, Arena &scratch,
                       hipStream_t s) {
  if (n <= 0) {
    if (total_dev) D3D_HIP_CHECK(hipMemsetAsync(total_dev, 0, sizeof(int32_t), s));
    return D3D_OK;
  }
  int nb = (n + kScanTile - 1) / kScanTile;
  D3D_ALLOC(sums, int32_t, scratch, nb);
  hipLaunchKernelGGL(k_scan_tiles, dim3(nb), dim3(kScanThreads), 0, s, in, out, n, sums);
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(kSumThreads), 0, s, sums, nb, total_dev);
  hipLaunchKernelGGL(k_scan_add, dim3(nb), dim3(kScanThreads), 0, s, out, n, sums);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

// ------------------------------------------------------------------------------------------
// Stable LSD radix sort of (uint32 key, int32 value) pairs by the low `bits` bits of the key: three launches per pass
// and no cross-workgroup waiting -- per-tile digit histograms -> per-digit scan over the tiles -> ranked scatter -- with
// 8-, 9- or 10-bit digits, whichever covers `bits` in the fewest passes (27 bits: 3 x 9; 19 bits: 2 x 10; 8 bits: one).
// rocPRIM's device sort takes ~20 dependent launches of 5-7 us (block sort + merge passes) for the 10^4 .. 5*10^5 rows of
// a rulebook -- 110-190 us, almost all launch latency -- and its Onesweep variant 25-33 us per pass at these sizes (the
// look-back chain over a few dozen tiles is serial); this one is bound by its 3 launches per pass (~17 us).
// Descending order sorts the complemented digits, so it is stable too.  The digits of the last pass are cut to the bits
// that remain (dmask): key bits above `bits` never take part, also where the digits cover more than `bits` (4 bits: one
// 8-bit digit; 19 bits: 2 x 10).  finalize_plan relies on it: its keys carry the rows' popcounts above the offset mask.
static constexpr int kRsThreads = 256;
static constexpr int kRsItems = 8;
static constexpr int kRsTile = kRsThreads * kRsItems;

template <int DB>
__device__ __forceinline__ uint32_t rs_digit(uint32_t k, int shift, bool desc, uint32_t dmask) {
  static_assert(DB >= 8 && DB <= 10, "digit width");
  return ((desc ? ~k : k) >> shift) & dmask;
}

// hist[digit][tile] of one pass
// n_dev (may be null): the element count on the device, for a sort enqueued with an upper bound `n` (and its n_tiles)
template <int DB>
__global__ __launch_bounds__(kRsThreads) void k_rs_count(const uint32_t *__restrict__ keys, int n, int n_tiles, int shift,
                                                         int desc, uint32_t dmask, uint32_t *__restrict__ hist,
                                                         const int32_t *__restrict__ n_dev) {
  D3D_SIDE_PRIO();
  constexpr int BINS = 1 << DB;
  __shared__ uint32_t h[BINS];
  if (n_dev) n = *n_dev;
  for (int b = threadIdx.x; b < BINS; b += kRsThreads) h[b] = 0;
  __syncthreads();
  const int base = blockIdx.x * kRsTile;
#pragma unroll
  for (int j = 0; j < kRsItems; j++) {
    const int i = base + j * kRsThreads + threadIdx.x;
    if (i < n) atomicAdd(&h[rs_digit<DB>(keys[i], shift, desc != 0, dmask)], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < BINS; b += kRsThreads) hist[(size_t)b * n_tiles + blockIdx.x] = h[b];
}

// one workgroup per digit: exclusive scan of its counts over the tiles (in place) and the digit's total
__global__ __launch_bounds__(kRsThreads) void k_rs_scan(uint32_t *__restrict__ hist, int n_tiles,
                                                        uint32_t *__restrict__ totals) {
  D3D_SIDE_PRIO();
  __shared__ uint32_t wave_tot[kRsThreads / 64];
  __shared__ uint32_t carry_s;
  uint32_t *row = hist + (size_t)blockIdx.x * n_tiles;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < n_tiles; base += kRsThreads) {
    const int i = base + tid;
    const uint32_t v = i < n_tiles ? row[i] : 0u;
    const uint32_t incl = (uint32_t)wave_inclusive_scan((int)v, lane);
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    uint32_t off = carry_s;
    for (int w = 0; w < wave; w++) off += wave_tot[w];
    if (i < n_tiles) row[i] = off + incl - v;
    __syncthreads();
    if (tid == kRsThreads - 1) carry_s = off + incl;
    __syncthreads();
  }
  if (tid == 0) totals[blockIdx.x] = carry_s;
}

// Ranked scatter of one tile.  Wave w owns the tile's elements [512 w, 512 w + 512) and walks them in 8 rounds of 64
// consecutive ones; the lanes of a round that hold the same digit find each other with DB ballots, take consecutive
// ranks behind the wave's running count of that digit, and the waves' counts are chained in wave order: the rank of an
// element is the number of elements of its digit before it in the tile, i.e. the pass is stable.
template <int DB>
__global__ __launch_bounds__(kRsThreads) void k_rs_scatter(const uint32_t *__restrict__ keys_in,
                                                           const int32_t *__restrict__ vals_in, int n, int n_tiles,
                                                           int shift, int desc, uint32_t dmask,
                                                           const uint32_t *__restrict__ hist,
                                                           const uint32_t *__restrict__ totals,
                                                           uint32_t *__restrict__ keys_out,
                                                           int32_t *__restrict__ vals_out,
                                                           const int32_t *__restrict__ n_dev) {
  D3D_SIDE_PRIO();
  constexpr int NW = kRsThreads / 64, BINS = 1 << DB, PER = BINS / kRsThreads;
  if (n_dev) n = *n_dev;
  __shared__ uint32_t wcnt[NW][BINS];
  __shared__ uint32_t wave_tot[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int b = tid; b < NW * BINS; b += kRsThreads) (&wcnt[0][0])[b] = 0;
  __syncthreads();
  const int base = blockIdx.x * kRsTile + wave * (64 * kRsItems);
  uint32_t key[kRsItems], dig[kRsItems], rank[kRsItems];
  const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < kRsItems; r++) {
    const int i = base + r * 64 + lane;
    const bool ok = i < n;
    key[r] = ok ? keys_in[i] : 0u;
    const uint32_t d = rs_digit<DB>(key[r], shift, desc != 0, dmask);
    dig[r] = d;
    unsigned long long m = __ballot(ok);
#pragma unroll
    for (int b = 0; b < DB; b++) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      m &= bit ? bal : ~bal;
    }
    // every lane of a group reads the count before the group's first lane adds to it (LDS serves a wave in order)
    const uint32_t before = ok ? wcnt[wave][d] : 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    rank[r] = before + (uint32_t)__popcll(m & lt);
    if (ok && (m & lt) == 0) wcnt[wave][d] = before + (uint32_t)__popcll(m);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  __syncthreads();
  // thread t, digits PER t .. PER t + PER - 1: where a digit of this tile starts = the digits before it (all tiles) +
  // the same digit in the tiles before this one, then the waves in order
  uint32_t pre[PER], sum = 0;
#pragma unroll
  for (int j = 0; j < PER; j++) {
    pre[j] = sum;
    sum += totals[tid * PER + j];
  }
  const uint32_t incl = (uint32_t)wave_inclusive_scan((int)sum, lane);
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  uint32_t first = incl - sum;
  for (int w = 0; w < wave; w++) first += wave_tot[w];
#pragma unroll
  for (int j = 0; j < PER; j++) {
    const int d = tid * PER + j;
    uint32_t off = first + pre[j] + hist[(size_t)d * n_tiles + blockIdx.x];
#pragma unroll
    for (int w = 0; w < NW; w++) {
      const uint32_t c = wcnt[w][d];
      wcnt[w][d] = off;
      off += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kRsItems; r++) {
    const int i = base + r * 64 + lane;
    if (i < n) {
      const uint32_t pos = wcnt[wave][dig[r]] + rank[r];
      if (keys_out) keys_out[pos] = key[r];
      vals_out[pos] = vals_in[i];
    }
  }
}

template <int DB>
static void rs_pass(const uint32_t *ksrc, const int32_t *vsrc, int n, int n_tiles, int shift, int bits, bool desc,
                    uint32_t *hist, uint32_t *totals, uint32_t *kdst, int32_t *vdst, hipStream_t s, const int32_t *n_dev) {
  const uint32_t dmask = (1u << std::min(DB, bits - shift)) - 1u;   // the digit, cut to the key bits that remain
  hipLaunchKernelGGL(k_rs_count<DB>, dim3(n_tiles), dim3(kRsThreads), 0, s, ksrc, n, n_tiles, shift, desc ? 1 : 0, dmask,
                     hist, n_dev);
  hipLaunchKernelGGL(k_rs_scan, dim3(1 << DB), dim3(kRsThreads), 0, s, hist, n_tiles, totals);
  hipLaunchKernelGGL(k_rs_scatter<DB>, dim3(n_tiles), dim3(kRsThreads), 0, s, ksrc, vsrc, n, n_tiles, shift, desc ? 1 : 0,
                     dmask, hist, totals, kdst, vdst, n_dev);
}
size_t sort_scratch_bytes(int n, int bits) {
  int passes, db;
  rs_layout(bits, passes, db);
  const size_t tiles = ((size_t)std::max(n, 1) + kRsTile - 1) / kRsTile;
  return (((size_t)1 << db) * (tiles + 1)) * 4 + 4 * ((size_t)std::max(n, 1) * 4 + 256) + 4096;
}

// keys_out may be null: the sorted keys are not wanted (saves the last pass's key stores).  `scratch` provides the
// intermediate buffers and the histograms (released by the caller's mark).
int sort_pairs_u32(const uint32_t *keys_in, uint32_t *keys_out, const int32_t *vals_in,
                   int32_t *vals_out, int n, int bits, Arena &scratch, hipStream_t s, bool descending,
                   const int32_t *n_dev) {
  if (n <= 0) return D3D_OK;
  int passes, db;
  rs_layout(bits, passes, db);
  const int n_tiles = (n + kRsTile - 1) / kRsTile;
  D3D_ALLOC(hist, uint32_t, scratch, ((size_t)n_tiles + 1) << db);
  uint32_t *totals = hist + ((size_t)n_tiles << db);
  uint32_t *ktmp[2] = {nullptr, nullptr};
  int32_t *vtmp[2] = {nullptr, nullptr};
  for (int j = 0; j < std::min(2, passes - 1); j++) {
    D3D_ALLOC(kt, uint32_t, scratch, n);
    D3D_ALLOC(vt, int32_t, scratch, n);
    ktmp[j] = kt;
    vtmp[j] = vt;
  }
  const uint32_t *ksrc = keys_in;
  const int32_t *vsrc = vals_in;
  for (int p = 0; p < passes; p++) {
    const bool last = p == passes - 1;
    uint32_t *kdst = last ? keys_out : ktmp[p & 1];
    int32_t *vdst = last ? vals_out : vtmp[p & 1];
    if (db == 8) rs_pass<8>(ksrc, vsrc, n, n_tiles, db * p, bits, descending, hist, totals, kdst, vdst, s, n_dev);
    else if (db == 9) rs_pass<9>(ksrc, vsrc, n, n_tiles, db * p, bits, descending, hist, totals, kdst, vdst, s, n_dev);
    else rs_pass<10>(ksrc, vsrc, n, n_tiles, db * p, bits, descending, hist, totals, kdst, vdst, s, n_dev);
    ksrc = kdst;
    vsrc = vdst;
  }
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

// 0xFF fill of hash tables and rulebook arrays.  hipMemsetAsync's fill kernel reaches ~0.3 TB/s on the 12-16 MB arrays
// of the fine levels (53 us for a 16 MB table); 16-byte stores from enough workgroups run at HBM speed.
__global__ __launch_bounds__(256) void k_fill_ones(uint4 *__restrict__ p, size_t n16) {
  D3D_SIDE_PRIO();
  const uint4 v = make_uint4(~0u, ~0u, ~0u, ~0u);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}
hipError_t fill_ones(void *ptr, size_t bytes, hipStream_t s) {
  if (bytes < ((size_t)1 << 18) || ((uintptr_t)ptr & 15)) return hipMemsetAsync(ptr, 0xFF, bytes, s);
  const size_t n16 = bytes / 16;
  const unsigned blocks = (unsigned)std::min<size_t>((n16 + 1023) / 1024, 256 * 16);
  hipLaunchKernelGGL(k_fill_ones, dim3(blocks), dim3(256), 0, s, (uint4 *)ptr, n16);
  if (bytes & 15) return hipMemsetAsync((char *)ptr + n16 * 16, 0xFF, bytes & 15, s);
  return hipGetLastError();
}

}  // namespace d3d

using namespace d3d;

extern "C" {

size_t d3d_sort_scratch_bytes(int n, int bits) { return sort_scratch_bytes(n, bits); }
int d3d_sort_pairs(const uint32_t *keys, const int32_t *vals, int n, int bits, int descending, uint32_t *keys_out,
                   int32_t *vals_out, void *scratch, size_t scratch_bytes, void *stream) {
  D3D_REQUIRE(n >= 0 && bits >= 1 && bits <= 32, "d3d_sort_pairs: bad arguments");
  if (n == 0) return D3D_OK;
  D3D_REQUIRE(keys && vals && vals_out && scratch, "d3d_sort_pairs: null pointer");
  D3D_REQUIRE(scratch_bytes >= sort_scratch_bytes(n, bits), "d3d_sort_pairs: scratch too small");
  Arena A = scratch_arena(scratch, scratch_bytes);
  return sort_pairs_u32(keys, keys_out, vals, vals_out, n, bits, A, (hipStream_t)stream, descending != 0);
}

}  // extern "C"
