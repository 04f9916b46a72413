// Rulebook plans: submanifold neighbour probes, the grouping sort of the rows, the transposed tables, and the calls
// that prepare, count and export them.
#include "grid_internal.h"

namespace d3d {

// a4. Submanifold neighbour probes (SubmanifoldConvolutionRules.h:13-45).  A 256-thread block owns 64
// output sites; its 64*K probes are spread over the threads (independent loads in flight), the [site][k]
// table is written coalesced, and the per-site offset masks are assembled in LDS.
// sort key of a plan row: (number of offsets << K) | offset mask (K > 27: the mask alone); the mask is its low K bits.
// The radix form of finalize_plan sorts ONLY those low K bits, descending and stable: rows come out by descending mask
// VALUE (rows with equal masks together, in site order), not by number of offsets -- the bits above the mask are carried
// but never sorted.  (The single-workgroup form has a key of its own, k_plan_small.)
__device__ __forceinline__ uint32_t plan_key(uint32_t m, int K) { return K <= 27 ? (((uint32_t)__popc(m) << K) | m) : m; }
__device__ __forceinline__ uint32_t plan_key_mask(uint32_t key, int K) { return K <= 27 ? (key & ((1u << K) - 1u)) : key; }

static constexpr int kNbrSites = 64;
// n_dev (may be null): the site count on the device, for a launch sized by an upper bound before the count is known
__global__ __launch_bounds__(256) void k_subm_nbr(const int32_t *__restrict__ loc, int n, int fx, int fy,
                                                  int fz, const HashEntry *__restrict__ tab, int cap,
                                                  int32_t *__restrict__ nbr, uint32_t *__restrict__ mask,
                                                  const int32_t *__restrict__ n_dev) {
  D3D_SIDE_PRIO();
  __shared__ uint32_t smask[kNbrSites];
  __shared__ int32_t sloc[kNbrSites * 4];
  const int K = fx * fy * fz;
  const int s0 = blockIdx.x * kNbrSites;
  if (n_dev) n = *n_dev;
  if (s0 >= n) return;
  const int ns = min(kNbrSites, n - s0);
  if (threadIdx.x < kNbrSites) smask[threadIdx.x] = 0;
  for (int e = threadIdx.x; e < ns * 4; e += 256) sloc[e] = loc[(size_t)s0 * 4 + e];
  __syncthreads();
  for (int e = threadIdx.x; e < ns * K; e += 256) {
    const int ls = e / K, k = e % K;
    const int dz = k % fz, dy = (k / fz) % fy, dx = k / (fz * fy);
    const int x = sloc[ls * 4] - fx / 2 + dx, y = sloc[ls * 4 + 1] - fy / 2 + dy, z = sloc[ls * 4 + 2] - fz / 2 + dz;
    int v = -1;
    if (x >= 0 && y >= 0 && z >= 0) v = hash_find(tab, cap, pack_key(sloc[ls * 4 + 3], x, y, z));
    nbr[(size_t)s0 * K + e] = v;
    if (v >= 0) atomicOr(&smask[ls], 1u << k);
  }
  __syncthreads();
  // the row's SORT KEY (popcount above the mask, plan_key): finalize_plan sorts its low K bits, the mask
  if (threadIdx.x < ns) mask[s0 + threadIdx.x] = plan_key(smask[threadIdx.x], K);
}

// The same table for an odd-sized filter with HALF the probes: site j is the neighbour of site i at offset k exactly when
// i is the neighbour of j at the mirrored offset K-1-k, so only the offsets before the centre are probed and every hit is
// written twice (nbr[i][k] = j, nbr[j][K-1-k] = i).  `nbr` is pre-filled with -1 and `mask` with 0 by the caller (the
// offsets after the centre of a site are written only by their partners); the masks are OR-ed together with atomics
// (order independent).  On the fine levels 9 of 10 probes find nothing, so the second writes are few: 12.5 M probes
// become 6 M at level 0 for 0.5 M scattered stores.
__global__ __launch_bounds__(256) void k_subm_nbr_sym(const int32_t *__restrict__ loc, int n, int fx, int fy, int fz,
                                                      const HashEntry *__restrict__ tab, int cap,
                                                      int32_t *__restrict__ nbr, uint32_t *__restrict__ mask,
                                                      const int32_t *__restrict__ n_dev) {
  D3D_SIDE_PRIO();
  __shared__ uint32_t smask[kNbrSites];
  __shared__ int32_t sloc[kNbrSites * 4];
  const int K = fx * fy * fz, H = K / 2;       // offsets 0 .. H-1 are probed, H is the site itself
  const int s0 = blockIdx.x * kNbrSites;
  if (n_dev) n = *n_dev;
  if (s0 >= n) return;
  const int ns = min(kNbrSites, n - s0);
  if (threadIdx.x < kNbrSites) smask[threadIdx.x] = 0;
  for (int e = threadIdx.x; e < ns * 4; e += 256) sloc[e] = loc[(size_t)s0 * 4 + e];
  __syncthreads();
  for (int e = threadIdx.x; e < ns * (H + 1); e += 256) {
    const int ls = e / (H + 1), k = e % (H + 1);
    const int self = s0 + ls;
    if (k == H) {                                // the centre offset
      nbr[(size_t)self * K + H] = self;
      atomicOr(&smask[ls], 1u << H);
      continue;
    }
    const int dz = k % fz, dy = (k / fz) % fy, dx = k / (fz * fy);
    const int x = sloc[ls * 4] - fx / 2 + dx, y = sloc[ls * 4 + 1] - fy / 2 + dy, z = sloc[ls * 4 + 2] - fz / 2 + dz;
    int v = -1;
    if (x >= 0 && y >= 0 && z >= 0) v = hash_find(tab, cap, pack_key(sloc[ls * 4 + 3], x, y, z));
    if (v >= 0) {
      nbr[(size_t)self * K + k] = v;
      nbr[(size_t)v * K + (K - 1 - k)] = self;
      atomicOr(&smask[ls], 1u << k);
      atomicOr(&mask[v], 1u << (K - 1 - k));
    }
  }
  __syncthreads();
  if (threadIdx.x < ns) atomicOr(&mask[s0 + threadIdx.x], smask[threadIdx.x]);
}
// The neighbour table of a submanifold rulebook: nbr[n][K] and the rows' offset masks (the low K bits of the sort key).
// The half-probe form pays two fills: measured rulebook builds 0.285 -> 0.230 ms at 462 k sites, 0.245 -> 0.208 at 371 k,
// 0.113 -> 0.130 at 193 k, 0.084 -> 0.104 at 57 k.
static constexpr int kSymMinSites = 262144;
// d3d_subm_probe_mode: 0 automatic (the site threshold above), 1 never the half-probe form, 2 wherever the filter allows
static int g_subm_probe_mode = 0;
bool subm_nbr_is_sym(int n_bound, const int *filt) {
  const int K = filt[0] * filt[1] * filt[2];
  if (!((filt[0] & 1) && (filt[1] & 1) && (filt[2] & 1) && K > 1) || g_subm_probe_mode == 1) return false;
  return g_subm_probe_mode == 2 || n_bound >= kSymMinSites;
}
// the two fills the half-probe form needs (table -1, masks 0); a caller may run them ahead of time on another stream
int subm_nbr_prefill(int n_bound, const int *filt, int32_t *nbr, uint32_t *mask, hipStream_t s) {
  const int K = filt[0] * filt[1] * filt[2];
  D3D_HIP_CHECK(fill_ones(nbr, sizeof(int32_t) * ((size_t)n_bound * K + 1), s));
  D3D_HIP_CHECK(hipMemsetAsync(mask, 0, sizeof(uint32_t) * (size_t)n_bound, s));
  return D3D_OK;
}
// sym: the caller's subm_nbr_is_sym decision (taken once per build: a prefill made ahead of time must match the launch)
int launch_subm_nbr(const int32_t *loc, int n_bound, const int *filt, const HashEntry *tab, int cap, int32_t *nbr,
                    uint32_t *mask, const int32_t *n_dev, hipStream_t s, bool sym, bool prefilled) {
  if (n_bound <= 0) return D3D_OK;
  if (sym) {
    if (!prefilled)
      if (int rc = subm_nbr_prefill(n_bound, filt, nbr, mask, s)) return rc;
    hipLaunchKernelGGL(k_subm_nbr_sym, grid1d(n_bound, kNbrSites), dim3(256), 0, s, loc, n_bound, filt[0], filt[1], filt[2],
                       tab, cap, nbr, mask, n_dev);
  } else {
    hipLaunchKernelGGL(k_subm_nbr, grid1d(n_bound, kNbrSites), dim3(256), 0, s, loc, n_bound, filt[0], filt[1], filt[2], tab,
                       cap, nbr, mask, n_dev);
  }
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

// ------------------------------------------------------------------------------------------
// d3d_plan_last_form: how the calling thread's most recently ENQUEUED plan was built (host stores only).  family 1
// identity, 2 single-workgroup sort, 3 radix sort, 4 radix sort enqueued by an upper bound with the count on the device
// (0: an empty plan, nothing launched); masks 0 computed in the finalisation / 1 handed in by the probes; probe 0 none,
// 1 plain, 2 half-probe; K, n_rows, n_bound, n_blk; passes and digit bits of the radix layout; grid 0 no grid build,
// 1 k_conv_grid_small, 2 the tiled chain, 3 an empty level.  Probe and grid are what the caller of finalize_plan did
// before it: left in t_plan_ctx and consumed by the record.
static constexpr int kPlanFormFields = 10;
static thread_local int t_plan_last_form[kPlanFormFields] = {};
thread_local int t_plan_ctx[2] = {0, 0};   // probe, grid of the plan about to be finalised
void plan_record(int family, int masks, int probe, int K, int n_rows, int n_bound, int n_blk, int passes, int db,
                 int grid) {
  const int f[kPlanFormFields] = {family, masks, probe, K, n_rows, n_bound, n_blk, passes, db, grid};
  std::copy(f, f + kPlanFormFields, t_plan_last_form);
}

// Plan finalisation: per-row offset masks, sort rows by mask, transpose, block masks.
__global__ void k_row_mask(const int32_t *__restrict__ nbr, int n, int K, uint32_t *mask) {
  D3D_SIDE_PRIO();
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t m = 0;
  for (int k = 0; k < K; k++) m |= (nbr[(size_t)i * K + k] >= 0 ? 1u : 0u) << k;
  mask[i] = plan_key(m, K);
}
// number of rules of a plan = valid entries of nbrT; only run when somebody asks for the MAC count
__global__ __launch_bounds__(256) void k_count_rules(const int32_t *__restrict__ nbrT, long total,
                                                     unsigned long long *n_rules) {
  D3D_SIDE_PRIO();
  __shared__ int wsum[4];
  int c = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
    c += nbrT[i] >= 0;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(n_rules, (unsigned long long)(wsum[0] + wsum[1] + wsum[2] + wsum[3]));
}
// nbr[row][K] (row-major, site order) -> nbrT[K][npos] in plan order, through an LDS tile: a workgroup
// owns kTP consecutive plan positions, reads their K-entry rows as contiguous 4K-byte runs and writes
// kTP-entry runs of every offset's column.  The same pass pads rows[] to npos with -1 and derives the
// per-block offset masks (ballot over the 32 positions of a block), so that the plan needs one launch
// after the sort.  HBM-bound: 2 * npos * K * 4 bytes.
static constexpr int kTP = 128;
// n_dev (may be null): the row count on the device; the launch is then sized by an upper bound and the layout (row
// stride npos of nbrT) is derived from the true count, exactly as a launch that knew it would have laid it out
__global__ __launch_bounds__(256) void k_plan_finish(const int32_t *__restrict__ nbr, int32_t *__restrict__ rows,
                                                     int n_rows, int npos, int K, int32_t *__restrict__ nbrT,
                                                     uint32_t *__restrict__ blkmask, const int32_t *__restrict__ n_dev) {
  D3D_SIDE_PRIO();
  extern __shared__ int32_t tile[];  // [kTP][S], S odd
  __shared__ int32_t rloc[kTP];
  __shared__ uint32_t bm[kTP / 32];
  const int S = K | 1;
  const int p0 = blockIdx.x * kTP;
  if (n_dev) {
    n_rows = *n_dev;
    npos = ((n_rows + 31) / 32) * 32;
    if (p0 >= npos) return;
  }
  const int np = min(kTP, npos - p0);  // multiple of 32
  if (threadIdx.x < kTP) {
    const int p = p0 + threadIdx.x;
    int r = -1;
    if (p < n_rows)
      r = rows[p];
    else if (p < npos)
      rows[p] = -1;
    rloc[threadIdx.x] = r;
  }
  if (threadIdx.x < kTP / 32) bm[threadIdx.x] = 0;
  __syncthreads();
  for (int idx = threadIdx.x; idx < np * K; idx += 256) {
    const int p = idx / K, k = idx - p * K;
    const int r = rloc[p];
    tile[p * S + k] = r >= 0 ? nbr[(size_t)r * K + k] : -1;
  }
  __syncthreads();
  // np is a multiple of 32 and 256 a multiple of 64: a wave covers two whole blocks of one offset
  for (int idx = threadIdx.x; idx < kTP * K; idx += 256) {
    const int k = idx / kTP, p = idx - k * kTP;
    int v = -1;
    if (p < np) {
      v = tile[p * S + k];
      nbrT[(size_t)k * npos + p0 + p] = v;
    }
    const unsigned long long bal = __ballot(v >= 0);
    if ((threadIdx.x & 63) == 0) {
      if (bal & 0xffffffffull) atomicOr(&bm[p >> 5], 1u << k);
      if (bal >> 32) atomicOr(&bm[(p >> 5) + 1], 1u << k);
    }
  }
  __syncthreads();
  if (threadIdx.x < np / 32) blkmask[p0 / 32 + threadIdx.x] = bm[threadIdx.x];
}
void launch_plan_finish(const int32_t *nbr, int32_t *rows, int n_rows, int npos, int K, int32_t *nbrT, uint32_t *blkmask,
                        const int32_t *n_dev, hipStream_t s) {
  hipLaunchKernelGGL(k_plan_finish, dim3((npos + kTP - 1) / kTP), dim3(256), (size_t)kTP * (K | 1) * sizeof(int32_t), s, nbr,
                     rows, n_rows, npos, K, nbrT, blkmask, n_dev);
}

// Row masks and the grouping sort of a SMALL plan (<= kSmallMax rows) in one single-workgroup launch (k_plan_finish
// follows).  The ten launches of 3-6 us each it replaces (mask, key, 7 radix-sort kernels) cost more in launch
// latency than the work; small layers are half of a network's plans.
// Sort: stable LSD radix, 4 passes of 4 bits on a 16-bit key in LDS; thread t owns a contiguous chunk of rows and
// the counter column cnt[digit][t], so ranks need no atomics and the order is deterministic.
// key16 = (K - popcount) << 11 | (mask if K <= 11 else an 11-bit hash of it): heaviest rows first, equal masks
// adjacent (hash collisions only cost a little padding).
static constexpr int kSmallMax = 8192;  // (16384 rows / 512 threads measured slower than the rocPRIM path)
static constexpr int kSmallThreads = 1024;
__global__ __launch_bounds__(kSmallThreads) void k_plan_small(const int32_t *__restrict__ nbr,
                                                              const uint32_t *__restrict__ mask_in, int n_rows,
                                                              int K, int32_t *__restrict__ rows) {
  D3D_SIDE_PRIO();
  __shared__ uint32_t buf[2][kSmallMax];          // (key16 << 16) | row
  __shared__ uint16_t cnt[16 * kSmallThreads];    // [digit][thread]
  __shared__ uint32_t wsum[kSmallThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = (n_rows + kSmallThreads - 1) / kSmallThreads;
  const int i0 = min(n_rows, tid * per), i1 = min(n_rows, i0 + per);
  for (int i = i0; i < i1; i++) {
    uint32_t m;
    if (mask_in)
      m = plan_key_mask(mask_in[i], K);
    else {
      m = 0;
      for (int k = 0; k < K; k++) m |= (nbr[(size_t)i * K + k] >= 0 ? 1u : 0u) << k;
    }
    const uint32_t lo = K <= 11 ? m : (m * 0x9E3779B1u) >> 21;
    buf[0][i] = ((((uint32_t)(K - __popc(m)) << 11) | lo) << 16) | (uint32_t)i;
  }
  __syncthreads();
  for (int pass = 0; pass < 4; pass++) {
    const uint32_t *src = buf[pass & 1];
    uint32_t *dst = buf[(pass & 1) ^ 1];
    const int shift = 16 + 4 * pass;
#pragma unroll
    for (int d = 0; d < 16; d++) cnt[d * kSmallThreads + tid] = 0;
    for (int i = i0; i < i1; i++) cnt[((src[i] >> shift) & 15u) * kSmallThreads + tid]++;
    __syncthreads();
    // exclusive scan of the flattened [digit][thread] counters: thread t owns entries [16 t, 16 t + 16)
    uint32_t loc[16], sum = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      loc[j] = sum;
      sum += cnt[tid * 16 + j];
    }
    uint32_t inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t t = __shfl_up(inc, d, 64);
      if (lane >= d) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t base = inc - sum;
    for (int w = 0; w < wave; w++) base += wsum[w];
#pragma unroll
    for (int j = 0; j < 16; j++) cnt[tid * 16 + j] = (uint16_t)(base + loc[j]);
    __syncthreads();
    for (int i = i0; i < i1; i++) {
      const uint32_t v = src[i];
      dst[cnt[((v >> shift) & 15u) * kSmallThreads + tid]++] = v;
    }
    __syncthreads();
  }
  const uint32_t *ord = buf[0];  // 4 passes: back in buffer 0
  for (int p = tid; p < n_rows; p += kSmallThreads) rows[p] = (int32_t)(ord[p] & 0xffffu);
}

// the persistent arrays of a plan of n_rows rows and filter volume K, taken from `A` in this order
static int alloc_plan(Arena &A, Plan &plan, int n_rows, int K) {
  plan.K = K;
  plan.n_rows = n_rows;
  plan.n_blk = (n_rows + 31) / 32;
  const size_t npos = (size_t)plan.n_blk * 32;
  D3D_ALLOC(rows, int32_t, A, npos + 1);
  D3D_ALLOC(nbrT, int32_t, A, npos * K + 1);
  D3D_ALLOC(blkmask, uint32_t, A, (size_t)plan.n_blk + 1);
  plan.rows = rows;
  plan.nbrT = nbrT;
  plan.blkmask = blkmask;
  return D3D_OK;
}

// `mask_in` (may be null): per-row offset masks already computed by the caller together with the
// rule count in plan.n_rules_dev.  The rule count stays on the device until somebody asks for it.
int finalize_plan(d3d_meta *m, const int32_t *nbr, int n_rows, int K, Plan &plan, hipStream_t s,
                  uint32_t *mask_in) {
  const int probe = t_plan_ctx[0], grid = t_plan_ctx[1];   // consumed whatever happens below
  t_plan_ctx[0] = t_plan_ctx[1] = 0;
  D3D_REQUIRE(K >= 1 && K <= 32, "filter volume %d not supported (1..32)", K);
  Arena &A = lane_arena(m, s);
  if (int rc = alloc_plan(A, plan, n_rows, K)) return rc;
  const int npos = plan.n_blk * 32;
  int32_t *rows = plan.rows, *nbrT = plan.nbrT;
  uint32_t *blkmask = plan.blkmask;
  plan.n_rules = n_rows == 0 ? 0 : -1;
  if (n_rows == 0) {
    plan_record(0, 0, probe, K, 0, 0, 0, 0, 0, grid);
    return D3D_OK;
  }
  if (n_rows <= kSmallMax) {
    plan_record(2, mask_in ? 1 : 0, probe, K, n_rows, n_rows, plan.n_blk, 0, 0, grid);
    hipLaunchKernelGGL(k_plan_small, dim3(1), dim3(kSmallThreads), 0, s, nbr, mask_in, n_rows, K, rows);
    launch_plan_finish(nbr, rows, n_rows, npos, K, nbrT, blkmask, nullptr, s);
    D3D_LAUNCH_CHECK();
    return D3D_OK;
  }
  size_t mark = A.used;
  uint32_t *mask = mask_in;
  if (!mask) {
    mask = A.get<uint32_t>(n_rows);
    if (!mask) {
      set_error("metadata arena exhausted while finalising a rulebook");
      return D3D_ERR_NOMEM;
    }
    hipLaunchKernelGGL(k_row_mask, grid1d(n_rows), dim3(256), 0, s, nbr, n_rows, K, mask);
  }
  // Exact, STABLE sort by the mask value alone (descending; the popcount above it in the key is not sorted): rows of a
  // mask class are contiguous and stay in site-id order, i.e. consecutive positions of a block read (centre offset) and
  // write nearly consecutive feature rows.  Measured alternative: grouping the rows
  // by hashing their masks into a class table (4 launches instead of ~19, same executed / useful steps within 10 %)
  // hands out positions by atomics, loses that order, and made the 64 -> 64 convolutions 29 % slower.  Leaving the
  // k = s = 2 plans unsorted (absent gathers cost no memory traffic) saves four sorts per building and costs the
  // strided convolutions 0.25 ms of zero tiles: 6.45 against 6.37 ms per building.
  D3D_REQUIRE(m->iota && n_rows <= m->iota_n, "finalize_plan: %d rows exceed the input layer's %d points", n_rows, m->iota_n);
  {
    int passes, db;
    rs_layout(std::min(K, 32), passes, db);
    plan_record(3, mask_in ? 1 : 0, probe, K, n_rows, n_rows, plan.n_blk, passes, db, grid);
  }
  int rc = sort_pairs_u32(mask, nullptr, m->iota, rows, n_rows, std::min(K, 32), A, s, true, nullptr);   // low K bits: the mask
  if (rc) return rc;
  launch_plan_finish(nbr, rows, n_rows, npos, K, nbrT, blkmask, nullptr, s);
  D3D_LAUNCH_CHECK();
  A.used = mark;  // scratch released (stream-ordered reuse)
  return D3D_OK;
}

// reads the rule count back (one stream sync) the first time it is asked for
int plan_rules(d3d_meta *m, Plan &p, hipStream_t s, long *out) {
  if (p.n_rules < 0) {
    Arena &A = m->feat_arena;   // may run on the feature stream while geometry is built on another one
    size_t mark = A.used;
    D3D_ALLOC(cnt, unsigned long long, A, 1);
    D3D_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long), s));
    const long total = (long)p.n_blk * 32 * p.K;
    hipLaunchKernelGGL(k_count_rules, dim3((unsigned)std::min<long>(1024, (total + 255) / 256)), dim3(256), 0, s,
                       p.nbrT, total, cnt);
    D3D_LAUNCH_CHECK();
    A.used = mark;
    // (a pinned word of its own: the geometry thread may be reading a site count back at the same time)
    D3D_HIP_CHECK(hipMemcpyAsync(&m->host_words[8], cnt, sizeof(long), hipMemcpyDeviceToHost, s));
    D3D_HIP_CHECK(hipStreamSynchronize(s));
    p.n_rules = m->host_words[8];
  }
  *out = p.n_rules;
  return D3D_OK;
}

__global__ void k_identity_plan(int32_t *rows, int32_t *nbrT, uint32_t *blkmask, int n, int npos, int n_blk) {
  D3D_SIDE_PRIO();
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < npos) {
    int v = i < n ? i : -1;
    rows[i] = v;
    nbrT[i] = v;
  }
  if (i < n_blk) blkmask[i] = 1u;
}

const Plan *find_plan(d3d_meta *m, int kind, const int *in_size, const int *filt, const int *stride) {
  D3D_LOCK(m);
  auto it = m->plans.find(make_key(kind, in_size, filt, stride));
  return it == m->plans.end() ? nullptr : &it->second;
}

int get_deconv_plan(d3d_meta *m, const int *fine_size, const int *filt, const int *stride,
                    hipStream_t s, const Plan **out) {
  PlanKey key = make_key(2, fine_size, filt, stride);
  std::map<PlanKey, Plan>::iterator it;
  std::map<PlanKey, StridedRaw>::iterator raw;
  bool have, have_raw;
  {
    D3D_LOCK(m);
    it = m->plans.find(key);
    have = it != m->plans.end();
    raw = m->strided_raw.find(make_key(1, fine_size, filt, stride));
    have_raw = raw != m->strided_raw.end();
  }
  if (!have) {
    D3D_REQUIRE_STATE(have_raw, "deconvolution: no strided rulebook for this (size, filter, stride); run the "
                                "matching convolution (d3d_conv_prepare) first");
    Plan p;
    int K = filt[0] * filt[1] * filt[2];
    int rc = finalize_plan(m, raw->second.nbr_dec, raw->second.n_in, K, p, s, nullptr);
    if (rc) return rc;
    D3D_LOCK(m);
    auto go = m->grids.find(raw->second.out_size);
    p.n_in = go == m->grids.end() ? 0 : go->second.n;   // gathers from the coarse tensor
    it = m->plans.emplace(key, p).first;
  }
  *out = &it->second;
  return D3D_OK;
}

__global__ void k_export_plan(const int32_t *__restrict__ nbrT, const int32_t *__restrict__ rows,
                              int npos, int K, int swap, int32_t *triples, long capacity,
                              unsigned long long *count) {
  D3D_SIDE_PRIO();
  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)npos * K) return;
  int k = (int)(t / npos), p = (int)(t % npos);
  int src = nbrT[t];
  if (src < 0) return;
  unsigned long long w = atomicAdd(count, 1ull);
  if ((long)w < capacity) {
    triples[w * 3 + 0] = swap ? rows[p] : src;
    triples[w * 3 + 1] = swap ? src : rows[p];
    triples[w * 3 + 2] = k;
  }
}

struct CapGuard {  // temporarily shrinks the arena so that a raw table can sit at its far end
  Arena &a;
  size_t save;
  CapGuard(Arena &a_, size_t new_cap) : a(a_), save(a_.cap) { a.cap = new_cap; }
  ~CapGuard() { a.cap = save; }
};

}  // namespace d3d

using namespace d3d;

extern "C" {

int d3d_subm_prepare(d3d_meta *m, const int *size, const int *filt, void *stream, long *n_rules_host) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && size && filt, "null argument");
  PlanKey key = make_key(0, size, filt, nullptr);
  std::map<PlanKey, Plan>::iterator it;
  bool have;
  {
    D3D_LOCK(m);
    it = m->plans.find(key);
    have = it != m->plans.end();
  }
  if (!have) {
    Grid *g = find_grid(m, size);
    D3D_REQUIRE_STATE(g, "submanifold rulebook: no grid of spatial size [%d,%d,%d]", size[0], size[1], size[2]);
    int K = filt[0] * filt[1] * filt[2];
    D3D_REQUIRE(filt[0] > 0 && filt[1] > 0 && filt[2] > 0 && K <= 32, "filter volume %d not supported", K);
    Plan p;
    Arena &A = lane_arena(m, s);
    // raw table lives above the plan's persistent arrays: allocate persistent part first
    // (finalize_plan), so stage the raw table at the far end of the arena instead.
    size_t raw_bytes = ((size_t)g->n * K + 1) * sizeof(int32_t);
    if (A.used + 2 * raw_bytes + (size_t)g->n * 16 + (1 << 20) > A.cap) {
      set_error("metadata arena exhausted while building a submanifold rulebook");
      return D3D_ERR_NOMEM;
    }
    if (K == 1) {
      // 1x1x1 submanifold convolution: every site is its own (only) neighbour -> identity rulebook
      if (int rc = alloc_plan(A, p, g->n, 1)) return rc;
      p.n_rules = g->n;
      const int npos = p.n_blk * 32;
      if (npos) hipLaunchKernelGGL(k_identity_plan, grid1d(npos), dim3(256), 0, s, p.rows, p.nbrT, p.blkmask, g->n, npos, p.n_blk);
      D3D_LAUNCH_CHECK();
      plan_record(1, 0, 0, 1, g->n, g->n, p.n_blk, 0, 0, 0);
    } else if (m->pre_nbr && s == m->pre_stream && g->size[0] == m->in_size[0] && g->size[1] == m->in_size[1] &&
               g->size[2] == m->in_size[2] && filt[0] == m->pre_filt[0] && filt[1] == m->pre_filt[1] &&
               filt[2] == m->pre_filt[2]) {
      // the table d3d_input_layer_build_prefetch started on this stream
      t_plan_ctx[0] = m->pre_sym ? 2 : 1;
      int rc = finalize_plan(m, m->pre_nbr, g->n, K, p, s, m->pre_mask);
      if (rc) return rc;
    } else {
      int32_t *nbr = (int32_t *)(A.base + ((A.cap - raw_bytes) & ~size_t(255)));
      uint32_t *mask = (uint32_t *)((char *)nbr - (((size_t)g->n * 4 + 511) & ~size_t(255)));
      const bool sym = subm_nbr_is_sym(g->n, filt);
      if (int rc2 = launch_subm_nbr(g->loc, g->n, filt, g->tab, g->cap, nbr, mask, nullptr, s, sym)) return rc2;
      t_plan_ctx[0] = sym ? 2 : 1;
      int rc;
      {
        CapGuard guard(A, (size_t)((char *)mask - A.base) & ~size_t(255));
        rc = finalize_plan(m, nbr, g->n, K, p, s, mask);
      }
      if (rc) return rc;
    }
    p.n_in = g->n;
    D3D_LOCK(m);
    it = m->plans.emplace(key, p).first;
  }
  if (n_rules_host) return plan_rules(m, it->second, s, n_rules_host);
  return D3D_OK;
}

int d3d_deconv_prepare(d3d_meta *m, const int *in_size, const int *out_size, const int *filt,
                       const int *stride, void *stream, long *n_rules_host) {
  (void)in_size;
  D3D_REQUIRE(m && out_size && filt && stride, "null argument");
  const Plan *p = nullptr;
  int rc = get_deconv_plan(m, out_size, filt, stride, (hipStream_t)stream, &p);
  if (rc) return rc;
  if (n_rules_host) return plan_rules(m, *const_cast<Plan *>(p), (hipStream_t)stream, n_rules_host);
  return D3D_OK;
}

int d3d_export_rules(d3d_meta *m, int kind, const int *in_size, const int *filt, const int *stride,
                     int32_t *triples, long capacity, long *n_host, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && in_size && filt && n_host && (kind == 0 || kind == 1 || kind == 2), "bad arguments");
  const Plan *p = find_plan(m, kind, in_size, filt, kind == 0 ? nullptr : stride);
  D3D_REQUIRE_STATE(p, "export: rulebook not built");
  *n_host = 0;
  if (p->n_rows == 0) return D3D_OK;
  Arena &A = lane_arena(m, s);
  size_t mark = A.used;
  D3D_ALLOC(cnt, unsigned long long, A, 1);
  D3D_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long), s));
  const int npos = p->n_blk * 32;
  // kind 2 (deconvolution plan): rows are fine sites = the rule's "in" side of the strided conv
  hipLaunchKernelGGL(k_export_plan, grid1d((long)npos * p->K), dim3(256), 0, s, p->nbrT, p->rows, npos, p->K, kind == 2 ? 1 : 0, triples, capacity, cnt);
  D3D_LAUNCH_CHECK();
  D3D_HIP_CHECK(hipMemcpyAsync(&m->host_words[9], cnt, sizeof(long), hipMemcpyDeviceToHost, s));
  D3D_HIP_CHECK(hipStreamSynchronize(s));
  *n_host = m->host_words[9];
  A.used = mark;
  return D3D_OK;
}

// debug / measurement: how well a plan's blocks are grouped.  executed = sum over blocks of 32 * popcount(block mask)
// (row-offset steps the convolution runs), useful = rules.  executed / useful = 1 is a perfect grouping.
int d3d_plan_stats(d3d_meta *m, int kind, const int *in_size, const int *filt, const int *stride, long *n_blocks_host,
                   long *executed_host, long *rules_host, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && in_size && filt && n_blocks_host && executed_host && rules_host, "bad arguments");
  Plan *p = const_cast<Plan *>(find_plan(m, kind, in_size, filt, kind == 0 ? nullptr : stride));
  D3D_REQUIRE_STATE(p, "plan_stats: rulebook not built");
  *n_blocks_host = p->n_blk;
  *executed_host = 0;
  int rc = plan_rules(m, *p, s, rules_host);
  if (rc || p->n_blk == 0) return rc;
  std::vector<uint32_t> bm(p->n_blk);
  D3D_HIP_CHECK(hipMemcpyAsync(bm.data(), p->blkmask, sizeof(uint32_t) * p->n_blk, hipMemcpyDeviceToHost, s));
  D3D_HIP_CHECK(hipStreamSynchronize(s));
  long ex = 0;
  for (uint32_t v : bm) ex += 32L * __builtin_popcount(v);
  *executed_host = ex;
  return D3D_OK;
}

int d3d_plan_export(d3d_meta *m, int kind, const int *in_size, const int *filt, const int *stride, int32_t *rows,
                    int32_t *nbrT, uint32_t *blkmask, int *dims_host, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && in_size && filt && dims_host && (kind == 0 || kind == 1 || kind == 2), "bad arguments");
  const Plan *p = find_plan(m, kind, in_size, filt, kind == 0 ? nullptr : stride);
  D3D_REQUIRE_STATE(p, "export: rulebook not built");
  dims_host[0] = p->K;
  dims_host[1] = p->n_rows;
  dims_host[2] = p->n_in;
  dims_host[3] = p->n_blk;
  const size_t npos = (size_t)p->n_blk * 32;
  if (npos == 0) return D3D_OK;
  if (rows) D3D_HIP_CHECK(hipMemcpyAsync(rows, p->rows, sizeof(int32_t) * npos, hipMemcpyDeviceToDevice, s));
  if (nbrT) D3D_HIP_CHECK(hipMemcpyAsync(nbrT, p->nbrT, sizeof(int32_t) * npos * p->K, hipMemcpyDeviceToDevice, s));
  if (blkmask) D3D_HIP_CHECK(hipMemcpyAsync(blkmask, p->blkmask, sizeof(uint32_t) * p->n_blk, hipMemcpyDeviceToDevice, s));
  return D3D_OK;
}

int d3d_plan_last_form(int *out, int n) {
  for (int i = 0; out && i < n && i < kPlanFormFields; i++) out[i] = t_plan_last_form[i];
  std::fill(t_plan_last_form, t_plan_last_form + kPlanFormFields, 0);
  return kPlanFormFields;
}

int d3d_subm_probe_mode(int mode) {
  const int was = g_subm_probe_mode;
  if (mode >= 0 && mode <= 2) g_subm_probe_mode = mode;
  return was;
}

}  // extern "C"
