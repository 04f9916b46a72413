// Strided grids: the output grid and raw neighbour tables of a strided convolution, for one level or a whole pyramid.
#include "grid_internal.h"

namespace d3d {

// ------------------------------------------------------------------------------------------
// a5. Strided convolution: output grid + raw neighbour tables (ConvolutionRules.h:12-34).
struct ConvGeom {
  int filt[3], stride[3], out_size[3];
  int max_out;
};
__device__ __forceinline__ bool conv_entry(const ConvGeom &g, const int32_t *p, int j, int *o,
                                           int *off) {
  int lb[3], cnt[3];
#pragma unroll
  for (int d = 0; d < 3; d++) {
    int t = p[d] - g.filt[d] + g.stride[d];
    int l = t < 0 ? 0 : t / g.stride[d];          // max(0, (in - size + stride) / stride)
    int u = min(g.out_size[d] - 1, p[d] / g.stride[d]);
    lb[d] = l;
    cnt[d] = u - l + 1;
    if (cnt[d] <= 0) return false;
  }
  if (j >= cnt[0] * cnt[1] * cnt[2]) return false;
  int jz = j % cnt[2], jy = (j / cnt[2]) % cnt[1], jx = j / (cnt[2] * cnt[1]);
  o[0] = lb[0] + jx;
  o[1] = lb[1] + jy;
  o[2] = lb[2] + jz;
  *off = ((p[0] - o[0] * g.stride[0]) * g.filt[1] + (p[1] - o[1] * g.stride[1])) * g.filt[2] +
         (p[2] - o[2] * g.stride[2]);
  return true;
}
// n_in_dev (may be null): the input site count on the device, for a launch sized by an upper bound of it
__global__ void k_conv_insert(const int32_t *__restrict__ loc, long n_entries, ConvGeom g,
                              HashEntry *tab, int cap, int32_t *eslot, const int32_t *__restrict__ n_in_dev) {
  D3D_SIDE_PRIO();
  long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n_in_dev) n_entries = (long)*n_in_dev * g.max_out;
  if (e >= n_entries) return;
  int i = (int)(e / g.max_out), j = (int)(e % g.max_out);
  const int32_t *p = loc + (size_t)i * 4;
  int o[3], off;
  if (!conv_entry(g, p, j, o, &off)) {
    eslot[e] = -1;
    return;
  }
  int slot = hash_insert(tab, cap, pack_key(p[3], o[0], o[1], o[2]));
  atomicMin(&tab[slot].first, (uint32_t)e);
  eslot[e] = slot;
}
// nbr_dec may be null (no deconvolution / backward view of this rulebook will be asked for)
__global__ void k_conv_fill(const int32_t *__restrict__ loc, long n_entries, ConvGeom g, int K,
                            const int32_t *__restrict__ eslot, const HashEntry *__restrict__ tab,
                            int32_t *nbr_fwd, int32_t *nbr_dec, const int32_t *__restrict__ n_in_dev) {
  D3D_SIDE_PRIO();
  long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n_in_dev) n_entries = (long)*n_in_dev * g.max_out;
  if (e >= n_entries || eslot[e] < 0) return;
  int i = (int)(e / g.max_out), j = (int)(e % g.max_out);
  const int32_t *p = loc + (size_t)i * 4;
  int o[3], off;
  conv_entry(g, p, j, o, &off);
  int oid = tab[eslot[e]].val;
  nbr_fwd[(size_t)oid * K + off] = i;
  if (nbr_dec) nbr_dec[(size_t)i * K + off] = oid;
}

// First-touch numbering of a strided grid's output sites without a scan over the entries: a tile of kChainTile entries
// leaves its first-touch flags as 32 ballot words and their number (k_chain_flag); k_chain_assign then sums the counts of
// the tiles before its own (a few hundred integers, no cross-workgroup waiting), ranks its flags with popcounts and writes
// site ids, coordinates and -- the last tile -- the site count, all on the device.  Two launches where a flag kernel,
// a three-kernel scan and an assignment kernel took five, and nothing the host has to read before the next level starts.
static constexpr int kChainTile = 2048;   // = 256 threads x 8 rounds; word w of a tile = its entries 64 w .. 64 w + 63
__global__ __launch_bounds__(256) void k_chain_flag(const int32_t *__restrict__ eslot, const HashEntry *__restrict__ tab,
                                                    long n_entries, int max_out, const int32_t *__restrict__ n_in_dev,
                                                    unsigned long long *__restrict__ flagbits,
                                                    int32_t *__restrict__ tile_cnt) {
  D3D_SIDE_PRIO();
  __shared__ int wcnt[4];
  if (n_in_dev) n_entries = (long)*n_in_dev * max_out;
  const long base = (long)blockIdx.x * kChainTile;
  if (base >= n_entries) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int c = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int w = j * 4 + wave;
    const long e = base + w * 64 + lane;
    bool f = false;
    if (e < n_entries) {
      const int sl = eslot[e];
      f = sl >= 0 && tab[sl].first == (uint32_t)e;
    }
    const unsigned long long bal = __ballot(f);
    if (lane == 0) flagbits[(size_t)blockIdx.x * 32 + w] = bal;
    c += __popcll(bal);
  }
  if (lane == 0) wcnt[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}
__global__ __launch_bounds__(256) void k_chain_assign(const int32_t *__restrict__ loc, long n_entries, ConvGeom g,
                                                      const int32_t *__restrict__ n_in_dev,
                                                      const int32_t *__restrict__ eslot,
                                                      const unsigned long long *__restrict__ flagbits,
                                                      const int32_t *__restrict__ tile_cnt, HashEntry *tab,
                                                      int32_t *__restrict__ loc_out, int32_t *__restrict__ n_out_dev) {
  D3D_SIDE_PRIO();
  __shared__ int red[4];
  __shared__ int wpre[33];
  __shared__ unsigned long long words[32];
  if (n_in_dev) n_entries = (long)*n_in_dev * g.max_out;
  if (n_entries <= 0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_out_dev = 0;
    return;
  }
  const int n_tiles = (int)((n_entries + kChainTile - 1) / kChainTile);
  if ((int)blockIdx.x >= n_tiles) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int part = 0;
  for (int t = threadIdx.x; t < (int)blockIdx.x; t += 256) part += tile_cnt[t];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o, 64);
  if (lane == 0) red[wave] = part;
  if (threadIdx.x < 32) {
    const unsigned long long w = flagbits[(size_t)blockIdx.x * 32 + threadIdx.x];
    words[threadIdx.x] = w;
    const int pc = __popcll(w);
    int inc = pc;
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) {
      const int t = __shfl_up(inc, d, 64);
      if (lane >= d) inc += t;
    }
    wpre[threadIdx.x] = inc - pc;
    if (threadIdx.x == 31) wpre[32] = inc;
  }
  __syncthreads();
  const int off = red[0] + red[1] + red[2] + red[3];
  const long base = (long)blockIdx.x * kChainTile;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int w = j * 4 + wave;
    const unsigned long long word = words[w];
    if (!((word >> lane) & 1ull)) continue;
    const long e = base + w * 64 + lane;
    const int id = off + wpre[w] + __popcll(word & ((1ull << lane) - 1ull));
    const int i = (int)(e / g.max_out), jj = (int)(e % g.max_out);
    const int32_t *p = loc + (size_t)i * 4;
    int o[3], offk;
    conv_entry(g, p, jj, o, &offk);
    tab[eslot[e]].val = id;
    loc_out[(size_t)id * 4 + 0] = o[0];
    loc_out[(size_t)id * 4 + 1] = o[1];
    loc_out[(size_t)id * 4 + 2] = o[2];
    loc_out[(size_t)id * 4 + 3] = p[3];
  }
  if ((int)blockIdx.x == n_tiles - 1 && threadIdx.x == 0) *n_out_dev = off + wpre[32];
}
// 0xFF fill of up to kFillSegs memory ranges in one launch (blockIdx.y = range)
static constexpr int kFillSegs = 48;
struct FillSegs {
  uint4 *ptr[kFillSegs];
  unsigned long long n16[kFillSegs];
};
__global__ __launch_bounds__(256) void k_fill_ones_multi(FillSegs f) {
  D3D_SIDE_PRIO();
  const uint4 v = make_uint4(~0u, ~0u, ~0u, ~0u);
  uint4 *__restrict__ p = f.ptr[blockIdx.y];
  const size_t n = f.n16[blockIdx.y];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}
// the site counts of the chain's levels -> a pinned host array (one system-scope release store each)
static constexpr int kChainMax = 24;
struct CountPtrs {
  const int32_t *p[kChainMax];
  int n;
};
__global__ void k_store_counts(CountPtrs c, int32_t *__restrict__ host) {
  D3D_SIDE_PRIO();
  const int i = threadIdx.x;
  if (i < c.n) __hip_atomic_store(&host[i], *c.p[i], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The whole strided-grid build of a SMALL level in one single-workgroup launch: insertion, first-touch flags, their
// exclusive scan in entry order, site numbering, and the forward / decoded rulebook fill -- what the large path spreads
// over four launches (k_conv_insert, k_chain_flag, k_chain_assign, k_conv_fill).  The coarse pyramid levels are pure
// latency (each launch a dependent step of the chain), so fewer steps is what matters; the results are the large
// path's, bit for bit.  Table and rulebook arrays already hold 0xFF (the chain's one fill launch).
// Threads keep their entries' slots in registers; table fields other threads wrote are read with agent-scope atomic
// loads (L2), never through a possibly stale L1 line.
static constexpr int kSmallGrid = 4096;                        // entries one workgroup takes (16 k: slower than the large path)
static constexpr int kSmallGridThreads = 256;                  // 4 waves: finds a slot on a busy CU (see k_plan_small)
static constexpr int kSmallGridEPT = kSmallGrid / kSmallGridThreads;
// n_in_dev (may be null): the input site count on the device (n_entries is then an upper bound); nbr_dec may be null.
__global__ __launch_bounds__(kSmallGridThreads) void k_conv_grid_small(const int32_t *__restrict__ loc, int n_entries, ConvGeom g,
                                                          int K, HashEntry *tab, int cap,
                                                          int32_t *__restrict__ loc_out, int32_t *__restrict__ nbr_fwd,
                                                          int32_t *__restrict__ nbr_dec, int32_t *__restrict__ total,
                                                          const int32_t *__restrict__ n_in_dev) {
  D3D_SIDE_PRIO();
  __shared__ int wsum[kSmallGridThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (n_in_dev) n_entries = *n_in_dev * g.max_out;
  int slot_r[kSmallGridEPT];
#pragma unroll
  for (int it = 0; it < kSmallGridEPT; it++) {
    const int e = it * kSmallGridThreads + tid;
    int slot = -1;
    if (e < n_entries) {
      const int32_t *p = loc + (size_t)(e / g.max_out) * 4;
      int o[3], off;
      if (conv_entry(g, p, e % g.max_out, o, &off)) {
        slot = hash_insert(tab, cap, pack_key(p[3], o[0], o[1], o[2]));
        atomicMin(&tab[slot].first, (uint32_t)e);
      }
    }
    slot_r[it] = slot;
  }
  __syncthreads();   // every wave's stores have reached L2 ...
  if (tid == 0) __threadfence();   // ... one agent-scope fence for the workgroup (as in k_bn_stats)
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int it = 0; it < kSmallGridEPT; it++) {
    if (it * kSmallGridThreads >= n_entries) break;                                       // block-uniform
    const int e = it * kSmallGridThreads + tid, slot = slot_r[it];
    const bool first = slot >= 0 &&
                       __hip_atomic_load(&tab[slot].first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (uint32_t)e;
    const unsigned long long bal = __ballot(first);
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kSmallGridThreads / 64; w++) {
      const int c = wsum[w];
      before += w < wave ? c : 0;
      all += c;
    }
    if (first) {
      const int id = base + before + __popcll(bal & ((1ull << lane) - 1ull));
      const int32_t *p = loc + (size_t)(e / g.max_out) * 4;
      int o[3], off;
      conv_entry(g, p, e % g.max_out, o, &off);
      __hip_atomic_store(&tab[slot].val, id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      loc_out[id * 4 + 0] = o[0];
      loc_out[id * 4 + 1] = o[1];
      loc_out[id * 4 + 2] = o[2];
      loc_out[id * 4 + 3] = p[3];
    }
    base += all;
    __syncthreads();
  }
  if (tid == 0) *total = base;
  __syncthreads();   // every wave's stores have reached L2 ...
  if (tid == 0) __threadfence();   // ... one agent-scope fence for the workgroup (as in k_bn_stats)
  __syncthreads();
#pragma unroll
  for (int it = 0; it < kSmallGridEPT; it++) {
    const int e = it * kSmallGridThreads + tid, slot = slot_r[it];
    if (slot < 0) continue;
    const int i = e / g.max_out;
    const int32_t *p = loc + (size_t)i * 4;
    int o[3], off;
    conv_entry(g, p, e % g.max_out, o, &off);
    const int oid = __hip_atomic_load(&tab[slot].val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    nbr_fwd[(size_t)oid * K + off] = i;
    if (nbr_dec) nbr_dec[(size_t)i * K + off] = oid;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Grid chain: the one builder of strided grids (+ raw rule tables) -- a whole pyramid enqueued WITHOUT a host read-back
// between the levels (the geometry thread), or a single level (d3d_conv_prepare).  Reading every new grid's site count
// back before the next level is sized costs 11 stream synchronisations per building, each with the GPU idle on that
// stream for the round trip.  Here every level is sized by an upper bound known ahead of time -- sites(out) <=
// min(entries(in), cells of the occupied box at that level), from the input grid's site count and coordinate
// extents, which arrive in ONE read-back (an input grid without known extents: the entry bound alone) -- its kernels
// read the true count from the device word the level before left, all tables get their 0xFF fill in one launch up
// front, and the counts of all levels come back together behind the last kernel (k_store_counts -> pinned words, one
// event).  Only then are the grids published and the rulebooks finalised (exact sizes), in order.
// Sites are numbered by first touch in entry order (ConvolutionRules.h:12-34), whatever the bounds and however many
// levels one call takes: tests/test_scn_gpu.py and tests/test_fullsize_gpu.py pin that numbering to the CPU oracle.
int run_grid_chain(d3d_meta *m, const std::vector<ChainSpec> &specs, hipStream_t s, std::vector<int> &n_out,
                   ChainHook on_grid, ChainHook on_done, void *hook_arg) {
  const int L = (int)specs.size();
  n_out.assign(L, 0);
  if (L == 0) return D3D_OK;
  D3D_REQUIRE(L <= kChainMax, "grid chain: %d levels (at most %d)", L, kChainMax);
  if (int rc = check_build_stream(m, s, "grid chain")) return rc;
  struct Level {
    ConvGeom geo;
    int K = 0;
    const int32_t *loc_in = nullptr;
    const int32_t *n_in_dev = nullptr;   // null: n_in_host is exact
    int n_in_host = 0, src = -1;         // src: chain level that produces the input grid, or -1
    long bound_in = 0, bound_entries = 0, bound_out = 0;
    int ext_out[4] = {0, 0, 0, 0};
    Grid go;
    int32_t *n_out_dev = nullptr, *eslot = nullptr, *tile_cnt = nullptr, *nbr_fwd = nullptr, *nbr_dec = nullptr;
    unsigned long long *flagbits = nullptr;
    bool small = false;
  };
  std::vector<Level> lv(L);
  std::map<Size3, int> made;             // output size -> chain level
  Arena &A = m->arena;
  const size_t cap_save = A.cap;
  struct Restore {                        // the raw tables sit at the far end of the lane until the rulebooks are enqueued
    Arena &a;
    size_t cap;
    ~Restore() { a.cap = cap; }
  } restore{A, cap_save};
  auto top = [&](size_t bytes) -> void * {
    bytes = (bytes + 255) & ~size_t(255);
    if (A.used + bytes + (size_t)(1 << 20) > A.cap) return nullptr;
    A.cap = (A.cap - bytes) & ~size_t(255);
    return A.base + A.cap;
  };
  FillSegs fs = {};
  int n_seg = 0;
  D3D_REQUIRE(3 * L <= kFillSegs, "grid chain: too many levels for one fill launch");
  auto add_fill = [&](void *p, size_t bytes) {   // bytes rounded up to 16 (allocations are 256-byte aligned and padded)
    fs.ptr[n_seg] = (uint4 *)p;
    fs.n16[n_seg] = (bytes + 15) / 16;
    n_seg++;
  };
  // A level that cannot be planned (bad sizes, missing input grid, arena exhausted) ends the chain in front of it: the
  // levels before it are built and published as usual, then its error is returned (what a caller that prepares the
  // levels one by one would see).
  auto plan_level = [&](int i) -> int {
    const ChainSpec &sp = specs[i];
    Level &v = lv[i];
    int K = 1, max_out = 1;
    for (int d = 0; d < 3; d++) {
      D3D_REQUIRE(sp.filt[d] > 0 && sp.stride[d] > 0 && sp.out_size[d] > 0, "bad filter/stride/size");
      D3D_REQUIRE((sp.out_size[d] - 1) * sp.stride[d] + sp.filt[d] == sp.in_size[d],
                  "convolution sizes inconsistent: (out-1)*stride+filter != in (convolution.py:37-38)");
      v.geo.filt[d] = sp.filt[d];
      v.geo.stride[d] = sp.stride[d];
      v.geo.out_size[d] = sp.out_size[d];
      K *= sp.filt[d];
      max_out *= std::min((sp.filt[d] + sp.stride[d] - 1) / sp.stride[d], sp.out_size[d]);
    }
    v.geo.max_out = max_out;
    v.K = K;
    D3D_REQUIRE(K <= 32, "filter volume %d not supported (<= 32)", K);
    D3D_REQUIRE(max_out <= 8, "each input site may feed at most 8 outputs");
    const Size3 in_sz{sp.in_size[0], sp.in_size[1], sp.in_size[2]}, out_sz{sp.out_size[0], sp.out_size[1], sp.out_size[2]};
    D3D_REQUIRE_STATE(!find_grid(m, sp.out_size) && !made.count(out_sz), "grid chain: output grid [%d,%d,%d] already exists",
                      sp.out_size[0], sp.out_size[1], sp.out_size[2]);
    int ext_in[4];
    auto src = made.find(in_sz);
    if (src != made.end()) {
      const Level &u = lv[src->second];
      v.src = src->second;
      v.loc_in = u.go.loc;
      v.n_in_dev = u.n_out_dev;
      v.bound_in = u.bound_out;
      for (int d = 0; d < 4; d++) ext_in[d] = u.ext_out[d];
    } else {
      Grid *gi = find_grid(m, sp.in_size);
      D3D_REQUIRE_STATE(gi, "grid chain: no grid of spatial size [%d,%d,%d]", sp.in_size[0], sp.in_size[1], sp.in_size[2]);
      v.loc_in = gi->loc;
      v.n_in_host = gi->n;
      v.bound_in = gi->n;
      const bool known = gi->hext[0] > 0 && gi->hext[3] > 0;
      for (int d = 0; d < 3; d++) ext_in[d] = known ? gi->hext[d] : sp.in_size[d];
      ext_in[3] = known ? gi->hext[3] : 0;            // 0: number of examples unknown -> no cell bound
    }
    v.bound_entries = v.bound_in * max_out;
    long cells = ext_in[3] > 0 ? ext_in[3] : -1;
    for (int d = 0; d < 3; d++) {
      v.ext_out[d] = std::max(1, std::min(sp.out_size[d], (ext_in[d] - 1) / sp.stride[d] + 1));
      if (cells >= 0) cells = std::min<long>(cells * v.ext_out[d], (long)1 << 40);
    }
    v.ext_out[3] = ext_in[3];
    v.bound_out = cells >= 0 ? std::min(v.bound_entries, cells) : v.bound_entries;
    D3D_REQUIRE(v.bound_entries < (1L << 30), "grid chain: %ld candidate entries", v.bound_entries);
    v.small = v.bound_entries > 0 && v.bound_entries <= kSmallGrid;
    // persistent: table, coordinates, decoded rule table; temporaries (far end): entry slots, flags, raw forward table
    for (int d = 0; d < 3; d++) v.go.size[d] = sp.out_size[d];
    v.go.cap = next_pow2(2L * std::max<long>(v.bound_out, 1));
    D3D_ALLOC(tab, HashEntry, A, v.go.cap);
    D3D_ALLOC(loc_out, int32_t, A, (size_t)v.bound_out * 4 + 4);
    D3D_ALLOC(cnt, int32_t, A, 4);
    v.go.tab = tab;
    v.go.loc = loc_out;
    v.n_out_dev = cnt;
    add_fill(tab, sizeof(HashEntry) * (size_t)v.go.cap);       // (an empty level too: its grid still answers probes)
    if (sp.need_dec) {
      D3D_ALLOC(dec, int32_t, A, (size_t)v.bound_in * K + 4);
      v.nbr_dec = dec;
      add_fill(dec, sizeof(int32_t) * ((size_t)v.bound_in * K + 1));
    }
    if (v.bound_entries > 0) {
      const size_t fwd_bytes = sizeof(int32_t) * ((size_t)v.bound_out * K + 4);
      v.nbr_fwd = (int32_t *)top(fwd_bytes);
      if (!v.small) {
        const size_t tiles = ((size_t)v.bound_entries + kChainTile - 1) / kChainTile;
        v.eslot = (int32_t *)top(sizeof(int32_t) * (size_t)v.bound_entries);
        v.flagbits = (unsigned long long *)top(sizeof(unsigned long long) * tiles * 32);
        v.tile_cnt = (int32_t *)top(sizeof(int32_t) * tiles);
      }
      if (!v.nbr_fwd || (!v.small && (!v.eslot || !v.flagbits || !v.tile_cnt))) {
        set_error("metadata arena exhausted while building a grid chain");
        return D3D_ERR_NOMEM;
      }
      add_fill(v.nbr_fwd, fwd_bytes);
    }
    made[out_sz] = i;
    return D3D_OK;
  };
  int L_ok = L, fail_rc = D3D_OK;
  char fail_msg[512] = "";
  for (int i = 0; i < L; i++) {
    const size_t used0 = A.used, cap0 = A.cap;
    const int seg0 = n_seg;
    if (int rc = plan_level(i)) {
      A.used = used0;
      A.cap = cap0;
      n_seg = seg0;
      L_ok = i;
      fail_rc = rc;
      snprintf(fail_msg, sizeof(fail_msg), "%s", d3d_last_error());
      break;
    }
  }
  if (L_ok == 0) return fail_rc;          // (the error text is still the level's own message)
  // one fill for every table of every level, then the levels back to back
  if (n_seg > 0) {
    size_t most = 0;
    for (int j = 0; j < n_seg; j++) most = std::max<size_t>(most, fs.n16[j]);
    const unsigned bx = (unsigned)std::max<size_t>(1, std::min<size_t>((most + 1023) / 1024, 512));
    hipLaunchKernelGGL(k_fill_ones_multi, dim3(bx, n_seg), dim3(256), 0, s, fs);
  }
  CountPtrs cp = {};
  cp.n = L_ok;
  for (int i = 0; i < L_ok; i++) {
    Level &v = lv[i];
    cp.p[i] = v.n_out_dev;
    if (v.bound_entries == 0) {
      D3D_HIP_CHECK(hipMemsetAsync(v.n_out_dev, 0, sizeof(int32_t), s));
      continue;
    }
    if (v.small) {
      hipLaunchKernelGGL(k_conv_grid_small, dim3(1), dim3(kSmallGridThreads), 0, s, v.loc_in, (int)v.bound_entries, v.geo, v.K,
                         v.go.tab, v.go.cap, v.go.loc, v.nbr_fwd, v.nbr_dec, v.n_out_dev, v.n_in_dev);
      continue;
    }
    const long ne = v.bound_entries;
    const dim3 tiles((unsigned)((ne + kChainTile - 1) / kChainTile));
    hipLaunchKernelGGL(k_conv_insert, grid1d(ne), dim3(256), 0, s, v.loc_in, ne, v.geo, v.go.tab, v.go.cap, v.eslot, v.n_in_dev);
    hipLaunchKernelGGL(k_chain_flag, tiles, dim3(256), 0, s, v.eslot, v.go.tab, ne, v.geo.max_out, v.n_in_dev, v.flagbits,
                       v.tile_cnt);
    hipLaunchKernelGGL(k_chain_assign, tiles, dim3(256), 0, s, v.loc_in, ne, v.geo, v.n_in_dev, v.eslot, v.flagbits,
                       v.tile_cnt, v.go.tab, v.go.loc, v.n_out_dev);
    hipLaunchKernelGGL(k_conv_fill, grid1d(ne), dim3(256), 0, s, v.loc_in, ne, v.geo, v.K, v.eslot, v.go.tab, v.nbr_fwd,
                       v.nbr_dec, v.n_in_dev);
  }
  hipLaunchKernelGGL(k_store_counts, dim3(1), dim3(64), 0, s, cp, m->host_counts);
  D3D_LAUNCH_CHECK();
  if (!m->chain_ev) D3D_HIP_CHECK(hipEventCreateWithFlags(&m->chain_ev, hipEventDisableTiming));
  D3D_HIP_CHECK(hipEventRecord(m->chain_ev, s));
  D3D_HIP_CHECK(hipEventSynchronize(m->chain_ev));          // the one read-back of the chain
  for (int i = 0; i < L_ok; i++) {
    n_out[i] = ((volatile int32_t *)m->host_counts)[i];
    D3D_REQUIRE(n_out[i] >= 0 && n_out[i] <= lv[i].bound_out, "grid chain: level %d has %d sites, bound %ld", i, n_out[i],
                lv[i].bound_out);
  }
  // the grids exist: publish them all, then the rulebooks (exact sizes) in order
  for (int i = 0; i < L_ok; i++) {
    lv[i].go.n = n_out[i];
    for (int d = 0; d < 4; d++) lv[i].go.hext[d] = lv[i].ext_out[d];
    {
      D3D_LOCK(m);
      m->grids[Size3{specs[i].out_size[0], specs[i].out_size[1], specs[i].out_size[2]}] = lv[i].go;
    }
    if (on_grid) on_grid(hook_arg, i, n_out[i], s);
  }
  for (int i = 0; i < L_ok; i++) {
    Level &v = lv[i];
    const ChainSpec &sp = specs[i];
    const int n_in = v.src >= 0 ? n_out[v.src] : v.n_in_host;
    Plan p;
    t_plan_ctx[1] = v.bound_entries == 0 ? 3 : v.small ? 1 : 2;
    int rc = finalize_plan(m, v.nbr_fwd, n_out[i], v.K, p, s, nullptr);
    if (rc) return rc;
    {
      D3D_LOCK(m);
      const PlanKey key = make_key(1, sp.in_size, sp.filt, sp.stride);
      if (v.nbr_dec) {
        StridedRaw raw;
        raw.nbr_dec = v.nbr_dec;
        raw.n_in = n_in;
        raw.out_size = Size3{sp.out_size[0], sp.out_size[1], sp.out_size[2]};
        m->strided_raw[key] = raw;
      }
      p.n_in = n_in;
      m->plans.emplace(key, p);
    }
    if (on_done) on_done(hook_arg, i, n_out[i], s);
  }
  if (fail_rc != D3D_OK) {
    set_error("%s", fail_msg);
    return fail_rc;
  }
  return D3D_OK;
}

}  // namespace d3d

using namespace d3d;

extern "C" {

int d3d_conv_prepare(d3d_meta *m, const int *in_size, const int *out_size, const int *filt,
                     const int *stride, void *stream, int *n_out_host, long *n_rules_host) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && in_size && out_size && filt && stride, "null argument");
  Plan *p = const_cast<Plan *>(find_plan(m, 1, in_size, filt, stride));
  if (!p) {                                  // a chain of one level, decoded table kept
    ChainSpec sp;
    for (int d = 0; d < 3; d++) {
      sp.in_size[d] = in_size[d];
      sp.out_size[d] = out_size[d];
      sp.filt[d] = filt[d];
      sp.stride[d] = stride[d];
    }
    sp.need_dec = 1;
    std::vector<int> n_out;
    if (int rc = run_grid_chain(m, {sp}, s, n_out, nullptr, nullptr, nullptr)) return rc;
    p = const_cast<Plan *>(find_plan(m, 1, in_size, filt, stride));
  }
  if (n_out_host) *n_out_host = p->n_rows;
  if (n_rules_host) return plan_rules(m, *p, s, n_rules_host);
  return D3D_OK;
}

}  // extern "C"
