// Sparse-grid metadata on the device: the error text, the metadata handle and its arena lanes, and the input layer
// (voxel hash-scatter, per-site point lists).  Strided grids: grid_chain.hip; rulebooks ("plans"): plan.hip; locations,
// sparse->dense: grid_views.hip.  Replaces the single-threaded CPU rule builders of SCN/Metadata/* (see include/d3d_hip.h).
#include "grid_internal.h"

namespace d3d {

static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// While a geometry stream is set (d3d_meta_set_geometry_stream) the slab has two single-stream lanes: the geometry
// stream builds grids + strided rulebooks in `arena`, every other stream (the feature pass: submanifold / deconvolution
// rulebooks built by the first convolution that needs them, partial tiles, rule counts) works in `feat_arena`, so
// neither carves temporaries out of memory the other stream may still be using.
// A plan stream (d3d_meta_set_plan_stream) adds a third lane for the rulebooks that are views of an existing grid.
Arena &lane_arena(d3d_meta *m, hipStream_t s) {
  if (!m->geo_locked || s == m->geo_stream) return m->arena;
  return (m->plan_stream && s == m->plan_stream) ? m->plan_arena : m->feat_arena;
}

// New grids come from the geometry stream alone.
int check_build_stream(d3d_meta *m, hipStream_t s, const char *what) {
  D3D_REQUIRE_STATE(!m->geo_locked || s == m->geo_stream,
                    "%s requested on a stream other than the metadata's geometry stream (d3d_meta_set_geometry_stream): "
                    "prepare it there first", what);
  return D3D_OK;
}

Grid *find_grid(d3d_meta *m, const int *size) {
  D3D_LOCK(m);
  auto it = m->grids.find(Size3{size[0], size[1], size[2]});
  return it == m->grids.end() ? nullptr : &it->second;
}

// 0, 1, 2, ...: the values every plan sort permutes (d3d_meta::iota)
__global__ void k_iota(int32_t *p, int n) {
  D3D_SIDE_PRIO();
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = i;
}

// ------------------------------------------------------------------------------------------
// a2. Input layer: hash insert + first-occurrence numbering (IOLayersRules.h:72-95).
// ext (may be null): device int32[5], zero-initialised by the caller.  [0..3] = 1 + the largest x, y, z and example index
// over all points: one atomicMax per dimension and 256-thread block.  The host reads them back with the site count and
// bounds the site counts of the coarser grids with them (grid_chain.hip), so that no further count has to be read back.
// [4] = 1 + the index of a point that cannot be a site of this grid (0: none): a coordinate outside [0, size), or an
// example index outside [0, 32768).  Compared as int64, before pack_key keeps 16 bits of each.  The insertion itself
// needs no valid coordinate (it hashes the packed key); what indexes memory BY a coordinate (the dense views, the grid
// chain's cell bounds) runs only after the host has seen this word (d3d_input_layer_build_prefetch).
__global__ __launch_bounds__(256) void k_insert_points(const int64_t *__restrict__ coords, int n, int ncols,
                                                       HashEntry *tab, int cap, int32_t *pslot, int32_t *ext, int sx,
                                                       int sy, int sz) {
  D3D_SIDE_PRIO();
  __shared__ int red[4][5];
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int v[5] = {0, 0, 0, 0, 0};
  if (i < n) {
    const int64_t *c = coords + (size_t)i * ncols;
    const int64_t b64 = ncols == 4 ? c[3] : 0;
    int b = (int)b64;
    int slot = hash_insert(tab, cap, pack_key(b, (int)c[0], (int)c[1], (int)c[2]));
    atomicMin(&tab[slot].first, (uint32_t)i);
    pslot[i] = slot;
    if (c[0] < 0 || c[0] >= sx || c[1] < 0 || c[1] >= sy || c[2] < 0 || c[2] >= sz || b64 < 0 || b64 >= 32768) {
      v[4] = i + 1;
    } else {
      v[0] = (int)c[0] + 1;
      v[1] = (int)c[1] + 1;
      v[2] = (int)c[2] + 1;
      v[3] = b + 1;
    }
  }
  if (!ext) return;
#pragma unroll
  for (int d = 0; d < 5; d++) {
    int m = v[d];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][d] = m;
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    const int d = threadIdx.x;
    const int m = max(max(red[0][d], red[1][d]), max(red[2][d], red[3][d]));
    if (m > 0) atomicMax(&ext[d], m);
  }
}
__global__ void k_flag_first(const int32_t *__restrict__ pslot, const HashEntry *__restrict__ tab,
                             int n, int32_t *flag) {
  D3D_SIDE_PRIO();
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flag[i] = (pslot[i] >= 0 && tab[pslot[i]].first == (uint32_t)i) ? 1 : 0;
}
__global__ void k_assign_input_sites(const int64_t *__restrict__ coords, int n, int ncols,
                                     const int32_t *__restrict__ pslot,
                                     const int32_t *__restrict__ flag,
                                     const int32_t *__restrict__ rank, HashEntry *tab, int32_t *loc) {
  D3D_SIDE_PRIO();
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flag[i]) return;
  int id = rank[i];
  tab[pslot[i]].val = id;
  const int64_t *c = coords + (size_t)i * ncols;
  loc[id * 4 + 0] = (int)c[0];
  loc[id * 4 + 1] = (int)c[1];
  loc[id * 4 + 2] = (int)c[2];
  loc[id * 4 + 3] = ncols == 4 ? (int)c[3] : 0;
}
__global__ void k_point_site(const int32_t *__restrict__ pslot, const HashEntry *__restrict__ tab,
                             int n, uint32_t *psite, int32_t *cnt) {
  D3D_SIDE_PRIO();
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int s = tab[pslot[i]].val;
  psite[i] = (uint32_t)s;
  atomicAdd(&cnt[s], 1);
}
// a3. CPU/IOLayers.cpp:11-29: out[row] += mult * in[idx] in input order.
__global__ void k_input_forward(const float *__restrict__ in, int planes,
                                const int32_t *__restrict__ off, const int32_t *__restrict__ idx,
                                int n_active, int average, float *__restrict__ out) {
  D3D_SIDE_PRIO();
  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)n_active * planes) return;
  int row = (int)(t / planes), c = (int)(t % planes);
  int b = off[row], e = off[row + 1];
  int cnt = e - b;
  float mult = (average && cnt > 0) ? (float)1 / cnt : (float)1;
  float acc = 0.f;
  for (int j = b; j < e; j++) acc += mult * in[(size_t)idx[j] * planes + c];
  out[t] = acc;
}
// Input layer backward (CPU/IOLayers.cpp:30-47): every point receives multiplier * d_out[site].
__global__ void k_input_backward(const float *__restrict__ d_out, int planes, const int32_t *__restrict__ off,
                                 const int32_t *__restrict__ idx, int n_active, int average,
                                 float *__restrict__ d_in) {
  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)n_active * planes) return;
  const int row = (int)(t / planes), c = (int)(t % planes);
  const int b = off[row], e = off[row + 1];
  const float mult = (average && e > b) ? (float)1 / (e - b) : (float)1;
  const float g = mult * d_out[t];
  for (int j = b; j < e; j++) d_in[(size_t)idx[j] * planes + c] = g;
}
__global__ void k_export_input(const int32_t *a, int32_t *b, int n) {
  D3D_SIDE_PRIO();
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) b[i] = a[i];
}

static size_t point_list_scratch_bytes(int n) {   // what ensure_point_lists carves: site of every point, counts, scan sums, sort
  const size_t nn = (size_t)std::max(n, 1);
  return nn * 4 + 256 + (nn + 2) * 4 + 256 + ((nn + 1 + kScanTile - 1) / kScanTile) * 4 + 256 + sort_scratch_bytes(n, 32) + 4096;
}

// Per-site point lists in input order (stable sort of point ids by site id), built by the first consumer on ITS
// stream with temporaries from that stream's lane of the arena: the grid exists as soon as d3d_input_layer_build
// returns, so a caller may start the level-0 rulebook on another stream while the lists are sorted here.
// by_bound: nothing in the build depends on the site count (counters, scan and sort cover all n points' worth of
// sites: the sites past the true count hold zero points), so the lists can be enqueued before the count is read back.
static int build_point_lists(d3d_meta *m, hipStream_t s, bool by_bound) {
  const int n = m->in_n, n_sites = by_bound ? m->in_n : m->in_active;
  std::map<Size3, Grid>::iterator it;
  HashEntry *tab = nullptr;
  if (by_bound) {
    tab = (HashEntry *)m->pre_tab;
  } else {
    D3D_LOCK(m);
    it = m->grids.find(m->in_size);
    D3D_REQUIRE(it != m->grids.end(), "input layer: grid not found");
    tab = it->second.tab;
  }
  Arena own;                      // the region the build set aside: independent of the stream's lane
  own.base = m->pl_scratch;
  own.cap = m->pl_scratch_bytes;
  Arena &A = m->pl_scratch ? own : lane_arena(m, s);
  size_t mark = A.used;
  D3D_ALLOC(psite, uint32_t, A, n);
  D3D_ALLOC(cnt, int32_t, A, (size_t)n + 1);
  D3D_REQUIRE(m->iota && n <= m->iota_n, "input layer: point index table missing");
  D3D_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(int32_t) * ((size_t)n_sites + 1), s));
  hipLaunchKernelGGL(k_point_site, grid1d(n), dim3(256), 0, s, m->in_pslot, tab, n, psite, cnt);
  int rc = scan_exclusive_i32(cnt, m->in_off, n_sites + 1, nullptr, A, s);
  if (rc) return rc;
  int bits = 1;
  while ((1L << bits) < n_sites) bits++;
  rc = sort_pairs_u32(psite, nullptr, m->iota, m->in_idx, n, bits, A, s, false);
  if (rc) return rc;
  D3D_LAUNCH_CHECK();
  A.used = mark;
  return D3D_OK;
}
int ensure_point_lists(d3d_meta *m, hipStream_t s) {
  if (m->in_n == 0) return D3D_OK;
  if (m->in_lists) {
    // built on the library's own stream by the input-layer build: this stream waits for them
    if (m->lists_on_aux) D3D_HIP_CHECK(hipStreamWaitEvent(s, m->lists_ev, 0));
    return D3D_OK;
  }
  int rc = build_point_lists(m, s, false);
  if (rc) return rc;
  m->in_lists = true;
  return D3D_OK;
}

}  // namespace d3d

using namespace d3d;

extern "C" {

const char *d3d_last_error(void) { return d3d::g_err; }
int d3d_abi_version(void) { return 3; }

int d3d_meta_create(d3d_meta **out, size_t arena_bytes) {
  D3D_REQUIRE(out && arena_bytes >= (1u << 20), "d3d_meta_create: bad arguments");
  d3d_meta *m = new d3d_meta();
  hipError_t e = hipMalloc((void **)&m->arena.base, arena_bytes);
  if (e != hipSuccess) {
    set_error("hipMalloc(%zu) failed: %s", arena_bytes, hipGetErrorString(e));
    delete m;
    return D3D_ERR_HIP;
  }
  const size_t feat_bytes = (arena_bytes / 3) & ~size_t(255);   // second lane (see lane_arena)
  m->arena.cap = m->arena_cap_full = arena_bytes - feat_bytes;
  m->feat_arena.base = m->arena.base + m->arena.cap;
  m->feat_arena.cap = m->feat_cap_full = feat_bytes;
  e = hipHostMalloc((void **)&m->host_words, 16 * sizeof(long), hipHostMallocDefault);
  if (e == hipSuccess) e = hipHostMalloc((void **)&m->host_counts, 32 * sizeof(int32_t), hipHostMallocDefault);
  if (e != hipSuccess) {
    set_error("hipHostMalloc failed: %s", hipGetErrorString(e));
    (void)hipFree(m->arena.base);
    delete m;
    return D3D_ERR_HIP;
  }
  *out = m;
  return D3D_OK;
}
int d3d_meta_destroy(d3d_meta *m) {
  if (!m) return D3D_OK;
  geo_async_free(m);
  (void)hipFree(m->arena.base);
  (void)hipHostFree(m->host_words);
  if (m->host_counts) (void)hipHostFree(m->host_counts);
  if (m->count_ev) (void)hipEventDestroy(m->count_ev);
  if (m->chain_ev) (void)hipEventDestroy(m->chain_ev);
  if (m->grid_ev) (void)hipEventDestroy(m->grid_ev);
  if (m->lists_ev) (void)hipEventDestroy(m->lists_ev);
  if (m->fill_ev) (void)hipEventDestroy(m->fill_ev);
  if (m->aux_stream) (void)hipStreamDestroy(m->aux_stream);
  delete m;
  return D3D_OK;
}
int d3d_meta_clear(d3d_meta *m) {
  D3D_REQUIRE(m, "null metadata");
  geo_async_join(m);
  D3D_LOCK(m);
  m->arena.used = 0;
  m->arena.cap = m->arena_cap_full;
  m->pre_nbr = nullptr;
  m->pre_mask = nullptr;
  m->pre_plan_built = false;
  m->pre_sym = false;
  m->pre_tab = nullptr;
  m->lists_on_aux = false;
  m->feat_arena.used = 0;
  m->feat_arena.cap = m->feat_cap_full;
  m->plan_arena = Arena();
  m->plan_stream = nullptr;
  m->geo_locked = false;
  m->geo_stream = nullptr;
  m->grids.clear();
  m->plans.clear();
  m->strided_raw.clear();
  m->in_n = m->in_mode = m->in_active = 0;
  for (int d = 0; d < 4; d++) m->in_ext[d] = 0;
  m->in_off = m->in_idx = m->in_pslot = nullptr;
  m->pl_scratch = nullptr;
  m->pl_scratch_bytes = 0;
  m->iota = nullptr;
  m->iota_n = 0;
  m->in_lists = false;
  return D3D_OK;
}
int d3d_meta_set_geometry_stream(d3d_meta *m, void *stream, int enable) {
  D3D_REQUIRE(m, "null metadata");
  m->geo_locked = enable != 0;
  m->geo_stream = enable ? (hipStream_t)stream : nullptr;
  return D3D_OK;
}
int d3d_meta_set_plan_stream(d3d_meta *m, void *stream, int enable) {
  D3D_REQUIRE(m, "null metadata");
  if (!enable) {
    m->plan_stream = nullptr;   // the lane's rulebooks stay where they are until d3d_meta_clear
    return D3D_OK;
  }
  D3D_REQUIRE(m->geo_locked && stream && (hipStream_t)stream != m->geo_stream,
              "d3d_meta_set_plan_stream: set a geometry stream first, and a different one");
  if (!m->plan_arena.base) {    // first use for this scene: the upper 3/4 of the feature lane become the plan lane
    const size_t keep = (m->feat_arena.cap / 4) & ~size_t(255);
    D3D_REQUIRE(m->feat_arena.used <= keep, "d3d_meta_set_plan_stream: the feature lane is already %zu bytes deep",
                m->feat_arena.used);
    m->plan_arena.base = m->feat_arena.base + keep;
    m->plan_arena.cap = m->feat_arena.cap - keep;
    m->plan_arena.used = 0;
    m->feat_arena.cap = keep;
  }
  m->plan_stream = (hipStream_t)stream;
  return D3D_OK;
}
int d3d_meta_arena_used(d3d_meta *m, size_t *bytes_host) {
  D3D_REQUIRE(m && bytes_host, "null argument");
  *bytes_host = m->arena.used;
  return D3D_OK;
}

int d3d_input_layer_build(d3d_meta *m, const int64_t *coords, int n, int ncols, const int *size,
                          int batch_size, int mode, void *stream, int *n_active_host) {
  return d3d_input_layer_build_prefetch(m, coords, n, ncols, size, batch_size, mode, nullptr, stream, n_active_host);
}

int d3d_input_layer_build_prefetch(d3d_meta *m, const int64_t *coords, int n, int ncols, const int *size,
                                   int batch_size, int mode, const int *prefetch_filter, void *stream,
                                   int *n_active_host) {
  hipStream_t s = (hipStream_t)stream;
  (void)batch_size;
  D3D_REQUIRE(m && size && n_active_host, "null argument");
  D3D_REQUIRE(ncols == 3 || ncols == 4, "coords must be [n,3] or [n,4], got %d columns", ncols);
  D3D_REQUIRE(mode == 3 || mode == 4, "input layer mode %d not supported (3=sum, 4=mean)", mode);
  D3D_REQUIRE(n >= 0 && (n == 0 || coords), "bad coords");
  {
    D3D_LOCK(m);
    D3D_REQUIRE_STATE(m->grids.empty(), "input layer: metadata already holds grids; call d3d_meta_clear first");
  }
  for (int d = 0; d < 3; d++) D3D_REQUIRE(size[d] > 0 && size[d] <= 32768, "spatial size out of range");
  Arena &A = m->arena;
  Grid g;
  for (int d = 0; d < 3; d++) g.size[d] = size[d];
  g.cap = next_pow2(2L * n);
  D3D_ALLOC(tab, HashEntry, A, g.cap);
  D3D_ALLOC(loc, int32_t, A, (size_t)n * 4 + 4);
  D3D_ALLOC(in_off, int32_t, A, (size_t)n + 2);
  D3D_ALLOC(in_idx, int32_t, A, (size_t)n + 1);
  D3D_ALLOC(pslot, int32_t, A, (size_t)n + 1);
  D3D_ALLOC(iota, int32_t, A, (size_t)n + 1);   // 0, 1, 2, ...: the values every plan sort permutes (no grid has more rows)
  {
    const size_t pl = point_list_scratch_bytes(n);
    D3D_ALLOC(pls, char, A, pl);
    m->pl_scratch = pls;
    m->pl_scratch_bytes = pl;
  }
  m->iota = iota;
  m->iota_n = n;
  if (n > 0) hipLaunchKernelGGL(k_iota, grid1d(n), dim3(256), 0, s, iota, n);
  m->in_pslot = pslot;
  m->in_lists = false;
  m->in_size = Size3{size[0], size[1], size[2]};
  g.tab = tab;
  g.loc = loc;
  m->in_n = n;
  m->in_mode = mode;
  m->in_off = in_off;
  m->in_idx = in_idx;
  int n_active = 0;
  if (n > 0) {
    // [0] site count, [1..4] extents of the points, [5] 1 + a point outside the grid (k_insert_points).  NOT part of the
    // scratch released below: the prefetched neighbour probes read the count from it while other streams may already be
    // allocating from this lane.
    D3D_ALLOC(total, int32_t, A, 8);
    // (the arrays of the rulebook that is enqueued below before the count is back: sized by the point count)
    const int pre_K = prefetch_filter ? prefetch_filter[0] * prefetch_filter[1] * prefetch_filter[2] : 0;
    const int nblk_b = (n + 31) / 32, npos_b = nblk_b * 32;
    int32_t *prows = nullptr, *pnbrT = nullptr;
    uint32_t *pblk = nullptr;
    if (pre_K > 1 && pre_K <= 32) {
      prows = A.get<int32_t>((size_t)npos_b + 1);
      pnbrT = A.get<int32_t>((size_t)npos_b * pre_K + 1);
      pblk = A.get<uint32_t>((size_t)nblk_b + 1);
    }
    size_t mark = A.used;
    D3D_ALLOC(flag, int32_t, A, n);
    D3D_ALLOC(rank, int32_t, A, n);
    // Everything of the pass's start that does not need the site count ON THE HOST is enqueued before the count is read
    // back, sized by the point count and reading the site count on the device, so that the GPU keeps working while the
    // count travels: on this stream the submanifold rulebook the caller will ask for first -- hash probes of every site,
    // the sort of the rows by offset mask, the transposed table (raw table, masks and sort scratch live at the top of
    // the geometry lane, which stays that much shorter for the scene) -- and, on a stream of the library's own, the
    // fills of that table (beside the point insertion) and the input layer's point lists (beside the probes; counters,
    // scan and sort cover n sites' worth of entries, sites past the true count hold no points).  Launch ORDER follows
    // the critical path: the host needs ~4 us per launch, and the probes must not queue behind the lists' 12 launches.
    bool pre = false, sym = false;
    size_t raw = 0, msk = 0, srt = 0;
    if (prefetch_filter && m->pl_scratch) {
      raw = (((size_t)n * pre_K + 1) * sizeof(int32_t) + 255) & ~size_t(255);
      msk = ((size_t)n * sizeof(uint32_t) + 511) & ~size_t(255);
      srt = (sort_scratch_bytes(n, std::min(pre_K, 32)) + 255) & ~size_t(255);
      pre = pre_K > 1 && pre_K <= 32 && prows && pnbrT && pblk && A.used + raw + msk + srt + (64u << 20) < A.cap;
    }
    Arena sc;
    if (pre) {
      if (!m->aux_stream) {
        D3D_HIP_CHECK(hipStreamCreateWithFlags(&m->aux_stream, hipStreamNonBlocking));
        D3D_HIP_CHECK(hipEventCreateWithFlags(&m->grid_ev, hipEventDisableTiming));
        D3D_HIP_CHECK(hipEventCreateWithFlags(&m->lists_ev, hipEventDisableTiming));
        D3D_HIP_CHECK(hipEventCreateWithFlags(&m->fill_ev, hipEventDisableTiming));
      }
      A.cap = (A.cap - raw - msk - srt) & ~size_t(255);
      sc.base = A.base + A.cap;
      sc.cap = srt;
      m->pre_mask = (uint32_t *)(A.base + A.cap + srt);
      m->pre_nbr = (int32_t *)(A.base + A.cap + srt + msk);
      for (int d = 0; d < 3; d++) m->pre_filt[d] = prefetch_filter[d];
      m->pre_stream = s;
      sym = subm_nbr_is_sym(n, prefetch_filter);
      // the library's stream joins the caller's here (arena reuse from scene to scene is ordered by the caller's stream)
      D3D_HIP_CHECK(hipEventRecord(m->grid_ev, s));
      D3D_HIP_CHECK(hipStreamWaitEvent(m->aux_stream, m->grid_ev, 0));
      if (sym) {
        if (int rc2 = subm_nbr_prefill(n, prefetch_filter, m->pre_nbr, m->pre_mask, m->aux_stream)) return rc2;
        D3D_HIP_CHECK(hipEventRecord(m->fill_ev, m->aux_stream));
      }
    }
    D3D_HIP_CHECK(fill_ones(tab, sizeof(HashEntry) * g.cap, s));
    D3D_HIP_CHECK(hipMemsetAsync(total, 0, 8 * sizeof(int32_t), s));
    hipLaunchKernelGGL(k_insert_points, grid1d(n), dim3(256), 0, s, coords, n, ncols, tab, g.cap, pslot, total + 1,
                       size[0], size[1], size[2]);
    hipLaunchKernelGGL(k_flag_first, grid1d(n), dim3(256), 0, s, pslot, tab, n, flag);
    int rc = scan_exclusive_i32(flag, rank, n, total, A, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_assign_input_sites, grid1d(n), dim3(256), 0, s, coords, n, ncols, pslot, flag, rank, tab, loc);
    D3D_LAUNCH_CHECK();
    D3D_HIP_CHECK(hipMemcpyAsync(&m->host_words[0], total, 6 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    bool prefetched = false;
    if (pre) {
      if (!m->count_ev) D3D_HIP_CHECK(hipEventCreateWithFlags(&m->count_ev, hipEventDisableTiming));
      D3D_HIP_CHECK(hipEventRecord(m->count_ev, s));          // the host waits for the count, not for what follows
      // 1. the probes (the longest kernel of the start) ...
      if (sym) D3D_HIP_CHECK(hipStreamWaitEvent(s, m->fill_ev, 0));
      if (int rc2 = launch_subm_nbr(loc, n, prefetch_filter, tab, g.cap, m->pre_nbr, m->pre_mask, total, s, sym, sym)) return rc2;
      prefetched = true;
      // 2. ... beside them the point lists, behind the grid (count_ev marks it) ...
      D3D_HIP_CHECK(hipStreamWaitEvent(m->aux_stream, m->count_ev, 0));
      m->pre_tab = tab;
      if (int rc2 = build_point_lists(m, m->aux_stream, true)) return rc2;
      D3D_HIP_CHECK(hipEventRecord(m->lists_ev, m->aux_stream));
      m->in_lists = true;
      m->lists_on_aux = true;
      // 3. ... then the rows sorted by offset mask (low K bits of the keys the probes left) and the transposed table
      Plan &p = m->pre_plan;
      p = Plan();
      p.K = pre_K;
      p.rows = prows;
      p.nbrT = pnbrT;
      p.blkmask = pblk;
      if (int rc2 = sort_pairs_u32(m->pre_mask, nullptr, m->iota, p.rows, n, std::min(pre_K, 32), sc, s, true, total)) return rc2;
      launch_plan_finish(m->pre_nbr, p.rows, n, npos_b, pre_K, p.nbrT, p.blkmask, total, s);
      D3D_LAUNCH_CHECK();
      m->pre_plan_built = true;
      m->pre_sym = sym;
    }
    if (prefetched) D3D_HIP_CHECK(hipEventSynchronize(m->count_ev));
    else D3D_HIP_CHECK(hipStreamSynchronize(s));
    n_active = (int)*(int32_t *)&m->host_words[0];
    if (const int bad = ((const int32_t *)&m->host_words[0])[5]) {
      // A point that is no cell of this grid.  Nothing enqueued above indexes memory by a coordinate: insert, flag, scan,
      // assign, the probes, the point lists and the sorts go by hashes, ranks, site ids and point indices (all < n), so
      // the work in flight is harmless.  The caller's stream is put behind the library's stream, the handle goes back to
      // what d3d_meta_clear leaves (full arena, no prefetched plan, no input layer), and no grid is entered.
      if (m->lists_on_aux) D3D_HIP_CHECK(hipStreamWaitEvent(s, m->lists_ev, 0));
      d3d_meta_clear(m);
      *n_active_host = 0;
      set_error("input layer: point %d has a coordinate outside the spatial size [%d,%d,%d] or an example index outside "
                "[0, 32768)", bad - 1, size[0], size[1], size[2]);
      return D3D_ERR_ARG;
    }
    for (int d = 0; d < 4; d++) m->in_ext[d] = ((const int32_t *)&m->host_words[0])[1 + d];
    A.used = mark;
  } else {
    D3D_HIP_CHECK(fill_ones(tab, sizeof(HashEntry) * g.cap, s));   // an empty grid still answers probes
  }
  g.n = n_active;
  for (int d = 0; d < 4; d++) g.hext[d] = m->in_ext[d];
  m->in_active = n_active;
  {
    D3D_LOCK(m);
    m->grids[Size3{size[0], size[1], size[2]}] = g;
    if (m->pre_plan_built) {        // the rulebook enqueued above, now that its row count is known on the host
      Plan &p = m->pre_plan;
      p.n_rows = p.n_in = n_active;
      p.n_blk = (n_active + 31) / 32;
      p.n_rules = n_active == 0 ? 0 : -1;
      m->plans.emplace(make_key(0, size, m->pre_filt, nullptr), p);
      int passes, db;
      rs_layout(std::min(p.K, 32), passes, db);
      plan_record(4, 1, m->pre_sym ? 2 : 1, p.K, n_active, n, p.n_blk, passes, db, 0);
    }
  }
  *n_active_host = n_active;
  return D3D_OK;
}

int d3d_input_layer_prepare(d3d_meta *m, void *stream) {
  D3D_REQUIRE(m, "null metadata");
  D3D_REQUIRE_STATE(m->in_off, "input layer prepare before build");
  return ensure_point_lists(m, (hipStream_t)stream);
}

int d3d_input_layer_forward(d3d_meta *m, const float *feats, int planes, float *out, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && planes > 0, "bad arguments");
  D3D_REQUIRE_STATE(m->in_off, "input layer forward before build");
  if (m->in_active == 0) return D3D_OK;
  D3D_REQUIRE(feats && out, "null feature pointer");
  if (int rc = ensure_point_lists(m, s)) return rc;
  hipLaunchKernelGGL(k_input_forward, grid1d((long)m->in_active * planes), dim3(256), 0, s, feats,
                     planes, m->in_off, m->in_idx, m->in_active, m->in_mode == 4 ? 1 : 0, out);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

int d3d_input_layer_backward(d3d_meta *m, const float *d_out, int planes, float *d_in, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && planes > 0, "bad arguments");
  if (!m->in_off) {
    set_error("input layer backward before build");
    return D3D_ERR_STATE;
  }
  if (m->in_active == 0) return D3D_OK;
  D3D_REQUIRE(d_out && d_in, "null gradient pointer");
  if (int rc = ensure_point_lists(m, s)) return rc;
  long total = (long)m->in_active * planes;
  hipLaunchKernelGGL(k_input_backward, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_out, planes,
                     m->in_off, m->in_idx, m->in_active, m->in_mode == 4 ? 1 : 0, d_in);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

int d3d_input_layer_export(d3d_meta *m, int32_t *offsets, int32_t *idx, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && offsets && idx, "null argument");
  D3D_REQUIRE_STATE(m->in_off, "input layer export before build");
  if (m->in_n == 0) {             // no points: no list was built, the one offset is 0
    D3D_HIP_CHECK(hipMemsetAsync(offsets, 0, sizeof(int32_t), s));
    return D3D_OK;
  }
  if (int rc = ensure_point_lists(m, s)) return rc;
  hipLaunchKernelGGL(k_export_input, grid1d(m->in_active + 1), dim3(256), 0, s, m->in_off, offsets, m->in_active + 1);
  if (m->in_n) hipLaunchKernelGGL(k_export_input, grid1d(m->in_n), dim3(256), 0, s, m->in_idx, idx, m->in_n);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

}  // extern "C"
