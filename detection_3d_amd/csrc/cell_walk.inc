// The walk over the cell list of normals.hip with the query left open, and the lock-free union-find over the sorted
// positions with its labelling tail (consumers: clean.hip, planes.hip).  Included inside namespace d3d's anonymous
// namespace, after `using namespace celllist`: every translation unit gets its own instantiations.

constexpr int kThreads = 128;                     // 16 lane groups of 8, one query per group at a time
constexpr int kGroup = 8;
constexpr int kGroups = kThreads / kGroup;
constexpr int kSpan = 64;                         // sorted queries per workgroup
constexpr int kBudget = 1024;                     // staged candidates (16 KiB of LDS); beyond: read from global memory

struct Ranges {     // the 27 neighbour cells' candidates: positions in `pts` and, when staged, in the LDS copy
  int gb[27], ge[27], lb[27];
};

// f(C, pos) for the candidates of one query that lane gl of its group takes: l, l + 8, ... of every cell, cells in a
// fixed order; pos is the candidate's sorted position
template <bool STAGED, class F>
__device__ __forceinline__ void for_candidates(const float4 *__restrict__ pts, const float4 *cand, const Ranges &R, int gl,
                                               F f) {
#pragma unroll 1                      // unrolled 27-fold, the count query took 255 registers and one wave per SIMD
  for (int r = 0; r < 27; r++) {
    const int len = R.ge[r] - R.gb[r];
    for (int t = gl; t < len; t += kGroup) {
      const float4 C = STAGED ? cand[R.lb[r] + t] : pts[R.gb[r] + t];
      f(C, R.gb[r] + t);
    }
  }
}

__device__ __forceinline__ uint32_t dist2_bits(float4 C, float4 P) {
  const float dx = C.x - P.x, dy = C.y - P.y, dz = C.z - P.z;
  return __float_as_uint((dx * dx + dy * dy) + dz * dz);
}

// Lock-free union-find over the sorted positions.  par[x] <= x always and only ever decreases, every value it takes is a
// member of x's component, and every access inside the linking kernel is a device-scope atomic, so that no CU works on
// a cached copy.  Nothing here waits for another thread's store: a failed compare-and-swap returns the value that beat
// it, and the loop goes on from that value, strictly downwards.
__device__ __forceinline__ int uf_load(int32_t *par, int x) {
  return __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int uf_find(int32_t *par, int x) {
  while (true) {                        // path halving; x strictly decreases
    const int p = uf_load(par, x);
    if (p == x) return x;
    const int g = uf_load(par, p);
    if (g == p) return p;
    atomicMin(par + x, g);
    x = g;
  }
}
__device__ __forceinline__ void uf_unite(int32_t *par, int a, int b) {
  while (true) {                        // a + b strictly decreases
    a = uf_find(par, a);
    b = uf_find(par, b);
    if (a == b) return;
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicCAS(par + hi, hi, lo);      // hook a root under the lower id
    if (old == hi) return;
    a = old;                            // hi had been hooked meanwhile: go on from its parent
    b = lo;
  }
}

// k_nrm_search's walk with the query left open.  One workgroup per kSpan sorted queries.  The span is walked cell by
// cell: the 27 neighbour cells' ranges come from the table, their points are staged into LDS once (when they fit) and
// every query of the cell in the span reuses them.
template <class Q>
__global__ __launch_bounds__(kThreads) void k_cln_walk(const float4 *__restrict__ pts, const uint64_t *__restrict__ key,
                                                       int n, const HashEntry *__restrict__ tab, int cap, Q query) {
  __shared__ float4 cand[kBudget];
  __shared__ Ranges R;
  __shared__ int s_next, s_total;
  const int tid = threadIdx.x, grp = tid / kGroup, gl = tid % kGroup;
  int k = blockIdx.x * kSpan;
  const int kend = min(n, k + kSpan);
  while (k < kend) {                  // uniform over the workgroup
    const uint64_t ck = key[k];
    if (tid == 0) s_next = kend;
    __syncthreads();
    for (int t = k + 1 + tid; t < kend; t += kThreads)
      if (key[t] != ck) {
        atomicMin(&s_next, t);
        break;
      }
    if (tid < 27) {
      const int cx = (int)(ck >> (2 * kCellBits)) + tid / 9 - 1;
      const int cy = (int)((ck >> kCellBits) & kCellMax) + (tid / 3) % 3 - 1;
      const int cz = (int)(ck & kCellMax) + tid % 3 - 1;
      int2 g = make_int2(0, 0);
      if (cx >= 0 && cx <= kCellMax && cy >= 0 && cy <= kCellMax && cz >= 0 && cz <= kCellMax)
        g = cell_range(tab, cap, cell_key((uint32_t)cx, (uint32_t)cy, (uint32_t)cz));
      g.x = max(0, min(g.x, n));      // whatever the table holds, no range leaves the sorted points
      g.y = max(g.x, min(g.y, n));
      R.gb[tid] = g.x;
      R.ge[tid] = g.y;
    }
    __syncthreads();
    if (tid == 0) {
      int tot = 0;
      for (int r = 0; r < 27; r++) {
        R.lb[r] = tot;
        tot += R.ge[r] - R.gb[r];
      }
      s_total = tot;
    }
    __syncthreads();
    const int e = s_next;
    const bool staged = s_total <= kBudget;
    if (staged) {
      for (int r = grp; r < 27; r += kGroups) {
        const int len = R.ge[r] - R.gb[r];
        for (int t = gl; t < len; t += kGroup) cand[R.lb[r] + t] = pts[R.gb[r] + t];
      }
    }
    __syncthreads();
    for (int q = k + grp; q < e; q += kGroups) {
      if (staged) query.template run<true>(pts, cand, R, q, pts[q], gl);
      else query.template run<false>(pts, cand, R, q, pts[q], gl);
    }
    __syncthreads();
    k = e;
  }
}

// ---- connected components: after the linking ----
__global__ void k_cln_iota(int32_t *par, int n) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) par[k] = k;
}

// root of every sorted position (par is only read here), and per root the smallest original index and the point count:
// integer min and add, which commute.  A wave first gathers the lanes that share a root, so that a component of a
// whole building does not send one atomic per point to one address.
__global__ __launch_bounds__(256) void k_cln_roots(const int32_t *__restrict__ par, const float4 *__restrict__ pts, int n,
                                                   int32_t *root, int32_t *min_index, int32_t *size) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool active = k < n;
  int r = -1, idx = 0x7fffffff;
  if (active) {
    r = k;
    while (true) {
      const int p = par[r];
      if (p == r) break;
      r = p;
    }
    root[k] = r;
    idx = __float_as_int(pts[k].w);
  }
  unsigned long long todo = __ballot(active);
  while (todo) {                      // uniform over the wave; every round retires at least its leader
    const int leader = __ffsll((long long)todo) - 1;
    const int lr = __shfl(r, leader, 64);
    const bool same = active && r == lr;
    const unsigned long long m = __ballot(same);
    int v = same ? idx : 0x7fffffff;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = min(v, __shfl_xor(v, s, 64));
    if (lane == leader) {
      atomicAdd(size + lr, __popcll(m));
      atomicMin(min_index + lr, v);
    }
    todo &= ~m;
    active = active && !same;
  }
}

__global__ void k_cln_labels(const int32_t *__restrict__ root, const float4 *__restrict__ pts, int n,
                             const int32_t *__restrict__ min_index, const int32_t *__restrict__ csize, int32_t *label,
                             int32_t *size) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int i = __float_as_int(pts[k].w), r = root[k];
  label[i] = min_index[r];
  size[i] = csize[r];
}

// ---- host side ----
constexpr int kPhases = 5;            // cells, sort, table, search, tail

struct Timer {                        // events around the phases when the caller asked for their times
  hipEvent_t ev[kPhases + 1] = {};
  bool on = false;
  int start(bool want) {
    on = want;
    if (on)
      for (int k = 0; k <= kPhases; k++) D3D_HIP_CHECK(hipEventCreate(&ev[k]));
    return D3D_OK;
  }
  int mark(int k, hipStream_t s) {
    if (on) D3D_HIP_CHECK(hipEventRecord(ev[k], s));
    return D3D_OK;
  }
  int finish(float *ms) {
    if (!on) return D3D_OK;
    D3D_HIP_CHECK(hipEventSynchronize(ev[kPhases]));
    for (int k = 0; k < kPhases; k++) D3D_HIP_CHECK(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
    for (int k = 0; k <= kPhases; k++) (void)hipEventDestroy(ev[k]);
    return D3D_OK;
  }
};

bool args_ok(int n, int stride, float radius) {
  return n >= 0 && n <= kMaxPoints && stride >= 3 && radius > 0.f && radius < INFINITY;
}

// the bits of the fp32 product r r: the kernels compare distances as integers
uint32_t r2_bits(float radius) { return __builtin_bit_cast(uint32_t, radius * radius); }

void zero_phases(float *ms) {
  if (ms)
    for (int k = 0; k < kPhases; k++) ms[k] = 0.f;
}

template <class Q>
int launch_walk(const CellList &L, int n, Q q, hipStream_t s) {
  hipLaunchKernelGGL(k_cln_walk<Q>, dim3((unsigned)((n + kSpan - 1) / kSpan)), dim3(kThreads), 0, s, L.pts, L.key, n, L.tab,
                     L.cap, q);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

#define CLN_TRY(expr)        \
  do {                       \
    const int rc_ = (expr);  \
    if (rc_) return rc_;     \
  } while (0)
