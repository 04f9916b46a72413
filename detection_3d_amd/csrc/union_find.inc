// The lock-free union-find over the sorted positions of a cell list and its labelling tail (consumers: clean.hip,
// planes.hip).  Included inside namespace d3d's anonymous namespace: every translation unit gets its own instantiations.

// par[x] <= x always and only ever decreases, every value it takes is a member of x's component, and every access
// inside the linking kernel is a device-scope atomic, so that no CU works on a cached copy.  Nothing here waits for
// another thread's store: a failed compare-and-swap returns the value that beat it, and the loop goes on from that
// value, strictly downwards.
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
