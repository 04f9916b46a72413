// The one walk over a cloud's cell list (celllist.hip) with the query left open, the nearest-k cut that the queries
// share and the host-side helpers (consumers: normals.hip, clean.hip, planes.hip; register.hip takes the constants
// and helpers for a walk of its own).  Included inside namespace d3d's anonymous namespace, after
// `using namespace celllist`: every translation unit gets its own instantiations.

constexpr int kThreads = 128;                     // 16 lane groups of 8, one query per group at a time
constexpr int kGroup = 8;
constexpr int kGroups = kThreads / kGroup;
constexpr int kSpan = 64;                         // sorted queries per workgroup
constexpr int kBudget = 1024;                     // staged candidates (16 KiB of LDS); beyond: read from global memory

struct Ranges {     // the 27 neighbour cells' candidates: positions in `pts` and, when staged, in the LDS copy
  int gb[27], ge[27], lb[27];
};

// f(C, pos) for the candidates of one query that lane gl of its group takes: l, l + 8, ... of every cell, cells in a
// fixed order; pos is the candidate's sorted position.  The inner loop runs over the index that it loads from (the LDS
// copy's or the sorted points'), with pos as an offset from it: counted from 0 with two bases added, the compiler puts a
// longer dispatch between the unrolled loop and its remainder in front of every cell, and the normals at 1 M points
// took 3 % longer (DESIGN 6d)
template <bool STAGED, class F>
__device__ __forceinline__ void for_candidates(const float4 *__restrict__ pts, const float4 *cand, const Ranges &R, int gl,
                                               F f) {
#pragma unroll 1                      // unrolled 27-fold, the count query took 255 registers and one wave per SIMD
  for (int r = 0; r < 27; r++) {
    const int b = STAGED ? R.lb[r] : R.gb[r], e = b + (R.ge[r] - R.gb[r]), shift = R.gb[r] - b;
    for (int t = b + gl; t < e; t += kGroup) {
      const float4 C = STAGED ? cand[t] : pts[t];
      f(C, t + shift);
    }
  }
}

__device__ __forceinline__ uint32_t dist2_bits(float4 C, float4 P) {
  const float dx = C.x - P.x, dy = C.y - P.y, dz = C.z - P.z;
  return __float_as_uint((dx * dx + dy * dy) + dz * dz);
}

__device__ __forceinline__ int group_sum(int c) {
#pragma unroll
  for (int o = kGroup / 2; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
  return c;
}

// The nearest-`want` cut of one query's candidates by (d2, j), j the original index, for its whole lane group:
//   keep(d2, j) = d2 < T or (d2 == T and j <= J): T the want-th smallest d2 (bits of a non-negative float order like
//   the float), J the cut among the candidates tied at T.
// T enters as the bits of r2 and J leaves as 0x7fffffff unless ties had to be cut; returns the number kept,
// min(candidates within r, want).  d2 <= r2 <=> bits(d2) <= bits(r2); a NaN distance has larger bits than any finite r2
// and is never kept.  The counts do not depend on scheduling, so every lane of the group takes the same path.
template <bool STAGED>
__device__ __forceinline__ int nearest_cut(const float4 *__restrict__ pts, const float4 *cand, const Ranges &R, float4 P,
                                           int gl, int want, int n, uint32_t &T, int &J) {
  auto count_kept = [&](uint32_t t, int j) {
    int c = 0;
    for_candidates<STAGED>(pts, cand, R, gl, [&](float4 C, int) {
      const uint32_t u = dist2_bits(C, P);
      c += (u < t || (u == t && __float_as_int(C.w) <= j)) ? 1 : 0;
    });
    return group_sum(c);
  };
  J = 0x7fffffff;
  int m = count_kept(T, J);
  if (m > want) {
    uint32_t lo = 0, hi = T;          // invariant: count(d2 <= hi) = m_hi >= want
    int m_hi = m;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      const int c = count_kept(mid, J);
      if (c >= want) {
        hi = mid;
        m_hi = c;
      } else {
        lo = mid + 1;
      }
    }
    T = hi;
    if (m_hi > want) {                // ties at T: the smallest J with count(.., J) >= want, then exactly `want`
      int jl = 0, jh = n - 1;
      while (jl < jh) {
        const int mid = jl + (jh - jl) / 2;
        if (count_kept(T, mid) >= want) jh = mid;
        else jl = mid + 1;
      }
      J = jh;
    }
    m = want;
  }
  return m;
}

// The walk, with the query left open: Q::run<STAGED>(pts, cand, R, q, P, gl) is one query (sorted position q, point P)
// by lane gl of one lane group.  One workgroup per kSpan sorted queries.  The span is walked cell by cell: the 27
// neighbour cells' ranges come from the table, their points are staged into LDS once (when they fit) and every query of
// the cell in the span reuses them.
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

// ---- host side ----
constexpr int kPhases = 5;            // cells, sort, table, search, tail: kPhases + 1 events of a Timer (d3d_internal.h)

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
