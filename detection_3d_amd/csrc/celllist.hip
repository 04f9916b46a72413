// The cell list of a raw cloud (d3d_internal.h, namespace celllist; consumers: normals.hip, clean.hip, planes.hip,
// register.hip) and the (z, y, x)-digit sort chain that it shares with downsample.hip.
//
// Passes: per-axis min -> cell coordinates (cells of edge 1.0001 r, so that a neighbour is never two cells away) ->
// three stable radix sorts (z, y, x: z is the fastest digit of the order) -> sorted points and their 60-bit cell keys
// -> open-addressing table cell -> [first, last).
#include "d3d_internal.h"

#include <algorithm>

namespace d3d {

namespace {

using namespace celllist;                         // kCellBits, kCellMax, cell_key, cell_insert (d3d_internal.h)

// per-axis min: grid-stride, wave shuffle, LDS, one integer atomic per block and axis -- order-independent
__global__ __launch_bounds__(256) void k_cell_min(const float *__restrict__ xyz, int n, int stride, uint32_t *red) {
  __shared__ float lds[4][3];
  float v[3] = {INFINITY, INFINITY, INFINITY};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    for (int d = 0; d < 3; d++) v[d] = fminf(v[d], xyz[(size_t)i * stride + d]);
  for (int d = 0; d < 3; d++) {
    float x = v[d];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x = fminf(x, __shfl_xor(x, s, 64));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6][d] = x;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int d = threadIdx.x;
    const float x = fminf(fminf(lds[0][d], lds[1][d]), fminf(lds[2][d], lds[3][d]));
    atomicMin(&red[d], f32_ordered(x));
  }
}

// cell coordinate floor((p - min) / h) per axis in fp64 (p - min is exact there), clamped; anything unordered -> 0
__global__ void k_cell_coords(const float *__restrict__ xyz, int n, int stride, const uint32_t *__restrict__ red, double h,
                              uint32_t *cx, uint32_t *cy, uint32_t *cz, int32_t *iota) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t c[3];
  for (int d = 0; d < 3; d++) {
    const double q = floor(((double)xyz[(size_t)i * stride + d] - (double)ordered_to_f32(red[d])) / h);
    c[d] = q >= 0.0 ? (q < (double)kCellMax ? (uint32_t)q : (uint32_t)kCellMax) : 0u;
  }
  cx[i] = c[0];
  cy[i] = c[1];
  cz[i] = c[2];
  iota[i] = i;
}

__global__ void k_cell_gather(const uint32_t *__restrict__ src, const int32_t *__restrict__ perm, int n, uint32_t *dst) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) dst[k] = src[perm[k]];
}

// the points in cell order: (x, y, z, original index) and the cell key of every sorted position
__global__ void k_cell_sorted(const float *__restrict__ xyz, int n, int stride, const int32_t *__restrict__ perm,
                              const uint32_t *__restrict__ cx, const uint32_t *__restrict__ cy,
                              const uint32_t *__restrict__ cz, float4 *pts, uint64_t *key) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int i = perm[k];
  const float *p = xyz + (size_t)i * stride;
  pts[k] = make_float4(p[0], p[1], p[2], __int_as_float(i));
  key[k] = cell_key(cx[i], cy[i], cz[i]);
}

// cell -> [val, first) of the sorted positions: the first position of a cell stores val, the last one first; one
// thread each, so no two threads write the same word
__global__ void k_cell_table(const uint64_t *__restrict__ key, int n, HashEntry *tab, int cap) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint64_t c = key[k];
  const bool head = k == 0 || key[k - 1] != c, tail = k == n - 1 || key[k + 1] != c;
  if (!head && !tail) return;
  const int slot = cell_insert(tab, cap, c);
  if (head) tab[slot].val = k;
  if (tail) tab[slot].first = (uint32_t)(k + 1);
}

}  // namespace

int sort_cells_zyx(const uint32_t *cx, const uint32_t *cy, const uint32_t *cz, int32_t *perm_a, int32_t *perm_b,
                   uint32_t *ktmp, int n, int bits, int x_bits, Arena &A, hipStream_t s) {
  const size_t mark = A.used;
  // least significant digit first; every sort is stable and starts from 0, 1, 2, ...: the final order is (x, y, z, index)
  int rc = sort_pairs_u32(cz, nullptr, perm_a, perm_b, n, bits, A, s, false);
  if (rc) return rc;
  A.used = mark;
  hipLaunchKernelGGL(k_cell_gather, grid1d(n), dim3(256), 0, s, cy, (const int32_t *)perm_b, n, ktmp);
  rc = sort_pairs_u32(ktmp, nullptr, perm_b, perm_a, n, bits, A, s, false);
  if (rc) return rc;
  A.used = mark;
  hipLaunchKernelGGL(k_cell_gather, grid1d(n), dim3(256), 0, s, cx, (const int32_t *)perm_a, n, ktmp);
  rc = sort_pairs_u32(ktmp, nullptr, perm_a, perm_b, n, x_bits, A, s, false);
  if (rc) return rc;
  A.used = mark;
  return D3D_OK;                      // the order is in perm_b
}

namespace celllist {

int table_cap(int n) {
  long c = 1024;
  while (c < 2l * n) c <<= 1;
  return (int)c;
}

size_t scratch_bytes(int n) {
  const size_t N = (size_t)std::max(1, std::min(n, kMaxPoints));
  // the arrays of build() (256-byte aligned each), the table and one sort's temporaries
  return 6 * (N * 4 + 256) + (N * 16 + 256) + (N * 8 + 256) + ((size_t)table_cap((int)N) * sizeof(HashEntry) + 256) +
         sort_scratch_bytes((int)N, kCellBits) + 1024;
}

int build(const float *xyz, int n, int stride, float radius, Arena &A, hipStream_t s, CellList *out, hipEvent_t *ev) {
  D3D_REQUIRE(n >= 1 && n <= kMaxPoints && stride >= 3 && xyz && out, "cell list: bad point count, row stride or pointer");
#define CELL_MARK(k) \
  if (ev) D3D_HIP_CHECK(hipEventRecord(ev[k], s))
  const int cap = table_cap(n);
  D3D_ALLOC(red, uint32_t, A, 4);
  D3D_ALLOC(cx, uint32_t, A, n);
  D3D_ALLOC(cy, uint32_t, A, n);
  D3D_ALLOC(cz, uint32_t, A, n);
  D3D_ALLOC(perm_a, int32_t, A, n);
  D3D_ALLOC(perm_b, int32_t, A, n);
  D3D_ALLOC(ktmp, uint32_t, A, n);
  D3D_ALLOC(pts, float4, A, n);
  D3D_ALLOC(key, uint64_t, A, n);
  D3D_ALLOC(tab, HashEntry, A, cap);
  CELL_MARK(0);
  D3D_HIP_CHECK(hipMemsetAsync(red, 0xFF, 16, s));
  hipLaunchKernelGGL(k_cell_min, dim3(std::max(1u, std::min(1024u, grid1d(n).x))), dim3(256), 0, s, xyz, n, stride, red);
  hipLaunchKernelGGL(k_cell_coords, grid1d(n), dim3(256), 0, s, xyz, n, stride, (const uint32_t *)red,
                     (double)radius * 1.0001, cx, cy, cz, perm_a);
  D3D_LAUNCH_CHECK();
  CELL_MARK(1);
  const int rc = sort_cells_zyx(cx, cy, cz, perm_a, perm_b, ktmp, n, kCellBits, kCellBits, A, s);
  if (rc) return rc;
  hipLaunchKernelGGL(k_cell_sorted, grid1d(n), dim3(256), 0, s, xyz, n, stride, (const int32_t *)perm_b,
                     (const uint32_t *)cx, (const uint32_t *)cy, (const uint32_t *)cz, pts, key);
  D3D_LAUNCH_CHECK();
  CELL_MARK(2);
  D3D_HIP_CHECK(hipMemsetAsync(tab, 0xFF, (size_t)cap * sizeof(HashEntry), s));
  hipLaunchKernelGGL(k_cell_table, grid1d(n), dim3(256), 0, s, (const uint64_t *)key, n, tab, cap);
  D3D_LAUNCH_CHECK();
  CELL_MARK(3);
#undef CELL_MARK
  out->pts = pts;
  out->key = key;
  out->tab = tab;
  out->cap = cap;
  out->red = red;
  out->h = (double)radius * 1.0001;
  return D3D_OK;
}

}  // namespace celllist
}  // namespace d3d
