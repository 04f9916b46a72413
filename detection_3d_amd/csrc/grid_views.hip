// Views of a finished grid: occupied extent and dense index, site coordinates, anchors, sparse <-> dense.
#include "grid_internal.h"

namespace d3d {

// occupied extent of a grid (1 + max coordinate per axis), what sparse_3d_to_dense_2d crops the dense map to; and, when
// the grid's bounding box is small (host-side bounds `hext` from the input layer / the grid chain), a DENSE INDEX of that
// box: dense[((b * e0 + x) * e1 + y) * e2 + z] = 1 + site id, 0 = empty.  The rotated RoIAlign samples through it with
// one load per trilinear corner instead of a probe sequence through the hash table (a pyramid level the pooler reads is
// ~40 k cells: the index stays in L2 / L1).
static constexpr long kDenseMaxCells = 8L << 20;
__global__ void k_grid_extent(const int32_t *__restrict__ loc, int n, int32_t *__restrict__ extent,
                              int32_t *__restrict__ dense, int e0, int e1, int e2) {
  D3D_SIDE_PRIO();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  int v[3] = {0, 0, 0};
  if (i < n) {
    const int x = loc[(size_t)i * 4], y = loc[(size_t)i * 4 + 1], z = loc[(size_t)i * 4 + 2], b = loc[(size_t)i * 4 + 3];
    v[0] = x + 1;
    v[1] = y + 1;
    v[2] = z + 1;
    if (dense) dense[(((size_t)b * e0 + x) * e1 + y) * e2 + z] = i + 1;
  }
#pragma unroll
  for (int d = 0; d < 3; d++) {
    int m = v[d];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(&extent[d], m);
  }
}
int grid_extent(d3d_meta *m, Grid &g, hipStream_t s) {
  if (g.extent) return D3D_OK;
  Arena &A = lane_arena(m, s);
  long cells = 0;
  if (g.hext[0] > 0 && g.hext[3] > 0) {
    cells = (long)g.hext[3] * g.hext[0] * g.hext[1] * g.hext[2];
    if (cells > kDenseMaxCells) cells = 0;
  }
  D3D_ALLOC(e, int32_t, A, 64 + (size_t)cells);      // [0..3] extent, [64..] dense index: one zero fill for both
  D3D_HIP_CHECK(hipMemsetAsync(e, 0, (64 + (size_t)cells) * sizeof(int32_t), s));
  int32_t *dense = cells ? e + 64 : nullptr;
  if (g.n > 0)
    hipLaunchKernelGGL(k_grid_extent, grid1d(g.n), dim3(256), 0, s, g.loc, g.n, e, dense, g.hext[0], g.hext[1], g.hext[2]);
  D3D_LAUNCH_CHECK();
  g.extent = e;
  g.dense = dense;
  return D3D_OK;
}

__global__ void k_locations(const int32_t *__restrict__ loc, int n, int64_t *__restrict__ out) {
  D3D_SIDE_PRIO();
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n * 4) out[t] = loc[t];
}
// AnchorGenerator for one map: site i, cell anchor a -> (loc_i / voxel_scale * stride + base_a.xyz, base_a.size, yaw)
struct AnchorBase {
  float v[16 * 7];
};
__global__ void k_anchors(const int32_t *__restrict__ loc, int n, int A, AnchorBase base, float vs, float s0, float s1,
                          float s2, float *__restrict__ out) {
  D3D_SIDE_PRIO();
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * A) return;
  const int i = t / A, a = t - i * A;
  const int32_t *p = loc + (size_t)i * 4;
  const float *b = base.v + a * 7;
  float *o = out + (size_t)t * 7;
  // true division first, then the stride (anchor_generator_sparse3d.py:99), then + base (x + 0 keeps x)
  o[0] = (float)p[0] / vs * s0 + b[0];
  o[1] = (float)p[1] / vs * s1 + b[1];
  o[2] = (float)p[2] / vs * s2 + b[2];
  o[3] = 0.f + b[3];
  o[4] = 0.f + b[4];
  o[5] = 0.f + b[5];
  o[6] = 0.f + b[6];
}
// ... for up to kAnchorMaps maps in one launch: map m's sites are rows start[m] .. start[m+1]-1 of the row space
static constexpr int kAnchorMaps = 6, kAnchorA = 4;
struct AnchorMaps {
  const int32_t *loc[kAnchorMaps];
  int start[kAnchorMaps + 1];
  float stride[kAnchorMaps][3];
  float base[kAnchorMaps][kAnchorA * 7];
  int n_maps;
};
__global__ void k_anchors_maps(AnchorMaps am, int A, float vs, float *__restrict__ out) {
  D3D_SIDE_PRIO();
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= am.start[am.n_maps] * A) return;
  const int row = t / A, a = t - row * A;
  int m = 0;
  while (m + 1 < am.n_maps && row >= am.start[m + 1]) m++;
  const int32_t *p = am.loc[m] + (size_t)(row - am.start[m]) * 4;
  const float *b = am.base[m] + a * 7;
  float *o = out + (size_t)t * 7;
  // the same operations, in the same order, as k_anchors
  o[0] = (float)p[0] / vs * am.stride[m][0] + b[0];
  o[1] = (float)p[1] / vs * am.stride[m][1] + b[1];
  o[2] = (float)p[2] / vs * am.stride[m][2] + b[2];
  o[3] = 0.f + b[3];
  o[4] = 0.f + b[4];
  o[5] = 0.f + b[5];
  o[6] = 0.f + b[6];
}
__global__ void k_sparse_to_dense(const float *__restrict__ in, int planes,
                                  const int32_t *__restrict__ loc, int n, int sx, int sy, int sz,
                                  float *__restrict__ out) {
  D3D_SIDE_PRIO();
  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)n * planes) return;
  // consecutive threads -> consecutive sites (coalesced-ish writes along z), plane-major loop
  int i = (int)(t % n), c = (int)(t / n);
  const int32_t *p = loc + (size_t)i * 4;
  size_t vol = (size_t)sx * sy * sz;
  size_t off = ((size_t)p[0] * sy + p[1]) * sz + p[2];
  out[((size_t)p[3] * planes + c) * vol + off] = in[(size_t)i * planes + c];
}
// SparseToDense backward (CPU/SparseToDense.cpp:22-33): d_in[i][c] = d_out[dense cell of site i][c]
__global__ void k_sparse_to_dense_bwd(const float *__restrict__ d_out, int planes, const int32_t *__restrict__ loc,
                                      int n, int sx, int sy, int sz, float *__restrict__ d_in) {
  D3D_SIDE_PRIO();
  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)n * planes) return;
  int i = (int)(t % n), c = (int)(t / n);
  const int32_t *p = loc + (size_t)i * 4;
  size_t vol = (size_t)sx * sy * sz;
  size_t off = ((size_t)p[0] * sy + p[1]) * sz + p[2];
  d_in[(size_t)i * planes + c] = d_out[((size_t)p[3] * planes + c) * vol + off];
}

}  // namespace d3d

using namespace d3d;

extern "C" {

int d3d_get_n_active(d3d_meta *m, const int *size, int *n_host) {
  D3D_REQUIRE(m && size && n_host, "null argument");
  Grid *g = find_grid(m, size);
  D3D_REQUIRE_STATE(g, "no grid of spatial size [%d,%d,%d]", size[0], size[1], size[2]);
  *n_host = g->n;
  return D3D_OK;
}

int d3d_get_spatial_locations(d3d_meta *m, const int *size, int64_t *out, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && size, "null argument");
  Grid *g = find_grid(m, size);
  D3D_REQUIRE_STATE(g, "no grid of spatial size [%d,%d,%d]", size[0], size[1], size[2]);
  if (g->n == 0) return D3D_OK;
  D3D_REQUIRE(out, "null output");
  hipLaunchKernelGGL(k_locations, grid1d((long)g->n * 4), dim3(256), 0, s, g->loc, g->n, out);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

int d3d_anchors(d3d_meta *m, const int *size, const float *base_host, int A, const float *stride_host,
                float voxel_scale, float *out, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && size && base_host && stride_host && A >= 1 && A <= 16 && voxel_scale > 0, "anchors: bad arguments");
  Grid *g = find_grid(m, size);
  D3D_REQUIRE_STATE(g, "anchors: no grid of spatial size [%d,%d,%d]", size[0], size[1], size[2]);
  if (g->n == 0) return D3D_OK;
  D3D_REQUIRE(out, "null output");
  AnchorBase base;
  for (int i = 0; i < A * 7; i++) base.v[i] = base_host[i];
  hipLaunchKernelGGL(k_anchors, grid1d((long)g->n * A), dim3(256), 0, s, g->loc, g->n, A, base, voxel_scale,
                     stride_host[0], stride_host[1], stride_host[2], out);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

int d3d_anchors_maps(d3d_meta *m, int n_maps, const int *sizes_host, const float *bases_host, int A,
                     const float *strides_host, float voxel_scale, float *out, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && sizes_host && bases_host && strides_host && n_maps >= 1 && n_maps <= kAnchorMaps && A >= 1 &&
                  A <= kAnchorA && voxel_scale > 0,
              "anchors_maps: 1..%d maps, 1..%d anchors per site", kAnchorMaps, kAnchorA);
  AnchorMaps am = {};
  long n = 0;
  for (int i = 0; i < n_maps; i++) {
    Grid *g = find_grid(m, sizes_host + 3 * i);
    D3D_REQUIRE_STATE(g, "anchors: no grid of spatial size [%d,%d,%d]",
                      sizes_host[3 * i], sizes_host[3 * i + 1], sizes_host[3 * i + 2]);
    am.loc[i] = g->loc;
    am.start[i] = (int)n;
    n += g->n;
    for (int d = 0; d < 3; d++) am.stride[i][d] = strides_host[3 * i + d];
    for (int j = 0; j < A * 7; j++) am.base[i][j] = bases_host[(size_t)i * A * 7 + j];
  }
  D3D_REQUIRE(n * A * 7 < (1L << 31), "anchors_maps: %ld sites", n);
  for (int i = n_maps; i <= kAnchorMaps; i++) am.start[i] = (int)n;
  am.n_maps = n_maps;
  if (n == 0) return D3D_OK;
  D3D_REQUIRE(out, "null output");
  hipLaunchKernelGGL(k_anchors_maps, grid1d(n * A), dim3(256), 0, s, am, A, voxel_scale, out);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

int d3d_sparse_to_dense_forward(d3d_meta *m, const int *size, const float *in, int planes, int batch,
                                float *out, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && size && out && planes > 0 && batch > 0, "bad arguments");
  Grid *g = find_grid(m, size);
  D3D_REQUIRE_STATE(g, "sparse_to_dense: no grid of spatial size [%d,%d,%d]", size[0], size[1], size[2]);
  // k_sparse_to_dense indexes the volume by every site's example index: the batch must cover them (hext[3] = 1 + the
  // largest, 0 where it is not known; the coordinates themselves were checked against `size` when the grid was built)
  D3D_REQUIRE(g->hext[3] <= batch, "sparse_to_dense: batch %d, but the grid holds examples up to index %d", batch,
              g->hext[3] - 1);
  size_t vol = (size_t)size[0] * size[1] * size[2];
  D3D_HIP_CHECK(hipMemsetAsync(out, 0, sizeof(float) * vol * planes * batch, s));
  if (g->n == 0) return D3D_OK;
  D3D_REQUIRE(in, "null input");
  hipLaunchKernelGGL(k_sparse_to_dense, grid1d((long)g->n * planes), dim3(256), 0, s, in, planes, g->loc, g->n, size[0], size[1], size[2], out);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

int d3d_sparse_to_dense_backward(d3d_meta *m, const int *size, const float *d_out, int planes, float *d_in,
                                 void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && size && planes > 0, "bad arguments");
  Grid *g = find_grid(m, size);
  D3D_REQUIRE_STATE(g, "sparse_to_dense backward: no grid of spatial size [%d,%d,%d]", size[0], size[1], size[2]);
  if (g->n == 0) return D3D_OK;
  D3D_REQUIRE(d_out && d_in, "null pointer");
  hipLaunchKernelGGL(k_sparse_to_dense_bwd, grid1d((long)g->n * planes), dim3(256), 0, s, d_out, planes, g->loc, g->n,
                     size[0], size[1], size[2], d_in);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

}  // extern "C"
