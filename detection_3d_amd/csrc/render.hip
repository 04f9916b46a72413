// Posed depth frames from a triangle mesh: the step the reference leaves to an external OpenGL tool (scn2img, between
// gen_house_obj and gen_pcl of data3d/suncg_utils/suncg_preprocess.py).  The arithmetic contract is written out in
// include/d3d_hip.h: a pixel-triangle test in homogeneous form, fp64 in a fixed order, the smallest depth
// and then the lowest triangle index wins.  Brute force over pixels x triangles is the semantics; this file bins.
//
// Tiles of 16 x 16 pixels.  k_rd_bin<false> gives every (frame, triangle) a conservative rectangle of tiles and counts it
// into every tile of the rectangle; scan_exclusive_i32 turns the counts into list offsets; k_rd_bin<true> finds the same
// rectangles again and writes the triangle index into a slot of every tile's list (the slot comes from an atomic, so the
// order inside a list is arbitrary, which the (z, index) minimum does not see).  No per-(frame, triangle) array exists:
// the rectangle costs ~50 flops and is computed twice.  k_rd_tiles is one workgroup per (frame, tile): it stages up to
// 256 triangles of its list in LDS, ten doubles each (the three edge normals and D, from the fp32 vertices and the fp64
// camera), then every lane tests its pixel against the staged triangles, which it reads as LDS broadcasts, and keeps
// (z, index, e0, e1, e2) of the best hit in registers.  Depth, index and colour are written once; no atomic touches an image.
//
// The rectangle: a triangle with a vertex index outside [0, V) or a non-finite vertex is in no list.  One whose three
// camera-space z are <= 0 is in none either: a hit's depth is a convex combination of them.  One with all z > 0 and
// projections below 1e9 px in magnitude takes the bounding box of its projected vertices, grown by a pixel (the rounding
// of the fp64 projection is below 1e-6 px there); anything else (crossing the camera plane, a camera row that is
// not finite) takes the whole frame.
#include "d3d_internal.h"

#include <algorithm>
#include <cmath>

namespace d3d {

namespace {

#include "depth_frames.inc"   // Camera, load_camera; DepthView and frames_shape, frames_view for the frames a call fills

constexpr int kTile = 16;
constexpr int kThreads = kTile * kTile;
constexpr int kBatch = 256;                  // triangles staged at a time: 10 doubles + an index each, 21 KiB of LDS
constexpr double kMaxPx = 1e9;

struct Mesh {
  const float *vertices;
  const int32_t *triangles;
  int V, T;
};

struct Views {
  const double *intr, *extr;                 // [F, 4], [F, 3, 4]
  int F, H, W, tx, ty;                       // tiles per row and per column of one frame
};

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < INFINITY; }      // false for NaN
__device__ __forceinline__ bool finite_d(double v) { return fabs(v) < (double)INFINITY; }

// camera-space vertices P[j] = R^T (x_j - t) of triangle `tri`; false: the triangle never hits (index outside [0, V) or a
// non-finite vertex), and nothing outside the arrays has been read.  idx: its three vertex indices.
__device__ __forceinline__ bool camera_vertices(const Mesh &M, const Camera &K, int tri, double (&P)[3][3], int (&idx)[3]) {
  if (tri < 0 || tri >= M.T) return false;
#pragma unroll
  for (int j = 0; j < 3; j++) idx[j] = M.triangles[3 * (long)tri + j];
#pragma unroll
  for (int j = 0; j < 3; j++)
    if (idx[j] < 0 || idx[j] >= M.V) return false;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const float *x = M.vertices + 3 * (long)idx[j];
    const float x0 = x[0], x1 = x[1], x2 = x[2];
    ok = ok && finite_f(x0) && finite_f(x1) && finite_f(x2);
    const double d0 = (double)x0 - K.t[0], d1 = (double)x1 - K.t[1], d2 = (double)x2 - K.t[2];
#pragma unroll
    for (int k = 0; k < 3; k++) P[j][k] = (K.R[0][k] * d0 + K.R[1][k] * d1) + K.R[2][k] * d2;
  }
  return ok;
}

__device__ __forceinline__ void cross(const double (&p)[3], const double (&q)[3], double (&n)[3]) {
  n[0] = p[1] * q[2] - p[2] * q[1];
  n[1] = p[2] * q[0] - p[0] * q[2];
  n[2] = p[0] * q[1] - p[1] * q[0];
}

// the rectangle of tiles [x0, x1] x [y0, y1] of one (frame, triangle); false: none
__device__ __forceinline__ bool tile_rect(const Mesh &M, const Views &C, const Camera &K, int tri, int &x0, int &x1, int &y0,
                                          int &y1) {
  double P[3][3];
  int idx[3];
  if (!camera_vertices(M, K, tri, P, idx)) return false;
  x0 = 0, y0 = 0, x1 = C.tx - 1, y1 = C.ty - 1;
  bool fin = finite_d(K.fx) && finite_d(K.fy) && finite_d(K.cx) && finite_d(K.cy) && K.fx != 0.0 && K.fy != 0.0;
#pragma unroll
  for (int j = 0; j < 3; j++) fin = fin && finite_d(P[j][0]) && finite_d(P[j][1]) && finite_d(P[j][2]);
  if (!fin) return true;
  const double zlo = fmin(fmin(P[0][2], P[1][2]), P[2][2]), zhi = fmax(fmax(P[0][2], P[1][2]), P[2][2]);
  if (zhi <= 0.0) return false;
  if (zlo <= 0.0) return true;
  double ulo = INFINITY, uhi = -INFINITY, vlo = INFINITY, vhi = -INFINITY;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const double u = P[j][0] / P[j][2] * K.fx + K.cx, v = P[j][1] / P[j][2] * K.fy + K.cy;
    if (!(fabs(u) < kMaxPx && fabs(v) < kMaxPx)) return true;
    ulo = fmin(ulo, u), uhi = fmax(uhi, u), vlo = fmin(vlo, v), vhi = fmax(vhi, v);
  }
  const double pu0 = fmax(ceil(ulo - 1.0), 0.0), pu1 = fmin(floor(uhi + 1.0), (double)(C.W - 1));
  const double pv0 = fmax(ceil(vlo - 1.0), 0.0), pv1 = fmin(floor(vhi + 1.0), (double)(C.H - 1));
  if (pu0 > pu1 || pv0 > pv1) return false;
  x0 = (int)pu0 / kTile, x1 = (int)pu1 / kTile, y0 = (int)pv0 / kTile, y1 = (int)pv1 / kTile;
  return true;
}

// FILL == false: counts[tile] += 1 for every tile of every rectangle, and total += the entries.  FILL == true: the
// triangle goes into a slot of every such tile's list; `cursor` holds the lists' begins and ends up with their ends.
template <bool FILL>
__global__ __launch_bounds__(kThreads) void k_rd_bin(Mesh M, Views C, int32_t *__restrict__ counts_or_cursor,
                                                     unsigned long long *__restrict__ total, int32_t *__restrict__ lists,
                                                     long n_entries) {
  __shared__ unsigned long long block_total;
  if (!FILL) {
    if (threadIdx.x == 0) block_total = 0ull;
    __syncthreads();
  }
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i < (long)C.F * M.T) {
    const int f = (int)(i / M.T), tri = (int)(i - (long)f * M.T);
    Camera K;
    load_camera(C.intr, C.extr, f, K);
    int x0, x1, y0, y1;
    if (tile_rect(M, C, K, tri, x0, x1, y0, y1)) {
      int32_t *tiles = counts_or_cursor + (long)f * C.tx * C.ty;
      for (int y = y0; y <= y1; y++)
        for (int x = x0; x <= x1; x++) {
          const int slot = atomicAdd(tiles + y * C.tx + x, 1);
          if (FILL && slot >= 0 && slot < n_entries) lists[slot] = tri;     // never past the caller's list
        }
      if (!FILL) atomicAdd(&block_total, (unsigned long long)((x1 - x0 + 1) * (y1 - y0 + 1)));
    }
  }
  if (!FILL) {
    __syncthreads();
    if (threadIdx.x == 0 && block_total) atomicAdd(total, block_total);
  }
}

struct Output {
  void *depth;                               // fp32 or uint16 [F, H, W]
  int32_t *tri;                              // [F, H, W] or null
  void *color;                               // fp32 or uint8 [F, H, W, 3] or null
  const void *vertex_color;                  // fp32 or uint8 [V, 3]
  int depth_u16, color_u8;
  double depth_scale, zmin, zmax;
};

__global__ __launch_bounds__(kThreads) void k_rd_tiles(Mesh M, Views C, const int32_t *__restrict__ counts,
                                                       const int32_t *__restrict__ ends,
                                                       const int32_t *__restrict__ lists, long n_entries, Output O) {
  __shared__ double sh[10][kBatch];
  __shared__ int32_t sh_id[kBatch];
  const int tid = threadIdx.x;
  const int per_frame = C.tx * C.ty;
  const int f = blockIdx.x / per_frame, t = blockIdx.x - f * per_frame;
  const int u = (t % C.tx) * kTile + (tid & (kTile - 1)), v = (t / C.tx) * kTile + tid / kTile;
  Camera K;
  load_camera(C.intr, C.extr, f, K);
  const double dx = ((double)u - K.cx) / K.fx, dy = ((double)v - K.cy) / K.fy;
  double bz = INFINITY, be0 = 0.0, be1 = 0.0, be2 = 0.0;
  int bid = -1;
  int n = counts[blockIdx.x];
  long begin = (long)ends[blockIdx.x] - n;
  if (n < 0 || begin < 0 || begin + n > n_entries) n = 0;      // lists that are not the ones k_rd_bin left: read nothing
  for (int base = 0; base < n; base += kBatch) {
    const int m = min(kBatch, n - base);
    __syncthreads();
    if (tid < m) {
      const int tri = lists[begin + base + tid];
      double P[3][3] = {}, nb[3][3];
      int idx[3];
      const bool ok = camera_vertices(M, K, tri, P, idx);
      cross(P[1], P[2], nb[0]);
      cross(P[2], P[0], nb[1]);
      cross(P[0], P[1], nb[2]);
      const double D = (P[0][0] * nb[0][0] + P[0][1] * nb[0][1]) + P[0][2] * nb[0][2];
#pragma unroll
      for (int k = 0; k < 9; k++) sh[k][tid] = ok ? nb[k / 3][k % 3] : (double)NAN;     // NaN: no comparison holds
      sh[9][tid] = ok ? D : (double)NAN;
      sh_id[tid] = tri;
    }
    __syncthreads();
    for (int j = 0; j < m; j++) {
      const double e0 = (dx * sh[0][j] + dy * sh[1][j]) + sh[2][j];
      const double e1 = (dx * sh[3][j] + dy * sh[4][j]) + sh[5][j];
      const double e2 = (dx * sh[6][j] + dy * sh[7][j]) + sh[8][j];
      const bool in = (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
      if (!in) continue;
      const double S = (e0 + e1) + e2;
      if (!(S != 0.0)) continue;
      const double z = sh[9][j] / S;
      if (!(z > 0.0 && z < (double)INFINITY && z >= O.zmin && z <= O.zmax)) continue;
      const int id = sh_id[j];
      if (z < bz || (z == bz && id < bid)) bz = z, bid = id, be0 = e0, be1 = e1, be2 = e2;
    }
  }
  if (u >= C.W || v >= C.H) return;
  const long p = ((long)f * C.H + v) * C.W + u;
  const bool hit = bid >= 0;
  if (O.depth_u16) {
    const double q = hit ? rint(bz / O.depth_scale) : 0.0;
    ((uint16_t *)O.depth)[p] = (q >= 1.0 && q <= 65535.0) ? (uint16_t)q : (uint16_t)0;
  } else {
    ((float *)O.depth)[p] = hit ? (float)bz : 0.f;
  }
  if (O.tri) O.tri[p] = bid;
  if (!O.color) return;
  double c[3] = {0.0, 0.0, 0.0};
  if (hit) {
    const double S = (be0 + be1) + be2;
    const double w0 = be0 / S, w1 = be1 / S, w2 = be2 / S;
    int idx[3];
#pragma unroll
    for (int j = 0; j < 3; j++) idx[j] = M.triangles[3 * (long)bid + j];      // a listed triangle: indices in range
#pragma unroll
    for (int k = 0; k < 3; k++) {
      double ca, cb, cc;
      if (O.color_u8) {
        const uint8_t *vc = (const uint8_t *)O.vertex_color;
        ca = (double)vc[3 * (long)idx[0] + k], cb = (double)vc[3 * (long)idx[1] + k], cc = (double)vc[3 * (long)idx[2] + k];
      } else {
        const float *vc = (const float *)O.vertex_color;
        ca = (double)vc[3 * (long)idx[0] + k], cb = (double)vc[3 * (long)idx[1] + k], cc = (double)vc[3 * (long)idx[2] + k];
      }
      c[k] = (w0 * ca + w1 * cb) + w2 * cc;
    }
  }
  if (O.color_u8) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double r = rint(c[k]);
      ((uint8_t *)O.color)[3 * p + k] = (uint8_t)(r >= 255.0 ? 255.0 : (r >= 0.0 ? r : 0.0));     // NaN -> 0
    }
  } else {
#pragma unroll
    for (int k = 0; k < 3; k++) ((float *)O.color)[3 * p + k] = (float)c[k];
  }
}

struct Layout {
  unsigned long long *total;
  int32_t *counts, *offsets;                 // per (frame, tile); offsets become the lists' ends in d3d_render_fill
};

inline long tiles_of(int n) { return ((long)n + kTile - 1) / kTile; }

int carve(Arena &A, long n_tiles, Layout &L) {
  D3D_ALLOC(total, unsigned long long, A, 32);
  D3D_ALLOC(counts, int32_t, A, (size_t)n_tiles + 2);
  D3D_ALLOC(offsets, int32_t, A, (size_t)n_tiles + 2);
  L = Layout{total, counts, offsets};
  return D3D_OK;
}

// the checked descriptors -> mesh and views; n_tiles == 0 or T == 0 or V == 0: nothing to do, and no pointer is wanted
int make_views(const char *who, const d3d_triangle_mesh *mesh, const d3d_depth_frames *frames, Mesh &M, Views &C,
               long &n_tiles) {
  D3D_REQUIRE(mesh, "%s: null pointer", who);
  D3D_REQUIRE(mesh->n_vertices >= 0 && mesh->n_triangles >= 0, "%s: %d vertices, %d triangles", who, mesh->n_vertices,
              mesh->n_triangles);
  long P = 0;
  const int rc = frames_shape(who, frames, P);
  if (rc) return rc;
  D3D_REQUIRE((double)frames->frames * (double)mesh->n_triangles < 2147483648.0 * (double)kThreads,
              "%s: %d frames x %d triangles are too many for one call (use fewer frames per call)", who, frames->frames,
              mesh->n_triangles);
  M = Mesh{mesh->vertices, mesh->triangles, mesh->n_vertices, mesh->n_triangles};
  C = Views{frames->intrinsics, frames->extrinsics, frames->frames, frames->height, frames->width,
            (int)tiles_of(frames->width), (int)tiles_of(frames->height)};
  n_tiles = (long)C.F * C.tx * C.ty;
  return D3D_OK;
}

int open_scratch(const char *who, void *scratch, size_t scratch_bytes, const Views &C, long n_tiles, Arena &A, Layout &L) {
  D3D_REQUIRE(scratch, "%s: null pointer", who);
  D3D_REQUIRE(scratch_bytes >= d3d_render_scratch_bytes(C.F, C.H, C.W), "%s: scratch too small", who);
  A = scratch_arena(scratch, scratch_bytes);
  return carve(A, n_tiles, L);
}

}  // namespace
}  // namespace d3d

using namespace d3d;

size_t d3d_render_scratch_bytes(int frames, int height, int width) {
  const size_t n = (size_t)std::max(frames, 0) * (size_t)tiles_of(std::max(width, 0)) * (size_t)tiles_of(std::max(height, 0));
  return 512 + 2 * ((n + 2) * 4 + 256) + (n / 2048 + 1) * 4 + 4096;
}

int d3d_render_bin(const d3d_triangle_mesh *mesh, const d3d_depth_frames *frames, void *scratch, size_t scratch_bytes,
                   int64_t *info_host, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(info_host, "d3d_render_bin: null pointer");
  info_host[0] = 0;
  Mesh M;
  Views C;
  long n_tiles;
  int rc = make_views("d3d_render_bin", mesh, frames, M, C, n_tiles);
  if (rc) return rc;
  if (n_tiles == 0 || M.T == 0 || M.V == 0) return D3D_OK;
  D3D_REQUIRE(M.vertices && M.triangles && C.intr && C.extr, "d3d_render_bin: null pointer");
  Arena A;
  Layout L;
  rc = open_scratch("d3d_render_bin", scratch, scratch_bytes, C, n_tiles, A, L);
  if (rc) return rc;
  D3D_HIP_CHECK(hipMemsetAsync(L.total, 0, 32 * sizeof(unsigned long long), s));
  D3D_HIP_CHECK(hipMemsetAsync(L.counts, 0, ((size_t)n_tiles + 2) * sizeof(int32_t), s));
  const long work = (long)C.F * M.T;
  hipLaunchKernelGGL(k_rd_bin<false>, dim3((unsigned)((work + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, M, C,
                     L.counts, L.total, (int32_t *)nullptr, 0L);
  D3D_LAUNCH_CHECK();
  rc = scan_exclusive_i32(L.counts, L.offsets, (int)n_tiles, nullptr, A, s);
  if (rc) return rc;
  rc = readback_publish(L.total, 2, s);
  if (rc) return rc;
  return readback_wait(info_host, 2);
}

int d3d_render_fill(const d3d_triangle_mesh *mesh, const d3d_depth_frames *frames, const int64_t *info_host,
                    void *scratch, size_t scratch_bytes, int32_t *lists, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(info_host, "d3d_render_fill: null pointer");
  Mesh M;
  Views C;
  long n_tiles;
  int rc = make_views("d3d_render_fill", mesh, frames, M, C, n_tiles);
  if (rc) return rc;
  const int64_t E = info_host[0];
  D3D_REQUIRE(E >= 0 && E < 2147483648LL, "d3d_render_fill: %lld list entries do not fit 31 bits (use fewer frames per call)",
              (long long)E);
  if (n_tiles == 0 || M.T == 0 || M.V == 0 || E == 0) return D3D_OK;
  D3D_REQUIRE(M.vertices && M.triangles && C.intr && C.extr && lists, "d3d_render_fill: null pointer");
  Arena A;
  Layout L;
  rc = open_scratch("d3d_render_fill", scratch, scratch_bytes, C, n_tiles, A, L);
  if (rc) return rc;
  const long work = (long)C.F * M.T;
  hipLaunchKernelGGL(k_rd_bin<true>, dim3((unsigned)((work + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, M, C,
                     L.offsets, (unsigned long long *)nullptr, lists, (long)E);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

int d3d_render_tiles(const d3d_triangle_mesh *mesh, const d3d_depth_frames *frames, double min_depth, double max_depth,
                     const int64_t *info_host, const void *scratch, size_t scratch_bytes, const int32_t *lists,
                     int32_t *tri, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(info_host, "d3d_render_tiles: null pointer");
  Mesh M;
  Views C;
  long n_tiles;
  int rc = make_views("d3d_render_tiles", mesh, frames, M, C, n_tiles);
  if (rc) return rc;
  DepthView V;                               // the images to fill: the depth format, and the pointers wanted when P > 0
  rc = frames_view("d3d_render_tiles", frames, 1, min_depth, max_depth, kFramesDepth | kFramesCameras, V);
  if (rc) return rc;
  D3D_REQUIRE(!frames->color == !mesh->vertex_color, "d3d_render_tiles: a colour image needs vertex colours and the reverse");
  const int64_t E = info_host[0];
  D3D_REQUIRE(E >= 0 && E < 2147483648LL, "d3d_render_tiles: %lld list entries do not fit 31 bits", (long long)E);
  if (n_tiles == 0) return D3D_OK;
  D3D_REQUIRE(M.T > 0 && M.V > 0, "d3d_render_tiles: an empty mesh has no lists (the images are zeros)");
  D3D_REQUIRE(M.vertices && M.triangles && (lists || E == 0), "d3d_render_tiles: null pointer");
  Arena A;
  Layout L;
  rc = open_scratch("d3d_render_tiles", const_cast<void *>(scratch), scratch_bytes, C, n_tiles, A, L);
  if (rc) return rc;
  const Output O{frames->depth, tri, frames->color, mesh->vertex_color, V.is_u16, mesh->color_is_u8 ? 1 : 0, V.scale, V.zmin, V.zmax};
  hipLaunchKernelGGL(k_rd_tiles, dim3((unsigned)n_tiles), dim3(kThreads), 0, s, M, C, (const int32_t *)L.counts,
                     (const int32_t *)L.offsets, lists, (long)E, O);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}
