// Posed depth frames -> a truncated signed-distance volume (KinectFusion-style projective fusion) -> its surface
// cloud.  The arithmetic contract is written out in include/d3d_hip.h: fp64 in a stated order, every stored
// value rounded once to fp32, so that a numpy restatement gives the same bits.
//
// The voxels live in blocks of 8 x 8 x 8, found through the grid hash of d3d_internal.h (key: pack_key of the block
// coordinate, 16 bits per axis).  The caller owns every array: the table, the block coordinates [max_blocks, 3], three
// state words (blocks handed out, clipped, full) and the per-voxel state, block id major and the voxel inside the block
// as (lx 8 + ly) 8 + lz.  Block ids are handed out in the order the touch pass's atomics arrive, so they depend on
// scheduling; nothing a caller sees does: d3d_tsdf_order sorts the ids by coordinate and every output follows it.
//
// Three passes.
//   touch      one lane per pixel (k_up_count's mapping), 2 reach + 1 samples along its ray.  A sample probes with a
//              plain load; only a key that is absent costs a 64-bit compare-and-swap, and a lane drops a sample that
//              falls into the block of its previous one.  The winner of the swap takes the next id.  A table walk ends
//              after `slots` probes and no id past max_blocks gets storage: a full volume is a flag, never a fault.
//   integrate  one workgroup per block, one lane per voxel, the frames in ascending order with the sums in registers;
//              the state is read and written once.  Before the walk, lane t decides for frame t whether the block can
//              be skipped: a sphere about the block centre against the frame's depth-positive half space and the four
//              sides of its image, with a margin nine orders above the rounding of the test (block_culled).
//   surface    one workgroup per block in coordinate order stages the 9^3 apron of tsdf and weight in LDS (the +x, +y,
//              +z neighbour blocks through the hash), counts its crossing edges; scan; read-back; the rows kernel ranks
//              (voxel, axis) with mbcnt over the wave's ballots, packs rows in LDS and stores whole lines, and never
//              writes past the rows it was given.
// No float atomics: the only atomics are the swap on a table key and integer counters.
// The volume as a kernel sees it (sizes, state words, VolumeView, block_find, Apron and its staging) and the host's check
// of a d3d_tsdf_volume are tsdf_volume.inc, shared with tsdf_mesh.hip, which turns the same volume into a triangle mesh.
#include "d3d_internal.h"

#include <algorithm>
#include <cmath>

namespace d3d {

namespace {

#include "depth_frames.inc"
#include "tsdf_volume.inc"

constexpr int kTouchThreads = 256;
constexpr int kTouchSteps = 8;
constexpr int kTouchRun = kTouchThreads * kTouchSteps;   // pixels of one workgroup
constexpr int kStageRows = 512;                          // rows packed in LDS per round of k_tsdf_rows
constexpr int kMaxReach = 256;
constexpr double kBlockCoords = 65536.0;

// ---- touch ----

// block `key` = (qx, qy, qz) is in the table afterwards, or the volume is marked full
__device__ __forceinline__ void block_touch(HashEntry *tab, int cap, uint64_t key, int qx, int qy, int qz,
                                            int32_t *coords, int max_blocks, int32_t *state) {
  uint32_t slot = hash_key(key) & (uint32_t)(cap - 1), round = 0;
  for (int probes = 0; probes < cap; probes++) {
    unsigned long long cur = __atomic_load_n((unsigned long long *)&tab[slot].key, __ATOMIC_RELAXED);
    if (cur == kEmptyKey) {
      // no room: the key is not inserted, so the table never holds more than max_blocks keys plus those in flight
      if (__atomic_load_n(&state[kStBlocks], __ATOMIC_RELAXED) >= max_blocks) {
        state[kStFull] = 1;
        return;
      }
      cur = atomicCAS((unsigned long long *)&tab[slot].key, (unsigned long long)kEmptyKey, (unsigned long long)key);
      if (cur == kEmptyKey) {
        const int id = atomicAdd(&state[kStBlocks], 1);
        if (id < max_blocks) {
          coords[3 * (size_t)id + 0] = qx;
          coords[3 * (size_t)id + 1] = qy;
          coords[3 * (size_t)id + 2] = qz;
          tab[slot].val = id;
        } else {
          state[kStFull] = 1;                // val stays -1: the block has no storage
        }
        return;
      }
    }
    if (cur == key) return;
    slot = probe_next(slot, round, cap);
  }
  state[kStFull] = 1;
}

__global__ __launch_bounds__(kTouchThreads) void k_tsdf_touch(DepthView V, const double *__restrict__ intr,
                                                              const double *__restrict__ extr, VolumeView G, int reach,
                                                              HashEntry *tab, int cap, int32_t *coords, int max_blocks,
                                                              int32_t *state) {
  bool clipped = false;
  for (int it = 0; it < kTouchSteps; it++) {
    const long p = (long)blockIdx.x * kTouchRun + it * kTouchThreads + threadIdx.x;
    int f = 0, v = 0, u = 0;
    double z = 0.0;
    if (!kept_at(V, p, f, v, u, z)) continue;
    Camera K;
    load_camera(intr, extr, f, K);
    uint64_t last = kEmptyKey;
    for (int k = -reach; k <= reach; k++) {
      const double zk = z + (double)k * G.voxel;
      if (!(zk > 0.0)) continue;
      double C[3], q[3];
      cam_point(K, u, v, zk, C);
      bool inside = true;
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const double X = ((K.R[i][0] * C[0] + K.R[i][1] * C[1]) + K.R[i][2] * C[2]) + K.t[i];
        q[i] = floor((X - G.origin[i]) / G.block);
        inside = inside && q[i] >= 0.0 && q[i] < kBlockCoords;   // false for NaN
      }
      if (!inside) {
        clipped = true;
        continue;
      }
      const int qx = (int)q[0], qy = (int)q[1], qz = (int)q[2];
      const uint64_t key = pack_key(0, qx, qy, qz);
      if (key == last) continue;
      last = key;
      block_touch(tab, cap, key, qx, qy, qz, coords, max_blocks, state);
    }
  }
  if (clipped) state[kStClipped] = 1;        // every writer stores the same value
}

// ---- integrate ----

// True only when no voxel of the block whose centre is Xc can pass the tests of the walk for this frame.  Every voxel
// centre lies within rad = 4 sqrt(3) voxel of Xc (3.5 sqrt(3) in fact), so its camera coordinate c_j lies within
// r_j = |column j of R| rad of the centre's, whatever R is.  A voxel is skipped by the walk when c_2 <= 0, or when
// fx c_0 + (cx + 0.5) c_2 < 0 (pu < 0), or fx c_0 + (cx + 0.5 - W) c_2 >= 0 (pu >= W), likewise for v: linear in c, so
// the extreme over the box c_j +- r_j decides for all voxels.  tol is 1e-9 of the magnitudes involved, the rounding of
// the walk's chain 1e-15 of them.  Any NaN or inf makes a comparison false: no cull.
__device__ __forceinline__ bool block_culled(const Camera &K, const double (&Xc)[3], double rad, int W, int H) {
  double d[3], cc[3], r[3], mag = rad;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    d[i] = Xc[i] - K.t[i];
    mag += fabs(Xc[i]) + fabs(K.t[i]);
  }
  const double reach = rad + 1e-9 * mag;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    cc[j] = (K.R[0][j] * d[0] + K.R[1][j] * d[1]) + K.R[2][j] * d[2];
    r[j] = sqrt((K.R[0][j] * K.R[0][j] + K.R[1][j] * K.R[1][j]) + K.R[2][j] * K.R[2][j]) * reach * (1.0 + 1e-9);
  }
  if (cc[2] + r[2] <= 0.0) return true;
  const double zmag = fabs(cc[2]) + r[2];
  const double f[2] = {K.fx, K.fy}, c[2] = {K.cx, K.cy}, size[2] = {(double)W, (double)H};
#pragma unroll
  for (int a = 0; a < 2; a++) {
    const double lo = c[a] + 0.5, hi = c[a] + 0.5 - size[a];
    const double tol = 1e-9 * (fabs(f[a]) * (fabs(cc[a]) + r[a]) + (fabs(c[a]) + 1.0 + size[a]) * zmag);
    if (f[a] * cc[a] + lo * cc[2] + fabs(f[a]) * r[a] + fabs(lo) * r[2] < -tol) return true;
    if (f[a] * cc[a] + hi * cc[2] - fabs(f[a]) * r[a] - fabs(hi) * r[2] > tol) return true;
  }
  return false;
}

// COLOR: 0 no colour image, 1 uint8, 2 fp32
template <int COLOR>
__global__ __launch_bounds__(kVox) void k_tsdf_integrate(DepthView V, const void *__restrict__ color, double color_div,
                                                         const double *__restrict__ intr,
                                                         const double *__restrict__ extr, int frames, VolumeView G,
                                                         const int32_t *__restrict__ coords, float *tsdf, float *weight,
                                                         float *cstate, float *cweight,
                                                         unsigned long long *culled_pairs) {
  __shared__ unsigned char skip[kVox];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int g0[3] = {8 * coords[3 * (size_t)b + 0], 8 * coords[3 * (size_t)b + 1], 8 * coords[3 * (size_t)b + 2]};
  const int l[3] = {tid >> 6, (tid >> 3) & 7, tid & 7};
  double X[3], Xc[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    X[i] = G.origin[i] + (double)(g0[i] + l[i]) * G.voxel;
    Xc[i] = G.origin[i] + ((double)g0[i] + 3.5) * G.voxel;
  }
  const double rad = 6.9282032302755092 * G.voxel;   // 4 sqrt(3) voxel
  double S = 0.0, CS[3] = {0.0, 0.0, 0.0};
  int n = 0, cn = 0, culled = 0;
  for (int f0 = 0; f0 < frames; f0 += kVox) {
    const int nf = min(kVox, frames - f0);
    __syncthreads();
    if (tid < nf) {
      Camera K;
      load_camera(intr, extr, f0 + tid, K);
      skip[tid] = block_culled(K, Xc, rad, V.W, V.H) ? 1 : 0;
    }
    __syncthreads();
    for (int j = 0; j < nf; j++) {
      if (skip[j]) {                         // the same in every lane
        culled++;
        continue;
      }
      const int f = f0 + j;
      Camera K;
      load_camera(intr, extr, f, K);
      const double d[3] = {X[0] - K.t[0], X[1] - K.t[1], X[2] - K.t[2]};
      double c[3];
#pragma unroll
      for (int k = 0; k < 3; k++) c[k] = (K.R[0][k] * d[0] + K.R[1][k] * d[1]) + K.R[2][k] * d[2];
      if (!(c[2] > 0.0)) continue;
      const double pu = floor((c[0] * K.fx / c[2] + K.cx) + 0.5), pv = floor((c[1] * K.fy / c[2] + K.cy) + 0.5);
      if (!(pu >= 0.0 && pu < (double)V.W && pv >= 0.0 && pv < (double)V.H)) continue;   // false for NaN
      const long p = ((long)f * V.H + (int)pv) * V.W + (int)pu;
      const double zp = depth_at(V, p);
      if (!valid_z(V, zp)) continue;
      const double sdf = zp - c[2];
      if (sdf < -G.trunc) continue;
      const double q = sdf / G.trunc;
      S += q > 1.0 ? 1.0 : q;
      n++;
      if (COLOR != 0 && sdf <= G.trunc) {
        if (COLOR == 1) {
          const uint8_t *px = (const uint8_t *)color + 3 * p;
#pragma unroll
          for (int k = 0; k < 3; k++) CS[k] += (double)px[k] / color_div;
        } else {
          const float *px = (const float *)color + 3 * p;
#pragma unroll
          for (int k = 0; k < 3; k++) CS[k] += (double)px[k];
        }
        cn++;
      }
    }
  }
  const size_t i = (size_t)b * kVox + tid;
  if (n > 0) {
    const double w = (double)weight[i], wn = w + (double)n;
    tsdf[i] = (float)((w * (double)tsdf[i] + S) / wn);
    weight[i] = (float)wn;
  }
  if (COLOR != 0 && cn > 0) {
    const double w = (double)cweight[i], wn = w + (double)cn;
#pragma unroll
    for (int k = 0; k < 3; k++) cstate[3 * i + k] = (float)((w * (double)cstate[3 * i + k] + CS[k]) / wn);
    cweight[i] = (float)wn;
  }
  if (culled_pairs && tid == 0 && culled) atomicAdd(culled_pairs, (unsigned long long)culled);
}

// ---- order ----

__global__ void k_tsdf_digits(const int32_t *__restrict__ coords, int n, uint32_t *cx, uint32_t *cy, uint32_t *cz,
                              int32_t *iota) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  cx[i] = (uint32_t)coords[3 * (size_t)i + 0];
  cy[i] = (uint32_t)coords[3 * (size_t)i + 1];
  cz[i] = (uint32_t)coords[3 * (size_t)i + 2];
  iota[i] = i;
}

struct OrderLayout {
  uint32_t *cx, *cy, *cz, *ktmp;
  int32_t *perm_a;
};

int carve_order(Arena &A, int n, OrderLayout &L) {
  const size_t N = (size_t)n + 2;
  D3D_ALLOC(cx, uint32_t, A, N);
  D3D_ALLOC(cy, uint32_t, A, N);
  D3D_ALLOC(cz, uint32_t, A, N);
  D3D_ALLOC(ktmp, uint32_t, A, N);
  D3D_ALLOC(perm_a, int32_t, A, N);
  L = OrderLayout{cx, cy, cz, ktmp, perm_a};
  return D3D_OK;
}

// ---- surface ----

// block_find, Apron, load_apron: tsdf_volume.inc.  The edges of a voxel run along the axes, so the face neighbours do.
struct Edges {
  float Dg, Dh[3];
  bool seen_h[3], cross[3];
};

// voxel `tid` of the staged block: its forward neighbours and which of its three edges cross the surface
__device__ __forceinline__ void voxel_edges(const Apron &S, int tid, double min_weight, Edges &E) {
  const int l[3] = {tid >> 6, (tid >> 3) & 7, tid & 7};
  const int at = (l[0] * 9 + l[1]) * 9 + l[2];
  const int stride[3] = {81, 9, 1};
  E.Dg = S.D[at];
  const bool seen_g = (double)S.W[at] >= min_weight;   // false for NaN
#pragma unroll
  for (int a = 0; a < 3; a++) {
    E.Dh[a] = S.D[at + stride[a]];
    E.seen_h[a] = (double)S.W[at + stride[a]] >= min_weight;
    E.cross[a] = seen_g && E.seen_h[a] && ((E.Dg < 0.f) != (E.Dh[a] < 0.f));
  }
}

__global__ __launch_bounds__(kVox) void k_tsdf_count(const int32_t *__restrict__ coords, const int32_t *__restrict__ order,
                                                     int n_blocks, const HashEntry *__restrict__ tab, int cap,
                                                     const float *__restrict__ tsdf, const float *__restrict__ weight,
                                                     double min_weight, int32_t *__restrict__ counts) {
  __shared__ Apron S;
  __shared__ int wave_cnt[kVox / 64];
  const int tid = threadIdx.x;
  const int b = order[blockIdx.x];
  if ((unsigned)b >= (unsigned)n_blocks) {   // the same in every thread
    if (tid == 0) counts[blockIdx.x] = 0;
    return;
  }
  load_apron<false>(S, b, coords, tab, cap, n_blocks, tsdf, weight);
  Edges E;
  voxel_edges(S, tid, min_weight, E);
  const int cnt = (__popcll(__ballot(E.cross[0])) + __popcll(__ballot(E.cross[1]))) + __popcll(__ballot(E.cross[2]));
  if ((tid & 63) == 0) wave_cnt[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < kVox / 64; w++) total += wave_cnt[w];
    counts[blockIdx.x] = total;
  }
}

template <int NC>
__global__ __launch_bounds__(kVox) void k_tsdf_rows(const int32_t *__restrict__ coords, const int32_t *__restrict__ order,
                                                    int n_blocks, const HashEntry *__restrict__ tab, int cap,
                                                    const float *__restrict__ tsdf, const float *__restrict__ weight,
                                                    const float *__restrict__ cstate, const float *__restrict__ cweight,
                                                    VolumeView G, double min_weight, const int32_t *__restrict__ bases,
                                                    int n_rows, float *__restrict__ out, int32_t *__restrict__ voxels) {
  __shared__ Apron S;
  __shared__ float stage[kStageRows * NC];
  __shared__ int wave_cnt[kVox / 64];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int b = order[blockIdx.x];
  if ((unsigned)b >= (unsigned)n_blocks) return;   // the same in every thread
  load_apron<false>(S, b, coords, tab, cap, n_blocks, tsdf, weight);
  Edges E;
  voxel_edges(S, tid, min_weight, E);
  const unsigned long long b0 = __ballot(E.cross[0]), b1 = __ballot(E.cross[1]), b2 = __ballot(E.cross[2]);
  int rank = (lanes_below(b0) + lanes_below(b1)) + lanes_below(b2);   // rows of the wave's lower voxels
  if ((tid & 63) == 0) wave_cnt[wave] = (__popcll(b0) + __popcll(b1)) + __popcll(b2);
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int w = 0; w < kVox / 64; w++) {
    const int c = wave_cnt[w];
    rank += w < wave ? c : 0;
    total += c;
  }
  if (total == 0) return;                    // the same in every thread
  const long row0 = bases[blockIdx.x];
  const int l[3] = {tid >> 6, (tid >> 3) & 7, tid & 7};
  int g[3];
#pragma unroll
  for (int i = 0; i < 3; i++) g[i] = 8 * coords[3 * (size_t)b + i] + l[i];
  // the normal is the voxel's, shared by its rows
  float nrm[3] = {0.f, 0.f, 0.f};
  if (NC >= 9 && (E.cross[0] || E.cross[1] || E.cross[2])) {
    bool ok = fabsf(E.Dg) < 1.f;
#pragma unroll
    for (int k = 0; k < 3; k++) ok = ok && E.seen_h[k] && fabsf(E.Dh[k]) < 1.f;
    if (ok) {
      const double m[3] = {(double)E.Dh[0] - (double)E.Dg, (double)E.Dh[1] - (double)E.Dg, (double)E.Dh[2] - (double)E.Dg};
      const double l2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
      if (l2 > 0.0) {
        const double len = sqrt(l2);
#pragma unroll
        for (int k = 0; k < 3; k++) nrm[k] = (float)(m[k] / len);
      }
    }
  }
  for (int c0 = 0; c0 < total; c0 += kStageRows) {
    int r = rank;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      if (!E.cross[a]) continue;
      const int local = r - c0;
      r++;
      if (local < 0 || local >= kStageRows) continue;
      const double s = (double)E.Dg / ((double)E.Dg - (double)E.Dh[a]);
      float *o = stage + local * NC;
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const double X = G.origin[i] + (double)g[i] * G.voxel;
        o[i] = (float)(i == a ? X + s * G.voxel : X);
      }
      if (NC >= 6) {
        float col[3] = {0.f, 0.f, 0.f};
        if (cstate) {
          int lh[3] = {l[0], l[1], l[2]};
          const int hb = lh[a] == 7 ? S.nb[1 << a] : b;   // >= 0: the edge crosses, so the neighbour is allocated
          lh[a] = (lh[a] + 1) & 7;
          const size_t ig = (size_t)b * kVox + tid, ih = (size_t)hb * kVox + (lh[0] * 8 + lh[1]) * 8 + lh[2];
          const bool has_g = cweight[ig] > 0.f, has_h = hb >= 0 && cweight[ih] > 0.f;
#pragma unroll
          for (int k = 0; k < 3; k++) {
            if (has_g && has_h) {
              const double cg = (double)cstate[3 * ig + k], ch = (double)cstate[3 * ih + k];
              col[k] = (float)(cg + s * (ch - cg));
            } else if (has_g) {
              col[k] = cstate[3 * ig + k];
            } else if (has_h) {
              col[k] = cstate[3 * ih + k];
            }
          }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) o[3 + k] = col[k];
      }
      if (NC >= 9) {
#pragma unroll
        for (int k = 0; k < 3; k++) o[6 + k] = nrm[k];
      }
      const long row = row0 + c0 + local;
      if (voxels && row < n_rows) {
#pragma unroll
        for (int i = 0; i < 3; i++) voxels[3 * row + i] = g[i];
      }
    }
    __syncthreads();
    // never past the rows the caller allocated, whatever the volume holds by now
    const long first = row0 + c0;
    const int rows = (int)std::min<long>(std::min(total - c0, kStageRows), std::max<long>((long)n_rows - first, 0));
    float *dst = out + first * NC;
    for (int k = tid; k < rows * NC; k += kVox) dst[k] = stage[k];
    __syncthreads();
  }
}

struct SurfaceLayout {
  int32_t *total, *counts, *bases;
};

int carve_surface(Arena &A, int n, SurfaceLayout &L) {
  const size_t N = (size_t)n + 2;
  D3D_ALLOC(total, int32_t, A, 64);
  D3D_ALLOC(counts, int32_t, A, N);
  D3D_ALLOC(bases, int32_t, A, N);
  L = SurfaceLayout{total, counts, bases};
  return D3D_OK;
}

// the carve of an op plus what its scans and sorts take from the arena behind it
size_t order_bytes(int n) {
  Arena A = sizing_arena();
  OrderLayout L;
  (void)carve_order(A, n, L);
  return A.used + sort_scratch_bytes(n + 2, 16) + 4096;
}
size_t surface_bytes(int n) {
  Arena A = sizing_arena();
  SurfaceLayout L;
  (void)carve_surface(A, n, L);
  return A.used + ((size_t)n / 2048 + 1) * 4 + 4096;
}

}  // namespace
}  // namespace d3d

using namespace d3d;

int d3d_tsdf_table_slots(int max_blocks) {
  long c = 1024;
  while (c < 2l * std::max(0, std::min(max_blocks, kMaxBlocks))) c <<= 1;
  return (int)c;
}

int d3d_tsdf_touch(const d3d_depth_frames *frames, int step, double min_depth, double max_depth,
                   const d3d_tsdf_volume *volume, int reach, int *info_host, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(info_host, "d3d_tsdf_touch: null pointer");
  info_host[0] = info_host[1] = info_host[2] = 0;
  DepthView V;
  int rc = frames_view("d3d_tsdf_touch", frames, step, min_depth, max_depth, kFramesDepth | kFramesCameras, V);
  if (rc) return rc;
  VolumeView G;
  rc = volume_view("d3d_tsdf_touch", volume, kVolGeometry | kVolGrow, G);
  if (rc) return rc;
  D3D_REQUIRE(reach >= 0 && reach <= kMaxReach, "d3d_tsdf_touch: reach %d outside [0, %d] voxels", reach, kMaxReach);
  if (V.P > 0) {
    hipLaunchKernelGGL(k_tsdf_touch, dim3((unsigned)((V.P + kTouchRun - 1) / kTouchRun)), dim3(kTouchThreads), 0, s, V,
                       frames->intrinsics, frames->extrinsics, G, reach, (HashEntry *)volume->table, volume->table_slots,
                       volume->block_coords, volume->max_blocks, volume->state);
    D3D_LAUNCH_CHECK();
  }
  rc = readback_publish(volume->state, kStWords, s);
  if (rc) return rc;
  int32_t host[kStWords];
  rc = readback_wait(host, kStWords);
  if (rc) return rc;
  info_host[0] = host[kStBlocks];
  info_host[1] = host[kStClipped];
  info_host[2] = (host[kStFull] || host[kStBlocks] > volume->max_blocks || host[kStBlocks] < 0) ? 1 : 0;
  return D3D_OK;
}

int d3d_tsdf_integrate(const d3d_depth_frames *frames, double min_depth, double max_depth, double color_div,
                       const d3d_tsdf_volume *volume, int first_new, unsigned long long *culled_pairs, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  DepthView V;
  int rc = frames_view("d3d_tsdf_integrate", frames, 1, min_depth, max_depth, kFramesDepth | kFramesCameras, V);
  if (rc) return rc;
  VolumeView G;
  rc = volume_view("d3d_tsdf_integrate", volume, kVolGeometry | kVolTrunc | kVolBlocks | kVolTsdf | kVolWeight, G);
  if (rc) return rc;
  const int n_blocks = volume->n_blocks;
  float *tsdf = volume->tsdf, *weight = volume->weight, *color_state = volume->color_state,
        *color_weight = volume->color_weight;
  const void *color = frames->color;
  D3D_REQUIRE(first_new >= 0 && first_new <= n_blocks, "d3d_tsdf_integrate: %d blocks, the new ones from %d", n_blocks,
              first_new);
  D3D_REQUIRE(!(color && frames->color_is_u8) || (color_div > 0.0 && color_div < (double)INFINITY),
              "d3d_tsdf_integrate: color_div %g must be positive and finite", color_div);
  D3D_REQUIRE(!color || (color_state && color_weight), "d3d_tsdf_integrate: a colour image and a volume without colour");
  if (n_blocks == 0) return D3D_OK;
  const size_t at = (size_t)first_new * kVox, fresh = (size_t)(n_blocks - first_new) * kVox;
  if (fresh > 0) {                           // blocks the touch pass added: all state zero
    D3D_HIP_CHECK(hipMemsetAsync(tsdf + at, 0, fresh * sizeof(float), s));
    D3D_HIP_CHECK(hipMemsetAsync(weight + at, 0, fresh * sizeof(float), s));
    if (color_state) D3D_HIP_CHECK(hipMemsetAsync(color_state + 3 * at, 0, 3 * fresh * sizeof(float), s));
    if (color_weight) D3D_HIP_CHECK(hipMemsetAsync(color_weight + at, 0, fresh * sizeof(float), s));
  }
  if (V.P == 0) return D3D_OK;
  const dim3 grid((unsigned)n_blocks), block(kVox);
#define D3D_TSDF_INTEGRATE(COLOR)                                                                                         \
  hipLaunchKernelGGL(k_tsdf_integrate<COLOR>, grid, block, 0, s, V, color, color_div, frames->intrinsics,                \
                     frames->extrinsics, frames->frames, G, (const int32_t *)volume->block_coords, tsdf, weight, color_state, \
                     color_weight, culled_pairs)
  if (!color) D3D_TSDF_INTEGRATE(0);
  else if (frames->color_is_u8) D3D_TSDF_INTEGRATE(1);
  else D3D_TSDF_INTEGRATE(2);
#undef D3D_TSDF_INTEGRATE
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

size_t d3d_tsdf_order_scratch_bytes(int n_blocks) { return order_bytes(std::max(0, std::min(n_blocks, kMaxBlocks))); }

int d3d_tsdf_order(const int32_t *block_coords, int n_blocks, int32_t *order, void *scratch, size_t scratch_bytes,
                   void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(n_blocks >= 0 && n_blocks <= kMaxBlocks, "d3d_tsdf_order: %d blocks", n_blocks);
  if (n_blocks == 0) return D3D_OK;
  D3D_REQUIRE(block_coords && order && scratch, "d3d_tsdf_order: null pointer");
  D3D_REQUIRE(scratch_bytes >= d3d_tsdf_order_scratch_bytes(n_blocks), "d3d_tsdf_order: scratch too small");
  Arena A = scratch_arena(scratch, scratch_bytes);
  OrderLayout L;
  const int rc = carve_order(A, n_blocks, L);
  if (rc) return rc;
  hipLaunchKernelGGL(k_tsdf_digits, grid1d(n_blocks), dim3(256), 0, s, block_coords, n_blocks, L.cx, L.cy, L.cz, L.perm_a);
  D3D_LAUNCH_CHECK();
  return sort_cells_zyx(L.cx, L.cy, L.cz, L.perm_a, order, L.ktmp, n_blocks, 16, 16, A, s);
}

size_t d3d_tsdf_surface_scratch_bytes(int n_blocks) { return surface_bytes(std::max(0, std::min(n_blocks, kMaxBlocks))); }

int d3d_tsdf_surface_count(const d3d_tsdf_volume *volume, double min_weight, void *scratch, size_t scratch_bytes,
                           int *info_host, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(info_host, "d3d_tsdf_surface_count: null pointer");
  info_host[0] = 0;
  VolumeView G;
  int rc = volume_view("d3d_tsdf_surface_count", volume, kVolBlocks | kVolLookup | kVolTsdf | kVolWeight, G);
  if (rc) return rc;
  const int n_blocks = volume->n_blocks;
  D3D_REQUIRE(min_weight >= 0.0, "d3d_tsdf_surface_count: min_weight %g must not be negative", min_weight);
  if (n_blocks == 0) return D3D_OK;
  D3D_REQUIRE(scratch, "d3d_tsdf_surface_count: null pointer");
  D3D_REQUIRE(scratch_bytes >= d3d_tsdf_surface_scratch_bytes(n_blocks), "d3d_tsdf_surface_count: scratch too small");
  Arena A = scratch_arena(scratch, scratch_bytes);
  SurfaceLayout L;
  rc = carve_surface(A, n_blocks, L);
  if (rc) return rc;
  hipLaunchKernelGGL(k_tsdf_count, dim3((unsigned)n_blocks), dim3(kVox), 0, s, (const int32_t *)volume->block_coords,
                     volume->order, n_blocks, (const HashEntry *)volume->table, volume->table_slots,
                     (const float *)volume->tsdf, (const float *)volume->weight, min_weight, L.counts);
  D3D_LAUNCH_CHECK();
  rc = scan_exclusive_i32(L.counts, L.bases, n_blocks, L.total, A, s);
  if (rc) return rc;
  rc = readback_publish(L.total, 1, s);
  if (rc) return rc;
  return readback_wait(info_host, 1);
}

int d3d_tsdf_surface_rows(const d3d_tsdf_volume *volume, double min_weight, int ncols, const int *info_host,
                          const void *scratch, size_t scratch_bytes, float *out, int32_t *voxels, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(info_host, "d3d_tsdf_surface_rows: null pointer");
  D3D_REQUIRE(ncols == 3 || ncols == 6 || ncols == 9, "d3d_tsdf_surface_rows: %d columns (3, 6 or 9)", ncols);
  VolumeView G;
  int rc = volume_view("d3d_tsdf_surface_rows", volume,
                       kVolGeometry | kVolBlocks | kVolLookup | kVolTsdf | kVolWeight | kVolColor, G);
  if (rc) return rc;
  const int n_blocks = volume->n_blocks;
  D3D_REQUIRE(min_weight >= 0.0, "d3d_tsdf_surface_rows: min_weight %g must not be negative", min_weight);
  const int N = info_host[0];
  D3D_REQUIRE(N >= 0 && (long)N <= 3l * kVox * n_blocks, "d3d_tsdf_surface_rows: %d rows of %d blocks", N, n_blocks);
  if (n_blocks == 0 || N == 0) return D3D_OK;
  D3D_REQUIRE(scratch && out, "d3d_tsdf_surface_rows: null pointer");
  D3D_REQUIRE(scratch_bytes >= d3d_tsdf_surface_scratch_bytes(n_blocks), "d3d_tsdf_surface_rows: scratch too small");
  Arena A = scratch_arena(scratch, scratch_bytes);
  SurfaceLayout L;
  rc = carve_surface(A, n_blocks, L);
  if (rc) return rc;
  const dim3 grid((unsigned)n_blocks), block(kVox);
#define D3D_TSDF_ROWS(NC)                                                                                              \
  hipLaunchKernelGGL(k_tsdf_rows<NC>, grid, block, 0, s, (const int32_t *)volume->block_coords, volume->order, n_blocks, \
                     (const HashEntry *)volume->table, volume->table_slots, (const float *)volume->tsdf,               \
                     (const float *)volume->weight, (const float *)volume->color_state,                                \
                     (const float *)volume->color_weight, G, min_weight, (const int32_t *)L.bases, N, out, voxels)
  if (ncols == 3) D3D_TSDF_ROWS(3);
  else if (ncols == 6) D3D_TSDF_ROWS(6);
  else D3D_TSDF_ROWS(9);
#undef D3D_TSDF_ROWS
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}
