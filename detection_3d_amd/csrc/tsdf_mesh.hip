// The TSDF volume of tsdf.hip -> a triangle mesh of its zero crossing: marching tetrahedra on the Kuhn split of every
// voxel cell (include/d3d_hip.h).  Six tetrahedra per cell, one per permutation of the axes, all sharing the
// cell's main diagonal; their faces match across cells, so there is no ambiguous face and the surface is closed wherever
// the cells around it are emitted.  A mesh vertex sits on an edge from a voxel g to g + e, e one of seven kinds (x, y, z,
// xy, xz, yz, xyz), and is owned by g: kinds 0..2 are the rows of d3d_tsdf_surface_rows.
//
// One workgroup of 512 lanes per block in coordinate order, one lane per voxel (and per cell), as in tsdf.hip.
//   count      stages the full 9^3 apron of tsdf and weight (load_apron with the seven forward neighbour blocks),
//              finds the voxel's 7-bit vertex mask and its cell's triangle count, ranks the vertices inside the block
//              and leaves one word per voxel: rank (12 bits, <= 3584), mask (7), inside (1), seen (1).  Per-block
//              totals, two 64-bit integer sums for the limits, two scans, one read-back.
//   vertices   stages the apron of tsdf alone, reads its words back, packs positions and colours in LDS and stores
//              whole lines; never past V.
//   triangles  stages, for the 9^3 apron, the index of each voxel's first vertex (its block's base plus its rank) and
//              its mask, inside and seen bits; a vertex is first + popcount(mask below its kind).  Triangles are ranked
//              by mbcnt over the ballots of the count's bits plus the waves' totals; never past T.
// Integer counters only; the case table (2 signs x 16 masks) is constant data.
#include "d3d_internal.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace d3d {

namespace {

#include "tsdf_volume.inc"

constexpr int kStageVerts = 512;                         // vertices packed in LDS per round of k_mesh_vertices
constexpr int kMaxBlockVerts = 7 * kVox, kMaxBlockTris = 12 * kVox;

// A cube corner is the bits cx | cy << 1 | cz << 2, an edge kind's direction likewise.
// kind -> direction, 3 bits each: x, y, z, xy, xz, yz, xyz
constexpr uint32_t kKindDir = 1u | 2u << 3 | 4u << 6 | 3u << 9 | 5u << 12 | 6u << 15 | 7u << 18;
// direction -> kind, 3 bits each from direction 1
constexpr uint32_t kDirKind = 0u << 3 | 1u << 6 | 3u << 9 | 2u << 12 | 4u << 15 | 5u << 18 | 6u << 21;

__host__ __device__ constexpr int kind_dir(int k) { return (int)(kKindDir >> (3 * k)) & 7; }
__host__ __device__ constexpr int dir_kind(int d) { return (int)(kDirKind >> (3 * d)) & 7; }
__host__ __device__ constexpr int apron_offset(int c) { return (c & 1) * 81 + ((c >> 1) & 1) * 9 + ((c >> 2) & 1); }

// corner j of tetrahedron t: the path 0, e_p1, e_p1 + e_p2, (1, 1, 1) of the t-th permutation p in lexicographic order
__host__ __device__ constexpr int tet_corner(int t, int j) {
  const int a1 = t >> 1;
  const int lo = a1 == 0 ? 1 : 0, hi = a1 == 2 ? 1 : 2;
  const int a2 = (t & 1) ? hi : lo;
  return j == 0 ? 0 : j == 1 ? 1 << a1 : j == 2 ? (1 << a1) | (1 << a2) : 7;
}
__host__ __device__ constexpr bool tet_plus(int t) { return (((t >> 1) + (t & 1)) & 1) == 0; }   // an even permutation

// The triangles of one case: n, then per triangle vertex the tetrahedron corners (inside, outside) of its edge.  The
// last two vertices of each triangle are swapped where the normal would point from outside to inside otherwise.
struct TetCase {
  int n;
  int v[6][2];
};
constexpr int kSwapPlus = 0x4D24, kSwapMinus = 0x32DA;   // masks {2, 5, 8, 10, 11, 14}; the other non-empty ones

constexpr TetCase tet_case(bool plus, int mask) {
  TetCase c{0, {{-1, -1}, {-1, -1}, {-1, -1}, {-1, -1}, {-1, -1}, {-1, -1}}};
  int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
  for (int j = 0; j < 4; j++) {
    if ((mask >> j) & 1) in[ni++] = j;
    else out[no++] = j;
  }
  if (ni == 0 || no == 0) return c;
  if (ni == 1) {
    c.n = 1;
    for (int k = 0; k < 3; k++) c.v[k][0] = in[0], c.v[k][1] = out[k];
  } else if (no == 1) {
    c.n = 1;
    for (int k = 0; k < 3; k++) c.v[k][0] = in[k], c.v[k][1] = out[0];
  } else {
    c.n = 2;
    const int q[4][2] = {{in[0], out[0]}, {in[0], out[1]}, {in[1], out[1]}, {in[1], out[0]}};
    const int pick[6] = {0, 1, 2, 0, 2, 3};
    for (int k = 0; k < 6; k++) c.v[k][0] = q[pick[k]][0], c.v[k][1] = q[pick[k]][1];
  }
  if (((plus ? kSwapPlus : kSwapMinus) >> mask) & 1) {
    for (int i = 0; i < c.n; i++) {
      for (int s = 0; s < 2; s++) {
        const int x = c.v[3 * i + 1][s];
        c.v[3 * i + 1][s] = c.v[3 * i + 2][s];
        c.v[3 * i + 2][s] = x;
      }
    }
  }
  return c;
}

// the device's form of a case: n in bits 0..1, then per triangle vertex 4 bits, the lower corner of its edge (the owner
// of the vertex) and the higher one
constexpr uint32_t tet_word(bool plus, int mask) {
  const TetCase c = tet_case(plus, mask);
  uint32_t w = (uint32_t)c.n;
  for (int k = 0; k < 3 * c.n; k++) {
    const int lo = c.v[k][0] < c.v[k][1] ? c.v[k][0] : c.v[k][1], hi = c.v[k][0] < c.v[k][1] ? c.v[k][1] : c.v[k][0];
    w |= (uint32_t)(lo | hi << 2) << (2 + 4 * k);
  }
  return w;
}
#define D3D_TET_ROW(P)                                                                                                  \
  {tet_word(P, 0), tet_word(P, 1), tet_word(P, 2), tet_word(P, 3), tet_word(P, 4), tet_word(P, 5), tet_word(P, 6),      \
   tet_word(P, 7), tet_word(P, 8), tet_word(P, 9), tet_word(P, 10), tet_word(P, 11), tet_word(P, 12), tet_word(P, 13),  \
   tet_word(P, 14), tet_word(P, 15)}
__constant__ const uint32_t kTetWords[2][16] = {D3D_TET_ROW(true), D3D_TET_ROW(false)};
#undef D3D_TET_ROW

// the word of a voxel that the count pass leaves
constexpr int kWordMaskShift = 12, kWordInside = 1 << 19, kWordSeen = 1 << 20;

// ---- count ----

// the triangles of the cell whose corners' inside bits are in8
__device__ __forceinline__ int cell_triangles(int in8) {
  int cnt = 0;
#pragma unroll
  for (int t = 0; t < 6; t++) {
    int mask = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) mask |= ((in8 >> tet_corner(t, j)) & 1) << j;
    cnt += mask == 0 || mask == 15 ? 0 : (__popc(mask) == 2 ? 2 : 1);
  }
  return cnt;
}

__global__ __launch_bounds__(kVox) void k_mesh_count(const int32_t *__restrict__ coords, const int32_t *__restrict__ order,
                                                     int n_blocks, const HashEntry *__restrict__ tab, int cap,
                                                     const float *__restrict__ tsdf, const float *__restrict__ weight,
                                                     double min_weight, uint32_t *__restrict__ words,
                                                     int32_t *__restrict__ vcounts, int32_t *__restrict__ tcounts,
                                                     unsigned long long *__restrict__ totals) {
  __shared__ Apron S;
  __shared__ int wave_v[kVox / 64], wave_t[kVox / 64];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int b = order[blockIdx.x];
  if ((unsigned)b >= (unsigned)n_blocks) {   // the same in every thread
    if (tid == 0) vcounts[blockIdx.x] = tcounts[blockIdx.x] = 0;
    return;
  }
  load_apron<true>(S, b, coords, tab, cap, n_blocks, tsdf, weight);
  const int at = ((tid >> 6) * 9 + ((tid >> 3) & 7)) * 9 + (tid & 7);
  const bool seen_g = (double)S.W[at] >= min_weight, in_g = S.D[at] < 0.f;   // false for NaN
  int mask = 0, in8 = in_g ? 1 : 0;
  bool all_seen = seen_g;
#pragma unroll
  for (int k = 0; k < 7; k++) {
    const int c = kind_dir(k), h = at + apron_offset(c);
    const bool seen_h = (double)S.W[h] >= min_weight, in_h = S.D[h] < 0.f;
    all_seen = all_seen && seen_h;
    in8 |= (in_h ? 1 : 0) << c;
    mask |= (seen_g && seen_h && in_g != in_h ? 1 : 0) << k;
  }
  const int nv = __popc(mask), nt = all_seen ? cell_triangles(in8) : 0;
  const unsigned long long v0 = __ballot(nv & 1), v1 = __ballot(nv & 2), v2 = __ballot(nv & 4);
  int rank = lanes_below(v0) + 2 * lanes_below(v1) + 4 * lanes_below(v2);
  const unsigned long long t0 = __ballot(nt & 1), t1 = __ballot(nt & 2), t2 = __ballot(nt & 4), t3 = __ballot(nt & 8);
  if ((tid & 63) == 0) {
    wave_v[wave] = __popcll(v0) + 2 * __popcll(v1) + 4 * __popcll(v2);
    wave_t[wave] = (__popcll(t0) + 2 * __popcll(t1)) + (4 * __popcll(t2) + 8 * __popcll(t3));
  }
  __syncthreads();
  int total_v = 0, total_t = 0;
#pragma unroll
  for (int w = 0; w < kVox / 64; w++) {
    rank += w < wave ? wave_v[w] : 0;
    total_v += wave_v[w];
    total_t += wave_t[w];
  }
  words[(size_t)b * kVox + tid] =
      (uint32_t)rank | (uint32_t)mask << kWordMaskShift | (in_g ? kWordInside : 0) | (seen_g ? kWordSeen : 0);
  if (tid == 0) {
    vcounts[blockIdx.x] = total_v;
    tcounts[blockIdx.x] = total_t;
    if (total_v) atomicAdd(&totals[0], (unsigned long long)total_v);
    if (total_t) atomicAdd(&totals[1], (unsigned long long)total_t);
  }
}

// base_of_block[id] = the first vertex of block id
__global__ void k_mesh_block_bases(const int32_t *__restrict__ order, const int32_t *__restrict__ vbases, int n_blocks,
                                   int32_t *__restrict__ base_of_block) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_blocks) return;
  const int b = order[i];
  if ((unsigned)b < (unsigned)n_blocks) base_of_block[b] = vbases[i];
}

// ---- vertices ----

__global__ __launch_bounds__(kVox) void k_mesh_vertices(const int32_t *__restrict__ coords, const int32_t *__restrict__ order,
                                                        int n_blocks, const HashEntry *__restrict__ tab, int cap,
                                                        const float *__restrict__ tsdf, const float *__restrict__ cstate,
                                                        const float *__restrict__ cweight, VolumeView G,
                                                        const uint32_t *__restrict__ words,
                                                        const int32_t *__restrict__ vcounts,
                                                        const int32_t *__restrict__ vbases, int n_verts,
                                                        float *__restrict__ out, float *__restrict__ out_color,
                                                        int32_t *__restrict__ edges) {
  __shared__ float D[kApron];
  __shared__ float stage[kStageVerts * 3], stage_c[kStageVerts * 3];
  __shared__ int nb[8];
  const int tid = threadIdx.x;
  const int b = order[blockIdx.x];
  if ((unsigned)b >= (unsigned)n_blocks) return;   // the same in every thread
  const int total = min(max(vcounts[blockIdx.x], 0), kMaxBlockVerts);
  if (total == 0) return;                    // the same in every thread
  find_neighbours<true>(nb, b, coords, tab, cap, n_blocks);
  for (int i = tid; i < kApron; i += kVox) {
    int o, voxel;
    apron_source(i, o, voxel);
    const int src = nb[o];
    D[i] = src >= 0 ? tsdf[(size_t)src * kVox + voxel] : 0.f;
  }
  __syncthreads();
  const uint32_t word = words[(size_t)b * kVox + tid];
  const int rank = (int)(word & 0xfff), mask = (int)(word >> kWordMaskShift) & 0x7f;
  const long row0 = vbases[blockIdx.x];
  if (row0 < 0) return;                      // the same in every thread; no count of a valid call is negative
  const int l[3] = {tid >> 6, (tid >> 3) & 7, tid & 7};
  const int at = (l[0] * 9 + l[1]) * 9 + l[2];
  int g[3];
#pragma unroll
  for (int i = 0; i < 3; i++) g[i] = 8 * coords[3 * (size_t)b + i] + l[i];
  const float Dg = D[at];
  for (int c0 = 0; c0 < total; c0 += kStageVerts) {
    int r = rank;
#pragma unroll
    for (int k = 0; k < 7; k++) {
      if (!((mask >> k) & 1)) continue;
      const int local = r - c0;
      r++;
      if (local < 0 || local >= kStageVerts) continue;
      const int e = kind_dir(k);
      const float Dh = D[at + apron_offset(e)];
      const double s = (double)Dg / ((double)Dg - (double)Dh);
      float *o = stage + local * 3;
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const double X = G.origin[i] + (double)g[i] * G.voxel;
        o[i] = (float)(((e >> i) & 1) ? X + s * G.voxel : X);
      }
      if (out_color) {
        float col[3] = {0.f, 0.f, 0.f};
        if (cstate) {
          int over = 0, lh[3];
#pragma unroll
          for (int i = 0; i < 3; i++) {
            const int p = l[i] + ((e >> i) & 1);
            over |= (p >> 3) << i;
            lh[i] = p & 7;
          }
          const int hb = nb[over];           // >= 0: the edge crosses, so the neighbour is allocated
          const size_t ig = (size_t)b * kVox + tid, ih = (size_t)max(hb, 0) * kVox + (lh[0] * 8 + lh[1]) * 8 + lh[2];
          const bool has_g = cweight[ig] > 0.f, has_h = hb >= 0 && cweight[ih] > 0.f;
#pragma unroll
          for (int c = 0; c < 3; c++) {
            if (has_g && has_h) {
              const double cg = (double)cstate[3 * ig + c], ch = (double)cstate[3 * ih + c];
              col[c] = (float)(cg + s * (ch - cg));
            } else if (has_g) {
              col[c] = cstate[3 * ig + c];
            } else if (has_h) {
              col[c] = cstate[3 * ih + c];
            }
          }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) stage_c[local * 3 + c] = col[c];
      }
      const long row = row0 + c0 + local;
      if (edges && row < n_verts) {
#pragma unroll
        for (int i = 0; i < 3; i++) edges[4 * row + i] = g[i];
        edges[4 * row + 3] = k;
      }
    }
    __syncthreads();
    // never past the vertices the caller allocated
    const long first = row0 + c0;
    const int rows = (int)std::min<long>(std::min(total - c0, kStageVerts), std::max<long>((long)n_verts - first, 0));
    for (int k = tid; k < rows * 3; k += kVox) out[first * 3 + k] = stage[k];
    if (out_color)
      for (int k = tid; k < rows * 3; k += kVox) out_color[first * 3 + k] = stage_c[k];
    __syncthreads();
  }
}

// ---- triangles ----

__global__ __launch_bounds__(kVox) void k_mesh_triangles(const int32_t *__restrict__ coords, const int32_t *__restrict__ order,
                                                         int n_blocks, const HashEntry *__restrict__ tab, int cap,
                                                         const uint32_t *__restrict__ words,
                                                         const int32_t *__restrict__ base_of_block,
                                                         const int32_t *__restrict__ tcounts,
                                                         const int32_t *__restrict__ tbases, int n_tris,
                                                         int32_t *__restrict__ out) {
  __shared__ int32_t first[kApron];          // the index of the voxel's first vertex
  __shared__ uint16_t bits[kApron];          // mask, inside (bit 7), seen (bit 8); 0: no such voxel
  __shared__ int nb[8];
  __shared__ int wave_t[kVox / 64];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int b = order[blockIdx.x];
  if ((unsigned)b >= (unsigned)n_blocks) return;   // the same in every thread
  if (tcounts[blockIdx.x] <= 0) return;      // the same in every thread
  find_neighbours<true>(nb, b, coords, tab, cap, n_blocks);
  for (int i = tid; i < kApron; i += kVox) {
    int o, voxel;
    apron_source(i, o, voxel);
    const int src = nb[o];
    int32_t f = 0;
    uint32_t w = 0;
    if (src >= 0) {
      w = words[(size_t)src * kVox + voxel];
      f = base_of_block[src] + (int32_t)(w & 0xfff);
    }
    first[i] = f;
    bits[i] = (uint16_t)(w >> kWordMaskShift);
  }
  __syncthreads();
  const int at = ((tid >> 6) * 9 + ((tid >> 3) & 7)) * 9 + (tid & 7);
  int in8 = 0;
  bool all_seen = true;
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const int w = bits[at + apron_offset(c)];
    all_seen = all_seen && ((w >> 8) & 1);
    in8 |= ((w >> 7) & 1) << c;
  }
  const int nt = all_seen ? cell_triangles(in8) : 0;
  const unsigned long long t0 = __ballot(nt & 1), t1 = __ballot(nt & 2), t2 = __ballot(nt & 4), t3 = __ballot(nt & 8);
  int rank = (lanes_below(t0) + 2 * lanes_below(t1)) + (4 * lanes_below(t2) + 8 * lanes_below(t3));
  if ((tid & 63) == 0) wave_t[wave] = (__popcll(t0) + 2 * __popcll(t1)) + (4 * __popcll(t2) + 8 * __popcll(t3));
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kVox / 64; w++) rank += w < wave ? wave_t[w] : 0;
  if (nt == 0) return;
  long row = (long)tbases[blockIdx.x] + rank;
#pragma unroll
  for (int t = 0; t < 6; t++) {
    int mask = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) mask |= ((in8 >> tet_corner(t, j)) & 1) << j;
    if (mask == 0 || mask == 15) continue;
    const uint32_t path = tet_corner(t, 1) << 3 | tet_corner(t, 2) << 6 | 7 << 9;
    const uint32_t cw = kTetWords[tet_plus(t) ? 0 : 1][mask];
    const int n = (int)(cw & 3);
    for (int i = 0; i < n; i++, row++) {
      if (row < 0 || row >= n_tris) continue;   // never outside the triangles the caller allocated
#pragma unroll
      for (int v = 0; v < 3; v++) {
        const uint32_t pair = cw >> (2 + 4 * (3 * i + v));
        const int lo = (int)(path >> (3 * (pair & 3))) & 7, hi = (int)(path >> (3 * ((pair >> 2) & 3))) & 7;
        const int owner = at + apron_offset(lo), kind = dir_kind(hi ^ lo);
        out[3 * row + v] = first[owner] + __popc(bits[owner] & ((1 << kind) - 1));
      }
    }
  }
}

// ---- insert ----

// block i of `in` gets id i in an empty table: the touch pass's probe sequence and bounds.  A coordinate out of range or
// met twice, or a table that runs full, sets state[kStFull]; nothing is written out of bounds.
__global__ void k_tsdf_insert(const int32_t *__restrict__ in, int n, HashEntry *tab, int cap, int32_t *coords,
                              int32_t *state) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) state[kStBlocks] = n;
  if (i >= n) return;
  const int x = in[3 * (size_t)i + 0], y = in[3 * (size_t)i + 1], z = in[3 * (size_t)i + 2];
  if (((x | y | z) & ~0xffff) != 0) {
    state[kStFull] = 1;
    return;
  }
  const uint64_t key = pack_key(0, x, y, z);
  uint32_t slot = hash_key(key) & (uint32_t)(cap - 1), round = 0;
  for (int probes = 0; probes < cap; probes++) {
    unsigned long long cur = __atomic_load_n((unsigned long long *)&tab[slot].key, __ATOMIC_RELAXED);
    if (cur == kEmptyKey) {
      cur = atomicCAS((unsigned long long *)&tab[slot].key, (unsigned long long)kEmptyKey, (unsigned long long)key);
      if (cur == kEmptyKey) {
        coords[3 * (size_t)i + 0] = x;
        coords[3 * (size_t)i + 1] = y;
        coords[3 * (size_t)i + 2] = z;
        tab[slot].val = i;
        return;
      }
    }
    if (cur == key) break;                   // the coordinate of another row
    slot = probe_next(slot, round, cap);
  }
  state[kStFull] = 1;
}

// ---- scratch ----

struct MeshLayout {
  unsigned long long *totals;                // V, T
  int32_t *vcounts, *tcounts, *vbases, *tbases, *base_of_block;
  uint32_t *words;                           // one per voxel of every block, by block id
};

int carve_mesh(Arena &A, int n, MeshLayout &L) {
  const size_t N = (size_t)n + 2;
  D3D_ALLOC(totals, unsigned long long, A, 32);
  D3D_ALLOC(vcounts, int32_t, A, N);
  D3D_ALLOC(tcounts, int32_t, A, N);
  D3D_ALLOC(vbases, int32_t, A, N);
  D3D_ALLOC(tbases, int32_t, A, N);
  D3D_ALLOC(base_of_block, int32_t, A, N);
  D3D_ALLOC(words, uint32_t, A, N * kVox);
  L = MeshLayout{totals, vcounts, tcounts, vbases, tbases, base_of_block, words};
  return D3D_OK;
}

// the carve plus what the two scans take from the arena behind it
size_t mesh_bytes(int n) {
  Arena A = sizing_arena();
  MeshLayout L;
  (void)carve_mesh(A, n, L);
  return A.used + 2 * (((size_t)n / 2048 + 1) * 4 + 4096);
}

int mesh_counts(const char *who, const int *info_host, int n_blocks, int &V, int &T) {
  D3D_REQUIRE(info_host, "%s: null pointer", who);
  V = info_host[0];
  T = info_host[1];
  D3D_REQUIRE(V >= 0 && (long)V <= (long)kMaxBlockVerts * n_blocks && T >= 0 && (long)T <= (long)kMaxBlockTris * n_blocks,
              "%s: %d vertices and %d triangles of %d blocks", who, V, T, n_blocks);
  return D3D_OK;
}

}  // namespace
}  // namespace d3d

using namespace d3d;

int d3d_tsdf_mesh_table(int8_t *out) {
  D3D_REQUIRE(out, "d3d_tsdf_mesh_table: null pointer");
  for (int t = 0; t < 6; t++) {
    for (int mask = 0; mask < 16; mask++) {
      const TetCase c = tet_case(tet_plus(t), mask);
      int8_t *o = out + (t * 16 + mask) * 13;
      o[0] = (int8_t)c.n;
      for (int k = 0; k < 6; k++) {
        o[1 + 2 * k] = (int8_t)c.v[k][0];
        o[2 + 2 * k] = (int8_t)c.v[k][1];
      }
    }
  }
  return D3D_OK;
}

size_t d3d_tsdf_mesh_scratch_bytes(int n_blocks) { return mesh_bytes(std::max(0, std::min(n_blocks, kMaxBlocks))); }

int d3d_tsdf_mesh_count(const d3d_tsdf_volume *volume, double min_weight, void *scratch, size_t scratch_bytes,
                        int *info_host, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(info_host, "d3d_tsdf_mesh_count: null pointer");
  info_host[0] = info_host[1] = 0;
  VolumeView G;
  int rc = volume_view("d3d_tsdf_mesh_count", volume, kVolBlocks | kVolLookup | kVolTsdf | kVolWeight, G);
  if (rc) return rc;
  const int n_blocks = volume->n_blocks;
  D3D_REQUIRE(min_weight >= 0.0, "d3d_tsdf_mesh_count: min_weight %g must not be negative", min_weight);
  if (n_blocks == 0) return D3D_OK;
  D3D_REQUIRE(scratch, "d3d_tsdf_mesh_count: null pointer");
  D3D_REQUIRE(scratch_bytes >= d3d_tsdf_mesh_scratch_bytes(n_blocks), "d3d_tsdf_mesh_count: scratch too small");
  Arena A = scratch_arena(scratch, scratch_bytes);
  MeshLayout L;
  rc = carve_mesh(A, n_blocks, L);
  if (rc) return rc;
  D3D_HIP_CHECK(hipMemsetAsync(L.totals, 0, 2 * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(k_mesh_count, dim3((unsigned)n_blocks), dim3(kVox), 0, s, (const int32_t *)volume->block_coords,
                     volume->order, n_blocks, (const HashEntry *)volume->table, volume->table_slots,
                     (const float *)volume->tsdf, (const float *)volume->weight, min_weight, L.words, L.vcounts, L.tcounts,
                     L.totals);
  D3D_LAUNCH_CHECK();
  rc = readback_publish(L.totals, 4, s);
  if (rc) return rc;
  // behind the publish: the host waits while these run.  Their sums wrap where a total is past the limit; the 64-bit
  // totals decide, and the caller gets no count to size or index anything with then.
  rc = scan_exclusive_i32(L.vcounts, L.vbases, n_blocks, nullptr, A, s);
  if (rc) return rc;
  rc = scan_exclusive_i32(L.tcounts, L.tbases, n_blocks, nullptr, A, s);
  if (rc) return rc;
  hipLaunchKernelGGL(k_mesh_block_bases, grid1d(n_blocks), dim3(256), 0, s, volume->order, (const int32_t *)L.vbases,
                     n_blocks, L.base_of_block);
  D3D_LAUNCH_CHECK();
  unsigned long long totals[2] = {0, 0};
  rc = readback_wait(totals, 4);
  if (rc) return rc;
  D3D_REQUIRE(totals[0] <= (unsigned long long)INT_MAX && totals[1] <= (unsigned long long)INT_MAX,
              "d3d_tsdf_mesh_count: %llu vertices and %llu triangles; int32 indices hold 2^31 - 1 (extract a part of "
              "the volume, or fuse at a larger voxel)", totals[0], totals[1]);
  info_host[0] = (int)totals[0];
  info_host[1] = (int)totals[1];
  return D3D_OK;
}

int d3d_tsdf_mesh_vertices(const d3d_tsdf_volume *volume, const int *info_host, const void *scratch,
                           size_t scratch_bytes, float *vertices, float *vertex_color, int32_t *edges, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  VolumeView G;
  int rc = volume_view("d3d_tsdf_mesh_vertices", volume, kVolGeometry | kVolBlocks | kVolLookup | kVolTsdf | kVolColor, G);
  if (rc) return rc;
  const int n_blocks = volume->n_blocks;
  int V = 0, T = 0;
  rc = mesh_counts("d3d_tsdf_mesh_vertices", info_host, n_blocks, V, T);
  if (rc) return rc;
  if (n_blocks == 0 || V == 0) return D3D_OK;
  D3D_REQUIRE(scratch && vertices, "d3d_tsdf_mesh_vertices: null pointer");
  D3D_REQUIRE(scratch_bytes >= d3d_tsdf_mesh_scratch_bytes(n_blocks), "d3d_tsdf_mesh_vertices: scratch too small");
  Arena A = scratch_arena(scratch, scratch_bytes);
  MeshLayout L;
  rc = carve_mesh(A, n_blocks, L);
  if (rc) return rc;
  hipLaunchKernelGGL(k_mesh_vertices, dim3((unsigned)n_blocks), dim3(kVox), 0, s, (const int32_t *)volume->block_coords,
                     volume->order, n_blocks, (const HashEntry *)volume->table, volume->table_slots,
                     (const float *)volume->tsdf, (const float *)volume->color_state, (const float *)volume->color_weight,
                     G, (const uint32_t *)L.words, (const int32_t *)L.vcounts, (const int32_t *)L.vbases, V, vertices,
                     vertex_color, edges);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

int d3d_tsdf_mesh_triangles(const d3d_tsdf_volume *volume, const int *info_host, const void *scratch,
                            size_t scratch_bytes, int32_t *triangles, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  VolumeView G;
  int rc = volume_view("d3d_tsdf_mesh_triangles", volume, kVolBlocks | kVolLookup, G);
  if (rc) return rc;
  const int n_blocks = volume->n_blocks;
  int V = 0, T = 0;
  rc = mesh_counts("d3d_tsdf_mesh_triangles", info_host, n_blocks, V, T);
  if (rc) return rc;
  if (n_blocks == 0 || T == 0) return D3D_OK;
  D3D_REQUIRE(scratch && triangles, "d3d_tsdf_mesh_triangles: null pointer");
  D3D_REQUIRE(scratch_bytes >= d3d_tsdf_mesh_scratch_bytes(n_blocks), "d3d_tsdf_mesh_triangles: scratch too small");
  Arena A = scratch_arena(scratch, scratch_bytes);
  MeshLayout L;
  rc = carve_mesh(A, n_blocks, L);
  if (rc) return rc;
  hipLaunchKernelGGL(k_mesh_triangles, dim3((unsigned)n_blocks), dim3(kVox), 0, s, (const int32_t *)volume->block_coords,
                     volume->order, n_blocks, (const HashEntry *)volume->table, volume->table_slots,
                     (const uint32_t *)L.words, (const int32_t *)L.base_of_block, (const int32_t *)L.tcounts,
                     (const int32_t *)L.tbases, T, triangles);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

int d3d_tsdf_insert_blocks(const int32_t *coords, int n, const d3d_tsdf_volume *volume, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  VolumeView G;
  int rc = volume_view("d3d_tsdf_insert_blocks", volume, kVolGrow, G);
  if (rc) return rc;
  D3D_REQUIRE(n >= 0 && n <= volume->max_blocks, "d3d_tsdf_insert_blocks: %d blocks into a volume of %d", n,
              volume->max_blocks);
  if (n == 0) return D3D_OK;
  D3D_REQUIRE(coords, "d3d_tsdf_insert_blocks: null pointer");
  hipLaunchKernelGGL(k_tsdf_insert, grid1d(n), dim3(256), 0, s, coords, n, (HashEntry *)volume->table, volume->table_slots,
                     volume->block_coords, volume->state);
  D3D_LAUNCH_CHECK();
  rc = readback_publish(volume->state, kStWords, s);
  if (rc) return rc;
  int32_t host[kStWords];
  rc = readback_wait(host, kStWords);
  if (rc) return rc;
  D3D_REQUIRE(!host[kStFull] && host[kStBlocks] == n,
              "d3d_tsdf_insert_blocks: a block coordinate outside [0, 65536) or given twice, or a table that was not "
              "empty; the table wants clearing");
  return D3D_OK;
}
