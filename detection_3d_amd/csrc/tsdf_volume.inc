// The block volume of tsdf.hip as its kernels see it, shared with tsdf_mesh.hip: the sizes, the state words, the volume's
// geometry, the bounded lookup of a block, the LDS apron of a block's tsdf and weight, and the host's one check of a
// d3d_tsdf_volume.  Included inside namespace d3d's anonymous namespace, after d3d_internal.h.

constexpr int kVox = 512;                                // voxels of a block = threads of its workgroup
constexpr int kApron = 9 * 9 * 9;
constexpr int kMaxBlocks = 1 << 22;

enum { kStBlocks = 0, kStClipped = 1, kStFull = 2, kStWords = 3 };   // state (device int32[>= 3])

struct VolumeView {
  double voxel, trunc, block;                // block = 8 voxel
  double origin[3];
};

// the id of block (x, y, z), or -1: absent, without storage, or outside the coordinate range.  At most `cap` probes.
__device__ __forceinline__ int block_find(const HashEntry *__restrict__ tab, int cap, int x, int y, int z, int n_blocks) {
  if (((x | y | z) & ~0xffff) != 0) return -1;
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const uint64_t key = pack_key(0, x, y, z);
  uint32_t slot = hash_key(key) & (uint32_t)(cap - 1), round = 0;
  for (int probes = 0; probes < cap; probes++) {
    const u32x4 e = *(const u32x4 *)&tab[slot];
    const uint64_t k = ((uint64_t)e[1] << 32) | e[0];
    if (k == key) return (unsigned)e[2] < (unsigned)n_blocks ? (int)e[2] : -1;
    if (k == kEmptyKey) return -1;
    slot = probe_next(slot, round, cap);
  }
  return -1;
}

// ---- the apron ----

// nb[o], o = ox | oy << 1 | oz << 2: the block at +o of block b, or -1; nb[0] = b.  DIAGONALS: whether the four
// neighbours across an edge or the corner (o = 3, 5, 6, 7) are looked up; without, they are -1 and cost no probe.
template <bool DIAGONALS>
__device__ __forceinline__ void find_neighbours(int *nb, int b, const int32_t *__restrict__ coords,
                                                const HashEntry *__restrict__ tab, int cap, int n_blocks) {
  const int o = threadIdx.x;
  if (o < 8) {
    int id = o == 0 ? b : -1;
    if (o != 0 && (DIAGONALS || (o & (o - 1)) == 0)) {
      const int x = coords[3 * (size_t)b + 0] + (o & 1), y = coords[3 * (size_t)b + 1] + ((o >> 1) & 1),
                z = coords[3 * (size_t)b + 2] + ((o >> 2) & 1);
      id = block_find(tab, cap, x, y, z, n_blocks);
    }
    nb[o] = id;
  }
  __syncthreads();
}

// apron cell i -> the neighbour o it lies in and its voxel there
__device__ __forceinline__ void apron_source(int i, int &o, int &voxel) {
  int a[3] = {i / 81, (i / 9) % 9, i % 9};
  o = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (a[k] == 8) {
      o |= 1 << k;
      a[k] = 0;
    }
  }
  voxel = (a[0] * 8 + a[1]) * 8 + a[2];
}

struct Apron {
  float D[kApron], W[kApron];                // W = NaN: no such voxel (its block is not allocated, or its D is not finite)
  int nb[8];                                 // find_neighbours
};

// stages block b's 9^3 apron of tsdf and weight.  Without DIAGONALS a cell across an edge or the corner has W = NaN.
template <bool DIAGONALS>
__device__ __forceinline__ void load_apron(Apron &S, int b, const int32_t *__restrict__ coords,
                                           const HashEntry *__restrict__ tab, int cap, int n_blocks,
                                           const float *__restrict__ tsdf, const float *__restrict__ weight) {
  find_neighbours<DIAGONALS>(S.nb, b, coords, tab, cap, n_blocks);
  for (int i = threadIdx.x; i < kApron; i += kVox) {
    int o, voxel;
    apron_source(i, o, voxel);
    const int src = S.nb[o];
    float D = 0.f, W = __builtin_nanf("");
    if (src >= 0) {
      D = tsdf[(size_t)src * kVox + voxel];
      W = weight[(size_t)src * kVox + voxel];
      if (!(fabsf(D) < INFINITY)) W = __builtin_nanf("");   // a tsdf that is not finite: not seen
    }
    S.D[i] = D;
    S.W[i] = W;
  }
  __syncthreads();
}

__device__ __forceinline__ int lanes_below(unsigned long long ballot) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

// ---- the host's check of a d3d_tsdf_volume ----

// What a call uses of the volume (include/d3d_hip.h has the table per entry point).  The pointers behind kVolBlocks,
// kVolLookup, kVolTsdf and kVolWeight are wanted only when there are blocks.
enum {
  kVolGeometry = 1,                          // voxel, origin
  kVolTrunc = 2,
  kVolGrow = 4,                              // max_blocks, a table of d3d_tsdf_table_slots(max_blocks), block_coords, state
  kVolBlocks = 8,                            // n_blocks, block_coords
  kVolLookup = 16,                           // a table of two slots per block at least, order
  kVolTsdf = 32,
  kVolWeight = 64,
  kVolColor = 128,                           // color_state and color_weight, both or neither
};

inline bool table_ok(const void *table, int slots, int max_blocks) {
  return table && slots >= 1024 && (slots & (slots - 1)) == 0 && (long)slots >= 2l * max_blocks;
}

// the checked descriptor -> the geometry; everything else a kernel takes is a typed field of the descriptor
inline int volume_view(const char *who, const d3d_tsdf_volume *v, int needs, VolumeView &G) {
  D3D_REQUIRE(v, "%s: null pointer", who);
  if (needs & kVolGeometry) {
    D3D_REQUIRE(v->voxel > 0.0 && v->voxel < (double)INFINITY, "%s: voxel %g must be positive and finite", who, v->voxel);
    D3D_REQUIRE(!(needs & kVolTrunc) || (v->trunc > 0.0 && v->trunc < (double)INFINITY),
                "%s: trunc %g must be positive and finite", who, v->trunc);
    for (int i = 0; i < 3; i++)
      D3D_REQUIRE(fabs(v->origin[i]) < (double)INFINITY, "%s: origin[%d] = %g must be finite", who, i, v->origin[i]);
  }
  G = VolumeView{v->voxel, (needs & kVolTrunc) ? v->trunc : v->voxel, 8.0 * v->voxel, {v->origin[0], v->origin[1], v->origin[2]}};
  if (needs & kVolGrow) {
    D3D_REQUIRE(v->max_blocks >= 1 && v->max_blocks <= kMaxBlocks, "%s: max_blocks %d outside [1, 2^22]", who, v->max_blocks);
    D3D_REQUIRE(table_ok(v->table, v->table_slots, v->max_blocks) && v->block_coords && v->state,
                "%s: the table has d3d_tsdf_table_slots(max_blocks) slots; null pointer", who);
  }
  if (needs & kVolBlocks) {
    D3D_REQUIRE(v->n_blocks >= 0 && v->n_blocks <= kMaxBlocks, "%s: %d blocks", who, v->n_blocks);
    const bool ok = v->n_blocks == 0 ||
                    (v->block_coords && (!(needs & kVolLookup) || (table_ok(v->table, v->table_slots, v->n_blocks) && v->order)) &&
                     (!(needs & kVolTsdf) || v->tsdf) && (!(needs & kVolWeight) || v->weight));
    if (needs & kVolLookup) D3D_REQUIRE(ok, "%s: null pointer, or a table of fewer than two slots per block", who);
    D3D_REQUIRE(ok, "%s: null pointer", who);
  }
  D3D_REQUIRE(!(needs & kVolColor) || !v->color_state == !v->color_weight, "%s: colour and colour weight go together", who);
  return D3D_OK;
}
