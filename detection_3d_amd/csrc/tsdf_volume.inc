// The block volume of tsdf.hip as its kernels see it, shared with tsdf_mesh.hip: the sizes, the state words, the volume's
// geometry, the bounded lookup of a block and the LDS apron of a block's tsdf and weight.  Included inside namespace d3d's
// anonymous namespace, after d3d_internal.h.

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

struct Apron {
  float D[kApron], W[kApron];                // W = NaN: no such voxel (its block is not allocated, or its D is not finite)
  int nb[3];                                 // the +x, +y, +z neighbour blocks, or -1
};

__device__ __forceinline__ int lanes_below(unsigned long long ballot) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

inline int make_volume(const char *who, double voxel, double trunc, const double *origin, VolumeView &G) {
  D3D_REQUIRE(voxel > 0.0 && voxel < (double)INFINITY, "%s: voxel %g must be positive and finite", who, voxel);
  D3D_REQUIRE(trunc > 0.0 && trunc < (double)INFINITY, "%s: trunc %g must be positive and finite", who, trunc);
  D3D_REQUIRE(origin, "%s: null pointer", who);
  for (int i = 0; i < 3; i++)
    D3D_REQUIRE(fabs(origin[i]) < (double)INFINITY, "%s: origin[%d] = %g must be finite", who, i, origin[i]);
  G = VolumeView{voxel, trunc, 8.0 * voxel, {origin[0], origin[1], origin[2]}};
  return D3D_OK;
}

inline bool table_ok(const void *table, int slots, int max_blocks) {
  return table && slots >= 1024 && (slots & (slots - 1)) == 0 && (long)slots >= 2l * max_blocks;
}
