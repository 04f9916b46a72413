// What the RoIAlignRotated3D files share (roi_forward.hip, roi_backward.hip, roi_backward_det.hip): the geometry of a
// RoI, its sample positions and the interpolation set-up (maskrcnn_benchmark/csrc/cuda/ROIAlignRotated3D_cuda.cu:15-62,
// :150-163), the form record and the grid look-up of the backward entry points.  Included inside namespace d3d, after
// grid_internal.h.

struct RoiGeom {
  int b;
  float cw, ch, cz, bh, bw, bz, sh, sw, sz, cosT, sinT;
  int gh, gw, gz;
};
__device__ __forceinline__ RoiGeom roi_geom(const float *r, float spatial_scale, int PH, int PW, int PZ,
                                            int sampling_ratio) {
  RoiGeom g;
  g.b = (int)r[0];
  g.cw = r[1] * spatial_scale;
  g.ch = r[2] * spatial_scale;
  g.cz = r[3] * spatial_scale;
  float rw = r[4] * spatial_scale, rh = r[5] * spatial_scale, rz = r[6] * spatial_scale;
  const float theta = (float)((double)r[7] * 3.14159265358979323846 / 180.0);
  rw = fmaxf(rw, 1.f);
  rh = fmaxf(rh, 1.f);
  rz = fmaxf(rz, 1.f);
  g.bh = rh / (float)PH;
  g.bw = rw / (float)PW;
  g.bz = rz / (float)PZ;
  g.gh = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rh / PH);
  g.gw = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rw / PW);
  g.gz = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rz / PZ);
  g.sh = (float)(-rh / 2.0);
  g.sw = (float)(-rw / 2.0);
  g.sz = (float)(-rz / 2.0);
  g.cosT = (float)cos((double)theta);
  g.sinT = (float)sin((double)theta);
  return g;
}
// sample position of (bin, sub-sample) in map coordinates (:150-163)
__device__ __forceinline__ void sample_pos(const RoiGeom &g, int ph, int pw, int pz, int iy, int ix,
                                           int iz, float &y, float &x, float &z) {
  const float yy = g.sh + ph * g.bh + (float)(iy + .5f) * g.bh / (float)g.gh;
  const float xx = g.sw + pw * g.bw + (float)(ix + .5f) * g.bw / (float)g.gw;
  const float zz = g.sz + pz * g.bz + (float)(iz + .5f) * g.bz / (float)g.gz;
  x = xx * g.cosT + yy * g.sinT + g.cw;
  y = yy * g.cosT - xx * g.sinT + g.ch;
  z = zz + g.cz;
}
// interpolation set-up of bilinear_interpolate (:15-62): returns false for an empty sample
struct Tri {
  int yl, yh, xl, xh, zl, zh;
  float ly, lx, lz, hy, hx, hz;
};
__device__ __forceinline__ bool tri_setup(float y, float x, float z, int H, int W, int Z, Tri &t) {
  if (y < -1.0 || y > H || x < -1.0 || x > W || z < -1.0) return false;
  if (y <= 0) y = 0;
  if (x <= 0) x = 0;
  if (z <= 0) z = 0;
  t.yl = (int)y;
  t.xl = (int)x;
  t.zl = (int)z;
  if (t.yl >= H - 1) { t.yh = t.yl = H - 1; y = (float)t.yl; } else t.yh = t.yl + 1;
  if (t.xl >= W - 1) { t.xh = t.xl = W - 1; x = (float)t.xl; } else t.xh = t.xl + 1;
  if (t.zl >= Z - 1) { t.zh = t.zl = Z - 1; z = (float)t.zl; } else t.zh = t.zl + 1;
  t.ly = y - t.yl;
  t.lx = x - t.xl;
  t.lz = z - t.zl;
  t.hy = 1. - t.ly;
  t.hx = 1. - t.lx;
  t.hz = 1. - t.lz;
  return true;
}

// d3d_roi_last_form: what the calling thread's last RoIAlign call launched (host stores only).  family (1 k_roi_dense,
// 2 k_roi_sparse, 3 k_roi_dense_bwd, 4 k_roi_sparse_bwd, 5 the fixed-order backward), storage type (1 fp32, 2 bf16),
// lookup (bit 0: a level probes the hash table, bit 1: a level reads the dense index; 0 for the dense kernels), extent
// (1 the caller's crop, 2 read on the device, 0 for the dense kernels), grid x / y / z and workgroup size of the family's
// main kernel (5: k_roi_det_sum), levels with a table, workgroups of k_roi_f32_to_bf16 (4 on bf16 rows), and for 5
// n_max, n_chunks and the sort's key bits.  A call that launches nothing leaves the record as it is.
// The record is one object for the three files that write it: defined, with roi_record, in roi_forward.hip.
static constexpr int kRoiFormFields = 13;
extern thread_local int t_roi_last_form[kRoiFormFields];
enum RoiFamily { kRoiFamDense = 1, kRoiFamSparse = 2, kRoiFamDenseBwd = 3, kRoiFamSparseBwd = 4, kRoiFamDet = 5 };
void roi_record(int family, size_t type_bytes, int lookup, int extent, dim3 grid, int block, int levels, long cvt = 0,
                long n_max = 0, long n_chunks = 0, int bits = 0);

// the grid of spatial size `size`, or D3D_ERR_STATE (the backward entry points)
static inline int roi_grid_of(d3d_meta *m, const int *size, const char *what, const Grid **out) {
  *out = find_grid(m, size);
  if (!*out) {
    set_error("%s: no grid of spatial size [%d,%d,%d]", what, size[0], size[1], size[2]);
    return D3D_ERR_STATE;
  }
  return D3D_OK;
}
