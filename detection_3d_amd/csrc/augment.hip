// Training-time augmentation of one scene on the device (data3d/suncg_utils/suncg_dataset.py:113-149, elastic() at
// :220-233): the fp64 linear transform of the points folded into the passes of d3d_voxelize (min / max -> flag -> scan ->
// write), the elastic noise fields' separable blur and their trilinear sampling at every point.
//
// Arithmetic contract (the tests' numpy oracle repeats it bit for bit): a_j = ((x M0j + y M1j) + z M2j) in fp64 with
// explicit round-to-nearest products and sums, no contraction; a += offset; the bounds filter and the trunc of
// d3d_voxelize; feats xyz = a / scale.  With M = diag(scale), no offset draw and no feature terms the bits are those of
// d3d_voxelize.
#include "d3d_internal.h"

#include <algorithm>

namespace d3d {

namespace {


// by value: every kernel gets the scene's matrices in its argument block
struct AugArgs {
  double m[9], nrm[9], color[3], u1[3], u2[3];
  int origin_offset, color_col, normal_col;
};

// ((x m0j + y m1j) + z m2j), the order of the oracle
__device__ __forceinline__ double row_times(const double *m, int j, double x, double y, double z) {
  return __dadd_rn(__dadd_rn(__dmul_rn(x, m[j]), __dmul_rn(y, m[3 + j])), __dmul_rn(z, m[6 + j]));
}

// the point's transformed position: supplied fp64 points, or xyz . M of the cloud
__device__ __forceinline__ void point_at(const float *__restrict__ pcl, int nfeat, const double *__restrict__ pts,
                                         const AugArgs &g, int i, double a[3]) {
  if (pts) {
    for (int d = 0; d < 3; d++) a[d] = pts[(size_t)i * 3 + d];
  } else {
    const double x = pcl[(size_t)i * nfeat], y = pcl[(size_t)i * nfeat + 1], z = pcl[(size_t)i * nfeat + 2];
    for (int d = 0; d < 3; d++) a[d] = row_times(g.m, d, x, y, z);
  }
}

// per-axis min and max of the transformed points (red[0..2] min, red[3..5] max, order-preserving uint64): grid-stride,
// wave shuffle, LDS, one atomic per block and value -- order-independent.  pts_out: the fp64 points are written too.
// finite_only: +-Inf is skipped like a NaN (the extent that sizes the elastic noise grid); the voxelizer's minimum keeps
// a -Inf, by d3d_voxelize's contract.
__global__ __launch_bounds__(256) void k_aug_minmax(const float *__restrict__ pcl, int n, int nfeat,
                                                    const double *__restrict__ pts, AugArgs g, double *pts_out,
                                                    int finite_only, unsigned long long *red) {
  __shared__ double lds[4][6];
  double v[6] = {1e300, 1e300, 1e300, -1e300, -1e300, -1e300};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    double a[3];
    point_at(pcl, nfeat, pts, g, i, a);
    if (pts_out)
      for (int d = 0; d < 3; d++) pts_out[(size_t)i * 3 + d] = a[d];
    for (int d = 0; d < 3; d++) {
      if (finite_only && !isfinite(a[d])) continue;
      v[d] = fmin(v[d], a[d]);
      v[3 + d] = fmax(v[3 + d], a[d]);
    }
  }
  for (int d = 0; d < 6; d++) {
    double x = v[d];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x = d < 3 ? fmin(x, __shfl_xor(x, s, 64)) : fmax(x, __shfl_xor(x, s, 64));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6][d] = x;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int d = threadIdx.x;
    double x = lds[0][d];
    for (int w = 1; w < 4; w++) x = d < 3 ? fmin(x, lds[w][d]) : fmax(x, lds[w][d]);
    if (d < 3)
      atomicMin(&red[d], f64_ordered(x));
    else
      atomicMax(&red[d], f64_ordered(x));
  }
}

// offset = -m (+ clip(full - M + m - 0.001, 0, inf) u1 + clip(full - M + m + 0.001, -inf, 0) u2), suncg_dataset.py:127-132
__global__ void k_aug_offset(const unsigned long long *red, AugArgs g, int fx, int fy, int fz, double *off) {
  const int d = threadIdx.x;
  if (d >= 3) return;
  const double full = (double)(d == 0 ? fx : d == 1 ? fy : fz);
  const double lo = ordered_to_f64(red[d]), hi = ordered_to_f64(red[3 + d]);
  double o = -lo;
  if (g.origin_offset) {
    const double q = __dadd_rn(__dsub_rn(full, hi), lo);
    const double up = fmax(__dsub_rn(q, 0.001), 0.0), dn = fmin(__dadd_rn(q, 0.001), 0.0);
    o = __dadd_rn(o, __dadd_rn(__dmul_rn(up, g.u1[d]), __dmul_rn(dn, g.u2[d])));
  }
  off[d] = o;
}

__global__ void k_aug_flag(const float *__restrict__ pcl, int n, int nfeat, const double *__restrict__ pts, AugArgs g,
                           const double *__restrict__ off, int fx, int fy, int fz, int32_t *flag) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int full[3] = {fx, fy, fz};
  double a[3];
  point_at(pcl, nfeat, pts, g, i, a);
  bool ok = true;
  for (int d = 0; d < 3; d++) {
    const double b = __dadd_rn(a[d], off[d]);
    ok = ok && (b >= 0) && (b < (double)full[d]);
  }
  flag[i] = ok ? 1 : 0;
}

__global__ void k_aug_write(const float *__restrict__ pcl, int n, int nfeat, const double *__restrict__ pts, AugArgs g,
                            double scale, const double *__restrict__ off, const int32_t *__restrict__ flag,
                            const int32_t *__restrict__ rank, int64_t *coords, float *feats) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const int o = rank[i];
  const float *p = pcl + (size_t)i * nfeat;
  float *f = feats + (size_t)o * nfeat;
  double a[3];
  point_at(pcl, nfeat, pts, g, i, a);
  for (int d = 0; d < 3; d++) {
    const double b = __dadd_rn(a[d], off[d]);
    coords[(size_t)o * 3 + d] = (int64_t)b;                  // trunc, suncg_dataset.py:173
    f[d] = (float)__ddiv_rn(b, scale);                        // :149
  }
  for (int c = 3; c < nfeat; c++) f[c] = p[c];
  if (g.color_col >= 0)                                       // :140-142, one draw per scene
    for (int k = 0; k < 3; k++) f[g.color_col + k] = (float)__dadd_rn((double)p[g.color_col + k], g.color[k]);
  if (g.normal_col >= 0) {                                    // n . (F Rz), rounded once
    const double x = p[g.normal_col], y = p[g.normal_col + 1], z = p[g.normal_col + 2];
    for (int k = 0; k < 3; k++) f[g.normal_col + k] = (float)row_times(g.nrm, k, x, y, z);
  }
}

// one pass of the 3-tap 1/3 box filter along `axis` of `nf` fields [nf][D0][D1][D2], zero padded: scipy.ndimage's
// correlate -- the taps in footprint order (-1, 0, +1) summed in fp64 from 0 with the fp32 weight, rounded to fp32
__global__ void k_elastic_blur(const float *__restrict__ in, float *__restrict__ out, int nf, int D0, int D1, int D2,
                               int axis) {
  const long total = (long)nf * D0 * D1 * D2;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int k = (int)(t % D2);
  const int j = (int)((t / D2) % D1);
  const int i = (int)((t / ((long)D2 * D1)) % D0);
  const int pos = axis == 0 ? i : axis == 1 ? j : k;
  const int len = axis == 0 ? D0 : axis == 1 ? D1 : D2;
  const long stride = axis == 0 ? (long)D1 * D2 : axis == 1 ? (long)D2 : 1;
  const double w = (double)(1.0f / 3.0f);
  double s = 0.0;
  for (int q = -1; q <= 1; q++) {
    const int r = pos + q;
    const double x = (r >= 0 && r < len) ? (double)in[t + q * stride] : 0.0;
    s = __dadd_rn(s, __dmul_rn(x, w));
  }
  out[t] = (float)s;
}

// RegularGridInterpolator(linear, bounds_error=False, fill_value=0) of the 3 fields on the axes
// linspace(-(b-1) gran, (b-1) gran, b) (spacing 2 gran), then a += disp * mag; red: min / max of the displaced points
// that are finite (the extent sizes the next pass's grid)
__global__ __launch_bounds__(256) void k_elastic_apply(double *pts, int n, const float *__restrict__ fields, int D0,
                                                       int D1, int D2, double gran, double mag,
                                                       unsigned long long *red) {
  __shared__ double lds[4][6];
  double v[6] = {1e300, 1e300, 1e300, -1e300, -1e300, -1e300};
  const int D[3] = {D0, D1, D2};
  const double step = 2.0 * gran;
  const long vol = (long)D0 * D1 * D2;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    double a[3], tt[3];
    int lo[3];
    bool in = true;
    for (int d = 0; d < 3; d++) {
      a[d] = pts[(size_t)i * 3 + d];
      const double g0 = -(double)(D[d] - 1) * gran, g1 = (double)(D[d] - 1) * gran;
      in = in && a[d] >= g0 && a[d] <= g1;
      // searchsorted(grid, x, 'left') - 1, clipped to [0, b-2]: the cell (g_i, g_i+1] holding x
      int c = (int)ceil((a[d] - g0) / step) - 1;
      c = c < 0 ? 0 : (c > D[d] - 2 ? D[d] - 2 : c);
      lo[d] = in ? c : 0;
      const double gl = g0 + (double)lo[d] * step, gh = g0 + (double)(lo[d] + 1) * step;
      tt[d] = (a[d] - gl) / (gh - gl);
    }
    double disp[3] = {0.0, 0.0, 0.0};
    if (in) {
      for (int f = 0; f < 3; f++) {
        const float *F = fields + f * vol;
        double acc = 0.0;
        for (int c = 0; c < 8; c++) {           // itertools.product order: (lo, hi) per axis, axis 2 fastest
          const int b0 = (c >> 2) & 1, b1 = (c >> 1) & 1, b2 = c & 1;
          const double w = ((1.0 * (b0 ? tt[0] : 1.0 - tt[0])) * (b1 ? tt[1] : 1.0 - tt[1])) * (b2 ? tt[2] : 1.0 - tt[2]);
          const long idx = ((long)(lo[0] + b0) * D1 + (lo[1] + b1)) * D2 + (lo[2] + b2);
          acc = __dadd_rn(acc, __dmul_rn((double)F[idx], w));
        }
        disp[f] = acc;
      }
    }
    for (int d = 0; d < 3; d++) {
      const double b = __dadd_rn(a[d], __dmul_rn(disp[d], mag));
      pts[(size_t)i * 3 + d] = b;
      if (!isfinite(b)) continue;             // a NaN or +-Inf row keeps its bits and sizes no grid
      v[d] = fmin(v[d], b);
      v[3 + d] = fmax(v[3 + d], b);
    }
  }
  for (int d = 0; d < 6; d++) {
    double x = v[d];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x = d < 3 ? fmin(x, __shfl_xor(x, s, 64)) : fmax(x, __shfl_xor(x, s, 64));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6][d] = x;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int d = threadIdx.x;
    double x = lds[0][d];
    for (int w = 1; w < 4; w++) x = d < 3 ? fmin(x, lds[w][d]) : fmax(x, lds[w][d]);
    if (d < 3)
      atomicMin(&red[d], f64_ordered(x));
    else
      atomicMax(&red[d], f64_ordered(x));
  }
}

AugArgs to_args(const d3d_augment_params *p) {
  AugArgs g;
  for (int k = 0; k < 9; k++) {
    g.m[k] = p->m[k];
    g.nrm[k] = p->nrm[k];
  }
  for (int k = 0; k < 3; k++) {
    g.color[k] = p->color[k];
    g.u1[k] = p->u1[k];
    g.u2[k] = p->u2[k];
  }
  g.origin_offset = p->origin_offset;
  g.color_col = p->color_col;
  g.normal_col = p->normal_col;
  return g;
}

unsigned reduce_blocks(int n) { return std::max(1u, std::min(1024u, (unsigned)((n + 255) / 256))); }

// the six min / max words -> host doubles
int read_minmax(const unsigned long long *red, double *minmax_host, hipStream_t s) {
  unsigned long long u[6];
  if (int rc = readback_publish(red, 12, s)) return rc;
  if (int rc = readback_wait(u, 12)) return rc;
  for (int d = 0; d < 6; d++) minmax_host[d] = ordered_to_f64(u[d]);
  return D3D_OK;
}

}  // namespace
}  // namespace d3d

using namespace d3d;

size_t d3d_augment_scratch_bytes(int n) { return d3d_voxelize_scratch_bytes(n) + 1024; }

int d3d_augment_transform(const float *pcl, int n, int nfeat, const d3d_augment_params *prm_host, double *points_out,
                          double *minmax_host, void *scratch, size_t scratch_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(pcl && prm_host && points_out && minmax_host && scratch && nfeat >= 3 && n > 0,
              "d3d_augment_transform: bad arguments");
  D3D_REQUIRE(scratch_bytes >= 64, "d3d_augment_transform: scratch too small");
  unsigned long long *red = (unsigned long long *)scratch;
  D3D_HIP_CHECK(hipMemsetAsync(red, 0xFF, 3 * 8, s));
  D3D_HIP_CHECK(hipMemsetAsync(red + 3, 0, 3 * 8, s));
  hipLaunchKernelGGL(k_aug_minmax, dim3(reduce_blocks(n)), dim3(256), 0, s, pcl, n, nfeat, (const double *)nullptr,
                     to_args(prm_host), points_out, 1, red);
  D3D_LAUNCH_CHECK();
  return read_minmax(red, minmax_host, s);
}

int d3d_elastic_blur(float *fields, int nfields, const int *dims_host, float *tmp, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(fields && tmp && dims_host && nfields > 0, "d3d_elastic_blur: bad arguments");
  const int D0 = dims_host[0], D1 = dims_host[1], D2 = dims_host[2];
  D3D_REQUIRE(D0 > 0 && D1 > 0 && D2 > 0, "d3d_elastic_blur: empty grid");
  const long total = (long)nfields * D0 * D1 * D2;
  D3D_REQUIRE(total < (1l << 31) * 256, "d3d_elastic_blur: grid too large");
  const dim3 grid((unsigned)((total + 255) / 256));
  // axes 0, 1, 2, 0, 1, 2 (elastic(), suncg_dataset.py:223-228), ping-pong: the 6th pass lands in `fields`
  for (int p = 0; p < 6; p++) {
    const float *in = (p & 1) ? tmp : fields;
    float *out = (p & 1) ? fields : tmp;
    hipLaunchKernelGGL(k_elastic_blur, grid, dim3(256), 0, s, in, out, nfields, D0, D1, D2, p % 3);
  }
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

int d3d_elastic_apply(double *points, int n, const float *fields, const int *dims_host, double gran, double mag,
                      double *minmax_host, void *scratch, size_t scratch_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(points && fields && dims_host && scratch && n > 0 && gran > 0, "d3d_elastic_apply: bad arguments");
  D3D_REQUIRE(dims_host[0] >= 2 && dims_host[1] >= 2 && dims_host[2] >= 2, "d3d_elastic_apply: grid below 2 per axis");
  D3D_REQUIRE(scratch_bytes >= 64, "d3d_elastic_apply: scratch too small");
  unsigned long long *red = (unsigned long long *)scratch;
  D3D_HIP_CHECK(hipMemsetAsync(red, 0xFF, 3 * 8, s));
  D3D_HIP_CHECK(hipMemsetAsync(red + 3, 0, 3 * 8, s));
  hipLaunchKernelGGL(k_elastic_apply, dim3(reduce_blocks(n)), dim3(256), 0, s, points, n, fields, dims_host[0],
                     dims_host[1], dims_host[2], gran, mag, red);
  D3D_LAUNCH_CHECK();
  if (!minmax_host) return D3D_OK;
  return read_minmax(red, minmax_host, s);
}

int d3d_augment_voxelize(const float *pcl, int n, int nfeat, const double *points, const d3d_augment_params *prm_host,
                         double scale, const int *full_scale_host, int64_t *coords_out, float *feats_out,
                         int *n_kept_host, double *offset_host, void *scratch, size_t scratch_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(pcl && prm_host && coords_out && feats_out && n_kept_host && offset_host && full_scale_host &&
                  nfeat >= 3 && n >= 0,
              "d3d_augment_voxelize: bad arguments");
  D3D_REQUIRE(prm_host->color_col < 0 || (prm_host->color_col >= 3 && prm_host->color_col + 3 <= nfeat),
              "d3d_augment_voxelize: colour columns outside the features");
  D3D_REQUIRE(prm_host->normal_col < 0 || (prm_host->normal_col >= 3 && prm_host->normal_col + 3 <= nfeat),
              "d3d_augment_voxelize: normal columns outside the features");
  D3D_REQUIRE(scratch_bytes >= d3d_augment_scratch_bytes(n), "d3d_augment_voxelize: scratch too small");
  *n_kept_host = 0;
  for (int d = 0; d < 3; d++) offset_host[d] = 0.0;
  if (n == 0) return D3D_OK;
  const AugArgs g = to_args(prm_host);
  const int fx = full_scale_host[0], fy = full_scale_host[1], fz = full_scale_host[2];
  Arena A = scratch_arena(scratch, scratch_bytes);
  D3D_ALLOC(red, unsigned long long, A, 16);       // min[3], max[3], offset[3] (fp64), kept count (int32)
  D3D_ALLOC(flag, int32_t, A, n);
  D3D_ALLOC(rank, int32_t, A, n);
  double *off = (double *)(red + 6);
  int32_t *total = (int32_t *)(red + 9);
  D3D_HIP_CHECK(hipMemsetAsync(red, 0xFF, 3 * 8, s));
  D3D_HIP_CHECK(hipMemsetAsync(red + 3, 0, 3 * 8, s));
  hipLaunchKernelGGL(k_aug_minmax, dim3(reduce_blocks(n)), dim3(256), 0, s, pcl, n, nfeat, points, g, (double *)nullptr,
                     0, red);
  hipLaunchKernelGGL(k_aug_offset, dim3(1), dim3(64), 0, s, (const unsigned long long *)red, g, fx, fy, fz, off);
  hipLaunchKernelGGL(k_aug_flag, grid1d(n), dim3(256), 0, s, pcl, n, nfeat, points, g, (const double *)off, fx, fy, fz,
                     flag);
  D3D_LAUNCH_CHECK();
  int rc = scan_exclusive_i32(flag, rank, n, total, A, s);
  if (rc) return rc;
  // offset and count (adjacent in `red`) are published with an event behind the store; the write pass runs while the
  // host waits
  rc = readback_publish(off, 7, s);
  if (rc) return rc;
  hipLaunchKernelGGL(k_aug_write, grid1d(n), dim3(256), 0, s, pcl, n, nfeat, points, g, scale, (const double *)off,
                     flag, rank, coords_out, feats_out);
  D3D_LAUNCH_CHECK();
  struct {
    double off[3];
    int32_t kept;
  } back;
  rc = readback_wait(&back, 7);
  if (rc) return rc;
  *n_kept_host = back.kept;
  for (int d = 0; d < 3; d++) offset_host[d] = back.off[d];
  return D3D_OK;
}
