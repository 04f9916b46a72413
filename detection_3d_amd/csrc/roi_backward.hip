// a21. RoIAlignRotated3D backward with fp32 atomics, as the reference sums it
// (maskrcnn_benchmark/csrc/cuda/ROIAlignRotated3D_cuda.cu:182-354): the dense form and the sparse form over the hash
// grid, the latter also for bf16 rows.  The fixed-order form is roi_backward_det.hip.
#include "grid_internal.h"

namespace d3d {

#include "roi_geometry.inc"

// Dense backward, _C.roi_align_rotated_3d_backward (ROIAlignRotated3D_cuda.cu:238-354): one thread per
// pooled element, 8 fp32 atomics per sub-sample into the zeroed dense gradient.
__global__ __launch_bounds__(256) void k_roi_dense_bwd(const float *__restrict__ top_diff, int C, int H, int W,
                                                       int Z, const float *__restrict__ rois, long nthreads,
                                                       float spatial_scale, int PH, int PW, int PZ,
                                                       int sampling_ratio, float *__restrict__ bottom_diff) {
  long index = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (index >= nthreads) return;
  const int pz = index % PZ;
  const int pw = (index / PZ) % PW;
  const int ph = (index / PZ / PW) % PH;
  const int c = (index / PZ / PW / PH) % C;
  const int n = index / PZ / PW / PH / C;
  const RoiGeom g = roi_geom(rois + (size_t)n * 8, spatial_scale, PH, PW, PZ, sampling_ratio);
  float *d = bottom_diff + ((size_t)g.b * C + c) * H * W * Z;
  const float count = (float)(g.gh * g.gw * g.gz);
  const float top = top_diff[index];
  for (int iy = 0; iy < g.gh; iy++)
    for (int ix = 0; ix < g.gw; ix++)
      for (int iz = 0; iz < g.gz; iz++) {
        float y, x, z;
        sample_pos(g, ph, pw, pz, iy, ix, iz, y, x, z);
        Tri t;
        if (z > Z || !tri_setup(y, x, z, H, W, Z, t)) continue;   // backward bound test (:190)
        const float w[8] = {t.hy * t.hx * t.hz, t.hy * t.lx * t.hz, t.ly * t.hx * t.hz, t.ly * t.lx * t.hz,
                            t.hy * t.hx * t.lz, t.hy * t.lx * t.lz, t.ly * t.hx * t.lz, t.ly * t.lx * t.lz};
#pragma unroll
        for (int q = 0; q < 8; q++) {
          const int yy = (q >> 1) & 1 ? t.yh : t.yl, xx = q & 1 ? t.xh : t.xl, zz = q >> 2 ? t.zh : t.zl;
          atomicAdd(d + ((size_t)yy * W + xx) * Z + zz, top * w[q] / count);
        }
      }
}

// Backward of the sparse variant: the dense gradient of RoIAlignRotated3DBackwardFeature (:238-354)
// restricted to the active sites (what SparseToDense_updateGradInput would gather back).  Keeps the
// backward's own bound test `z > zsize` (:190).  fp32 atomics, like the reference.  TT = storage type of top_diff
// (float, or bf16 bits widened as they are read); d_feats is fp32 either way.
static constexpr int kRoiBwdCch = 64;
template <typename TT>
__global__ __launch_bounds__(256) void k_roi_sparse_bwd(
    const HashEntry *__restrict__ tab, int cap, int C, int H, int W, int Z, const float *__restrict__ rois,
    float spatial_scale, int PH, int PW, int PZ, int sampling_ratio, const TT *__restrict__ top_diff,
    float *__restrict__ d_feats) {
  extern __shared__ float tile[];  // [kRoiBwdCch][NB + 1]
  const int n = blockIdx.x, cc = blockIdx.y;
  const int NB = PH * PW * PZ, LD = NB + 1;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nch = min(kRoiBwdCch, C - cc * kRoiBwdCch);
  const TT *g0 = top_diff + ((size_t)n * C + (size_t)cc * kRoiBwdCch) * NB;
  for (int idx = threadIdx.x; idx < nch * NB; idx += 256) tile[(idx / NB) * LD + idx % NB] = ld1(g0 + idx);
  __syncthreads();
  const RoiGeom g = roi_geom(rois + (size_t)n * 8, spatial_scale, PH, PW, PZ, sampling_ratio);
  const int NS = g.gh * g.gw * g.gz;
  const float count = (float)NS;
  const int c = cc * kRoiBwdCch + lane;
  const bool cok = c < C;
  for (int bin = wave; bin < NB; bin += 4) {
    const int pz = bin % PZ, pw = (bin / PZ) % PW, ph = bin / (PZ * PW);
    const float top = cok ? tile[lane * LD + bin] : 0.f;
    for (int s0 = 0; s0 < NS; s0 += 8) {
      const int s = s0 + (lane >> 3), corner = lane & 7;
      int row = -1;
      float wgt = 0.f;
      if (s < NS) {
        const int iz = s % g.gz, ix = (s / g.gz) % g.gw, iy = s / (g.gz * g.gw);
        float y, x, z;
        sample_pos(g, ph, pw, pz, iy, ix, iz, y, x, z);
        Tri t;
        if (!(z > Z) && tri_setup(y, x, z, H, W, Z, t)) {
          const int zb = corner >> 2, yb = (corner >> 1) & 1, xb = corner & 1;
          wgt = (yb ? t.ly : t.hy) * (xb ? t.lx : t.hx) * (zb ? t.lz : t.hz);
          row = hash_find(tab, cap, pack_key(g.b, yb ? t.yh : t.yl, xb ? t.xh : t.xl, zb ? t.zh : t.zl));
        }
      }
      // the 64 taps of a step fall into a handful of cells: one atomic per (cell, channel) with the taps' weights summed
      // by a wave butterfly (as the forward does) instead of one per tap -- 5x fewer atomics on the hot rows
      unsigned long long m = __ballot(row >= 0);
      while (m) {
        const int rr = __shfl(row, __builtin_ctzll(m), 64);   // wave-uniform cell
        const bool mine = row == rr;
        float ww = mine ? wgt : 0.f;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) ww += __shfl_xor(ww, d, 64);
        if (cok) atomicAdd(d_feats + (size_t)rr * C + c, top * ww / count);
        m &= ~__ballot(mine);
      }
    }
  }
}

// fp32 -> bf16 (round to nearest even), n elements; in 16-byte and out 8-byte aligned (checked by the caller)
__global__ __launch_bounds__(256) void k_roi_f32_to_bf16(const float *__restrict__ in, long n,
                                                         unsigned short *__restrict__ out) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i + 4 <= n)
    store4(out + i, load4<float>(in + i));
  else
    for (long j = i; j < n; j++) st1(out + j, in[j]);
}

}  // namespace d3d

using namespace d3d;

extern "C" {

int d3d_roi_align_rotated_3d_backward(const float *top_diff, int B, int C, int H, int W, int Z,
                                      const float *rois, int K, float spatial_scale, int ph, int pw, int pz,
                                      int sampling_ratio, float *bottom_diff, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && Z > 0 && K >= 0 && ph > 0 && pw > 0 && pz > 0 && bottom_diff,
              "roi_align_backward: bad arguments");
  D3D_HIP_CHECK(hipMemsetAsync(bottom_diff, 0, sizeof(float) * (size_t)B * C * H * W * Z, s));
  if (K == 0) return D3D_OK;
  D3D_REQUIRE(top_diff && rois, "roi_align_backward: null pointer");
  long nthreads = (long)K * C * ph * pw * pz;
  hipLaunchKernelGGL(k_roi_dense_bwd, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, s, top_diff, C, H, W, Z,
                     rois, nthreads, spatial_scale, ph, pw, pz, sampling_ratio, bottom_diff);
  D3D_LAUNCH_CHECK();
  roi_record(kRoiFamDenseBwd, 4, 0, 0, dim3((unsigned)((nthreads + 255) / 256)), 256, 0);
  return D3D_OK;
}

// d_feats [n_active, C] is accumulated into (zero it first)
int d3d_roi_align_rotated_3d_sparse_backward(d3d_meta *m, const int *size, const float *top_diff, int C,
                                             const int *crop, const float *rois, int K, float spatial_scale,
                                             int ph, int pw, int pz, int sampling_ratio, float *d_feats,
                                             void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && size && crop && C > 0 && K >= 0 && ph > 0 && pw > 0 && pz > 0, "roi_align_sparse_backward: bad arguments");
  const Grid *gp;
  if (int rc = roi_grid_of(m, size, "roi_align_sparse_backward", &gp)) return rc;
  if (K == 0) return D3D_OK;
  D3D_REQUIRE(top_diff && rois && d_feats, "roi_align_sparse_backward: null pointer");
  const Grid &g = *gp;
  const int NB = ph * pw * pz;
  size_t lds = (size_t)kRoiBwdCch * (NB + 1) * sizeof(float);
  D3D_REQUIRE(lds <= 64 * 1024, "roi_align_sparse_backward: pooled volume %d too large", NB);
  hipLaunchKernelGGL(k_roi_sparse_bwd<float>, dim3(K, (C + kRoiBwdCch - 1) / kRoiBwdCch), dim3(256), lds, s, g.tab, g.cap,
                     C, crop[0], crop[1], crop[2], rois, spatial_scale, ph, pw, pz, sampling_ratio, top_diff, d_feats);
  D3D_LAUNCH_CHECK();
  roi_record(kRoiFamSparseBwd, 4, 1, 1, dim3(K, (C + kRoiBwdCch - 1) / kRoiBwdCch), 256, 1);
  return D3D_OK;
}

size_t d3d_roi_align_rotated_3d_sparse_backward_bf16_scratch_bytes(int C, int n_rows) {
  if (C <= 0 || n_rows < 0) return 0;
  return (size_t)n_rows * C * sizeof(float) + 256;   // + alignment of the caller's base
}

int d3d_roi_align_rotated_3d_sparse_backward_bf16(d3d_meta *m, const int *size, const void *top_diff, int C,
                                                  const int *crop, const float *rois, int K, float spatial_scale, int ph,
                                                  int pw, int pz, int sampling_ratio, void *d_feats, int n_rows,
                                                  void *scratch, size_t scratch_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && size && crop && C > 0 && K >= 0 && ph > 0 && pw > 0 && pz > 0 && n_rows >= 0,
              "roi_align_sparse_backward_bf16: bad arguments");
  const int NB = ph * pw * pz;
  const size_t lds = (size_t)kRoiBwdCch * (NB + 1) * sizeof(float);
  D3D_REQUIRE(lds <= 64 * 1024, "roi_align_sparse_backward_bf16: pooled volume %d too large", NB);
  const size_t need = d3d_roi_align_rotated_3d_sparse_backward_bf16_scratch_bytes(C, n_rows);
  D3D_REQUIRE(scratch_bytes >= need, "roi_align_sparse_backward_bf16: scratch %zu < %zu bytes", scratch_bytes, need);
  const Grid *gp;
  if (int rc = roi_grid_of(m, size, "roi_align_sparse_backward_bf16", &gp)) return rc;
  D3D_REQUIRE(n_rows == gp->n, "roi_align_sparse_backward_bf16: n_rows %d != %d active sites", n_rows, gp->n);
  if (n_rows == 0) return D3D_OK;
  D3D_REQUIRE(d_feats && scratch && (K == 0 || (top_diff && rois)), "roi_align_sparse_backward_bf16: null pointer");
  D3D_REQUIRE(((uintptr_t)d_feats & 7) == 0, "roi_align_sparse_backward_bf16: d_feats not 8-byte aligned");
  float *acc = (float *)(((uintptr_t)scratch + 255) & ~(uintptr_t)255);
  const long total = (long)n_rows * C;
  D3D_HIP_CHECK(hipMemsetAsync(acc, 0, sizeof(float) * (size_t)total, s));
  if (K > 0) {
    const Grid &g = *gp;
    hipLaunchKernelGGL(k_roi_sparse_bwd<unsigned short>, dim3(K, (C + kRoiBwdCch - 1) / kRoiBwdCch), dim3(256), lds, s,
                       g.tab, g.cap, C, crop[0], crop[1], crop[2], rois, spatial_scale, ph, pw, pz, sampling_ratio,
                       (const unsigned short *)top_diff, acc);
  }
  hipLaunchKernelGGL(k_roi_f32_to_bf16, dim3((unsigned)((total + 1023) / 1024)), dim3(256), 0, s, acc, total,
                     (unsigned short *)d_feats);
  D3D_LAUNCH_CHECK();
  roi_record(kRoiFamSparseBwd, 2, 1, 1, K > 0 ? dim3(K, (C + kRoiBwdCch - 1) / kRoiBwdCch) : dim3(0, 0, 0), 256, 1,
             (total + 1023) / 1024);
  return D3D_OK;
}

}  // extern "C"
