// Point-cloud voxelisation (a1) and the read-back of a few device words through the calling thread's pinned word.
#include "grid_internal.h"

namespace d3d {

// a1 -------------------------------------------------------------------------------------
// d3d_voxelize: a = double(x) * scale, then a + (-min) as a second fp64 operation (never one fused multiply-add: the
// truncation must be numpy's), keep 0 <= a < full, trunc.
// Contract on non-finite coordinates: the minimum is an fmin reduction, which ignores a NaN, so a NaN coordinate drops
// that point alone (its comparisons fail), and so does a +Inf one.  numpy's min propagates the NaN, makes the offset
// NaN and drops the whole cloud: the deviation is deliberate.  A -Inf coordinate is the minimum, the shift is +Inf and
// every point goes (Inf - Inf for the point itself), as in numpy.
__global__ __launch_bounds__(256) void k_vox_min(const float *__restrict__ pcl, int n, int nfeat,
                                                 double scale,
                                                 unsigned long long *mins /*3, ordered-uint*/) {
  D3D_SIDE_PRIO();
  // per-axis min of (double)x*scale: grid-stride, wave shuffle, LDS, then ONE atomic per block
  // (doubles mapped to order-preserving uint64)
  __shared__ double red[4][3];
  double v[3] = {1e300, 1e300, 1e300};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    for (int d = 0; d < 3; d++) v[d] = fmin(v[d], (double)pcl[(size_t)i * nfeat + d] * scale);
  for (int d = 0; d < 3; d++) {
    double x = v[d];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x = fmin(x, __shfl_xor(x, s, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][d] = x;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double x = fmin(fmin(red[0][threadIdx.x], red[1][threadIdx.x]), fmin(red[2][threadIdx.x], red[3][threadIdx.x]));
    atomicMin(&mins[threadIdx.x], f64_ordered(x));
  }
}
__global__ void k_vox_flag(const float *__restrict__ pcl, int n, int nfeat, double scale,
                           const unsigned long long *mins, int fx, int fy, int fz, int32_t *flag) {
  D3D_SIDE_PRIO();
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int full[3] = {fx, fy, fz};
  bool ok = true;
  for (int d = 0; d < 3; d++) {
    double a = (double)pcl[(size_t)i * nfeat + d] * scale + (-ordered_to_f64(mins[d]));
    ok = ok && (a >= 0) && (a < (double)full[d]);
  }
  flag[i] = ok ? 1 : 0;
}
__global__ void k_vox_write(const float *__restrict__ pcl, int n, int nfeat, double scale,
                            const unsigned long long *mins, const int32_t *__restrict__ flag,
                            const int32_t *__restrict__ rank, int64_t *coords, float *feats) {
  D3D_SIDE_PRIO();
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flag[i]) return;
  int o = rank[i];
  for (int d = 0; d < 3; d++) {
    double a = (double)pcl[(size_t)i * nfeat + d] * scale + (-ordered_to_f64(mins[d]));
    coords[(size_t)o * 3 + d] = (int64_t)a;                  // trunc, suncg_dataset.py:173
    feats[(size_t)o * nfeat + d] = (float)(a / scale);        // :149
  }
  for (int c = 3; c < nfeat; c++) feats[(size_t)o * nfeat + c] = pcl[(size_t)i * nfeat + c];
}

// The pinned word of the calling host thread on the current device, and the event recorded behind the stores to it.
struct ReadbackWord {
  int32_t *word = nullptr;   // 64 bytes, pinned
  hipEvent_t ev = nullptr;
};
static ReadbackWord *readback_word() {
  static thread_local ReadbackWord words[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) {
    set_error("read-back: no current device");
    return nullptr;
  }
  ReadbackWord &w = words[dev];
  if (!w.word) {
    hipError_t e = hipHostMalloc((void **)&w.word, 64, hipHostMallocPortable);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&w.ev, hipEventDisableTiming);
    if (e != hipSuccess) {
      set_error("read-back: pinned word / event: %s", hipGetErrorString(e));
      w.word = nullptr;
      return nullptr;
    }
  }
  return &w;
}
// one wave: word[t] = src[t] for t < n_words <= 16, every word a system-scope release store (vector memory)
__global__ __launch_bounds__(64) void k_readback_words(const int32_t *__restrict__ src, int n_words,
                                                       int32_t *__restrict__ word) {
  D3D_SIDE_PRIO();
  const int t = threadIdx.x;
  if (t < n_words && t < 16) __hip_atomic_store(word + t, src[t], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
int readback_publish(const void *src_dev, int n_words, hipStream_t s) {
  D3D_REQUIRE(src_dev && n_words >= 1 && n_words <= 16, "read-back: %d words (1..16)", n_words);
  ReadbackWord *w = readback_word();
  if (!w) return D3D_ERR_HIP;
  hipLaunchKernelGGL(k_readback_words, dim3(1), dim3(64), 0, s, (const int32_t *)src_dev, n_words, w->word);
  D3D_LAUNCH_CHECK();
  D3D_HIP_CHECK(hipEventRecord(w->ev, s));
  return D3D_OK;
}
int readback_wait(void *dst_host, int n_words) {
  D3D_REQUIRE(dst_host && n_words >= 1 && n_words <= 16, "read-back: %d words (1..16)", n_words);
  ReadbackWord *w = readback_word();
  if (!w) return D3D_ERR_HIP;
  D3D_HIP_CHECK(hipEventSynchronize(w->ev));
  for (int k = 0; k < n_words; k++) ((int32_t *)dst_host)[k] = ((volatile int32_t *)w->word)[k];
  return D3D_OK;
}
}  // namespace d3d

using namespace d3d;

extern "C" {

size_t d3d_voxelize_scratch_bytes(int n) {
  size_t nb = ((size_t)n + kScanTile - 1) / kScanTile;
  return 256 * 4 + (size_t)n * 8 + nb * 4 + 4096;
}

int d3d_voxelize(const float *pcl, int n, int nfeat, double scale, const int *full, int64_t *coords,
                 float *feats, int *n_kept_host, void *scratch, size_t scratch_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  // (an empty cloud has no rows to point at: torch hands over null pointers for it)
  D3D_REQUIRE(n_kept_host && full && nfeat >= 3 && n >= 0 && (n == 0 || (pcl && coords && feats)),
              "d3d_voxelize: bad arguments");
  D3D_REQUIRE(scratch_bytes >= d3d_voxelize_scratch_bytes(n), "d3d_voxelize: scratch too small");
  *n_kept_host = 0;
  if (n == 0) return D3D_OK;
  Arena A = scratch_arena(scratch, scratch_bytes);
  D3D_ALLOC(mins, unsigned long long, A, 4);
  D3D_ALLOC(flag, int32_t, A, n);
  D3D_ALLOC(rank, int32_t, A, n);
  D3D_HIP_CHECK(hipMemsetAsync(mins, 0xFF, 4 * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(k_vox_min, dim3(std::min(1024u, grid1d(n).x)), dim3(256), 0, s, pcl, n, nfeat, scale, mins);
  hipLaunchKernelGGL(k_vox_flag, grid1d(n), dim3(256), 0, s, pcl, n, nfeat, scale, mins, full[0], full[1], full[2], flag);
  int rc = scan_exclusive_i32(flag, rank, n, (int32_t *)(mins + 3), A, s);
  if (rc) return rc;
  // the count goes to a pinned word by a store of its own launch, with an event behind it: the host waits for that
  // event while k_vox_write runs (a pageable hipMemcpy + stream synchronise took the write's time and a staged copy more)
  rc = readback_publish(mins + 3, 1, s);
  if (rc) return rc;
  hipLaunchKernelGGL(k_vox_write, grid1d(n), dim3(256), 0, s, pcl, n, nfeat, scale, mins, flag, rank, coords, feats);
  D3D_LAUNCH_CHECK();
  return readback_wait(n_kept_host, 1);
}

}  // extern "C"
