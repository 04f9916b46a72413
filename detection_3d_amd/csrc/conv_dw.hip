// a7. Backward of the sparse convolutions (training rows): dInput / dWeight.  Reference: SCN/CUDA/Convolution.cu:249-442
// (fused dI + dW with atomicAdd on dW).  The other backward ops sit with their forward halves: BatchNorm in
// bn_backward.hip (beside bn.hip), the input layer in grid.hip, RoIAlign in roi_backward.hip / roi_backward_det.hip.
//
// dInput needs no new kernel: it is the forward gather-GEMM on the transposed rulebook with W^T
//   submanifold: nbr[i][k] = j  <=>  nbr[j][K-1-k] = i  -> same plan, offsets flipped;
//   strided conv: the deconvolution plan;  deconvolution: the convolution plan.
// dWeight[k] = sum over rules of offset k of in[r_in]^T (x) dOut[r_out]: MFMA with the rule index
// as the contraction dimension, partial tiles added with fp32 atomics (as the reference does).
#include <algorithm>

#include "d3d_internal.h"

namespace d3d {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// packed_t[k'][g][ci][j] = w[k][ci][4g+j]  (a conv weight with Cin' = cout, Cout' = cin), k' = flip ? K-1-k : k
__global__ void k_pack_weight_t(const float *__restrict__ w, int fv, int cin, int cout, int cp, int flip,
                                float *__restrict__ packed) {
  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)fv * cp * cin;
  if (t >= total) return;
  int j = (int)(t & 3);
  long u = t >> 2;
  int ci = (int)(u % cin);
  u /= cin;
  int g = (int)(u % (cp / 4));
  int kp = (int)(u / (cp / 4));
  int k = flip ? fv - 1 - kp : kp;
  int co = 4 * g + j;
  packed[t] = co < cout ? w[((size_t)k * cin + ci) * cout + co] : 0.f;
}

void launch_pack_weight_t(const float *w, int fv, int cin, int cout, int cp, int flip, float *packed, hipStream_t s) {
  hipLaunchKernelGGL(k_pack_weight_t, grid1d((long)fv * cp * cin), dim3(256), 0, s, w, fv, cin, cout, cp, flip, packed);
}

static constexpr int kDwBlocksPerWg = 64;
static constexpr int kDwTargetWgs = 1024;
static constexpr int kDwMaxChunk = 8;

// One workgroup: offset k = blockIdx.y, a run of kDwBlocksPerWg row blocks, a group of <= 16 output tiles (32x32).
// The blocks of the run that have offset k are found with one ballot; their operands (32 gathered input rows and
// the 32 dOut rows) go through registers one block ahead and their row indices two blocks ahead, all loads
// branch-free (an absent row reads row 0 and is zeroed on the way to LDS), so the gathers of the next block fly
// under the MFMAs of the current one -- the same pipeline as the forward kernel.
// DET (d3d_conv_dw_deterministic): no atomics.  Workgroup blockIdx.x walks the runs blockIdx.x, + gridDim.x, ... in order
// (all of a run's active blocks, no chunks), keeps the sum in its accumulators and STORES it as partial `blockIdx.x` of
// dW (zeros when it met no rule); k_dw_reduce adds the partials to dW in a fixed order.
template <int CP, int COUT, bool DET>
__global__ __launch_bounds__(256) void k_conv_dw(const float *__restrict__ in, int cin,
                                                 const float *__restrict__ d_out,
                                                 const int32_t *__restrict__ nbrT, int npos,
                                                 const int32_t *__restrict__ rows,
                                                 const uint32_t *__restrict__ blkmask, int n_blk, int run,
                                                 int chunk, int nz_tiles, float *__restrict__ dW) {
  constexpr int NTI = CP / 32, NTJ = COUT / 32, T = NTI * NTJ;
  constexpr int TPG = T < 16 ? T : 16;             // tiles per group (grid.z)
  constexpr int TPW = (TPG + 3) / 4;               // tiles per wave
  constexpr int A4 = CP / 4, B4 = COUT / 4;        // float4 per row
  constexpr int NA = (32 * A4 + 255) / 256, NB = (32 * B4 + 255) / 256;  // float4 per thread and block
  static_assert(kDwBlocksPerWg == 64, "one ballot covers the longest run");
  __shared__ __attribute__((aligned(16))) float As[32 * CP];
  __shared__ __attribute__((aligned(16))) float Bs[32 * COUT];
  const int k = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = lane & 31, kk = lane >> 5;
  int b0 = blockIdx.x * run;
  const int n_runs = (n_blk + run - 1) / run;
  int rx = blockIdx.x;            // the run being walked (DET: then rx + gridDim.x, ...)
  // blocks of a run (<= 64) that have a rule at offset k
  auto run_mask = [&](int first) -> unsigned long long {
    const uint32_t mm = (lane < run && first + lane < n_blk) ? blkmask[first + lane] : 0u;
    return __ballot((mm >> k) & 1u);
  };
  unsigned long long active = run_mask(b0);
  // The run's active blocks are dealt out in chunks of `chunk` to the workgroups blockIdx.z / nz_tiles = 0, 1, ...:
  // a dense offset (the centre one is present in every block) no longer makes one workgroup walk the whole run
  // while the workgroups of the sparse offsets have long finished.
  if constexpr (!DET) {
    const int c = blockIdx.z / nz_tiles;
    for (int d = 0; d < c * chunk && active; d++) active &= active - 1;
    unsigned long long keep = 0, rest = active;
    for (int d = 0; d < chunk && rest; d++) {
      keep |= rest & (~rest + 1);
      rest &= rest - 1;
    }
    active = keep;
  }
  if constexpr (!DET) {
    if (!active) return;
  }
  const int zt = blockIdx.z % nz_tiles;   // tile group
  f32x16 acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; t++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[t][r] = 0.f;
  const bool vec = (cin == CP);

  int ia[NA], ib[NB];           // row indices of the block whose operands are requested next
  f32x4 sa[NA], sb[NB];         // operands in flight
  uint32_t real_a = 0, real_b = 0;
  auto load_idx = [&](int b) {
#pragma unroll
    for (int j = 0; j < NA; j++) {
      const int e = threadIdx.x + j * 256;
      ia[j] = nbrT[(size_t)k * npos + b * 32 + (e < 32 * A4 ? e / A4 : 0)];
    }
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const int e = threadIdx.x + j * 256;
      ib[j] = rows[b * 32 + (e < 32 * B4 ? e / B4 : 0)];
    }
  };
  auto issue_data = [&]() {
    real_a = real_b = 0;
#pragma unroll
    for (int j = 0; j < NA; j++) {
      const int e = threadIdx.x + j * 256;
      const int c4 = e % A4;
      const int s = e < 32 * A4 ? ia[j] : -1;
      if (s >= 0) real_a |= 1u << j;
      const float *p = in + (size_t)(s < 0 ? 0 : s) * cin + c4 * 4;
      if (vec) {
        sa[j] = *(const f32x4 *)p;
      } else {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (c4 * 4 + 0 < cin) v[0] = p[0];
        if (c4 * 4 + 1 < cin) v[1] = p[1];
        if (c4 * 4 + 2 < cin) v[2] = p[2];
        if (c4 * 4 + 3 < cin) v[3] = p[3];
        sa[j] = v;
      }
    }
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const int e = threadIdx.x + j * 256;
      const int c4 = e % B4;
      const int o = e < 32 * B4 ? ib[j] : -1;
      if (o >= 0) real_b |= 1u << j;
      sb[j] = *(const f32x4 *)(d_out + (size_t)(o < 0 ? 0 : o) * COUT + c4 * 4);
    }
  };
  auto commit = [&]() {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NA; j++) {
      const int e = threadIdx.x + j * 256;
      if (e < 32 * A4) *(f32x4 *)(As + (e / A4) * CP + (e % A4) * 4) = ((real_a >> j) & 1u) ? sa[j] : zero;
    }
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const int e = threadIdx.x + j * 256;
      if (e < 32 * B4) *(f32x4 *)(Bs + (e / B4) * COUT + (e % B4) * 4) = ((real_b >> j) & 1u) ? sb[j] : zero;
    }
  };
  auto pop = [&]() -> int {  // next active block of the run (DET: of this workgroup's runs), or -1
    if constexpr (DET) {
      while (!active) {        // (uniform over the workgroup: every wave walks the same runs)
        rx += gridDim.x;
        if (rx >= n_runs) return -1;
        b0 = rx * run;
        active = run_mask(b0);
      }
    } else {
      if (!active) return -1;
    }
    const int j = __builtin_ctzll(active);
    active &= active - 1;
    return b0 + j;
  };

  int bc = pop();               // block being computed
  if (bc >= 0) {
    load_idx(bc);
    issue_data();
  }
  int bn = pop();               // block whose operands are requested during bc's MFMAs
  if (bn >= 0) load_idx(bn);
  while (bc >= 0) {
    commit();
    __syncthreads();
    const int bnn = bn >= 0 ? pop() : -1;
    if (bn >= 0) {
      issue_data();               // operands of bn (its indices arrived during the previous block)
      if (bnn >= 0) load_idx(bnn);
    }
#pragma unroll
    for (int t = 0; t < TPW; t++) {
      const int tile = zt * TPG + wave * TPW + t;
      if (wave * TPW + t >= TPG || tile >= T) continue;
      const int ti = tile / NTJ, tj = tile % NTJ;
#pragma unroll
      for (int s = 0; s < 16; s++) {
        const float a = As[(2 * s + kk) * CP + ti * 32 + i];
        const float bb = Bs[(2 * s + kk) * COUT + tj * 32 + i];
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, acc[t], 0, 0, 0);
      }
    }
    __syncthreads();
    bc = bn;
    bn = bnn;
  }
#pragma unroll
  for (int t = 0; t < TPW; t++) {
    const int tile = zt * TPG + wave * TPW + t;
    if (wave * TPW + t >= TPG || tile >= T) continue;
    const int ti = tile / NTJ, tj = tile % NTJ;
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
      const int ci = ti * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * kk;
      const int co = tj * 32 + i;
      if constexpr (DET) {
        if (ci < cin) dW[(((size_t)blockIdx.x * gridDim.y + k) * cin + ci) * COUT + co] = acc[t][reg];
      } else {
        if (ci < cin) atomicAdd(dW + ((size_t)k * cin + ci) * COUT + co, acc[t][reg]);
      }
    }
  }
}

// dW[e] += partial[0][e] + partial[1][e] + ...  (in that order)
__global__ __launch_bounds__(256) void k_dw_reduce(const float *__restrict__ part, int n_part, size_t n, float *__restrict__ dW) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  float v = 0.f;
  for (int g = 0; g < n_part; g++) v += part[(size_t)g * n + e];
  dW[e] += v;
}

// ---- bf16 storage: dW[k] += in[rows_k]^T . dOut[rows_k] on v_mfma_f32_32x32x16_bf16 (fp32 accumulators, fp32 dW) ----
// The decomposition of k_conv_dw (offset per blockIdx.y, ballot-found runs of 32-row blocks, chunks of dense offsets,
// the DET form's partials), with half the bytes per row and K = 16 rows per MFMA instead of 2.  Both operands sum over
// the row index, so both tiles are staged row-major in LDS as gathered (16-byte pieces) and read column-wise with
// ds_read_b64_tr_b16.
typedef unsigned short bf16_t;   // bf16 storage at the ABI (raw bits)
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// LDS row stride (elements) of a staged [32][w] tile: >= w and = 32 (mod 64), so that the 32 lanes of a half-wave's
// transposed read (4 rows x 32 columns, 8 bytes a lane) fall on 64 different banks
constexpr int dw_lds_ld(int w) { return w + (32 - w % 64 + 64) % 64; }

// The 32x32x16 operand fragment of columns col0 .. col0+31 over rows row0 .. row0+15 of a row-major LDS tile: lane l
// gets column col0 + (l & 31), rows row0 + 8 (l >> 5) + j in element j -- A[i][k] (or B[k][j]) with the row as k.
// Two ds_read_b64_tr_b16 (rows +0..3, +4..7): lane 4q + p of a 16-lane group gives the address of row q, columns
// 4p .. 4p+3 of the group's 4 x 16 block, and lane i receives column i with row q in element q.  The instruction
// gathers across lanes: EXEC must be full (callers branch on wave-uniform conditions only).
__device__ __forceinline__ bf16x8 dw_frag(const bf16_t *tile, int ld, int row0, int col0, int lane) {
  const int i = lane & 15;
  const bf16_t *a = tile + (row0 + 8 * (lane >> 5) + (i >> 2)) * ld + col0 + 16 * ((lane >> 4) & 1) + 4 * (i & 3);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)a);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(a + 4 * ld));
  const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

// CS = stored Cin (16 .. 256), `cin` = Cin of dW (<= CS: the first layer stores 9 channels as 16); dW rows ci >= cin are
// not written.  DET as k_conv_dw.
template <int CS, int COUT, bool DET>
__global__ __launch_bounds__(256) void k_conv_dw_bf16(const bf16_t *__restrict__ in, int cin,
                                                      const bf16_t *__restrict__ d_out,
                                                      const int32_t *__restrict__ nbrT, int npos,
                                                      const int32_t *__restrict__ rows,
                                                      const uint32_t *__restrict__ blkmask, int n_blk, int run,
                                                      int chunk, int nz_tiles, float *__restrict__ dW) {
  constexpr int CP = CS < 32 ? 32 : CS;            // Cin covered by output tiles
  constexpr int NTI = CP / 32, NTJ = COUT / 32, T = NTI * NTJ;
  constexpr int TPG = T < 16 ? T : 16;             // tiles per group (grid.z)
  constexpr int TPW = (TPG + 3) / 4;               // tiles per wave
  constexpr int A8 = CS / 8, B8 = COUT / 8;        // 16-byte pieces per row
  constexpr int NA = (32 * A8 + 255) / 256, NB = (32 * B8 + 255) / 256;  // pieces per thread and block
  constexpr int LDA = dw_lds_ld(CP), LDB = dw_lds_ld(COUT);
  static_assert(kDwBlocksPerWg == 64, "one ballot covers the longest run");
  __shared__ __attribute__((aligned(16))) bf16_t As[32 * LDA];
  __shared__ __attribute__((aligned(16))) bf16_t Bs[32 * LDB];
  const int k = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = lane & 31, kk = lane >> 5;
  int b0 = blockIdx.x * run;
  const int n_runs = (n_blk + run - 1) / run;
  int rx = blockIdx.x;
  auto run_mask = [&](int first) -> unsigned long long {
    const uint32_t mm = (lane < run && first + lane < n_blk) ? blkmask[first + lane] : 0u;
    return __ballot((mm >> k) & 1u);
  };
  unsigned long long active = run_mask(b0);
  if constexpr (!DET) {
    const int c = blockIdx.z / nz_tiles;
    for (int d = 0; d < c * chunk && active; d++) active &= active - 1;
    unsigned long long keep = 0, rest = active;
    for (int d = 0; d < chunk && rest; d++) {
      keep |= rest & (~rest + 1);
      rest &= rest - 1;
    }
    active = keep;
    if (!active) return;
  }
  const int zt = blockIdx.z % nz_tiles;
  f32x16 acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; t++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[t][r] = 0.f;
  if constexpr (CS < CP) {   // channels CS .. CP-1 of the A tile are never staged: zeros
    for (int e = threadIdx.x; e < 32 * (CP - CS); e += 256) As[(e / (CP - CS)) * LDA + CS + e % (CP - CS)] = 0;
  }

  int ia[NA], ib[NB];
  u32x4 sa[NA], sb[NB];
  uint32_t real_a = 0, real_b = 0;
  auto load_idx = [&](int b) {
#pragma unroll
    for (int j = 0; j < NA; j++) {
      const int e = threadIdx.x + j * 256;
      ia[j] = nbrT[(size_t)k * npos + b * 32 + (e < 32 * A8 ? e / A8 : 0)];
    }
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const int e = threadIdx.x + j * 256;
      ib[j] = rows[b * 32 + (e < 32 * B8 ? e / B8 : 0)];
    }
  };
  auto issue_data = [&]() {   // branch-free: an absent row reads row 0 and is zeroed in commit()
    real_a = real_b = 0;
#pragma unroll
    for (int j = 0; j < NA; j++) {
      const int e = threadIdx.x + j * 256;
      const int sidx = e < 32 * A8 ? ia[j] : -1;
      if (sidx >= 0) real_a |= 1u << j;
      sa[j] = *(const u32x4 *)(in + (size_t)(sidx < 0 ? 0 : sidx) * CS + (e % A8) * 8);
    }
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const int e = threadIdx.x + j * 256;
      const int o = e < 32 * B8 ? ib[j] : -1;
      if (o >= 0) real_b |= 1u << j;
      sb[j] = *(const u32x4 *)(d_out + (size_t)(o < 0 ? 0 : o) * COUT + (e % B8) * 8);
    }
  };
  auto commit = [&]() {
    const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < NA; j++) {
      const int e = threadIdx.x + j * 256;
      if (e < 32 * A8) *(u32x4 *)(As + (e / A8) * LDA + (e % A8) * 8) = ((real_a >> j) & 1u) ? sa[j] : zero;
    }
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const int e = threadIdx.x + j * 256;
      if (e < 32 * B8) *(u32x4 *)(Bs + (e / B8) * LDB + (e % B8) * 8) = ((real_b >> j) & 1u) ? sb[j] : zero;
    }
  };
  auto pop = [&]() -> int {
    if constexpr (DET) {
      while (!active) {
        rx += gridDim.x;
        if (rx >= n_runs) return -1;
        b0 = rx * run;
        active = run_mask(b0);
      }
    } else {
      if (!active) return -1;
    }
    const int j = __builtin_ctzll(active);
    active &= active - 1;
    return b0 + j;
  };

  int bc = pop();
  if (bc >= 0) {
    load_idx(bc);
    issue_data();
  }
  int bn = pop();
  if (bn >= 0) load_idx(bn);
  while (bc >= 0) {
    commit();
    __syncthreads();
    const int bnn = bn >= 0 ? pop() : -1;
    if (bn >= 0) {
      issue_data();
      if (bnn >= 0) load_idx(bnn);
    }
#pragma unroll
    for (int t = 0; t < TPW; t++) {
      const int tile = zt * TPG + wave * TPW + t;
      if (wave * TPW + t >= TPG || tile >= T) continue;   // wave-uniform: EXEC stays full for the transposed reads
      const int ti = tile / NTJ, tj = tile % NTJ;
#pragma unroll
      for (int s = 0; s < 2; s++) {
        const bf16x8 a = dw_frag(As, LDA, 16 * s, ti * 32, lane);
        const bf16x8 b = dw_frag(Bs, LDB, 16 * s, tj * 32, lane);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[t], 0, 0, 0);
      }
    }
    __syncthreads();
    bc = bn;
    bn = bnn;
  }
#pragma unroll
  for (int t = 0; t < TPW; t++) {
    const int tile = zt * TPG + wave * TPW + t;
    if (wave * TPW + t >= TPG || tile >= T) continue;
    const int ti = tile / NTJ, tj = tile % NTJ;
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
      const int ci = ti * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * kk;
      const int co = tj * 32 + i;
      if constexpr (DET) {
        if (ci < cin) dW[(((size_t)blockIdx.x * gridDim.y + k) * cin + ci) * COUT + co] = acc[t][reg];
      } else {
        if (ci < cin) atomicAdd(dW + ((size_t)k * cin + ci) * COUT + co, acc[t][reg]);
      }
    }
  }
}

static bool g_dw_deterministic = [] {
  const char *e = getenv("D3D_DW_DETERMINISTIC");
  return e && e[0] != '0';
}();
// d3d_conv_dw_thread_mode: the fixed order for the calling thread only, partials in the caller's buffer
struct DwThreadMode {
  bool on = false;
  void *scratch = nullptr;
  size_t bytes = 0;
};
static thread_local DwThreadMode t_dw;
static constexpr int kDwDetPartials = 32;   // at most this many workgroups (and partial sums) per offset and tile group
static constexpr size_t kDwDetBudget = 64u << 20;   // bytes of partials: fewer partials where G x [K, cin, COUT] exceeds it
// partial sums of the fixed-order dW: a function of the plan's run count and the layer's size only
static inline int dw_det_partials(int n_runs, size_t n) {
  const size_t by_budget = std::max<size_t>(1, kDwDetBudget / (n * sizeof(float)));
  return (int)std::min<size_t>((size_t)std::min(n_runs, kDwDetPartials), by_budget);
}

// the dW kernels of both storage types (S = float: k_conv_dw, bf16: k_conv_dw_bf16), atomic and fixed-order form
template <typename S>
using DwKernel = void (*)(const S *, int, const S *, const int32_t *, int, const int32_t *, const uint32_t *, int, int, int,
                          int, float *);

// d3d_conv_dw_last_form: family (1 fp32, 2 bf16), CP / CS, COUT, cin, T, nz, run, chunk, n_chunks, grid x / y / z, DET,
// G, scratch (0 none, 1 caller buffer, 2 feature lane, 3 stream-ordered allocation), n_blk, K
static constexpr int kDwFormFields = 17;
static thread_local int t_dw_last_form[kDwFormFields] = {};
enum DwScratch { kDwScratchNone = 0, kDwScratchCaller = 1, kDwScratchLane = 2, kDwScratchAsync = 3 };

// grid, run length and scratch of one dW launch; T = output tiles (32 x 32) of the layer, `cin` = Cin of dW, `cw` = the
// kernel's channel class (CP of k_conv_dw, CS of k_conv_dw_bf16)
template <typename S>
static int launch_dw_with(d3d_meta *m, const Plan &p, int cw, int T, DwKernel<S> k_atomic, DwKernel<S> k_det, const S *in,
                          int cin, const S *d_out, int cout, float *dW, hipStream_t s) {
  const int TPG = T < 16 ? T : 16;
  const int nz = (T + TPG - 1) / TPG;
  auto record = [&](int run, int chunk, int n_chunks, dim3 grid, bool det, int G, int scratch) {
    const int f[kDwFormFields] = {sizeof(S) == 4 ? 1 : 2, cw, cout, cin, T, nz, run, chunk, n_chunks, (int)grid.x,
                                  (int)grid.y, (int)grid.z, det ? 1 : 0, G, scratch, p.n_blk, p.K};
    std::copy(f, f + kDwFormFields, t_dw_last_form);
  };
  if (g_dw_deterministic || t_dw.on) {
    // fixed summation order: run r belongs to workgroup r % G, which adds its runs' blocks in order; the G partial
    // sums are added in order by k_dw_reduce.  Scratch: G x (K, cin, cout) floats, G <= kDwDetPartials and within
    // kDwDetBudget bytes (one partial at least) -- the caller's buffer (d3d_conv_dw_thread_mode), else the feature
    // lane, else a stream-ordered allocation when the lane is too small.
    const int run = kDwBlocksPerWg;
    const int n_runs = (p.n_blk + run - 1) / run;
    const size_t n = (size_t)p.K * cin * cout;
    const int G = dw_det_partials(n_runs, n);
    const size_t bytes = (size_t)G * n * sizeof(float);
    auto launch = [&](float *part) {
      hipLaunchKernelGGL(k_det, dim3(G, p.K, nz), dim3(256), 0, s, in, cin, d_out, p.nbrT,
                         p.n_blk * 32, p.rows, p.blkmask, p.n_blk, run, run, nz, part);
      hipLaunchKernelGGL(k_dw_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, G, n, dW);
    };
    if (t_dw.on && t_dw.scratch) {
      D3D_REQUIRE(t_dw.bytes >= bytes, "deterministic conv backward: scratch %zu < %zu bytes (d3d_conv_dw_scratch_bytes)",
                  t_dw.bytes, bytes);
      record(run, run, 1, dim3(G, p.K, nz), true, G, kDwScratchCaller);
      launch((float *)t_dw.scratch);
    } else {
      D3D_REQUIRE(m, "deterministic conv backward needs the metadata (its scratch lane)");
      D3D_LOCK(m);   // the mark / reset of the feature lane must not interleave with another thread's allocations
      const size_t mark = m->feat_arena.used;
      float *part = m->feat_arena.get<float>((size_t)G * n);
      if (part) {
        record(run, run, 1, dim3(G, p.K, nz), true, G, kDwScratchLane);
        launch(part);
        m->feat_arena.used = mark;   // stream-ordered scratch
      } else {                       // the lane is too small: a stream-ordered buffer of its own, the same partials
        m->feat_arena.used = mark;
        void *buf = nullptr;
        D3D_HIP_CHECK(hipMallocAsync(&buf, bytes, s));
        record(run, run, 1, dim3(G, p.K, nz), true, G, kDwScratchAsync);
        launch((float *)buf);
        D3D_HIP_CHECK(hipFreeAsync(buf, s));
      }
    }
    D3D_LAUNCH_CHECK();
    return D3D_OK;
  }
  // run length: long runs amortise the final atomics of a workgroup (T * 1024 of them), short runs keep a small
  // plan from being walked serially by a handful of workgroups -- aim at >= kDwTargetWgs workgroups.  Plans so large
  // that the run hits the 64 blocks one ballot covers deal the run's active blocks out in chunks of kDwMaxChunk
  // instead: the dense offsets (the centre one is in every block) would otherwise set the kernel's duration
  // (measured: Cin = Cout = 64 at 370 k rows 236 -> 186 us, 32 at 460 k rows 124 -> 90 us; smaller plans lose).
  long run = ((long)p.n_blk * p.K * nz + kDwTargetWgs - 1) / kDwTargetWgs;
  long chunk;
  if (run >= kDwBlocksPerWg) {
    run = kDwBlocksPerWg;
    chunk = kDwMaxChunk;
  } else {
    run = std::max<long>(2, run);
    chunk = run;
  }
  const int n_chunks = (int)((run + chunk - 1) / chunk);
  dim3 grid((unsigned)((p.n_blk + run - 1) / run), p.K, nz * n_chunks);
  record((int)run, (int)chunk, n_chunks, grid, false, 0, kDwScratchNone);
  hipLaunchKernelGGL(k_atomic, grid, dim3(256), 0, s, in, cin, d_out, p.nbrT, p.n_blk * 32, p.rows,
                     p.blkmask, p.n_blk, (int)run, (int)chunk, nz, dW);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}
template <int CP, int COUT>
static int launch_dw_t(d3d_meta *m, const Plan &p, const float *in, int cin, const float *d_out, float *dW, hipStream_t s) {
  return launch_dw_with<float>(m, p, CP, (CP / 32) * (COUT / 32), k_conv_dw<CP, COUT, false>, k_conv_dw<CP, COUT, true>, in,
                               cin, d_out, COUT, dW, s);
}
template <int CP>
static int launch_dw_c(d3d_meta *m, const Plan &p, const float *in, int cin, const float *d_out, int cout, float *dW,
                       hipStream_t s) {
  switch (cout) {
    case 32: return launch_dw_t<CP, 32>(m, p, in, cin, d_out, dW, s);
    case 64: return launch_dw_t<CP, 64>(m, p, in, cin, d_out, dW, s);
    case 128: return launch_dw_t<CP, 128>(m, p, in, cin, d_out, dW, s);
    case 256: return launch_dw_t<CP, 256>(m, p, in, cin, d_out, dW, s);
  }
  set_error("conv backward: Cout=%d not supported", cout);
  return D3D_ERR_UNSUPPORTED;
}
// dW[K, cin, cout] += ...   (dW pre-zeroed by the caller, like the reference's d_weight)
static int launch_dw(d3d_meta *m, const Plan &p, const float *in, int cin, const float *d_out, int cout, float *dW,
                     hipStream_t s) {
  if (p.n_rows == 0) return D3D_OK;
  D3D_REQUIRE(in && d_out && dW, "conv backward: null pointer");
  if (cin <= 32) return launch_dw_c<32>(m, p, in, cin, d_out, cout, dW, s);
  if (cin <= 64) return launch_dw_c<64>(m, p, in, cin, d_out, cout, dW, s);
  if (cin <= 128) return launch_dw_c<128>(m, p, in, cin, d_out, cout, dW, s);
  if (cin <= 256) return launch_dw_c<256>(m, p, in, cin, d_out, cout, dW, s);
  set_error("conv backward: Cin=%d not supported", cin);
  return D3D_ERR_UNSUPPORTED;
}

template <int CS>
static int launch_dw_bf16_c(d3d_meta *m, const Plan &p, const bf16_t *in, int cin, const bf16_t *d_out, int cout,
                            float *dW, hipStream_t s) {
  constexpr int NTI = CS < 32 ? 1 : CS / 32;
  switch (cout) {
    case 32: return launch_dw_with<bf16_t>(m, p, CS, NTI, k_conv_dw_bf16<CS, 32, false>, k_conv_dw_bf16<CS, 32, true>, in, cin, d_out, 32, dW, s);
    case 64: return launch_dw_with<bf16_t>(m, p, CS, NTI * 2, k_conv_dw_bf16<CS, 64, false>, k_conv_dw_bf16<CS, 64, true>, in, cin, d_out, 64, dW, s);
    case 128: return launch_dw_with<bf16_t>(m, p, CS, NTI * 4, k_conv_dw_bf16<CS, 128, false>, k_conv_dw_bf16<CS, 128, true>, in, cin, d_out, 128, dW, s);
    case 256: return launch_dw_with<bf16_t>(m, p, CS, NTI * 8, k_conv_dw_bf16<CS, 256, false>, k_conv_dw_bf16<CS, 256, true>, in, cin, d_out, 256, dW, s);
  }
  set_error("bf16 conv backward: Cout=%d not supported", cout);
  return D3D_ERR_UNSUPPORTED;
}
// dW[K, cin, cout] += ... from bf16 rows stored `cs` channels wide
static int launch_dw_bf16(d3d_meta *m, const Plan &p, const void *in_, int cs, int cin, const void *d_out_, int cout,
                          float *dW, hipStream_t s) {
  if (p.n_rows == 0) return D3D_OK;
  const bf16_t *in = (const bf16_t *)in_, *d_out = (const bf16_t *)d_out_;
  D3D_REQUIRE(in && d_out && dW, "bf16 conv backward: null pointer");
  D3D_REQUIRE((((uintptr_t)in | (uintptr_t)d_out) & 15) == 0, "bf16 conv backward: rows must be 16-byte aligned");
  switch (cs) {
    case 16: return launch_dw_bf16_c<16>(m, p, in, cin, d_out, cout, dW, s);
    case 32: return launch_dw_bf16_c<32>(m, p, in, cin, d_out, cout, dW, s);
    case 64: return launch_dw_bf16_c<64>(m, p, in, cin, d_out, cout, dW, s);
    case 128: return launch_dw_bf16_c<128>(m, p, in, cin, d_out, cout, dW, s);
    case 256: return launch_dw_bf16_c<256>(m, p, in, cin, d_out, cout, dW, s);
  }
  set_error("bf16 conv backward: stored Cin=%d not supported", cs);
  return D3D_ERR_UNSUPPORTED;
}

// Shapes of a bf16 backward call, checked before anything is launched: rows stored `cs` = 16 .. 256 channels wide for a
// weight of Cin = cin (cs = the padded width of cin), Cout 32 .. 256; dInput is the bf16 convolution with Cin' = cout and
// Cout' = cin, so it needs cin = cs in 32 .. 256.
static int check_bwd_bf16(int cs, int cin, int cout, bool want_d_in) {
  const bool cs_ok = cs == 16 || cs == 32 || cs == 64 || cs == 128 || cs == 256;
  const bool cout_ok = cout == 32 || cout == 64 || cout == 128 || cout == 256;
  if (!cs_ok || !cout_ok || cin < 1 || cin > cs || (cs > 16 && 2 * cin <= cs)) {
    set_error("bf16 conv backward: Cin=%d stored as %d, Cout=%d not supported", cin, cs, cout);
    return D3D_ERR_UNSUPPORTED;
  }
  if (want_d_in && (cin != cs || cs < 32)) {
    set_error("bf16 conv backward: dInput for Cin=%d (stored %d) is not built", cin, cs);
    return D3D_ERR_UNSUPPORTED;
  }
  return D3D_OK;
}

}  // namespace d3d

using namespace d3d;

extern "C" {

// The backward pass of a convolution of kind 0 submanifold (`in_size` is its spatial size, no out_size / stride), 1 strided
// or 2 deconvolution, rows of any d3d_dtype: d_in [rows_in, cs] (overwritten), d_weight [fv, cin, cout] fp32 (accumulated
// into; pre-zero it).  `cs` = stored width of `in` (and of d_in), `cin` = Cin of the weight / d_weight: equal for fp32
// rows (D3D_F32, or D3D_F32_X3: dInput as bf16x3 where it is served, dWeight exact either way).  dInput is a forward
// launch over the opposite view of the rulebook with W^T, dWeight runs over the view the forward pass used.
static int conv_backward(d3d_meta *m, int kind, const char *name, const int *in_size, const int *out_size,
                         const int *filt, const int *stride, const void *in, int cs, int cin, const void *packed_wt,
                         int cout, const void *d_out, void *d_in, float *d_weight, int dtype, hipStream_t s) {
  D3D_REQUIRE(is_conv_dtype(dtype), "%s: dtype %d is not a d3d_dtype", name, dtype);
  if (dtype != D3D_BF16)
    D3D_REQUIRE(cs == cin, "%s: fp32 rows are stored %d channels wide, not %d", name, cin, cs);
  else if (int rc = check_bwd_bf16(cs, cin, cout, d_in != nullptr))
    return rc;
  D3D_REQUIRE(m && in_size && filt && (kind == 0 || (out_size && stride)), "null argument");
  const int *fine = kind == 2 ? out_size : in_size;
  const Plan *fwd = nullptr;   // the submanifold rulebook, or fine -> coarse of a strided pair
  const Plan *dec = nullptr;   // coarse -> fine of a strided pair, finalised where it is first needed
  if (kind == 0) {
    for (int d = 0; d < 3; d++) D3D_REQUIRE(filt[d] % 2 == 1, "submanifold backward needs odd filter sizes");
    if (int rc = d3d_subm_prepare(m, in_size, filt, s, nullptr)) return rc;
    fwd = find_plan(m, 0, in_size, filt, nullptr);
  } else if (!(fwd = find_plan(m, 1, fine, filt, stride))) {
    set_error(kind == 1 ? "conv backward: forward rulebook not built" : "deconv backward: strided rulebook not built");
    return D3D_ERR_STATE;
  }
  if (d_in) {
    if (kind == 1)
      if (int rc = get_deconv_plan(m, fine, filt, stride, s, &dec)) return rc;
    if (int rc = launch_conv_dt(m, kind == 1 ? *dec : *fwd, d_out, cout, packed_wt, cs, nullptr, d_in, s, nullptr, dtype))
      return rc;
  }
  if (!d_weight) return D3D_OK;
  if (kind == 2)
    if (int rc = get_deconv_plan(m, fine, filt, stride, s, &dec)) return rc;
  const Plan &own = kind == 2 ? *dec : *fwd;
  if (dtype == D3D_BF16) return launch_dw_bf16(m, own, in, cs, cin, d_out, cout, d_weight, s);
  return launch_dw(m, own, (const float *)in, cin, (const float *)d_out, cout, d_weight, s);
}

int d3d_subm_conv_backward_dt(d3d_meta *m, const int *size, const int *filt, const void *in, int cs, int cin,
                              const void *packed_wt_flipped, int cout, const void *d_out, void *d_in, float *d_weight,
                              int dtype, void *stream) {
  return conv_backward(m, 0, "subm_conv_backward_dt", size, nullptr, filt, nullptr, in, cs, cin, packed_wt_flipped, cout,
                       d_out, d_in, d_weight, dtype, (hipStream_t)stream);
}

int d3d_conv_backward_dt(d3d_meta *m, const int *in_size, const int *out_size, const int *filt, const int *stride,
                         const void *in, int cs, int cin, const void *packed_wt, int cout, const void *d_out, void *d_in,
                         float *d_weight, int dtype, void *stream) {
  return conv_backward(m, 1, "conv_backward_dt", in_size, out_size, filt, stride, in, cs, cin, packed_wt, cout, d_out,
                       d_in, d_weight, dtype, (hipStream_t)stream);
}

int d3d_deconv_backward_dt(d3d_meta *m, const int *in_size, const int *out_size, const int *filt, const int *stride,
                           const void *in, int cs, int cin, const void *packed_wt, int cout, const void *d_out,
                           void *d_in, float *d_weight, int dtype, void *stream) {
  return conv_backward(m, 2, "deconv_backward_dt", in_size, out_size, filt, stride, in, cs, cin, packed_wt, cout, d_out,
                       d_in, d_weight, dtype, (hipStream_t)stream);
}

int d3d_conv_dw_deterministic(int on) {
  const int was = g_dw_deterministic ? 1 : 0;
  if (on >= 0) g_dw_deterministic = on != 0;
  return was;
}

int d3d_conv_dw_last_form(int *out, int n) {
  for (int i = 0; out && i < n && i < kDwFormFields; i++) out[i] = t_dw_last_form[i];
  std::fill(t_dw_last_form, t_dw_last_form + kDwFormFields, 0);
  return kDwFormFields;
}

size_t d3d_conv_dw_scratch_bytes(int filter_volume, int cin, int cout) {
  if (filter_volume <= 0 || cin <= 0 || cout <= 0) return 0;
  const size_t n = (size_t)filter_volume * cin * cout;
  return (size_t)dw_det_partials(kDwDetPartials, n) * n * sizeof(float);
}

int d3d_conv_dw_thread_mode(int on, void *scratch, size_t scratch_bytes) {
  const int was = t_dw.on ? 1 : 0;
  if (on < 0) return was;
  D3D_REQUIRE(on == 0 || (scratch && scratch_bytes > 0), "conv_dw_thread_mode: fixed order needs a scratch buffer");
  t_dw.on = on != 0;
  t_dw.scratch = t_dw.on ? scratch : nullptr;
  t_dw.bytes = t_dw.on ? scratch_bytes : 0;
  return was;
}

}  // extern "C"
