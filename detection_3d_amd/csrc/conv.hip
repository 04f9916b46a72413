// a6. Sparse convolution forward as ONE output-stationary launch per layer (the reference issues
// one kernel + one blocking rule memcpy per filter offset, SCN/CUDA/RuleBookIterator.h:15-32).
//
// Work decomposition: a block of 32 output rows (rows sorted by neighbour mask, see plan.hip
// finalize_plan) is owned by COUT/32/NT waves, each holding NT 32x32 accumulator tiles.  For
// every filter offset k present in the block's mask the waves gather the 32 input rows into an
// LDS tile (full rows, 16 B per thread, coalesced; register-staged one step ahead so that the
// loads overlap the matrix work), then run v_mfma_f32_32x32x2_f32 over Cin with the B operand
// (k-interleaved packed weights, L2-resident) read straight from global memory.  Accumulators
// stay in registers across all offsets; every output row is written exactly once (no atomics,
// deterministic, independent of how rows are grouped).
#include <algorithm>
#include <climits>

#include "d3d_internal.h"

namespace d3d {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void wave_lds_sync() {
  // LDS operations of one wave execute in issue order; this only stops the compiler from
  // moving LDS accesses of different lanes across the hand-off point.
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// packed[k][g][co][j] = w[k][4g+j][co]  (zero for 4g+j >= cin)
__global__ void k_pack_weight(const float *__restrict__ w, int fv, int cin, int cout, int cp,
                              float *__restrict__ packed) {
  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)fv * cp * cout;
  if (t >= total) return;
  int j = (int)(t & 3);
  long u = t >> 2;
  int co = (int)(u % cout);
  u /= cout;
  int g = (int)(u % (cp / 4));
  int k = (int)(u / (cp / 4));
  int ci = 4 * g + j;
  packed[t] = ci < cin ? w[((size_t)k * cin + ci) * cout + co] : 0.f;
}

void launch_pack_weight(const float *w, int fv, int cin, int cout, int cp, float *packed, hipStream_t s) {
  hipLaunchKernelGGL(k_pack_weight, grid1d((long)fv * cp * cout), dim3(256), 0, s, w, fv, cin, cout, cp, packed);
}

// CT   = Cin tile staged in LDS per step (multiple of 8, <= 128); NCT tiles cover Cin
// NT   = 32-column accumulator tiles per wave; a row block is shared by WPBLK = COUT/32/NT waves
// BPW  = row blocks per workgroup (only with WPBLK == 1, where waves never synchronise)
// VEC  = Cin equals the padded CT * NCT (16-byte row pieces): branch-free, VALU-lean gather
//
// The fp32 MFMA shares the SIMD's vector ALU with ordinary VALU instructions (scripts/mfma_probe.hip: every VALU
// instruction issued by ANY wave of the SIMD takes ~3.5 cycles away from the matrix pipe, nothing co-executes), so
// the gather costs as few VALU instructions as possible: wave-uniform (scalar) base pointers + 32-bit per-lane byte
// offsets, one multiplier per row (1 = real, 0 = absent neighbour) instead of per-element selects, fused multiply-add
// + max for the BatchNorm + ReLU prologue.
// LATE = the next step's gather (and index) loads are issued after the step's FIRST q-iteration instead of ahead of its matrix
//        work, branch-free (a step without successor requests absent rows).  The compiler's s_waitcnt placement is
//        conservative at the loop header: the wait in front of the step's first MFMA -- for weight fragments requested a
//        step ago -- also covered every load issued since, i.e. the gathers just requested: each step began with the
//        wave stalled for a full gather round trip.  Issued behind the first MFMAs, only loads of the previous step are
//        outstanding at that wait, and the counted waits inside the straight-line q-loop leave the gathers in flight.
template <int CT, int NCT, int COUT, int NT, int BPW, bool VEC, bool LATE = false>
__global__ __launch_bounds__(BPW *(COUT / 32 / NT) * 64) void k_conv(
    const float *__restrict__ in, int cin, const float *__restrict__ wp,
    const int32_t *__restrict__ nbrT, int npos, const int32_t *__restrict__ rows,
    const uint32_t *__restrict__ blkmask, int n_blk, const float *__restrict__ residual,
    float *__restrict__ out, int n_split, float *__restrict__ partial, BnPre pre, uint32_t in_bytes,
    double *__restrict__ stat) {
  __shared__ __attribute__((aligned(16))) float smem[BPW * 32 * (CT + 4)];
  const unsigned bx = blockIdx.x, by = blockIdx.y;
#include "conv_block.inc"
}

// ---- grouped launches (d3d_conv_group_forward): independent convolutions that resolve to the same instantiation run as
// ONE launch.  The members' kernel arguments travel as a table in the kernel argument segment; the grid is flat, member
// i owns the workgroups [first[i], first[i + 1]) = its own (ceil(n_blk / BPW), n_split) grid in x-major order, and a
// workgroup finds its member by a search over `first` (wave-uniform: the member's arguments stay in SGPRs), then runs
// k_conv's body (conv_block.inc) with exactly the arguments the member's own k_conv launch would have had.
struct ConvArgs {   // the arguments of one k_conv launch
  const float *in, *wp;
  const int32_t *nbrT, *rows;
  const uint32_t *blkmask;
  const float *residual;
  float *out, *partial;
  double *stat;
  BnPre pre;
  int cin, npos, n_blk, n_split;
  uint32_t in_bytes;
};
static constexpr int kGroupCap = 8;   // members per launch (a 1.1 KiB table); longer groups take several launches
struct ConvTable {
  ConvArgs m[kGroupCap];
  int first[kGroupCap + 1];   // prefix sums of the members' workgroup counts; INT_MAX behind the last member's end
};

template <int CT, int NCT, int COUT, int NT, int BPW, bool VEC, bool LATE>
__global__ __launch_bounds__(BPW *(COUT / 32 / NT) * 64) void k_conv_group(const ConvTable t) {
  __shared__ __attribute__((aligned(16))) float smem[BPW * 32 * (CT + 4)];
  const int wg = (int)blockIdx.x;
  int mi = 0;
#pragma unroll
  for (int i = 1; i < kGroupCap; i++) mi += wg >= t.first[i] ? 1 : 0;   // first[] never decreases
  const ConvArgs &a = t.m[mi];
  const float *__restrict__ in = a.in, *__restrict__ wp = a.wp, *__restrict__ residual = a.residual;
  const int32_t *__restrict__ nbrT = a.nbrT, *__restrict__ rows = a.rows;
  const uint32_t *__restrict__ blkmask = a.blkmask;
  float *__restrict__ out = a.out, *__restrict__ partial = a.partial;
  double *__restrict__ stat = a.stat;
  const BnPre pre = a.pre;
  const int cin = a.cin, npos = a.npos, n_blk = a.n_blk, n_split = a.n_split;
  const uint32_t in_bytes = a.in_bytes;
  const unsigned local = (unsigned)(wg - t.first[mi]), gx = (unsigned)((n_blk + BPW - 1) / BPW);
  const unsigned by = local / gx, bx = local - by * gx;
#include "conv_block.inc"
}

// out[rows[pos]] = sum_y partial[y][pos] (+ residual), y in increasing order.  `stat` (may be null): per-workgroup column
// sums / sums of squares of the rows it wrote, [gridDim.x][2 * cout] (see k_conv); a workgroup covers 1024 / cout rows.
// conv_reduce_block: workgroup bx of the member's own grid (blockIdx.x of k_conv_reduce); red = the kernel's 16 KiB of LDS.
__device__ __forceinline__ void conv_reduce_block(double (*red)[256][4], const unsigned bx,
                                                  const float *__restrict__ partial, int n_split, int npos, int cout4,
                                                  const int32_t *__restrict__ rows, const float *__restrict__ residual,
                                                  float *__restrict__ out, double *__restrict__ stat) {
  const long t = (long)bx * blockDim.x + threadIdx.x;
  const bool in_range = t < (long)npos * cout4;
  const int pos = in_range ? (int)(t / cout4) : 0, c4 = (int)(t % cout4);
  const int orow = in_range ? rows[pos] : -1;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (orow >= 0) {
    for (int y = 0; y < n_split; y++) acc += *(const f32x4 *)(partial + (((size_t)y * npos + pos) * cout4 + c4) * 4);
    const size_t o = ((size_t)orow * cout4 + c4) * 4;
    if (residual) acc += *(const f32x4 *)(residual + o);
    *(f32x4 *)(out + o) = acc;
  }
  if (!stat) return;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const double d = orow >= 0 ? (double)acc[j] : 0.0;
    red[0][threadIdx.x][j] = d;
    red[1][threadIdx.x][j] = d * d;
  }
  __syncthreads();
  if ((int)threadIdx.x < cout4) {   // (256 is a multiple of cout4: thread c4 of the first row owns channel group c4)
    double *sp = stat + (size_t)bx * (8 * cout4);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      double a = 0.0, b = 0.0;
      for (int q = threadIdx.x; q < 256; q += cout4) {
        a += red[0][q][j];
        b += red[1][q][j];
      }
      sp[c4 * 4 + j] = a;
      sp[4 * cout4 + c4 * 4 + j] = b;
    }
  }
}

__global__ __launch_bounds__(256) void k_conv_reduce(const float *__restrict__ partial, int n_split,
                                                     int npos, int cout4, const int32_t *__restrict__ rows,
                                                     const float *__restrict__ residual,
                                                     float *__restrict__ out, double *__restrict__ stat) {
  __shared__ double red[2][256][4];
  conv_reduce_block(red, blockIdx.x, partial, n_split, npos, cout4, rows, residual, out, stat);
}

// the reductions of a group's offset-split members as one launch: the table idea of k_conv_group
struct ReduceArgs {   // the arguments of one k_conv_reduce launch
  const float *partial;
  const int32_t *rows;
  const float *residual;
  float *out;
  double *stat;
  int n_split, npos, cout4;
};
struct ReduceTable {
  ReduceArgs m[kGroupCap];
  int first[kGroupCap + 1];
};

__global__ __launch_bounds__(256) void k_conv_reduce_group(const ReduceTable t) {
  __shared__ double red[2][256][4];
  const int wg = (int)blockIdx.x;
  int mi = 0;
#pragma unroll
  for (int i = 1; i < kGroupCap; i++) mi += wg >= t.first[i] ? 1 : 0;
  const ReduceArgs &a = t.m[mi];
  conv_reduce_block(red, (unsigned)(wg - t.first[mi]), a.partial, a.n_split, a.npos, a.cout4, a.rows, a.residual, a.out,
                    a.stat);
}

static constexpr int kSplitTargetWaves = 4096;  // below this many waves the launch is offset-split
static bool g_conv_late = [] {            // D3D_CONV_LATE=0: gathers issued ahead of the step's matrix work (A/B runs)
  const char *e = getenv("D3D_CONV_LATE");
  return !(e && e[0] == '0');
}();
static int g_conv_split = 0;   // d3d_conv_split_mode: 0 automatic, 1 never split, 2 split wherever the form allows it

int conv_n_split(bool allowed, int K, long waves, long target) {
  if (!allowed || K <= 1 || g_conv_split == 1) return 1;
  const int n = (int)std::min<long>(K, (target + waves - 1) / waves);
  if (g_conv_split == 2) return std::max(n, 2);
  return waves < target ? n : 1;
}

// d3d_conv_last_form: family, CT, NCT, COUT, BPW, RB, VEC, LATE, n_split, stats, n_blk, K
static constexpr int kFormFields = 12;
static thread_local int t_last_form[kFormFields] = {};
void conv_record_form(int family, int ct, int nct, int cout, int bpw, int rb, bool vec, bool late, int n_split,
                      bool stats, int n_blk, int K) {
  const int f[kFormFields] = {family, ct, nct, cout, bpw, rb, vec ? 1 : 0, late ? 1 : 0, n_split, stats ? 1 : 0, n_blk, K};
  std::copy(f, f + kFormFields, t_last_form);
}

// d3d_conv_time_next: HIP events the next k_conv launch of this thread is bracketed with (measurement only)
static thread_local hipEvent_t t_time_start = nullptr, t_time_stop = nullptr;
void conv_timing_take(hipEvent_t *start, hipEvent_t *stop) {
  *start = t_time_start;
  *stop = t_time_stop;
  t_time_start = t_time_stop = nullptr;
}

struct StatOut {   // d3d_bn_prologue.out_stats*: where the launch leaves the column statistics of its output
  double *buf;
  int cap;
  int *rows_host;
};

// ---- a group being collected (d3d_conv_group_forward): launch_t parks the launches it would have made here, and
// conv_group_flush issues them, one k_conv_group per instantiation and kGroupCap members, then one k_conv_reduce_group
typedef void (*GroupLaunchFn)(int variant, const ConvTable &t, unsigned blocks, hipStream_t s);
struct PendingConv {
  ConvArgs a;
  GroupLaunchFn fn;      // launches the member's instantiation family ...
  int variant;           // ... 0: plain gather, 1: VEC, 2: VEC + LATE
  int bpw, cout;         // BPW and COUT of the instantiation
  double *reduce_stat;   // the column statistics of an offset-split member come from its reduction
};
static constexpr int kMaxGroup = 32;   // launches parked at a time (d3d_conv_group_forward flushes when full)
struct ConvGroup {
  PendingConv conv[kMaxGroup];
  int n = 0;
  bool holds_partials = false;
  size_t mark = 0;    // feat_arena.used in front of the group's first partial buffer
};
static thread_local ConvGroup *t_group = nullptr;

// prefix sums of the workgroup counts of a table's n members -> first[]; returns the total
template <typename Table, typename Count>
static unsigned group_prefix(Table &t, int n, Count count) {
  long total = 0;
  for (int i = 0; i <= kGroupCap; i++) {
    t.first[i] = i <= n ? (int)total : INT_MAX;
    if (i < n) total += count(i);
  }
  return (unsigned)total;
}

static int conv_group_flush(d3d_meta *m, hipStream_t s) {
  ConvGroup *g = t_group;
  if (!g || g->n == 0) return D3D_OK;
  bool done[kMaxGroup] = {};
  for (int i = 0; i < g->n; i++) {
    if (done[i]) continue;
    // the members of member i's instantiation, in table order, kGroupCap at a time
    ConvTable t;
    int n = 0;
    for (int j = i; j <= g->n; j++) {
      const bool same = j < g->n && !done[j] && g->conv[j].fn == g->conv[i].fn && g->conv[j].variant == g->conv[i].variant;
      if (same) {
        t.m[n++] = g->conv[j].a;
        done[j] = true;
      }
      if (n == kGroupCap || (j == g->n && n > 0)) {
        const ConvTable &tc = t;
        const unsigned blocks = group_prefix(t, n, [&](int q) {
          return (long)((tc.m[q].n_blk + g->conv[i].bpw - 1) / g->conv[i].bpw) * tc.m[q].n_split;
        });
        g->conv[i].fn(g->conv[i].variant, t, blocks, s);
        n = 0;
      }
    }
  }
  ReduceTable r;
  int n = 0;
  for (int j = 0; j <= g->n; j++) {
    if (j < g->n && g->conv[j].a.n_split > 1) {
      const ConvArgs &a = g->conv[j].a;
      r.m[n++] = {a.partial, a.rows, a.residual, a.out, g->conv[j].reduce_stat, a.n_split, a.npos, g->conv[j].cout / 4};
    }
    if (n == kGroupCap || (j == g->n && n > 0)) {
      const ReduceTable &rc = r;
      const unsigned blocks = group_prefix(r, n, [&](int q) { return ((long)rc.m[q].npos * rc.m[q].cout4 + 255) / 256; });
      hipLaunchKernelGGL(k_conv_reduce_group, dim3(blocks), dim3(256), 0, s, r);
      n = 0;
    }
  }
  if (g->holds_partials) m->feat_arena.used = g->mark;  // stream-ordered scratch
  g->n = 0;
  g->holds_partials = false;
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

template <int CT, int NCT, int COUT, int NT, int BPW>
static void launch_group_t(int variant, const ConvTable &t, unsigned blocks, hipStream_t s) {
  constexpr int threads = BPW * (COUT / 32 / NT) * 64;
  if (variant == 2)
    hipLaunchKernelGGL((k_conv_group<CT, NCT, COUT, NT, BPW, true, true>), dim3(blocks), dim3(threads), 0, s, t);
  else if (variant == 1)
    hipLaunchKernelGGL((k_conv_group<CT, NCT, COUT, NT, BPW, true, false>), dim3(blocks), dim3(threads), 0, s, t);
  else
    hipLaunchKernelGGL((k_conv_group<CT, NCT, COUT, NT, BPW, false, false>), dim3(blocks), dim3(threads), 0, s, t);
}

template <int CT, int NCT, int COUT, int NT, int BPW>
static int launch_t(d3d_meta *m, const Plan &p, const float *in, int cin, const float *wp,
                    const float *residual, float *out, hipStream_t s, BnPre pre, const StatOut &so) {
  constexpr int WPBLK = COUT / 32 / NT;
  constexpr int threads = BPW * WPBLK * 64;
  const int npos = p.n_blk * 32;
  const long waves = (long)p.n_blk * WPBLK;
  ConvGroup *grp = t_group;   // collecting a group: the launch is parked, not made
  int n_split = conv_n_split(BPW == 1 && m, p.K, waves, kSplitTargetWaves);
  float *partial = nullptr;
  size_t mark = 0;
  if (n_split > 1) {
    mark = m->feat_arena.used;
    partial = m->feat_arena.get<float>((size_t)n_split * npos * COUT);
    if (!partial && grp && grp->holds_partials) {
      // the partial buffers of the members parked so far are in the way: launch those first, so that this member splits
      // exactly where its own call would have
      const int rc = conv_group_flush(m, s);
      if (rc) return rc;
      mark = m->feat_arena.used;
      partial = m->feat_arena.get<float>((size_t)n_split * npos * COUT);
    }
    if (!partial) n_split = 1;  // no room: fall back to the unsplit launch
  }
  const dim3 grid((p.n_blk + BPW - 1) / BPW, n_split);
  // column statistics of the output for the BatchNorm that follows: one vector pair per row block, or per workgroup of
  // the reduction when the launch is offset-split
  const long reduce_blocks = ((long)npos * (COUT / 4) + 255) / 256;
  const long stat_rows = n_split > 1 ? reduce_blocks : p.n_blk;
  double *stat = (so.buf && stat_rows <= so.cap) ? so.buf : nullptr;
  if (so.rows_host) *so.rows_host = stat ? (int)stat_rows : 0;
  const uint32_t in_bytes = (uint32_t)((size_t)p.n_in * (size_t)cin * 4);   // < 4 GiB (launch_conv checks)
  const hipEvent_t ev_start = t_time_start, ev_stop = t_time_stop;
  t_time_start = t_time_stop = nullptr;
  if (ev_start) (void)hipEventRecord(ev_start, s);
  const bool vec = cin == CT * NCT, late = vec && g_conv_late && CT >= 32;
  if (vec && n_split == 1 && launch_conv_ws(p, in, cin, wp, COUT, residual, out, s, pre, stat, in_bytes)) {
    // (taken by the weight-sharing kernel: same products in the same order; it records its form)
  } else {
    conv_record_form(kFormConv, CT, NCT, COUT, BPW, 1, vec, late, n_split, stat != nullptr, p.n_blk, p.K);
    if (grp) {
      if (partial && !grp->holds_partials) {
        grp->holds_partials = true;
        grp->mark = mark;
      }
      PendingConv &pc = grp->conv[grp->n++];
      pc.a = {in, wp, p.nbrT, p.rows, p.blkmask, residual, out, partial, n_split > 1 ? nullptr : stat, pre,
              cin, npos, p.n_blk, n_split, in_bytes};
      pc.fn = launch_group_t<CT, NCT, COUT, NT, BPW>;
      pc.variant = late ? 2 : (vec ? 1 : 0);
      pc.bpw = BPW;
      pc.cout = COUT;
      pc.reduce_stat = n_split > 1 ? stat : nullptr;
      return D3D_OK;
    }
    if (late)
      hipLaunchKernelGGL((k_conv<CT, NCT, COUT, NT, BPW, true, true>), grid, dim3(threads), 0, s, in, cin, wp, p.nbrT,
                         npos, p.rows, p.blkmask, p.n_blk, residual, out, n_split, partial, pre, in_bytes,
                         n_split > 1 ? nullptr : stat);
    else if (vec)
      hipLaunchKernelGGL((k_conv<CT, NCT, COUT, NT, BPW, true>), grid, dim3(threads), 0, s, in, cin, wp, p.nbrT, npos,
                         p.rows, p.blkmask, p.n_blk, residual, out, n_split, partial, pre, in_bytes,
                         n_split > 1 ? nullptr : stat);
    else
      hipLaunchKernelGGL((k_conv<CT, NCT, COUT, NT, BPW, false>), grid, dim3(threads), 0, s, in, cin, wp, p.nbrT, npos,
                         p.rows, p.blkmask, p.n_blk, residual, out, n_split, partial, pre, in_bytes,
                         n_split > 1 ? nullptr : stat);
  }
  if (ev_stop) (void)hipEventRecord(ev_stop, s);   // k_conv alone: the reduction of an offset-split launch follows
  if (n_split > 1) {
    const long total = (long)npos * (COUT / 4);
    hipLaunchKernelGGL(k_conv_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, partial, n_split,
                       npos, COUT / 4, p.rows, residual, out, stat);
    m->feat_arena.used = mark;  // stream-ordered scratch
  }
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

template <int CT, int NCT>
static int launch_c(d3d_meta *m, const Plan &p, const float *in, int cin, const float *wp, int cout,
                    const float *residual, float *out, hipStream_t s, BnPre pre, const StatOut &so) {
  switch (cout) {
    case 32: return launch_t<CT, NCT, 32, 1, 4>(m, p, in, cin, wp, residual, out, s, pre, so);    // 4 independent waves
    // (NT = 2 -- half as many waves per row block, no or fewer barriers -- measured slower; DESIGN.md lists the other
    //  variants that lost to this shape: 64-row groups, streaming workgroups, LDS-free A, shared weight tile)
    case 64: return launch_t<CT, NCT, 64, 1, 1>(m, p, in, cin, wp, residual, out, s, pre, so);    // 2 waves / block
    case 128: return launch_t<CT, NCT, 128, 1, 1>(m, p, in, cin, wp, residual, out, s, pre, so);  // 4 waves / block
    case 256: return launch_t<CT, NCT, 256, 1, 1>(m, p, in, cin, wp, residual, out, s, pre, so);  // 8 waves / block
  }
  set_error("convolution: Cout=%d not supported (32, 64, 128, 256)", cout);
  return D3D_ERR_UNSUPPORTED;
}

int launch_conv(d3d_meta *m, const Plan &p, const float *in, int cin, const float *packed_w, int cout,
                const float *residual, float *out, hipStream_t s, const d3d_bn_prologue *bn) {
  if (bn && bn->out_stats_rows) *bn->out_stats_rows = 0;
  if (p.n_rows == 0) {
    if (t_time_start) (void)hipEventRecord(t_time_start, s);
    if (t_time_stop) (void)hipEventRecord(t_time_stop, s);
    t_time_start = t_time_stop = nullptr;
    return D3D_OK;
  }
  D3D_REQUIRE(in && packed_w && out, "convolution: null pointer");
  D3D_REQUIRE((size_t)p.n_in * (size_t)cin * 4 < ((size_t)1 << 32),
              "convolution: gathered tensor of %d rows x %d channels exceeds the 4 GiB of the 32-bit gather offsets", p.n_in, cin);
  BnPre pre = {nullptr, nullptr, nullptr, nullptr, 0.f};
  StatOut so = {nullptr, 0, nullptr};
  if (bn) {
    so = {bn->out_stats, bn->out_stats_cap, bn->out_stats_rows};
    if (so.rows_host) *so.rows_host = 0;
  }
  if (bn && bn->mean) {
    D3D_REQUIRE(bn->invstd && cin % 8 == 0 && padded_cin(cin) == cin, "fused BatchNorm prologue needs Cin in {32,64,128,256}");
    pre = {bn->mean, bn->invstd, bn->weight, bn->bias, bn->leakiness};
  }
  switch (padded_cin(cin)) {
    case 16: return launch_c<16, 1>(m, p, in, cin, packed_w, cout, residual, out, s, pre, so);
    case 32: return launch_c<32, 1>(m, p, in, cin, packed_w, cout, residual, out, s, pre, so);
    case 64: return launch_c<64, 1>(m, p, in, cin, packed_w, cout, residual, out, s, pre, so);
    case 128: return launch_c<128, 1>(m, p, in, cin, packed_w, cout, residual, out, s, pre, so);
    case 256: return launch_c<128, 2>(m, p, in, cin, packed_w, cout, residual, out, s, pre, so);
  }
  set_error("convolution: Cin=%d not supported (<= 256)", cin);
  return D3D_ERR_UNSUPPORTED;
}

void launch_conv_reduce(const float *partial, int n_split, int npos, int cout, const int32_t *rows, const float *residual,
                        float *out, hipStream_t s) {
  const long total = (long)npos * (cout / 4);
  hipLaunchKernelGGL(k_conv_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, partial, n_split, npos,
                     cout / 4, rows, residual, out, nullptr);
}

int launch_conv_dt(d3d_meta *m, const Plan &p, const void *in, int cin, const void *packed_w, int cout,
                   const void *residual, void *out, hipStream_t s, const d3d_bn_prologue *bn, int dtype) {
  if (dtype == D3D_BF16 || (dtype == D3D_F32_X3 && conv_x3_serves(p.K, cin, cout)))
    return launch_conv_bf16(m, p, in, cin, packed_w, cout, residual, out, s, bn, dtype);
  return launch_conv(m, p, (const float *)in, cin, (const float *)packed_w, cout, (const float *)residual, (float *)out,
                     s, bn);
}

}  // namespace d3d

using namespace d3d;

extern "C" {

int d3d_conv_late_mode(int on) {
  const int was = g_conv_late ? 1 : 0;
  if (on >= 0) g_conv_late = on != 0;
  return was;
}

int d3d_conv_split_mode(int mode) {
  const int was = g_conv_split;
  if (mode >= 0 && mode <= 2) g_conv_split = mode;
  return was;
}

int d3d_conv_last_form(int *out, int n) {
  for (int i = 0; out && i < n && i < kFormFields; i++) out[i] = t_last_form[i];
  std::fill(t_last_form, t_last_form + kFormFields, 0);
  return kFormFields;
}

int d3d_conv_time_next(void *start_event, void *stop_event) {
  t_time_start = (hipEvent_t)start_event;
  t_time_stop = (hipEvent_t)stop_event;
  return D3D_OK;
}

// The plan of a forward call, built on first use: kind 0 submanifold (`in_size` is its spatial size, no out_size / stride),
// 1 strided convolution, 2 deconvolution (in = coarse, out = fine features; reuses the strided rulebook of the matching
// convolution with the roles swapped, SCN/CPU/Deconvolution.cpp:17,33-37).  With `macs_host`, the multiply-accumulates
// of a cin -> cout layer over that plan are counted too.
static int forward_plan(d3d_meta *m, int kind, const int *in_size, const int *out_size, const int *filt,
                        const int *stride, hipStream_t s, int cin, int cout, double *macs_host, const Plan **out) {
  const Plan *p = nullptr;
  int rc;
  if (kind == 0) {
    rc = d3d_subm_prepare(m, in_size, filt, s, nullptr);
    if (!rc) p = find_plan(m, 0, in_size, filt, nullptr);
  } else if (kind == 1) {
    rc = d3d_conv_prepare(m, in_size, out_size, filt, stride, s, nullptr, nullptr);
    if (!rc) p = find_plan(m, 1, in_size, filt, stride);
  } else {
    rc = get_deconv_plan(m, out_size, filt, stride, s, &p);
  }
  if (rc) return rc;
  if (macs_host && p) {
    long nr;
    rc = plan_rules(m, *const_cast<Plan *>(p), s, &nr);
    if (rc) return rc;
    *macs_host = (double)nr * cin * cout;
  }
  *out = p;
  return D3D_OK;
}

// Storage types (d3d_dtype, launch_conv_dt): D3D_F32 runs k_conv, D3D_BF16 runs conv_bf16.hip, D3D_F32_X3 runs
// conv_bf16.hip's bf16x3 form where conv_x3_serves(K, cin, cout) and k_conv elsewhere.
// For bf16, `cin` is the stored row width (16, 32, 64, 128 or 256 channels; narrower inputs are zero padded).
int d3d_subm_conv_forward_dt(d3d_meta *m, const int *size, const int *filt, const void *in, int cin,
                             const void *packed_w, int cout, const void *residual, void *out, int dtype, void *stream,
                             double *macs_host, const d3d_bn_prologue *bn) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(is_conv_dtype(dtype) && m && size && filt, "subm_conv_forward_dt: bad arguments");
  const Plan *p = nullptr;
  if (int rc = forward_plan(m, 0, size, nullptr, filt, nullptr, s, cin, cout, macs_host, &p)) return rc;
  return launch_conv_dt(m, *p, in, cin, packed_w, cout, residual, out, s, bn, dtype);
}

int d3d_conv_forward_dt(d3d_meta *m, const int *in_size, const int *out_size, const int *filt, const int *stride,
                        const void *in, int cin, const void *packed_w, int cout, void *out, int dtype, void *stream,
                        double *macs_host, const d3d_bn_prologue *bn) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(is_conv_dtype(dtype) && m && in_size && out_size && filt && stride, "conv_forward_dt: bad arguments");
  const Plan *p = nullptr;
  if (int rc = forward_plan(m, 1, in_size, out_size, filt, stride, s, cin, cout, macs_host, &p)) return rc;
  return launch_conv_dt(m, *p, in, cin, packed_w, cout, nullptr, out, s, bn, dtype);
}

int d3d_deconv_forward_dt(d3d_meta *m, const int *in_size, const int *out_size, const int *filt, const int *stride,
                          const void *in, int cin, const void *packed_w, int cout, const void *residual, void *out,
                          int dtype, void *stream, double *macs_host, const d3d_bn_prologue *bn) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(is_conv_dtype(dtype) && m && in_size && out_size && filt && stride, "deconv_forward_dt: bad arguments");
  const Plan *p = nullptr;
  if (int rc = forward_plan(m, 2, in_size, out_size, filt, stride, s, cin, cout, macs_host, &p)) return rc;
  return launch_conv_dt(m, *p, in, cin, packed_w, cout, residual, out, s, bn, dtype);
}

// One call for n independent convolutions (no member reads what another writes): every member that resolves to the same
// k_conv instantiation runs in one k_conv_group launch, the reductions of the offset-split members in one
// k_conv_reduce_group launch.  What does not resolve to k_conv (the weight-sharing kernel, bf16 rows, bf16x3 products)
// and every member that carries timing events runs at once, as its own call would.
int d3d_conv_group_forward(d3d_meta *m, const d3d_conv_desc *descs, int n, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  D3D_REQUIRE(m && n >= 0 && (descs || n == 0), "conv_group_forward: bad arguments");
  D3D_REQUIRE(!t_group, "conv_group_forward: a group is already being collected on this thread");
  // every plan first: building a rulebook takes scratch where the partial buffers of parked members live
  for (int i = 0; i < n; i++) {
    const d3d_conv_desc &d = descs[i];
    D3D_REQUIRE(d.kind >= 0 && d.kind <= 2, "conv_group_forward: member %d has kind %d (0, 1 or 2)", i, d.kind);
    D3D_REQUIRE(is_conv_dtype(d.dtype), "conv_group_forward: member %d: bad dtype", i);
    const Plan *p = nullptr;
    if (int rc = forward_plan(m, d.kind, d.in_size, d.out_size, d.filter, d.stride, s, d.cin, d.cout, d.macs_host, &p))
      return rc;
    D3D_REQUIRE(p, "conv_group_forward: member %d has no plan", i);
  }
  ConvGroup g;
  int rc = D3D_OK;
  for (int i = 0; i < n && !rc; i++) {
    const d3d_conv_desc &d = descs[i];
    const Plan *p = nullptr;
    rc = forward_plan(m, d.kind, d.in_size, d.out_size, d.filter, d.stride, s, d.cin, d.cout, nullptr, &p);   // a lookup now
    if (rc) break;
    t_group = &g;
    if (g.n == kMaxGroup) rc = conv_group_flush(m, s);
    if (rc) break;
    if (d.time_start || d.time_stop) {   // measured: its events bracket a k_conv launch of its own
      t_group = nullptr;
      t_time_start = (hipEvent_t)d.time_start;
      t_time_stop = (hipEvent_t)d.time_stop;
    }
    std::fill(t_last_form, t_last_form + kFormFields, 0);
    rc = launch_conv_dt(m, *p, d.in, d.cin, d.packed_w, d.cout, d.kind == 1 ? nullptr : d.residual, d.out, s, d.bn_host, d.dtype);
    if (d.form) std::copy(t_last_form, t_last_form + kFormFields, d.form);
  }
  t_group = &g;
  if (!rc) {
    rc = conv_group_flush(m, s);
  } else if (g.holds_partials) {
    m->feat_arena.used = g.mark;
  }
  t_group = nullptr;
  return rc;
}

}  // extern "C"
