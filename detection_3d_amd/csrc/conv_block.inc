// The body of one k_conv workgroup, included by k_conv and k_conv_group (conv.hip) so that both compile the very same
// statements.  In scope at the point of inclusion: the template parameters CT, NCT, COUT, NT, BPW, VEC, LATE; the
// arguments of a k_conv launch (in, cin, wp, nbrT, npos, rows, blkmask, n_blk, residual, out, n_split, partial, pre,
// in_bytes, stat); `unsigned bx, by`, the workgroup's coordinates in the launch's own grid (ceil(n_blk / BPW), n_split);
// and `float smem[BPW * 32 * (CT + 4)]` in LDS.
  constexpr int WPBLK = COUT / 32 / NT;
  static_assert(WPBLK == 1 || BPW == 1, "row blocks sharing a workgroup must be single-wave");
  constexpr int TPB = WPBLK * 64;  // threads working on one row block
  constexpr int LDA = CT + 4;      // +4 dwords: conflict-free ds_read_b128 of 32 rows
  constexpr int CP = CT * NCT;
  constexpr int LPR = CT / 4;      // threads per gathered row (16 B each)
  constexpr int RPP = TPB / LPR;   // rows per gather pass
  constexpr int NIT = (32 / RPP) > 0 ? (32 / RPP) : 1;
  constexpr int NQ = CT / 8;       // q-iterations (4 MFMAs per accumulator tile each) of a step
  // weight fragments in flight (ring): 8 q-iterations = 2048 matrix cycles of lead (4: the 128 -> 128 family 0.91 ms per
  // building against 0.89, 2: 0.95; D3D_QA at compile time)
#ifndef D3D_QA
#define D3D_QA 8
#endif
  constexpr int QA = NQ < D3D_QA ? NQ : D3D_QA;
  static_assert(NQ % QA == 0, "ring depth must divide the q-iterations of a step");

  const int slot = threadIdx.x / TPB, tib = threadIdx.x % TPB;
  const int blk = bx * BPW + slot;
  if (blk >= n_blk) return;  // BPW > 1 only when waves are independent (no barrier below)
  float *As = smem + slot * 32 * LDA;
  const int lane = tib & 63, wib = tib >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int grow = tib / LPR, gc4 = tib % LPR;
  const int colbase = wib * NT * 32;

  auto block_sync = [&]() {
    if constexpr (WPBLK == 1)
      wave_lds_sync();
    else
      __syncthreads();
  };

  // active offsets of the block; wave-uniform: keep it (and with it k, the weight / index base pointers and the loop
  // control) in SGPRs
  uint32_t mask = __builtin_amdgcn_readfirstlane(blkmask[blk]);
  if (n_split > 1) {
    // offset-split launch (few rows): this workgroup keeps every n_split-th active offset and
    // writes a partial tile; k_conv_reduce sums the partials in a fixed order.
    // by the offset's INDEX, not by its rank among the block's active offsets: which partial sum an offset of a row
    // lands in then does not depend on the other rows of the block, so the result is independent of how rows are
    // grouped into blocks (e.g. the same rows reached through plans of different builds)
    uint32_t keep = 0;
    for (uint32_t m = mask; m; m &= m - 1) {
      const int kk = __builtin_ctz(m);
      if (kk % n_split == (int)by) keep |= 1u << kk;
    }
    mask = keep;
  }
  const int rowid = rows[blk * 32 + r];
  f32x16 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; nt++)
#pragma unroll
    for (int i = 0; i < 16; i++) acc[nt][i] = 0.f;

  const int32_t *nb = nbrT + (size_t)blk * 32;
  // Gather of (offset k, Cin tile ct) in two independent waves of loads, both issued ahead of their use:
  //   load_idx(k)   : the NIT input-row indices this thread needs for offset k   (one step before issue_data)
  //   issue_data(ct): the 16-byte row pieces, branch-free -- an absent neighbour reads row 0 and is zeroed
  //                   at commit time, so that no load waits for another one
  //   commit_gather : registers -> LDS (+ the fused BatchNorm), after the previous step's MFMAs
  int idx[NIT];
  f32x4 stage[NIT];
  float mreal[NIT];  // 1.f for a real row, 0.f for an absent one
  int stage_ct = 0;
  // optional fused BatchNorm + leaky ReLU of the producer layer (y = leaky(fma(x, w, b)), applied to real rows
  // only: a missing neighbour contributes zeros, as a zero row of the normalised tensor would not);
  // this thread always gathers the same 4 channels of a Cin tile, so w and b are fetched once
  f32x4 bnw[NCT], bnb[NCT];
#pragma unroll
  for (int t = 0; t < NCT; t++) {
    bnw[t] = {1.f, 1.f, 1.f, 1.f};
    bnb[t] = {0.f, 0.f, 0.f, 0.f};
    if (pre.mean) {
      const int c = t * CT + gc4 * 4;
      const f32x4 is = *(const f32x4 *)(pre.invstd + c), mu = *(const f32x4 *)(pre.mean + c);
      const f32x4 one = {1.f, 1.f, 1.f, 1.f}, zero = {0.f, 0.f, 0.f, 0.f};
      const f32x4 ga = pre.weight ? *(const f32x4 *)(pre.weight + c) : one;
      const f32x4 be = pre.bias ? *(const f32x4 *)(pre.bias + c) : zero;
      bnw[t] = is * ga;
      bnb[t] = -mu * bnw[t] + be;
    }
  }
  const uint32_t lane_piece = (uint32_t)gc4 * 16u, lane_idx = (uint32_t)grow * 4u;
  // The gathered tensor as a raw buffer of in_bytes: a row piece of an ABSENT neighbour is requested at an offset past
  // the end, which the hardware range check answers with zeros -- no branch, no select, and nothing of a real row
  // (row 0 used to stand in, and its NaN or Inf would have spread through the 0 * x of the commit) reaches the tile.
  const __amdgpu_buffer_rsrc_t in_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)in, 0, (int)in_bytes, 0x00020000);
  auto load_idx = [&](int k) {
    const char *kb = (const char *)(nb + (size_t)k * npos);  // wave-uniform
#pragma unroll
    for (int it = 0; it < NIT; it++) {
      if constexpr (RPP <= 32) {
        idx[it] = *(const int32_t *)(kb + (lane_idx + (uint32_t)(it * RPP * 4)));
      } else {  // a pass wider than the block (tiny Cin tile, many waves): threads past row 31 idle
        idx[it] = grow < 32 ? *(const int32_t *)(kb + lane_idx) : -1;
      }
    }
  };
  auto issue_data = [&](int ct) {
    stage_ct = ct;
#pragma unroll
    for (int it = 0; it < NIT; it++) {
      const int s = idx[it];
      mreal[it] = s >= 0 ? 1.f : 0.f;
      if constexpr (VEC) {
        // rows are CP * 4 bytes (< 4 GiB tensor); 0xfffffff0 + 16 exceeds any buffer size
        const uint32_t off = s < 0 ? 0xfffffff0u : (uint32_t)s * (uint32_t)(CP * 4) + (uint32_t)(ct * CT * 4) + lane_piece;
        stage[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, (int)off, 0, 0));
      } else {
        const float *p = in + (size_t)(s < 0 ? 0 : s) * cin + ct * CT + gc4 * 4;
        const int c = ct * CT + gc4 * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (c + 0 < cin) v[0] = p[0];
        if (c + 1 < cin) v[1] = p[1];
        if (c + 2 < cin) v[2] = p[2];
        if (c + 3 < cin) v[3] = p[3];
        stage[it] = v;
      }
    }
  };
  auto commit_gather = [&]() {
    const f32x4 bw = stage_ct == 0 ? bnw[0] : bnw[NCT - 1], bb = stage_ct == 0 ? bnb[0] : bnb[NCT - 1];
#pragma unroll
    for (int it = 0; it < NIT; it++) {
      const int row = it * RPP + grow;
      f32x4 v = stage[it];
      if constexpr (VEC) {
        // an absent row arrived as zeros; only the fused BatchNorm turns them into leaky(beta'), which the row's
        // multiplier (0 or 1, one VALU instruction per 2 elements) takes out again -- finite times 0
        if (pre.mean) v = bn_act(v, bw, bb, pre.leak) * mreal[it];
      } else {
        if (pre.mean) v = bn_act(v, bw, bb, pre.leak);
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        v = mreal[it] != 0.f ? v : zero;     // a select: row 0 stood in for the absent neighbour
      }
      if (row < 32) *(f32x4 *)(As + row * LDA + gc4 * 4) = v;
    }
  };

  // step tokens: (offset k, Cin tile ct) in increasing (k, ct) order over the active offsets
  auto next_k = [&](int k) -> int {
    const uint32_t m = k >= 31 ? 0u : (mask & ~((2u << k) - 1u));
    return m ? __builtin_ctz(m) : -1;
  };
  int k = mask ? __builtin_ctz(mask) : -1;
  int ct = 0;
  // weight fragments (packed weights, L2-resident, shared by every block) come through a ring of QA q-iterations
  // in flight that runs across step boundaries: the last QA refills of a step fetch the first fragments of the
  // next one (the compiler alone keeps only ~1 load ahead)
  f32x4 ring[QA][NT];
  const uint32_t lane_b = (uint32_t)(h * COUT + r) * 16u;   // this lane's byte offset inside a weight fragment row
  if (k >= 0) {
    load_idx(k);
    issue_data(0);
    const int k_after = NCT > 1 ? k : next_k(k);   // indices of the step after this one
    if (k_after >= 0 && k_after != k) load_idx(k_after);
    const char *wk0 = (const char *)(wp + ((size_t)(k * (CP / 4)) * COUT + colbase) * 4);
#pragma unroll
    for (int q = 0; q < QA; q++)
#pragma unroll
      for (int nt = 0; nt < NT; nt++)
        ring[q][nt] = *(const f32x4 *)(wk0 + (lane_b + (uint32_t)((2 * q * COUT + nt * 32) * 16)));
  }
  while (k >= 0) {
    commit_gather();
    block_sync();
    // next (offset, tile) step
    int nk = k, nct = ct + 1;
    if (nct == NCT) {
      nct = 0;
      nk = next_k(k);
    }
    const int k2 = nk < 0 ? -1 : ((nct + 1 < NCT) ? nk : next_k(nk));   // the step after that: its indices are requested now
    if constexpr (!LATE) {
      if (nk >= 0) {
        issue_data(nct);  // loads fly while the matrix cores work; idx holds offset nk
        if (k2 >= 0 && k2 != nk) load_idx(k2);
      }
    }
    __builtin_amdgcn_s_setprio(1);
    // ---- 32 x (NT*32) += A[32 x CT] * W[k][CT x cols] ----
    const char *wk = (const char *)(wp + ((size_t)(k * (CP / 4) + ct * (CT / 4)) * COUT + colbase) * 4);
    const char *wk_next = nk >= 0 ? (const char *)(wp + ((size_t)(nk * (CP / 4) + nct * (CT / 4)) * COUT + colbase) * 4) : wk;
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      f32x4 b[NT];
#pragma unroll
      for (int nt = 0; nt < NT; nt++) b[nt] = ring[q % QA][nt];
      {
        const char *src = (q + QA < NQ) ? wk : wk_next;   // wave-uniform base + per-lane byte offset
        const int qq = (q + QA) % NQ;
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
          ring[q % QA][nt] = *(const f32x4 *)(src + (lane_b + (uint32_t)((2 * qq * COUT + nt * 32) * 16)));
      }
      const f32x4 a = *(const f32x4 *)(As + r * LDA + q * 8 + h * 4);
#pragma unroll
      for (int nt = 0; nt < NT; nt++) {
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b[nt][0], acc[nt], 0, 0, 0);
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], b[nt][1], acc[nt], 0, 0, 0);
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], b[nt][2], acc[nt], 0, 0, 0);
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], b[nt][3], acc[nt], 0, 0, 0);
      }
      if constexpr (LATE) {
        if (q == 0) {
          // branch-free: without a next step the rows asked for are absent ones (zeros from the range check, never
          // committed), and the index loads repeat offset k's
          if (nk < 0) {
#pragma unroll
            for (int it = 0; it < NIT; it++) idx[it] = -1;
          }
          issue_data(nk >= 0 ? nct : 0);
          load_idx(k2 >= 0 ? k2 : k);
        }
      }
    }
    // order of the step's instruction stream: the gather / index loads up front, then per q-iteration one MFMA,
    // one LDS read (A of the next iteration), one weight load (ring refill QA iterations ahead), the other MFMAs
    if constexpr (!LATE) {
      __builtin_amdgcn_sched_group_barrier(0x020, 2 * NIT, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#pragma unroll
      for (int q = 0; q < NQ; q++) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, NT, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 4 * NT - 1, 0);
      }
    } else {
      // LATE: A of q = 0, its first MFMA, A of q = 1, the ring refill, the other MFMAs of q = 0, THEN the gather and
      // index loads, then the remaining q-iterations as above
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#pragma unroll
      for (int q = 0; q < NQ; q++) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, NT, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 4 * NT - 1, 0);
        if (q == 0) __builtin_amdgcn_sched_group_barrier(0x020, 2 * NIT, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    block_sync();
    k = nk;
    ct = nct;
  }
  // ---- epilogue: C/D layout col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5) ----
  if (n_split > 1) {
    float *pt = partial + ((size_t)by * npos + (size_t)blk * 32) * COUT;
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
      const int row_in = (reg & 3) + 8 * (reg >> 2) + 4 * h;
#pragma unroll
      for (int nt = 0; nt < NT; nt++) pt[(size_t)row_in * COUT + colbase + nt * 32 + r] = acc[nt][reg];
    }
    return;
  }
  // four rows at a time: residual reads first (a padded row reads row 0 and is dropped), then adds and stores --
  // no load waits for another, and the epilogue does not set the kernel's register budget
  // `stat`: column sums and sums of squares (fp64) of the block's real rows, as they are stored -- the statistics of the
  // BatchNorm that follows are then a fixed-order sum of n_blk small vectors instead of a second pass over the tensor
  double cs[NT], css[NT];
#pragma unroll
  for (int nt = 0; nt < NT; nt++) cs[nt] = css[nt] = 0.0;
#pragma unroll
  for (int g4 = 0; g4 < 4; g4++) {
    int orow[4];
    float res[4][NT];
#pragma unroll
    for (int j = 0; j < 4; j++) orow[j] = __shfl(rowid, j + 8 * g4 + 4 * h, 64);
    if (residual) {
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
          res[j][nt] = residual[(size_t)(orow[j] < 0 ? 0 : orow[j]) * COUT + colbase + nt * 32 + r];
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[nt][g4 * 4 + j] += res[j][nt];
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (orow[j] < 0) continue;
#pragma unroll
      for (int nt = 0; nt < NT; nt++) out[(size_t)orow[j] * COUT + colbase + nt * 32 + r] = acc[nt][g4 * 4 + j];
      if (stat) {
#pragma unroll
        for (int nt = 0; nt < NT; nt++) {
          const double d = (double)acc[nt][g4 * 4 + j];
          cs[nt] += d;
          css[nt] += d * d;
        }
      }
    }
  }
  if (stat) {   // rows 0-3, 8-11, .. live in lanes 0-31, the others in lanes 32-63: both halves form the same sum
    double *sp = stat + (size_t)blk * (2 * COUT);
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
      const double a = cs[nt] + __shfl_xor(cs[nt], 32, 64), b = css[nt] + __shfl_xor(css[nt], 32, 64);
      if (h == 0) {
        sp[colbase + nt * 32 + r] = a;
        sp[COUT + colbase + nt * 32 + r] = b;
      }
    }
  }
