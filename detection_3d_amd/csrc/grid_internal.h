// What the grid family shares and the rest of the library does not: grid.hip (metadata, input layer), grid_chain.hip
// (strided grids), plan.hip (rulebook plans), geometry_async.hip (the geometry threads), grid_views.hip (dense views),
// scan_sort.hip (scan, radix sort, fills) and voxelize.hip.
#pragma once
#include <algorithm>
#include <vector>

#include "d3d_internal.h"

// Every kernel of the family raises its waves' issue priority: they are short chains of latency-bound steps that share
// the CUs with the convolutions of the caller's stream, whose waves hold priority 1 through their matrix loops
// (conv.hip); at equal or lower priority a geometry wave waited behind them for every instruction it issued.  Measured
// on the 500 k-point building: k_plan_finish 0.48 -> 0.33 ms, k_subm_nbr 0.32 -> 0.23 ms per building, the pass 4.84 -> 4.78 ms.
#ifndef D3D_SIDE_PRIO_LEVEL
#define D3D_SIDE_PRIO_LEVEL 3
#endif
#define D3D_SIDE_PRIO() __builtin_amdgcn_s_setprio(D3D_SIDE_PRIO_LEVEL)

namespace d3d {

// scan_sort.hip ---------------------------------------------------------------------------
static constexpr int kScanThreads = 256;
static constexpr int kScanItems = 8;
static constexpr int kScanTile = kScanThreads * kScanItems;   // elements per partial sum scan_exclusive_i32 allocates
// passes and digit bits of a sort_pairs_u32 over `bits` key bits
static inline void rs_layout(int bits, int &passes, int &db) {
  passes = std::max(1, (bits + 9) / 10);
  db = std::min(10, std::max(8, (bits + passes - 1) / passes));
}
hipError_t fill_ones(void *ptr, size_t bytes, hipStream_t s);   // 0xFF fill of hash tables and rulebook arrays

// grid.hip --------------------------------------------------------------------------------
Grid *find_grid(d3d_meta *m, const int *size);
static inline int next_pow2(long v) {
  long c = 1024;
  while (c < v) c <<= 1;
  return (int)c;
}

// grid_chain.hip --------------------------------------------------------------------------
struct ChainSpec {              // one strided rulebook: sizes as d3d_conv_prepare takes them
  int in_size[3], out_size[3], filt[3], stride[3];
  int need_dec;                 // keep the decoded table (deconvolution / backward view will be asked for)
};
typedef void (*ChainHook)(void *arg, int level, int n_out, hipStream_t s);   // level published / level's rulebook enqueued
int run_grid_chain(d3d_meta *m, const std::vector<ChainSpec> &specs, hipStream_t s, std::vector<int> &n_out,
                   ChainHook on_grid, ChainHook on_done, void *hook_arg);

// plan.hip --------------------------------------------------------------------------------
static inline PlanKey make_key(int kind, const int *in_size, const int *filt, const int *stride) {
  PlanKey k;
  k[0] = kind;
  for (int d = 0; d < 3; d++) {
    k[1 + d] = in_size[d];
    k[4 + d] = filt[d];
    k[7 + d] = stride ? stride[d] : 0;
  }
  return k;
}
// the neighbour table of a submanifold rulebook (see launch_subm_nbr): whether the half-probe form serves, the two
// fills it needs, and the probes themselves
bool subm_nbr_is_sym(int n_bound, const int *filt);
int subm_nbr_prefill(int n_bound, const int *filt, int32_t *nbr, uint32_t *mask, hipStream_t s);
int launch_subm_nbr(const int32_t *loc, int n_bound, const int *filt, const HashEntry *tab, int cap, int32_t *nbr,
                    uint32_t *mask, const int32_t *n_dev, hipStream_t s, bool sym, bool prefilled = false);
// k_plan_finish over npos positions; n_dev (may be null): the row count on the device, n_rows / npos then upper bounds
void launch_plan_finish(const int32_t *nbr, int32_t *rows, int n_rows, int npos, int K, int32_t *nbrT, uint32_t *blkmask,
                        const int32_t *n_dev, hipStream_t s);
// d3d_plan_last_form's record, and what the caller of finalize_plan did before it (probe, grid): consumed by the record
void plan_record(int family, int masks, int probe, int K, int n_rows, int n_bound, int n_blk, int passes, int db, int grid);
extern thread_local int t_plan_ctx[2];

// geometry_async.hip ----------------------------------------------------------------------
void geo_async_join(d3d_meta *m);   // waits until both workers have finished the chain that was started
void geo_async_free(d3d_meta *m);

}  // namespace d3d
