// Rooms from boxes (include/d3d_hip.h, d3d_floorplan_*): a plan of square cells in which the selected boxes block the
// cells whose centre they hold, the 4-connected components of the free cells as rooms, what lies on either side of a
// box, and the room of every point.  Everything is defined on the fp64 box table (xc, yc, cos, sin, hx, hy) the caller
// hands in, with every product and sum rounded on its own (-ffp-contract=off), so that numpy restates it bit for bit.
//
// Raster: box-major.  A workgroup takes kRasterRows rows of one box's clipped bounding cells, a wave a row at a time, 64
// cells per step aligned to two bitmap words; a ballot is the two words, and a word whose bits are all set already is
// not written again.  A floor-sized box is spread over ceil(H / kRasterRows) workgroups.
//
// Labelling works on the runs of free bits of a row.  k_fp_runs gives every free cell the first cell of its run as its
// parent (one wave per row, a max-scan of the last blocked column over the row's words); k_fp_links unites, through the
// lock-free union-find of union_find.inc, every run with the runs of the row above that it overlaps -- one unite per
// overlap, at the overlap's first column, found with word arithmetic.  Hooking puts the higher root under the lower,
// and a run's first cell is its smallest, so a component's root is its smallest cell id.  k_fp_roots then writes every
// cell's root and sums per root the cell count and the border flag into one word (integer add and or; a wave first
// gathers the lanes that share a root), the room roots are ranked in cell order by the library's exclusive scan, and
// k_fp_write turns roots into labels and takes the rooms' bounds with integer min / max, per wave and room, and only
// where the wave's extent lies outside the bounds read so far.  Nothing waits for another thread's store.
#include <algorithm>
#include <cmath>

#include "grid_internal.h"

namespace d3d {
namespace {

#include "union_find.inc"

constexpr int kMaxSide = 4096;
constexpr int kMaxBoxes = 4096;
constexpr int kRasterRows = 32;
constexpr int32_t kOutside = -1, kBlocked = -2, kSmall = -3, kNone = -4;
constexpr int32_t kBorderBit = 1 << 30;          // of a root's info word; the cell count (<= 2^24) lies below it
constexpr int32_t kCountMask = kBorderBit - 1;

// the cell along one axis of a coordinate, -1 off the lattice (a NaN included)
__device__ __forceinline__ int fp_cell(double x, double o, double cell, int n) {
  const double f = floor((x - o) / cell);
  return (f >= 0.0 && f < (double)n) ? (int)f : -1;
}

__global__ __launch_bounds__(256) void k_fp_raster(const double *__restrict__ table, const uint8_t *__restrict__ select,
                                                   double cell, double ox, double oy, int h, int w, int nw,
                                                   uint32_t *bitmap) {
  const int b = blockIdx.y;
  if (select && !select[b]) return;
  const double *t = table + (size_t)b * 6;
  const double xc = t[0], yc = t[1], c = t[2], s = t[3], hx = t[4], hy = t[5];
  if (!(isfinite(xc) && isfinite(yc) && isfinite(c) && isfinite(s) && isfinite(hx) && isfinite(hy))) return;
  // the cells that can pass the test: the box's bounding rectangle, a cell and the rounding of the test wider
  const double ex = fabs(c) * hx + fabs(s) * hy, ey = fabs(s) * hx + fabs(c) * hy;
  const double pad = cell + 1e-9 * (fabs(xc) + fabs(yc) + fabs(ox) + fabs(oy) + fabs(ex) + fabs(ey));
  const double fx0 = floor((xc - ex - pad - ox) / cell), fx1 = floor((xc + ex + pad - ox) / cell);
  const double fy0 = floor((yc - ey - pad - oy) / cell), fy1 = floor((yc + ey + pad - oy) / cell);
  if (!(fx1 >= 0.0 && fy1 >= 0.0 && fx0 <= (double)(w - 1) && fy0 <= (double)(h - 1))) return;
  const int ix0 = (int)fmax(fx0, 0.0), ix1 = (int)fmin(fx1, (double)(w - 1));
  const int iy0 = (int)fmax(fy0, 0.0), iy1 = (int)fmin(fy1, (double)(h - 1));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long first = (long)iy0 + (long)blockIdx.x * kRasterRows;
  for (int r = wave; r < kRasterRows; r += 4) {
    const long iy = first + r;
    if (iy > iy1) break;
    const double Y = oy + ((double)iy + 0.5) * cell, dy = Y - yc;
    uint32_t *row = bitmap + (size_t)iy * nw;
    for (int base = ix0 & ~63; base <= ix1; base += 64) {
      const int ix = base + lane;
      bool in = false;
      if (ix >= ix0 && ix <= ix1) {
        const double X = ox + ((double)ix + 0.5) * cell, dx = X - xc;
        const double lx = c * dx - s * dy, ly = s * dx + c * dy;
        in = fabs(lx) <= hx && fabs(ly) <= hy;
      }
      const unsigned long long m = __ballot(in);
      if (lane < 2) {
        const uint32_t bits = (uint32_t)(m >> (32 * lane));
        const int wi = (base >> 5) + lane;            // bits != 0 only for columns < w, so wi < nw
        if (bits && (__hip_atomic_load(row + wi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bits) != bits)
          atomicOr(row + wi, bits);
      }
    }
  }
}

// word wi of a bitmap row with the columns from w on counted as blocked
__device__ __forceinline__ uint32_t fp_word(const uint32_t *__restrict__ row, int wi, int nw, int w) {
  uint32_t v = row[wi];
  if (wi == nw - 1 && (w & 31)) v |= ~0u << (w & 31);
  return v;
}

__device__ __forceinline__ int wave_max_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(v, d, 64);
    if (lane >= d) v = max(v, t);
  }
  return v;
}

// par[cell] = the first cell of its run of free cells; a blocked cell is its own parent and is never united.  One wave
// per row: lane l holds words l and l + 64 (W <= 4096) and the column at which the run that enters each word began.
__global__ __launch_bounds__(256) void k_fp_runs(const uint32_t *__restrict__ bitmap, int h, int w, int nw,
                                                 int32_t *__restrict__ par) {
  const int lane = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (y >= h) return;                                  // the whole wave
  const uint32_t *row = bitmap + (size_t)y * nw;
  uint32_t wd[2];
  int last[2];
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const int wi = lane + 64 * q;
    wd[q] = wi < nw ? fp_word(row, wi, nw, w) : ~0u;
    last[q] = wd[q] ? 32 * wi + 31 - __clz((int)wd[q]) : -1;      // the word's last blocked column
  }
  const int inc0 = wave_max_scan(last[0], lane);
  const int tot0 = __shfl(inc0, 63, 64);
  const int inc1 = max(wave_max_scan(last[1], lane), tot0);
  int ex0 = __shfl_up(inc0, 1, 64), ex1 = __shfl_up(inc1, 1, 64);
  if (lane == 0) ex0 = -1, ex1 = tot0;
  const int carry0 = ex0 + 1, carry1 = ex1 + 1;
  const int rowbase = y * w;
  for (int base = 0; base < w; base += 64) {
    const int col = base + lane, wi = col >> 5, src = wi & 63;
    const bool upper = (base >> 11) != 0;              // words 64 .. 127: uniform over the wave
    const uint32_t word = (uint32_t)__shfl((int)(upper ? wd[1] : wd[0]), src, 64);
    const int carry = __shfl(upper ? carry1 : carry0, src, 64);
    if (col < w) {
      const int b = col & 31;
      const uint32_t below = word & ((1u << b) - 1u);
      const int start = below ? (wi << 5) + 32 - __clz((int)below) : carry;
      par[rowbase + col] = ((word >> b) & 1u) ? rowbase + col : rowbase + start;
    }
  }
}

// one unite per overlap of a run with a run of the row above, at the overlap's first column
__global__ __launch_bounds__(256) void k_fp_links(const uint32_t *__restrict__ bitmap, int h, int w, int nw,
                                                  int32_t *par) {
  const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (long)(h - 1) * nw) return;
  const int y = 1 + (int)(k / nw), wi = (int)(k % nw);
  const uint32_t *r1 = bitmap + (size_t)y * nw, *r0 = r1 - nw;
  const uint32_t both = ~fp_word(r1, wi, nw, w) & ~fp_word(r0, wi, nw, w);
  const uint32_t prev = wi > 0 ? (~fp_word(r1, wi - 1, nw, w) & ~fp_word(r0, wi - 1, nw, w)) >> 31 : 0u;
  uint32_t link = both & ~((both << 1) | prev);
  while (link) {
    const int b = __ffs((int)link) - 1;
    link &= link - 1u;
    const int id = y * w + (wi << 5) + b;
    uf_unite(par, id, id - w);
  }
}

// label[cell] = its root (kBlocked for a blocked cell); info[root] += the cells, |= kBorderBit for a cell of the
// lattice's border.  par is only read.
__global__ __launch_bounds__(256) void k_fp_roots(const uint32_t *__restrict__ bitmap, const int32_t *__restrict__ par,
                                                  int h, int w, int nw, int32_t *__restrict__ label, int32_t *info) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool active = false, border = false;
  int r = -1;
  if (id < (long)h * w) {
    const int y = (int)(id / w), x = (int)(id % w);
    active = !((bitmap[(size_t)y * nw + (x >> 5)] >> (x & 31)) & 1u);
    if (active) {
      border = y == 0 || x == 0 || y == h - 1 || x == w - 1;
      r = (int)id;
      while (true) {
        const int p = par[r];
        if (p == r) break;
        r = p;
      }
    }
    label[id] = active ? r : kBlocked;
  }
  unsigned long long todo = __ballot(active);
  while (todo) {                      // uniform over the wave; every round retires at least its leader
    const int leader = __ffsll((long long)todo) - 1;
    const int lr = __shfl(r, leader, 64);
    const bool same = active && r == lr;
    const unsigned long long m = __ballot(same);
    const unsigned long long mb = __ballot(same && border);
    if (lane == leader) {
      atomicAdd(info + lr, __popcll(m));
      if (mb && !(__hip_atomic_load(info + lr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kBorderBit))
        atomicOr(info + lr, kBorderBit);
    }
    todo &= ~m;
    active = active && !same;
  }
}

// flag[cell] = 1 for the root of a room: not outside and not small
__global__ void k_fp_flags(const int32_t *__restrict__ label, const int32_t *__restrict__ info, long n, int min_cells,
                           int32_t *__restrict__ flag) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n) return;
  const int32_t v = info[id];
  flag[id] = label[id] == (int32_t)id && !(v & kBorderBit) && (v & kCountMask) >= min_cells;
}

__global__ void k_fp_tables(int max_rooms, int h, int w, int32_t *cells, int32_t *bounds, int32_t *seed) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= max_rooms) return;
  cells[i] = 0;
  seed[i] = -1;
  bounds[4 * i + 0] = w, bounds[4 * i + 1] = h, bounds[4 * i + 2] = -1, bounds[4 * i + 3] = -1;
}

__device__ __forceinline__ int32_t fp_peek(const int32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// roots -> labels, and the tables of the rooms below max_rooms
__global__ __launch_bounds__(256) void k_fp_write(const int32_t *__restrict__ info, const int32_t *__restrict__ rank,
                                                  int h, int w, int min_cells, int max_rooms, int32_t *label,
                                                  int32_t *cells, int32_t *bounds, int32_t *seed) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool active = false;
  int room = -1, x = 0, y = 0;
  if (id < (long)h * w) {
    const int r = label[id];
    if (r >= 0) {
      const int32_t v = info[r];
      const int n = v & kCountMask;
      room = (v & kBorderBit) ? kOutside : n < min_cells ? kSmall : rank[r];
      label[id] = room;
      active = room >= 0 && room < max_rooms;
      if (active && r == (int)id) cells[room] = n, seed[room] = r;
      y = (int)(id / w), x = (int)(id % w);
    }
  }
  unsigned long long todo = __ballot(active);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int lr = __shfl(room, leader, 64);
    const bool same = active && room == lr;
    const unsigned long long m = __ballot(same);
    int x0 = same ? x : 0x7fffffff, y0 = same ? y : 0x7fffffff, x1 = same ? x : -1, y1 = same ? y : -1;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      x0 = min(x0, __shfl_xor(x0, s, 64)), y0 = min(y0, __shfl_xor(y0, s, 64));
      x1 = max(x1, __shfl_xor(x1, s, 64)), y1 = max(y1, __shfl_xor(y1, s, 64));
    }
    if (lane == leader) {       // a bound only ever tightens: a stale read costs an atomic that changes nothing, never one
      int32_t *bd = bounds + 4 * (size_t)lr;
      if (x0 < fp_peek(bd + 0)) atomicMin(bd + 0, x0);
      if (y0 < fp_peek(bd + 1)) atomicMin(bd + 1, y0);
      if (x1 > fp_peek(bd + 2)) atomicMax(bd + 2, x1);
      if (y1 > fp_peek(bd + 3)) atomicMax(bd + 3, y1);
    }
    todo &= ~m;
    active = active && !same;
  }
}

// thread 2 j + e: side e (0: -lx, 1: +lx) of box j
__global__ void k_fp_sides(const double *__restrict__ table, int k, const int32_t *__restrict__ label, double cell,
                           double ox, double oy, int h, int w, int n_probe, int32_t *__restrict__ sides) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * k) return;
  const double *t = table + (size_t)(i >> 1) * 6;
  const double xc = t[0], yc = t[1], c = t[2], s = t[3], hx = t[4];
  int32_t out = kNone;
  for (int p = 0; p < n_probe; p++) {
    const double d = hx + ((double)p + 0.5) * cell, tt = (i & 1) ? d : -d;
    const double px = xc + c * tt, py = yc - s * tt;
    const int ix = fp_cell(px, ox, cell, w), iy = fp_cell(py, oy, cell, h);
    if (ix < 0 || iy < 0) {
      out = kOutside;
      break;
    }
    const int32_t v = label[(size_t)iy * w + ix];
    if (v != kBlocked) {
      out = v;
      break;
    }
  }
  sides[i] = out;
}

__global__ void k_fp_points(const float *__restrict__ xyz, int n, int stride, const double *__restrict__ origin,
                            const int32_t *__restrict__ label, double cell, double ox, double oy, int h, int w,
                            int32_t *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float *p = xyz + (size_t)i * stride;
  double x = (double)p[0], y = (double)p[1], z = (double)p[2];
  if (origin) x -= origin[0], y -= origin[1], z -= origin[2];
  int32_t v = kNone;
  if (isfinite(x) && isfinite(y) && isfinite(z)) {
    const int ix = fp_cell(x, ox, cell, w), iy = fp_cell(y, oy, cell, h);
    v = (ix < 0 || iy < 0) ? kOutside : label[(size_t)iy * w + ix];
  }
  out[i] = v;
}

struct Layout {
  int32_t *par = nullptr;    // [H W] union-find parents; the room-root flags once the roots are written
  int32_t *info = nullptr;   // [H W] per root: cell count | kBorderBit
  int32_t *rank = nullptr;   // [H W] exclusive scan of the flags
  char *scan = nullptr;      // the scan's tile sums
  size_t scan_bytes = 0;
};

int carve(Arena &A, int h, int w, Layout &L) {
  const size_t n = (size_t)h * w;
  D3D_ALLOC(par, int32_t, A, n);
  D3D_ALLOC(info, int32_t, A, n);
  D3D_ALLOC(rank, int32_t, A, n);
  L.scan_bytes = ((n + kScanTile - 1) / kScanTile) * sizeof(int32_t) + 256;
  D3D_ALLOC(scan, char, A, L.scan_bytes);
  L.par = par, L.info = info, L.rank = rank, L.scan = scan;
  return D3D_OK;
}

bool lattice_ok(double cell, double ox, double oy, int h, int w) {
  return cell > 0.0 && std::isfinite(cell) && std::isfinite(ox) && std::isfinite(oy) && h >= 1 && w >= 1 &&
         h <= kMaxSide && w <= kMaxSide;
}

}  // namespace
}  // namespace d3d

using namespace d3d;

size_t d3d_floorplan_scratch_bytes(int h, int w, int k) {
  (void)k;                              // the raster and the sides need no scratch
  Arena A = sizing_arena();
  Layout L;
  (void)carve(A, std::min(std::max(h, 1), kMaxSide), std::min(std::max(w, 1), kMaxSide), L);
  return A.used;
}

int d3d_floorplan_raster(const double *table, const uint8_t *select, int k, double cell, double ox, double oy, int h,
                         int w, uint32_t *bitmap, void *stream) {
  D3D_REQUIRE(k >= 0 && k <= kMaxBoxes, "d3d_floorplan_raster: %d boxes, 0 .. %d", k, kMaxBoxes);
  D3D_REQUIRE(lattice_ok(cell, ox, oy, h, w), "d3d_floorplan_raster: lattice %d x %d, cell %g, origin (%g, %g)", h, w,
              cell, ox, oy);
  D3D_REQUIRE(bitmap && (k == 0 || table), "d3d_floorplan_raster: null pointer (table, bitmap)");
  hipStream_t s = (hipStream_t)stream;
  const int nw = (w + 31) / 32;
  D3D_HIP_CHECK(hipMemsetAsync(bitmap, 0, (size_t)h * nw * sizeof(uint32_t), s));
  if (k > 0) {
    hipLaunchKernelGGL(k_fp_raster, dim3((unsigned)((h + kRasterRows - 1) / kRasterRows), (unsigned)k), dim3(256), 0, s,
                       table, select, cell, ox, oy, h, w, nw, bitmap);
    D3D_LAUNCH_CHECK();
  }
  return D3D_OK;
}

int d3d_floorplan_rooms(const uint32_t *bitmap, int h, int w, int min_cells, int max_rooms, int32_t *label,
                        int32_t *count, int32_t *cells, int32_t *bounds, int32_t *seed, void *scratch,
                        size_t scratch_bytes, void *stream, float *phase_ms_host) {
  D3D_REQUIRE(h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "d3d_floorplan_rooms: lattice %d x %d, 1 .. %d", h, w,
              kMaxSide);
  D3D_REQUIRE(min_cells >= 1 && max_rooms >= 0, "d3d_floorplan_rooms: min_cells %d < 1 or max_rooms %d < 0", min_cells,
              max_rooms);
  D3D_REQUIRE(bitmap && label && count && scratch, "d3d_floorplan_rooms: null pointer (bitmap, label, count, scratch)");
  D3D_REQUIRE(max_rooms == 0 || (cells && bounds && seed), "d3d_floorplan_rooms: null pointer (cells, bounds, seed)");
  D3D_REQUIRE(scratch_bytes >= d3d_floorplan_scratch_bytes(h, w, 0), "d3d_floorplan_rooms: scratch too small");
  hipStream_t s = (hipStream_t)stream;
  Arena A = scratch_arena(scratch, scratch_bytes);
  Layout L;
  if (int rc = carve(A, h, w, L)) return rc;
  const int nw = (w + 31) / 32;
  const long n = (long)h * w;
  Timer T;
  if (int rc = T.start(phase_ms_host != nullptr, 6)) return rc;
  if (int rc = T.mark(0, s)) return rc;
  hipLaunchKernelGGL(k_fp_runs, dim3((unsigned)((h + 3) / 4)), dim3(256), 0, s, bitmap, h, w, nw, L.par);
  if (int rc = T.mark(1, s)) return rc;
  if (h > 1) hipLaunchKernelGGL(k_fp_links, grid1d((long)(h - 1) * nw), dim3(256), 0, s, bitmap, h, w, nw, L.par);
  if (int rc = T.mark(2, s)) return rc;
  D3D_HIP_CHECK(hipMemsetAsync(L.info, 0, (size_t)n * sizeof(int32_t), s));
  hipLaunchKernelGGL(k_fp_roots, grid1d(n), dim3(256), 0, s, bitmap, L.par, h, w, nw, label, L.info);
  if (int rc = T.mark(3, s)) return rc;
  int32_t *flag = L.par;                // the parents are done with
  hipLaunchKernelGGL(k_fp_flags, grid1d(n), dim3(256), 0, s, label, L.info, n, min_cells, flag);
  Arena S = scratch_arena(L.scan, L.scan_bytes);
  if (int rc = scan_exclusive_i32(flag, L.rank, (int)n, count, S, s)) return rc;
  if (int rc = T.mark(4, s)) return rc;
  if (max_rooms > 0) hipLaunchKernelGGL(k_fp_tables, grid1d(max_rooms), dim3(256), 0, s, max_rooms, h, w, cells, bounds, seed);
  hipLaunchKernelGGL(k_fp_write, grid1d(n), dim3(256), 0, s, L.info, L.rank, h, w, min_cells, max_rooms, label, cells,
                     bounds, seed);
  if (int rc = T.mark(5, s)) return rc;
  D3D_LAUNCH_CHECK();
  return T.finish(phase_ms_host);
}

int d3d_floorplan_sides(const double *table, int k, const int32_t *label, double cell, double ox, double oy, int h,
                        int w, int n_probe, int32_t *sides, void *stream) {
  D3D_REQUIRE(k >= 0 && k <= kMaxBoxes, "d3d_floorplan_sides: %d boxes, 0 .. %d", k, kMaxBoxes);
  D3D_REQUIRE(lattice_ok(cell, ox, oy, h, w), "d3d_floorplan_sides: lattice %d x %d, cell %g, origin (%g, %g)", h, w,
              cell, ox, oy);
  D3D_REQUIRE(n_probe >= 0, "d3d_floorplan_sides: %d probes", n_probe);
  if (k == 0) return D3D_OK;
  D3D_REQUIRE(table && label && sides, "d3d_floorplan_sides: null pointer (table, label, sides)");
  hipLaunchKernelGGL(k_fp_sides, grid1d(2L * k), dim3(256), 0, (hipStream_t)stream, table, k, label, cell, ox, oy, h, w,
                     n_probe, sides);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}

int d3d_floorplan_points(const float *xyz, int n, int row_stride_floats, const double *origin_dev, const int32_t *label,
                         double cell, double ox, double oy, int h, int w, int32_t *room, void *stream) {
  D3D_REQUIRE(n >= 0, "d3d_floorplan_points: n %d must not be negative", n);
  D3D_REQUIRE(row_stride_floats >= 3, "d3d_floorplan_points: row stride %d < 3 floats", row_stride_floats);
  D3D_REQUIRE(lattice_ok(cell, ox, oy, h, w), "d3d_floorplan_points: lattice %d x %d, cell %g, origin (%g, %g)", h, w,
              cell, ox, oy);
  if (n == 0) return D3D_OK;
  D3D_REQUIRE(xyz && label && room, "d3d_floorplan_points: null pointer (xyz, label, room)");
  hipLaunchKernelGGL(k_fp_points, grid1d(n), dim3(256), 0, (hipStream_t)stream, xyz, n, row_stride_floats, origin_dev,
                     label, cell, ox, oy, h, w, room);
  D3D_LAUNCH_CHECK();
  return D3D_OK;
}
