/*
 * d3d_hip.h -- C ABI of libd3d_hip.so, the MI355X (gfx950) implementation of the hot path of
 * zhupan007/Detection_3D:  points -> voxel hash-scatter -> sparse-3D-conv rulebooks +
 * gather-GEMM-scatter -> rotated IoU / NMS -> rotated 3-D RoIAlign.
 *
 * Conventions
 *  - every pointer argument is a DEVICE pointer unless its name ends in _host;
 *  - every function takes the hipStream_t to enqueue on (passed as void* so that this header
 *    needs no HIP include) and returns 0 on success or a negative d3d_status; it never throws.
 *    d3d_last_error() returns a thread-local message for the last failure;
 *  - functions that must tell the host a size (number of active sites ...) synchronise the
 *    stream once; all others are asynchronous;
 *  - feature matrices are row-major fp32 [rows, planes]; coordinates int64 [n, 3|4] (x,y,z[,b]).
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference
 * repository root; SCN = SparseConvNet/sparseconvnet/SCN).
 */
#ifndef D3D_HIP_H
#define D3D_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  D3D_OK = 0,
  D3D_ERR_ARG = -1,      /* bad argument (shape, null pointer, unsupported mode) */
  D3D_ERR_HIP = -2,      /* a HIP runtime call failed */
  D3D_ERR_NOMEM = -3,    /* metadata arena exhausted */
  D3D_ERR_STATE = -4,    /* grid / rulebook not built (call order) */
  D3D_ERR_UNSUPPORTED = -5
} d3d_status;

const char *d3d_last_error(void);
int d3d_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Metadata: replaces class sparseconvnet.SCN.Metadata_3 (SCN/pybind.cpp:12-32,
 * SCN/Metadata/Metadata.h:36-130).  Owns the per-scale hash grids and the lazily built,
 * cached rulebooks ("plans"), all resident in one HBM arena of `arena_bytes`.
 * Not re-entrant per object (same as the reference: lazy cache mutation).                  */
typedef struct d3d_meta d3d_meta;
int d3d_meta_create(d3d_meta **out, size_t arena_bytes);
int d3d_meta_destroy(d3d_meta *m);
int d3d_meta_clear(d3d_meta *m);                       /* Metadata::clear, Metadata.cpp:30-45 */
int d3d_meta_arena_used(d3d_meta *m, size_t *bytes_host);
/* Two-lane building (no reference counterpart; the reference builds rulebooks on the CPU inside each layer's forward,
 * Metadata.cpp:430-510).  enable != 0: new grids + strided rulebooks (d3d_conv_prepare) may only be BUILT on `stream`
 * from now on (requested on another stream they fail with D3D_ERR_STATE instead of racing), and everything any other
 * stream builds or stages (submanifold / deconvolution rulebooks, partial tiles) comes from a separate third of the
 * slab -- so the caller may run the grid chain of the coarser levels, with its count read-backs, on `stream` while the
 * convolutions of the finer levels run on another one.  The caller orders the two streams with events.  Reset by
 * d3d_meta_clear.                                                                                                    */
int d3d_meta_set_geometry_stream(d3d_meta *m, void *stream, int enable);
/* Measurement / A-B switch of the fp32 sparse convolutions: 0 (default) = every launch through k_conv; 1 = the large
 * launches of the 64 -> 64 and 128 -> 128 layers through the weight-sharing kernel (conv_ws.hip, measured slower); 2 =
 * those layers' launches of every size (tests).  Same results bit for bit.  mode < 0: query only.  -> the previous setting.
 * Environment: D3D_CONV_WS.                                                                                          */
int d3d_conv_ws_mode(int mode);
/* ... and whether k_conv requests the next step's gathered rows behind the step's first MFMAs (1, default) or ahead of its
 * matrix work (0).  Same results.  on < 0: query only.  -> previous setting.  Environment: D3D_CONV_LATE.              */
int d3d_conv_late_mode(int on);
/* Test hook of every sparse convolution launch (k_conv and the bf16 / bf16x3 kernel, process-wide): 0 (default) =
 * offset-split below the launch's wave target, 1 = never split, 2 = split every launch whose form allows it (one row
 * block per workgroup, filter volume > 1).  Same products, other summation grouping.  mode < 0: query only.
 * -> the previous setting.                                                                                          */
int d3d_conv_split_mode(int mode);
/* The form of the calling thread's most recent sparse convolution launch, recorded on the host: up to n of the ints
 * family (0 none, 1 k_conv, 2 k_conv_ws, 3 bf16, 4 bf16x3), CT, NCT, COUT, BPW, RB, VEC, LATE, n_split, statistics
 * epilogue written (0 / 1), row blocks, filter volume.  The record is cleared by the call (out may be null).
 * -> the number of fields the record has.                                                                            */
int d3d_conv_last_form(int *out, int n);
/* The chain of strided grids run by a thread of the library (no reference counterpart; a caller that builds the levels
 * itself, one d3d_conv_prepare at a time, waits for one blocking read-back of a site count per level, during which it
 * cannot enqueue feature kernels; the thread builds the levels back to back, sized by bounds, with two read-backs).
 * start: `specs` = n x 13 ints (kind, in_size[3], out_size[3], filter[3], stride[3]), built in order:
 *   kind 1: what d3d_conv_prepare builds (a new grid + strided rulebook) on `stream`, which must be the metadata's
 *           geometry stream; kind 3: the same without the decoded table a deconvolution view needs;
 *   kind 0: d3d_subm_prepare(in_size, filter), kind 2: d3d_deconv_prepare -- views of grids that exist by then, enqueued
 *           on `view_stream` (the metadata's plan stream, d3d_meta_set_plan_stream) behind the newest grid.
 * The caller has already ordered `stream` after whatever built the first input grid and must not build on either stream
 * (or touch their lanes of the arena) until finish.
 * wait: blocks until entry `index` is built (enqueued, for views), returns its output site count (kind 1) and makes
 *       `wait_stream` wait for it.
 * finish: joins the thread (d3d_meta_clear / _destroy do so too) and reports its error, if any.                       */
int d3d_geometry_async_start(d3d_meta *m, const int *specs_host, int n, void *stream, void *view_stream);
int d3d_geometry_async_wait(d3d_meta *m, int index, int *n_out_host, void *wait_stream);
int d3d_geometry_async_finish(d3d_meta *m);
/* Third lane (needs a geometry stream): rulebooks that are views of an existing grid -- submanifold, deconvolution --
 * built on `stream` take their memory from a part of the slab of their own (the upper 3/4 of the feature lane, carved
 * once per scene), so that they can be built while the geometry stream works on the next grid and a third stream
 * convolves.  enable == 0 ends the routing; the rulebooks stay valid until d3d_meta_clear.                            */
int d3d_meta_set_plan_stream(d3d_meta *m, void *stream, int enable);

/* The stable radix sort behind the rulebooks' row order and the input layer's point lists (no reference counterpart: the
 * reference keeps rulebooks in insertion order on the CPU, RuleBookIterator.h:15-32), exported so that it can be tested
 * on its own.  Sorts (key, value) pairs by the low `bits` bits of the key, ascending or descending, stably; keys_out
 * may be null.  `scratch`: d3d_sort_scratch_bytes(n, bits) bytes of device memory.                                     */
size_t d3d_sort_scratch_bytes(int n, int bits);
int d3d_sort_pairs(const uint32_t *keys, const int32_t *vals, int n, int bits, int descending, uint32_t *keys_out,
                   int32_t *vals_out, void *scratch, size_t scratch_bytes, void *stream);

/* a1. data3d/suncg_utils/suncg_dataset.py:97-177: a = xyz*scale in fp64, shift by per-axis min,
 * drop points outside [0, full_scale), trunc -> int64; feats[:,0:3] = a/scale.
 * pcl fp32 [n, nfeat] (xyz first).  coords_out int64 [n,3], feats_out fp32 [n,nfeat]
 * (compacted, input order preserved).  Synchronises; *n_kept_host = rows written.
 * x*scale and the shift are two fp64 operations, never one fused multiply-add; columns 3.. are copied bit for bit.
 * Non-finite coordinates: the per-axis minimum is an fmin, which IGNORES a NaN, so a NaN coordinate (like a +Inf one)
 * drops that point only.  This departs from the numpy recipe, whose NaN-propagating min makes the offset NaN and drops
 * the whole cloud (as it does for an Inf, which its product with the diagonal scale matrix turns into a NaN).  A -Inf
 * coordinate is the minimum: the shift becomes +Inf and every point is dropped, as in numpy. */
int d3d_voxelize(const float *pcl, int n, int nfeat, double scale, const int *full_scale_host,
                 int64_t *coords_out, float *feats_out, int *n_kept_host, void *scratch,
                 size_t scratch_bytes, void *stream);
size_t d3d_voxelize_scratch_bytes(int n);

/* Training-time augmentation of one scene, data3d/suncg_utils/suncg_dataset.py:113-149 (hard-wired off in the reference,
 * :78-83).  Points are in voxel units: a = xyz . M, a_j = ((x m[0+j] + y m[3+j]) + z m[6+j]) in fp64 without contraction
 * (m row-major, scale included, :115-122).  nrm: the normals' matrix (row-major, no scale); color: added to the three
 * colour columns in fp64 (:140-142); u1, u2: the origin-offset draws of :127-132, used when origin_offset != 0.
 * color_col / normal_col: first of the three colour / normal columns of the features, -1 when absent.             */
typedef struct d3d_augment_params {
  double m[9];
  double nrm[9];
  double color[3];
  double u1[3];
  double u2[3];
  int origin_offset;
  int color_col;
  int normal_col;
  int reserved;
} d3d_augment_params;
/* d3d_voxelize with the augmentation folded in: a = points (fp64 [n,3], from d3d_augment_transform and
 * d3d_elastic_apply) or xyz . M when points is null; offset = -min(a) (+ the origin offset), :126-133; the bounds filter,
 * trunc and feats[:,0:3] = (a + offset)/scale of d3d_voxelize; colour and normal columns transformed, other columns
 * copied.  Identity parameters (m = diag(scale), nothing else) give d3d_voxelize's bits.  Synchronises once;
 * *n_kept_host = rows written, offset_host[3] = the shift applied (voxel units).  scratch: d3d_augment_scratch_bytes. */
int d3d_augment_voxelize(const float *pcl, int n, int nfeat, const double *points, const d3d_augment_params *prm_host,
                         double scale, const int *full_scale_host, int64_t *coords_out, float *feats_out,
                         int *n_kept_host, double *offset_host, void *scratch, size_t scratch_bytes, void *stream);
size_t d3d_augment_scratch_bytes(int n);
/* a = xyz . M into points_out (fp64 [n,3]) for the elastic passes; minmax_host[6] = per-axis min, then max (the grid of
 * elastic(), :221, needs max |a|) over the finite values only: a NaN or +-Inf coordinate sizes no grid (1e300 / -1e300
 * for an axis without a finite value).  Synchronises once.  scratch: >= 64 bytes.                                      */
int d3d_augment_transform(const float *pcl, int n, int nfeat, const d3d_augment_params *prm_host, double *points_out,
                          double *minmax_host, void *scratch, size_t scratch_bytes, void *stream);
/* elastic(), :223-228: the 3-tap 1/3 box filter along axes 0, 1, 2, 0, 1, 2 of nfields fp32 fields [nfields][d0][d1][d2]
 * (dims_host[3]), zero padded, fp64 sums rounded to fp32 after every pass (scipy.ndimage.convolve, mode 'constant'), in
 * place; tmp: a buffer of the same size.  Asynchronous.                                                               */
int d3d_elastic_blur(float *fields, int nfields, const int *dims_host, float *tmp, void *stream);
/* elastic(), :229-233: points += mag * (3 blurred fields [3][d0][d1][d2] sampled trilinearly in fp64 on the axes
 * linspace(-(d-1) gran, (d-1) gran, d), 0 outside -- RegularGridInterpolator(bounds_error=0, fill_value=0)).
 * A point outside the axes, NaN and +-Inf included, keeps its bits.
 * minmax_host: null (asynchronous) or [6], per-axis min and max of the finite displaced points (synchronises once).
 * scratch: >= 64 bytes.                                                                                              */
int d3d_elastic_apply(double *points, int n, const float *fields, const int *dims_host, double gran, double mag,
                      double *minmax_host, void *scratch, size_t scratch_bytes, void *stream);

/* Point normals for a cloud that has none (data3d/indoor_data_util.py:73-76, add_norm: open3d's hybrid search).  For
 * every point i of xyz (fp32, row i at xyz + i * row_stride_floats, so the xyz columns of an [n, 6] or [n, 9] cloud are
 * read in place): the candidates are all j, i included, with d2 = (dx dx + dy dy) + dz dz <= radius * radius in fp32 from
 * the fp32 offset p_j - p_i; more than max_nn candidates are cut to the max_nn smallest by (d2, j); counts[i] = the
 * number kept.  Fewer than 3, or coincident points: normal (0, 0, 1).  Otherwise the unit eigenvector of the smallest
 * eigenvalue of the kept points' covariance (fp32 sums about the query, fp64 eigen solve), with its component of
 * largest magnitude positive (ties: lowest axis) when viewpoint_host is null, else with n . (v - p_i) >= 0.  The same
 * input gives the same bits.  Asynchronous, no host read-back; scratch: d3d_estimate_normals_scratch_bytes(n, max_nn)
 * bytes, which depend on n alone and not on the cloud's extent.                                                       */
size_t d3d_estimate_normals_scratch_bytes(int n, int max_nn);
int d3d_estimate_normals(const float *xyz, int n, int row_stride_floats, float radius, int max_nn,
                         const float *viewpoint_host /* NULL: canonical sign */, float *normals /* [n,3] */,
                         int32_t *counts /* [n] or NULL */, void *scratch, size_t scratch_bytes, void *stream);
/* The same, timed: phase_ms_host[4] = cell coordinates, sort, cell table, search (events on `stream`).  Synchronises. */
int d3d_estimate_normals_phases(const float *xyz, int n, int row_stride_floats, float radius, int max_nn,
                                const float *viewpoint_host, float *normals, int32_t *counts, void *scratch,
                                size_t scratch_bytes, void *stream, float *phase_ms_host);

/* Cleaning a raw scan before it is voxelised (the reference's users call open3d's remove_radius_outlier,
 * remove_statistical_outlier and a clustering pass on the CPU; restatements that are not pinned against open3d itself).
 * All three read xyz as d3d_estimate_normals does (fp32, row i at xyz + i * row_stride_floats), use its cell list and
 * its distances: d2 = (dx dx + dy dy) + dz dz in fp32 from the fp32 offset p_j - p_i, "within radius" iff d2 <= radius *
 * radius (fp32 product) by comparison of the bits, the point itself included.  0 <= n <= 2^28.  Asynchronous on `stream`,
 * no host read-back, no float atomics, every sum in an order fixed by the data: the same input gives the same bits.
 * scratch: the matching _scratch_bytes(n), linear in n and independent of the extent.  phase_ms_host: NULL, or [5] =
 * milliseconds of the cell coordinates, the sorts, the cell table, the search and what follows it (events on `stream`;
 * the call then synchronises).
 *
 * d3d_radius_neighbors: count[i] = the points within radius of point i (int32 [n], >= 1).                             */
size_t d3d_radius_neighbors_scratch_bytes(int n);
int d3d_radius_neighbors(const float *xyz, int n, int row_stride_floats, float radius, int32_t *count, void *scratch,
                         size_t scratch_bytes, void *stream, float *phase_ms_host);
/* d3d_knn_mean_distance: the candidates within radius are cut to the k + 1 smallest by (d2, j), the point itself (d2 = 0)
 * among them; found[i] = the kept candidates - 1 (int32 [n]); mean[i] = (sum of sqrt(double(d2)) over the kept) / k in
 * fp64 [n], or +inf for a sparse point (found < k).  stats (device, 2 doubles) = the mean of the finite mean[i] and the
 * square root of their summed squared deviations / (count - 1): per block of 1024 rows the count, the sum and the squared
 * deviations about the block's own mean, then one block adds the partials in block order (no finite value: (0, 0); one:
 * deviation 0).  keep (uint8 [n] or NULL): 1 iff the point is not sparse and mean[i] <= stats[0] + std_ratio * stats[1].
 * k >= 1.  n == 0 zeroes stats.                                                                                        */
size_t d3d_knn_mean_distance_scratch_bytes(int n);
int d3d_knn_mean_distance(const float *xyz, int n, int row_stride_floats, float radius, int k, double std_ratio,
                          double *mean, int32_t *found, double *stats, uint8_t *keep, void *scratch,
                          size_t scratch_bytes, void *stream, float *phase_ms_host);
/* d3d_connected_components: the components of the graph whose edges join the points within radius of one another.
 * label[i] = the smallest row index of i's component, size[i] = its number of points (int32 [n] each).  A lock-free
 * union-find over the points in cell order (hooking by compare-and-swap on roots, the lower id wins; path halving), a
 * flatten pass, then integer min and add per root: integers, so the order of arrival does not show.                   */
size_t d3d_connected_components_scratch_bytes(int n);
int d3d_connected_components(const float *xyz, int n, int row_stride_floats, float radius, int32_t *label, int32_t *size,
                             void *scratch, size_t scratch_bytes, void *stream, float *phase_ms_host);

/* Planar patches of a cloud that carries normals, and the plane of every patch: what lies between "a cloud with normals"
 * and "an instance id per point" for the planar classes.  Pairwise region growing, not RANSAC: a smoothly curved surface
 * chains into one patch, and the points on the crease between two planes carry mixed normals and fall into small patches.
 *
 * d3d_segment_planes: d3d_connected_components with a narrower edge.  xyz, n, radius, scratch, phase_ms_host[5] as there;
 * normals fp32 [n, 3] contiguous.  Points P and C are joined iff all three hold, d = C - P, everything in fp32 without
 * contraction:
 *   (dx dx + dy dy) + dz dz <= radius * radius, by comparison of the bits;
 *   |(nPx nCx + nPy nCy) + nPz nCz| >= cos_min (the caller rounds cos(angle) from fp64 once; a normal's sign is free);
 *   |(nPx dx + nPy dy) + nPz dz| <= offset and |(nCx dx + nCy dy) + nCz dz| <= offset.
 * Each test is bitwise symmetric in P and C (products commute, d negates exactly, the absolute values are equal), so the
 * components are those of an undirected graph.  Each is a "passes if": a zero or non-finite normal and a NaN position
 * fail it and leave the point a patch of its own.  label[i] = the smallest row index of i's patch, size[i] = its number
 * of points.  0 <= cos_min <= 1, 0 <= offset < inf.  The same input gives the same bits.                               */
size_t d3d_segment_planes_scratch_bytes(int n);
int d3d_segment_planes(const float *xyz, int n, int row_stride_floats, const float *normals, float radius, float cos_min,
                       float offset, int32_t *label, int32_t *size, void *scratch, size_t scratch_bytes, void *stream,
                       float *phase_ms_host);
/* d3d_fit_planes: the least-squares plane of every patch.  plane_of_point int32 [n]: the plane of every row in [0, k), or
 * -1; the caller lists the rows by (plane, row) as for d3d_fit_boxes: order int32 [n], offsets int32 [k + 1]; a listed row
 * whose plane_of_point is not the list's plane is skipped.  Per plane, in fp64: the origin o is its first listed row;
 * q = p - o; the count m, sum q and sum q q^T are taken over chunks of 1024 listed rows (thread t of 256 adds rows t,
 * t + 256, ... of the chunk, the lanes are added pairwise, the waves in order), then over the chunks in order: no float
 * atomics, the same input gives the same bits.  centroid = o + sum q / m; C = sum q q^T / m - mean mean^T; normal = the
 * unit eigenvector of C's smallest eigenvalue (cyclic Jacobi, as d3d_estimate_normals), its component of largest
 * magnitude positive (ties: lowest axis); d = (nx cx + ny cy) + nz cz; eigenvalues ascending: the normal's Rayleigh
 * quotient and the two of C restricted to the plane across it; rms = sqrt(max(smallest, 0)).  A plane whose largest
 * eigenvalue is not positive (one point, coincident points): normal, d, rms and eigenvalues 0.  A plane without rows:
 * count 0 and zeros.  Outputs fp64: normal [k, 3], d [k], centroid [k, 3], rms [k], eigenvalues [k, 3]; count int32 [k].
 * 0 <= k <= 4096 (k == 0 touches nothing), 0 <= n <= 2^28; scratch of d3d_fit_planes_scratch_bytes(n, k) bytes (0 when
 * out of range).  Asynchronous, no read-back.  phase_ms_host (NULL: none): two floats, the milliseconds of the moments
 * and of the solve; the call then synchronises.                                                                        */
size_t d3d_fit_planes_scratch_bytes(int n, int k);
int d3d_fit_planes(const float *xyz, int n, int row_stride_floats, const int32_t *plane_of_point, const int32_t *order,
                   const int32_t *offsets, int k, double *normal, double *d, double *centroid, int32_t *count, double *rms,
                   double *eigenvalues, void *scratch, size_t scratch_bytes, void *stream, float *phase_ms_host);

/* Aligning overlapping scans (the reference's users call open3d's compute_point_cloud_distance and registration_icp on
 * the CPU; restatements that are not pinned against open3d itself).
 *
 * d3d_nearest: for every query row the nearest row of another cloud within radius.  cloud and query are read as
 * d3d_estimate_normals reads xyz (fp32, row i at base + i * stride floats, stride >= 3).  The cloud's cell list is
 * queried by the foreign points: the query's cell is floor((double(q) - min) / h) per axis, the list's own arithmetic,
 * clamped to [-1, 2^20 - 1], and the 27 cells around it are searched.  A cloud row competes with
 * d2 = (dx dx + dy dy) + dz dz, dx = C.x - Q.x, in fp32 without contraction, iff d2 <= radius * radius (fp32 product) by
 * comparison of the bits as unsigned integers; the winner is the minimum of (bits of d2, row), so a tie goes to the lowest
 * row.  index int32 [m]: that row, or -1; dist2 fp32 [m] (or NULL): that d2, or +inf.  A query with a non-finite
 * coordinate gets -1 / +inf; a cloud row with a non-finite coordinate is never a neighbour.  0 <= n, m <= 2^28; n == 0
 * gives -1 / +inf throughout, m == 0 touches nothing.  Asynchronous, no read-back, no atomics: numpy in fp32 reproduces
 * every bit.  scratch: d3d_nearest_scratch_bytes(n, m).  phase_ms_host: NULL, or [5] as d3d_radius_neighbors (the last
 * one 0); the call then synchronises.                                                                                 */
size_t d3d_nearest_scratch_bytes(int n_cloud, int n_query);
int d3d_nearest(const float *cloud, int n, int row_stride_floats, const float *query, int m, int query_stride_floats,
                float radius, int32_t *index, float *dist2, void *scratch, size_t scratch_bytes, void *stream,
                float *phase_ms_host);
/* d3d_icp: up to `iterations` Gauss-Newton steps of ICP from the pose in pose_inout_dev (device, 16 doubles, row-major
 * 4 x 4; x' = R x + t maps source into the target's frame; the last row is carried along untouched), without a host
 * read-back in between.  The target's cell list (cells of max_dist) is built once.  Per step and source row, p the row
 * widened to fp64:
 *   p'_k = ((R_k0 x + R_k1 y) + R_k2 z) + t_k; the query is fp32(p'), j = d3d_nearest(query, target, max_dist);
 *   method 0 (point to plane), q = target[j], n = target_normals[j] widened: r = ((p'_0 - q_0) n_0 + (p'_1 - q_1) n_1) +
 *     (p'_2 - q_2) n_2, J = (p' x n, n); a normal that is not finite or is zero contributes nothing;
 *   method 1 (point to point): the residuals p' - q with the rows (-[p']x, I); target_normals may be NULL;
 *   A += J^T J (21 entries, upper triangle by rows), b += J^T r, e += r r, c += 1 per contributing row: 29 fp64 sums, per
 *   block of 4096 rows (thread t of 256 adds rows t, t + 256, ... in order, lanes pairwise, waves in order), then the
 *   blocks in order: no float atomics, the same input gives the same bits.
 * A xi = -b by Cholesky, xi = (w, v).  Degenerate (c < 6, or a pivot <= 1e-12 of A's largest diagonal entry): the pose
 * stays, status 2.  Otherwise dR = Rodrigues(w), R <- dR R, t <- dR t + v; |w| <= tol and |v| <= tol: status 1.  Once
 * the status is non-zero the remaining steps' kernels return at once.
 *   history_dev fp64 [iterations, 20]: one row per executed step: the 16 pose entries after it, c, e, |w|, |v| (0, 0 for a
 *     degenerate step); the other rows are not touched;
 *   state_dev int32 [2] = (steps executed, status 0 running out of iterations / 1 converged / 2 degenerate);
 *   last_index int32 [m] or NULL, last_system fp64 [29] or NULL: j (-1: none) and the 29 sums of the last executed step.
 * 0 <= iterations <= 10000, tol >= 0.  scratch: d3d_icp_scratch_bytes(n, m).  phase_ms_host: NULL, or [7] = milliseconds
 * of the list's cell coordinates, sorts and table, then of the transform, nearest, accumulate and solve kernels summed
 * over the steps; the call then synchronises.                                                                         */
size_t d3d_icp_scratch_bytes(int n_target, int n_source);
int d3d_icp(const float *source, int m, int source_stride_floats, const float *target, int n, int target_stride_floats,
            const float *target_normals, int normal_stride_floats, float max_dist, int method, int iterations, double tol,
            double *pose_inout_dev, double *history_dev, int32_t *state_dev, int32_t *last_index, double *last_system,
            void *scratch, size_t scratch_bytes, void *stream, float *phase_ms_host);

/* The points of each rotated box (Bbox3D.points_in_bbox, utils3d/bbox3d_ops.py:731-755; the counts of split_bbox,
 * data3d/indoor_data_util.py:244-254; the extents of crop_bbox_by_points, bbox3d_ops.py:873-878), without an [n, k] mask.
 * Point i = the first three floats of row xyz + i * row_stride_floats (>= 3: an [n, 9] cloud is read in place); with
 * origin_dev (device, 3 doubles; NULL: none) the point is float(double(x) - origin), which puts a raw cloud into the
 * detector's min-shifted frame without a host read-back.  boxes [k, 7] yx_zb (xc, yc, z_bot, d3, d4, dz, yaw), BEV
 * geometry of the IoU kernels: c = cos(yaw), s = sin(yaw) in fp64 rounded to fp32, lx = c (X - xc) - s (Y - yc),
 * ly = s (X - xc) + c (Y - yc), lz = Z - z_bot in fp32 without contraction.  Member iff |lx| <= max(d3, grow_yx) / 2,
 * |ly| <= max(d4, grow_yx) / 2 and 0 <= lz <= max(dz, grow_z), all closed (grow 0: the box as given; 0.3, 0.3: split_bbox's
 * clip); a NaN coordinate is a member of nothing.
 *   owner int32 [n]:    the lowest box index that holds the point, -1 for none (pass boxes in descending score order);
 *   count int32 [k]:    all members of each box, owned by it or not;
 *   lo, hi fp32 [k, 3]: minimum and maximum of (lx, ly, lz) over the members, a zero always as +0; +inf / -inf for an
 *                       empty box.
 * The outputs need no initialisation by the caller: the call starts its accumulators itself.  Counts are summed with
 * integer adds and extents taken with integer min / max of an order-preserving image of the floats; these commute, so
 * the same input gives the same bits without a fixed-order form, whatever torch's deterministic mode says.
 * n >= 0, 0 <= k <= 4096; n == 0 or k == 0 touch nothing out of bounds.  Asynchronous, no scratch, no read-back.       */
int d3d_points_in_boxes(const float *xyz, int n, int row_stride_floats, const double *origin_dev, const float *boxes,
                        int k, float grow_yx, float grow_z, int32_t *owner, int32_t *count, float *lo, float *hi,
                        void *stream);

/* Rotated boxes fitted to labelled points: per instance the yx_zb box of its points, the inverse of d3d_points_in_boxes.
 * The best of 256 coarse and then 256 fine candidate directions by a defined sweep (to pi / 65536 = 0.00275 degrees), not
 * the rotating-calipers optimum of a hull.  Point i as in d3d_points_in_boxes (row stride, origin_dev).  The caller lists
 * the rows by instance: order int32 [n] (row of every sorted position), sorted_id int32 [n] (its instance), offsets int32
 * [k + 1] (instance g owns the sorted positions offsets[g] .. offsets[g + 1] - 1; positions from offsets[k] on belong to
 * nothing).  Rows with a non-finite coordinate must not be listed.  coarse_dev, fine_dev: device fp64 [256, 2] (cos, sin)
 * of a 128 Q and of (i - 128) Q, Q = M_PI / 65536, made on the host, so that no device cos / sin enters the result.
 *   direction: coarse a: c = float(C[a].cos), s = float(C[a].sin); fine (a, i): c = float(Ca Fc - Sa Fs),
 *     s = float(Sa Fc + Ca Fs), products and sums separate fp64 operations;
 *   extents: u = c x - s y, v = s x + c y in fp32 without contraction, a zero always as +0; umin, umax, vmin, vmax over
 *     the instance's rows; area = (double(umax) - double(umin)) (double(vmax) - double(vmin));
 *   choice: the coarse a of the smallest area, then the fine i around it, the lowest index among equals; an instance with
 *     yaw_free[g] == 0 (uint8 [k]; NULL: all free) takes a = 0, i = 128;
 *   box, in fp64 and rounded once: t = 128 a + i - 128, theta = t Q; eu, ev the extents' lengths, mu, mv their middles;
 *     xc = c mu + s mv, yc = -s mu + c mv; free and eu > ev: d3 = ev, d4 = eu, yaw = theta + pi / 2, otherwise d3 = eu,
 *     d4 = ev, yaw = theta; yaw >= pi / 2 loses pi; z_bot = zmin, dz = zmax - zmin.
 * Outputs: boxes fp32 [k, 7], count int32 [k], choice int32 [k, 2] (a, i), extent fp32 [k, 6] (umin, umax, vmin, vmax,
 * zmin, zmax of the chosen direction).  An instance without rows: a zero box, count 0, choice (-1, -1), extents +inf / -inf.
 * Only min, max and integer arithmetic touch shared memory, so the result depends on the set of rows alone, not on their
 * order.  0 <= k <= 4096 (k == 0 touches nothing), n >= 0; scratch of d3d_fit_boxes_scratch_bytes(k) bytes (0 for a k out
 * of range).  Asynchronous, no read-back.  phase_ms_host (NULL: none): two floats, the milliseconds of pass 1 and of pass 2
 * (accumulator fill, sweep and pick each) between device events; the call then synchronises.                          */
size_t d3d_fit_boxes_scratch_bytes(int k);
int d3d_fit_boxes(const float *xyz, int n, int row_stride_floats, const double *origin_dev, const int32_t *order,
                  const int32_t *sorted_id, const int32_t *offsets, int k, const uint8_t *yaw_free,
                  const double *coarse_dev, const double *fine_dev, float *boxes, int32_t *count, int32_t *choice,
                  float *extent, void *scratch, size_t scratch_bytes, void *stream, float *phase_ms_host);

/* Rooms from boxes: a floor plan of square cells.  Lattice: cell (iy, ix), 0 <= iy < h, 0 <= ix < w, h, w <= 4096, id
 * iy w + ix, centre X = ox + (ix + 0.5) cell, Y = oy + (iy + 0.5) cell; a coordinate x lies in ix = floor((x - ox) /
 * cell), a non-finite or out-of-range index is off the lattice.  Everything is fp64, every product, sum and quotient
 * rounded on its own.  table fp64 [k, 6] on the device: (xc, yc, c, s, hx, hy) of every box, c, s = cos, sin of its yaw,
 * hx, hy its half sizes along lx = c (X - xc) - s (Y - yc) and ly = s (X - xc) + c (Y - yc); the caller makes it.
 * 0 <= k <= 4096.  All calls are asynchronous on `stream` and read nothing back; the same input gives the same bits.
 *
 * d3d_floorplan_raster: bitmap uint32 [h, ceil(w / 32)], bit ix & 31 of word ix >> 5 of row iy set iff for at least one
 * row j of the table with select[j] != 0 (select NULL: every row) |lx| <= hx and |ly| <= hy at the cell's centre; faces
 * are closed; a row with a non-finite entry blocks nothing.  The call clears the bitmap first; bits from w on stay 0.
 *
 * d3d_floorplan_rooms: the free cells (bit clear) joined over 4-connectivity.  label int32 [h, w]: -2 for a blocked
 * cell, -1 for a component that holds a cell of the lattice's border, -3 for one of fewer than min_cells (>= 1) cells,
 * else the room's number: rooms are numbered 0 .. R - 1 by ascending smallest cell id.  count int32 [1] = R.  Per room
 * below max_rooms: cells int32 (its cell count), bounds int32 [max_rooms, 4] (ix_min, iy_min, ix_max, iy_max), seed int32
 * (its smallest cell id); rows from R on hold 0, (w, h, -1, -1) and -1.  Rooms from max_rooms on keep their number in
 * label.  scratch: d3d_floorplan_scratch_bytes(h, w, k) bytes (k does not matter today).  phase_ms_host: NULL, or [5] =
 * milliseconds of the runs, the links, the roots, the ranking and the final write; the call then synchronises.
 *
 * d3d_floorplan_sides: sides int32 [k, 2], column 0 the -lx side.  Probe p = 0 .. n_probe - 1 of a side sits at
 * t = -+(hx + (p + 0.5) cell) along lx, the world point (xc + c t, yc - s t); the first probe whose cell is not blocked
 * gives the value (its label); a probe off the lattice gives -1 and ends the walk; no value: -4.
 *
 * d3d_floorplan_points: point i as in d3d_points_in_boxes (row stride; origin_dev subtracted in fp64, the difference is
 * not rounded to fp32).  room int32 [n]: the label of the point's cell, -1 off the lattice, -4 for a position with a
 * non-finite x, y or z.                                                                                              */
size_t d3d_floorplan_scratch_bytes(int h, int w, int k);
int d3d_floorplan_raster(const double *table, const uint8_t *select, int k, double cell, double ox, double oy, int h,
                         int w, uint32_t *bitmap, void *stream);
int d3d_floorplan_rooms(const uint32_t *bitmap, int h, int w, int min_cells, int max_rooms, int32_t *label,
                        int32_t *count, int32_t *cells, int32_t *bounds, int32_t *seed, void *scratch,
                        size_t scratch_bytes, void *stream, float *phase_ms_host);
int d3d_floorplan_sides(const double *table, int k, const int32_t *label, double cell, double ox, double oy, int h,
                        int w, int n_probe, int32_t *sides, void *stream);
int d3d_floorplan_points(const float *xyz, int n, int row_stride_floats, const double *origin_dev, const int32_t *label,
                         double cell, double ox, double oy, int h, int w, int32_t *room, void *stream);

/* The Manhattan frame of a scan from its normals: the rotation from the scan's frame to a level, wall-aligned one, the
 * best of 3 x 256 tilt and 2 x 256 heading candidates by a defined integer vote.  normals fp32, row i at normals +
 * i * row_stride_floats (three floats; unit length, any sign).  Every fp32 operation below is a multiply, add, min or max
 * of its own, in the order written, without contraction; no device sin / cos / sqrt / divide enters.
 *   voting rows: m = (n0 n0 + n1 n1) + n2 n2; a row votes iff 0.5 <= m <= 2 (NaN, infinite and zero rows fail);
 *   vote of a row for a unit direction u with tolerance s2: d = (n0 u0 + n1 u1) + n2 u2, a2 = d d, r = min(a2, max(m - a2,
 *     0)), v = max(s2 - r, 0), the integer trunc(v 2^30): a truncated quadratic that peaks where the normal is along +-u
 *     (floor, ceiling) or across it (walls).  Scores are 64-bit sums of these integers;
 *   tilt, passes k = 1, 2, 3 (skipped when tilt_tables_dev is NULL: B_3 = B_0, choice 136, score 0): tilt_tables_dev fp64
 *     [3, 256, 9], row-major rotations M_k[c] made on the host (entry 136 the identity); b0_host: 9 doubles on the host,
 *     the row-major frame B_0 (NULL: the identity); candidate frame B_{k-1} M_k[c] in fp64, element (r, c) = (B[r,0] M[0,c]
 *     + B[r,1] M[1,c]) + B[r,2] M[2,c]; the candidate direction is its third column rounded to fp32, the tolerance
 *     s2_host[k - 1]; the winner a_k has the highest score, the lowest index among equals, 136 when that score is 0;
 *     B_k = B_{k-1} M_k[a_k];
 *   heading, two passes over the wall rows: the voting rows with a2 <= s2_host[3] for u = the fp32 third column of B_3;
 *     p, q = the dot products (as d) of the normal with the fp32 first and second column of B_3; candidate (c, s):
 *     d1 = c p + s q, d2 = c q - s p, r = min(d1 d1, d2 d2), v = max(s2_host[3] - r, 0), vote as above; coarse_dev, fine_dev
 *     as d3d_fit_boxes takes them: coarse candidates float(C[a]), fine ones float(Ca Fc - Sa Fs), float(Sa Fc + Ca Fs);
 *     winners as above, a score of 0 gives coarse 0 and fine 128;
 *   result: t = 128 ia + ib - 128, (C, S) = (Ca Fc - Sa Fs, Sa Fc + Ca Fs) in fp64; t >= 16384: (C, S) <- (S, -C), the heading
 *     within 45 degrees of the scan's own; pose fp64 [4, 4] = [(B_3 Rz(C, S))^T 0; 0 1], aligned <- scan, the product as
 *     above with Rz = [C -S 0; S C 0; 0 0 1].
 * Outputs (device): pose; choice int32 [5]; score int64 [5], the winner's score per pass; support int32 [2], the voting
 * rows and the wall rows.  n == 0 gives B_0's pose, choice (136, 136, 136, 0, 128) and zeros.  Integer sums commute: the
 * bits depend on the set of rows alone.  s2_host: four floats in (0, 0.125].  scratch: d3d_manhattan_frame_scratch_bytes()
 * bytes.  Eleven launches on `stream`, asynchronous, no read-back.  phase_ms_host (NULL: none): five floats, the
 * milliseconds of each pass (sweep and pick) between device events; the call then synchronises.                       */
size_t d3d_manhattan_frame_scratch_bytes(void);
int d3d_manhattan_frame(const float *normals, int n, int row_stride_floats, const double *tilt_tables_dev,
                        const double *b0_host, const float *s2_host, const double *coarse_dev, const double *fine_dev,
                        double *pose, int32_t *choice, int64_t *score, int32_t *support, void *scratch,
                        size_t scratch_bytes, void *stream, float *phase_ms_host);

/* The coarse pose between two scans that come without one: a quarter turn, an integer shift on a lattice and a z shift,
 * for two clouds that are each levelled and squared already (d3d_manhattan_frame).  d3d_icp refines it.  Every table is
 * made of integers and every peak and pick is defined exactly, so the outputs depend on the sets of rows alone.
 *   inputs: per cloud xyz fp32 (row i at xyz + i * stride) and normals fp32 (likewise), and an origin o (device, 3 doubles;
 *     the cloud's per-axis minimum); bin > 0; lattice = (Lx, Ly, Lz), Lx == Ly = L a multiple of 32 in [32, 4096], Lz in
 *     [1, 4096]; c2 = float(cos^2(tol)), tol in (0, 20] degrees; peaks = K in [1, 64]; sep in [0, 64] bins.
 *   rows: m = (n0 n0 + n1 n1) + n2 n2 in fp32 without contraction; a row takes part iff 0.5 <= m <= 2 and its position is
 *     finite.  Its cell is c_a = floor((double(p_a) - o_a) / bin) in fp64; a row with a cell outside [0, L_a) is dropped
 *     and counted, the others are used.  The class of a used row is the axis a with n_a n_a >= c2 m (fp32; at most one
 *     axis, possibly none: such a row is used and enters nothing).
 *   per cloud: histograms H_a[c_a] over the rows of class a (int32), and for the wall classes x and y a bitmap of L x L
 *     bits, bit (cx, cy) = bit (cy L + cx) mod 32 of word (cy L + cx) / 32.  The source's bitmaps hold its occupied cells;
 *     the target's are dilated 3 x 3, clipped at the lattice edge.  The source's set bits are listed per class in
 *     ascending order of cy L + cx as cy << 16 | cx.
 *   quarter turns about the lattice centre, q = 0..3: (x, y) -> (x, y), (L-1-y, x), (L-1-x, L-1-y), (y, L-1-x); the source's
 *     classes x and y swap for odd q.  The turned source histogram along x is Hs_x, rev(Hs_y), rev(Hs_x), Hs_y, along y
 *     Hs_y, Hs_x, rev(Hs_y), rev(Hs_x).
 *   correlations, int64: Ht~[c] = 2 Ht[c] + Ht[c-1] + Ht[c+1] (0 outside the lattice); C[s] = sum_c Hs'[c] Ht~[c + s] for
 *     -L_a < s < L_a.  Correlation 2 q + 0 is along x and 2 q + 1 along y under turn q, correlation 8 is z.
 *   peaks: s is a peak iff C[s] > 0, no s' in [s - sep, s) has C[s'] >= C[s] and no s' in (s, s + sep] has C[s'] > C[s]
 *     (shifts outside the range do not count).  The K largest by (C descending, s ascending) are kept in that order;
 *     an unused slot has the value -1 and the shift 0.  z takes the first slot of correlation 8, or 0 when it is unused.
 *   verification of the candidates (q, i, j), 4 K K: with (sx, sy) = the shifts of slot i of correlation 2 q and slot j
 *     of 2 q + 1, score = the number of listed source cells (both classes) whose turned cell plus (sx, sy) lies in the
 *     lattice and is set in the target's dilated bitmap of the class the turn gives it.  A candidate with an unused
 *     slot scores -1.  Every occupied cell counts once: point density does not weigh.
 *   pick: the highest score, the lowest (q, i, j) among equals.  status 0; status 1 when that score is <= 0 (a cloud
 *     without walls, or without rows): choice is then zero and the pose the translation o_t - o_s.
 *   pose, fp64 row-major 4 x 4, x_t = R x_s + t: with h = L / 2, u = (o_s,x + bin h, o_s,y + bin h, o_s,z), v = (o_t,x + bin
 *     double(sx + h), o_t,y + bin double(sy + h), o_t,z + bin double(sz)) and R = Rz(q), whose entries are exactly 0 and
 *     +-1: t = v - R u, where R u is (ux, uy), (-uy, ux), (-ux, -uy), (uy, -ux) for q = 0..3 and uz.
 * Outputs (device, no read-back): pose; choice int32 [4] = (q, sx, sy, sz); score int64 [6] = the best score of each
 * heading, the best of all, and the runner-up (the highest score among all other candidates); support int32 [4] = rows
 * used and dropped of the source, then of the target; status int32 [1].  details (NULL: none): device buffers, each NULL
 * or filled with hist int32 [2, 2 L + Lz] (source, target; x, y, z), cells int32 [2, max(1, min(m, L L))] and cell_count
 * int32 [2] (the source's lists), target_bits uint32 [2, L L / 32], corr int64 [9, 2 max(L, Lz) - 1] (entry s + L_a - 1,
 * zeros behind), peak_value int64 [9, K], peak_shift int32 [9, K], scores int32 [4, K, K].
 * Limits: the overlap is maximised and free space costs nothing, so a half turn of a point-symmetric building can win
 * through a small overlap (score[5] / score[4] near 1 shows it); z is one peak, a storey off in a multi-storey partial
 * overlap; the accuracy is half a bin per axis and the frames' heading error.  0 <= m, n <= 2^28; an empty cloud gives
 * status 1.  Integer atomics only (add, or, max).  scratch: d3d_global_align_scratch_bytes(m, lattice, peaks) (0 for
 * arguments out of range).  Asynchronous.  phase_ms_host (NULL: none): six floats, the milliseconds of rows, cells,
 * correlate, peaks, verify, pick between device events; the call then synchronises.                                  */
typedef struct d3d_global_align_details {
  int32_t *hist, *cells, *cell_count;
  uint32_t *target_bits;
  int64_t *corr, *peak_value;
  int32_t *peak_shift, *scores;
} d3d_global_align_details;
size_t d3d_global_align_scratch_bytes(int n_source, const int *lattice, int peaks);
int d3d_global_align(const float *source, int m, int source_stride_floats, const float *source_normals,
                     int source_normal_stride_floats, const double *source_origin_dev, const float *target, int n,
                     int target_stride_floats, const float *target_normals, int target_normal_stride_floats,
                     const double *target_origin_dev, double bin, const int *lattice, float c2, int peaks, int sep,
                     double *pose, int32_t *choice, int64_t *score, int32_t *support, int32_t *status,
                     const d3d_global_align_details *details, void *scratch, size_t scratch_bytes, void *stream,
                     float *phase_ms_host);

/* Voxel down-sampling of a raw scan: one row per occupied voxel, every column the mean over the voxel's points
 * (data3d/suncg_utils/suncg_preprocess.py:748-767, open3d.voxel_down_sample(pcd, voxel_size=0.02)).  A restatement of
 * open3d's VoxelDownSample that is not pinned against open3d itself.  pcl fp32 [n, ncols], 3 <= ncols <= 16, contiguous,
 * columns 0:3 the position.
 *   dropped rows: a row whose position is not finite belongs to no voxel;
 *   cell of a point: lo_a = double(min over the kept rows of axis a) - 0.5 voxel; cell_a = floor((double(p_a) - lo_a) /
 *     voxel), fp64 subtraction and IEEE fp64 division, no contraction, no multiplication by a reciprocal;
 *   output values: per column the fp64 sum over the voxel's points, one fp64 division by the count, one rounding to fp32;
 *     with normal_col >= 0 the means m of columns normal_col .. normal_col + 2 are divided in fp64 by
 *     sqrt((m0 m0 + m1 m1) + m2 m2) before the rounding when that is positive, and stay as they are when it is zero;
 *     a voxel of one point is not scaled, so that its row is that point bit for bit;
 *   output order: the order of each voxel's first point in the input (the input layer's site numbering);
 *   summation order, fixed by the data: the points of a voxel in input order when there are at most 64; otherwise in
 *     chunks of 512 consecutive points, inside a chunk lane l of 64 adds points l, l + 64, ... in order, the lanes are
 *     added pairwise (l with l ^ 32, then ^ 16, ... ^ 1), and the chunk sums are added in chunk order.  No float atomics:
 *     the same input gives the same bits, whatever torch's deterministic mode says;
 *   limit: at most 2^21 cells per axis.  A wider cloud makes _cells return D3D_ERR_ARG, with a message that names the
 *     limit and the extent, and no output exists yet.
 * Two calls, because the caller allocates the outputs from the voxel count:
 *   _cells: everything up to the segments, then the one host read-back: info_host[0] = voxels M, info_host[1] = the
 *     number of 512-row chunks (both 0 for n == 0); synchronises once.
 *   _rows:  out fp32 [M, ncols]; inverse int32 [n] or NULL: the output row of every input row, -1 for a dropped row;
 *     counts int32 [M] or NULL: the points of every voxel.  `scratch` and info_host as _cells left them, same pcl, n and
 *     ncols, same stream.  Asynchronous.
 * scratch: d3d_voxel_downsample_scratch_bytes(n, ncols) bytes, linear in n and independent of the extent: 40 bytes per
 * point for the cells, permutations, keys and segments (eight int32 arrays, one int64), ncols / 8 bytes per point of
 * chunk sums, and the radix sort's 16.5 bytes per point: 59 bytes per point at ncols = 16, plus a few KiB.            */
size_t d3d_voxel_downsample_scratch_bytes(int n, int ncols);
int d3d_voxel_downsample_cells(const float *pcl, int n, int ncols, double voxel, void *scratch, size_t scratch_bytes,
                               int *info_host /* [2] */, void *stream);
int d3d_voxel_downsample_rows(const float *pcl, int n, int ncols, int normal_col /* -1: none */, const int *info_host,
                              const void *scratch, size_t scratch_bytes, float *out, int32_t *inverse, int32_t *counts,
                              void *stream);

/* A uniform random subset of k of n rows without replacement, the only_reduce form of random_sample_pcl
 * (data3d/indoor_data_util.py:59-71), in ascending row order (the reference returns it shuffled).  Row i gets the key
 *   mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16      (uint32 arithmetic)
 *   s0 = mix(uint32(seed) + 0x9e3779b9), s1 = mix(uint32(seed >> 32) ^ s0), key(i) = mix(mix(i ^ s0) + s1)
 * and the k rows with the smallest (key, i) are kept.  The mix is a bijection of the 32-bit i, so no two rows of one
 * call tie.  rows int32 [min(k, n)]; k >= n gives 0 .. n - 1.  A pure function of (n, k, seed).  Asynchronous, no
 * read-back; scratch: d3d_sample_rows_scratch_bytes(n) bytes (8 per row).                                             */
size_t d3d_sample_rows_scratch_bytes(int n);
int d3d_sample_rows(int n, int k, uint64_t seed, int32_t *rows, void *scratch, size_t scratch_bytes, void *stream);

/* The descriptors of the raw-scan chain below (d3d_unproject_*, d3d_tsdf_*, d3d_render_*): a batch of posed depth frames,
 * a TSDF block volume and a triangle mesh, each spelled out once.  Host structs of device pointers (origin: host values),
 * read during the call only; a NULL descriptor is an error.  What a call chooses for itself (step, the depth range,
 * color_div, min_weight, scratch, outputs, the stream) stays an argument.  The fields mean what the API group that
 * follows says; a call reads every field of its descriptors except those it ignores:
 *   call                      ignores of d3d_depth_frames             ignores of d3d_tsdf_volume
 *   d3d_unproject_count       color, color_is_u8, in-, extrinsics
 *   d3d_unproject_rows        -
 *   d3d_tsdf_touch            color, color_is_u8                      trunc, n_blocks, order, tsdf .. color_weight
 *   d3d_tsdf_integrate        -                                       table, table_slots, max_blocks, state, order
 *   d3d_tsdf_insert_blocks                                            voxel, trunc, origin, and as _touch
 *   d3d_tsdf_surface_count                                            voxel, trunc, origin, max_blocks, state, color_*
 *   d3d_tsdf_surface_rows                                             trunc, max_blocks, state
 *   d3d_tsdf_mesh_count                                               as _surface_count
 *   d3d_tsdf_mesh_vertices                                            trunc, max_blocks, state, weight
 *   d3d_tsdf_mesh_triangles                                           as _surface_count, and tsdf, weight
 *   d3d_render_bin, _fill     depth .. color_is_u8, depth_scale       (of d3d_triangle_mesh: vertex_color, color_is_u8)
 *   d3d_render_tiles          color_is_u8 (the mesh's holds)
 * _touch and _insert_blocks write table, block_coords and state; _integrate writes tsdf .. color_weight; _render_tiles
 * writes depth and color.  The calls that read n_blocks want a table of two slots per block at least, _touch and
 * _insert_blocks one of d3d_tsdf_table_slots(max_blocks) slots; color_state and color_weight go together.              */
typedef struct d3d_depth_frames {
  void *depth;                /* uint16 or fp32 [frames, height, width] */
  int depth_is_u16;
  void *color;                /* uint8 or fp32 [frames, height, width, 3], or NULL */
  int color_is_u8;
  const double *intrinsics;   /* fp64 [frames, 4] (fx, fy, cx, cy) */
  const double *extrinsics;   /* fp64 [frames, 3, 4] (camera to world, R | t) */
  int frames, height, width;
  double depth_scale;         /* z = double(d) * depth_scale for uint16; ignored for fp32 */
} d3d_depth_frames;

typedef struct d3d_tsdf_volume {
  double voxel, trunc, origin[3];
  void *table;                /* table_slots hash slots of 16 bytes, all ones when empty */
  int table_slots;
  int32_t *block_coords;      /* [max_blocks, 3] */
  int max_blocks, n_blocks;   /* the storage; the blocks allocated so far */
  int32_t *state;             /* [3]: blocks handed out, clipped, full; zero when empty */
  const int32_t *order;       /* [n_blocks], as d3d_tsdf_order leaves it */
  float *tsdf, *weight;       /* [n_blocks, 512] */
  float *color_state;         /* [n_blocks, 512, 3], or NULL */
  float *color_weight;        /* [n_blocks, 512], or NULL */
} d3d_tsdf_volume;

typedef struct d3d_triangle_mesh {
  const float *vertices;      /* fp32 [n_vertices, 3], world coordinates */
  int n_vertices;
  const int32_t *triangles;   /* int32 [n_triangles, 3] */
  int n_triangles;
  const void *vertex_color;   /* uint8 or fp32 [n_vertices, 3], or NULL */
  int color_is_u8;
} d3d_triangle_mesh;

/* Posed depth frames -> one cloud with colours and image-space normals: depth_2_pcl of
 * data3d/suncg_utils/suncg_preprocess.py:790-832 for a batch of frames, and what gen_pcl (:718-764) concatenates.  A
 * restatement that is not pinned against a run of the reference.  frames, a d3d_depth_frames: depth [frames, height,
 * width], uint16 or fp32; color [frames, height, width, 3], uint8 or fp32, or NULL; intrinsics fp64 [frames, 4] (fx, fy,
 * cx, cy) and extrinsics fp64 [frames, 3, 4] (camera to world, R | t), both on the device.  Every operation below is fp64
 * in exactly this order, without contraction; each output value is rounded once to fp32.
 *   pixel (f, v, u), u the column in 0 .. width - 1, v the row in 0 .. height - 1;
 *   depth: z = double(d) * depth_scale for uint16, z = double(d) for fp32 (depth_scale is ignored);
 *   valid: z is finite, z > 0 and min_depth <= z <= max_depth; kept: valid, u % step == 0 and v % step == 0;
 *   camera frame, x right, y down, z forward (the reference's [r, -u, t, v] extrinsics): zx = z / fx, zy = z / fy,
 *     C = ((double(u) - cx) * zx, (double(v) - cy) * zy, z);
 *   world position, columns 0:3: X_k = ((R[k][0] * C.x + R[k][1] * C.y) + R[k][2] * C.z) + t[k];
 *   colour, columns 3:6 (ncols >= 6): uint8: float(double(c) / color_div) (the reference divides by 256, :828); fp32:
 *     copied bit for bit; no colour pointer: zeros;
 *   normal, columns 6:9 (ncols == 9), from the raw neighbours u +- 1 and v +- 1 whatever step is.  A neighbour q of p is
 *     usable when it is inside the image, valid, and fabs(z_q - z_p) <= edge * z_p.  Horizontal difference a: both
 *     usable: C(u + 1, v) - C(u - 1, v); only the right one: C(u + 1, v) - C(u, v); only the left one: C(u, v) -
 *     C(u - 1, v); neither: no normal.  Vertical difference b: the same with v.  m = a x b = (a.y b.z - a.z b.y,
 *     a.z b.x - a.x b.z, a.x b.y - a.y b.x); l2 = (m.x m.x + m.y m.y) + m.z m.z; not l2 > 0: no normal.  If (m.x C.x +
 *     m.y C.y) + m.z C.z > 0 then m = -m: the normal faces its camera.  n = m / sqrt(l2) per component; world normal
 *     per axis k: (R[k][0] * n.x + R[k][1] * n.y) + R[k][2] * n.z.  R is taken as orthonormal, nothing is normalised
 *     again.  "No normal" is (0, 0, 0), which the voxel mean of d3d_voxel_downsample_rows (normal_col 6) ignores;
 *   order: the kept pixels in ascending (f * height + v) * width + u; pixel_of_point holds that index.
 * The same input gives the same bits.  frames * height * width >= 2^31 is an error.
 * Two calls, because the caller allocates the rows from their number:
 *   _count: one count of kept pixels per run of 2048 pixels, their scan, and the one host read-back: info_host[0] = N
 *     (0 for an empty batch); synchronises once.
 *   _rows:  out fp32 [N, ncols], ncols 3, 6 or 9; pixel_of_point int32 [N] or NULL.  Same frames, step, depth
 *     range, stream, and `scratch` and info_host as _count left them.  Asynchronous.  Never writes past N rows.
 * scratch: d3d_unproject_scratch_bytes bytes: 8 per run of 2048 pixels plus a few KiB, whatever step is.              */
size_t d3d_unproject_scratch_bytes(int frames, int height, int width, int step);
int d3d_unproject_count(const d3d_depth_frames *frames, int step, double min_depth, double max_depth, void *scratch,
                        size_t scratch_bytes, int *info_host /* [0] = N */, void *stream);
int d3d_unproject_rows(const d3d_depth_frames *frames, int step, double min_depth, double max_depth, double color_div,
                       double edge, int ncols /* 3, 6 or 9 */, const int *info_host, const void *scratch,
                       size_t scratch_bytes, float *out, int32_t *pixel_of_point, void *stream);

/* Posed depth frames -> a truncated signed-distance volume (TSDF) -> its surface cloud: KinectFusion-style projective
 * fusion; the reference has nothing like it.  Frames (a d3d_depth_frames; min_depth,
 * max_depth, step, color_div) as for d3d_unproject_*.  Every operation below is fp64 in exactly this order,
 * without contraction; each stored or returned value is rounded once to fp32.
 *   volume, a d3d_tsdf_volume: voxel > 0, trunc > 0, origin fp64 [3] (host).  Block b in [0, 65536)^3, voxel g = 8 b +
 *     l, l in [0, 8)^3, voxel position X_i = origin_i + double(g_i) * voxel.  The caller owns: table
 *     (d3d_tsdf_table_slots(max_blocks) hash slots of 16 bytes, all ones when empty), block_coords int32 [max_blocks, 3],
 *     state int32 [3] (blocks handed out, clipped, full; zero when empty), and per voxel, block id major and (lx 8 + ly)
 *     8 + lz inside the block: tsdf D, weight W, color_state C [.., 3], color_weight CW, all fp32.  Block ids depend on
 *     scheduling; d3d_tsdf_order gives the ids in ascending (x, y, z) of their coordinates and every output follows it.
 *   _touch (allocation), for every kept pixel (valid, u % step == 0 and v % step == 0) of depth z and k = -reach ..
 *     reach (the host's ceil(trunc / voxel)): z_k = z + double(k) * voxel, skipped when z_k <= 0; C = ((double(u) - cx)
 *     * (z_k / fx), (double(v) - cy) * (z_k / fy), z_k); X as in d3d_unproject_rows; q_i = floor((X_i - origin_i) /
 *     (8.0 * voxel)); a sample with a q_i outside [0, 65536) is dropped and sets `clipped`; otherwise block q is
 *     allocated if absent.  A block that no sample of a ray hits is not allocated.  One read-back: info_host[0] = blocks
 *     allocated so far, [1] = clipped, [2] = full.  Full: a block was wanted past max_blocks; it got no storage, nothing
 *     was written out of bounds, the table is then unspecified and wants clearing (all ones; state zero).
 *   _integrate: first sets the state of blocks [first_new, n_blocks) to zero, then every voxel of blocks [0, n_blocks)
 *     walks the frames f = 0 .. frames - 1 in ascending order with S = n = CS = cn = 0: d = X - t; c_j = (R[0][j] * d.x
 *     + R[1][j] * d.y) + R[2][j] * d.z; skip unless c.z > 0; pu = floor((c.x * fx / c.z + cx) + 0.5), pv likewise with
 *     fy, cy; skip unless 0 <= pu < width and 0 <= pv < height (compared in fp64; a NaN skips); zp = depth of pixel (f,
 *     pv, pu), skip unless valid (step plays no part); sdf = zp - c.z, skip when sdf < -trunc; S += min(1.0, sdf /
 *     trunc), n += 1; when sdf <= trunc and there is a colour image: CS_k += colour_k (uint8: double(c) / color_div;
 *     fp32: double(c)), cn += 1.  After the last frame, where n > 0: D = float((double(W) * double(D) + S) / (double(W)
 *     + double(n))), W = float(double(W) + double(n)); the same for C_k and CW with CS_k and cn where cn > 0; where n ==
 *     0 the stored bits do not change.  A (block, frame) pair is skipped as a whole only when no voxel of the block can
 *     pass the tests; culled_pairs (device, or NULL) is incremented by the number of such pairs.  One call of F frames
 *     and F calls of one frame may differ in the last bit.  Asynchronous.
 *   _order: order int32 [n_blocks], the block ids in ascending (x, y, z).  Asynchronous.
 *   _surface_*: a voxel is seen when double(W) >= min_weight (false for a NaN) and its D is finite.  A D of NaN or +-inf is
 *     not seen at any min_weight, so every row is finite; _integrate never produces one from finite state, and where a
 *     caller stored one it stays ((W NaN + S) / (W + n) is NaN).  Seen voxels in the order (block as in `order`, l with z
 *     fastest), and for each axis a = x, y, z: h = g + e_a (in a neighbouring block where l_a = 7) must be allocated and
 *     seen; the edge crosses when (D_g < 0) != (D_h < 0) and then gives one row: s = double(D_g) / (double(D_g) -
 *     double(D_h)); position X_g with s * voxel added on axis a; colour (ncols >= 6): C_g + s * (C_h - C_g) per channel
 *     when both CW > 0, the one that has colour when only one does, else 0 (and 0 without colour state); normal (ncols
 *     == 9), shared by the voxel's rows: when |D_g| < 1 and all three g + e_k are allocated, seen and have |D| < 1: m_k
 *     = double(D_{g + e_k}) - double(D_g), l2 = (m.x m.x + m.y m.y) + m.z m.z, m / sqrt(l2) per component when l2 > 0;
 *     otherwise (0, 0, 0).  The gradient points into free space, towards the cameras.
 *     _count: one read-back, info_host[0] = N.  _rows: out fp32 [N, ncols], voxels int32 [N, 3] (g) or NULL; same
 *     arguments, `scratch` and info_host as _count left them; asynchronous; never writes past N rows.
 * The same calls give the same bits whatever the block ids were.  No float atomics.                                   */
int d3d_tsdf_table_slots(int max_blocks);
int d3d_tsdf_touch(const d3d_depth_frames *frames, int step, double min_depth, double max_depth,
                   const d3d_tsdf_volume *volume, int reach, int *info_host /* [3] */, void *stream);
int d3d_tsdf_integrate(const d3d_depth_frames *frames, double min_depth, double max_depth, double color_div,
                       const d3d_tsdf_volume *volume, int first_new, unsigned long long *culled_pairs, void *stream);
size_t d3d_tsdf_order_scratch_bytes(int n_blocks);
int d3d_tsdf_order(const int32_t *block_coords, int n_blocks, int32_t *order, void *scratch, size_t scratch_bytes,
                   void *stream);
size_t d3d_tsdf_surface_scratch_bytes(int n_blocks);
int d3d_tsdf_surface_count(const d3d_tsdf_volume *volume, double min_weight, void *scratch, size_t scratch_bytes,
                           int *info_host /* [0] = N */, void *stream);
int d3d_tsdf_surface_rows(const d3d_tsdf_volume *volume, double min_weight, int ncols, const int *info_host,
                          const void *scratch, size_t scratch_bytes, float *out, int32_t *voxels, void *stream);

/* The TSDF volume above -> a triangle mesh of its zero crossing: marching tetrahedra on the Kuhn split of
 * every voxel cell; the reference has nothing like it.  The volume as for d3d_tsdf_surface_*; `seen`, `inside`
 * (D < 0), X_i, s and the colour rule are those of d3d_tsdf_surface_rows; so a voxel whose D is NaN or +-inf is not seen,
 * gives no vertex, and no cell it is a corner of is emitted: every vertex is finite.
 *   cells: the cell of voxel g has the corners g + c, c in {0, 1}^3, in up to eight blocks (a block coordinate outside
 *     [0, 65536) is absent); it is emitted when all eight are allocated and seen.
 *   tetrahedra: t = 0..5 for the permutations p of the axes (x = 0, y = 1, z = 2) in lexicographic order xyz, xzy, yxz,
 *     yzx, zxy, zyx with signs + - - + + -; corners c_0 = 0, c_1 = e_p1, c_2 = c_1 + e_p2, c_3 = (1, 1, 1); mask = sum of
 *     inside(c_j) 2^j.
 *   vertices: one per (g, k), k = 0..6 for e = x, y, z, xy, xz, yz, xyz, when g and g + e are allocated and seen and
 *     inside(g) != inside(g + e): s = double(D_g) / (double(D_g) - double(D_{g+e})); coordinate i is float(X_i + s *
 *     voxel) where e_i = 1 and float(X_i) elsewhere; the colour as for a surface row over g and g + e.  Ordered by
 *     (block as in `order`, l with z fastest, k); kinds 0..2 are exactly the rows of d3d_tsdf_surface_rows.  A vertex
 *     none of whose cells is emitted stays in the list, unreferenced.
 *   triangles of a tetrahedron, v(i, o) the vertex on the edge between inside corner i and outside corner o (owned by
 *     the corner with the smaller index): one inside corner a, outside b < c < d: (v(a,b), v(a,c), v(a,d)); one outside
 *     corner a, inside b < c < d: (v(b,a), v(c,a), v(d,a)); inside a < b, outside c < d: q = v(a,c), v(a,d), v(b,d),
 *     v(b,c) gives (q0, q1, q2) and (q0, q2, q3).  The last two indices of each triangle are then swapped for sign + and
 *     mask in {2, 5, 8, 10, 11, 14}, and for sign - and every other non-empty mask, so that (v1 - v0) x (v2 - v0) points
 *     from inside to outside: into free space, the normals' convention.  Ordered by (block, l, t, triangle); int32
 *     indices into the vertex list.
 *   _mesh_table: out int8 [6][16][13], per (t, mask) the triangle count, then for two triangles x three vertices, after
 *     the swap, the pair (inside corner, outside corner) as tetrahedron corners j = 0..3, -1 where unused.  Host only.
 *   _mesh_count: one read-back, info_host[0] = V, [1] = T; fails (and sets both to 0) when either is past 2^31 - 1.
 *     scratch: d3d_tsdf_mesh_scratch_bytes(n_blocks), about 4 bytes per voxel of the allocated blocks.
 *   _mesh_vertices: vertices fp32 [V, 3]; vertex_color fp32 [V, 3] or NULL (zeros without colour state); edges int32
 *     [V, 4] (g, k) or NULL.  _mesh_triangles: triangles int32 [T, 3].  Both take `scratch` and info_host as _mesh_count
 *     left them, are asynchronous and never write past V rows or T rows.
 *   _insert_blocks: puts coords int32 [n, 3] (device) into an empty table (all ones, state zero) with ids 0..n-1, the
 *     touch pass's probe sequence and bounds, and copies them to block_coords; one read-back; fails when a coordinate is
 *     outside [0, 65536) or given twice (the table then wants clearing).  The caller fills the voxel state.
 * The same calls give the same bits whatever the block ids were.  Integer counters only, no float atomics.            */
int d3d_tsdf_mesh_table(int8_t *out /* [6][16][13] */);
size_t d3d_tsdf_mesh_scratch_bytes(int n_blocks);
int d3d_tsdf_mesh_count(const d3d_tsdf_volume *volume, double min_weight, void *scratch, size_t scratch_bytes,
                        int *info_host /* [0] = V, [1] = T */, void *stream);
int d3d_tsdf_mesh_vertices(const d3d_tsdf_volume *volume, const int *info_host, const void *scratch,
                           size_t scratch_bytes, float *vertices, float *vertex_color, int32_t *edges, void *stream);
int d3d_tsdf_mesh_triangles(const d3d_tsdf_volume *volume, const int *info_host, const void *scratch,
                            size_t scratch_bytes, int32_t *triangles, void *stream);
int d3d_tsdf_insert_blocks(const int32_t *coords, int n, const d3d_tsdf_volume *volume, void *stream);

/* Posed depth frames from a triangle mesh: the step between gen_house_obj and gen_pcl of
 * data3d/suncg_utils/suncg_preprocess.py, which the reference leaves to an external OpenGL tool (scn2img).  mesh, a
 * d3d_triangle_mesh: vertices fp32 [n_vertices, 3] in world coordinates, triangles int32 [n_triangles, 3], vertex_color
 * fp32 or uint8 [n_vertices, 3] or NULL; frames, the d3d_depth_frames the calls fill: intrinsics fp64 [frames, 4] (fx,
 * fy, cx, cy) and extrinsics fp64 [frames, 3, 4] (camera to world, R | t, the camera looking along +z with x right and y
 * down) as for d3d_unproject_*, all on the device.  Every operation below is fp64 in exactly this order, without
 * contraction:
 *   camera-space vertex p = R^T (x - t): d = double(x) - t, p_k = (R[0][k] * d.x + R[1][k] * d.y) + R[2][k] * d.z, a
 *     function of (frame, vertex) alone;
 *   triangle with camera-space vertices a, b, c: n_bc = b x c with (p x q) = (p.y q.z - p.z q.y, p.z q.x - p.x q.z,
 *     p.x q.y - p.y q.x), n_ca = c x a, n_ab = a x b; D = (a.x * n_bc.x + a.y * n_bc.y) + a.z * n_bc.z;
 *   pixel (f, v, u): d = ((double(u) - cx) / fx, (double(v) - cy) / fy, 1); e0 = (d.x * n_bc.x + d.y * n_bc.y) + n_bc.z,
 *     e1 likewise from n_ca, e2 from n_ab; S = (e0 + e1) + e2;
 *   hit: S != 0 and (e0, e1, e2 all >= 0 or all <= 0): two-sided, closed edges; z = D / S, the z-depth of
 *     d3d_unproject_*; it counts when z is finite, z > 0 and min_depth <= z <= max_depth.  A triangle with a vertex
 *     index outside [0, n_vertices) or a non-finite vertex never hits (and nothing is read out of bounds);
 *   winner of a pixel: the smallest z, then the lowest triangle index: independent of any processing order;
 *   the images of `frames`: depth [frames, height, width]: fp32: float(z), 0 without a hit; uint16: rint(z /
 *     depth_scale), and 0 where that is 0 or above 65535; tri int32 [frames, height, width] or NULL: the winner, -1 for
 *     none; color [frames, height, width, 3] (with vertex_color, of its type): (w0 * c_a + w1 * c_b) + w2 * c_c with w_i
 *     = e_i / S, fp32: rounded once, uint8: rint clamped to [0, 255]; 0 without a hit.
 * Tiles of 16 x 16 pixels, three calls on one stream with the same mesh, cameras and shape:
 *   _bin:   a conservative rectangle of tiles per (frame, triangle), the list length of every tile and their scan; the
 *           one host read-back: info_host[0] = E, all list entries (0 for an empty mesh or no frame); synchronises once.
 *   _fill:  lists int32 [E], allocated by the caller: every tile's triangles, in no particular order.  Asynchronous.
 *   _tiles: one workgroup per (frame, tile) writes the images.  Asynchronous.  E >= 2^31 is an error in _fill and _tiles
 *           (use fewer frames per call), as is frames * height * width >= 2^31 everywhere.
 * scratch: d3d_render_scratch_bytes bytes, 8 per tile plus a few KiB; the lists take 4 E bytes more.                     */
size_t d3d_render_scratch_bytes(int frames, int height, int width);
int d3d_render_bin(const d3d_triangle_mesh *mesh, const d3d_depth_frames *frames, void *scratch, size_t scratch_bytes,
                   int64_t *info_host /* [0] = E */, void *stream);
int d3d_render_fill(const d3d_triangle_mesh *mesh, const d3d_depth_frames *frames, const int64_t *info_host,
                    void *scratch, size_t scratch_bytes, int32_t *lists, void *stream);
int d3d_render_tiles(const d3d_triangle_mesh *mesh, const d3d_depth_frames *frames, double min_depth, double max_depth,
                     const int64_t *info_host, const void *scratch, size_t scratch_bytes, const int32_t *lists,
                     int32_t *tri, void *stream);

/* a2/a3. InputLayer_updateOutput (SCN/sparseconvnet.h:159-163; SCN/Metadata/IOLayersRules.h:19-125;
 * SCN/CPU/IOLayers.cpp:11-47), split into the hash build (sizes) and the feature pass.
 * mode 3 = sum, 4 = mean.  Site ids follow first occurrence in input order (bit-exact with
 * the reference); duplicates are accumulated in input order.
 * Every point must be a cell of the grid: 0 <= x, y, z < spatial_size (each at most 32768) and an example index in
 * [0, 32768).  The build finds a point outside on the device, reads that back with the site count, and then returns
 * D3D_ERR_ARG with a message that names the point: no grid is entered, and the handle is left as d3d_meta_clear leaves
 * it, so the next build on it succeeds.  (Before that check the dense views and the site keys, which keep 16 bits of a
 * coordinate, took such a point as it came.)  batch_size is not used.                        */
int d3d_input_layer_build(d3d_meta *m, const int64_t *coords, int n, int ncols,
                          const int *spatial_size_host, int batch_size, int mode, void *stream,
                          int *n_active_host);
/* The same, and while the host waits for the site count the neighbour table of the submanifold rulebook
 * (spatial_size, prefetch_filter) -- the one d3d_subm_prepare is asked for first -- is already being probed on
 * `stream`, sized by n and reading the count on the device; d3d_subm_prepare on the same stream picks it up.
 * prefetch_filter NULL: plain d3d_input_layer_build.  (The reference builds that rulebook inside the first
 * convolution's forward, Metadata.cpp:430-443.)                                                              */
int d3d_input_layer_build_prefetch(d3d_meta *m, const int64_t *coords, int n, int ncols,
                                   const int *spatial_size_host, int batch_size, int mode,
                                   const int *prefetch_filter_host, void *stream, int *n_active_host);
/* The per-site point lists d3d_input_layer_forward / _backward read (IOLayersRules.h:19-125 builds them with the
 * grid) are built by the first call that needs them, on ITS stream; this builds them explicitly, e.g. on a side stream
 * while the caller's stream already probes the level-0 rulebook.                                               */
int d3d_input_layer_prepare(d3d_meta *m, void *stream);
int d3d_input_layer_forward(d3d_meta *m, const float *feats, int planes, float *out, void *stream);
/* debug exporter: rule table rows [count, idx0..] (IOLayersRules.h:112-124) as CSR.
 * offsets int32 [n_active+1], idx int32 [n].                                                 */
int d3d_input_layer_export(d3d_meta *m, int32_t *offsets, int32_t *idx, void *stream);

/* Metadata::getNActive / getSpatialLocations (SCN/Metadata/Metadata.cpp:148-168): int64 [n,4]. */
int d3d_get_n_active(d3d_meta *m, const int *spatial_size_host, int *n_host);
int d3d_get_spatial_locations(d3d_meta *m, const int *spatial_size_host, int64_t *out, void *stream);

/* AnchorGenerator.forward for one feature map (modeling/rpn/anchor_generator_sparse3d.py:86-120): for active site i
 * (in getSpatialLocations order) and cell anchor a < A (<= 16): out[(i*A + a)] = (loc_i / voxel_scale * stride, 0,0,0,0)
 * + base[a], fp32 with the reference's operation order.  base_host [A,7], stride_host [3]; out [n_active*A, 7]. */
int d3d_anchors(d3d_meta *m, const int *spatial_size_host, const float *base_host, int A,
                const float *stride_host, float voxel_scale, float *out, void *stream);
/* ... for all selected maps in one launch (the concatenation of AnchorGenerator.forward's list, rpn_sparse3d.py:246):
 * sizes_host [n_maps*3], bases_host [n_maps, A, 7], strides_host [n_maps*3]; n_maps <= 6, A <= 4;
 * out [sum_m n_active_m * A, 7], map after map.  Bit-identical to d3d_anchors per map.                              */
int d3d_anchors_maps(d3d_meta *m, int n_maps, const int *sizes_host, const float *bases_host, int A,
                     const float *strides_host, float voxel_scale, float *out, void *stream);

/* a12. RPN head at inference, SingleConvRPNHead_Sparse3D.forward + cat_scales_obj_reg
 * (modeling/rpn/rpn_sparse3d.py:80-131 and :19-77) for all selected maps in ONE launch:
 *   t = relu(x W1^T + b1);  objectness = t Wc^T + bc  [n, a];  regression = t Wr^T + br  [n, 7a]
 * over the n = sum(rows_host) site rows of the maps laid end to end (scale, site, anchor order).
 * maps_host[m]: device pointer of map m's features [rows_host[m], channels] fp32 (channels 128 or 256);
 * w1_packed [channels/4, channels, 4] with w1_packed[g][co][j] = W1[co][4g+j] (W1 = conv.weight [channels, channels]);
 * w2_packed [channels/4, NOUT, 4] likewise for the rows of (Wc; Wr) = [8a, channels] zero-padded to
 * NOUT = 32*ceil(8a/32) columns; b1 [channels], b2 [8a] = (bc; br).  a = anchors per site x class groups.          */
#define D3D_RPN_MAX_MAPS 6
int d3d_rpn_head(const float *const *maps_host, const int *rows_host, int n_maps, int channels,
                 const float *w1_packed, const float *b1, const float *w2_packed, const float *b2, int a,
                 float *objectness, float *regression, void *stream);
/* The same head over bf16 rows (bf16 storage of the heads, SparseRCNN.head_dtype): maps_host[m] bf16 [rows_host[m],
 * channels] (16-byte aligned), channels 128 or 256, and 8a <= channels (one 32-column output tile per wave at most;
 * wider heads are the caller's library GEMMs).  Weights bf16, packed [channels/8, NOUT, 8] with
 * packed[g][co][j] = W[co][8g+j] (w1: NOUT = channels; w2: the rows of (Wc; Wr) zero-padded to NOUT = 32*ceil(8a/32)),
 * 16-byte aligned; b1 / b2 fp32.  Products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; the hidden
 * t = relu(x W1^T + b1) is rounded to bf16 before the second stage; objectness and regression are fp32.           */
int d3d_rpn_head_bf16(const void *const *maps_host, const int *rows_host, int n_maps, int channels, const void *w1_packed,
                      const float *b1, const void *w2_packed, const float *b2, int a, float *objectness,
                      float *regression, void *stream);
/* a22. The box head behind fc6 at inference (roi_box_feature_extractors.py:110-117, roi_box_predictors.py:33-55) with the
 * same kernel:  t = relu(relu?(x) W1^T + b1)  [rows, channels];  out_a = t Wa^T + ba  [rows, a];  out_7a = t Wb^T + bb
 * [rows, 7a]  (a = classes: cls_score and bbox_pred).  x [rows, channels] fp32, channels 128, 256 or 512; relu_in != 0
 * rectifies x as it is read (fc6's output).  w1_packed / w2_packed / b2 as for d3d_rpn_head; either stage may be left out:
 * w1_packed == NULL -> the rows are t already (the predictor alone), w2_packed == NULL -> only t_out is written (fc7
 * alone).  t_out (may be NULL when stage 2 runs) receives t.  One launch for both stages gives the bits of the two
 * stages launched one after the other.                                                                              */
int d3d_mlp_heads(const float *x, int rows, int channels, int relu_in, const float *w1_packed, const float *b1,
                  float *t_out, const float *w2_packed, const float *b2, int a, float *out_a, float *out_7a, void *stream);

/* a4. Metadata::getSubmanifoldRuleBook (Metadata.cpp:430-443; SubmanifoldConvolutionRules.h:27-45).
 * Builds (or finds cached) the rulebook; *n_rules_host = number of (in,out) pairs.           */
int d3d_subm_prepare(d3d_meta *m, const int *spatial_size_host, const int *filter_host,
                     void *stream, long *n_rules_host);
/* a5. Metadata::getRuleBook (Metadata.cpp:485-510; ConvolutionRules.h:12-34): builds the output
 * grid of spatial size `out_size` and the rulebook.  Output sites are numbered by first touch
 * while visiting input sites in id order (canonical; the reference's order is hash-iteration
 * dependent).  A rulebook that is not cached yet is built as a grid chain of one level -- the
 * builder the geometry thread runs for a whole pyramid (d3d_geometry_async_start): same sizing by
 * bounds, the new grid carries coordinate bounds (dense index for the RoI pooler), one read-back
 * of the site count.  The call shares that read-back's pinned words and event with the geometry
 * thread: building on the geometry stream from two threads at once is not supported (it never
 * was: the arena is unlocked).                                                                 */
int d3d_conv_prepare(d3d_meta *m, const int *in_size_host, const int *out_size_host,
                     const int *filter_host, const int *stride_host, void *stream,
                     int *n_out_host, long *n_rules_host);
/* Deconvolution view of the strided rulebook of (fine size `out_size`, filter, stride): rows are the
 * fine sites (SCN/CPU/Deconvolution.cpp:17).  Requires the matching d3d_conv_prepare.          */
int d3d_deconv_prepare(d3d_meta *m, const int *in_size_host, const int *out_size_host,
                       const int *filter_host, const int *stride_host, void *stream,
                       long *n_rules_host);
/* debug exporter: rulebook as (in,out,offset) int32 triples in unspecified order; capacity in
 * triples; *n_host receives the count.  kind: 0 submanifold (out_size ignored), 1 strided.    */
int d3d_export_rules(d3d_meta *m, int kind, const int *in_size_host, const int *filter_host,
                     const int *stride_host, int32_t *triples, long capacity, long *n_host,
                     void *stream);

/* debug / measurement: grouping quality of a built rulebook.  *executed_host = 32 x the sum over the 32-row blocks of the
 * number of filter offsets the block runs, *rules_host = (in, out) pairs; executed / rules = 1 when every block's rows
 * share one offset mask.  kind as d3d_export_rules (2 = deconvolution view).  Synchronises.                          */
int d3d_plan_stats(d3d_meta *m, int kind, const int *in_size_host, const int *filter_host, const int *stride_host,
                   long *n_blocks_host, long *executed_host, long *rules_host, void *stream);

/* debug exporter: the raw tables of a built rulebook, copied on `stream` (kind, sizes as d3d_export_rules):
 *   rows    int32 [n_blk*32]     output row of every position, -1 in the padding behind n_rows
 *   nbrT    int32 [K][n_blk*32]  input row feeding position p through filter offset k, or -1
 *   blkmask uint32 [n_blk]       the offsets each block of 32 positions executes
 * dims_host[4] receives K, n_rows, n_in, n_blk; any of the three buffers may be NULL (all NULL: the sizes only).      */
int d3d_plan_export(d3d_meta *m, int kind, const int *in_size_host, const int *filter_host, const int *stride_host,
                    int32_t *rows, int32_t *nbrT, uint32_t *blkmask, int *dims_host, void *stream);
/* How the calling thread's most recently enqueued rulebook was built, recorded on the host by the call that enqueues it
 * (d3d_subm_prepare, d3d_conv_prepare / the grid chain, d3d_deconv_prepare, d3d_input_layer_build_prefetch; a cached
 * rulebook records nothing): up to n of the ints
 *   family      0 empty (nothing launched), 1 identity (1x1x1), 2 single-workgroup sort, 3 radix sort, 4 radix sort
 *               enqueued by an upper bound of the row count, the count read on the device (the prefetched rulebook)
 *   masks       0 computed in the finalisation, 1 handed in by the neighbour probes
 *   probe       0 none (strided / decoded table), 1 plain probes, 2 half-probe form
 *   K, n_rows, n_bound (what the launches were sized by), n_blk
 *   passes, digit_bits of the radix sort (0 otherwise)
 *   grid        0 no grid built with it, 1 single-workgroup grid build, 2 tiled chain, 3 empty level
 * The record is cleared by the call (out may be null).  -> the number of fields the record has.                       */
int d3d_plan_last_form(int *out, int n);
/* Test hook of the submanifold neighbour probes (process-wide; d3d_subm_prepare and the prefetch of
 * d3d_input_layer_build_prefetch): 0 (default) = the half-probe form from 262144 sites on, 1 = never, 2 = wherever the
 * filter allows it (odd in every dimension, volume > 1) at any site count.  Same tables.  mode < 0: query only.
 * -> the previous setting.                                                                                           */
int d3d_subm_probe_mode(int mode);

/* Measurement hook (bench.py's roofline leg; no reference counterpart): the next sparse-convolution launch made by
 * the calling thread records the two HIP events (hipEvent_t, created with timing) on its stream immediately before
 * and after the k_conv kernel itself -- not the k_conv_reduce of an offset-split launch -- so that the live average
 * is the duration `rocprofv3 --kernel-trace --stats` reports for that kernel name.  NULLs disarm.                */
int d3d_conv_time_next(void *start_event, void *stop_event);
/* Conv weights: reference layout [filter_volume, groups=1, Cin, Cout]
 * (sparseconvnet/submanifoldConvolution.py:24-26).  The kernels read a k-interleaved copy
 * [fv][ceil(Cin/8)*2][Cout][4] (Cin padded to 16, 32, 64, 128 or 256); pack once per weight update
 * (d3d_packed_weight_bytes / d3d_pack_conv_weight_dt below).                                 */

/* a6. SubmanifoldConvolution_updateOutput (SCN/sparseconvnet.h:99-105), Convolution_updateOutput
 * (:85-91), Deconvolution_updateOutput (:147-152): out[r_out] = sum_k in[r_in(k)] @ W[k],
 * bias-free (fpn_net.py builds every conv with bias=False).  `residual` (may be null) is added
 * in the epilogue (fuses sparseconvnet/tables.py AddTable).  *macs_host (may be null)
 * receives rules*Cin*Cout like the reference's return value.                                 */
/* Optional fusion of the PRODUCER's BatchNormalization (+ leaky ReLU) into the gather of a convolution:
 * the conv reads the un-normalised rows and applies y = leaky(x * (invstd*weight) + (bias - mean*invstd*weight))
 * on the fly (same arithmetic as d3d_bn_forward_dt), which removes one full read+write of the tensor.  Host
 * struct with device pointers; pass NULL (or mean == NULL) for none.                                 */
typedef struct {
  const float *mean, *invstd, *weight, *bias; /* [Cin]; weight / bias may be NULL */
  float leakiness;
  /* ... and of the statistics pass of the CONSUMER's BatchNormalization into the epilogue (fp32 storage): when
   * out_stats != NULL the convolution also leaves, per 32-row block (per workgroup of the reduction for an offset-split
   * launch), the fp64 sums and sums of squares of the output columns it stored: out_stats[row][2 * Cout], at most
   * out_stats_cap rows (ceil(n_out / 32) * max(1, Cout / 32) always suffice); *out_stats_rows (host) receives the
   * number of rows written, 0 when nothing was (bf16 storage, capacity too small).  d3d_bn_stats_from_partials turns
   * them into the BatchNorm's statistics in a fixed summation order.  No reference counterpart: SCN/CPU/BatchNormalization.cpp:20-31
   * makes its own pass over the tensor.                                                                             */
  double *out_stats;
  int out_stats_cap;
  int *out_stats_rows;
} d3d_bn_prologue;

/* ---- Storage types.  D3D_F32: fp32 rows, packed weights and outputs, `cin` <= 256 channels as they are.
 * D3D_BF16: bf16 storage (BASELINE.json configs[4]; the reference dispatches on the tensor type in
 * SCN/CUDA/Convolution.cu:444-521 and sparseconvnet_cuda.cpp).  Feature rows, packed weights and outputs are bf16
 * (raw 16-bit words), accumulation is fp32 on v_mfma_f32_32x32x16_bf16, BatchNorm statistics stay fp64/fp32.
 * For D3D_BF16 `cin` is the STORED row width: 16, 32, 64, 128 or 256 channels (narrower inputs are zero padded by
 * the caller; d3d_pack_conv_weight_dt pads the weights to match).                                               */
typedef enum { D3D_F32 = 0, D3D_BF16 = 1, D3D_F32_X3 = 2 } d3d_dtype;
/* D3D_F32_X3: fp32 rows, residual and outputs, as D3D_F32, with bf16x3 products -- what torch's
 * set_float32_matmul_precision('high') / matmul.fp32_precision = 'tf32' permits (gfx950 has no xf32 MFMA).  Each fp32
 * value x (row after the fused BatchNorm prologue, or weight) is split into hi = x truncated to bf16 and
 * lo = bf16(x - hi), and a 16-wide K step sums lo*Whi, hi*Wlo, hi*Whi (in that order) on v_mfma_f32_32x32x16_bf16 into
 * one fp32 accumulator.  Error of a product <= 2^-13 |x||w| (lo*Wlo dropped: < 2^-14; rounding of the two lo: 2^-16
 * each); of an output, with the fp32 accumulation, <= 2.5e-4 * sum_k |x_k||w_k|.  A non-finite x splits as (x, 0):
 * Inf and NaN reach the outputs as in D3D_F32 (a weight that bf16 holds exactly gets lo = hi * 2^-24, so that Inf * w
 * keeps its sign).  Bit-stable from run to run.  The library picks the launches by (filter volume, Cin, Cout), where
 * bf16x3 measured faster: Cin in {32, 64, 128, 256}, Cout in {32, 64, 128}, except 2x2x2 filters with Cin >= 128; every
 * other shape (the 9-channel input layer among them) runs the exact fp32 kernel, and d3d_pack_conv_weight_dt /
 * _transposed_dt pack each shape for the kernel that will read it (4 bytes per weight either way,
 * d3d_packed_weight_bytes).  Rows are stored exactly `cin` wide as for D3D_F32.  The consumer's column statistics
 * (d3d_bn_prologue.out_stats) come only from exact launches (*out_stats_rows = 0 otherwise).  In the backward
 * functions dInput runs the same way on W^T; dWeight is the exact fp32 accumulation of D3D_F32 (atomic or fixed order). */
size_t d3d_packed_weight_bytes(int filter_volume, int cin, int cout, int dtype);
int d3d_pack_conv_weight_dt(const float *w, int filter_volume, int cin, int cout, void *packed, int dtype,
                            void *stream);
int d3d_subm_conv_forward_dt(d3d_meta *m, const int *spatial_size_host, const int *filter_host, const void *in,
                             int cin, const void *packed_w, int cout, const void *residual, void *out, int dtype,
                             void *stream, double *macs_host, const d3d_bn_prologue *bn_host);
int d3d_conv_forward_dt(d3d_meta *m, const int *in_size_host, const int *out_size_host, const int *filter_host,
                        const int *stride_host, const void *in, int cin, const void *packed_w, int cout, void *out,
                        int dtype, void *stream, double *macs_host, const d3d_bn_prologue *bn_host);
int d3d_deconv_forward_dt(d3d_meta *m, const int *in_size_host, const int *out_size_host, const int *filter_host,
                          const int *stride_host, const void *in, int cin, const void *packed_w, int cout,
                          const void *residual, void *out, int dtype, void *stream, double *macs_host,
                          const d3d_bn_prologue *bn_host);
/* Grouped launches: n INDEPENDENT convolutions (no member reads what another member writes) in one call.  A descriptor
 * holds what the member's own call takes -- kind 0: d3d_subm_conv_forward_dt (in_size = the spatial size; out_size and
 * stride ignored), 1: d3d_conv_forward_dt (residual ignored), 2: d3d_deconv_forward_dt.  Members that resolve to the
 * same fp32 k_conv instantiation (padded Cin, Cout, gather form) run as ONE launch of at most 8 members (longer groups
 * take several), whose workgroups find their member in a table passed as a kernel argument; the reductions of all
 * offset-split members run as one launch as well.  Each member keeps the tiles, the step and summation order, its own
 * n_split and partial buffer, and the epilogue of its own call: every output, and every column-statistics row, is
 * bit-identical to the one-by-one calls.  Members served by the weight-sharing kernel, by bf16 rows or by bf16x3
 * products, and members that carry timing events (time_start / time_stop: recorded around that member's own k_conv
 * launch, as d3d_conv_time_next arranges for a single call) are launched one by one inside the call.  `form` (may be
 * NULL) receives the member's 12 form fields as d3d_conv_last_form reports them (zeros: nothing launched).  No
 * reference counterpart.                                                                                          */
typedef struct {
  int kind;
  int in_size[3], out_size[3], filter[3], stride[3];
  const void *in;
  int cin;
  const void *packed_w;
  int cout;
  const void *residual;
  void *out;
  int dtype; /* d3d_dtype */
  double *macs_host;
  const d3d_bn_prologue *bn_host;
  void *time_start, *time_stop; /* hipEvent_t or NULL */
  int *form;
} d3d_conv_desc;
int d3d_conv_group_forward(d3d_meta *m, const d3d_conv_desc *descs_host, int n, void *stream);
/* Tuning / test hook of the bf16 convolution (process-wide): `row_blocks` (1, 2 or 4) consecutive 32-row blocks share
 * every weight fetch in launches that keep at least min_waves * row_blocks waves (min_waves < 0: the default).
 * Results do not depend on it beyond the summation grouping of offset-split launches.                           */
int d3d_conv_bf16_tuning(int row_blocks, long min_waves);
/* d3d_bn_batch_stats (want_invstd == 0: mean, unbiased var) / d3d_bn_batch_invstd_dt (want_invstd != 0: mean,
 * powf(var + eps, -0.5)) from the column sums a convolution left per row block (d3d_bn_prologue.out_stats: partial_rows
 * rows of [2 * planes] fp64) instead of from the tensor; `rows` = rows of the tensor.  Same arithmetic after the sums,
 * a fixed summation order (deterministic), one launch.  planes: a multiple of 4, at most 512 or a multiple of 512 up
 * to 4096 (the finish walks the 2 * planes values in whole passes of 1024 threads).                                  */
int d3d_bn_stats_from_partials(const double *partials, int partial_rows, int rows, int planes, float eps,
                               int want_invstd, float *mean, float *var_or_invstd, void *scratch, size_t scratch_bytes,
                               void *stream);
/* What the calling thread's BatchNorm launch sequences chose since the last read (host side only): up to n of 19 ints,
 * a section per stage, a section zero when its stage did not run.
 *   statistics: source (1 tensor, 2 partials, 3 running statistics: nothing else recorded), storage (1 fp32, 2 bf16,
 *     3 the fp64 partials), mode of the finish (0 mean / unbiased var, 1 train, 2 mean / invstd), threads across a row,
 *     rows (of the tensor, or of partials) in flight per pass, row slices, first-level groups, slices of the last group,
 *     rows per slice;
 *   apply: kernel (1 row-walking, 2 general float4, 3 general scalar), storage, workgroups, 1 when the grid is capped far
 *     enough that the 4-rows-in-flight loop is entered;
 *   backward: partial kernel (1 float4, 2 scalar), slices, apply kernel (1 row-walking, 2 float4, 3 scalar), workgroups,
 *     1 when the two-row loop is entered, storage.
 * The record is cleared by the call (out may be null).  -> the number of fields the record has.                      */
int d3d_bn_last_form(int *out, int n);
/* The two halves of an inference BatchNorm on a tensor of storage type D3D_F32 or D3D_BF16 (statistics and parameters
 * fp32).  d3d_bn_batch_invstd_dt: mean(0) and invstd = powf(var_unbiased(0) + eps, -0.5), what the eval path with
 * track_running_stats=False feeds the normalisation with; use with d3d_bn_prologue.  d3d_bn_apply_dt: the normalisation
 * alone, y = leaky(x * (invstd*gamma) + (beta - mean*invstd*gamma)) (BatchNormalization.cpp:46-59), for a consumer of a
 * deferred BatchNorm that is not a convolution (bf16 rows: planes / 4 a divisor of 256).                             */
int d3d_bn_batch_invstd_dt(const void *in, int rows, int planes, float eps, float *mean, float *invstd,
                           void *scratch, size_t scratch_bytes, int dtype, void *stream);
int d3d_bn_apply_dt(const void *in, void *out, int rows, int planes, const float *mean, const float *invstd,
                    const float *weight, const float *bias, float leakiness, int dtype, void *stream);
/* fp32 rows [rows, cin] -> bf16 rows [rows, width], width >= cin a multiple of 8, the channels past cin zero, round to
 * nearest even: the input layer's output as the bf16 backbone stores it (fpn_net.py:150 hands the fp32 means to the first
 * convolution; the bf16 storage of BASELINE configs[4] pads the 9 input channels to 16).  One launch instead of a pad and a
 * cast.                                                                                                             */
int d3d_rows_to_bf16(const float *in, long rows, int cin, int width, void *out, void *stream);

/* a7. Backward (training).  SubmanifoldConvolution_backward / Convolution_backward / Deconvolution_backward
 * (SCN/sparseconvnet.h:92-98,106-111,153-158; SCN/CUDA/Convolution.cu:249-442): d_in is overwritten,
 * d_weight [fv, Cin, Cout] is accumulated into (the caller pre-zeroes it, as the reference's Python does).
 * `packed_wt*` is the transposed packing of d3d_pack_conv_weight_transposed_dt (flip=1 for submanifold).
 * Either gradient pointer may be null to skip it.  dWeight uses fp32 atomics (like the reference).
 * fp32 rows (D3D_F32, D3D_F32_X3): `in`, `d_out` and `d_in` are fp32 and cs == cin.
 * bf16 storage (D3D_BF16): `in`, `d_out` and `d_in` are bf16 rows; `cs` is the STORED width of `in` and `d_in` (16, 32, 64,
 * 128 or 256, as for the forward _dt functions) and `cin` the Cin of
 * the weight and of d_weight [fv, cin, cout], which stays fp32 (cs is cin padded to the next stored width: the first
 * layer stores 9 channels as 16 and its d_weight keeps 9).  dWeight is fp32-accumulated on v_mfma_f32_32x32x16_bf16
 * (atomic or fixed-order form, see below); dInput is the bf16 forward convolution with the W^T packing of
 * d3d_pack_conv_weight_transposed_dt(..., D3D_BF16) and needs cin = cs >= 32.  Other shapes: D3D_ERR_UNSUPPORTED before
 * any launch.                                                                                                     */
int d3d_pack_conv_weight_transposed_dt(const float *w, int filter_volume, int cin, int cout, int flip, void *packed,
                                       int dtype, void *stream);   /* size d3d_packed_weight_bytes(fv, cout, cin, dtype) */
int d3d_subm_conv_backward_dt(d3d_meta *m, const int *spatial_size_host, const int *filter_host, const void *in,
                              int cs, int cin, const void *packed_wt_flipped, int cout, const void *d_out, void *d_in,
                              float *d_weight, int dtype, void *stream);
int d3d_conv_backward_dt(d3d_meta *m, const int *in_size_host, const int *out_size_host, const int *filter_host,
                         const int *stride_host, const void *in, int cs, int cin, const void *packed_wt, int cout,
                         const void *d_out, void *d_in, float *d_weight, int dtype, void *stream);
int d3d_deconv_backward_dt(d3d_meta *m, const int *in_size_host, const int *out_size_host, const int *filter_host,
                           const int *stride_host, const void *in, int cs, int cin, const void *packed_wt, int cout,
                           const void *d_out, void *d_in, float *d_weight, int dtype, void *stream);
/* Process-wide switch of the dWeight accumulation of the three backward entry points above: 0 (default) = fp32 atomics
 * like the reference (SCN/CUDA/Convolution.cu:249-442 accumulates with atomicAdd: the last bits differ from run to run),
 * 1 = a fixed summation order (every workgroup sums its row blocks in order into a partial dWeight held in the
 * metadata's feature lane, taken under its lock, or in a stream-ordered allocation when the lane is too small -- at
 * most 32 x [fv, Cin, Cout] floats and at most 64 MB unless one partial is larger --, the partials are added in order): the same bits in
 * every run; the backward pass of a 6c training step at 500 k points takes 15.7 instead of 10.1 ms.  on < 0: query.  -> previous setting.  Environment: D3D_DW_DETERMINISTIC=1.       */
int d3d_conv_dw_deterministic(int on);
/* The same fixed-order dWeight for the calling thread only (what torch.use_deterministic_algorithms(True) selects in the
 * Python wrappers), whatever the process-wide switch says.  on = 1: the three backward entry points above, called from
 * this thread, sum dWeight in a fixed order with their partial sums in `scratch` (device memory of at least
 * d3d_conv_dw_scratch_bytes(fv, Cin, Cout) bytes for every layer called; it must stay valid until the launches have
 * run).  on = 0: back to the process-wide setting.  on < 0: query.  -> previous thread setting, or an error (< 0).
 * The number of partials is min(32, row-block runs, 64 MB / (4 fv Cin Cout)), at least one: a function of the rulebook
 * and the layer's size, so the bits are the same in every run.                                                      */
int d3d_conv_dw_thread_mode(int on, void *scratch, size_t scratch_bytes);
size_t d3d_conv_dw_scratch_bytes(int filter_volume, int cin, int cout);
/* The form of the calling thread's most recent dWeight launch, recorded on the host: up to n of the ints family (0 none,
 * 1 k_conv_dw on fp32 rows, 2 k_conv_dw_bf16), the kernel's channel class (CP of fp32, the stored width CS of bf16), COUT,
 * Cin of dWeight, T (32 x 32 output tiles), nz (tile groups), run (row blocks per workgroup), chunk (active blocks of a run
 * per workgroup), n_chunks, grid x / y / z, DET (0 atomic, 1 fixed order), G (partial sums; 0 in the atomic form), scratch
 * of the partials (0 none, 1 the caller's buffer, 2 the feature lane, 3 a stream-ordered allocation), row blocks, filter
 * volume.  The record is cleared by the call (out may be null).  -> the number of fields the record has.             */
int d3d_conv_dw_last_form(int *out, int n);
/* BatchNormalization_backward (SCN/sparseconvnet.h:27-32; SCN/CPU/BatchNormalization.cpp:62-107) on fp32 or bf16 rows
 * `in`, `out` (the forward's output, for the activation's mask), `d_out` and `d_in`: fp32 arithmetic and fp64 partial
 * sums either way; save_mean / save_invstd / weight and d_weight / d_bias stay fp32. */
size_t d3d_bn_backward_scratch_bytes(int planes);
int d3d_bn_backward_dt(const void *in, const void *out, const void *d_out, void *d_in, int rows, int planes,
                       const float *save_mean, const float *save_invstd, const float *weight, float *d_weight,
                       float *d_bias, float leakiness, void *scratch, size_t scratch_bytes, int dtype, void *stream);
/* InputLayer_updateGradInput (SCN/sparseconvnet.h:164-167; SCN/CPU/IOLayers.cpp:30-47). */
int d3d_input_layer_backward(d3d_meta *m, const float *d_out, int planes, float *d_in, void *stream);
/* SparseToDense_updateGradInput (SCN/sparseconvnet.h:218-222): d_in [n_active, planes] gathered from the
 * dense gradient [batch, planes, X, Y, Z].                                                          */
int d3d_sparse_to_dense_backward(d3d_meta *m, const int *spatial_size_host, const float *d_out, int planes,
                                 float *d_in, void *stream);
/* _C.roi_align_rotated_3d_backward (maskrcnn_benchmark/csrc/ROIAlignRotated3D.h:28-47): bottom_diff
 * [B,C,H,W,Z] is zeroed and accumulated into with fp32 atomics.                                      */
int d3d_roi_align_rotated_3d_backward(const float *top_diff, int B, int C, int H, int W, int Z,
                                      const float *rois, int K, float spatial_scale, int ph, int pw,
                                      int pz, int sampling_ratio, float *bottom_diff, void *stream);
/* roi_align_rotated_3d_backward restricted to the active sites (csrc/cuda/ROIAlignRotated3D_cuda.cu:238-354
 * followed by SparseToDense_updateGradInput); d_feats [n_active, C] is accumulated into.                */
int d3d_roi_align_rotated_3d_sparse_backward(d3d_meta *m, const int *spatial_size_host,
                                             const float *top_diff, int C, const int *crop_host,
                                             const float *rois, int K, float spatial_scale, int ph,
                                             int pw, int pz, int sampling_ratio, float *d_feats,
                                             void *stream);
/* The same gradient in a fixed summation order, with no float atomics: the same bits in every run
 * (torch.use_deterministic_algorithms(True)).  Taps are merged per (RoI, bin, step of 8 sub-samples, cell) into
 * records, the records are sorted stably by destination row, and every row adds its records in list order
 * (lists longer than 64 records in chunks of 64 whose partial sums are added in chunk order).  d_feats [n_rows, C]
 * (n_rows = the grid's active sites) is accumulated into.  sampling_ratio must be > 0.  `scratch`: device memory of
 * d3d_roi_align_rotated_3d_sparse_backward_deterministic_scratch_bytes(K, C, ph, pw, pz, sampling_ratio, n_rows)
 * bytes (0: arguments out of range).  It is sized for one record per tap (K x NB x sampling_ratio^3 x 8 records:
 * records, sort buffers and chunk partials all scale with that bound) -- about 310 MB for the box head's K = 512,
 * [7,7,3] bins, C = 128 at sampling ratio 2, twice that at two examples per batch.                                  */
int d3d_roi_align_rotated_3d_sparse_backward_deterministic(d3d_meta *m, const int *spatial_size_host,
                                                           const float *top_diff, int C, const int *crop_host,
                                                           const float *rois, int K, float spatial_scale, int ph,
                                                           int pw, int pz, int sampling_ratio, float *d_feats,
                                                           int n_rows, void *scratch, size_t scratch_bytes,
                                                           void *stream);
size_t d3d_roi_align_rotated_3d_sparse_backward_deterministic_scratch_bytes(int K, int C, int ph, int pw, int pz,
                                                                           int sampling_ratio, int n_rows);
/* bf16 forms of the two sparse backwards above: top_diff bf16 [K, C, ph, pw, pz] (the bf16 forward's layout 0), d_feats
 * bf16 [n_rows, C] with n_rows = the grid's active sites.  Unlike the fp32 forms they WRITE a fresh gradient (every row
 * of d_feats is written, rows no tap reaches get 0), they do not add to one.
 * _bf16: the fp32 atomics of d3d_roi_align_rotated_3d_sparse_backward into an fp32 buffer in `scratch` (zeroed by the
 *   call), then one launch rounds it to d_feats.  scratch: d3d_roi_align_rotated_3d_sparse_backward_bf16_scratch_bytes
 *   (C, n_rows) bytes (0: arguments out of range); d_feats 8-byte aligned.
 * _deterministic_bf16: the records, sort and chunk order of the fixed-order form with fp32 sums; a row is rounded when
 *   it is written, so d_feats equals the fp32 fixed-order form run on the widened top_diff into zeros, rounded to bf16,
 *   bit for bit.  sampling_ratio must be > 0 (adaptive sampling has no record bound before the launch).  scratch:
 *   d3d_roi_align_rotated_3d_sparse_backward_deterministic_bf16_scratch_bytes(K, C, ph, pw, pz, sampling_ratio, n_rows)
 *   bytes (0: arguments out of range).                                                                               */
int d3d_roi_align_rotated_3d_sparse_backward_bf16(d3d_meta *m, const int *spatial_size_host, const void *top_diff, int C,
                                                  const int *crop_host, const float *rois, int K, float spatial_scale,
                                                  int ph, int pw, int pz, int sampling_ratio, void *d_feats, int n_rows,
                                                  void *scratch, size_t scratch_bytes, void *stream);
size_t d3d_roi_align_rotated_3d_sparse_backward_bf16_scratch_bytes(int C, int n_rows);
int d3d_roi_align_rotated_3d_sparse_backward_deterministic_bf16(d3d_meta *m, const int *spatial_size_host,
                                                                const void *top_diff, int C, const int *crop_host,
                                                                const float *rois, int K, float spatial_scale, int ph,
                                                                int pw, int pz, int sampling_ratio, void *d_feats,
                                                                int n_rows, void *scratch, size_t scratch_bytes,
                                                                void *stream);
size_t d3d_roi_align_rotated_3d_sparse_backward_deterministic_bf16_scratch_bytes(int K, int C, int ph, int pw, int pz,
                                                                                int sampling_ratio, int n_rows);
/* Test hook: what the calling thread's last RoIAlign call launched (host stores only; a call that launches nothing
 * leaves the record as it is).  Fields: family (1 dense forward, 2 sparse forward, 3 dense backward, 4 sparse backward
 * with atomics, 5 its fixed-order form), storage type (1 fp32, 2 bf16), lookup (bit 0: a level probes the hash table,
 * bit 1: a level reads the dense index), extent (1 the caller's crop, 2 read on the device), grid x / y / z and
 * workgroup size of the family's main kernel (5: the chunk sums), levels with a table, workgroups of the fp32 -> bf16
 * pass (4 on bf16 rows), and for 5 the record bound n_max, its chunks and the sort's key bits.
 * The record is cleared by the call (out may be null).  -> the number of fields the record has.                      */
int d3d_roi_last_form(int *out, int n);

/* a8. BatchNormalization_updateOutput (SCN/sparseconvnet.h:21-26; SCN/CPU/BatchNormalization.cpp:12-60).
 * train!=0: batch statistics, running update r = m*r + (1-m)*batch.  train==0: uses
 * running_mean / running_var.  d3d_bn_batch_stats computes mean(0) and the UNBIASED var(0)
 * that sparseconvnet/batchNormalization.py:51-56 feeds in when track_running_stats=False.
 * d3d_bn_forward_dt takes rows of storage type D3D_F32 or D3D_BF16 (bf16: statistics in fp64 / fp32 as for fp32 rows,
 * y rounded once; save_mean, save_invstd and the running statistics fp32, same semantics).  */
int d3d_bn_forward_dt(const void *in, void *out, int rows, int planes, float *save_mean, float *save_invstd,
                      float *running_mean, float *running_var, const float *weight, const float *bias, float eps,
                      float momentum, int train, float leakiness, void *scratch, size_t scratch_bytes, int dtype,
                      void *stream);
int d3d_bn_batch_stats(const float *in, int rows, int planes, float *mean, float *var_unbiased,
                       void *scratch, size_t scratch_bytes, void *stream);
/* scratch of d3d_bn_forward_dt / d3d_bn_batch_stats / d3d_bn_batch_invstd_dt: device memory of this many bytes whose
 * first 256 bytes (ticket counters) are ZERO before the first call; the library leaves them zero.  planes must
 * be a multiple of 4 with planes/4 dividing 1024 (planes = 4, 8, ..., 4096).                                     */
size_t d3d_bn_scratch_bytes(int planes);
/* sparseconvnet/utils.py:61-66 add_feature_planes / tables.py AddTable: out = a + b. */
int d3d_add(const float *a, const float *b, float *out, size_t n, void *stream);

/* a20. SparseToDense_updateOutput (SCN/sparseconvnet.h:214-217; SCN/CPU/SparseToDense.cpp:7-60):
 * zero-filled dense [batch, planes, X, Y, Z].  batch must cover the grid's examples (1 + the largest example
 * index of the input points, where the library knows it): a smaller one is D3D_ERR_ARG before anything is
 * enqueued; a larger one leaves the trailing volumes zero.                                    */
int d3d_sparse_to_dense_forward(d3d_meta *m, const int *spatial_size_host, const float *in,
                                int planes, int batch, float *out, void *stream);

/* Pooler pre-processing in one launch: convert_metric_to_pixel (roi_box_feature_extractors.py:100), BoxList3D
 * yx_zb -> standard + convert_to_roi_format (modeling/poolers_3d.py:107-124, structures/bounding_box_3d.py:221-242)
 * and LevelMapper (poolers_3d.py:19-54 in its sqrt(max size)/canonical form).  boxes_metric [n,7] yx_zb in metres ->
 * rois [n,8] (example index, x, y, z centre, x, y, z size in full-resolution pixels, yaw in degrees) and, for
 * n_levels > 1, levels[n] = argmin_l |scales[l] - sqrt(max(size_y, size_x)) / canonical_size| (first minimum).
 * batch_ids [n] (device, may be NULL = example 0): the example each box belongs to (poolers_3d.py:112-118).      */
int d3d_roi_prepare(const float *boxes_metric, int n, float voxel_scale, const float *scales_host, int n_levels,
                    float canonical_size, const int32_t *batch_ids, float *rois, int32_t *levels, void *stream);
/* ... for a proposal list padded to n rows whose real length *count_dev (<= n) is still on the device (the survivor
 * count of the RPN's NMS, rpn/inference_3d.py:127-131, not yet read back): rows >= *count_dev get zero RoIs and level
 * -1, so no level's RoIAlign launch pools them.  count_dev NULL: all n rows are real (= d3d_roi_prepare).          */
int d3d_roi_prepare_counted(const float *boxes_metric, int n, const int32_t *count_dev, float voxel_scale,
                            const float *scales_host, int n_levels, float canonical_size, const int32_t *batch_ids,
                            float *rois, int32_t *levels, void *stream);
/* a21. _C.roi_align_rotated_3d_forward (maskrcnn_benchmark/csrc/ROIAlignRotated3D.h:10-26;
 * csrc/cuda/ROIAlignRotated3D_cuda.cu:89-177).  Dense input [B,C,H,W,Z]; rois [K,8].          */
int d3d_roi_align_rotated_3d_forward(const float *input, int B, int C, int H, int W, int Z,
                                     const float *rois, int K, float spatial_scale, int ph, int pw,
                                     int pz, int sampling_ratio, float *out, void *stream);
/* Same result sampled straight from the sparse tensor through the hash grid (no 1 GB dense
 * map): equals sparse_3d_to_dense_2d (sparseconvnet/tools_3d_2d.py:7-48, crop to the occupied
 * extent crop_host[3]; NULL: the extent of the grid itself, found on the device without a host read-back)
 * followed by the dense op.
 * roi_levels (device int32[K], nullable): only RoIs with roi_levels[i] == level are pooled, the other output
 * slots are left untouched, so that the per-level calls of poolers_3d.py:150-168 fill one result tensor
 * without nonzero / index / index_put passes.
 * layout 0: out[slot][C][ph][pw][pz] (the reference's); layout 1: out[slot][ph][pw][C][pz], the row-major
 * operand of the box head's [1,1,pz] convolution (roi_box_feature_extractors.py:68-77) as a GEMM.   */
int d3d_roi_align_rotated_3d_sparse_forward(d3d_meta *m, const int *spatial_size_host,
                                            const float *feats, int C, const int *crop_host,
                                            const float *rois, int K, float spatial_scale, int ph,
                                            int pw, int pz, int sampling_ratio, const int *roi_levels,
                                            int level, int layout, float *out, void *stream);
/* ... all levels of the pooler (poolers_3d.py:150-168) in ONE launch: RoI i is pooled from the map of level
 * roi_levels[i] (0 <= level < n_levels <= 4; any other value, e.g. the -1 of d3d_roi_prepare_counted, leaves its slot
 * untouched).  sizes_host [n_levels*3] spatial sizes of the maps, feats_host[l] device pointer of map l's features
 * [n_active_l, C], scales_host[l] its spatial scale; the occupied extent of every map is found on the device.
 * roi_levels may be NULL only for n_levels == 1.                                                                      */
int d3d_roi_align_rotated_3d_sparse_forward_levels(d3d_meta *m, int n_levels, const int *sizes_host,
                                                   const float *const *feats_host, int C, const float *scales_host,
                                                   const float *rois, int K, int ph, int pw, int pz,
                                                   int sampling_ratio, const int *roi_levels, int layout, float *out,
                                                   void *stream);
/* bf16 forms of the two above: feats bf16 [n_active, C] (4-byte aligned), out bf16 in the same layouts.  The taps are
 * widened to fp32 and summed in the fp32 kernel's order, and each bin is rounded once when it is stored: the result is
 * the fp32 op on the widened map, rounded to bf16 (round to nearest even), bit for bit.                              */
int d3d_roi_align_rotated_3d_sparse_forward_bf16(d3d_meta *m, const int *spatial_size_host, const void *feats, int C,
                                                 const int *crop_host, const float *rois, int K, float spatial_scale,
                                                 int ph, int pw, int pz, int sampling_ratio, const int *roi_levels,
                                                 int level, int layout, void *out, void *stream);
int d3d_roi_align_rotated_3d_sparse_forward_levels_bf16(d3d_meta *m, int n_levels, const int *sizes_host,
                                                        const void *const *feats_host, int C, const float *scales_host,
                                                        const float *rois, int K, int ph, int pw, int pz,
                                                        int sampling_ratio, const int *roi_levels, int layout, void *out,
                                                        void *stream);

/* a17. rotate_iou_gpu_eval (second/core/non_max_suppression/nms_gpu.py:614-664) incl.
 * check_same_boxes: boxes [N,5], query [K,5] -> out [N,K].                                   */
int d3d_rotate_iou_eval(const float *boxes, int N, const float *query, int K, int criterion,
                        float *out, void *stream);
/* a16. boxes_iou_3d (utils3d/rotate_nms_3d_torch.py:23-88): targets [M,7], anchors [N,7] yx_zb,
 * aug_host = {target_Y, target_Z, anchor_Y, anchor_Z}.                                       */
int d3d_boxes_iou_3d(const float *targets, int M, const float *anchors, int N,
                     const float *aug_host, int criterion, int only_xy, float *out, void *stream);
/* Label assignment of several segments in one launch set (rpn/loss_3d.py:178-213 and box_head_3d/loss.py:66-160 per
 * image, matcher.py:13-177, box_coder_3d.py:31-36): GT [M,7] grouped by segment (rows [gt_off_host[s],
 * gt_off_host[s+1]) of segment s; gt_off_host[0] = 0, M = gt_off_host[S], S <= 256); predictions pred [N,7] in any order,
 * pred_seg device int32 [N] = segment of each (out of range: no GT).  Every prediction is matched against its own
 * segment's GT only: quality = boxes_iou_3d (aug_host, criterion; the values of d3d_boxes_iou_3d) x, unless
 * yaw_threshold > 1.58, (|limit_period(yaw_gt - yaw_pred, 0.5, pi)| < yaw_threshold); Matcher(high, low,
 * allow_low_quality).  matched int32 [N] = GLOBAL GT row, -1 below low (and every row of a segment without GT), -2
 * between; reg_targets [N,7] (may be NULL) = box_encode(gt[max(matched, first row of the segment)], pred) x
 * encode_weights_host (NULL: ones), zeros for a segment without GT.  No host synchronisation;
 * scratch >= d3d_match_segments_scratch_bytes(M, N).                                                                  */
int d3d_match_segments(const float *gt, const int *gt_off_host, int S, const float *pred, int N, const int32_t *pred_seg,
                       const float *aug_host, int criterion, float yaw_threshold, float high, float low,
                       int allow_low_quality, const float *encode_weights_host, int32_t *matched, float *reg_targets,
                       void *scratch, size_t scratch_bytes, void *stream);
size_t d3d_match_segments_scratch_bytes(int M, int N);
/* a15/a18. rotate_nms_3d_cc (second/core/non_max_suppression/nms_cpu.py:32-44) + spconv's
 * rotate_non_max_suppression_cpu: boxes [n,7] yx_zb ALREADY sorted by descending score
 * (the callers top-k first, box_torch_ops.py:495-499).  keep int32 [n] receives positions in
 * selection order; n_keep (device int32).  The sweep may stop once max_keep (> 0) survivors exist: the
 * callers truncate to post_max_size anyway (box_torch_ops.py:506).  scratch >= d3d_nms_scratch_bytes(n). */
int d3d_rotate_nms_3d_sorted(const float *boxes, int n, float thresh, int max_keep, int32_t *keep,
                             int32_t *n_keep, void *scratch, size_t scratch_bytes, void *stream);
size_t d3d_nms_scratch_bytes(int n);
/* The same sweep for `segments` independent candidate lists in one set of launches (the classes of
 * roi_heads/box_head_3d/inference.py:113-139, or one list with its top-k order): candidate i of segment b is box
 * order[b*stride + i] of boxes [*,7] (b*stride + i when order is NULL), i < counts[b] (device int32, NULL: n_max
 * each, <= 4096), in descending score order.  min_yx / min_z: the NMS_AUG_THICKNESS clamp of boxlist_nms_3d
 * (structures/boxlist_ops_3d.py:18-52) applied for the IoU only.  keep int32 [segments, n_max] receives the BOX
 * indices of the survivors in selection order, n_keep int32 [segments] their number (<= max_keep when > 0).   */
int d3d_rotate_nms_3d_batched(const float *boxes, const int32_t *order, int stride, const int32_t *counts,
                              int segments, int n_max, float thresh, float min_yx, float min_z,
                              int max_keep, int32_t *keep, int32_t *n_keep, void *scratch,
                              size_t scratch_bytes, void *stream);
/* a15. rotate_nms_3d AS THE REFERENCE DEFINES IT (second/pytorch/core/box_torch_ops.py:489-514, called by
 * boxlist_nms_3d, structures/boxlist_ops_3d.py:14-62, with its size clamp): boxes [n,7] yx_zb and scores [n] in any order.
 * Candidates = the pre_max_size best scores (<= 0: all; at most d3d_topk_max()); descending score, and among EQUAL scores
 * the lower index first -- torch.topk / numpy argsort (nms_cpu.py:37) leave that order open, here and in the oracle port
 * it is defined: the stable argsort of -scores, under which -0.0 and +0.0 are EQUAL scores (the index decides) and a NaN
 * of either sign comes last, behind -inf.  Sizes clamped for the IoU only (dy, dx >= aug_yx, dz >= aug_z); greedy rotated NMS at `thresh`; at
 * most post_max_size survivors (<= 0: all).  keep_out int64 [min(n, pre_max_size)] = indices into the input in selection
 * order (the LongTensor the reference returns); n_keep_dev device int32 [1]; n_keep_host (NULL: no read-back) receives
 * the count after one stream synchronisation.  scratch >= d3d_rotate_nms_3d_scratch_bytes(pre_max_size, 0); with
 * d3d_rotate_nms_3d_scratch_bytes(pre_max_size, n) bytes the selection also caches its keys there (faster for large n). */
int d3d_rotate_nms_3d(const float *boxes, const float *scores, int n, int pre_max_size, int post_max_size, float thresh,
                      float aug_yx, float aug_z, int64_t *keep_out, int32_t *n_keep_dev, int *n_keep_host, void *scratch,
                      size_t scratch_bytes, void *stream);
size_t d3d_rotate_nms_3d_scratch_bytes(int pre_max_size, int n);   /* n = input boxes (0: no key scratch, slower selection) */
/* a13. The selection of RPNPostProcessor.forward_for_single_feature_map (modeling/rpn/inference_3d.py:105-123), and of
 * the per-class candidate lists of the box head's post-processing (roi_heads/box_head_3d/inference.py:113-131), for
 * n_examples x n_groups segments in ONE launch.  Segment s = example * n_groups + group reads element i at
 * vals[group * group_stride + i * elem_stride] (apply_sigmoid: 1 / (1 + exp(-x)) first, inference_3d.py:105) over the
 * elements with example[i] == its example (example NULL when n_examples == 1), keeps the k best (k <= d3d_topk_max();
 * descending, equal scores: lower index first; -0.0 and +0.0 are equal scores, a NaN of either sign sorts last, behind
 * -inf, and is never > min_value) and writes rows [s * k, s * k + min(k, elements)) of the outputs: element
 * indices (idx32_out = i * idx_map[0] + idx_map[1] + group * idx_map[2], idx_map_host NULL: i; idx64_out = i), scores
 * and -- when props_out is given -- the decoded boxes BoxCoder3D.decode(reg[i * reg_stride + 7 group .. + 7],
 * anchors[i]) with unit weights (box_coder_3d.py:38-65, inference_3d.py:123).  counts_out int32 [segments] =
 * min(k, elements of the segment), or with min_value_host the number of kept elements with value > *min_value_host
 * (the score threshold of inference.py:118; a prefix of the sorted list).  Outputs other than counts_out may be NULL. */
int d3d_topk_segments(const float *vals, int n, int elem_stride, int group_stride, int n_groups, const int32_t *example,
                      int n_examples, int k, int apply_sigmoid, const float *min_value_host, const int *idx_map_host,
                      const float *reg, int reg_stride, const float *anchors, float clip, int32_t *idx32_out,
                      int64_t *idx64_out, float *scores_out, float *props_out, int32_t *counts_out, void *scratch,
                      size_t scratch_bytes, void *stream);
/* scratch (may be NULL; 16-byte aligned, >= d3d_topk_scratch_bytes(n, segments)): the selection then evaluates every
 * element once and re-reads cached keys with wide loads in its later passes (several times faster for n ~ 10^5).      */
size_t d3d_topk_scratch_bytes(int n, int segments);
int d3d_topk_max(void);
size_t d3d_nms_batched_scratch_bytes(int segments, int n_max);
/* Measurement / test switch of the greedy sweep behind d3d_rotate_nms_3d_batched (and the two entries built on it),
 * process-wide: 0 (default) = the LDS-staged sweep k_nms_sweep_lds, 1 = the single-wave register sweep k_nms_sweep,
 * 2 = the LDS-staged sweep.  Same survivor lists.  mode < 0: query only.  -> the previous setting.
 * Environment: D3D_NMS_SWEEP (r...: starts at 1).                                                                   */
int d3d_nms_sweep_mode(int mode);
/* The form of the calling thread's most recent d3d_rotate_nms_3d_batched launch, recorded on the host: up to n of the
 * ints sweep family (0 none, 1 k_nms_sweep, 2 k_nms_sweep_lds), NCBMAX of the LDS form (16 / 32 / 64; 0 for the register
 * form), ncb (64-bit words per mask row), segments, n_max, the resolved max_keep (n_max when the caller passed <= 0),
 * dynamic LDS bytes of the sweep.  A call that launches nothing (no segments, n_max == 0) does not touch the record.
 * The record is cleared by the call (out may be null).  -> the number of fields the record has.                     */
int d3d_nms_last_form(int *out, int n);
/* Box-head post-processing glue around the batched NMS (roi_heads/box_head_3d/inference.py:113-148), one launch each:
 * post_scores: sc[(nc-1), K] = prob[i][j+1] if > thresh else -1 (class-major), counts[nc-1] = candidates per class
 *              (`inds = scores[:, j] > score_thresh`, :118);
 * post_order:  order[j][i] = idx[j][i] * nc + j + 1, the box index of class j+1's i-th best RoI (idx = stable
 *              descending argsort of sc rows) in the [K, nc] box layout -- the segments d3d_rotate_nms_3d_batched takes;
 * post_gather: survivors class-major in selection order: flat[t] = keep[t], scores[t] = prob_flat[keep[t]] for
 *              t % n_max < n_keep[t / n_max], else (0, -1) (:140-148 then picks the top detections_per_img). */
int d3d_post_scores(const float *prob, int K, int nc, float thresh, float *sc, int32_t *counts, void *stream);
int d3d_post_order(const int64_t *idx, int K, int nc, int32_t *order, void *stream);
int d3d_post_gather(const int32_t *keep, const int32_t *n_keep, int segments, int n_max, const float *prob_flat,
                    float *scores, int64_t *flat, void *stream);
/* post_select: post_gather, the cut to `detections` per image and the final gathers of :140-148 in one launch.  Over the
 * candidates t (class-major, selection order) with score s[t] = prob_flat[keep[t]] (survivors) or -1 (padding): thresh =
 * the detections-th largest s when 0 < detections < segments * n_max, clamped to >= 0, else 0; every t with
 * s[t] >= thresh is kept IN t ORDER (ties at the threshold all stay, like `cls_scores >= image_thresh`, :146) and
 * out_boxes [n,7] = boxes[keep[t]], out_scores [n] = s[t], out_labels int64 [n] = keep[t] % nc, *out_n (device) = n.
 * Every float is treated as the tensor spelling treats it (torch.sort, clamp_min(0), >=): a score of -0.0 is 0.0 and stays,
 * a NaN of either sign ranks above +inf and is never kept, and when the detections-th largest is a NaN nothing is kept.
 * Output capacity: segments * n_max rows.  segments * n_max <= d3d_post_select_max().
 * out_n (and any other count this header returns through a device pointer) may be pinned host memory: the kernel's
 * store is then the read-back, visible to the host behind an event recorded after the launch.                          */
int d3d_post_select_max(void);
int d3d_post_select(const int32_t *keep, const int32_t *n_keep, int segments, int n_max, const float *prob_flat,
                    const float *boxes, int nc, int detections, float *out_boxes, float *out_scores, int64_t *out_labels,
                    int32_t *out_n, void *stream);
/* a14. BoxCoder3D.decode (maskrcnn_benchmark/modeling/box_coder_3d.py:38-65).  The size deltas are clamped to `clip` as
 * torch.clamp(max=) clamps them: +inf becomes the clip, a NaN stays a NaN (so does the decoded size). */
int d3d_box_decode(const float *enc, const float *anchors, int n, const float *weights_host,
                   float clip, float *out, void *stream);
/* ... of class-wise encodings (roi_heads/box_head_3d/inference.py:84-87 `box_coder.decode(box_regression.view(sum, -1),
 * concat_boxes)`): enc [n, 7 nc], anchors [n, 7] -> out [n, 7 nc], every class of row i decoded against anchor i. */
int d3d_box_decode_classes(const float *enc, const float *anchors, int n, int nc, const float *weights_host,
                           float clip, float *out, void *stream);
/* ... of the rows the RPN's top-k selected (rpn/inference_3d.py:109-123: `box_regression[topk_idx]`,
 * `concat_anchors[topk_idx]`, then decode): out[i] = decode(enc[rows[i]], anchors[rows[i]]), rows int64 [n] on the device. */
int d3d_box_decode_rows(const float *enc, const float *anchors, const int64_t *rows, int n,
                        const float *weights_host, float clip, float *out, void *stream);
/* The survivors of the RPN's NMS (rpn/inference_3d.py:127-131 `boxlist = boxlist[keep]`) as a list padded to P rows
 * while their count is still on the device: for i < *n_keep_dev, out_boxes[i] = boxes[keep[i]] with the three sizes
 * clamped to >= min_size (BoxList3D.clamp_size, structures/bounding_box_3d.py) and out_scores[i] = scores[keep[i]];
 * rows >= *n_keep_dev repeat candidate 0 (d3d_roi_prepare_counted switches them off).  keep int32 (device).
 * count_out (nullable): receives *n_keep_dev by a system-scope store -- pinned host memory: the host reads it after
 * an event recorded behind this launch, while later launches of the stream (the pooler) are already running.       */
int d3d_gather_kept(const float *boxes, const float *scores, const int32_t *keep, const int32_t *n_keep_dev, int P,
                    float min_size, float *out_boxes, float *out_scores, int32_t *count_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D3D_HIP_H */
