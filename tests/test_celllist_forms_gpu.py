"""Every cell-list query on exact lattice clouds, nothing excused: d3d_radius_neighbors, d3d_knn_mean_distance,
d3d_connected_components (csrc/clean.hip), d3d_estimate_normals (csrc/normals.hip), d3d_segment_planes
(csrc/planes.hip) and d3d_nearest (csrc/register.hip), all of which stand on celllist::build (csrc/celllist.hip),
k_cln_walk<Q> / nearest_cut (csrc/cell_walk.inc) and the union-find (csrc/union_find.inc).  tests/celllist_forms.py
holds the brute-force reference and the designed clouds, tests/test_celllist_forms_cpu.py asserts on the CPU that the
reference's exact and fp32 modes agree on every cloud and that every cloud meets its design condition.

The C entries are called through ctypes as they are.  Every output is prefilled with a sentinel (NaN; integers -7) in
a buffer PAD rows longer than needed, and the rows past n must still hold it.  Every case runs with row stride 3 and
with stride 9 (a column slice of a wider cloud, read in place), twice each, and all four runs must give the same bits.

Comparisons.  count, found, label, size, the normals' counts and the nearest index: equal everywhere.  dist2 of
d3d_nearest: bit for bit.  mean: +inf exactly where the reference has it, elsewhere
|got - ref| <= (k + 4) 2^-52 ref.  Derivation: the d2 are exact, so got and ref sum the same k + 1 numbers sqrt(d2_j);
each correctly rounded square root is off by at most 2^-53 of itself (k + 1 terms, summed: (k + 1) 2^-53 of the sum, all
terms being non-negative); k additions in any order add at most k 2^-53 of the final sum to first order; the division
2^-53; the reference (math.fsum, one division) 2 2^-53: (2 k + 4) 2^-53 in all, which (k + 4) 2^-52 covers with the
second-order terms.  stats and keep are rebuilt from the GPU's own means: mu to 1e-12 relative and sigma to 1e-9 relative
against exactly rounded sums (test_clean_gpu.py's bounds), keep bit for bit from the GPU's own (mu, sigma).  Normals:
(0, 0, 1) exactly where count < 3 or all kept points coincide; unit length to 1e-6; where the reference's gap
(l1 - l0) / l2 is at least 1e-2 the angle to the reference stays below 1e-5 / gap (test_normals_gpu.py's bound) and the
sign agrees wherever the sign rule is decided by more than 2e-3 (the angle bound at the smallest gap compared is 1e-3, so
a component or a cosine moves by less than that).

Rows that are not finite: such a row has count 0, found -1, mean +inf, its own label with size 1, normal
(0, 0, 1) with count 0 and, as a query of d3d_nearest, index -1; every other row gives what it gives in the cloud without
those rows: the integers and the normals bit for bit through the row map (the extra rows keep the old rows' order, and
the normals' fp32 sums are exact on the lattice), the means within the bound above (their fp64 sums follow the sorted
positions, which the extra rows shift).

  form                                     reached by
  celllist::build: min, coords, sort,      every test; negative and far coordinates test_arith[*]; the key's high word,
  table                                    cells kCellMax - 1 | kCellMax and a cluster merged into the last cell
                                           test_clamp[0, 1, 2]; -inf as a minimum test_nonfinite[ninf_*, mixed]
  cell_insert / cell_range                 probe chains that wrap from slot cap - 1 to 0, an empty cell whose chain
                                           passes occupied slots: test_table[1024, 8192]
  k_cln_walk, staged / unstaged            test_blob[1023, 1024] staged, [1025, 2048] and test_shells_*[1000.0] unstaged
  k_cln_walk, spans and lane groups        test_walk[1, 2, 63, 64, 65, 129]: cells of 1 .. 33 points, a cell across
                                           position 64, one starting on 128, a last workgroup of one query
  neighbours across faces, edges, corners  test_arith[*]: 26 directions at exactly d == r; test_past_r[0, 1, 2]: an offset
                                           past r in the reals that fp32 rounds to r (the margin of the cell edge)
  CountQuery                               test_shells_count[*] and check_all of every case
  KnnQuery, nearest_cut: no cut, cut on    test_shells_knn[*] (k 18: a shell edge; 20: inside a shell; 27, 28, 29: k + 1,
  a shell edge, ties cut by row            k, k - 1 neighbours at the corners), test_blob[*], test_staircase
  k_cln_stat_*                             every knn run; test_stats_edges (n = 1, no finite mean, exactly one, a mean
                                           equal to the threshold); 1023, 1024, 1025 and 2049 means test_blob / test_stats_2049
  LinkQuery, union-find, roots, labels     test_shells_components[*], test_chains[single, doubled] (1000 deep, a link at
                                           exactly r, a gap of r + 1 step), check_all of every case
  NormalQuery                              test_shells_normals[*] (max_nn 19, 21, 28, 29, 30; with a viewpoint),
                                           test_staircase (the tie rule decides the normal), test_coincident
  PlaneLinkQuery                           test_planes[*]: cos_min 0, 1, 0.5; offset 0 and 1/32 with eP == offset; a NaN
                                           and a zero normal; shells and the 1025-point blob
  k_reg_nearest, query_cell                test_nearest_shells (ties across cells, exactly r, cells -1 and below),
                                           test_nearest_clamp[0, 1, 2] (queries past kCellMax), test_nonfinite[*]
  Python wrappers                          test_wrapper_* (radius_neighbors, knn_mean_distance, connected_components,
                                           estimate_normals, segment_planes, nearest), test_clean_cloud_drops_nonfinite

Not reached: n near 2^28 (the largest cloud here has 4000 rows); the automatic timing path (phase_ms_host is null
throughout); ICP beyond its nearest step (d3d_icp is not called); a stream other than the current one; d3d_fit_planes.

Cost: the module's 90 tests take 7.2 s on an MI355X, references included; the largest launch is the 2048-point blob.

Fixes these tests asked for: none.  Every test passed against the library as it stood; on the lattice the worst mean
error was 0.18 of its bound and the worst angle x gap 2.3e-8 against 1e-5.  The four suspects were read and held: the tie
search's bounds jl = 0, jh = n - 1 cover every original row; the range clamp turns a wrong table entry into a short
or empty range, which shows as a wrong count (the range_nowrap mutant); for_candidates' t + shift is the sorted position in both
forms (components equal on staged and unstaged blobs); k_cell_coords' clamp and query_cell's agree on every cell >= 0
(test_nearest_clamp).

Mutants (each built apart, the module run once against it, not kept):
  `<=` to `<` in nearest_cut's tie rule     33 tests fail: test_shells_knn[0.09375-*], [0.1f-20], [1000.0-20], every
  (count_kept)                             test_shells_normals, test_clamp[*], test_table[8192], test_chains[doubled],
                                           test_nonfinite[*], test_wrapper_knn_mean_distance, test_wrapper_estimate_normals
  want = k in KnnQuery                     39 fail: every test that calls d3d_knn_mean_distance but test_walk[1, 2]
  want = max_nn - 1 in NormalQuery         34 fail: every test_shells_normals, test_blob[*], test_walk[63 .. 129],
                                           test_clamp[*], test_table[8192], test_staircase, test_many_coincident,
                                           test_nonfinite[*], test_wrapper_estimate_normals
  26 of the 27 cells walked                24 fail, among them test_arith[origin, negative, far] (the corner pair) and
                                           test_shells_count[0.09375]
  cell edge r instead of 1.0001 r          test_past_r[0, 1, 2] fail, nothing else: on a lattice no accepted offset
  (builder and queries)                    exceeds r, so no lattice cloud can need the margin
  no kCellMax clamp in k_cell_coords       9 fail: test_clamp[0], test_nearest_clamp[0, 1, 2], test_extreme_radii[1e-30],
                                           test_nonfinite[ninf_x, ninf_yz, mixed], test_clean_cloud_drops_nonfinite
  cell_range's probing does not wrap       test_table[1024, 8192] fail, nothing else (run as "the lookup ends at the
                                           table's end": the literal mutant, slot + 1 without the mask, reads past it)
  staged = s_total < kBudget               survives, as it must: at exactly 1024 candidates the unstaged form reads the
                                           same points in the same order and gives the same bits; only the time differs
  pos <= q in LinkQuery                    survives, as it must: the extra pair is the point itself, and
                                           uf_unite(q, q) returns at once"""
import functools

import numpy as np
import pytest
import torch

from tests import celllist_forms as F

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAD = 3
SENT_I = -7
SENT_U8 = 249


def _lib():
    from detection_3d_amd._lib import lib
    return lib()


def _call(rc):
    from detection_3d_amd._lib import check
    check(rc)
    torch.cuda.synchronize()


def P(t):
    from detection_3d_amd._lib import ptr
    return ptr(t)


def S():
    from detection_3d_amd._lib import stream_of
    return stream_of()


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def place(dev, xyz, stride):
    """-> (the tensor to hand over, its row stride): contiguous rows, or columns 2:5 of a nine-column cloud"""
    x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    if stride == 3:
        return T(x, dev), 3
    wide = np.full((len(x), 9), 7777.0, np.float32)
    wide[:, 2:5] = x
    return T(wide, dev)[:, 2:5], 9


def out(n, dtype, dev, width=1):
    fill = NAN if dtype.is_floating_point else (SENT_U8 if dtype == torch.uint8 else SENT_I)
    return torch.full(((n + PAD) * width,), fill, dtype=dtype, device=dev)


def take(buf, n, width=1):
    tail = buf[n * width:]
    ok = torch.isnan(tail).all() if tail.is_floating_point() else (tail == (SENT_U8 if tail.dtype == torch.uint8 else SENT_I)).all()
    assert bool(ok), "written past the last row"
    a = buf[:n * width].cpu().numpy()
    return a.reshape(n, width) if width > 1 else a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def four_runs(fn):
    """fn(stride) twice at stride 3 and twice at stride 9: the same bits in every output"""
    first = fn(3)
    for stride in (3, 9, 9):
        again = fn(stride)
        assert all(same_bits(a, b) for a, b in zip(first, again)), ("runs differ", stride)
    return first


def scratch(nbytes, dev):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


# ------------------------------------------------------------------------------------------------------------- entries
def run_count(dev, xyz, r):
    n = len(xyz)

    def once(stride):
        x, st = place(dev, xyz, stride)
        count = out(n, torch.int32, dev)
        nb = _lib().d3d_radius_neighbors_scratch_bytes(n)
        sc = scratch(nb, dev)
        _call(_lib().d3d_radius_neighbors(P(x), n, st, r, P(count), P(sc), nb, S(), None))
        return (take(count, n),)
    return four_runs(once)[0]


def run_knn(dev, xyz, r, k, ratio=2.0):
    n = len(xyz)

    def once(stride):
        x, st = place(dev, xyz, stride)
        mean, found, keep = out(n, torch.float64, dev), out(n, torch.int32, dev), out(n, torch.uint8, dev)
        stats = out(2, torch.float64, dev)
        nb = _lib().d3d_knn_mean_distance_scratch_bytes(n)
        sc = scratch(nb, dev)
        _call(_lib().d3d_knn_mean_distance(P(x), n, st, r, k, ratio, P(mean), P(found), P(stats), P(keep), P(sc), nb, S(),
                                           None))
        return take(mean, n), take(found, n), take(stats, 2), take(keep, n)
    return four_runs(once)


def run_components(dev, xyz, r):
    n = len(xyz)

    def once(stride):
        x, st = place(dev, xyz, stride)
        label, size = out(n, torch.int32, dev), out(n, torch.int32, dev)
        nb = _lib().d3d_connected_components_scratch_bytes(n)
        sc = scratch(nb, dev)
        _call(_lib().d3d_connected_components(P(x), n, st, r, P(label), P(size), P(sc), nb, S(), None))
        return take(label, n), take(size, n)
    return four_runs(once)


def run_normals(dev, xyz, r, max_nn, vp=None):
    from detection_3d_amd._lib import floats
    n = len(xyz)

    def once(stride):
        x, st = place(dev, xyz, stride)
        normals, counts = out(n, torch.float32, dev, 3), out(n, torch.int32, dev)
        nb = _lib().d3d_estimate_normals_scratch_bytes(n, max_nn)
        sc = scratch(nb, dev)
        _call(_lib().d3d_estimate_normals(P(x), n, st, r, max_nn, floats(vp) if vp is not None else None, P(normals),
                                          P(counts), P(sc), nb, S()))
        return take(normals, n, 3), take(counts, n)
    return four_runs(once)


def run_planes(dev, xyz, nrm, r, cos_min, offset):
    n = len(xyz)

    def once(stride):
        x, st = place(dev, xyz, stride)
        v = T(np.ascontiguousarray(nrm, np.float32), dev)
        label, size = out(n, torch.int32, dev), out(n, torch.int32, dev)
        nb = _lib().d3d_segment_planes_scratch_bytes(n)
        sc = scratch(nb, dev)
        _call(_lib().d3d_segment_planes(P(x), n, st, P(v), r, cos_min, offset, P(label), P(size), P(sc), nb, S(), None))
        return take(label, n), take(size, n)
    return four_runs(once)


def run_nearest(dev, cloud, query, r):
    n, m = len(cloud), len(query)

    def once(stride):
        c, cs = place(dev, cloud, stride)
        q, qs = place(dev, query, 12 - stride)           # the two strides crossed
        index, dist2 = out(m, torch.int32, dev), out(m, torch.float32, dev)
        nb = _lib().d3d_nearest_scratch_bytes(n, m)
        sc = scratch(nb, dev)
        _call(_lib().d3d_nearest(P(c), n, cs, P(q), m, qs, r, P(index), P(dist2), P(sc), nb, S(), None))
        return take(index, m), take(dist2, m)
    return four_runs(once)


# -------------------------------------------------------------------------------------------------------------- checks
def eq(tag, got, want):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (tag, len(bad), "first", bad[:5], got[bad[:5]], want[bad[:5]])


def check_knn(tag, got, ref, k, ratio=2.0):
    mean, found, stats, keep = got
    rmean, rfound = ref
    eq((tag, "found"), found, rfound)
    eq((tag, "mean is inf"), np.isinf(mean) & (mean > 0), np.isinf(rmean))
    fin = np.isfinite(rmean)
    err, bound = np.abs(mean[fin] - rmean[fin]), (k + 4) * 2.0 ** -52 * rmean[fin]
    worst = float((err / np.maximum(bound, 1e-300)).max()) if fin.any() else 0.0
    print(f"{tag}: k {k}, {int(fin.sum())} finite means, worst error / bound {worst:.3f}")
    assert (err <= bound).all(), (tag, "mean", float(err.max()), worst)
    check_stats(tag, mean, stats, keep, ratio)


def check_stats(tag, mean, stats, keep, ratio):
    mu, sigma = F.stats_of(mean)
    print(f"{tag}: mu {stats[0]!r} (rebuilt {mu!r}), sigma {stats[1]!r} (rebuilt {sigma!r})")
    assert abs(stats[0] - mu) <= 1e-12 * mu and abs(stats[1] - sigma) <= 1e-9 * sigma, (tag, stats, mu, sigma)
    eq((tag, "keep"), keep, (np.isfinite(mean) & (mean <= stats[0] + ratio * stats[1])).astype(np.uint8))


def angles(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.arcsin(np.minimum(1.0, np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) *
                                                                             np.linalg.norm(b, axis=1))))


def check_normals(tag, got, ref, L=None, vp=None):
    gn, gc = got
    rn, rc, gap, flat = ref
    eq((tag, "counts"), gc, rc)
    assert same_bits(gn[flat], np.tile(np.float32([0, 0, 1]), (int(flat.sum()), 1))), (tag, "flat rows")
    length = np.linalg.norm(gn.astype(np.float64), axis=1)
    assert np.abs(length - 1.0).max(initial=0.0) <= 1e-6, tag
    sel = ~flat & (gap >= 1e-2)
    ang = angles(gn[sel], rn[sel])
    worst = float((ang * gap[sel]).max()) if sel.any() else 0.0
    print(f"{tag}: {int(sel.sum())} of {len(gc)} normals compared, max angle * gap {worst:.3e} (bound 1e-5)")
    assert (ang <= 1e-5 / gap[sel]).all(), (tag, worst)
    if vp is None:
        a = np.sort(np.abs(rn), axis=1)
        decided = sel & (a[:, 2] - a[:, 1] > 2e-3)
    else:
        to = np.asarray(vp, np.float64) - np.asarray(L, np.float64)
        decided = sel & (np.abs((rn * to).sum(1)) > 2e-3 * np.linalg.norm(to, axis=1))
    assert ((gn[decided].astype(np.float64) * rn[decided]).sum(1) > 0).all(), (tag, "sign")
    return int(sel.sum()), int(decided.sum())


@functools.lru_cache(maxsize=None)
def case(name, arg=None):
    """-> (L, e, r) of a designed cloud"""
    if name == "shells":
        return F.shells() + (arg,)
    if name == "blob":
        return F.blob(arg) + (F.BLOB_R,)
    if name == "walk":
        return F.walk(arg) + (F.BLOB_R,)
    if name == "arith":
        return F.arith(F.ARITH_SHIFTS[arg])[:2] + (F.ARITH_R,)
    if name == "clamp":
        return F.clamp(arg) + (F.CLAMP_R,)
    if name == "table":
        return F.table(arg)[:2] + (F.TABLE_R,)
    if name == "chains":
        return F.chains(doubled=arg) + (F.CHAIN_R,)
    if name == "stair":
        return F.staircase() + (F.STAIR_R,)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def nbs(name, arg=None):
    L, e, r = case(name, arg)
    return F.neighbours_exact(L, e, r)


def check_all(dev, name, arg, k, max_nn):
    """the four entries that take a cloud alone, on one designed cloud"""
    L, e, r = case(name, arg)
    x, nb, tag = F.xyz_of(L, e), nbs(name, arg), (name, arg)
    eq((tag, "count"), run_count(dev, x, r), F.count_ref(nb))
    check_knn(tag, run_knn(dev, x, r, k), F.knn_ref(nb, k), k)
    label, size = run_components(dev, x, r)
    rl, rs = F.components_ref(nb)
    eq((tag, "label"), label, rl)
    eq((tag, "size"), size, rs)
    if max_nn:
        check_normals(tag, run_normals(dev, x, r, max_nn), F.normals_ref(nb, L, max_nn))


# -------------------------------------------------------------------------------------------------------------- 1. shells
@pytest.mark.parametrize("r", F.SHELL_RADII)
def test_shells_count(dev, r):
    L, e, _ = case("shells", r)
    eq(("shells", r), run_count(dev, F.xyz_of(L, e), r), F.count_ref(nbs("shells", r)))


@pytest.mark.parametrize("r,k", [(F.SHELL_RADII[0], k) for k in F.SHELL_K] +
                         [(F.SHELL_RADII[1], 20), (F.SHELL_RADII[2], 1), (F.SHELL_RADII[3], 20), (F.SHELL_RADII[3], 1727)])
def test_shells_knn(dev, r, k):
    L, e, _ = case("shells", r)
    check_knn(("shells", r, k), run_knn(dev, F.xyz_of(L, e), r, k), F.knn_ref(nbs("shells", r), k), k)


@pytest.mark.parametrize("r", F.SHELL_RADII)
def test_shells_components(dev, r):
    L, e, _ = case("shells", r)
    label, size = run_components(dev, F.xyz_of(L, e), r)
    rl, rs = F.components_ref(nbs("shells", r))
    eq(("shells", r, "label"), label, rl)
    eq(("shells", r, "size"), size, rs)


SHELL_VP = (440 + 3, -136 + 20, 36 - 9)         # lattice units: beside the cube


@pytest.mark.parametrize("vp", [False, True])
@pytest.mark.parametrize("r,nn", [(F.SHELL_RADII[0], nn) for nn in F.SHELL_NN] + [(F.SHELL_RADII[1], 50), (F.SHELL_RADII[3], 30)])
def test_shells_normals(dev, r, nn, vp):
    L, e, _ = case("shells", r)
    v = np.array(SHELL_VP, np.float64) if vp else None
    got = run_normals(dev, F.xyz_of(L, e), r, nn, None if v is None else list(v * 2.0 ** -e))
    compared, decided = check_normals(("shells", r, nn, vp), got, F.normals_ref(nbs("shells", r), L, nn, v), L, v)
    assert compared >= 300 and decided >= 100


# -------------------------------------------------------------------------------------------- 2 .. 7: the designed clouds
@pytest.mark.parametrize("m", F.BLOB_SIZES)
def test_blob(dev, m):
    check_all(dev, "blob", m, 20, 50)
    L, e, r = case("blob", m)
    check_knn(("blob", m, 49), run_knn(dev, F.xyz_of(L, e), r, 49, 0.0), F.knn_ref(nbs("blob", m), 49), 49, 0.0)


@pytest.mark.parametrize("n", F.WALK_N)
def test_walk(dev, n):
    check_all(dev, "walk", n, 3 if n > 2 else 1, 9)


@pytest.mark.parametrize("where", sorted(F.ARITH_SHIFTS))
def test_arith(dev, where):
    check_all(dev, "arith", where, 1, 3)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_past_r(dev, axis):
    """an offset that exceeds r in the reals and equals it in fp32: a neighbour only the margin of the cell edge finds"""
    x, r = F.past_r(axis)
    nb = F.neighbours_f32(x, r)
    eq("count", run_count(dev, x, r), [2, 3, 2])
    check_knn(("past r", axis), run_knn(dev, x, r, 2), F.knn_ref(nb, 2), 2)
    label, size = run_components(dev, x, r)
    eq("label", label, [0, 0, 0])
    eq("size", size, [3, 3, 3])
    eq("normal counts", run_normals(dev, x, r, 3)[1], [2, 3, 2])
    index, dist2 = run_nearest(dev, x[:2], x[2:], r)
    ri, rd = F.nearest_ref(x[:2], x[2:], r)
    eq("index", index, ri)
    assert list(ri) == [1] and same_bits(dist2, rd)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_clamp(dev, axis):
    check_all(dev, "clamp", axis, 6, 10)


@pytest.mark.parametrize("cap", [1024, 8192])
def test_table(dev, cap):
    check_all(dev, "table", cap, 1, 3)


@pytest.mark.parametrize("doubled", [False, True], ids=["single", "doubled"])
def test_chains(dev, doubled):
    check_all(dev, "chains", doubled, 2, 0)


def test_staircase(dev):
    L, e, r = case("stair")
    nb = nbs("stair")
    got = run_normals(dev, F.xyz_of(L, e), r, F.STAIR_NN)
    compared, _ = check_normals("stair", got, F.normals_ref(nb, L, F.STAIR_NN))
    assert compared >= 50
    check_knn("stair", run_knn(dev, F.xyz_of(L, e), r, F.STAIR_NN - 1), F.knn_ref(nb, F.STAIR_NN - 1), F.STAIR_NN - 1)


def test_coincident(dev):
    L = np.array([[5, 5, 5]] * 4 + [[5, 5, 6]] * 2 + [[90, 90, 90]])
    nb = F.neighbours_exact(L, 5, 1.0 / 64.0)
    got = run_normals(dev, F.xyz_of(L, 5), 1.0 / 64.0, 30)
    check_normals("coincident", got, F.normals_ref(nb, L, 30))
    assert same_bits(got[0], np.tile(np.float32([0, 0, 1]), (7, 1)))


def test_many_coincident(dev):
    """ties at d2 == 0: 40 copies of one point among others; the cut keeps the lowest rows, every kept distance is 0"""
    L = np.concatenate([np.tile([[7, 7, 7]], (40, 1)), [[7, 7, 8], [8, 7, 7], [300, 0, 0]], np.tile([[7, 7, 7]], (3, 1))])
    L = L[np.random.RandomState(13).permutation(len(L))]
    nb = F.neighbours_exact(L, 5, 1.0 / 16.0)
    x = F.xyz_of(L, 5)
    got = run_knn(dev, x, 1.0 / 16.0, 5)
    check_knn("coincident", got, F.knn_ref(nb, 5), 5)
    assert (got[0][(L == 7).all(1)] == 0.0).all()
    check_normals("coincident", run_normals(dev, x, 1.0 / 16.0, 10), F.normals_ref(nb, L, 10))
    label, size = run_components(dev, x, 1.0 / 16.0)
    rl, rs = F.components_ref(nb)
    eq("label", label, rl)
    eq("size", size, rs)


@pytest.mark.parametrize("r", [1e30, 1e-30])
def test_extreme_radii(dev, r):
    """fl32(r r) is +inf (every finite pair is within r) or 0 (coincident points only, and every cell but the first
    is the last one)"""
    L, e, _ = case("blob", 1023)
    x = F.xyz_of(L, e)
    nb = F.neighbours_f32(x, r)
    count = F.count_ref(nb)
    assert (count == len(L)).all() if r > 1 else (count.max() == 2 and count.min() == 1)
    eq("count", run_count(dev, x, r), count)
    check_knn(("extreme", r), run_knn(dev, x, r, 1), F.knn_ref(nb, 1), 1)
    label, size = run_components(dev, x, r)
    rl, rs = F.components_ref(nb)
    eq("label", label, rl)
    eq("size", size, rs)


# --------------------------------------------------------------------------------------------------------------- stats
def test_stats_edges(dev):
    one = F.xyz_of([[3, 4, 5]], 5)
    mean, found, stats, keep = run_knn(dev, one, 0.25, 1)
    assert np.isposinf(mean[0]) and found[0] == 0 and same_bits(stats, np.zeros(2)) and keep[0] == 0      # no finite mean
    line = F.xyz_of([[0, 0, 0], [8, 0, 0], [16, 0, 0]], 5)                 # exactly one finite mean: the middle point
    got = run_knn(dev, line, 0.25, 2)
    check_knn("line", got, F.knn_ref(F.neighbours_exact([[0, 0, 0], [8, 0, 0], [16, 0, 0]], 5, 0.25), 2), 2)
    assert list(np.isfinite(got[0])) == [False, True, False] and same_bits(got[2], np.array([0.25, 0.0])) and list(got[3]) == [0, 1, 0]
    pair = F.xyz_of([[0, 0, 0], [8, 0, 0]], 5)                             # both means equal mu, the threshold at ratio 0
    mean, found, stats, keep = run_knn(dev, pair, 0.25, 1, 0.0)
    assert same_bits(mean, np.array([0.25, 0.25])) and same_bits(stats, np.array([0.25, 0.0])) and list(keep) == [1, 1]


def test_stats_2049(dev):
    L, e, r = case("blob", 2048)
    L = np.concatenate([L, [[5000, 0, 0]]])
    nb = F.neighbours_exact(L, e, r)
    check_knn("2049", run_knn(dev, F.xyz_of(L, e), r, 20), F.knn_ref(nb, 20), 20)


# --------------------------------------------------------------------------------------------------- 8. non-finite rows
@functools.lru_cache(maxsize=None)
def small_cube():
    L, e = F.shells(6)
    r = F.SHELL_RADII[0]
    return L, e, r, F.neighbours_exact(L, e, r)


@pytest.mark.parametrize("name", sorted(F.NONFINITE))
def test_nonfinite(dev, name):
    L, e, r, nb0 = small_cube()
    base = F.xyz_of(L, e)
    x, src = F.with_rows(base, F.NONFINITE[name])
    bad, ok = src < 0, src >= 0
    old = src[ok]
    new_row = np.flatnonzero(ok)                                  # row of the old cloud -> row of the new one
    k, nn = 20, 21
    # the fp32 definition on the whole cloud, and the cloud without the rows
    nb = F.neighbours_f32(x, r)
    count = run_count(dev, x, r)
    eq((name, "count"), count, F.count_ref(nb))
    eq((name, "count, old rows"), count[ok], run_count(dev, base, r)[old])
    assert (count[bad] == 0).all()
    got = run_knn(dev, x, r, k)
    check_knn(name, got, F.knn_ref(nb, k), k)
    assert (got[1][bad] == -1).all() and np.isposinf(got[0][bad]).all() and (got[3][bad] == 0).all()
    eq((name, "found, old rows"), got[1][ok], run_knn(dev, base, r, k)[1][old])
    label, size = run_components(dev, x, r)
    l0, s0 = run_components(dev, base, r)
    eq((name, "label"), label[ok], new_row[l0][old])
    eq((name, "size"), size[ok], s0[old])
    eq((name, "own label"), label[bad], np.flatnonzero(bad))
    assert (size[bad] == 1).all()
    gn, gc = run_normals(dev, x, r, nn)
    gn0, gc0 = run_normals(dev, base, r, nn)
    assert same_bits(gn[ok], gn0[old]) and same_bits(gc[ok], gc0[old]), (name, "normals of the old rows")
    check_normals(name, (gn0, gc0), F.normals_ref(nb0, L, nn))
    assert same_bits(gn[bad], np.tile(np.float32([0, 0, 1]), (int(bad.sum()), 1))) and (gc[bad] == 0).all()
    v = F.plane_normals(len(x), special=False)
    pl, ps = run_planes(dev, x, v, r, 0.0, 1.0 / 32.0)
    pl0, ps0 = run_planes(dev, base, v[ok], r, 0.0, 1.0 / 32.0)
    eq((name, "plane label"), pl[ok], new_row[pl0][old])
    eq((name, "plane size"), ps[ok], ps0[old])
    eq((name, "plane own label"), pl[bad], np.flatnonzero(bad))
    # as queries, and as rows of the cloud that is searched
    index, dist2 = run_nearest(dev, base, x, r)
    ri, rd = F.nearest_ref(base, x, r)
    eq((name, "index"), index, ri)
    assert same_bits(dist2, rd) and (index[bad] == -1).all() and np.isposinf(dist2[bad]).all()
    q = F.nearest_queries_shells(L)[:200]
    index, dist2 = run_nearest(dev, x, q, r)
    ri, rd = F.nearest_ref(x, q, r)
    eq((name, "index into the cloud with the rows"), index, ri)
    assert same_bits(dist2, rd)
    i0, d0 = run_nearest(dev, base, q, r)
    eq((name, "index, old rows"), np.where(index >= 0, src[np.maximum(index, 0)], -1), i0)
    assert same_bits(dist2, d0)


def test_nan_rows_only(dev):
    x = np.full((5, 3), NAN, np.float32)
    x[1, 1] = 2.0
    x[3] = (np.inf, -np.inf, NAN)
    r = 0.25
    assert (run_count(dev, x, r) == 0).all()
    mean, found, stats, keep = run_knn(dev, x, r, 1)
    assert np.isposinf(mean).all() and (found == -1).all() and same_bits(stats, np.zeros(2)) and (keep == 0).all()
    label, size = run_components(dev, x, r)
    eq("label", label, np.arange(5))
    assert (size == 1).all()
    gn, gc = run_normals(dev, x, r, 3)
    assert same_bits(gn, np.tile(np.float32([0, 0, 1]), (5, 1))) and (gc == 0).all()
    index, dist2 = run_nearest(dev, x, F.xyz_of([[0, 0, 0], [1, 64, 3]], 5), r)
    assert (index == -1).all() and np.isposinf(dist2).all()


def test_clean_cloud_drops_nonfinite(dev):
    from detection_3d_amd.clean import clean_cloud
    L, e, r, nb0 = small_cube()
    x, src = F.with_rows(F.xyz_of(L, e), F.NONFINITE["mixed"] + F.NONFINITE["nan"])
    pcl = T(np.concatenate([x, np.arange(len(x), dtype=np.float32)[:, None]], 1), dev)
    kept = clean_cloud(pcl, radius=r, min_neighbors=1)
    eq("radius_outliers", kept[:, 3].cpu().numpy(), np.flatnonzero(src >= 0))
    k = 20
    mean, found = F.knn_ref(F.neighbours_f32(x, r), k)
    kept, source = clean_cloud(pcl, radius=r, statistical=(k, 100.0), return_source=True)
    eq("statistical_outliers", kept[:, 3].cpu().numpy(), np.flatnonzero(found >= k))
    assert (source.cpu().numpy()[src < 0] == -1).all() and (found[src < 0] == -1).all()


# ------------------------------------------------------------------------------------------------------- 9. plane links
@pytest.mark.parametrize("offset", [0.0, 1.0 / 32.0])
@pytest.mark.parametrize("cos_min", F.PLANE_COS)
@pytest.mark.parametrize("cloud", ["shells", "blob"])
def test_planes(dev, cloud, cos_min, offset):
    name, arg = ("shells", F.SHELL_RADII[0]) if cloud == "shells" else ("blob", 1025)
    L, e, r = case(name, arg)
    x, v = F.xyz_of(L, e), F.plane_normals(len(L))
    label, size = run_planes(dev, x, v, r, cos_min, offset)
    rl, rs, _, _ = F.plane_links_ref(nbs(name, arg), x, v, cos_min, offset)
    eq((cloud, cos_min, offset, "label"), label, rl)
    eq((cloud, cos_min, offset, "size"), size, rs)
    assert (size[np.isnan(v).any(1)] == 1).all()                  # a NaN fails every test it enters


# ---------------------------------------------------------------------------------------------------------- 10. nearest
def test_nearest_shells(dev):
    L, e, r = case("shells", F.SHELL_RADII[0])
    x, q = F.xyz_of(L, e), F.nearest_queries_shells(L)
    index, dist2 = run_nearest(dev, x, q, r)
    ri, rd = F.nearest_ref(x, q, r)
    eq("index", index, ri)
    assert same_bits(dist2, rd)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_nearest_clamp(dev, axis):
    L, e, r = case("clamp", axis)
    x, q = F.xyz_of(L, e), F.nearest_queries_clamp(axis)
    index, dist2 = run_nearest(dev, x, q, r)
    ri, rd = F.nearest_ref(x, q, r)
    eq("index", index, ri)
    assert same_bits(dist2, rd)


# ------------------------------------------------------------------------------------------------------------- wrappers
def _shells(dev):
    L, e, r = case("shells", F.SHELL_RADII[0])
    return L, e, r, nbs("shells", r), T(F.xyz_of(L, e), dev)


def test_wrapper_radius_neighbors(dev):
    from detection_3d_amd.clean import radius_neighbors, radius_outliers
    L, e, r, nb, x = _shells(dev)
    eq("count", radius_neighbors(x, r).cpu().numpy(), F.count_ref(nb))
    eq("keep", radius_outliers(x, r, 123).cpu().numpy(), F.count_ref(nb) >= 123)


def test_wrapper_knn_mean_distance(dev):
    from detection_3d_amd.clean import knn_mean_distance, statistical_outliers
    L, e, r, nb, x = _shells(dev)
    mean, found, stats, keep = knn_mean_distance(x, 20, 0.5, r)
    got = (mean.cpu().numpy(), found.cpu().numpy(), stats.cpu().numpy(), keep.cpu().numpy().astype(np.uint8))
    check_knn("wrapper", got, F.knn_ref(nb, 20), 20, 0.5)
    eq("keep", statistical_outliers(x, 20, 0.5, r).cpu().numpy().astype(np.uint8), got[3])


def test_wrapper_connected_components(dev):
    from detection_3d_amd.clean import connected_components
    L, e, r, nb, x = _shells(dev)
    for radius in (r, F.SHELL_RADII[2]):
        label, size = connected_components(x, radius)
        rl, rs = F.components_ref(nbs("shells", radius))
        eq("label", label.cpu().numpy(), rl)
        eq("size", size.cpu().numpy(), rs)


def test_wrapper_estimate_normals(dev):
    from detection_3d_amd.normals import estimate_normals
    L, e, r, nb, x = _shells(dev)
    for vp in (None, np.array(SHELL_VP, np.float64)):
        n, c = estimate_normals(x, r, 21, orient=None if vp is None else tuple(vp * 2.0 ** -e), return_counts=True)
        check_normals(("wrapper", vp is not None), (n.cpu().numpy(), c.cpu().numpy()), F.normals_ref(nb, L, 21, vp), L, vp)


def test_wrapper_segment_planes(dev):
    from detection_3d_amd.planes import cos_min, segment_planes
    L, e, r, nb, x = _shells(dev)
    v = F.plane_normals(len(L))
    for angle in (0.0, 60.0, 90.0):
        label, size = segment_planes(x, T(v, dev), r, angle, 1.0 / 32.0)
        rl, rs, _, _ = F.plane_links_ref(nb, F.xyz_of(L, e), v, cos_min(angle), 1.0 / 32.0)
        eq(("label", angle), label.cpu().numpy(), rl)
        eq(("size", angle), size.cpu().numpy(), rs)
    assert cos_min(0.0) == 1.0 and cos_min(60.0) == 0.5


def test_wrapper_nearest(dev):
    from detection_3d_amd.register import nearest
    L, e, r, nb, x = _shells(dev)
    q = F.nearest_queries_shells(L)
    index, dist2 = nearest(T(q, dev), x, r, return_dist2=True)
    ri, rd = F.nearest_ref(F.xyz_of(L, e), q, r)
    eq("index", index.cpu().numpy(), ri)
    assert same_bits(dist2.cpu().numpy(), rd)
