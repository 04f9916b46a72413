"""Model of the rulebook plan builder (detection_3d_amd/csrc/plan.hip: finalize_plan, d3d_subm_prepare; grid_chain.hip:
run_grid_chain; grid.hip: d3d_input_layer_build_prefetch) in numpy: which build form a plan takes, the row order that form defines, the
properties every correct plan has, and the scenes the plan tests run on.  No GPU; the reference tables come from the
CPU oracle alone (oracle.subm_nbr, oracle.conv_rules, the identity for a 1x1x1 filter).

A plan: rows[npos] (output rows, -1 padded to a multiple of 32), nbrT[K][npos] (input row feeding position p through
offset k, or -1), blkmask[n_blk] (the offsets each block of 32 positions executes).  Here a plan is a dict with K,
n_rows, n_blk and those three numpy arrays (blkmask uint32)."""
import functools
import itertools

import numpy as np

# ---- the builder's thresholds, restated once ----------------------------------------------------------------------
BLOCK = 32                # positions per block (rows padding, blkmask granularity)
SMALL_MAX = 8192          # kSmallMax: rows the single-workgroup sort (k_plan_small) takes
SYM_MIN_SITES = 262144    # kSymMinSites: automatic half-probe form (k_subm_nbr_sym) from this site bound on
SMALL_GRID = 4096         # kSmallGrid: candidate entries k_conv_grid_small takes
NBR_SITES = 64            # kNbrSites: sites per workgroup of the neighbour probes
TP = 128                  # kTP: positions per workgroup of k_plan_finish
RADIX_TILE = 2048         # kRsTile: elements per workgroup of a radix pass
HASH_MUL, HASH_SHIFT, KEY_LO_BITS = 0x9E3779B1, 21, 11    # k_plan_small: key16 = (K - popcount) << 11 | lo

PLAN_FIELDS = ("family", "masks", "probe", "K", "n_rows", "n_bound", "n_blk", "passes", "digit_bits", "grid")
EMPTY, IDENTITY, SMALL, RADIX, BOUND = 0, 1, 2, 3, 4                  # family
NO_PROBE, PLAIN, HALF = 0, 1, 2                                       # probe
NO_GRID, GRID_SMALL, GRID_TILED, GRID_EMPTY = 0, 1, 2, 3              # grid
SUBM, STRIDED, DECONV = 0, 1, 2                                       # kind


def radix_layout(bits):
    """(passes, digit bits) of the radix sort of `bits`-bit keys: 8- to 10-bit digits, fewest passes (rs_layout)"""
    passes = max(1, (bits + 9) // 10)
    return passes, min(10, max(8, (bits + passes - 1) // passes))


def half_probe_allowed(filt):
    return all(int(f) & 1 for f in filt) and int(np.prod(filt)) > 1


def takes_half_probe(n_bound, filt, probe_mode=0):
    if not half_probe_allowed(filt) or probe_mode == 1:
        return False
    return probe_mode == 2 or n_bound >= SYM_MIN_SITES


def expect_plan_form(kind, n_rows, K, filt, prefetch_points=None, probe_mode=0, grid_entries=None):
    """The record d3d_plan_last_form must hold after the call that enqueued the plan.  prefetch_points: the point count
    of a level-0 plan enqueued by d3d_input_layer_build_prefetch (sized by it, the site count on the device);
    grid_entries (kind 1): input sites x candidate outputs per site, what picks the grid build."""
    assert int(np.prod(filt)) == K
    n_blk = (n_rows + BLOCK - 1) // BLOCK
    f = dict.fromkeys(PLAN_FIELDS, 0)
    f.update(K=K, n_rows=n_rows, n_bound=n_rows, n_blk=n_blk)
    if kind == SUBM and K == 1:
        f.update(family=IDENTITY)
        return f
    if kind == SUBM:
        n_bound = n_rows if prefetch_points is None else prefetch_points
        f.update(probe=HALF if takes_half_probe(n_bound, filt, probe_mode) else PLAIN)
    elif kind == STRIDED:
        assert grid_entries is not None
        f.update(grid=GRID_EMPTY if grid_entries == 0 else GRID_SMALL if grid_entries <= SMALL_GRID else GRID_TILED)
    if prefetch_points is not None:
        assert kind == SUBM and prefetch_points >= max(n_rows, 1)
        passes, db = radix_layout(min(K, 32))
        f.update(family=BOUND, masks=1, n_bound=prefetch_points, passes=passes, digit_bits=db)
    elif n_rows == 0:
        f.update(family=EMPTY)
    elif n_rows <= SMALL_MAX:
        f.update(family=SMALL, masks=int(kind == SUBM))
    else:
        passes, db = radix_layout(min(K, 32))
        f.update(family=RADIX, masks=int(kind == SUBM), passes=passes, digit_bits=db)
    return f


# ---- masks and the defined row order ------------------------------------------------------------------------------
def popcount(m):
    m = np.asarray(m, np.uint64)
    return np.array([bin(int(v)).count("1") for v in m.ravel()], np.int64).reshape(m.shape)


def masks_of(nbr):
    """uint32 offset mask of every row of a table nbr[n, K] (bit k: offset k has an input)"""
    nbr = np.asarray(nbr)
    w = (np.uint64(1) << np.arange(nbr.shape[1], dtype=np.uint64))
    return ((nbr >= 0).astype(np.uint64) * w[None]).sum(1).astype(np.uint32)


def small_key(masks, K):
    """the 16-bit key of the single-workgroup sort (k_plan_small)"""
    m = np.asarray(masks, np.uint64)
    lo = m if K <= KEY_LO_BITS else ((m * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(HASH_SHIFT)
    return ((K - popcount(m)) << KEY_LO_BITS | lo.astype(np.int64)).astype(np.int64)


def expected_rows(masks, K, family):
    """Row ids in the order the build form `family` defines: identity 0..n-1; the radix forms a stable sort descending
    by the mask value (the low K bits of plan_key: all finalize_plan sorts); the single-workgroup form a stable sort
    ascending by its 16-bit key."""
    masks = np.asarray(masks, np.uint32)
    if family == IDENTITY:
        return np.arange(masks.size, dtype=np.int32)
    if family in (RADIX, BOUND):
        return np.argsort(-masks.astype(np.int64), kind="stable").astype(np.int32)
    assert family == SMALL, family
    return np.argsort(small_key(masks, K), kind="stable").astype(np.int32)


def synth_plan(nbr, family):
    """a correct plan of the table nbr[n, K] in the order of `family`"""
    nbr = np.asarray(nbr, np.int32)
    n, K = nbr.shape
    masks = masks_of(nbr)
    n_blk = (n + BLOCK - 1) // BLOCK
    rows = np.full(n_blk * BLOCK, -1, np.int32)
    rows[:n] = expected_rows(masks, K, family)
    nbrT = np.full((K, n_blk * BLOCK), -1, np.int32)
    nbrT[:, :n] = nbr[rows[:n]].T
    pm = np.zeros(n_blk * BLOCK, np.uint32)
    pm[:n] = masks[rows[:n]]
    blkmask = np.bitwise_or.reduce(pm.reshape(n_blk, BLOCK), axis=1) if n_blk else np.zeros(0, np.uint32)
    return dict(K=K, n_rows=n, n_blk=n_blk, rows=rows, nbrT=nbrT, blkmask=blkmask.astype(np.uint32))


def model_executed(masks, K, family):
    """32 x the offsets the blocks of the plan in the defined order execute (d3d_plan_stats `executed`)"""
    return int(BLOCK * popcount(synth_plan_blkmask(masks, K, family)).sum())


def synth_plan_blkmask(masks, K, family):
    masks = np.asarray(masks, np.uint32)
    n = masks.size
    n_blk = (n + BLOCK - 1) // BLOCK
    pm = np.zeros(n_blk * BLOCK, np.uint32)
    pm[:n] = masks[expected_rows(masks, K, family)]
    return np.bitwise_or.reduce(pm.reshape(n_blk, BLOCK), axis=1) if n_blk else np.zeros(0, np.uint32)


def check_plan_valid(plan, nbr):
    """The order-independent properties of a correct plan of the table nbr[n, K] (AssertionError otherwise)."""
    nbr = np.asarray(nbr, np.int32)
    n, K = nbr.shape
    rows, nbrT, blkmask = (np.asarray(plan[k]) for k in ("rows", "nbrT", "blkmask"))
    assert plan["K"] == K and plan["n_rows"] == n, (plan["K"], plan["n_rows"], K, n)
    n_blk = (n + BLOCK - 1) // BLOCK
    npos = n_blk * BLOCK
    assert plan["n_blk"] == n_blk and rows.shape == (npos,) and nbrT.shape == (K, npos) and blkmask.shape == (n_blk,)
    assert np.array_equal(np.sort(rows[:n]), np.arange(n)), "rows[:n_rows] is not a permutation of the row ids"
    assert (rows[n:] == -1).all(), "padding of rows is not -1"
    assert np.array_equal(nbrT[:, :n], nbr[rows[:n]].T), "nbrT is not the table of its rows"
    assert (nbrT[:, n:] == -1).all(), "padding of nbrT is not -1"
    masks = masks_of(nbr)
    pm = np.zeros(npos, np.uint32)
    pm[:n] = masks[rows[:n]]
    want = np.bitwise_or.reduce(pm.reshape(n_blk, BLOCK), axis=1) if n_blk else np.zeros(0, np.uint32)
    assert np.array_equal(blkmask.astype(np.uint32), want.astype(np.uint32)), "blkmask is not the OR of its rows' masks"
    # rows of one mask value in ascending id order: group the positions by mask, positions in order inside a group
    order = np.argsort(pm[:n], kind="stable")
    same = np.diff(pm[:n][order].astype(np.int64)) == 0
    assert (np.diff(rows[:n][order].astype(np.int64))[same] > 0).all(), "rows of one mask class are not in id order"


def check_plan_order(plan, masks, family):
    """rows in the order the build form defines (kept apart from check_plan_valid: a change of the order edits
    expected_rows alone)"""
    n = plan["n_rows"]
    assert np.array_equal(np.asarray(plan["rows"])[:n], expected_rows(masks, plan["K"], family)), "row order"


# ---- reference tables (the oracle) --------------------------------------------------------------------------------
def subm_table(loc, filt):
    """-> nbr[n, K], rule count of the submanifold rulebook of the sites loc[n, 4]"""
    import oracle
    if int(np.prod(filt)) == 1:
        n = np.asarray(loc).shape[0]
        return np.arange(n, dtype=np.int32)[:, None].copy(), n
    return oracle.subm_nbr(loc, list(filt))


def strided_tables(loc, filt, stride, out_size):
    """-> loc_out, nbr[n_out, K] (forward), nbr_dec[n_in, K] (its transpose by input: the deconvolution view), rules"""
    import oracle
    lo, ru = oracle.conv_rules(loc, list(filt), list(stride), list(out_size))
    K = int(np.prod(filt))
    nbr = np.full((lo.shape[0], K), -1, np.int32)
    dec = np.full((np.asarray(loc).shape[0], K), -1, np.int32)
    nbr[ru[:, 1], ru[:, 2]] = ru[:, 0]
    dec[ru[:, 0], ru[:, 2]] = ru[:, 1]
    assert (nbr >= 0).sum() == ru.shape[0] == (dec >= 0).sum()       # an output / input meets an offset at most once
    return lo, nbr, dec, ru.shape[0]


# ---- scenes -------------------------------------------------------------------------------------------------------
SUBM_SIZE = (128, 128, 32)          # grid of the submanifold scenes


def _frozen(a):
    a = np.ascontiguousarray(a, np.int64)
    a.setflags(write=False)
    return a


def _box(cells, zmax=32):
    c = int(min(zmax, max(1, np.ceil(cells ** (1 / 3)))))
    a = int(np.ceil(np.sqrt(cells / c)))
    return a, a, c


@functools.lru_cache(maxsize=None)
def blob(n, seed, fill=0.4, origin=(0, 0, 0), zmax=32):
    """n random distinct voxels of a compact box filled to `fill`, int64 [n, 3], in random (site) order: nearly every
    row has an offset mask of its own, and the hashed keys of the single-workgroup sort collide"""
    rng = np.random.RandomState(seed)
    a, b, c = _box(max(n / fill, n), zmax)
    idx = rng.permutation(a * b * c)[:n]
    pts = np.stack([idx // (b * c), (idx // c) % b, idx % c], 1) + np.asarray(origin)
    return _frozen(pts)


@functools.lru_cache(maxsize=None)
def structured(n, seed, size=SUBM_SIZE):
    """n distinct sites of `size` in random (site) order, after _structured_coords of test_conv_forms_gpu.py: dense
    blocks (rows with all 27 offsets), 2x2x2 cubes, 2x2 squares, 3-site lines and isolated sites -- few masks, with
    hundreds of rows each.  Structures sit in 8^3 cells of their own, isolated sites on the even points of the other
    cells, so no two of them touch.  Below 696 sites the structures are one 3^3 block, one cube, one square and one
    line (42 sites), the rest isolated."""
    rng = np.random.RandomState(seed)
    cells = [np.array(c) for c in itertools.product(*(range(0, s, 8) for s in size))]
    cells = [cells[i] for i in rng.permutation(len(cells))]
    if n >= 696:
        pts = [cells[0] + d for d in itertools.product(range(6), repeat=3)]
        for c in cells[1:6]:
            for o in itertools.product((0, 4), repeat=3):
                pts += [c + np.array(o) + d for d in itertools.product((0, 1), repeat=3)]
        for c in cells[6:8]:
            for o in itertools.product((0, 4), repeat=3):
                pts += [c + np.array(o) + (i, j, 0) for i in (0, 1) for j in (0, 1)]
        for o in itertools.product((0, 4), (0, 2, 4, 6), (0, 2, 4, 6)):
            pts += [cells[8] + np.array(o) + (i, 0, 0) for i in range(3)]
        free = cells[9:]
    else:
        pts = [cells[0] + d for d in itertools.product(range(3), repeat=3)]
        pts += [cells[1] + d for d in itertools.product((0, 1), repeat=3)]
        pts += [cells[2] + (i, j, 0) for i in (0, 1) for j in (0, 1)]
        pts += [cells[3] + (i, 0, 0) for i in range(3)]
        free = cells[4:]
        pts = pts[:n]
    need = n - len(pts)
    if need > 0:
        even = np.array(list(itertools.product((0, 2, 4, 6), repeat=3)))
        cand = (np.array(free)[:, None, :] + even[None]).reshape(-1, 3)
        assert need <= len(cand)
        pts += list(cand[rng.permutation(len(cand))[:need]])
    pts = np.array(pts, np.int64)
    assert len(np.unique(pts, axis=0)) == n
    return _frozen(pts[rng.permutation(n)])


@functools.lru_cache(maxsize=None)
def border(n, seed, size=(64, 64, 32)):
    """n distinct sites on the faces of the grid `size` (a coordinate at 0 or at size - 1), its 8 corners among them"""
    rng = np.random.RandomState(seed)
    g = np.stack(np.meshgrid(*(np.arange(s) for s in size), indexing="ij"), -1).reshape(-1, 3)
    hi = np.asarray(size) - 1
    on_face = ((g == 0) | (g == hi)).any(1)
    corner = ((g == 0) | (g == hi)).all(1)
    rest = g[on_face & ~corner]
    assert 8 <= n <= 8 + len(rest)
    pts = np.concatenate([g[corner], rest[rng.permutation(len(rest))[:n - 8]]])
    return _frozen(pts[rng.permutation(n)])


def two_examples(coords):
    """[n, 3] -> [n, 4]: the first half as example 0, the second half moved onto the coordinates of the first as
    example 1 (the examples share coordinates; no rule may cross them)"""
    n = coords.shape[0]
    h = (n + 1) // 2
    c = np.concatenate([coords, np.zeros((n, 1), np.int64)], 1)
    c[h:, :3] = coords[:n - h]
    c[h:, 3] = 1
    return _frozen(c)


def with_batch(coords):
    return _frozen(np.concatenate([coords, np.zeros((coords.shape[0], 1), np.int64)], 1))


@functools.lru_cache(maxsize=None)
def duplicated_points(n_points, seed, fill=0.4):
    """a point list with duplicates: ceil(n_points / 2) distinct voxels of a blob, every other point a repeat of one
    of them, shuffled -> int64 [n_points, 4]"""
    rng = np.random.RandomState(seed + 7)
    sites = blob((n_points + 1) // 2, seed, fill)
    pts = np.concatenate([sites, sites[rng.randint(0, sites.shape[0], n_points - sites.shape[0])]])
    return with_batch(pts[rng.permutation(n_points)])


# name -> (filter, stride, input size, output size); the grids hold 16384 output cells, so that 8193 outputs fit
GEOMETRIES = {
    "f2s2": ((2, 2, 2), (2, 2, 2), (64, 64, 32), (32, 32, 16)),
    "f3s2": ((3, 3, 3), (2, 2, 2), (65, 65, 33), (32, 32, 16)),
    "proj4": ((1, 1, 4), (1, 1, 1), (128, 128, 4), (128, 128, 1)),
    "proj16": ((1, 1, 16), (1, 1, 1), (128, 128, 16), (128, 128, 1)),
    "proj32": ((1, 1, 32), (1, 1, 1), (128, 128, 32), (128, 128, 1)),
}


def max_out(filt, stride, out_size):
    """candidate outputs per input site (the grid chain's entry bound per site)"""
    return int(np.prod([min((f + s - 1) // s, o) for f, s, o in zip(filt, stride, out_size)]))


def _outputs_of(p, filt, stride, out_size):
    rng = []
    for d in range(3):
        t = p[d] - filt[d] + stride[d]
        lo = 0 if t < 0 else t // stride[d]
        rng.append(range(lo, min(out_size[d] - 1, p[d] // stride[d]) + 1))
    return list(itertools.product(*rng))


@functools.lru_cache(maxsize=None)
def strided_scene(name, n_out, seed):
    """input sites int64 [n, 4] of geometry `name` with exactly n_out output sites: random voxels of a box that holds
    about 1.5 n_out output cells, taken in random order while they keep the output count within n_out, up to
    3 n_out + 8 sites (never fewer sites than outputs)"""
    filt, stride, size, out_size = GEOMETRIES[name]
    rng = np.random.RandomState(seed)
    cells = max(1.5 * n_out, 1.0)
    oa, ob, oc = _box(cells, zmax=out_size[2])
    box = [min(size[d], o * stride[d] + filt[d] - stride[d]) for d, o in enumerate((oa, ob, oc))]
    g = np.stack(np.meshgrid(*(np.arange(b) for b in box), indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.permutation(len(g))]
    outs, pts = set(), []
    for p in g:
        o = _outputs_of(p, filt, stride, out_size)
        if len(outs) + sum(1 for c in o if c not in outs) <= n_out:
            outs.update(o)
            pts.append(p)
        if len(pts) >= 3 * n_out + 8:
            break
    assert len(outs) == n_out <= len(pts), (name, n_out, len(outs), len(pts))
    return with_batch(np.array(pts, np.int64))


@functools.lru_cache(maxsize=None)
def fine_scene(name, n_in, seed):
    """n_in input sites of geometry `name` (the rows of its deconvolution view): a blob inside the input grid"""
    size = GEOMETRIES[name][2]
    pts = blob(n_in, seed, 0.4, zmax=size[2])
    assert (pts.max(0) < np.asarray(size)).all()
    return with_batch(pts)


# ---- the cases of tests/test_plan_forms_gpu.py (their scene conditions are asserted in tests/test_plan_forms_cpu.py) ----
# one site; a block, a probe workgroup, a transpose tile, the single-workgroup sort, each - 1 / exact / + 1; several radix tiles
SUBM_COUNTS = (1, BLOCK - 1, BLOCK, BLOCK + 1, NBR_SITES - 1, NBR_SITES, NBR_SITES + 1, TP - 1, TP, TP + 1,
               SMALL_MAX - 1, SMALL_MAX, SMALL_MAX + 1, 20000)
assert SUBM_COUNTS[-1] > 9 * RADIX_TILE
SUBM_FILTERS = ((3, 3, 3), (3, 3, 1), (1, 1, 3))
EXTRA_COUNTS = (129, 8193)                   # border and two-example scenes
PREFETCH_POINTS = (1, 33, 2049, 9000, 20000)
STRIDED_OUT_COUNTS = (1, 32, 33, 8192, 8193)
DECONV_IN_COUNTS = (33, 8193)
IDENTITY_COUNTS = (1, 32, 33, 8193)


def subm_scene(scene, n):
    """-> coords int64 [n, 4] (distinct voxels: site i is row i), grid size"""
    if scene == "blob":
        return with_batch(blob(n, n)), SUBM_SIZE
    if scene == "structured":
        return with_batch(structured(n, n)), SUBM_SIZE
    if scene == "border":
        return with_batch(border(n, n)), (64, 64, 32)
    assert scene == "two", scene
    return two_examples(blob(n, n + 1)), SUBM_SIZE


@functools.lru_cache(maxsize=None)
def subm_reference(scene, n, filt):
    """-> nbr[n, K], masks, rule count of the oracle for subm_scene(scene, n) (shared, never modified)"""
    import oracle
    coords, _ = subm_scene(scene, n)
    _, loc = oracle.input_sites(coords)
    assert np.array_equal(loc, coords)           # distinct voxels: numbered in input order
    nbr, total = subm_table(loc, filt)
    nbr.setflags(write=False)
    return nbr, masks_of(nbr), total


@functools.lru_cache(maxsize=None)
def strided_reference(name, coords_key):
    """-> loc_out, nbr, nbr_dec, rule count for the scene coords_key = ("out", n_out) or ("in", n_in) of geometry name"""
    import oracle
    filt, stride, size, out_size = GEOMETRIES[name]
    coords = strided_coords(name, coords_key)
    _, loc = oracle.input_sites(coords)
    assert np.array_equal(loc, coords)
    lo, nbr, dec, nr = strided_tables(loc, filt, stride, out_size)
    for a in (lo, nbr, dec):
        a.setflags(write=False)
    return lo, nbr, dec, nr


def strided_coords(name, coords_key):
    which, n = coords_key
    return strided_scene(name, n, n) if which == "out" else fine_scene(name, n, n)
