"""Exact references and designed clouds for the cell-list queries (csrc/celllist.hip, csrc/cell_walk.inc,
csrc/union_find.inc behind d3d_radius_neighbors, d3d_knn_mean_distance, d3d_connected_components, d3d_estimate_normals,
d3d_segment_planes and d3d_nearest), in the style of tests/tail_forms.py.

Every cloud lies on a lattice: row i is L[i] * 2^-e with integer L, |L| < 2^24, so the fp32 coordinates are exact, the
fp32 offsets C - P are exact and, the library being built with -ffp-contract=off, the kernel's
d2 = (dx dx + dy dy) + dz dz is the exact dyadic number |dL|^2 4^-e wherever that fits 24 bits.  The reference is brute
force over all pairs in two modes:

  exact   integer lattice offsets and the integer d2; the radius enters as the exact rational fl32(r * r), as the
          integer floor(fl32(r r) 4^e)
  fp32    the kernel's formula in numpy.float32, operation by operation, compared through the bit patterns as
          dist2_bits does; this mode also takes rows that are not finite

tests/test_celllist_forms_cpu.py asserts that the two agree on every lattice cloud (the same candidates in the same
(d2, row) order with the same d2), so the GPU tests excuse no point.  The cell coordinate, the sorted order and the table
slot are restated too, but only to design and certify the inputs (which cell a point falls in, which slot a key hashes
to); none of them decides an expected result."""
import math

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components as _cc

from tests.normals_ref import canonical_sign

K_CELL_BITS = 20
K_CELL_MAX = (1 << K_CELL_BITS) - 1
K_SPAN = 64
K_BUDGET = 1024
CHUNK = 256
NO_KEY = np.iinfo(np.int64).max


def bits(a):
    return np.atleast_1d(np.ascontiguousarray(a, np.float32)).view(np.uint32).reshape(np.shape(a) or (1,))


def xyz_of(L, e):
    """the fp32 rows of the lattice points L 2^-e, exact"""
    L = np.asarray(L, np.int64)
    assert np.abs(L).max(initial=0) < (1 << 24)
    x = (L.astype(np.float64) * 2.0 ** -e).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * 2.0 ** e, L)
    return x


def r2_f32(r):
    r = np.float32(r)
    with np.errstate(all="ignore"):                    # the product may overflow to +inf or underflow to 0, as the library's
        return np.float32(r * r)


def r2_bits(r):
    return int(bits(r2_f32(r))[0])


def r2_lattice(r, e):
    """the largest integer d2 (units of 4^-e) with d2 4^-e <= fl32(r r); the scaling by a power of two is exact"""
    return math.floor(float(r2_f32(r)) * 4.0 ** e)


# ------------------------------------------------------------------------------------------------------ neighbourhoods
class Neighbours:
    """idx[i]: the rows within r of row i, row i among them, sorted by (d2, row); key[i]: their d2 as an integer (exact:
    lattice units; fp32: the bit pattern); d2[i]: the same as real numbers, fp64"""

    def __init__(self, idx, key, d2):
        self.idx, self.key, self.d2 = idx, key, d2
        self.n = len(idx)


def _lists(n, keys_of, limit):
    idx, key = [], []
    for a in range(0, n, CHUNK):
        K = keys_of(a, min(n, a + CHUNK))
        W = K <= limit
        for t in range(K.shape[0]):
            j = np.flatnonzero(W[t])
            k = K[t, j]
            o = np.lexsort((j, k))
            idx.append(j[o])
            key.append(k[o])
    return idx, key


def neighbours_exact(L, e, r):
    L = np.asarray(L, np.int64)

    def keys_of(a, b):
        d = L[None, :, :] - L[a:b, None, :]
        return (d * d).sum(-1)

    idx, key = _lists(L.shape[0], keys_of, r2_lattice(r, e))
    return Neighbours(idx, key, [k.astype(np.float64) * 4.0 ** -e for k in key])


def d2_bits_f32(C, P):
    """dist2_bits of cell_walk.inc on broadcastable fp32 arrays [..., 3] -> int64 bit patterns"""
    C, P = np.asarray(C, np.float32), np.asarray(P, np.float32)
    with np.errstate(all="ignore"):
        dx, dy, dz = C[..., 0] - P[..., 0], C[..., 1] - P[..., 1], C[..., 2] - P[..., 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    return np.ascontiguousarray(d2).view(np.uint32).astype(np.int64)


def neighbours_f32(xyz, r):
    x = np.asarray(xyz, np.float32)
    idx, key = _lists(x.shape[0], lambda a, b: d2_bits_f32(x[None, :, :], x[a:b, None, :]), r2_bits(r))
    return Neighbours(idx, key, [k.astype(np.uint32).view(np.float32).astype(np.float64) for k in key])


def same_neighbours(A, B):
    """the two modes list the same rows in the same order with the same d2"""
    return A.n == B.n and all(np.array_equal(a, b) for a, b in zip(A.idx, B.idx)) and \
        all(np.array_equal(a, b) for a, b in zip(A.d2, B.d2))


# ------------------------------------------------------------------------------------------------------------- outputs
def count_ref(nb):
    return np.array([len(j) for j in nb.idx], np.int32)


def knn_ref(nb, k):
    """-> (mean fp64 [n], found int32 [n]): the k + 1 nearest by (d2, row), the point itself among them"""
    mean, found = np.full(nb.n, np.inf), np.zeros(nb.n, np.int32)
    for i in range(nb.n):
        d2 = nb.d2[i][:k + 1]
        found[i] = len(d2) - 1
        if found[i] >= k:
            mean[i] = math.fsum(math.sqrt(v) for v in d2) / k
    return mean, found


def cut_has_tie(nb, want):
    """bool [n]: more than `want` candidates, and the want-th and (want + 1)-th tie"""
    return np.array([len(k) > want and k[want - 1] == k[want] for k in nb.key])


def labels_of(n, a, b):
    """the components of the undirected graph with edges a[t] - b[t] -> (label: the lowest row, size)"""
    g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n))
    _, comp = _cc(g, directed=False)
    first = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(first, comp, np.arange(n))
    return first[comp].astype(np.int32), np.bincount(comp)[comp].astype(np.int32)


def pairs_of(nb):
    i = np.repeat(np.arange(nb.n), [len(j) for j in nb.idx])
    j = np.concatenate(nb.idx) if nb.n else np.zeros(0, np.int64)
    return i, j


def components_ref(nb):
    return labels_of(nb.n, *pairs_of(nb))


def normals_ref(nb, L, max_nn, viewpoint=None, tie="low"):
    """-> (normal fp64 [n, 3], count int32 [n], gap [n], flat bool [n]).  The kept set is the first max_nn of (d2, row)
    (tie='high': of (d2, -row), the mutation the staircase case is designed against); the covariance comes from the
    integer offsets; gap = (l1 - l0) / l2; flat: count < 3 or all kept points coincide, where (0, 0, 1) is required.
    viewpoint: in lattice units."""
    L = np.asarray(L, np.int64)
    n = nb.n
    normal, count = np.tile(np.array([0.0, 0.0, 1.0]), (n, 1)), np.zeros(n, np.int32)
    gap, flat = np.full(n, np.inf), np.ones(n, bool)
    for i in range(n):
        j = nb.idx[i]
        if tie == "high":
            j = j[np.lexsort((-j, nb.key[i]))]
        j = j[:max_nn]
        count[i] = len(j)
        if len(j) < 3:
            continue
        q = (L[j] - L[i]).astype(np.float64)
        c = q - q.mean(0)
        w, v = np.linalg.eigh(c.T @ c / len(j))
        if not w[2] > 0:
            continue
        flat[i] = False
        gap[i] = (w[1] - w[0]) / w[2]
        nv = v[:, 0] / np.linalg.norm(v[:, 0])
        if viewpoint is None:
            nv = canonical_sign(nv)
        elif np.dot(nv, np.asarray(viewpoint, np.float64) - L[i]) < 0:
            nv = -nv
        normal[i] = nv
    return normal, count, gap, flat


def plane_links_ref(nb, xyz, nrm, cos_min, offset):
    """PlaneLinkQuery's three tests in fp32 as the kernel writes them -> (label, size, eP [pairs], linked [pairs])"""
    x, v = np.asarray(xyz, np.float32), np.asarray(nrm, np.float32)
    i, j = pairs_of(nb)
    P, C, nP, nC = x[i], x[j], v[i], v[j]
    cm, off = np.float32(cos_min), np.float32(offset)
    with np.errstate(all="ignore"):
        dx, dy, dz = C[:, 0] - P[:, 0], C[:, 1] - P[:, 1], C[:, 2] - P[:, 2]
        c = (nP[:, 0] * nC[:, 0] + nP[:, 1] * nC[:, 1]) + nP[:, 2] * nC[:, 2]
        eP = np.abs((nP[:, 0] * dx + nP[:, 1] * dy) + nP[:, 2] * dz)
        eC = np.abs((nC[:, 0] * dx + nC[:, 1] * dy) + nC[:, 2] * dz)
        ok = (np.abs(c) >= cm) & (eP <= off) & (eC <= off)
    assert c.dtype == eP.dtype == np.float32
    label, size = labels_of(nb.n, np.concatenate([i[ok], np.arange(nb.n)]), np.concatenate([j[ok], np.arange(nb.n)]))
    return label, size, eP, ok


def nearest_ref(cloud, query, r):
    """-> (index int32 [m], dist2 fp32 [m]): the minimum over (bits of d2, row) among d2 <= r2; -1 and +inf for none"""
    c, q = np.asarray(cloud, np.float32), np.asarray(query, np.float32)
    m, n = q.shape[0], c.shape[0]
    index, dist2 = np.full(m, -1, np.int32), np.full(m, np.inf, np.float32)
    lim = r2_bits(r)
    for a in range(0, m if n else 0, CHUNK):
        K = d2_bits_f32(c[None, :, :], q[a:a + CHUNK, None, :])
        key = np.where(K <= lim, K * (1 << 31) + np.arange(n)[None, :], NO_KEY)
        best = key.argmin(1)
        hit = key[np.arange(len(best)), best] != NO_KEY
        index[a:a + CHUNK][hit] = best[hit]
        dist2[a:a + CHUNK][hit] = K[np.arange(len(best)), best][hit].astype(np.uint32).view(np.float32)
    return index, dist2


def stats_of(mean):
    """(mu, sigma) of the finite means with exactly rounded sums"""
    v = [float(x) for x in mean if math.isfinite(x)]
    if not v:
        return 0.0, 0.0
    mu = math.fsum(v) / len(v)
    return mu, (math.sqrt(math.fsum((x - mu) ** 2 for x in v) / (len(v) - 1)) if len(v) > 1 else 0.0)


# --------------------------------------------------------------------------- the build, restated to certify the inputs
def cells_of(xyz, r):
    """k_cell_coords: floor((p - min) / ((double)r 1.0001)) per axis in fp64, clamped; anything unordered -> 0"""
    x = np.asarray(xyz, np.float32)
    h = float(np.float32(r)) * 1.0001
    lo = np.fmin.reduce(x, axis=0, initial=np.float32(np.inf)).astype(np.float32)          # fminf drops a NaN
    with np.errstate(all="ignore"):
        q = np.floor((x.astype(np.float64) - lo.astype(np.float64)) / h)
        c = np.where(q >= 0.0, np.where(q < K_CELL_MAX, q, K_CELL_MAX), 0.0)
    return c.astype(np.int64), lo, h


def query_cells_of(query, lo, h):
    """query_cell of register.hip: clamped to [-1, kCellMax]; anything unordered -> -1"""
    with np.errstate(all="ignore"):
        q = np.floor((np.asarray(query, np.float32).astype(np.float64) - lo.astype(np.float64)) / h)
        c = np.where(q >= 0.0, np.where(q < K_CELL_MAX, q, K_CELL_MAX), -1.0)
    return c.astype(np.int64), q


def sorted_order(cells):
    """(cx, cy, cz, row)"""
    return np.lexsort((np.arange(cells.shape[0]), cells[:, 2], cells[:, 1], cells[:, 0]))


def cell_keys(cells):
    c = cells.astype(np.uint64)
    return (c[:, 0] << np.uint64(40)) | (c[:, 1] << np.uint64(20)) | c[:, 2]


def table_cap(n):
    c = 1024
    while c < 2 * n:
        c <<= 1
    return c


def cell_slot(keys, cap):
    """the 64-bit finaliser of d3d_internal.h, masked to cap"""
    c = np.array(keys, np.uint64, ndmin=1)
    with np.errstate(over="ignore"):
        c = c ^ (c >> np.uint64(33))
        c = c * np.uint64(0xff51afd7ed558ccd)
        c = c ^ (c >> np.uint64(33))
        c = c * np.uint64(0xc4ceb9fe1a85ec53)
        c = c ^ (c >> np.uint64(33))
    return (c & np.uint64(0xffffffff) & np.uint64(cap - 1)).astype(np.int64)


def table_of(keys, cap):
    """linear probing of the distinct keys -> {slot: key}; which slots end up taken does not depend on the order"""
    tab = {}
    for k in np.unique(np.asarray(keys, np.uint64)):
        s = int(cell_slot(k, cap)[0])
        while s in tab:
            s = (s + 1) & (cap - 1)
        tab[s] = int(k)
    return tab


def probe_chain(tab, cap, key):
    """the slots cell_range reads for `key`, the last one holding it or empty"""
    s, chain = int(cell_slot(key, cap)[0]), []
    while True:
        chain.append(s)
        if s not in tab or tab[s] == int(key):
            return chain
        s = (s + 1) & (cap - 1)


def walk_totals(cells):
    """per row: the points in the 27 cells around its own (what k_cln_walk stages, or does not)"""
    uniq, inv, cnt = np.unique(cells, axis=0, return_inverse=True, return_counts=True)
    table = {tuple(c): int(m) for c, m in zip(uniq, cnt)}
    tot = np.zeros(len(uniq), np.int64)
    for u, c in enumerate(uniq):
        tot[u] = sum(table.get((c[0] + a, c[1] + b, c[2] + d), 0) for a in (-1, 0, 1) for b in (-1, 0, 1) for d in (-1, 0, 1))
    return tot[inv.reshape(-1)]


# -------------------------------------------------------------------------------------------------------------- clouds
def _permuted(L, seed):
    return np.asarray(L, np.int64)[np.random.RandomState(seed).permutation(len(L))]


# 1. shells: a 12^3 cube, spacing 1/32, offset (13.75, -4.25, 1.125), rows permuted
SHELL_E = 5
SHELL_RADII = (3.0 / 32.0, float(np.float32(0.1)), 1.0 / 64.0, 1000.0)
SHELL_K = (18, 20, 27, 28, 29)            # r = 3/32: interior shells end at 1, 7, 19, 27, 33, 57, 81, 93, 123 candidates;
SHELL_NN = (19, 21, 28, 29, 30)           # a corner has 29.  want = k + 1 = max_nn: 19 a shell edge, 21 inside a shell


def shells(side=12):
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return _permuted(g + np.array([440, -136, 36]), 1), SHELL_E


# 2. staging budget: one blob inside one cell, r = 1/8 on a lattice of 2^-10 (a cell is 128.0128 steps wide)
BLOB_E = 10
BLOB_R = 1.0 / 8.0
BLOB_SIZES = (1023, 1024, 1025, 2048)


def blob(m, seed=0, span=100, coincident=16):
    """m points of a span^3 box that starts at the cloud's minimum (so at cell 0), `coincident` of them copies; the
    corner and two points at exactly r = 128 steps from it (still inside the cell of 128.0128) come first"""
    rs = np.random.RandomState(seed + m)
    flat = rs.choice(span ** 3, m - coincident - 3, replace=False)
    L = np.stack([flat // span ** 2, (flat // span) % span, flat % span], 1)
    L = np.concatenate([np.array([[0, 0, 0], [128, 0, 0], [0, 0, 128]]), L])
    return _permuted(np.concatenate([L, L[rs.choice(len(L), coincident)]]), seed), BLOB_E


# 3. walk geometry: adjacent cells along x with these numbers of points; in sorted order the cell of 17 holds
#    positions 56 .. 72 (it straddles 64), a cell starts exactly on 128 and the last workgroup holds that query alone
WALK_CELLS = (1, 7, 8, 9, 15, 16, 17, 33, 22, 1)
WALK_N = (1, 2, 63, 64, 65, 129)


def walk(n=129, seed=3):
    rs = np.random.RandomState(seed)
    rows = []
    for c, m in enumerate(WALK_CELLS):
        base = np.array([math.ceil(c * 128.0128), 0, 0])
        local = 4 + np.stack([rs.randint(0, 110, m), rs.randint(0, 110, m), rs.randint(0, 110, m)], 1)
        if c == 0:
            local[0] = 0                   # the minimum on every axis
        rows.append(base + local)
    L = np.concatenate(rows)[:n]           # cut in sorted order: the first n keep their cells
    return _permuted(L, seed), BLOB_E


# 4. cell arithmetic: 26 pairs at exactly d = r = 15/32, one per direction, each across a face, an edge or a corner
ARITH_E = 5
ARITH_R = 15.0 / 32.0
ARITH_SHIFTS = {"origin": (0, 0, 0), "negative": (-5000, -7000, -300), "far": (128000, 128000, 128000)}   # far: 4000 m


def arith_dirs():
    return [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]


def arith(shift=(0, 0, 0)):
    """-> (L, e, pairs): rows pairs[t] = (p, c) are 15 lattice steps apart along direction arith_dirs()[t]"""
    rows, pairs = [np.zeros(3, np.int64)], []
    for t, sg in enumerate(arith_dirs()):
        nz = [a for a in range(3) if sg[a]]
        mag = {1: (15,), 2: (9, 12), 3: (10, 10, 5)}[len(nz)]
        v, local = np.zeros(3, np.int64), np.full(3, 7, np.int64)
        for a, m in zip(nz, mag):
            v[a] = sg[a] * m
            local[a] = 14 if sg[a] > 0 else 1
        base = np.array([math.ceil(c * 15.0015) for c in (4 * t + 2, 2, 2)])
        pairs.append((len(rows), len(rows) + 1))
        rows += [base + local, base + local + v]
    L = np.stack(rows) + np.array(shift)
    perm = np.random.RandomState(4).permutation(len(L))
    inv = np.argsort(perm)
    return L[perm], ARITH_E, [(int(inv[p]), int(inv[c])) for p, c in pairs]


def past_r(axis=0):
    """Three fp32 rows on one axis, the one cloud here that is off the lattice: the minimum -0.09f, P three floats below
    fl32(-0.09f + 0.1f) and C = 0.11f.  The real offset C - P exceeds r = 0.1f by 2.8e-9, the fp32 subtraction rounds it
    to r and the distance test admits it: with cells of edge r the pair would lie two cells apart, the margin of
    1.0001 r keeps it in adjacent cells (asserted on the CPU).  -> (xyz fp32 [3, 3], r)"""
    r, lo = np.float32(0.1), np.float32(-0.09)
    p = np.float32(float(lo) + float(r))
    for _ in range(3):
        p = np.nextafter(p, np.float32(-np.inf))
    x = np.zeros((3, 3), np.float32)
    x[:, axis] = (lo, p, np.float32(0.11))
    return x, float(r)


# 5. keys and the clamp: r = 3/1024 (a cell is 3.0003 steps of 2^-10); 3^3 clusters along `axis` at the minimum, past
#    cell 2^17, across the boundary between cells kCellMax - 1 and kCellMax, and 1000 cells farther out
CLAMP_E = 10
CLAMP_R = 3.0 / 1024.0
CLAMP_AT = (0, 400000, 3146038, 3149040)


def clamp(axis=0):
    g = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3)
    rows = []
    for at in CLAMP_AT:
        o = np.zeros(3, np.int64)
        o[axis] = at
        rows.append(g + o)
    return _permuted(np.concatenate(rows), 5 + axis), CLAMP_E


# 6. table: occupied cells chosen so that three keys hash to the last slot and the probing wraps to slot 0; an empty
#    cell that hashes there too, beside an occupied one
TABLE_E = 10
TABLE_R = 1.0 / 8.0


def _cell_point(c):
    """a lattice point near the middle of cell c (r = 1/8 on 2^-10: a cell is 128.0128 steps wide)"""
    return np.floor((np.asarray(c, np.float64) + 0.5) * 128.0128).astype(np.int64)


def table(cap=1024):
    """-> (L, e, wrapped cells [3, 3], empty cell [3]).  cap 8192: a 13^3 grid of 2197 further points raises n"""
    side = 40 if cap == 1024 else 72
    g = np.stack(np.meshgrid(*[np.arange(1, side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    hit = g[cell_slot(cell_keys(g), cap) == cap - 1]
    # keep hits that are no neighbours of one another, so that the cell of index 3 stays empty
    chosen = []
    for c in hit:
        if all(np.abs(c - d).max() > 2 for d in chosen):
            chosen.append(c)
        if len(chosen) == 4:
            break
    wrapped, empty = np.stack(chosen[:3]), chosen[3]
    rows = [np.zeros(3, np.int64)]
    for c in wrapped:
        p = _cell_point(c)
        rows += [p, p + np.array([77, 0, 0])]          # the second one lies in the next cell, 77 steps < r away
    rows.append(_cell_point(empty + np.array([1, 0, 0])))
    if cap > 1024:
        far = np.stack(np.meshgrid(*[np.arange(13)] * 3, indexing="ij"), -1).reshape(-1, 3) * 40
        rows += list(far + _cell_point(np.array([side + 3, 3, 3])))
    return _permuted(np.stack(rows), 6), TABLE_E, wrapped, empty


# 7. deep unions: clean_ref.make_chains on the lattice.  r = 10/32; two lines 12 steps apart; line a has steps of 9 and
#    one of exactly 10 (= r: it holds), line b steps of 9 and one of 11 (it breaks there)
CHAIN_E = 5
CHAIN_R = 10.0 / 32.0


def chains(m=1000, doubled=False):
    step_a, step_b = np.full(m - 1, 9), np.full(m - 1, 9)
    step_a[m // 3] = 10
    step_b[m // 2] = 11
    a = np.stack([np.concatenate([[0], np.cumsum(step_a)]), np.zeros(m, np.int64), np.zeros(m, np.int64)], 1)
    b = np.stack([np.concatenate([[0], np.cumsum(step_b)]), np.full(m, 12), np.zeros(m, np.int64)], 1)
    L = np.concatenate([a, b]) + np.array([96, -64, 16])
    if doubled:
        L = np.concatenate([L, L])
    return _permuted(L, 7), CHAIN_E


# 8. rows that are not finite, put between the rows of a cloud -> (xyz fp32, map: row of the new cloud -> row of the
#    old one, -1 for an inserted row)
def with_rows(xyz, rows, seed=8):
    """the old rows keep their order (so ties between them break as before), the new ones go in between"""
    x = np.asarray(xyz, np.float32)
    extra = np.asarray(rows, np.float32).reshape(-1, 3)
    n = len(x) + len(extra)
    at = np.sort(np.random.RandomState(seed).choice(n, len(extra), replace=False))
    src = np.full(n, -1, np.int64)
    src[np.setdiff1d(np.arange(n), at)] = np.arange(len(x))
    both = np.empty((n, 3), np.float32)
    both[src >= 0] = x
    both[at] = extra
    return both, src


NAN, INF = float("nan"), float("inf")
NONFINITE = {
    "nan": [(NAN, -4.0, 1.5), (14.0, NAN, 1.5), (14.0, -4.0, NAN), (NAN, NAN, NAN)],
    "pinf": [(INF, -4.0, 1.5), (14.0, INF, 1.5), (14.0, -4.0, INF)],
    "ninf_x": [(-INF, -4.0, 1.5)],
    "ninf_yz": [(14.0, -INF, 1.5), (14.0, -4.0, -INF)],
    "mixed": [(NAN, -4.0, 1.5), (INF, -4.0, 1.5), (14.0, -INF, 1.5), (-INF, INF, NAN)],
}


# 9. plane links: normals from +-e_x, +-e_y, +-e_z and (0.6, 0.8, 0); a NaN normal and a zero normal
PLANE_NORMALS = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0.6, 0.8, 0)], np.float32)
PLANE_COS = (0.0, 1.0, 0.5)


def plane_normals(n, seed=9, special=True):
    rs = np.random.RandomState(seed)
    v = PLANE_NORMALS[rs.randint(0, len(PLANE_NORMALS), n)].copy()
    if special and n >= 8:
        v[rs.randint(0, n)] = (NAN, 0.0, 1.0)
        v[rs.randint(0, n)] = (0.0, 0.0, 0.0)
    return v


# staircase: z = x // 2 over a 14 x 14 patch, spacing 1/32: with max_nn cutting inside a shell, which of the tied rows
# stay decides the normal
STAIR_E = 5
STAIR_R = 3.0 / 32.0
STAIR_NN = 10


def staircase(side=14):
    i, j = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    L = np.stack([i.reshape(-1), j.reshape(-1), i.reshape(-1) // 2], 1) + np.array([64, 32, -16])
    return _permuted(L, 10), STAIR_E


# 10. nearest: queries on the half-step lattice around the shells cube (ties between rows of different cells, queries at
#     exactly r outside the faces, below the minimum by less and by more than a cell) and around the clamped clusters
def nearest_queries_shells(L):
    """-> fp32 queries for the shells cube at r = 3/32 (lattice 2^-6)"""
    rs = np.random.RandomState(11)
    L2 = 2 * np.asarray(L, np.int64)
    lo, hi = L2.min(0), L2.max(0)
    m = min(400, len(L2))
    mid = L2[rs.choice(len(L2), m, replace=False)] + rs.randint(-1, 2, (m, 3))      # on points, edges, face centres
    out = []
    for a in range(3):
        for side, sg in ((lo, -1), (hi, 1)):
            for d in (6, 7, 5, 12, 13, 40):                                              # 6 half steps = exactly r
                q = L2[rs.choice(len(L2), 6)].copy()
                q[:, a] = side[a] + sg * d
                out.append(q)
    q = np.concatenate([mid] + out)
    return xyz_of(q, SHELL_E + 1)


def nearest_queries_clamp(axis=0):
    """-> fp32 queries around every cluster of clamp(axis) at r = 3/1024 (lattice 2^-11), past kCellMax among them"""
    rs = np.random.RandomState(12)
    out = []
    for at in CLAMP_AT + (3146038 + 500, 3149040 + 9):
        o = np.zeros(3, np.int64)
        o[axis] = 2 * at
        out.append(o + rs.randint(-7, 12, (40, 3)))
    return xyz_of(np.concatenate(out), CLAMP_E + 1)
