"""The references and designed clouds of tests/celllist_forms.py without a GPU: the exact and the fp32 mode agree on
every lattice cloud (after which the GPU tests excuse no point), and every cloud meets the condition it was designed
for, asserted from the restated cell function, sorted order and table slot."""
import numpy as np
import pytest

from tests import celllist_forms as F


def _both(L, e, r):
    ex, fp = F.neighbours_exact(L, e, r), F.neighbours_f32(F.xyz_of(L, e), r)
    assert F.same_neighbours(ex, fp)
    return ex


# ---------------------------------------------------------------------------------------------------------- 1. shells
def test_fp32_d2_is_the_integer_d2_on_the_cube():
    L, e = F.shells()
    x = F.xyz_of(L, e)
    for a in range(0, len(L), 256):
        d = L[None, :, :] - L[a:a + 256, None, :]
        want = ((d * d).sum(-1).astype(np.float64) * 4.0 ** -e).astype(np.float32)
        got = F.d2_bits_f32(x[None, :, :], x[a:a + 256, None, :])
        assert np.array_equal(got, F.bits(want).astype(np.int64))


@pytest.mark.parametrize("r", F.SHELL_RADII)
def test_shells_modes_agree(r):
    L, e = F.shells()
    nb = _both(L, e, r)
    count = F.count_ref(nb)
    if r == 3.0 / 32.0:
        # every point has a candidate at exactly d2 == r2, an interior one sees 123, a corner 29
        assert all(k[-1] == 9 for k in nb.key) and F.r2_lattice(r, e) == 9
        assert count.max() == 123 and count.min() == 29
        assert int(F.cut_has_tie(nb, 21).sum()) == 1704            # k = 20: the cut falls inside a shell
        interior = count == 123
        assert not F.cut_has_tie(nb, 19)[interior].any() and F.cut_has_tie(nb, 21)[interior].all()
        # the numbers of neighbours k - 1, k and k + 1 all occur among the k (and max_nn) of the case
        for k in (27, 28, 29):
            assert (count - 1 == 28).any() and k in F.SHELL_K and k + 1 in F.SHELL_NN
        assert {18, 20} <= set(F.SHELL_K) and {19, 21} <= set(F.SHELL_NN)
    elif r == 1.0 / 64.0:
        assert (count == 1).all()
    elif r == 1000.0:
        assert (count == len(L)).all()
        cells, _, _ = F.cells_of(F.xyz_of(L, e), r)
        assert (cells == 0).all() and len(L) > F.K_BUDGET          # one cell, every query unstaged
    else:
        assert F.r2_lattice(r, e) == 10 and float(F.r2_f32(r)) * 1024.0 != 10.0            # off the lattice: the shell of d2 = 10
        assert count.max() == 147


# --------------------------------------------------------------------------------------------------- 2. staging budget
@pytest.mark.parametrize("m", F.BLOB_SIZES)
def test_blob_is_one_cell_of_exactly_m(m):
    L, e = F.blob(m)
    assert len(L) == m
    cells, _, _ = F.cells_of(F.xyz_of(L, e), F.BLOB_R)
    assert (cells == 0).all() and (F.walk_totals(cells) == m).all()
    assert len(np.unique(L, axis=0)) < m                           # coincident points
    nb = _both(L, e, F.BLOB_R)
    count = F.count_ref(nb)
    assert count.min() < count.max() <= m
    assert sum(int((k == F.r2_lattice(F.BLOB_R, e)).sum()) for k in nb.key) > 0     # pairs at exactly d == r
    assert F.cut_has_tie(nb, 21).sum() > 20 and F.cut_has_tie(nb, 50).sum() > 20


def test_budget_edges():
    assert [m <= F.K_BUDGET for m in F.BLOB_SIZES] == [True, True, False, False]


# ----------------------------------------------------------------------------------------------------- 3. walk geometry
def test_walk_cells_and_spans():
    L, e = F.walk()
    assert len(L) == 129
    cells, _, _ = F.cells_of(F.xyz_of(L, e), F.BLOB_R)
    order = F.sorted_order(cells)
    cx = cells[order, 0]
    assert (cells[:, 1:] == 0).all()
    sizes = np.bincount(cx)
    assert tuple(sizes) == F.WALK_CELLS and {1, 7, 8, 9, 15, 16, 17, 33} <= set(sizes)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    assert any(f < 64 < f + s for f, s in zip(first, sizes))       # a cell straddles position 64
    assert 128 in first and len(L) - 128 == 1                      # a cell starts on 128: the last workgroup's only query
    _both(L, e, F.BLOB_R)
    for n in F.WALK_N:
        Ln, _ = F.walk(n)
        assert len(Ln) == n
        _both(Ln, e, F.BLOB_R)


# ---------------------------------------------------------------------------------------------------- 4. cell arithmetic
@pytest.mark.parametrize("where", sorted(F.ARITH_SHIFTS))
def test_arith_pairs_cross_faces_edges_and_corners(where):
    L, e, pairs = F.arith(F.ARITH_SHIFTS[where])
    x = F.xyz_of(L, e)
    cells, _, _ = F.cells_of(x, F.ARITH_R)
    steps = {tuple(cells[c] - cells[p]) for p, c in pairs}
    assert steps == set(F.arith_dirs())                            # every direction, one cell away
    nb = _both(L, e, F.ARITH_R)
    for p, c in pairs:
        assert list(nb.idx[p]) == [p, c] and nb.key[p][1] == 225 == F.r2_lattice(F.ARITH_R, e)
    if where == "negative":
        assert (x < 0).all()
    if where == "far":
        assert (x >= 4000.0).all()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_past_r_needs_the_margin_of_the_cell_edge(axis):
    x, r = F.past_r(axis)
    lo, p, c = (float(v) for v in x[:, axis])
    assert c - p > r and np.float32(x[2, axis] - x[1, axis]) == np.float32(r)     # past r in the reals, r in fp32
    nb = F.neighbours_f32(x, r)
    assert [list(j) for j in nb.idx] == [[0, 1], [1, 0, 2], [2, 1]]
    assert nb.key[1][2] == F.r2_bits(r)
    cells, _, h = F.cells_of(x, r)
    assert list(cells[:, axis]) == [0, 0, 1] and h == r * 1.0001
    assert list(np.floor((x[:, axis].astype(np.float64) - lo) / r)) == [0.0, 0.0, 2.0]      # with cells of edge r


# ------------------------------------------------------------------------------------------------ 5. keys and the clamp
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_clamp_clusters(axis):
    L, e = F.clamp(axis)
    x = F.xyz_of(L, e)
    cells, _, h = F.cells_of(x, F.CLAMP_R)
    with np.errstate(all="ignore"):
        raw = np.floor(x.astype(np.float64)[:, axis] / h)          # the minimum is 0
    ca = cells[:, axis]
    assert ((ca > (1 << 17)) & (ca < F.K_CELL_MAX - 1)).any()
    assert (ca == F.K_CELL_MAX - 1).any() and ((ca == F.K_CELL_MAX) & (raw == F.K_CELL_MAX)).any()
    assert ((ca == F.K_CELL_MAX) & (raw > F.K_CELL_MAX + 900)).any()         # merged into the last cell
    keys = F.cell_keys(cells)
    assert axis == 2 or (keys >> np.uint64(32)).max() > 0          # x and y cells reach the key's high word
    nb = _both(L, e, F.CLAMP_R)
    # neighbours across the boundary between cells kCellMax - 1 and kCellMax
    assert any(ca[i] == F.K_CELL_MAX - 1 and (ca[j] == F.K_CELL_MAX).any() for i, j in enumerate(nb.idx))


# -------------------------------------------------------------------------------------------------------------- 6. table
@pytest.mark.parametrize("cap", [1024, 8192])
def test_table_wraps(cap):
    L, e, wrapped, empty = F.table(cap)
    assert F.table_cap(len(L)) == cap
    x = F.xyz_of(L, e)
    cells, _, _ = F.cells_of(x, F.TABLE_R)
    have = {tuple(c) for c in cells}
    assert all(tuple(c) in have for c in wrapped) and tuple(empty) not in have
    assert tuple(empty + np.array([1, 0, 0])) in have              # the empty cell is somebody's neighbour
    tab = F.table_of(F.cell_keys(cells), cap)
    wk = F.cell_keys(wrapped)
    assert (F.cell_slot(wk, cap) == cap - 1).all()
    assert {cap - 1, 0, 1} <= set(tab)                             # three keys from the last slot on: the chain wraps
    ends = [F.probe_chain(tab, cap, k) for k in wk]               # which key gets which slot depends on arrival order;
    assert sum(1 for c in ends if c[0] == cap - 1 and c[-1] < 8 and 0 in c) == 2       # two of the three wrap to slot 0
    chain = F.probe_chain(tab, cap, F.cell_keys(empty[None, :])[0])
    assert chain[0] == cap - 1 and len(chain) >= 4 and chain[-1] not in tab and 0 in chain
    nb = _both(L, e, F.TABLE_R)
    assert (F.count_ref(nb)[[i for i, c in enumerate(cells) if tuple(c) in {tuple(w) for w in wrapped}]] == 2).all()


# -------------------------------------------------------------------------------------------------------- 7. deep unions
@pytest.mark.parametrize("doubled", [False, True])
def test_chains(doubled):
    L, e = F.chains(doubled=doubled)
    nb = _both(L, e, F.CHAIN_R)
    label, size = F.components_ref(nb)
    mult = 2 if doubled else 1
    assert [int(v) for v in np.unique(size)] == [499 * mult, 501 * mult, 1000 * mult] and len(np.unique(label)) == 3
    assert any((k == 100).any() for k in nb.key)                   # a link at exactly r


# --------------------------------------------------------------------------------------------------- 8. non-finite rows
@pytest.mark.parametrize("name", sorted(F.NONFINITE))
def test_nonfinite_rows_by_the_fp32_definition(name):
    L, e = F.shells(6)
    base = F.xyz_of(L, e)
    x, src = F.with_rows(base, F.NONFINITE[name])
    r = F.SHELL_RADII[0]
    nb, nb0 = F.neighbours_f32(x, r), F.neighbours_f32(base, r)
    bad = src < 0
    assert bad.sum() == len(F.NONFINITE[name])
    count = F.count_ref(nb)
    assert (count[bad] == 0).all() and np.array_equal(count[~bad], F.count_ref(nb0)[src[~bad]])
    mean, found = F.knn_ref(nb, 5)
    assert (found[bad] == -1).all() and np.isinf(mean[bad]).all()
    label, size = F.components_ref(nb)
    assert np.array_equal(label[bad], np.flatnonzero(bad)) and (size[bad] == 1).all()
    assert all(np.array_equal(np.sort(src[j]), np.sort(j0)) for j, j0 in zip([nb.idx[i] for i in np.flatnonzero(~bad)],
                                                          [nb0.idx[i] for i in src[~bad]]))
    cells, lo, _ = F.cells_of(x, r)
    if name.startswith("ninf"):
        axes = [0] if name == "ninf_x" else [1, 2]
        assert all(np.isneginf(lo[a]) and (cells[~bad, a] == F.K_CELL_MAX).all() for a in axes)
    index, dist2 = F.nearest_ref(base, x, r)
    assert (index[bad] == -1).all() and np.isinf(dist2[bad]).all() and np.array_equal(index[~bad], src[~bad])


# ------------------------------------------------------------------------------------------------------- 9. plane links
def test_plane_offsets_hit_the_threshold():
    L, e = F.shells()
    x = F.xyz_of(L, e)
    nb = F.neighbours_exact(L, e, F.SHELL_RADII[0])
    v = F.plane_normals(len(L))
    assert np.isnan(v).any(1).sum() == 1 and (v == 0).all(1).sum() == 1
    sizes = {}
    for cm in F.PLANE_COS:
        for off in (0.0, 1.0 / 32.0):
            label, size, eP, ok = F.plane_links_ref(nb, x, v, cm, off)
            assert (eP == np.float32(off)).any() and ok.any() and not ok.all()
            sizes[cm, off] = int(size.max())
    assert len(set(sizes.values())) >= 4, sizes                    # the thresholds matter


# ---------------------------------------------------------------------------------------------------------- normals
def _angles(a, b):
    return np.arcsin(np.minimum(1.0, np.linalg.norm(np.cross(a, b), axis=1)))


def test_staircase_depends_on_the_tie_rule():
    L, e = F.staircase()
    nb = _both(L, e, F.STAIR_R)
    assert F.cut_has_tie(nb, F.STAIR_NN).sum() >= 100
    lowest, c0, g0, f0 = F.normals_ref(nb, L, F.STAIR_NN)
    highest, c1, g1, f1 = F.normals_ref(nb, L, F.STAIR_NN, tie="high")
    sel = ~f0 & ~f1 & (g0 >= 1e-2) & (g1 >= 1e-2)
    moved = _angles(lowest[sel], highest[sel]) > 1e-5 / np.minimum(g0[sel], g1[sel])
    assert int(moved.sum()) >= 50, int(moved.sum())


def test_shell_normals_have_points_to_compare():
    L, e = F.shells()
    nb = F.neighbours_exact(L, e, F.SHELL_RADII[0])
    for nn in F.SHELL_NN:
        _, count, gap, flat = F.normals_ref(nb, L, nn)
        assert (count == np.minimum(F.count_ref(nb), nn)).all() and not flat.any()
        assert ((gap >= 1e-2).sum()) >= 300


def test_coincident_points_are_flat():
    L = np.array([[5, 5, 5]] * 4 + [[5, 5, 6]] * 2 + [[90, 90, 90]])
    nb = _both(L, 5, 1.0 / 64.0)
    _, count, _, flat = F.normals_ref(nb, L, 30)
    assert list(count) == [4, 4, 4, 4, 2, 2, 1] and flat.all()


# ---------------------------------------------------------------------------------------------------------- 10. nearest
def test_nearest_queries_shells():
    L, e = F.shells()
    x, r = F.xyz_of(L, e), F.SHELL_RADII[0]
    q = F.nearest_queries_shells(L)
    cells, lo, h = F.cells_of(x, r)
    qc, raw = F.query_cells_of(q, lo, h)
    assert (raw == -1).any() and (raw < -1).any() and (qc >= -1).all()
    index, dist2 = F.nearest_ref(x, q, r)
    assert (index >= 0).sum() > 300 and (index < 0).sum() > 10
    assert (F.bits(dist2) == F.r2_bits(r)).any()            # a query at exactly r
    # a tie at the smallest d2 between rows of different cells
    K = F.d2_bits_f32(x[None, :, :], q[:, None, :])
    tied = 0
    for t in np.flatnonzero(index >= 0):
        rows = np.flatnonzero(K[t] == K[t].min())
        assert index[t] == rows.min()
        tied += len(rows) > 1 and len({tuple(c) for c in cells[rows]}) > 1
    assert tied >= 20


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_nearest_queries_clamp(axis):
    L, e = F.clamp(axis)
    x = F.xyz_of(L, e)
    q = F.nearest_queries_clamp(axis)
    _, lo, h = F.cells_of(x, F.CLAMP_R)
    qc, raw = F.query_cells_of(q, lo, h)
    assert (raw[:, axis] > F.K_CELL_MAX).any() and (raw < -1).any() and (raw == -1).any()
    index, _ = F.nearest_ref(x, q, F.CLAMP_R)
    far = raw[:, axis] > F.K_CELL_MAX
    assert (index[far] >= 0).any() and (index[far] < 0).any() and (index[raw[:, axis] < 0] >= 0).any()


# -------------------------------------------------------------------------------------------------------------- helpers
def test_stats_of():
    assert F.stats_of([np.inf, np.inf]) == (0.0, 0.0) and F.stats_of([np.inf, 2.5]) == (2.5, 0.0)
    mu, sigma = F.stats_of([1.0, 2.0, 3.0, np.inf])
    assert mu == 2.0 and sigma == 1.0
