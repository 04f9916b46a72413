"""The designed cases of tests/tsdf_forms.py meet their design conditions, asserted on the restatements alone
(tests/tsdf_ref.py, tests/tsdf_mesh_ref.py): tests/test_tsdf_forms_gpu.py relies on every one of them to reach the
launch form it names.  No GPU.

The second invariant is asserted per tetrahedron: the plane of a triangle separates the inside corners of its
tetrahedron from the outside ones (it crosses every edge between them strictly inside the edge), so the normal has a
positive dot product with the step from the mean of the one to the mean of the other.  Over the eight corners of the
cell that holds only on smooth volumes (signs, parity): on the checkerboard every triangle fails it and on random8 2991 of
25078 do, in a restatement whose orientation is derived in exact integer arithmetic."""
import numpy as np
import pytest

from tests import tsdf_forms as F
from tests.tsdf_mesh_ref import edge_census, euler_characteristic

STAGE = 512                                               # kStageRows = kStageVerts


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _counts(name, min_weight=1):
    """-> (rows per block, vertices per block, every vertex's index inside its block)"""
    _, voxels, _ = F.case_surface(name, 9, min_weight)
    edges = F.case_mesh(name, min_weight)[3]
    rows, _ = F.per_block(voxels)
    verts, local = F.per_block(edges[:, :3])
    return rows, verts, local


def test_loader_round_trips_blocks():
    for name in ("random8", "signs", "parity"):
        blocks = F.case(name)["blocks"]
        got = F.load_case(name).blocks()
        assert np.array_equal(got[0], blocks[0]) and got[0].dtype == np.int32
        for a, b in zip(got[1:], blocks[1:]):
            if b is None:
                assert not a.any()
            else:
                assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b))
    shuffled = np.random.RandomState(0).permutation(8)
    blocks = F.case("random8")["blocks"]
    ref = F.load_ref(*[a[shuffled] for a in blocks], F.VOXEL, F.ORIGIN)
    for a, b in zip(ref.blocks(), blocks):
        assert np.array_equal(_bits(a), _bits(b))


def test_every_case_sits_off_zero_on_dyadic_ground():
    for name in F.MESH_CASES:
        c = F.case(name)
        assert c["blocks"][0].min() >= 3 and c["voxel"] == 0.25 and all(o != 0 for o in c["origin"])
    for name in ("random8", "random1", "checker", "closed", "weights", "parity"):
        D = F.case(name)["blocks"][1].astype(np.float64)
        assert (D * 16 == np.round(D * 16)).all() and (D != 0).all() and (np.abs(D) < 1).all()


def test_random8_reaches_later_rounds_every_configuration_and_every_colour_case():
    rows, verts, local = _counts("random8")
    print(f"random8: rows per block {rows.tolist()}, vertices per block {verts.tolist()}")
    assert rows.max() > STAGE and verts.max() > 3 * STAGE
    conf = np.unique(F.cell_configurations(F.case("random8")["blocks"]))
    assert len(conf) == 256
    d = F.Dense(F.case("random8")["blocks"])
    g, h = F.vertex_ends(F.case_mesh("random8")[3])
    late = local >= STAGE
    has = set(zip((d.at(d.CW, g[late]) > 0).tolist(), (d.at(d.CW, h[late]) > 0).tolist()))
    assert has == {(False, False), (False, True), (True, False), (True, True)}
    # the cuts of the guard test fall inside a later round of the last block: not on a round's first row, not in the first
    assert (rows[-1] - 5) > STAGE and (rows[-1] - 5) % STAGE != 0
    assert (verts[-1] - 5) > 2 * STAGE and (verts[-1] - 5) % STAGE != 0
    assert len(F.case_mesh("random8")[1]) > 7


def test_random1_has_no_neighbour():
    c = F.case("random1")
    assert len(c["blocks"][0]) == 1
    vertices, triangles, _, edges = F.case_mesh("random1")
    assert len(vertices) > 2 * STAGE
    g, h = F.vertex_ends(edges)
    lo = 8 * c["blocks"][0][0].astype(np.int64)
    assert ((g >= lo) & (h < lo + 8)).all()               # no vertex on an edge that leaves the block
    assert len(triangles) > 0


def _cells(name):
    """the cells that gave a triangle: the lowest corner over the ends of the edges of its three vertices"""
    _, triangles, _, edges = F.case_mesh(name)
    g, h = F.vertex_ends(edges)
    return {tuple(c) for c in np.concatenate([g[triangles], h[triangles]], 1).min(1).tolist()}


def test_corner_voxel_crosses_into_every_forward_neighbour():
    """voxel CORNER_VOXEL of block BASE owns a vertex of every kind, each on an edge that ends in another block; the twin
    without neighbour o loses the vertex that ends there and keeps the other six, and a cell that needs o is not emitted"""
    from tests.tsdf_mesh_ref import KIND_DIR
    g = 8 * np.array(F.BASE, np.int64) + np.array(F.CORNER_VOXEL, np.int64)
    kinds_of = lambda edges: sorted(edges[(edges[:, :3] == g).all(1)][:, 3].tolist())
    full_edges = F.case_mesh("corner")[3]
    assert kinds_of(full_edges) == list(range(7))
    assert all(((g + KIND_DIR[k]) // 8 != g // 8).any() for k in range(7))
    rows_at = lambda name: int((F.case_surface(name, 9)[1] == g).all(1).sum())
    assert rows_at("corner") == 3
    for o in range(1, 8):
        name = f"corner_without_{o}"
        assert len(F.case(name)["blocks"][0]) == 7
        lost = [k for k in range(7) if (KIND_DIR[k] * (1, 2, 4)).sum() == o]
        assert len(lost) == 1 and kinds_of(F.case_mesh(name)[3]) == [k for k in range(7) if k != lost[0]]
        assert rows_at(name) == (2 if lost[0] < 3 else 3)
        assert tuple(g) in _cells("corner") and tuple(g) not in _cells(name)


def test_checker_ends_on_round_boundaries():
    rows, verts, _ = _counts("checker")
    assert rows[0] == 3 * STAGE and verts[0] == 4 * STAGE  # block (0, 0, 0) of the eight has all seven forward neighbours
    assert (np.abs(F.case("checker")["blocks"][1]) == 0.5).all()


def test_closed_is_a_closed_oriented_surface():
    _, triangles, _, _ = F.case_mesh("closed")
    assert len(triangles) > 20000
    assert edge_census(triangles) == (1, 0)
    assert euler_characteristic(triangles) % 2 == 0


def test_weights_decide_seen_at_every_min_weight():
    c = F.case("weights")
    d = F.Dense(c["blocks"])
    assert c["min_weights"] == (0, 0.5, 1, 2)
    V = []
    for mw in c["min_weights"]:
        vertices, _, _, edges = F.case_mesh("weights", mw)
        rows, voxels, _ = F.case_surface("weights", 9, mw)
        V.append(len(vertices))
        g, h = F.vertex_ends(edges)
        w = np.concatenate([d.at(d.W, g), d.at(d.W, h)])
        assert not np.isnan(w).any() and not (w == -1).any()
        assert (w == 0).any() == (mw == 0)
        assert (w[~np.isinf(w)] >= mw).all() and np.isinf(w).any()
        assert len(rows) == int((edges[:, 3] < 3).sum()) > 0
    print(f"weights: V = {V} at min_weight {c['min_weights']}")
    assert V[0] > V[1] > V[2] > V[3] > 0
    for value in F.WEIGHT_VALUES:
        W = c["blocks"][2]
        assert (np.isnan(W) if np.isnan(value) else W == value).sum() > 300


def _vertex(edges, g, kind):
    """the index of the vertex (g, kind), or -1"""
    hit = np.flatnonzero((edges[:, :3] == np.asarray(g)).all(1) & (edges[:, 3] == kind))
    assert len(hit) <= 1
    return int(hit[0]) if len(hit) else -1


def test_signs_zero_is_outside_subnormals_count_and_ends_are_exact():
    c = F.case("signs")
    vertices, _, _, edges = F.case_mesh("signs")
    rows, voxels, has = F.case_surface("signs", 9)
    X = lambda x, y, z: (np.array(F.ORIGIN) + F.signs_voxel(x, y, z) * F.VOXEL).astype(np.float32)
    d = F.Dense(c["blocks"])
    line = d.at(d.D, np.array([F.signs_voxel(x, 2, 2) for x in range(4, 16)]))
    assert np.array_equal(_bits(line), _bits(F.LINE_X))   # -0.0 and the subnormals arrive as they are
    along_x = {x: _vertex(edges, F.signs_voxel(x, 2, 2), 0) for x in range(3, 15)}
    # crossings: +1|-1, -1|-0.0, +0.0|-1 (across the blocks' border), -2^-149|+0.0, 2^-149|-2^-126, -2^-126|2^-126,
    # 2^-126|-2^-149, -2^-149|+1; none: -0.0|+1, +1|+0.0, -1|-2^-149, +0.0|2^-149
    assert [x for x in sorted(along_x) if along_x[x] >= 0] == [3, 4, 7, 9, 11, 12, 13, 14]
    # 9 and 14 exist, and 8 does not, only while -2^-149 stays a negative number
    assert np.array_equal(vertices[along_x[4]], X(5, 2, 2))        # Dg < 0, Dh = -0.0: s = 1, exactly at h
    assert np.array_equal(vertices[along_x[7]], X(7, 2, 2))        # Dg = +0.0, Dh < 0: s = 0, exactly at g
    assert np.array_equal(vertices[along_x[9]], X(10, 2, 2))       # -2^-149 against +0.0: s = 1
    assert np.array_equal(vertices[along_x[12]], X(12, 2, 2) + np.float32([0.125, 0, 0]))   # -2^-126 | 2^-126: s = 1 / 2
    i = _vertex(edges, F.signs_voxel(2, 2, 5), 1)                  # Dg = -0.0, Dh = -1 along y: s = -0.0
    assert i >= 0 and np.array_equal(vertices[i], X(2, 2, 5))
    assert _vertex(edges, F.signs_voxel(2, 1, 5), 1) < 0           # +1 | -0.0
    # |D| = 1 gives rows without a normal: here every row has such a voxel among the four it needs
    assert len(rows) == int((edges[:, 3] < 3).sum()) > 20 and not has.any()
    assert np.array_equal(_bits(rows[:, :3]), _bits(vertices[edges[:, 3] < 3]))


def test_nonfinite_voxels_are_not_seen():
    bad = F.case("nonfinite")["bad"]
    d = F.Dense(F.case("nonfinite")["blocks"])
    assert (d.at(d.W, bad) == 1).all() and not np.isfinite(d.at(d.D, bad)).any()
    for value in (np.nan, np.inf, -np.inf):
        D = d.at(d.D, bad)
        assert (np.isnan(D) if np.isnan(value) else D == value).sum() == 20
    got, want = F.case_mesh("nonfinite"), F.case_mesh("nonfinite_twin")
    assert len(got[0]) < len(F.case_mesh("random8")[0])
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.isfinite(a).all() and np.array_equal(_bits(a), _bits(b))
    for columns in (3, 6, 9):
        got, want = F.case_surface("nonfinite", columns), F.case_surface("nonfinite_twin", columns)
        for a, b in zip(got, want):
            assert a.shape == b.shape and np.isfinite(a).all() and np.array_equal(a, b)
        assert np.array_equal(_bits(got[0]), _bits(want[0]))
    g, h = F.vertex_ends(F.case_mesh("nonfinite")[3])
    key = lambda v: set(map(tuple, np.asarray(v).tolist()))
    assert not key(bad) & (key(g) | key(h))


def test_integrate_keeps_a_tsdf_that_is_not_finite():
    """(w NaN + S) / wn is NaN and (w inf + S) / wn is inf: fusion does not repair a voxel, it stays unseen"""
    ref = F.load_case("nonfinite")
    before, weight = F.Dense(ref.blocks()), ref.W.copy()
    ref.integrate(*F.nonfinite_frame())
    after = F.Dense(ref.blocks())
    bad = F.case("nonfinite")["bad"]
    hit = after.at(after.W, bad) > before.at(before.W, bad)
    assert hit.sum() >= 3
    a, b = after.at(after.D, bad), before.at(before.D, bad)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])
    assert (ref.W[:8] != weight).sum() > 100


def test_parity_fills_one_position_of_the_table():
    c = F.case("parity")
    coords = c["blocks"][0]
    assert len(coords) == 212 and ((coords % 2 == 0).all(1)).sum() == 200
    slots, share, turned_in, turned_out = F.table_census(coords, c["max_blocks"])
    print(f"parity: {slots} slots, {share} keys share a position, {turned_in} insertions and {turned_out} look-ups turn")
    assert slots == 1024 and slots // F.PROBE_STEP == 128 and share == 200 > 128
    assert turned_in >= 72 and turned_out >= 72
    # whatever order the insertions arrive in: at most 128 keys fit the position's own slots
    shuffled = coords[np.random.RandomState(3).permutation(len(coords))]
    assert min(F.table_census(shuffled, c["max_blocks"])[2:]) >= 72
    # the frame of the parity test updates old blocks and needs new ones, among them PARITY_TARGET: a lattice point that
    # was left out, so its key shares the position of the 200, finds all 128 slots of that position full in whatever
    # order the 200 went in, and block_touch takes the turn to insert it
    target = np.array(F.PARITY_TARGET)
    assert ((target - np.array(F.PARITY_BASE)) % 2 == 0).all() and not (coords == target).all(1).any()
    before, ref = F.load_case("parity").W, F.carried_on("parity")
    assert 212 < len(ref.coords) <= F.PARITY_MAX_BLOCKS and (ref.W[:212] != before).any() and not ref.clipped
    new = ref.coords[212:]
    assert (new == target).all(1).any()
    for order in (coords, shuffled):
        table = [None] * slots
        for c in order.tolist():
            table[F.table_walk(table, F.pack_key(*c))[0]] = F.pack_key(*c)
        assert sum(k is not None for k in table[F.hash_key(F.pack_key(*target)) & 7::8]) == 128
        slot, turns = F.table_walk(table, F.pack_key(*target))
        assert turns >= 1 and table[slot] is None
    assert len(F.per_block(F.case_mesh("parity")[3][:, :3])[0]) == 212   # a plane through every block


def test_frames513_weights_stay_exact():
    ref = F.frames_ref(513)
    W = ref.W.astype(np.float64)
    print(f"frames513: {len(ref.coords)} blocks, largest weight {W.max():.0f}")
    assert W.max() >= 411 and W.max() <= 513 < 2 ** 24 and (W == np.round(W)).all()
    assert len(ref.coords) <= 1024 and not ref.clipped
    assert len(ref.surface_points(9)[0]) > 0
    depth, intr, extr, col = F.frames513(513, color=True)
    assert depth.shape == (513, 6, 8) and col.shape == (513, 6, 8, 3) and col.dtype == np.uint8
    assert np.array_equal(depth[512], depth[2]) and np.array_equal(extr[512], extr[2])


@pytest.mark.parametrize("width,step", [(2048, 1), (2049, 1), (2049, 2)])
def test_pixels_last_pixel_alone_needs_its_blocks(width, step):
    """2048 pixels are one workgroup of the touch pass; the 2049th is the only pixel of the second"""
    ref, without = F.pixels_ref(width, step), F.pixels_ref(width, step, last=False)
    assert (width - 1) % step == 0
    assert 0 < len(without.coords) < len(ref.coords) <= 1024 and not ref.clipped
    assert len(ref.surface_points(9)[0]) > 0


def test_kinds_0_to_2_are_the_surface_rows_in_both_restatements():
    for name, mw in [("random8", 1), ("weights", 0), ("weights", 0.5), ("signs", 1), ("parity", 1)]:
        vertices, _, color, edges = F.case_mesh(name, mw)
        rows, voxels, _ = F.case_surface(name, 6, mw)
        axis = edges[:, 3] < 3
        assert 0 < axis.sum() == len(rows) < len(edges)
        assert np.array_equal(edges[axis][:, :3], voxels)
        assert np.array_equal(_bits(vertices[axis]), _bits(rows[:, :3]))
        if color is not None:
            assert np.array_equal(_bits(color[axis]), _bits(rows[:, 3:6]))


@pytest.mark.parametrize("name", F.MESH_CASES)
def test_invariants_hold_on_the_restatement(name):
    c = F.case(name)
    for mw in c["min_weights"]:
        vertices, triangles, _, edges = F.case_mesh(name, mw)
        F.vertices_on_their_edges(vertices, edges, c["voxel"], c["origin"])
        strict = F.triangles_face_outwards(vertices, triangles, edges, c["blocks"], c["voxel"], c["origin"], "tet")
        assert strict == len(triangles) or name == "signs"
        if name in ("signs", "parity"):
            F.triangles_face_outwards(vertices, triangles, edges, c["blocks"], c["voxel"], c["origin"], "cell")


def test_the_cell_form_of_the_orientation_invariant_needs_a_smooth_volume():
    c = F.case("checker")
    vertices, triangles, _, edges = F.case_mesh("checker")
    with pytest.raises(AssertionError):
        F.triangles_face_outwards(vertices, triangles, edges, c["blocks"], c["voxel"], c["origin"], "cell")


def test_every_case_hands_its_blocks_over_ascending():
    """as mesh_ref expects them"""
    for name in F.CASES:
        coords = F.case(name)["blocks"][0].astype(np.int64)
        key = (coords[:, 0] << 32) | (coords[:, 1] << 16) | coords[:, 2]
        assert (np.diff(key) > 0).all()
