"""The designed cases of tests/frames_forms.py meet their design conditions, asserted on the restatements alone
(tests/render_ref.py, tests/unproject_ref.py and frames_forms.tile_rects): tests/test_frames_forms_gpu.py relies on every
one of them to reach the launch form it names.  No GPU.  Every test prints the numbers its condition rests on: list
lengths, distinct winners, branch counts, kept pixels per step."""
import numpy as np
import pytest

from tests import frames_forms as F

INF = np.inf


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _winners_inside_their_rectangles(c, tri):
    """every pixel's winner has the pixel's tile in its rectangle: the restatement of tile_rect is conservative here"""
    branch, rect = F.case_rects(c)
    for f, v, u in zip(*np.nonzero(tri >= 0)):
        t = tri[f, v, u]
        x0, x1, y0, y1 = rect[f, t]
        assert branch[f, t] != F.NONE and x0 <= u // F.TILE <= x1 and y0 <= v // F.TILE <= y1, (f, v, u, t)


# ---- render ----
@pytest.mark.parametrize("T", F.R1_SIZES)
def test_r1_every_hit_pixel_has_its_own_winner_in_every_window(T):
    c = F.r1(T)
    counts = F.case_counts(c)
    assert counts.shape == (1, 1, 1) and counts[0, 0, 0] == T          # one tile: the list is the mesh
    rounds = -(-T // F.BATCH)
    assert rounds == {255: 1, 256: 1, 257: 2, 512: 2, 513: 3, 768: 3}[T]
    layer, depth = np.arange(T) % 3, F.r1_depth(np.arange(T))
    seen, rounds_seen = set(), set()
    for lo, hi in F.R1_WINDOWS:
        _, tri, _, z = F.render_case_ref(c, ("r1", T), min_depth=lo, max_depth=hi)
        hit = tri >= 0
        winners = np.unique(tri[hit])
        visible = (depth >= lo) & (depth <= hi)
        front = visible & (layer == layer[visible].min())              # the nearest layer the window lets through
        print(f"r1[{T}] window [{lo}, {hi}]: list {T} ({rounds} rounds), {int(hit.sum())} pixels hit, {winners.size} distinct "
              f"winners in layer {np.unique(winners % 3).tolist()}, staged in rounds {np.unique(winners // F.BATCH).tolist()}")
        assert winners.size == hit.sum() == front.sum() and np.array_equal(winners, np.flatnonzero(front))
        assert np.array_equal(z[hit], depth[tri[hit]])                 # z is the designed depth, exactly
        rounds_seen |= set((winners // F.BATCH).tolist())
        if hi == INF:
            seen |= set(winners.tolist())
        if (lo, hi) == (0.0, INF):
            assert hit.sum() == F.R1_HITS[T] == -(-T // 3)
        if hi in (2.125, 4.125) and T >= 512:                          # a window that ends inside a layer: the layer's
            assert ((layer == layer[front][0]) & (depth > hi)).sum() >= 42      # farther part would win without max_depth
    assert rounds_seen == set(range(rounds))                          # were the list in index order, every round would win
    if T == 768:
        assert seen == set(range(768))                                 # 3 x 256 distinct winners, together every triangle


def test_r2_walls_sit_on_the_uint16_edges():
    for d, q in zip(F.R2_DEPTHS, F.R2_QUANTA):
        c = F.r2(d)
        depth, tri, _, z = F.render_case_ref(c, ("r2", d), depth_dtype=np.uint16, depth_scale=F.R2_SCALE)
        print(f"r2[{d}]: z / depth_scale = {d / F.R2_SCALE}, q = {np.unique(depth).tolist()}")
        assert (tri >= 0).all() and (z == d).all() and (depth == q).all()
        as_float = F.render_case_ref(c, ("r2", d))[0]
        assert as_float.dtype == np.float32 and (as_float == np.float32(d)).all()
    halves = [d / F.R2_SCALE for d in F.R2_DEPTHS]
    assert halves == [0.5, 1.5, 2.5, 3.5, 65535.0, 65535.5]           # ties to even below and above; the last value; past it


def test_r3_colours_reach_the_special_values():
    c = F.r3(False)
    _, tri, color, _ = F.render_case_ref(c, ("r3", False))
    per = [color[tri == t] for t in range(6)]
    print("r3: pixels per triangle", [len(p) for p in per])
    assert all(len(p) >= 20 for p in per)
    assert np.isnan(per[0][:, 0]).all() and (per[0][:, 1] == INF).all()
    assert (_bits(per[0][:, 2]) == 0x80000000).all()                    # -0.0 keeps its sign
    assert (_bits(per[0][:, 0]) == 0x7FC00000).all()                    # the vertex's own quiet NaN, not a new one
    assert (_bits(per[1]) == _bits(np.array([F.DENORMAL]))[0]).all()    # a denormal survives the interpolation
    assert (per[2] > 255.0).all() and np.isfinite(per[2]).all()
    c8 = F.r3(True)
    _, tri8, color8, _ = F.render_case_ref(c8, ("r3", True))
    assert np.array_equal(tri8, tri) and color8.dtype == np.uint8
    assert (color8[tri8 == 0] == 0).all() and (color8[tri8 == 1] == 255).all()
    assert (color8[tri8 < 0] == 0).all() and (tri8 >= 0).all()
    # no pixel centre on an edge of the four triangles: no weight of exactly zero meets the +inf
    R = F._rr()
    P = R.camera_space(c["vertices"], c["extr"][0])
    v, u = np.mgrid[0:16, 0:16].astype(np.float64)
    dx, dy = (u - 8.0) / F.F_PX, (v - 8.0) / F.F_PX
    for t in c["triangles"][:4]:
        n0, n1, n2, _ = R.edge_normals(*(tuple(P[i]) for i in t))
        for n in (n0, n1, n2):
            assert ((dx * n[0] + dy * n[1]) + n[2] != 0).all()


def test_r4_every_branch_of_tile_rect_by_name():
    c = F.r4()
    ids = c["ids"]
    assert set(ids) == set(F.R4_PLAIN) and len(ids) == len(c["triangles"])
    branch, rect = F.case_rects(c)
    counts = np.array([[int((branch[f] == b).sum()) for b in (F.NONE, F.BOX, F.WHOLE)] for f in range(len(F.R4_CAMERAS))])
    for f, name in enumerate(F.R4_CAMERAS):
        print(f"r4 {name}: none / box / whole = {counts[f].tolist()}")
    for name, want in F.R4_PLAIN.items():
        assert branch[0, ids[name]] == want, name
    assert (counts[0] > 0).all()                                        # the plain camera alone takes every branch
    # a mirrored image: the same branches, other boxes
    assert np.array_equal(branch[1], branch[0]) and not np.array_equal(rect[1], rect[0])
    never = [ids[n] for n in ("nan_vertex", "bad_index", "negative_index")]
    for f in range(2, 7):                                               # a camera that is not finite, or fx = 0: the whole
        assert (branch[f, never] == F.NONE).all()                       # frame for whatever camera_vertices lets through,
        assert (np.delete(branch[f], never) == F.WHOLE).all()           # the triangle behind the camera included
    tiles = (-(-F.R4_W // F.TILE), -(-F.R4_H // F.TILE))
    assert tiles == (4, 3) and F.R4_W % F.TILE and F.R4_H % F.TILE      # partial last tiles on both axes
    # the seams: a vertex on pixel 15 reaches tile 1 through the one-pixel growth, one on pixel 16 reaches tile 0
    assert tuple(rect[0, ids["on_15"]]) == (0, 1, 0, 1) and tuple(rect[0, ids["on_16"]]) == (0, 1, 0, 1)
    assert tuple(rect[0, ids["on_31_32"]]) == (1, 2, 1, 2)
    assert tuple(rect[0, ids["on_last"]]) == (3, 3, 2, 2) and tuple(rect[0, ids["on_first"]]) == (0, 0, 0, 0)
    P = F._rr().camera_space(c["vertices"], c["extr"][0])
    esc = P[c["triangles"][ids["escape"]]]
    assert (esc[:, 2] > 0).all() and np.abs(esc[:, 0] / esc[:, 2] * F.F_PX + F.R4_CX).max() > F.MAX_PX
    cross = P[c["triangles"][ids["crossing"]], 2]
    assert (cross > 0).any() and (cross < 0).any()
    # the restatement has an answer for every camera
    _, tri, _, _ = F.render_case_ref(c, "r4")
    hits = [int((tri[f] >= 0).sum()) for f in range(len(F.R4_CAMERAS))]
    print(f"r4: pixels hit per camera {dict(zip(F.R4_CAMERAS, hits))}")
    assert hits == [F.R4_H * F.R4_W] * 3 + [0, 0, 0, 0]
    for name in ("on_15", "on_16", "on_31_32", "on_last", "on_first", "escape", "crossing"):
        assert (tri[0] == ids[name]).any() and (tri[1] == ids[name]).any(), name
    for name, (v, u) in dict(on_15=(15, 15), on_16=(16, 16), on_31_32=(31, 32), on_last=(36, 52), on_first=(0, 0)).items():
        assert tri[0, v, u] == ids[name]                                # the vertex's own pixel centre: two edges at zero
    for name in ("left", "above", "beyond", "below", "near_left", "behind", "zero_area", "nan_vertex", "bad_index",
                 "negative_index"):
        assert not (tri == ids[name]).any(), name
    assert np.array_equal(tri[1], tri[0][:, ::-1])                      # fx = -16 about column 26 of 53: the mirror image
    assert (tri[2] == tri[0][:, 26:27]).all()                           # fx = inf: every column shows the principal one
    _winners_inside_their_rectangles(c, tri)


@pytest.mark.parametrize("shape", F.R5_SHAPES)
def test_r5_thin_frames_see_the_seam_triangles(shape):
    c = F.r5(shape)
    ids = c["ids"]
    branch, rect = F.case_rects(c)
    _, tri, _, _ = F.render_case_ref(c, ("r5", shape))
    print(f"r5 {shape}: none / box / whole = {[int((branch == b).sum()) for b in (F.NONE, F.BOX, F.WHOLE)]}, winners "
          f"{[np.unique(tri[f]).tolist() for f in range(2)]}, list lengths up to {int(F.case_counts(c).max())}")
    assert tri.shape == shape and all((branch == b).any() for b in (F.NONE, F.BOX, F.WHOLE))
    assert (tri[0] == ids["on_15"]).any()
    assert (tri[1] == ids["on_last" if shape[1] == 1 else "on_16"]).any()
    last = tri[1].ravel()[-(300 % F.TILE):]                             # the partial tile at the end of the long axis
    assert (last == ids["on_last" if shape[1] == 1 else "on_16"]).any()
    _winners_inside_their_rectangles(c, tri)


def test_r6_entry_counts_of_the_existing_scenes():
    """what tests/test_render_gpu.py reaches: no list of its exact scenes is longer than one round"""
    for shape in F.EXACT_SHAPES:
        c = F.exact_case(shape)
        counts = F.case_counts(c)
        print(f"exact_scene{shape}: E per frame {F.entries(c).tolist()}, longest list {int(counts.max())}")
        assert F.entries(c).sum() == F.EXACT_ENTRIES[shape]
        assert counts.max() < F.BATCH
    assert F.case_counts(F.exact_case(F.EXACT_SHAPES[0])).max() == 33
    assert F.case_counts(F.exact_case(F.EXACT_SHAPES[1])).max() == 25
    for name, c in F.render_cases():
        E = F.entries(c)
        whole = c["triangles"].shape[0] * int(np.prod(F.case_counts(c).shape[1:]))
        print(f"{name}: E per frame {E.tolist()} (every rectangle the whole frame: {whole})")
        assert (E > 0).all()
    # a rectangle that is needlessly the whole frame shows in E
    c = F.r4()
    assert F.entries(c)[0] < F.entries(c)[2] == (len(c["triangles"]) - 3) * 12


def test_r7_cut_falls_inside_the_last_tile():
    c = F.r7()
    counts = F.case_counts(c)[0].ravel()
    ends = np.cumsum(counts)
    print(f"r7: list lengths {counts.tolist()}, ends {ends.tolist()}")
    assert counts.tolist() == [507, 195, 195, 75] and ends[-1] == 972
    assert counts[0] > F.BATCH                                          # the first tile stages two rounds
    cut = ends[-1] - 5
    assert (ends[:3] <= cut).all() and ends[2] < cut < ends[3]
    _, tri, _, _ = F.render_case_ref(c, "r7")
    for y in range(2):
        for x in range(2):
            assert (tri[0, 16 * y:16 * y + 16, 16 * x:16 * x + 16] >= 0).any()     # every tile shows something to lose


# ---- unproject ----
def _census(kept):
    census = F.kept_census(kept)
    return census, census.sum(-1)


@pytest.mark.parametrize("shape,pixels", list(zip(F.U1_SHAPES, F.U1_PIXELS)))
@pytest.mark.parametrize("float_depth", [False, True])
def test_u1_every_full_step_keeps_256_pixels(shape, pixels, float_depth):
    c = F.unproject_case("u1", shape, float_depth)
    rows, pix, has = F.unproject_case_ref(c, ("u1", shape, float_depth))
    assert np.prod(shape) == pixels == len(pix) and np.array_equal(pix, np.arange(pixels))
    census, steps = _census(F.kept_of(pix, shape))
    print(f"u1 {shape} {'fp32' if float_depth else 'uint16'}: kept per step {steps.tolist()}, {int(has.sum())} normals")
    full = pixels // F.THREADS
    assert (steps.ravel()[:full] == F.THREADS).all() and (census.reshape(-1, 4)[:full] == 64).all()
    assert steps.ravel()[full:].sum() == pixels % F.THREADS
    if pixels % F.RUN == 1:
        assert steps[-1].tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and len(steps) == pixels // F.RUN + 1
    if pixels == 2047:
        assert census[0, 7].tolist() == [64, 64, 64, 63]
    assert has.mean() > 0.9


@pytest.mark.parametrize("float_depth", [False, True])
def test_u2_empty_steps_and_runs(float_depth):
    c = F.unproject_case("u2", F.U2_SHAPE, float_depth, mask=F.u2_mask())
    rows, pix, has = F.unproject_case_ref(c, ("u2", float_depth))
    census, steps = _census(F.kept_of(pix, F.U2_SHAPE))
    print(f"u2: kept per (run, step) {steps.tolist()}; run 0 steps 4 and 7 per wave {census[0, 4].tolist()} "
          f"{census[0, 7].tolist()}; run 2 steps 0 and 7 per wave {census[2, 0].tolist()} {census[2, 7].tolist()}")
    assert np.array_equal(F.kept_of(pix, F.U2_SHAPE), F.u2_mask())
    assert steps[0].tolist() == [256, 0, 256, 0, 1, 256, 0, 1]
    assert all((census[0, s] == 64).all() for s in (0, 2, 5))
    assert census[0, 4].tolist() == [0, 0, 0, 1] and pix[512] == 4 * 256 + 255         # lane 63 of wave 3
    assert census[0, 7].tolist() == [1, 0, 0, 0] and pix[769] == 7 * 256               # lane 0 of wave 0
    assert steps[1].sum() == 0
    assert steps[2].tolist() == [1, 0, 0, 0, 0, 0, 0, 1] and census[2, 7].tolist() == [0, 0, 0, 1]
    assert len(pix) == 772 and has.sum() > 500 and not has[[512, 769, 770, 771]].any()


@pytest.mark.parametrize("step", F.U3_STEPS)
def test_u3_lattice(step):
    shape = F.U1_SHAPES[3]
    c = F.unproject_case("u1", shape, False)
    rows, pix, has = F.unproject_case_ref(c, ("u1", shape, False), step=step)
    _, steps = _census(F.kept_of(pix, shape))
    print(f"u3 step {step}: {len(pix)} rows, kept per (run, step) {steps.tolist()}")
    H, W = shape[1:]
    assert len(pix) == 2 * len(range(0, H, step)) * len(range(0, W, step))
    if step == 100:
        assert pix.tolist() == [0, H * W]
    assert has.all()                                                    # normals from the raw neighbours, off the lattice
    assert len(pix) < 2 * H * len(range(0, W, step))                    # a step applied to u alone would keep more


def test_u4_the_pixel_across_a_frame_seam_would_be_usable():
    shape, edge = F.U4_SHAPE, 1.0
    c = F.unproject_case("u4", shape, cams=F.u4_cameras())
    rows, pix, has = F.unproject_case_ref(c, "u4", edge=edge)
    Fr, H, W = shape
    z = c["depth"].astype(np.float64) * 0.001
    assert (z > 0).all() and len(pix) == Fr * H * W and has.all()
    flat = z.ravel()
    across, worst = 0, 0.0
    for f in range(Fr):
        for v, d in ((0, -W), (H - 1, W)):
            p = (f * H + v) * W + np.arange(W)
            q = p + d                                                    # the pixel at p -/+ W: in the neighbouring frame
            if q[0] < 0 or q[-1] >= flat.size:
                continue
            assert (q // (H * W) != f).all()
            ratio = np.abs(flat[q] - flat[p]) / flat[p]
            across, worst = across + W, max(worst, float(ratio.max()))
            assert (ratio <= edge).all() and (flat[q] != flat[p]).any()  # valid, within `edge`, and another depth
    seam_rows = np.zeros(Fr * H * W, bool)
    seam_rows.reshape(Fr, H, W)[:, [0, H - 1]] = True
    per_run = [int(seam_rows[g * F.RUN:(g + 1) * F.RUN].sum()) for g in range(-(-seam_rows.size // F.RUN))]
    print(f"u4: seam-row pixels per run {per_run}; {across} pixels have a usable pixel across a seam, largest "
          f"|z_q - z_p| / z_p {worst:.3f} (edge {edge})")
    assert all(n > 0 for n in per_run) and len(per_run) == 3 and across == 2 * (Fr - 1) * W


def test_u5_colours():
    mask = F.u2_mask()
    c = F.unproject_case("u5", F.U2_SHAPE, mask=mask, color="fp32")
    rows, pix, _ = F.unproject_case_ref(c, "u5")
    col = _bits(rows[:, 3:6])
    assert np.array_equal(col, _bits(c["color"].reshape(-1, 3)[pix]))
    assert np.isnan(rows[0, 4]) and col[0, 0] == 0x80000000 and col[0, 2] == _bits(np.array([F.DENORMAL]))[0]
    assert rows[1, 3] == INF and rows[1, 4] == -INF and np.isnan(rows[-1, 5])
    none = F.unproject_case("u5", F.U2_SHAPE, mask=mask, color=None)
    rows, _, _ = F.unproject_case_ref(none, "u5 none")
    assert not _bits(rows[:, 3:6]).any()


def test_u6_cut_falls_inside_the_last_step_of_the_last_run():
    shape = F.U1_SHAPES[3]
    N = int(np.prod(shape))
    assert N == 2 * F.RUN and (N - 5) // F.THREADS == N // F.THREADS - 1 and (N - 5) % F.THREADS != 0
