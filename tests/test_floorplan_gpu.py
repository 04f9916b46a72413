"""detection_3d_amd.floorplan (floorplan.hip) against the numpy restatement of its definitions in tests/floorplan_ref.py.
Every comparison is exact (array_equal) and leaves no element out: the reference takes the device's own fp64 box table
(read back), and from there every operation is a rounded fp64 product, sum or quotient on both sides, or integer min,
max and add.  The table itself is compared to numpy to 1e-12 (a correct fp64 cos of an argument this size is within a few
1e-16)."""
import math

import numpy as np
import pytest
import torch

import floorplan_ref as ref

pytestmark = pytest.mark.gpu


def _t(dev, a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev)


def _check_plan(plan, blk, min_cells, max_rooms):
    """every output of a Plan against the reference on the blocked map blk"""
    label, r, cells, bounds, seed = ref.rooms(blk, min_cells, max_rooms)
    assert plan.min_cells == min_cells and plan.max_rooms == max_rooms
    assert plan.label.dtype == torch.int32 and np.array_equal(plan.label.cpu().numpy(), label)
    assert plan.count_dev.dtype == torch.int32 and plan.count == r
    assert np.array_equal(plan.cells.cpu().numpy(), cells)
    assert np.array_equal(plan.bounds.cpu().numpy(), bounds)
    assert np.array_equal(plan.seed.cpu().numpy(), seed)
    return label, r


def _rooms_of_map(dev, blk, min_area=0.0, max_rooms=1024, cell=0.05):
    from detection_3d_amd import floorplan as fp
    bm = fp.Bitmap.from_blocked(torch.from_numpy(blk).to(dev), cell)
    assert np.array_equal(bm.blocked.cpu().numpy(), blk)
    plan = fp.label_rooms(bm, min_area, max_rooms)
    return plan, _check_plan(plan, blk, ref.min_cells(min_area, cell), max_rooms)


# ---- raster ----
def _dyadic_boxes():
    """cell 0.25 on a 45 x 70 lattice at the origin: centres and sizes on multiples of 1 / 8, so that cell centres fall
    exactly on faces at yaw 0"""
    rs = np.random.RandomState(5)
    rows = [[2.125, 3.125, 0, 0.5, 1.5, 1, 0.0],             # faces exactly on cell centres: 3 x 7 cells
            [6.0, 3.0, 0, 0.5, 2.0, 1, 0.0],                 # faces on cell borders: 2 x 8 cells
            [9.0, 6.0, 0, 0.5, 3.0, 1, math.pi / 2], [12.0, 2.0, 0, 0.25, 3.0, 1, -math.pi / 2],
            [5.0, 8.0, 0, 0.5, 4.0, 1, math.pi / 4], [14.0, 8.0, 0, 1.0, 1.0, 1, -math.pi / 4],
            [17.5, 5.0, 0, 2.0, 6.0, 1, 0.3],                # half off the lattice (W 0.25 = 17.5)
            [0.0, 11.25, 0, 3.0, 1.0, 1, 1.1],               # over a corner
            [40.0, 40.0, 0, 2.0, 2.0, 1, 0.5], [-30.0, 2.0, 0, 1.0, 50.0, 1, 0.0],      # wholly off
            [3.0, 3.0, 0, 1.0, 1.0, 1, np.nan], [np.nan, 3.0, 0, 1.0, 1.0, 1, 0.0], [3.0, 3.0, 0, np.inf, 1.0, 1, 0.0],
            [8.125, 1.125, 0, 0.0, 0.0, 1, 0.0],             # zero size on a cell centre: that one cell
            [8.25, 1.625, 0, 0.0, 0.0, 1, 0.0]]              # zero size on a cell border: nothing
    for _ in range(12):
        rows.append([rs.randint(0, 140) / 8, rs.randint(0, 90) / 8, 0, rs.randint(1, 16) / 8, rs.randint(1, 40) / 8, 1,
                     rs.uniform(-math.pi, math.pi)])
    return np.array(rows, dtype=np.float32)


def test_raster_exact_with_closed_faces(dev):
    from detection_3d_amd import floorplan as fp
    boxes = _dyadic_boxes()
    lat = fp.Lattice((0.0, 0.0), (45, 70))
    b = _t(dev, boxes)
    table = fp.box_table(b, 0.0)
    want_table = ref.box_table(boxes, 0.0)
    got_table = table.cpu().numpy()
    assert table.dtype == torch.float64 and np.array_equal(np.isfinite(got_table), np.isfinite(want_table))
    fin = np.isfinite(want_table)
    assert np.abs(got_table[fin] - want_table[fin]).max() <= 1e-12
    for grow in (0.0, 0.125, 0.1):
        t = fp.box_table(b, grow).cpu().numpy()
        bm = fp.rasterize(b, None, 0.25, lat, grow)
        assert bm.words.shape == (45, 3) and bm.words.dtype == torch.int32 and bm.lattice == lat
        got = bm.blocked.cpu().numpy()
        assert np.array_equal(got, ref.blocked_full(t, None, 0.25, lat.origin, lat.shape)), grow
        assert np.array_equal(got, ref.blocked(t, None, 0.25, lat.origin, lat.shape)), grow
        assert ((bm.words[:, 2].cpu().numpy().astype(np.int64) & 0xFFFFFFFF) >> 6 == 0).all()      # bits from W on stay 0
        one = np.zeros(len(boxes), dtype=bool)
        for j in range(len(boxes)):                          # every box alone, through the select mask
            one[:] = False
            one[j] = True
            alone = fp.rasterize(b, _t(dev, one, torch.bool), 0.25, lat, grow).blocked.cpu().numpy()
            assert np.array_equal(alone, ref.blocked_full(t, one, 0.25, lat.origin, lat.shape)), (grow, j)
            if grow == 0.0:
                n = int(alone.sum())
                if j == 0:
                    assert n == 3 * 7 and alone[9:16, 7:10].all()        # closed faces
                if j == 1:
                    assert n == 2 * 8
                if j in (8, 9, 10, 11, 12, 14):
                    assert n == 0, j
                if j == 13:
                    assert n == 1 and alone[4, 32]
                if j == 6:
                    assert 0 < n and alone[:, 69].any()
    half = np.arange(len(boxes)) % 2 == 0
    got = fp.rasterize(b, _t(dev, half, torch.bool), 0.25, lat, 0.0).blocked.cpu().numpy()
    assert np.array_equal(got, ref.blocked_full(got_table, half, 0.25, lat.origin, lat.shape))


def test_raster_box_counts_and_derived_lattice(dev):
    from detection_3d_amd import floorplan as fp
    lat = fp.Lattice((-1.0, 0.5), (45, 70))
    none = fp.rasterize(torch.zeros((0, 7), device=dev), None, 0.25, lat, 0.1)
    assert none.words.shape == (45, 3) and not none.blocked.any()
    plan = fp.rooms(torch.zeros((0, 7), device=dev), None, 0.25, lat, 0.1, 0.0)
    assert plan.count == 0 and (plan.label == fp.OUTSIDE).all()
    rs = np.random.RandomState(8)
    k = 4096
    boxes = np.stack([rs.uniform(-2, 17, k), rs.uniform(0, 12, k), np.zeros(k), rs.uniform(0, 0.4, k), rs.uniform(0, 1.5, k),
                      np.ones(k), rs.uniform(-4, 4, k)], 1).astype(np.float32)
    b = _t(dev, boxes)
    sel = rs.rand(k) < 0.05
    for select in (None, sel):
        bm = fp.rasterize(b, None if select is None else _t(dev, select, torch.bool), 0.25, lat, 0.05)
        t = fp.box_table(b, 0.05).cpu().numpy()
        assert np.array_equal(bm.blocked.cpu().numpy(), ref.blocked(t, select, 0.25, lat.origin, lat.shape))
    with pytest.raises(ValueError):
        fp.rasterize(torch.zeros((4097, 7), device=dev), None, 0.25, lat, 0.1)
    # lattice=None: around the selected blockers' corners, from the device's table
    for cell, margin, select in ((0.25, 2, sel), (0.05, 1, sel), (0.1, 5, None)):
        s = None if select is None else _t(dev, select, torch.bool)
        bm = fp.rasterize(b, s, cell, None, 0.1, margin)
        t = fp.box_table(b, 0.1).cpu().numpy()
        origin, shape = ref.lattice(t, select, cell, margin)
        assert bm.lattice == fp.Lattice(origin, shape)
        got = bm.blocked.cpu().numpy()
        assert np.array_equal(got, ref.blocked(t, select, cell, origin, shape))
        assert not got[:margin].any() and not got[-margin:].any() and not got[:, :margin].any() and not got[:, -margin:].any()
        assert got[margin + 1].any() or got[margin].any()


# ---- rooms ----
def _spiral(n=129):
    """a one-cell-wide corridor that winds to the centre: the longest parent chain"""
    blk = np.ones((n, n), dtype=bool)
    y, x, dy, dx = 1, 1, 0, 1
    blk[y, x] = False
    while True:
        moved = False
        for _ in range(2):
            ny, nx = y + dy, x + dx
            ahead_ok = 1 <= ny < n - 1 and 1 <= nx < n - 1 and blk[ny, nx]
            # stop one cell short of an earlier corridor
            ny2, nx2 = ny + dy, nx + dx
            if ahead_ok and (not (0 <= ny2 < n and 0 <= nx2 < n) or blk[ny2, nx2]):
                y, x = ny, nx
                blk[y, x] = False
                moved = True
                break
            dy, dx = dx, -dy
        if not moved:
            break
    return blk


def test_rooms_spiral_corridor(dev):
    blk = _spiral()
    assert (~blk).sum() > 3000
    plan, (label, r) = _rooms_of_map(dev, blk)
    assert r == 1 and plan.seed[0].item() == 129 + 1


def test_rooms_comb_joined_in_the_last_row(dev):
    blk = np.ones((130, 200), dtype=bool)
    blk[1:128, 1:199:2] = False                  # teeth
    blk[128, 1:199] = False                      # joined only here
    plan, (label, r) = _rooms_of_map(dev, blk)
    assert r == 1 and plan.cells[0].item() == 127 * 99 + 198
    blk[128, 100] = True                         # cut: two combs
    _, (_, r) = _rooms_of_map(dev, blk)
    assert r == 2


def test_rooms_seams_of_words_and_rows(dev):
    """one-cell corridors along columns 31 | 32 and 63 | 64 and along a row, joined and apart"""
    blk = np.ones((70, 100), dtype=bool)
    blk[1:69, 31] = blk[1:69, 32] = False
    blk[1:69, 63] = False
    blk[1:69, 65] = False                        # 64 stays blocked: 63 and 65 are apart
    blk[35, 33:63] = False                       # a row corridor joins 32 and 63
    blk[40, 66:99] = False
    _, (label, r) = _rooms_of_map(dev, blk)
    assert r == 2 and label[1, 31] == label[68, 63] == 0 and label[1, 65] == label[40, 98] == 1
    blk[35, 48] = True
    _, (_, r) = _rooms_of_map(dev, blk)
    assert r == 3
    # a free run that spans whole words, and rows that start and end free (the run carries over word ends)
    blk = np.zeros((5, 131), dtype=bool)
    blk[0] = blk[4] = True
    blk[:, 0] = blk[:, 130] = True
    _, (label, r) = _rooms_of_map(dev, blk)
    assert r == 1 and (label[1:4, 1:130] == 0).all()


def test_rooms_checkerboard_cuts_the_tables(dev):
    blk = np.ones((64, 96), dtype=bool)
    yy, xx = np.mgrid[0:64, 0:96]
    blk[((yy + xx) % 2 == 0) & (yy > 0) & (yy < 63) & (xx > 0) & (xx < 95)] = False
    plan, (label, r) = _rooms_of_map(dev, blk, 0.0, 16)
    assert r == 62 * 94 // 2 > 16 and plan.listed == 16 and label.max() == r - 1
    assert plan.area.shape == (16,) and plan.room_boxes().shape == (16, 7)


def test_rooms_smallest_plans(dev):
    for blk in (np.zeros((1, 1), dtype=bool), np.ones((1, 1), dtype=bool), np.ones((33, 65), dtype=bool),
                np.zeros((33, 65), dtype=bool), np.zeros((1, 200), dtype=bool), np.zeros((200, 1), dtype=bool)):
        _, (label, r) = _rooms_of_map(dev, blk)
        assert r == 0 and (label == (ref.BLOCKED if blk.all() else ref.OUTSIDE)).all()
    # a component that touches the border only at a corner cell
    blk = np.ones((40, 40), dtype=bool)
    blk[0, 0] = blk[1, 0] = blk[1, 1:20] = blk[2:30, 19] = False
    _, (label, r) = _rooms_of_map(dev, blk)
    assert r == 0 and label[29, 19] == ref.OUTSIDE
    blk[0, 0] = blk[1, 0] = True
    _, (label, r) = _rooms_of_map(dev, blk)
    assert r == 1 and label[29, 19] == 0
    blk = np.ones((40, 40), dtype=bool)
    blk[5:20, 5:20] = blk[30, 30] = blk[30, 32] = blk[31, 33] = False
    _, (label, r) = _rooms_of_map(dev, blk, 0.05 * 0.05 * 2)        # min_cells 2
    assert r == 1 and label[30, 30] == ref.SMALL


def test_rooms_six_room_plan(dev):
    from detection_3d_amd import floorplan as fp
    boxes = ref.six_rooms()
    b = _t(dev, boxes)
    lat = fp.Lattice((0.0, 0.0), (200, 280))
    plan = fp.rooms(b, None, 0.05, lat, 0.0)
    t = fp.box_table(b, 0.0).cpu().numpy()
    _check_plan(plan, ref.blocked(t, None, 0.05, lat.origin, lat.shape), ref.min_cells(1.0, 0.05), 1024)
    assert plan.count == 6 and plan.cells[:6].tolist() == [6084] * 6
    assert np.array_equal(plan.area.cpu().numpy(), np.full(6, 6084.0) * (0.05 * 0.05))
    want = ref.room_boxes(plan.bounds[:6].cpu().numpy(), 0.05, lat.origin, 0.25, 2.5).astype(np.float32)
    assert np.array_equal(plan.room_boxes(0.25, 2.5).cpu().numpy(), want)
    # the default grow and a derived lattice: the same six rooms, each a little smaller
    plan = fp.rooms(b)
    t = fp.box_table(b, 0.1).cpu().numpy()
    origin, shape = ref.lattice(t, None, 0.05, 2)
    assert plan.lattice == fp.Lattice(origin, shape)
    _check_plan(plan, ref.blocked(t, None, 0.05, origin, shape), 400, 1024)
    assert plan.count == 6 and plan.cells[:6].tolist() == [74 * 74] * 6


def test_rooms_random_plans_order_and_repetition(dev):
    """twenty seeded plans of axis-aligned and rotated walls in 200 x 150; a permutation of the boxes and a second run
    give the same bits"""
    from detection_3d_amd import floorplan as fp
    lat = fp.Lattice((0.0, 0.0), (150, 200))
    total = 0
    for seed in range(20):
        boxes = ref.random_plan(100 + seed)
        b = _t(dev, boxes)
        plan = fp.rooms(b, None, 0.05, lat, 0.1, 0.25, 8)
        t = fp.box_table(b, 0.1).cpu().numpy()
        _, r = _check_plan(plan, ref.blocked(t, None, 0.05, lat.origin, lat.shape), 100, 8)
        total += r
        perm = np.random.RandomState(seed).permutation(len(boxes))
        for other in (fp.rooms(_t(dev, boxes[perm]), None, 0.05, lat, 0.1, 0.25, 8), fp.rooms(b, None, 0.05, lat, 0.1, 0.25, 8)):
            for name in ("label", "count_dev", "cells", "bounds", "seed"):
                assert torch.equal(getattr(other, name), getattr(plan, name)), (seed, name)
            assert torch.equal(other.bitmap.words, plan.bitmap.words)
    assert total >= 20


def test_rooms_large_plan_of_random_blocks(dev):
    rs = np.random.RandomState(12)
    n = 2048
    blk = np.zeros((n, n), dtype=bool)
    for _ in range(6000):
        y, x = rs.randint(0, n), rs.randint(0, n)
        h, w = (rs.randint(1, 6), rs.randint(8, 120)) if rs.rand() < 0.5 else (rs.randint(8, 120), rs.randint(1, 6))
        blk[y:y + h, x:x + w] = True
    plan, (label, r) = _rooms_of_map(dev, blk, 0.0, 4096)
    assert r > 1024 and (label == ref.OUTSIDE).sum() > n * n // 10 and (label == ref.BLOCKED).sum() > n * n // 10


def test_strips_one_cell_thick_never_leak(dev):
    """a strip 1.01 cells thick through a closed frame, at 200 seeded yaws: always two rooms"""
    from detection_3d_amd import floorplan as fp
    cell = 0.05
    lat = fp.Lattice((0.0, 0.0), (80, 80))
    frame = [ref.wall(0.5, 0.5, 3.5, 0.5, 0.2), ref.wall(0.5, 3.5, 3.5, 3.5, 0.2), ref.wall(0.5, 0.5, 0.5, 3.5, 0.2),
             ref.wall(3.5, 0.5, 3.5, 3.5, 0.2)]
    rs = np.random.RandomState(77)
    for i in range(200):
        yaw = rs.uniform(-math.pi, math.pi)
        strip = [2.0 + rs.uniform(-0.3, 0.3), 2.0 + rs.uniform(-0.3, 0.3), 0.0, 1.01 * cell, 12.0, 2.5, yaw]
        b = _t(dev, np.array(frame + [strip], dtype=np.float32))
        plan = fp.rooms(b, None, cell, lat, 0.0, 0.0)
        t = fp.box_table(b, 0.0).cpu().numpy()
        _check_plan(plan, ref.blocked_full(t, None, cell, lat.origin, lat.shape), 1, 1024)
        assert plan.count == 2, (i, yaw)


# ---- sides ----
def _flat(dev):
    """two rooms joined by a door, a window to the outside, a closet below min_area
    -> boxes, classes per box"""
    w = ref.wall
    rows = [w(1, 1, 7, 1), w(1, 5, 7, 5), w(1, 1, 1, 5), w(7, 1, 7, 2.5), w(7, 3.5, 7, 5),       # outer walls
            w(4, 1, 4, 2.5), w(4, 3.5, 4, 5),                                                     # the middle wall
            w(4, 2.5, 4, 3.5, 0.08, 0.0, 2.0),                                                    # 7: the door
            w(7, 2.5, 7, 3.5, 0.06, 1.0, 1.0),                                                    # 8: the window
            w(1, 4.4, 1.6, 4.4), w(1.6, 4.4, 1.6, 5),                                             # a closet of 0.5 x 0.5
            [2.5, 3.0, 0, 5.0, 3.0, 0.1, 0.0]]                                                    # 11: a floor
    return np.array(rows, dtype=np.float32), ["wall"] * 7 + ["door", "window", "wall", "wall", "floor"]


def test_box_sides(dev):
    from detection_3d_amd import floorplan as fp
    boxes, names = _flat(dev)
    b = _t(dev, boxes)
    blockers = np.array([n != "floor" for n in names])
    plan = fp.rooms(b, _t(dev, blockers, torch.bool), 0.05, None, 0.1, 1.0)
    t = fp.box_table(b, 0.1).cpu().numpy()
    origin, shape = ref.lattice(t, blockers, 0.05, 2)
    label, r = _check_plan(plan, ref.blocked(t, blockers, 0.05, origin, shape), 400, 1024)
    assert r == 2 and (label == ref.SMALL).any()
    t0 = fp.box_table(b, 0.0).cpu().numpy()
    for reach in (0.5, 0.05, 0.12, 2.0, 20.0, 0.0):
        sides = fp.box_sides(plan, b, reach)
        assert sides.dtype == torch.int32 and sides.shape == (len(boxes), 2)
        assert np.array_equal(sides.cpu().numpy(), ref.sides(t0, label, 0.05, origin, reach)), reach
    s = fp.box_sides(plan, b).cpu().numpy()
    assert sorted(s[7].tolist()) == [0, 1]                                        # the door links the two rooms
    assert sorted(s[8].tolist()) == [ref.OUTSIDE, 1]                              # the window is on the facade
    assert ref.SMALL in s[9].tolist() and ref.SMALL in s[10].tolist()             # the closet's walls
    assert (fp.box_sides(plan, b, 0.05).cpu().numpy()[:11] == ref.NONE).all()     # a reach inside the grown wall
    assert (fp.box_sides(plan, b, 0.0).cpu().numpy() == ref.NONE).all()
    far = fp.box_sides(plan, b, 20.0).cpu().numpy()
    assert far[11].tolist() == [ref.OUTSIDE, 1]                # the floor: -lx leaves the lattice, +lx starts in room 1
    doors = _t(dev, np.array([n == "door" for n in names]), torch.bool)
    assert plan.graph(_t(dev, s, torch.int32), doors).cpu().tolist() == [[0, 1, 7]]
    perm = np.random.RandomState(2).permutation(len(boxes))
    assert np.array_equal(fp.box_sides(plan, _t(dev, boxes[perm])).cpu().numpy(), s[perm])
    # a tight explicit lattice: probes leave it; NaN rows are off the lattice too
    lat = fp.Lattice((0.9, 0.9), (84, 124))
    tight = fp.rooms(b, _t(dev, blockers, torch.bool), 0.05, lat, 0.1, 1.0)
    tl, _ = _check_plan(tight, ref.blocked(t, blockers, 0.05, lat.origin, lat.shape), 400, 1024)
    odd = np.concatenate([boxes, [[np.nan, 1, 0, 1, 1, 1, 0]], [[1, 1, 0, 1, 1, 1, np.inf]]]).astype(np.float32)
    got = fp.box_sides(tight, _t(dev, odd), 0.5).cpu().numpy()
    want = ref.sides(fp.box_table(_t(dev, odd), 0.0).cpu().numpy(), tl, 0.05, lat.origin, 0.5)
    assert np.array_equal(got, want) and ref.OUTSIDE in got[2].tolist() and got[12].tolist() == [ref.OUTSIDE] * 2
    assert fp.box_sides(plan, torch.zeros((0, 7), device=dev)).shape == (0, 2)


def test_floorplan_of_picks_the_blockers(dev):
    from detection_3d_amd import floorplan as fp
    from detection_3d_amd.config import class_to_label
    boxes, names = _flat(dev)
    classes = ["background", "wall", "window", "door", "floor", "room"]
    c2l = class_to_label(classes)
    labels = torch.tensor([c2l[n] for n in names], dtype=torch.int64)
    out = fp.floorplan_of({"bbox3d": _t(dev, boxes), "labels": labels}, classes, max_rooms=8)
    blockers = _t(dev, np.array([n != "floor" for n in names]), torch.bool)
    plan = fp.rooms(_t(dev, boxes), blockers, max_rooms=8)
    assert torch.equal(out["plan"].label, plan.label) and out["plan"].count == 2
    assert torch.equal(out["box_rooms"], fp.box_sides(plan, _t(dev, boxes)))
    rooms = out["rooms"]
    assert rooms["bbox3d"].shape == (8, 7) and rooms["bbox3d"].dtype == torch.float32 and rooms["count"].item() == 2
    want = ref.room_boxes(plan.bounds[:2].cpu().numpy(), 0.05, plan.lattice.origin, 0.0, 2.5).astype(np.float32)
    assert np.array_equal(rooms["bbox3d"][:2].cpu().numpy(), want) and not rooms["bbox3d"][2:].any()
    assert torch.equal(rooms["area"][:2], plan.area) and not rooms["area"][2:].any()
    # without a door class the door is no blocker: one room
    few = ["background", "wall", "window"]
    lab2 = torch.tensor([{"wall": 1, "window": 2}.get(n, 0) for n in names], dtype=torch.int64)
    assert fp.floorplan_of({"bbox3d": _t(dev, boxes), "labels": lab2}, few)["plan"].count == 1


def test_room_targets_appends_room_boxes(dev):
    from detection_3d_amd import floorplan as fp
    from detection_3d_amd.config import class_to_label
    boxes, names = _flat(dev)
    classes = ["background", "wall", "window", "door", "floor", "room"]
    c2l = class_to_label(classes)
    labels = torch.tensor([c2l[n] for n in names], dtype=torch.int64)
    tg = {"bbox3d": _t(dev, boxes), "labels": labels}
    out = fp.room_targets(tg, classes, cell=0.05, min_area=1.0)
    k = len(boxes)
    assert out["bbox3d"].shape == (k + 2, 7) and out["labels"].tolist() == labels.tolist() + [c2l["room"]] * 2
    assert torch.equal(out["bbox3d"][:k], tg["bbox3d"])
    blockers = _t(dev, np.array([n != "floor" for n in names]), torch.bool)
    plan = fp.rooms(_t(dev, boxes), blockers)
    want = ref.room_boxes(plan.bounds[:2].cpu().numpy(), 0.05, plan.lattice.origin, 0.0, 2.5).astype(np.float32)
    assert np.array_equal(out["bbox3d"][k:].cpu().numpy(), want)             # z from the walls: 0 .. 2.5
    again = fp.room_targets(out, classes)
    assert again["bbox3d"] is out["bbox3d"]                                    # rooms of its own: nothing added


# ---- points ----
def test_room_of_points(dev):
    from detection_3d_amd import floorplan as fp
    boxes, names = _flat(dev)
    b = _t(dev, boxes)
    lat = fp.Lattice((0.5, 0.25), (24, 30))
    plan = fp.rooms(b, None, 0.25, lat, 0.1, 0.5)
    label = plan.label.cpu().numpy()
    assert plan.count >= 2
    rs = np.random.RandomState(3)
    gx, gy = np.meshgrid(0.5 + 0.25 * np.arange(-1, 32), 0.25 + 0.25 * np.arange(-1, 26))      # exactly on cell borders
    grid = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], 1)
    rand = np.stack([rs.uniform(-1, 9, 4000), rs.uniform(-1, 7, 4000), rs.uniform(-1, 3, 4000)], 1)
    odd = np.array([[np.nan, 1, 1], [1, np.nan, 1], [1, 1, np.nan], [np.inf, 1, 1], [1, -np.inf, 1], [2, 2, np.inf],
                    [1e30, 2, 0], [2, -1e30, 0], [3e38, 3e38, 0], [0.5, 0.25, 0], [8.0, 6.25, 0],
                    [np.nextafter(np.float32(8.0), np.float32(0)), np.nextafter(np.float32(6.25), np.float32(0)), 0]])
    pts = np.concatenate([grid, rand, odd]).astype(np.float32)
    got = fp.room_of_points(_t(dev, pts), plan)
    want = ref.room_of_points(pts, label, 0.25, lat.origin)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    n = len(pts)
    assert want[n - 12:n - 6].tolist() == [ref.NONE] * 6 and want[n - 6:n - 3].tolist() == [ref.OUTSIDE] * 3
    assert want[n - 3] == label[0, 0] and want[n - 2] == ref.OUTSIDE and want[n - 1] == label[23, 29]
    assert {ref.OUTSIDE, ref.BLOCKED, 0, 1} <= set(want.tolist())
    # a strided [N, 9] cloud read in place, its slices, and an origin
    cloud = torch.zeros((n, 9), device=dev)
    cloud[:, :3] = _t(dev, pts)
    cloud[:, 3:6] = _t(dev, pts[::-1].copy())
    assert torch.equal(fp.room_of_points(cloud, plan), got)
    assert torch.equal(fp.room_of_points(cloud[:, :3], plan), got)
    assert torch.equal(fp.room_of_points(cloud[:, 3:6], plan), got.flip(0))
    assert torch.equal(fp.room_of_points(cloud[::3], plan), got[::3])
    shift = np.array([0.3, -1.7, 12.0])
    got = fp.room_of_points(cloud, plan, origin=shift)
    assert np.array_equal(got.cpu().numpy(), ref.room_of_points(pts, label, 0.25, lat.origin, shift))
    got = fp.room_of_points(cloud, plan, origin=torch.from_numpy(shift))
    assert np.array_equal(got.cpu().numpy(), ref.room_of_points(pts, label, 0.25, lat.origin, shift))
    fin = pts[:len(grid) + len(rand)] + np.float32(100.0)
    got = fp.room_of_points(_t(dev, fin), plan, origin="min")
    want = ref.room_of_points(fin, label, 0.25, lat.origin, ref.cloud_min(fin))
    assert np.array_equal(got.cpu().numpy(), want) and (want >= 0).any()
    assert fp.room_of_points(torch.zeros((0, 3), device=dev), plan).shape == (0,)


# ---- pipeline ----
def test_pipeline_adds_rooms_and_changes_nothing_else(dev):
    from detection_3d_amd import floorplan as fp
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.detector import build_detection_model
    from detection_3d_amd.serving import BuildingPipeline
    from detection_3d_amd.synthetic import make_scene
    cfg = get_cfg("4c_Fpn432")
    torch.manual_seed(1)
    model = build_detection_model(cfg).to(dev).eval()
    with torch.no_grad():                                                # the weights of tests/test_detector_gpu.py
        model.rpn.head.cls_logits.weight.mul_(60)
        model.rpn.head.bbox_pred.weight.mul_(20)
        model.roi_heads.box.predictor.cls_score.weight.mul_(40)
        model.roi_heads.box.predictor.bbox_pred.weight.mul_(100)
    pcl = torch.from_numpy(make_scene(11, 25000)).to(dev)
    opts = {"cell": 0.1, "min_area": 0.5, "max_rooms": 64}
    with torch.no_grad():
        plain = BuildingPipeline(model, cfg, in_flight=2, device=dev, point_owner=True).map([pcl])[0]
        got = BuildingPipeline(model, cfg, in_flight=2, device=dev, point_owner=True, rooms=opts).map([pcl, pcl])
        down = BuildingPipeline(model, cfg, in_flight=2, device=dev, point_owner=True, rooms=True,
                                downsample={"voxel": 0.1}).map([pcl])[0]
    torch.cuda.synchronize()
    assert "rooms" not in plain and "box_rooms" not in plain and "point_room" not in plain
    for g in got:
        assert set(g) == set(plain) | {"rooms", "box_rooms", "point_room"}
        for k in plain:
            assert g[k].shape == plain[k].shape and torch.equal(g[k], plain[k]), k
        assert g["bbox3d"].shape[0] > 0
        lat = fp.detector_lattice(cfg, 0.1)
        want = fp.floorplan_of(g, cfg.INPUT.CLASSES, lattice=lat, **opts)
        assert torch.equal(g["box_rooms"], want["box_rooms"]) and g["box_rooms"].shape == (g["bbox3d"].shape[0], 2)
        for k in ("bbox3d", "area", "count"):
            assert torch.equal(g["rooms"][k], want["rooms"][k]), k
        room = fp.room_of_points(pcl, want["plan"], origin="min")
        assert g["point_room"].dtype == torch.int32 and torch.equal(g["point_room"], room)
        # against the reference, from the device's table
        c2l = {c: i for i, c in enumerate(c for c in ["background", "wall", "window", "door", "floor", "ceiling", "room"]
                                          if c in cfg.INPUT.CLASSES)}
        lab = g["labels"].cpu().numpy()
        blockers = np.isin(lab, [c2l[c] for c in ("wall", "window", "door") if c in c2l])
        t = fp.box_table(g["bbox3d"].to(torch.float32), 0.1).cpu().numpy()
        _check_plan(want["plan"], ref.blocked(t, blockers, 0.1, lat.origin, lat.shape), 50, 64)
    print(f"pipeline: {got[0]['bbox3d'].shape[0]} detections, {got[0]['rooms']['count'].item()} rooms, "
          f"{int((got[0]['point_room'] >= 0).sum())} of {pcl.shape[0]} points in a room")
    # a row that the down-sampling merged away carries the room of the point it went into; none went nowhere here
    assert down["point_room"].shape == (pcl.shape[0],) and down["point_owner"].shape == (pcl.shape[0],)
    assert down["rooms"]["bbox3d"].shape == (1024, 7)
