"""detection_3d_amd.floorplan without a GPU: the numpy restatement (tests/floorplan_ref.py) on hand-built plans, the
argument checks on CPU tensors, and the host arithmetic (min_cells, room boxes from bounds, the derived lattice)."""
import inspect
import math

import numpy as np
import pytest
import torch

import floorplan_ref as ref


def test_reference_six_rooms():
    """walls 0.1 thick at x = 1, 5, 9, 13 and y = 1, 5, 9, grow 0, cell 0.05, 200 x 280: 6 rooms of 78 x 78 cells and
    one outside component"""
    table = ref.box_table(ref.six_rooms(), 0.0)
    blk = ref.blocked(table, None, 0.05, (0.0, 0.0), (200, 280))
    assert np.array_equal(blk, ref.blocked_full(table, None, 0.05, (0.0, 0.0), (200, 280)))
    label, r, cells, bounds, seed = ref.rooms(blk, ref.min_cells(1.0, 0.05), 1024)
    assert r == 6 and cells[:6].tolist() == [6084] * 6 and (cells[6:] == 0).all()
    assert sorted(np.unique(label).tolist()) == [ref.BLOCKED, ref.OUTSIDE, 0, 1, 2, 3, 4, 5]
    _, n_free = ref.ndimage.label(~blk, structure=ref.FOUR)
    assert n_free == 7
    assert bounds[0].tolist() == [21, 21, 98, 98] and seed[0] == 21 * 280 + 21
    assert bounds[5].tolist() == [181, 101, 258, 178]
    assert (bounds[6:] == [280, 200, -1, -1]).all() and (seed[6:] == -1).all()
    # rooms are numbered by their smallest cell id
    assert (np.diff(seed[:6]) > 0).all()
    boxes = ref.room_boxes(bounds[:6], 0.05, (0.0, 0.0), 0.0, 2.5)
    assert np.allclose(boxes[0], [3.0, 3.0, 0.0, 3.9, 3.9, 2.5, 0.0], atol=1e-12)


def test_reference_small_outside_and_cut_tables():
    blk = np.ones((7, 9), dtype=bool)
    blk[1, 1] = blk[3, 3:6] = blk[5, 1] = False           # three inner components: 1, 3 and 1 cells
    blk[0, 8] = False                                       # a border cell
    label, r, cells, bounds, seed = ref.rooms(blk, 2, 4)
    assert r == 1 and label[3, 4] == 0 and label[1, 1] == ref.SMALL and label[0, 8] == ref.OUTSIDE and label[0, 0] == ref.BLOCKED
    assert cells.tolist() == [3, 0, 0, 0] and bounds[0].tolist() == [3, 3, 5, 3] and seed[0] == 3 * 9 + 3
    label, r, cells, bounds, seed = ref.rooms(blk, 1, 2)
    assert r == 3 and cells.tolist() == [1, 3] and label[5, 1] == 2        # the third room keeps its number, has no row
    # a room that touches the border only at a corner cell is outside
    blk = np.ones((5, 5), dtype=bool)
    blk[0, 0] = blk[1, 0] = blk[1, 1] = blk[2, 1] = False
    label, r, _, _, _ = ref.rooms(blk, 1, 4)
    assert r == 0 and label[2, 1] == ref.OUTSIDE
    blk[0, 0] = blk[1, 0] = True
    label, r, _, _, _ = ref.rooms(blk, 1, 4)
    assert r == 1 and label[2, 1] == 0
    # 4-connectivity: a diagonal does not join
    blk = np.ones((4, 4), dtype=bool)
    blk[1, 1] = blk[2, 2] = False
    assert ref.rooms(blk, 1, 4)[1] == 2


def test_reference_sides_and_points():
    boxes = np.array([ref.wall(2.0, 0.5, 2.0, 3.5), ref.wall(0.5, 0.5, 0.5, 3.5), ref.wall(3.5, 0.5, 3.5, 3.5),
                      ref.wall(0.5, 0.5, 3.5, 0.5), ref.wall(0.5, 3.5, 3.5, 3.5)], dtype=np.float32)
    t = ref.box_table(boxes, 0.1)
    origin, shape = ref.lattice(t, None, 0.25, 2)
    assert origin == (-0.25, -0.25) and shape == (18, 18)
    label, r, cells, _, _ = ref.rooms(ref.blocked_full(t, None, 0.25, origin, shape), 1, 8)
    assert r == 2
    s = ref.sides(ref.box_table(boxes, 0.0), label, 0.25, origin, 0.5)
    assert s[0].tolist() == [0, 1] and s[1].tolist() == [ref.OUTSIDE, 0] and s[2].tolist() == [1, ref.OUTSIDE]
    assert ref.sides(ref.box_table(boxes, 0.0), label, 0.25, origin, 0.01)[0].tolist() == [ref.NONE, ref.NONE]
    pts = np.array([[1.0, 1.0, 0], [3.0, 1.0, 5], [2.0, 2.0, 0], [-9.0, 0, 0], [np.nan, 1, 1], [1, 1, np.inf]], np.float32)
    assert ref.room_of_points(pts, label, 0.25, origin).tolist() == [0, 1, ref.BLOCKED, ref.OUTSIDE, ref.NONE, ref.NONE]


def test_min_cells_and_room_boxes_and_lattice():
    from detection_3d_amd import floorplan as fp
    assert fp.min_cells_of(1.0, 0.05) == ref.min_cells(1.0, 0.05) == int(math.ceil(1.0 / (0.05 * 0.05)))
    assert fp.min_cells_of(0.0, 0.05) == 1 and fp.min_cells_of(1.0, 1.0) == 1 and fp.min_cells_of(1.01, 1.0) == 2
    assert fp.min_cells_of(0.3, 0.25) == 5
    for bad in ((-1.0, 0.05), (1.0, 0.0), (float("nan"), 0.05), (1.0, float("inf")), ("a", 0.05)):
        with pytest.raises(ValueError):
            fp.min_cells_of(*bad)
    bounds = torch.tensor([[21, 21, 98, 98], [0, 3, 0, 3], [5, 1, 6, 4]], dtype=torch.int32)
    got = fp.boxes_from_bounds(bounds, 0.05, (-0.1, 0.3), 0.25, 2.5)
    want = ref.room_boxes(bounds.numpy(), 0.05, (-0.1, 0.3), 0.25, 2.5)
    assert got.dtype == torch.float64 and np.array_equal(got.numpy(), want)
    assert want[1].tolist() == [-0.1 + 0.5 * 0.05, 0.3 + 3.5 * 0.05, 0.25, 0.05, 0.05, 2.5, 0.0]
    lat = fp.lattice_from_extent(0.94, 0.94, 13.06, 9.06, 0.05, 2)
    assert lat.shape == (ref.lattice(np.array([[7.0, 5.0, 1.0, 0.0, 6.06, 4.06]]), None, 0.05, 2)[1])
    assert lat == fp.Lattice(*ref.lattice(np.array([[7.0, 5.0, 1.0, 0.0, 6.06, 4.06]]), None, 0.05, 2))
    with pytest.raises(ValueError):
        fp.lattice_from_extent(0.0, 0.0, 300.0, 1.0, 0.05, 2)
    assert (fp.OUTSIDE, fp.BLOCKED, fp.SMALL, fp.NONE) == (-1, -2, -3, -4) == (ref.OUTSIDE, ref.BLOCKED, ref.SMALL, ref.NONE)


def test_box_table_and_extent_on_cpu_tensors():
    from detection_3d_amd import floorplan as fp
    boxes = np.concatenate([ref.random_plan(3), [[1, 2, 0, 0.5, 2, 1, np.nan]], [[np.inf, 2, 0, 0.5, 2, 1, 0.3]]]).astype(np.float32)
    got = fp.box_table(torch.from_numpy(boxes), 0.1)
    want = ref.box_table(boxes, 0.1)
    assert got.dtype == torch.float64 and got.shape == (boxes.shape[0], 6)
    assert np.array_equal(np.isnan(got.numpy()), np.isnan(want))
    fin = np.isfinite(want)
    assert np.abs(got.numpy()[fin] - want[fin]).max() <= 1e-12
    sel = torch.ones(boxes.shape[0], dtype=torch.bool)
    sel[0] = False
    ext = fp.table_extent(got, sel).tolist()
    assert fp.lattice_from_extent(*ext, 0.05, 3) == fp.Lattice(*ref.lattice(got.numpy(), sel.numpy(), 0.05, 3))
    assert fp.table_extent(got[:0]).tolist() == [0.0] * 4
    assert fp.table_extent(got[-2:]).tolist() == [0.0] * 4          # non-finite rows only
    assert fp.lattice_from_extent(0.0, 0.0, 0.0, 0.0, 0.05, 1).shape == (2, 2)


def _plan(fp, h=4, w=5):
    bm = fp.Bitmap(torch.zeros((h, (w + 31) // 32), dtype=torch.int32), fp.Lattice((0.0, 0.0), (h, w)), 0.05)
    z = torch.zeros
    return fp.Plan(bm, z((h, w), dtype=torch.int32), z(1, dtype=torch.int32), z(8, dtype=torch.int32),
                   z((8, 4), dtype=torch.int32), z(8, dtype=torch.int32), 1, 8)


def test_argument_faults_are_value_errors_on_cpu_tensors():
    from detection_3d_amd import floorplan as fp
    good = torch.zeros((3, 7))
    lat = fp.Lattice((0.0, 0.0), (8, 8))
    bad_boxes = (torch.zeros((3, 6)), torch.zeros(7), torch.zeros((3, 7), dtype=torch.float64), [[0.0] * 7],
                 torch.zeros((4097, 7)))
    for b in bad_boxes:
        for call in (lambda: fp.rasterize(b, lattice=lat), lambda: fp.rooms(b, lattice=lat), lambda: fp.box_table(b),
                     lambda: fp.box_sides(_plan(fp), b)):
            with pytest.raises(ValueError):
                call()
    for kw in ({"cell": 0.0}, {"cell": -1.0}, {"cell": float("nan")}, {"cell": "x"}, {"grow": -0.1}, {"grow": float("inf")},
               {"lattice": ((0.0, 0.0), (0, 8))}, {"lattice": ((0.0, 0.0), (8, 4097))}, {"lattice": ((0.0, float("nan")), (8, 8))},
               {"lattice": (0.0, 0.0, 8, 8)}, {"lattice": ((0.0, 0.0), (8.5, 8))}, {"margin": 0}, {"margin": 1.5},
               {"select": torch.ones(3)}, {"select": torch.ones(4, dtype=torch.bool)}, {"select": [True] * 3}):
        with pytest.raises(ValueError):
            fp.rasterize(good, **dict({"lattice": lat}, **kw))
    for kw in ({"min_area": -1.0}, {"min_area": float("nan")}, {"max_rooms": 0}, {"max_rooms": 2.5}, {"max_rooms": True},
               {"blockers": torch.ones(2, dtype=torch.bool)}, {"blockers": torch.ones(3, dtype=torch.int64)}, {"cell": 0.0},
               {"margin": 0}):
        with pytest.raises(ValueError):
            fp.rooms(good, **dict({"lattice": lat}, **kw))
    plan = _plan(fp)
    for call in (lambda: fp.box_sides(plan, good, reach=-1.0), lambda: fp.box_sides(plan, good, reach=float("nan")),
                 lambda: fp.box_sides(None, good), lambda: fp.room_of_points(torch.zeros((4, 2)), plan),
                 lambda: fp.room_of_points(torch.zeros((4, 3), dtype=torch.float64), plan),
                 lambda: fp.room_of_points(torch.zeros((4, 3)), None), lambda: fp.room_of_points(torch.zeros((4, 3)), plan, origin="max"),
                 lambda: fp.room_of_points(torch.zeros((4, 3)), plan, origin=[0.0, 1.0]),
                 lambda: fp.floorplan_of({"bbox3d": torch.zeros((2, 6)), "labels": torch.zeros(2)}, ["background", "wall"])):
        with pytest.raises(ValueError):
            call()
    for bad in ("yes", 5, {"cells": 0.1}, {"cell": 0.0}, {"grow": -1}, {"reach": "far"}, {"max_rooms": 0}, {"min_area": -2}):
        with pytest.raises(ValueError):
            fp.rooms_kwargs(bad)
    assert fp.rooms_kwargs(None) is None
    assert fp.rooms_kwargs(True) == {"cell": 0.05, "grow": 0.1, "min_area": 1.0, "reach": 0.5, "max_rooms": 1024}
    assert fp.rooms_kwargs({"cell": 0.1, "max_rooms": 16})["max_rooms"] == 16


def test_good_cpu_tensors_raise_d3d_error():
    from detection_3d_amd import floorplan as fp
    from detection_3d_amd._lib import D3DError
    good = torch.zeros((3, 7))
    lat = fp.Lattice((0.0, 0.0), (8, 8))
    plan = _plan(fp)
    for call in (lambda: fp.rasterize(good, lattice=lat), lambda: fp.rasterize(good), lambda: fp.rooms(good, lattice=lat),
                 lambda: fp.rooms(good, torch.ones(3, dtype=torch.bool)), lambda: fp.box_sides(plan, good),
                 lambda: fp.room_of_points(torch.zeros((4, 3)), plan), lambda: fp.room_of_points(torch.zeros((4, 9)), plan, origin="min"),
                 lambda: fp.floorplan_of({"bbox3d": good, "labels": torch.ones(3, dtype=torch.int64)}, ["background", "wall"],
                                         lattice=lat)):
        with pytest.raises(D3DError):
            call()


def test_graph_and_bitmap_view_are_plain_torch():
    from detection_3d_amd import floorplan as fp
    plan = _plan(fp)
    sides = torch.tensor([[0, 1], [1, 0], [2, 2], [-1, 3], [3, -3], [4, 2], [-4, -4]], dtype=torch.int32)
    assert plan.graph(sides).tolist() == [[0, 1, 0], [0, 1, 1], [2, 4, 5]]
    doors = torch.tensor([0, 1, 1, 1, 1, 0, 1], dtype=torch.bool)
    assert plan.graph(sides, doors).tolist() == [[0, 1, 1]]
    assert plan.graph(sides[:0]).shape == (0, 3)
    words = torch.tensor([[5, 1], [-(1 << 31), 2]], dtype=torch.int32)
    bm = fp.Bitmap(words, fp.Lattice((0.0, 0.0), (2, 35)), 0.05)
    want = np.zeros((2, 35), dtype=bool)
    want[0, [0, 2, 32]] = want[1, [31, 33]] = True
    assert np.array_equal(bm.blocked.numpy(), want)


def test_pipeline_takes_the_keyword_last_and_off():
    from detection_3d_amd import floorplan as fp
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.serving import BuildingPipeline
    params = list(inspect.signature(BuildingPipeline.__init__).parameters.values())
    assert params[-1].name == "rooms" and params[-1].default is None
    cfg = get_cfg("4c_Fpn432")
    lat = fp.detector_lattice(cfg, 0.05)
    n = int(math.ceil(cfg.SPARSE3D.VOXEL_FULL_SCALE[0] / cfg.SPARSE3D.VOXEL_SCALE / 0.05)) + 4
    assert lat.origin == (-0.1, -0.1) and lat.shape == (n, n)
    with pytest.raises(ValueError):
        fp.detector_lattice(cfg, 0.01)


def test_parse_rooms_and_room_targets_without_a_room_class():
    from detection_3d_amd import floorplan as fp
    assert fp.parse_rooms(None) is None
    assert fp.parse_rooms("") == {"cell": 0.05, "min_area": 1.0}
    assert fp.parse_rooms("0.1") == {"cell": 0.1, "min_area": 1.0} and fp.parse_rooms("0.1,2.5") == {"cell": 0.1, "min_area": 2.5}
    for bad in ("0", "a,b", "0.1,2,3", "0.1,-1"):
        with pytest.raises(ValueError):
            fp.parse_rooms(bad)
    tg = {"bbox3d": torch.zeros((2, 7)), "labels": torch.tensor([1, 1])}
    out = fp.room_targets(tg, ["background", "wall", "door"])                # no room class: as they are, no device needed
    assert out["bbox3d"] is tg["bbox3d"] and torch.equal(out["labels"], tg["labels"])
    tg = {"bbox3d": torch.zeros((2, 7)), "labels": torch.tensor([1, 2])}
    out = fp.room_targets(tg, ["background", "wall", "room"])                # a room of its own already
    assert out["bbox3d"] is tg["bbox3d"]


def test_hand_drawn_bitmaps():
    from detection_3d_amd import floorplan as fp
    from detection_3d_amd._lib import D3DError
    rs = np.random.RandomState(4)
    for h, w in ((1, 1), (3, 31), (5, 32), (4, 33), (2, 64), (7, 100)):
        blk = rs.rand(h, w) < 0.5
        bm = fp.Bitmap.from_blocked(torch.from_numpy(blk), 0.1, (1.0, -2.0))
        assert bm.words.shape == (h, (w + 31) // 32) and bm.words.dtype == torch.int32
        assert bm.lattice == fp.Lattice((1.0, -2.0), (h, w)) and bm.cell == 0.1
        assert np.array_equal(bm.blocked.numpy(), blk)
    for bad in (torch.zeros((3, 3)), torch.zeros(3, dtype=torch.bool), np.zeros((3, 3), dtype=bool),
                torch.zeros((0, 3), dtype=torch.bool)):
        with pytest.raises(ValueError):
            fp.Bitmap.from_blocked(bad)
    with pytest.raises(ValueError):
        fp.Bitmap.from_blocked(torch.zeros((3, 3), dtype=torch.bool), cell=0.0)
    bm = fp.Bitmap.from_blocked(torch.zeros((3, 3), dtype=torch.bool))
    for call in (lambda: fp.label_rooms(None), lambda: fp.label_rooms(bm, min_area=-1.0), lambda: fp.label_rooms(bm, max_rooms=0)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(D3DError):
        fp.label_rooms(bm)
