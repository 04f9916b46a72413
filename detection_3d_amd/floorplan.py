"""Rooms from detected boxes: a floor plan on the GPU (libd3d_hip, floorplan.hip).  The step after detection that
`points_in_boxes` does not take: which rooms there are, with their area and extent, which doors join which rooms, which
walls and windows face the outside, and which room every point of the scan lies in.  It also gives a scan labelled
through `label_planes` / `targets_from_labels` the `room` boxes that SUNCG's own room nodes give the reference
(suncg_preprocess.py:579-581).

This is geometry on boxes, nothing is learned.  The selected boxes (walls, windows, doors), grown by `grow` on every
side, block the cells of a square lattice whose centre they hold; the free cells are joined over 4-connectivity; a
component that reaches the lattice's border is the outside, a small one is noise, the others are the rooms, numbered by
their smallest cell.  A strip whose full thickness 2 (d3 / 2 + grow) is at least one cell separates its two sides under
4-connectivity at any yaw (one lattice step moves the normal coordinate by at most `cell`), which the default grow of
0.1 m guarantees at the default cell of 0.05 m.  The stated limits: a gap between two walls wider than 2 grow joins
their rooms (a door left out of the blockers does); a box's sides are probed along its centre line only; one storey:
the plan knows no z.

Boxes are yx_zb with the bird's-eye geometry of primitives.points_in_boxes: lx = c (X - xc) - s (Y - yc) runs along
d3, ly = s (X - xc) + c (Y - yc) along d4, +lx points along the world direction (c, -s).  Every output is defined exactly
on the fp64 table of `box_table`; tests/floorplan_ref.py restates the definitions in numpy, bit for bit.

Lattice: cell (iy, ix) of `shape` (H, W), H, W <= 4096, has id iy W + ix and the centre X = ox + (ix + 0.5) cell,
Y = oy + (iy + 0.5) cell; a point lies in ix = floor((x - ox) / cell), iy = floor((y - oy) / cell); a non-finite or
out-of-range index is off the lattice.  All fp64, every operation rounded on its own."""
import math
from collections import namedtuple

import torch

from ._cloud import fp32_cloud, gpu_rows, need_gpu, number, options, run, same_device, scratch, whole, PhaseTimer
from ._lib import ptr, stream_of
from .config import class_to_label
from .primitives import MAX_BOXES, _origin

OUTSIDE, BLOCKED, SMALL, NONE = -1, -2, -3, -4
MAX_SIDE = 4096
BLOCKER_CLASSES = ("wall", "window", "door")
ROOMS_PHASES = ("runs", "links", "roots", "rank", "write")

Lattice = namedtuple("Lattice", "origin shape")      # origin (ox, oy) in metres, shape (H, W) in cells


def _boxes(boxes):
    if (not isinstance(boxes, torch.Tensor) or boxes.dim() != 2 or boxes.shape[1] != 7 or
            boxes.dtype != torch.float32):
        raise ValueError("boxes must be a float32 tensor [K, 7] (yx_zb)")
    if boxes.shape[0] > MAX_BOXES:
        raise ValueError(f"{boxes.shape[0]} boxes: at most {MAX_BOXES} in one call")
    return boxes.detach()


def _select(select, k, what="select"):
    if select is None:
        return None
    if not isinstance(select, torch.Tensor) or select.dtype != torch.bool or tuple(select.shape) != (k,):
        raise ValueError(f"{what} must be None or a bool tensor [{k}]")
    return select.detach()


def _cell(cell):
    return number(cell, "cell", 0.0, lo_open=True)


def _lattice(lattice):
    """None -> None; (origin, shape) -> Lattice((float ox, float oy), (int H, int W))"""
    if lattice is None:
        return None
    try:
        (ox, oy), (h, w) = lattice
    except (TypeError, ValueError):
        raise ValueError(f"lattice must be None or Lattice(origin=(ox, oy), shape=(H, W)), got {lattice!r}") from None
    ox, oy = number(ox, "lattice origin x", -math.inf), number(oy, "lattice origin y", -math.inf)
    return Lattice((ox, oy), (whole(h, "lattice H", 1, MAX_SIDE), whole(w, "lattice W", 1, MAX_SIDE)))


def min_cells_of(min_area, cell):
    """max(1, ceil(min_area / cell^2)) in fp64 on the host: a component of fewer cells is SMALL"""
    return max(1, int(math.ceil(number(min_area, "min_area") / (_cell(cell) * _cell(cell)))))


def box_table(boxes, grow=0.0):
    """boxes fp32 [K, 7] yx_zb -> fp64 [K, 6] on the boxes' device: (xc, yc, c, s, hx, hy), c, s = cos, sin of
    double(yaw), hx = double(d3) / 2 + grow, hy = double(d4) / 2 + grow.  Plain torch (it runs on CPU tensors too);
    everything downstream is defined on this table.  A row with a non-finite entry blocks nothing."""
    g = number(grow, "grow")
    b = _boxes(boxes).to(torch.float64)
    return torch.stack([b[:, 0], b[:, 1], torch.cos(b[:, 6]), torch.sin(b[:, 6]), b[:, 3] / 2 + g, b[:, 4] / 2 + g],
                       1).contiguous()


def lattice_from_extent(x0, y0, x1, y1, cell, margin=2):
    """The lattice around the extent [x0, x1] x [y0, y1] (fp64 on the host): the lower ends floored to a multiple of
    `cell`, the upper ends ceiled, `margin` free cells added on every side."""
    i0, j0 = math.floor(x0 / cell) - margin, math.floor(y0 / cell) - margin
    i1, j1 = math.ceil(x1 / cell) + margin, math.ceil(y1 / cell) + margin
    h, w = j1 - j0, i1 - i0
    if h > MAX_SIDE or w > MAX_SIDE:
        raise ValueError(f"the blockers span {h} x {w} cells of {cell} m: at most {MAX_SIDE} x {MAX_SIDE}; pass a larger "
                         f"cell or an explicit lattice")
    return Lattice((i0 * cell, j0 * cell), (h, w))


def table_extent(table, select=None):
    """(x0, y0, x1, y1) fp64 [4] on the table's device: the extent of the corners xc +- (|c| hx + |s| hy),
    yc +- (|s| hx + |c| hy) of the selected rows without a non-finite entry; (0, 0, 0, 0) when there is none"""
    ok = torch.isfinite(table).all(1)
    if select is not None:
        ok = ok & select
    xc, yc, c, s, hx, hy = table.unbind(1)
    ex = c.abs() * hx + s.abs() * hy
    ey = s.abs() * hx + c.abs() * hy
    inf = torch.full_like(xc, math.inf)
    lo = torch.stack([torch.where(ok, xc - ex, inf), torch.where(ok, yc - ey, inf)])
    hi = torch.stack([torch.where(ok, xc + ex, -inf), torch.where(ok, yc + ey, -inf)])
    if table.shape[0] == 0:
        return torch.zeros(4, dtype=torch.float64, device=table.device)
    ext = torch.cat([lo.amin(1), hi.amax(1)])
    return torch.where(torch.isfinite(ext), ext, torch.zeros_like(ext))


class Bitmap(object):
    """words int32 [H, ceil(W / 32)] on the device: bit ix & 31 of word ix >> 5 of row iy is set iff cell (iy, ix) is
    blocked; `lattice`, `cell` as given or derived; `blocked`: the same as a bool tensor [H, W]."""

    def __init__(self, words, lattice, cell):
        self.words, self.lattice, self.cell = words, lattice, cell

    @classmethod
    def from_blocked(cls, blocked, cell=0.05, origin=(0.0, 0.0)):
        """blocked bool [H, W] (a plan drawn by hand, or edited) -> the Bitmap of it on the tensor's device.  Plain
        torch."""
        if not isinstance(blocked, torch.Tensor) or blocked.dtype != torch.bool or blocked.dim() != 2:
            raise ValueError("blocked must be a bool tensor [H, W]")
        lattice = _lattice((origin, tuple(blocked.shape)))
        h, w = lattice.shape
        nw = (w + 31) // 32
        bits = torch.zeros((h, nw * 32), dtype=torch.int64, device=blocked.device)
        bits[:, :w] = blocked
        words = (bits.reshape(h, nw, 32) << torch.arange(32, device=blocked.device)).sum(2)
        words = torch.where(words >= (1 << 31), words - (1 << 32), words).to(torch.int32)
        return cls(words.contiguous(), lattice, _cell(cell))

    @property
    def blocked(self):
        h, w = self.lattice.shape
        bits = (self.words.unsqueeze(2) >> torch.arange(32, device=self.words.device, dtype=torch.int32)) & 1
        return bits.reshape(h, -1)[:, :w].to(torch.bool)


def _lattice_args(cell, lat):
    return cell, lat.origin[0], lat.origin[1], lat.shape[0], lat.shape[1]


def _raster(boxes, select, cell, lattice, grow, margin):
    """the checks of rasterize / rooms that need no device, then the table, the lattice and the raster"""
    boxes = _boxes(boxes)
    k = boxes.shape[0]
    select = _select(select, k)
    cell, grow, lattice = _cell(cell), number(grow, "grow"), _lattice(lattice)
    margin = whole(margin, "margin", 1)
    need_gpu(boxes.device, "boxes")
    dev = same_device(boxes=boxes, select=select)
    table = box_table(boxes, grow)
    if lattice is None:
        lattice = lattice_from_extent(*table_extent(table, select).tolist(), cell, margin)     # the one read-back
    h, w = lattice.shape
    words = torch.empty((h, (w + 31) // 32), dtype=torch.int32, device=dev)
    sel = None if select is None else select.to(torch.uint8).contiguous()
    run(dev, "d3d_floorplan_raster", ptr(table), ptr(sel), k, *_lattice_args(cell, lattice), ptr(words), stream_of(dev))
    return Bitmap(words, lattice, cell)


def rasterize(boxes, select=None, cell=0.05, lattice=None, grow=0.1, margin=2):
    """boxes fp32 [K, 7] yx_zb on the GPU, K <= 4096; select: None (all) or bool [K] on the same GPU.  Cell (iy, ix) is
    blocked iff for at least one selected box |lx| <= d3 / 2 + grow and |ly| <= d4 / 2 + grow at the cell's centre (faces
    closed; the arithmetic: the module's docstring and include/d3d_hip.h).  lattice: a Lattice(origin, shape), or None
    for the one around the selected boxes' corners with `margin` (>= 1) free cells on every side, which costs one
    read-back of four numbers; an explicit lattice costs none.  -> Bitmap.  Runs on the current stream."""
    return _raster(boxes, select, cell, lattice, grow, margin)


def boxes_from_bounds(bounds, cell, origin, z_bot=0.0, height=0.0):
    """bounds integer [R, 4] (ix_min, iy_min, ix_max, iy_max) -> fp64 [R, 7] yaw-0 yx_zb rows: xc = ox + (ix_min + ix_max
    + 1) / 2 cell, d3 = (ix_max - ix_min + 1) cell, y likewise with d4; z_bot and height as given.  Plain torch."""
    b = bounds.to(torch.float64)
    ox, oy = origin
    out = torch.zeros((b.shape[0], 7), dtype=torch.float64, device=bounds.device)
    out[:, 0] = ox + (b[:, 0] + b[:, 2] + 1) / 2 * cell
    out[:, 1] = oy + (b[:, 1] + b[:, 3] + 1) / 2 * cell
    out[:, 2] = z_bot
    out[:, 3] = (b[:, 2] - b[:, 0] + 1) * cell
    out[:, 4] = (b[:, 3] - b[:, 1] + 1) * cell
    out[:, 5] = height
    return out


class Plan(object):
    """What `rooms` returns, all on the device: label int32 [H, W] (a room's number, OUTSIDE, BLOCKED or SMALL per cell),
    count_dev int32 [1] (R), cells int32 [max_rooms], bounds int32 [max_rooms, 4] (ix_min, iy_min, ix_max, iy_max), seed
    int32 [max_rooms] (the room's smallest cell id); rows from R on hold 0, (W, H, -1, -1) and -1; rooms from max_rooms
    on keep their number in label and have no row.  bitmap, lattice, cell, min_cells, max_rooms: what it was made with.
    `count`, `area` and `room_boxes` read R back on first use, like register.Registration."""

    def __init__(self, bitmap, label, count_dev, cells, bounds, seed, min_cells, max_rooms, phase_ms=None):
        self.bitmap, self.lattice, self.cell = bitmap, bitmap.lattice, bitmap.cell
        self.label, self.count_dev, self.cells, self.bounds, self.seed = label, count_dev, cells, bounds, seed
        self.min_cells, self.max_rooms, self.phase_ms = min_cells, max_rooms, phase_ms
        self._count = None

    @property
    def count(self):
        """R, the number of rooms (it may exceed max_rooms)"""
        if self._count is None:
            self._count = int(self.count_dev.item())
        return self._count

    @property
    def listed(self):
        """min(R, max_rooms): the rows of the tables that hold a room"""
        return min(self.count, self.max_rooms)

    @property
    def area(self):
        """fp64 [listed] on the device: cells cell^2"""
        return self.cells[:self.listed].to(torch.float64) * (self.cell * self.cell)

    def room_boxes(self, z_bot=0.0, height=0.0):
        """fp32 [listed, 7]: one yaw-0 yx_zb row per room from its bounds (boxes_from_bounds)"""
        return boxes_from_bounds(self.bounds[:self.listed], self.cell, self.lattice.origin, z_bot,
                                 height).to(torch.float32)

    def graph(self, sides, select=None):
        """sides int [K, 2] (box_sides) -> int64 [E, 3] rows (room a < room b, box index): the boxes (select: None or
        bool [K], the doors say) with a room on either side, and not the same one, in box order.  Plain torch."""
        a, b = sides[:, 0].to(torch.int64), sides[:, 1].to(torch.int64)
        link = (a >= 0) & (b >= 0) & (a != b)
        if select is not None:
            link = link & select.to(link.device)
        j = torch.nonzero(link).reshape(-1)
        return torch.stack([torch.minimum(a[j], b[j]), torch.maximum(a[j], b[j]), j], 1)


def _rooms_of(bitmap, min_cells, max_rooms, phases=False):
    dev = bitmap.words.device
    h, w = bitmap.lattice.shape
    label = torch.empty((h, w), dtype=torch.int32, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    cells = torch.empty((max_rooms,), dtype=torch.int32, device=dev)
    bounds = torch.empty((max_rooms, 4), dtype=torch.int32, device=dev)
    seed = torch.empty((max_rooms,), dtype=torch.int32, device=dev)
    buf, nbytes = scratch(dev, "d3d_floorplan_scratch_bytes", h, w, 0)
    timer = PhaseTimer(ROOMS_PHASES, phases)
    run(dev, "d3d_floorplan_rooms", ptr(bitmap.words), h, w, min_cells, max_rooms, ptr(label), ptr(count), ptr(cells),
        ptr(bounds), ptr(seed), ptr(buf), nbytes, stream_of(dev), timer.ms)
    return Plan(bitmap, label, count, cells, bounds, seed, min_cells, max_rooms, timer.read())


def label_rooms(bitmap, min_area=1.0, max_rooms=1024, return_phases=False):
    """The rooms of a Bitmap on the GPU (`rooms` without the raster; Bitmap.from_blocked takes a plan drawn by hand)
    -> Plan"""
    if not isinstance(bitmap, Bitmap):
        raise ValueError(f"bitmap must be a floorplan.Bitmap, got {type(bitmap).__name__}")
    min_cells = min_cells_of(min_area, bitmap.cell)
    max_rooms = whole(max_rooms, "max_rooms", 1, 1 << 24)
    need_gpu(bitmap.words.device, "bitmap")
    return _rooms_of(bitmap, min_cells, max_rooms, return_phases)


def rooms(boxes, blockers=None, cell=0.05, lattice=None, grow=0.1, min_area=1.0, max_rooms=1024, margin=2,
          return_phases=False):
    """The rooms between the blockers: boxes, blockers (None: every box, or bool [K]: the walls, windows and doors),
    cell, lattice, grow and margin as `rasterize` takes them.  Free cells are joined over 4-connectivity; a component
    with a cell on the lattice's border is OUTSIDE, one of fewer than max(1, ceil(min_area / cell^2)) cells is SMALL,
    the others are the rooms 0 .. R - 1 by ascending smallest cell id.  A strip of full thickness 2 (d3 / 2 + grow) >=
    cell separates its sides at any yaw; a gap between two walls wider than 2 grow joins their rooms: this is geometry
    on boxes and nothing is learned.  -> Plan.  Integer min, max and add only: the same boxes in any order give the same
    bits.  Runs on the current stream; no read-back with an explicit lattice.  return_phases: Plan.phase_ms holds the
    milliseconds of the labelling's phases (the call then synchronises)."""
    _boxes(boxes)
    _select(blockers, boxes.shape[0], "blockers")
    min_cells = min_cells_of(min_area, cell)
    max_rooms = whole(max_rooms, "max_rooms", 1, 1 << 24)
    bitmap = _raster(boxes, blockers, cell, lattice, grow, margin)
    return _rooms_of(bitmap, min_cells, max_rooms, return_phases)


def box_sides(plan, boxes, reach=0.5):
    """What lies on either side of every box (of any class): boxes fp32 [K, 7] on the plan's GPU.  Probe p = 0 ..
    ceil(reach / cell) - 1 of a side sits at t = -+(d3 / 2 + (p + 0.5) cell) along lx, the world point (xc + c t, yc -
    s t); the first probe whose cell is not BLOCKED gives the side's value (a room, OUTSIDE or SMALL), a probe off the
    lattice gives OUTSIDE and ends the walk, no value within reach is NONE.  -> int32 [K, 2], column 0 the -lx side: a
    door with two different rooms links them, a wall or window with OUTSIDE on one side is on the facade.  The walk
    follows the box's centre line only."""
    if not isinstance(plan, Plan):
        raise ValueError(f"plan must be a floorplan.Plan, got {type(plan).__name__}")
    boxes = _boxes(boxes)
    n_probe = int(math.ceil(number(reach, "reach") / plan.cell))
    need_gpu(boxes.device, "boxes")
    dev = same_device(label=plan.label, boxes=boxes)
    k = boxes.shape[0]
    table = box_table(boxes, 0.0)
    sides = torch.empty((k, 2), dtype=torch.int32, device=dev)
    run(dev, "d3d_floorplan_sides", ptr(table), k, ptr(plan.label), *_lattice_args(plan.cell, plan.lattice), n_probe,
        ptr(sides), stream_of(dev))
    return sides


def room_of_points(xyz, plan, origin=None):
    """xyz fp32 [N, >= 3] on the plan's GPU, read in place like primitives.points_in_boxes; origin as there (None, a
    3-vector, or 'min' for the cloud's own minimum), subtracted in fp64 first.  -> int32 [N]: the plan's label of the
    point's cell (a room, OUTSIDE, BLOCKED or SMALL), OUTSIDE off the lattice, NONE for a non-finite position."""
    fp32_cloud(xyz)
    if not isinstance(plan, Plan):
        raise ValueError(f"plan must be a floorplan.Plan, got {type(plan).__name__}")
    if isinstance(origin, str) and origin != "min":
        raise ValueError(f"origin must be None, a 3-vector or 'min', got {origin!r}")
    o = origin if origin is None or isinstance(origin, str) else _origin(origin, torch.empty(0))
    xyz, n, stride = gpu_rows(xyz)
    dev = same_device(xyz=xyz, label=plan.label)
    o = _origin(o, xyz) if isinstance(o, str) else (None if o is None else o.to(dev))
    room = torch.empty((n,), dtype=torch.int32, device=dev)
    run(dev, "d3d_floorplan_points", ptr(xyz), n, stride, ptr(o), ptr(plan.label),
        *_lattice_args(plan.cell, plan.lattice), ptr(room), stream_of(dev))
    return room


ROOMS_KEYS = ("cell", "grow", "min_area", "reach", "max_rooms")


def rooms_kwargs(value):
    """The `rooms=` keyword of serving.BuildingPipeline: None -> None, True -> the defaults, a dict with keys among
    cell, grow, min_area, reach, max_rooms -> a checked copy with every key."""
    if value is None or value is False:
        return None
    kw = {"cell": 0.05, "grow": 0.1, "min_area": 1.0, "reach": 0.5, "max_rooms": 1024}
    if value is not True:
        kw.update(options(value, "rooms", ROOMS_KEYS, "None, True"))
    kw["cell"], kw["grow"], kw["reach"] = _cell(kw["cell"]), number(kw["grow"], "grow"), number(kw["reach"], "reach")
    kw["min_area"] = number(kw["min_area"], "min_area")
    kw["max_rooms"] = whole(kw["max_rooms"], "max_rooms", 1, 1 << 24)
    return kw


def detector_lattice(cfg, cell, margin=2):
    """The lattice of the detections' min-shifted frame, known without a look at them: origin (-margin cell, -margin
    cell), shape ceil(VOXEL_FULL_SCALE / VOXEL_SCALE / cell) + 2 margin per axis (x is W, y is H)."""
    s3d = cfg.SPARSE3D
    w, h = (int(math.ceil(float(s3d.VOXEL_FULL_SCALE[d]) / float(s3d.VOXEL_SCALE) / cell)) + 2 * margin for d in (0, 1))
    if h > MAX_SIDE or w > MAX_SIDE:
        raise ValueError(f"rooms: the detector's lattice has {h} x {w} cells of {cell} m, at most {MAX_SIDE} x {MAX_SIDE}: "
                         f"pass a larger cell")
    return Lattice((-margin * cell, -margin * cell), (h, w))


def point_rooms(kept, raw, plan):
    """serving: room_of_points for every row of the raw cloud, carried through prepare.Kept exactly as point_owner is:
    NONE for a row that went nowhere"""
    room = room_of_points(raw if kept.cloud is None else kept.cloud, plan, origin="min")
    if kept.source is not None:
        table = torch.cat([room, torch.full((1,), NONE, dtype=room.dtype, device=room.device)])
        room = table[kept.source.long()]
    return room


def floorplan_of(result_or_targets, classes, reach=0.5, **kw):
    """The floor plan of a detection result or of training targets: a dict with "bbox3d" [K, 7] yx_zb and "labels" [K]
    (config.class_to_label ids of `classes`, the config's class list).  The blockers are the boxes of the classes wall,
    window and door that the list has; **kw go to `rooms`.  -> {"plan": the Plan, "rooms": {"bbox3d" fp32 [max_rooms, 7]
    (Plan.room_boxes' rows with z_bot the blockers' lowest z_bot and dz up to their highest top; zero rows from R on),
    "area" fp64 [max_rooms], "count" int32 [1]}, "box_rooms": box_sides of every box}.  Everything stays on the device
    and nothing is read back with an explicit lattice; cut the tables with plan.count."""
    c2l = class_to_label(classes)
    boxes = torch.as_tensor(result_or_targets["bbox3d"])
    labels = torch.as_tensor(result_or_targets["labels"])
    if boxes.dim() != 2 or boxes.shape[1] != 7 or labels.dim() != 1 or labels.shape[0] != boxes.shape[0]:
        raise ValueError("floorplan_of: \"bbox3d\" [K, 7] and \"labels\" [K]")
    boxes = boxes.detach().to(torch.float32)
    labels = labels.detach().to(boxes.device)
    blockers = torch.zeros(boxes.shape[0], dtype=torch.bool, device=boxes.device)
    for c in BLOCKER_CLASSES:
        if c in c2l:
            blockers |= labels == c2l[c]
    plan = rooms(boxes, blockers, **kw)
    sides = box_sides(plan, boxes, reach)
    z = boxes.to(torch.float64)
    inf = torch.full_like(z[:, 2], math.inf)
    zero = torch.zeros((), dtype=torch.float64, device=boxes.device)
    if boxes.shape[0]:
        z0, z1 = torch.where(blockers, z[:, 2], inf).amin(), torch.where(blockers, z[:, 2] + z[:, 5], -inf).amax()
        z0, z1 = torch.where(torch.isfinite(z0), z0, zero), torch.where(torch.isfinite(z1), z1, zero)
    else:
        z0 = z1 = zero
    rows = boxes_from_bounds(plan.bounds, plan.cell, plan.lattice.origin)
    rows[:, 2], rows[:, 5] = z0, z1 - z0
    listed = (plan.seed >= 0).unsqueeze(1)
    rows = torch.where(listed, rows, torch.zeros_like(rows)).to(torch.float32)
    area = plan.cells.to(torch.float64) * (plan.cell * plan.cell)
    return {"plan": plan, "rooms": {"bbox3d": rows, "area": area, "count": plan.count_dev}, "box_rooms": sides}


def parse_rooms(spec):
    """--rooms[=CELL,MIN_AREA] -> None (not given), or {"cell", "min_area"} (defaults 0.05 m and 1.0 m^2)"""
    if spec is None:
        return None
    kw = {"cell": 0.05, "min_area": 1.0}
    parts = [p for p in spec.split(",")] if spec else []
    if len(parts) > 2:
        raise ValueError(f"--rooms takes CELL,MIN_AREA, got {spec!r}")
    try:
        for key, p in zip(("cell", "min_area"), parts):
            kw[key] = float(p)
    except ValueError:
        raise ValueError(f"--rooms takes CELL,MIN_AREA, got {spec!r}") from None
    kw["cell"], kw["min_area"] = _cell(kw["cell"]), number(kw["min_area"], "min_area")
    return kw


def room_targets(targets, classes, **kw):
    """Training targets {"bbox3d" [K, 7] yx_zb on the GPU, "labels" [K]} with one `room` box per room appended (yaw 0,
    from the room's bounds; z_bot the walls' lowest and the top their highest): for a scan whose boxes were fitted to
    labelled points and that has no room nodes of its own.  Nothing is added when `classes` has no `room` or the targets
    hold a room already.  **kw go to `rooms` (cell, grow, min_area, ...).  One read-back for the lattice, one for R."""
    c2l = class_to_label(classes)
    boxes, labels = targets["bbox3d"], torch.as_tensor(targets["labels"])
    if "room" not in c2l or bool((labels == c2l["room"]).any()):
        return {"bbox3d": boxes, "labels": labels}
    labels_dev = labels.to(boxes.device)
    blockers = torch.zeros(boxes.shape[0], dtype=torch.bool, device=boxes.device)
    for c in BLOCKER_CLASSES:
        if c in c2l:
            blockers |= labels_dev == c2l[c]
    plan = rooms(boxes.to(torch.float32), blockers, **kw)
    walls = labels_dev == c2l["wall"] if "wall" in c2l else blockers
    if plan.count == 0 or not bool(walls.any()):
        return {"bbox3d": boxes, "labels": labels}
    z = boxes[walls].to(torch.float64)
    z0, z1 = float(z[:, 2].min()), float((z[:, 2] + z[:, 5]).max())
    added = plan.room_boxes(z0, z1 - z0).to(boxes.dtype)
    room = torch.full((added.shape[0],), c2l["room"], dtype=labels.dtype, device=labels.device)
    return {"bbox3d": torch.cat([boxes, added]), "labels": torch.cat([labels, room])}
