"""The points of each box: which points of a cloud lie in which rotated box, how many, and how far along each box they
reach -- the step after detection (the supporting points of every wall, window, door, floor and ceiling) and the step
before training on cropped scenes (the reference prepares every split scene with it: Bbox3D.points_in_bbox,
utils3d/bbox3d_ops.py:731-755; split_bbox, data3d/indoor_data_util.py:214-316; Bbox3D.crop_bbox_by_points,
bbox3d_ops.py:850-926).

`points_in_boxes` is one call on the GPU (libd3d_hip, points_in_boxes.hip) that builds no [N, K] mask; `point_lists`,
`crop_boxes` and `random_window` are plain torch on small tensors and run on CPU tensors too; `crop_scene` composes them.
`fit_boxes` is the inverse (box_fit.hip): the box of the points of every labelled instance, which `targets_from_labels`
turns into training targets for scans that come with an instance id per point and no boxes.

Boxes are yx_zb (xc, yc, z_bot, d3, d4, dz, yaw) with the BEV geometry of the IoU kernels: in the box frame
lx = c (X - xc) - s (Y - yc) runs along the thickness d3, ly = s (X - xc) + c (Y - yc) along the length d4 (c, s = cos, sin
of yaw: a wall along the world's x axis has yaw +-pi/2), lz = Z - z_bot upwards.  Detections live in the cloud's
min-shifted frame (voxelize, scene_targets): pass origin='min' with a raw cloud."""
import math

import numpy as np
import torch

from ._cloud import fp32_cloud, gpu_cloud, gpu_rows, need_gpu, options, run, same_device, scratch, whole
from ._lib import ptr, stream_of
from .config import class_to_label
from .scene_io import _ZERO_YAW_CLASSES

MAX_BOXES = 4096
THICKNESS_AUG = 0.3            # split_bbox's thickness_aug: the clip of the box sizes its counts are taken with
MIN_POINTS_PER_M2 = 10.0       # split_bbox: min_point_num_per1sm
MIN_POINTS_CAP = 200.0
MIN_POINTS_ANY = 10            # crop_bbox_by_points: fewer grown-box points than this, no box
MIN_LENGTH = 0.2               # split_bbox step (4): min_wall_size_x
FIT_CHUNK = 1024               # box_fit.hip kChunk: the sorted rows one workgroup of fit_boxes' sweep takes
FIT_Q = math.pi / 65536        # fit_boxes' fine step of yaw


def _sizes(values, what, names):
    """-> a list of len(names) finite floats >= 0"""
    try:
        v = [float(x) for x in values]
    except TypeError:
        raise ValueError(f"{what} must be ({', '.join(names)}), got {values!r}") from None
    if len(v) != len(names) or not all(0.0 <= x < float("inf") for x in v):
        raise ValueError(f"{what} must be {len(names)} finite values >= 0 ({', '.join(names)}), got {values!r}")
    return v


def _grow(grow):
    return _sizes(grow, "grow", ("grow_yx", "grow_z"))


def cloud_min(xyz):
    """per-axis minimum of the first three columns as fp64 [3] on the cloud's device, NaN rows ignored (zeros for an
    empty cloud): the shift voxelize applies, without a host read-back"""
    p = xyz[:, :3]
    if p.shape[0] == 0:
        return torch.zeros(3, dtype=torch.float64, device=xyz.device)
    p = torch.where(torch.isnan(p), torch.full_like(p, float("inf")), p)
    return p.amin(0).to(torch.float64)


def _origin(origin, xyz):
    if origin is None:
        return None
    if isinstance(origin, str):
        if origin != "min":
            raise ValueError(f"origin must be None, a 3-vector or 'min', got {origin!r}")
        return cloud_min(xyz)
    o = torch.as_tensor(origin, dtype=torch.float64).reshape(-1)
    if o.numel() != 3:
        raise ValueError(f"origin must be None, a 3-vector or 'min', got {tuple(o.shape)} values")
    return o.to(xyz.device).contiguous()


def points_in_boxes(xyz, boxes, grow=(0.0, 0.0), origin=None):
    """xyz fp32 [N, >= 3] on the GPU (the first three columns are the position; an [N, 9] cloud or its `[:, :3]` slice is
    read in place), boxes fp32 [K, 7] yx_zb on the same GPU, K <= 4096, in descending score order where ownership matters.
    grow = (grow_yx, grow_z): the horizontal sizes count as at least grow_yx and the height as at least grow_z
    ((0.3, 0.3) is split_bbox's clip).  origin: None, a 3-vector or tensor subtracted from every point in fp64, or 'min' for
    the cloud's own per-axis minimum (the frame of the detections of that cloud).
    -> owner int32 [N] (lowest box index that holds the point, -1: none), count int32 [K] (all members of each box),
    lo, hi fp32 [K, 3] (minimum and maximum of (lx, ly, lz) over each box's members; +inf / -inf for an empty box).
    Membership is closed on every face and a NaN point belongs to nothing.  Runs on the current stream without a host
    read-back; the same input gives the same bits."""
    g = _grow(grow)
    fp32_cloud(xyz)
    if (not isinstance(boxes, torch.Tensor) or boxes.dim() != 2 or boxes.shape[1] != 7 or
            boxes.dtype != torch.float32):
        raise ValueError("boxes must be a float32 tensor [K, 7] (yx_zb)")
    k = boxes.shape[0]
    if k > MAX_BOXES:
        raise ValueError(f"{k} boxes: at most {MAX_BOXES} in one call")
    xyz, n, stride = gpu_rows(xyz)
    need_gpu(boxes.device)
    dev = same_device(xyz=xyz, boxes=boxes)
    boxes = boxes.detach().contiguous()
    o = _origin(origin, xyz)
    owner = torch.empty((n,), dtype=torch.int32, device=dev)
    count = torch.empty((k,), dtype=torch.int32, device=dev)
    lo = torch.empty((k, 3), dtype=torch.float32, device=dev)
    hi = torch.empty((k, 3), dtype=torch.float32, device=dev)
    run(dev, "d3d_points_in_boxes", ptr(xyz), n, stride, ptr(o), ptr(boxes), k, g[0], g[1], ptr(owner), ptr(count),
        ptr(lo), ptr(hi), stream_of(dev))
    return owner, count, lo, hi


_FIT_TABLES = {}     # device -> (coarse, fine) fp64 [256, 2]


def _fit_tables(dev):
    """(cos, sin) of the 256 coarse directions a 128 Q and of the 256 fine turns (i - 128) Q, in numpy on the host: the
    library takes them as they are, so that no device cos / sin enters a fitted box"""
    t = _FIT_TABLES.get(dev)
    if t is None:
        a = np.arange(256, dtype=np.float64)
        coarse = np.stack([np.cos(a * 128 * FIT_Q), np.sin(a * 128 * FIT_Q)], 1)
        fine = np.stack([np.cos((a - 128) * FIT_Q), np.sin((a - 128) * FIT_Q)], 1)
        t = _FIT_TABLES[dev] = (torch.from_numpy(coarse).to(dev), torch.from_numpy(fine).to(dev))
    return t


def _fit_lists(xyz, inst, k, o):
    """the point lists of fit_boxes: a stable sort of the masked ids (k: belongs to nothing, sorts last) and the first
    sorted position of every id -> (order int32 [N], sorted ids int32 [N], offsets int32 [k + 1]); no read-back"""
    pos = xyz[:, :3]
    if o is not None:
        pos = (pos.to(torch.float64) - o).to(torch.float32)        # the kernel's own shift, for the finite test
    ok = (inst >= 0) & (inst < k) & torch.isfinite(pos).all(1)
    srt, order = torch.sort(torch.where(ok, inst, torch.full_like(inst, k)), stable=True)
    offsets = torch.searchsorted(srt, torch.arange(k + 1, dtype=torch.int64, device=xyz.device)).to(torch.int32)
    return order.to(torch.int32), srt.to(torch.int32), offsets


def _fit_call(xyz, o, order, srt, offsets, k, yaw_free, phase_ms=None):
    """d3d_fit_boxes on the lists of _fit_lists -> boxes, count, choice, extent; phase_ms: a ctypes float [2] that takes
    the milliseconds of the two passes (the call then synchronises)"""
    xyz, n, stride = gpu_rows(xyz)
    dev = xyz.device
    free = None if yaw_free is None else yaw_free.to(dev).to(torch.uint8).contiguous()
    boxes = torch.empty((k, 7), dtype=torch.float32, device=dev)
    count = torch.empty((k,), dtype=torch.int32, device=dev)
    choice = torch.empty((k, 2), dtype=torch.int32, device=dev)
    extent = torch.empty((k, 6), dtype=torch.float32, device=dev)
    if k > 0:
        coarse, fine = _fit_tables(dev)
        buf, nbytes = scratch(dev, "d3d_fit_boxes_scratch_bytes", k)
        run(dev, "d3d_fit_boxes", ptr(xyz), n, stride, ptr(o), ptr(order), ptr(srt), ptr(offsets), k, ptr(free),
            ptr(coarse), ptr(fine), ptr(boxes), ptr(count), ptr(choice), ptr(extent), ptr(buf), nbytes, stream_of(dev),
            phase_ms)
    return boxes, count, choice, extent


def fit_boxes(xyz, instance, k=None, yaw_free=None, origin=None, return_details=False):
    """The yx_zb box of the points of every instance: xyz fp32 [N, >= 3] on the GPU (read in place like points_in_boxes,
    `origin` as there), instance an integer tensor [N] on the same GPU with an id in [0, k) per row; a row with a
    negative id, an id >= k or a non-finite coordinate belongs to nothing.  k=None takes max(instance) + 1 with one host
    read-back, an explicit k (<= 4096) issues none.  yaw_free: bool [k], None for all free; an instance that is not free
    (floor, ceiling, room) gets yaw 0 and its sizes along the world's x and y.
    Per instance the call sweeps 256 coarse directions over a quarter turn, then 256 fine ones around the best, and
    keeps the one whose extents u = c x - s y, v = s x + c y enclose the smallest area (the lowest index among equals):
    the best of 256 + 256 candidates to pi / 65536 = 0.00275 degrees, not the rotating-calipers optimum of a hull.  A free
    box has d3 <= d4 and yaw in [-pi/2, pi/2); z_bot and dz are the points' own.  The exact arithmetic: include/d3d_hip.h,
    d3d_fit_boxes.
    -> boxes fp32 [k, 7], count int32 [k]; with return_details also choice int32 [k, 2] (coarse, fine index) and extent
    fp32 [k, 6] (umin, umax, vmin, vmax, zmin, zmax of the chosen direction).  An instance without points: a zero row,
    count 0, choice (-1, -1), extents +inf / -inf.  Only min, max and integer arithmetic: the bits depend on the set of
    points alone, not on the order of the rows.  Runs on the current stream."""
    n = fp32_cloud(xyz).shape[0]
    if (not isinstance(instance, torch.Tensor) or instance.dim() != 1 or instance.dtype.is_floating_point or
            instance.dtype.is_complex or instance.dtype == torch.bool):
        raise ValueError("instance must be an integer tensor [N]")
    if instance.shape[0] != n:
        raise ValueError(f"instance holds {instance.shape[0]} ids, xyz {n} rows")
    if k is not None:
        k = int(k)
        if k < 0:
            raise ValueError(f"k {k} < 0")
        if k > MAX_BOXES:
            raise ValueError(f"{k} instances: at most {MAX_BOXES} in one call")
    if yaw_free is not None:
        yaw_free = torch.as_tensor(yaw_free)
        if yaw_free.dtype != torch.bool or yaw_free.dim() != 1 or (k is not None and yaw_free.shape[0] != k):
            raise ValueError(f"yaw_free must be a bool tensor [k], got {yaw_free.dtype} {tuple(yaw_free.shape)}")
    if isinstance(origin, str) and origin != "min":
        raise ValueError(f"origin must be None, a 3-vector or 'min', got {origin!r}")
    o = origin if origin is None or isinstance(origin, str) else _origin(origin, torch.empty(0))
    xyz = gpu_cloud(xyz)                     # _fit_call reads it in place; the lists above it take the view as it is
    need_gpu(instance.device)
    dev = same_device(xyz=xyz, instance=instance)
    inst = instance.detach().to(torch.int64)
    if k is None:
        k = max(int(inst.max()) + 1, 0) if n else 0
        if k > MAX_BOXES:
            raise ValueError(f"{k} instances: at most {MAX_BOXES} in one call")
        if yaw_free is not None and yaw_free.shape[0] != k:
            raise ValueError(f"yaw_free must be a bool tensor [{k}], got {tuple(yaw_free.shape)}")
    o = _origin(o, xyz) if isinstance(o, str) else (None if o is None else o.to(dev))
    order, srt, offsets = _fit_lists(xyz, inst, k, o)
    boxes, count, choice, extent = _fit_call(xyz, o, order, srt, offsets, k, yaw_free)
    return (boxes, count, choice, extent) if return_details else (boxes, count)


def _min_size(min_size):
    return _sizes(min_size, "min_size", ("d3", "d4", "dz"))


def fit_kwargs(fit):
    """The `fit=` keyword of the loops: None -> targets_from_labels' defaults; a dict with keys among min_points,
    min_size -> a checked copy."""
    kw = {"min_points": MIN_POINTS_ANY, "min_size": (0.0, 0.0, 0.0)}
    kw.update(options(fit, "fit", tuple(kw)) or {})
    kw["min_points"] = whole(kw["min_points"], "fit: min_points", 0)
    kw["min_size"] = tuple(_min_size(kw["min_size"]))
    return kw


def is_labelled(targets):
    """targets of the form {"instance": int [N], "instance_labels": int64 [K]}: a scan with an instance id per point
    instead of boxes"""
    return isinstance(targets, dict) and "instance" in targets and "instance_labels" in targets


def targets_from_labels(pcl, instance, instance_labels, min_points=MIN_POINTS_ANY, min_size=(0, 0, 0), classes=None):
    """Training targets of a scan that carries an instance id per point: pcl fp32 [N, >= 3] on the GPU, instance an integer
    tensor [N] (fit_boxes), instance_labels int64 [K], the label id (config.class_to_label) of every instance, 0 for one
    that is not a target.  classes: the config's class list (cfg.INPUT.CLASSES); the instances of its floor, ceiling and
    room classes (scene_io._ZERO_YAW_CLASSES, which scene_targets passes through set_yaw_zero) are fitted with yaw 0;
    None: every instance is free.  An instance is dropped when its label is 0 or it has fewer than min_points points.
    min_size = (d3, d4, dz): smaller sizes are widened to these about the box's middle (a wall scanned from one side has no
    thickness of its own).
    -> {"bbox3d" fp32 [M, 7] yx_zb, "labels" int64 [M]} on the cloud's device and in the cloud's own frame."""
    ms = _min_size(min_size)
    min_points = whole(min_points, "min_points", 0)
    labels = torch.as_tensor(instance_labels)
    if labels.dim() != 1 or labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError("instance_labels must be an integer tensor [K]")
    k = labels.shape[0]
    if k > MAX_BOXES:
        raise ValueError(f"{k} instances: at most {MAX_BOXES} in one call")
    labels = labels.to(torch.int64)
    fixed = []
    if classes is not None:
        c2l = class_to_label(classes)
        fixed = [c2l[c] for c in _ZERO_YAW_CLASSES if c in c2l]
    free = torch.ones(k, dtype=torch.bool, device=labels.device)
    for f in fixed:
        free &= labels != f
    if isinstance(instance, torch.Tensor) and isinstance(pcl, torch.Tensor) and instance.device != pcl.device:
        instance = instance.to(pcl.device)
    boxes, count = fit_boxes(pcl, instance, k=k, yaw_free=free)
    labels = labels.to(boxes.device)
    keep = (labels > 0) & (count >= min_points)
    if any(v > 0 for v in ms):
        b = boxes.to(torch.float64)
        want = torch.tensor(ms, dtype=torch.float64, device=boxes.device)
        size = torch.maximum(b[:, 3:6], want)
        zb = b[:, 2] + (b[:, 5] - size[:, 2]) * 0.5
        wide = boxes.clone()
        wide[:, 3:6] = size.to(boxes.dtype)
        wide[:, 2] = torch.where(size[:, 2] > b[:, 5], zb.to(boxes.dtype), boxes[:, 2])
        boxes = wide
    return {"bbox3d": boxes[keep], "labels": labels[keep]}


def point_lists(owner, k):
    """owner [N] (box index per point, negative: none) -> (offsets int64 [k + 1], index int64 [M]): box b owns the points
    index[offsets[b]:offsets[b + 1]], in ascending point order (a stable sort of `owner`)."""
    k = int(k)
    if k < 0:
        raise ValueError(f"k {k} < 0")
    if not isinstance(owner, torch.Tensor) or owner.dim() != 1 or owner.dtype.is_floating_point:
        raise ValueError("owner must be an integer tensor [N]")
    own = owner.to(torch.int64)
    if own.numel() and int(own.max()) >= k:
        raise ValueError(f"owner holds box index {int(own.max())}, k = {k}")
    srt, order = torch.sort(own, stable=True)
    index = order[srt >= 0]
    counts = torch.bincount(srt[srt >= 0], minlength=k)
    offsets = torch.zeros(k + 1, dtype=torch.int64, device=owner.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return offsets, index


def crop_boxes(boxes, count, lo, hi, min_points=None, min_length=MIN_LENGTH):
    """The arithmetic of Bbox3D.crop_bbox_by_points and of split_bbox's steps (1) and (4) on yx_zb boxes [K, 7], from the
    count [K] and extents lo, hi [K, 3] that points_in_boxes took with the grown boxes.  The length axis is ly (d4): the
    new extent is [max(lo_y, -d4/2), min(hi_y, d4/2)], the centre moves by its midpoint m along the length direction
    (world dx = s m, dy = c m); thickness, z_bot, dz and yaw stay.  A box is dropped when count <= min(10 d4 dz, 200)
    (min_points overrides that number), when count < 10, or when the cropped length is <= min_length.
    -> (boxes' [K, 7], keep bool [K]); dropped rows of boxes' hold the input box."""
    if boxes.dim() != 2 or boxes.shape[1] != 7:
        raise ValueError("boxes must be [K, 7] (yx_zb)")
    k = boxes.shape[0]
    if tuple(count.shape) != (k,) or tuple(lo.shape) != (k, 3) or tuple(hi.shape) != (k, 3):
        raise ValueError(f"count, lo, hi must be [{k}], [{k}, 3], [{k}, 3], got {tuple(count.shape)}, {tuple(lo.shape)}, "
                         f"{tuple(hi.shape)}")
    if min_points is not None and not float(min_points) >= 0:
        raise ValueError(f"min_points {min_points} < 0")
    if not float(min_length) >= 0:
        raise ValueError(f"min_length {min_length} < 0")
    b = boxes.to(torch.float64)
    cnt = count.to(b.device)
    some = cnt > 0
    half = b[:, 4] * 0.5
    zero = torch.zeros_like(half)
    y0 = torch.maximum(torch.where(some, lo[:, 1].to(b), zero), -half)      # an empty box: no inf - inf below
    y1 = torch.minimum(torch.where(some, hi[:, 1].to(b), zero), half)
    length = torch.clamp(y1 - y0, min=0.0)
    mid = (y0 + y1) * 0.5
    if min_points is None:
        need = torch.clamp(MIN_POINTS_PER_M2 * b[:, 4] * b[:, 5], max=MIN_POINTS_CAP)
    else:
        need = torch.full_like(half, float(min_points))
    keep = (cnt.to(b) > need) & (cnt >= MIN_POINTS_ANY) & (length > float(min_length))
    out = b.clone()
    out[:, 0] = torch.where(keep, b[:, 0] + torch.sin(b[:, 6]) * mid, b[:, 0])
    out[:, 1] = torch.where(keep, b[:, 1] + torch.cos(b[:, 6]) * mid, b[:, 1])
    out[:, 4] = torch.where(keep, length, b[:, 4])
    return out.to(boxes.dtype), keep


def random_window(pcl, size_xy, generator=None):
    """(xmin, ymin, xmax, ymax) of a window of size_xy = (sx, sy) placed uniformly inside the x, y extent of the cloud
    [N, >= 2] (draws from the host `generator`); an axis along which the cloud is not larger than the window gets the
    whole extent, its upper end one float32 step above the maximum because windows are half open (crop_scene)."""
    sx, sy = (float(v) for v in size_xy)
    if not (sx > 0 and sy > 0):
        raise ValueError(f"window size {size_xy} must be positive")
    if pcl.dim() != 2 or pcl.shape[1] < 2 or pcl.shape[0] == 0:
        raise ValueError("random_window: a cloud [N >= 1, >= 2]")
    xy = pcl[:, :2].detach()
    ext = torch.stack([xy.amin(0), xy.amax(0)]).to(torch.float64).cpu()
    u = torch.rand(2, dtype=torch.float64, generator=generator)
    lo_, hi_ = [], []
    for d, size in enumerate((sx, sy)):
        a, b = float(ext[0, d]), float(ext[1, d])
        if b - a <= size:
            lo_.append(a)
            hi_.append(float(torch.nextafter(torch.tensor(b, dtype=torch.float32), torch.tensor(float("inf")))))
        else:
            start = a + float(u[d]) * (b - a - size)
            lo_.append(start)
            hi_.append(min(start + size, b))
    return (lo_[0], lo_[1], hi_[0], hi_[1])


def crop_scene(pcl, targets, window, grow=(THICKNESS_AUG, THICKNESS_AUG)):
    """One scene cut to window = (xmin, ymin, xmax, ymax), all in the cloud's frame: pcl fp32 [N, F] on the GPU keeps the
    rows with min <= coordinate < max (split_xyz), in input order; targets {"bbox3d" [K, 7] yx_zb, "labels" [K]} are
    counted against the remaining points with points_in_boxes(..., grow) and cropped or dropped by crop_boxes, so that no
    box hangs over space the window emptied.  Classes with yaw set to zero (floor, ceiling, room) take the same path.
    -> (pcl', {"bbox3d", "labels"}), the targets where they were (device and type of tensor)."""
    x0, y0, x1, y1 = (float(v) for v in window)
    if not (x0 < x1 and y0 < y1):
        raise ValueError(f"window {window!r}: (xmin, ymin, xmax, ymax) with min < max")
    need_gpu(pcl.device)
    x, y = pcl[:, 0], pcl[:, 1]
    pcl = pcl[(x >= x0) & (x < x1) & (y >= y0) & (y < y1)]
    bx, lb = targets["bbox3d"], targets["labels"]
    bx_t = bx if isinstance(bx, torch.Tensor) else torch.as_tensor(bx)
    lb_t = lb if isinstance(lb, torch.Tensor) else torch.as_tensor(lb)
    dev_boxes = bx_t.detach().to(device=pcl.device, dtype=torch.float32).reshape(-1, 7)
    out, keep = [], []
    for o in range(0, max(dev_boxes.shape[0], 1), MAX_BOXES):
        part = dev_boxes[o:o + MAX_BOXES]
        _, count, lo, hi = points_in_boxes(pcl, part, grow)
        b, k = crop_boxes(part, count, lo, hi)
        out.append(b)
        keep.append(k)
    out, keep = torch.cat(out), torch.cat(keep)
    return pcl, {"bbox3d": out[keep].to(device=bx_t.device, dtype=bx_t.dtype),
                 "labels": lb_t[keep.to(lb_t.device)]}


def shift_targets(pcl, targets, scale):
    """targets in the cloud's frame -> the frame voxelize puts the points in, as scene_targets(shift=True) does: the
    offset is -min(xyz * scale) / scale in fp64, added to the fp32 box origins in fp64."""
    bx = targets["bbox3d"]
    bx = bx if isinstance(bx, torch.Tensor) else torch.as_tensor(bx)
    if pcl.shape[0] == 0 or bx.shape[0] == 0:
        return {"bbox3d": bx, "labels": targets["labels"]}
    offset = (-(pcl[:, :3].detach().amin(0).to(torch.float64) * float(scale)) / float(scale)).to(bx.device)
    out = bx.clone()
    out[:, 0:3] = (bx[:, 0:3].to(torch.float64) + offset).to(bx.dtype)
    return {"bbox3d": out, "labels": targets["labels"]}


RANK_SEED_STRIDE = 1000003


class RandomCrop(object):
    """crop=(sx, sy) of the training loops: every scene is cut to a random_window of that size with crop_scene.  One host
    torch.Generator per instance places the windows."""

    def __init__(self, size_xy, seed=0, grow=(THICKNESS_AUG, THICKNESS_AUG)):
        sx, sy = (float(v) for v in size_xy)
        if not (sx > 0 and sy > 0 and math.isfinite(sx) and math.isfinite(sy)):
            raise ValueError(f"crop {size_xy!r}: two positive sizes in metres (sx, sy)")
        self.size_xy, self.seed, self.grow = (sx, sy), int(seed), tuple(_grow(grow))
        self.generator = torch.Generator()
        self.generator.manual_seed(self.seed)

    def __repr__(self):
        return f"RandomCrop({self.size_xy}, seed={self.seed}, grow={self.grow})"

    def for_rank(self, rank):
        """the same crop with seed + 1000003 rank: the ranks of a data-parallel run draw differently"""
        return RandomCrop(self.size_xy, self.seed + RANK_SEED_STRIDE * int(rank), self.grow)

    def __call__(self, pcl, targets):
        if pcl.shape[0] == 0:
            return pcl, targets
        return crop_scene(pcl, targets, random_window(pcl, self.size_xy, self.generator), self.grow)


_CROPS = {}      # (sx, sy) -> RandomCrop: a plain tuple keeps drawing from one generator across calls


def as_crop(crop):
    """The `crop=` keyword of the loops: None -> None, a RandomCrop -> itself, (sx, sy) -> the RandomCrop of that size
    (seed 0, one per size and process)."""
    if crop is None or isinstance(crop, RandomCrop):
        return crop
    try:
        key = tuple(float(v) for v in crop)
    except (TypeError, ValueError):
        raise ValueError(f"crop must be None, (sx, sy) or a RandomCrop, got {crop!r}") from None
    if len(key) != 2:
        raise ValueError(f"crop must be None, (sx, sy) or a RandomCrop, got {crop!r}")
    if key not in _CROPS:
        _CROPS[key] = RandomCrop(key)
    return _CROPS[key]


def parse_crop(spec, seed=0):
    """--crop SX,SY -> RandomCrop; None or '' -> None"""
    if not spec:
        return None
    parts = spec.split(",")
    if len(parts) != 2:
        raise ValueError(f"--crop takes SX,SY in metres, got {spec!r}")
    return RandomCrop((float(parts[0]), float(parts[1])), seed=seed)
