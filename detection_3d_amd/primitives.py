"""The points of each box: which points of a cloud lie in which rotated box, how many, and how far along each box they
reach -- the step after detection (the supporting points of every wall, window, door, floor and ceiling) and the step
before training on cropped scenes (the reference prepares every split scene with it: Bbox3D.points_in_bbox,
utils3d/bbox3d_ops.py:731-755; split_bbox, data3d/indoor_data_util.py:214-316; Bbox3D.crop_bbox_by_points,
bbox3d_ops.py:850-926).

`points_in_boxes` is one call on the GPU (libd3d_hip, points_in_boxes.hip) that builds no [N, K] mask; `point_lists`,
`crop_boxes` and `random_window` are plain torch on small tensors and run on CPU tensors too; `crop_scene` composes them.

Boxes are yx_zb (xc, yc, z_bot, d3, d4, dz, yaw) with the BEV geometry of the IoU kernels: in the box frame
lx = c (X - xc) - s (Y - yc) runs along the thickness d3, ly = s (X - xc) + c (Y - yc) along the length d4 (c, s = cos, sin
of yaw: a wall along the world's x axis has yaw +-pi/2), lz = Z - z_bot upwards.  Detections live in the cloud's
min-shifted frame (voxelize, scene_targets): pass origin='min' with a raw cloud."""
import math

import torch

from ._lib import D3DError, check, lib, ptr, stream_of

MAX_BOXES = 4096
THICKNESS_AUG = 0.3            # split_bbox's thickness_aug: the clip of the box sizes its counts are taken with
MIN_POINTS_PER_M2 = 10.0       # split_bbox: min_point_num_per1sm
MIN_POINTS_CAP = 200.0
MIN_POINTS_ANY = 10            # crop_bbox_by_points: fewer grown-box points than this, no box
MIN_LENGTH = 0.2               # split_bbox step (4): min_wall_size_x


def _grow(grow):
    try:
        g = [float(v) for v in grow]
    except TypeError:
        raise ValueError(f"grow must be (grow_yx, grow_z), got {grow!r}") from None
    if len(g) != 2 or not all(0.0 <= v < float("inf") for v in g):
        raise ValueError(f"grow must be two finite values >= 0 (grow_yx, grow_z), got {grow!r}")
    return g


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
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 2 or xyz.shape[1] < 3:
        raise ValueError("xyz must be a tensor [N, >= 3]")
    if not isinstance(boxes, torch.Tensor) or boxes.dim() != 2 or boxes.shape[1] != 7:
        raise ValueError("boxes must be a tensor [K, 7] (yx_zb)")
    for t in (xyz, boxes):
        if not t.is_cuda:
            raise D3DError("this op runs on the MI355X only: tensor is on %s (no CPU fallback)" % t.device)
    if xyz.dtype != torch.float32 or boxes.dtype != torch.float32:
        raise ValueError(f"xyz and boxes must be float32, got {xyz.dtype} and {boxes.dtype}")
    if boxes.device != xyz.device:
        raise ValueError(f"xyz is on {xyz.device}, boxes on {boxes.device}")
    n, k = xyz.shape[0], boxes.shape[0]
    if k > MAX_BOXES:
        raise ValueError(f"{k} boxes: at most {MAX_BOXES} in one call")
    xyz, boxes = xyz.detach(), boxes.detach().contiguous()
    o = _origin(origin, xyz)
    if n > 1 and (xyz.stride(1) != 1 or xyz.stride(0) < 3):
        xyz = xyz[:, :3].contiguous()        # a transposed or broadcast view: the three columns only
    stride = xyz.stride(0) if n > 1 else max(3, xyz.stride(0))
    dev = xyz.device
    owner = torch.empty((n,), dtype=torch.int32, device=dev)
    count = torch.empty((k,), dtype=torch.int32, device=dev)
    lo = torch.empty((k, 3), dtype=torch.float32, device=dev)
    hi = torch.empty((k, 3), dtype=torch.float32, device=dev)
    check(lib().d3d_points_in_boxes(ptr(xyz), n, stride, ptr(o), ptr(boxes), k, g[0], g[1], ptr(owner), ptr(count),
                                    ptr(lo), ptr(hi), stream_of(dev)))
    return owner, count, lo, hi


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
    if not pcl.is_cuda:
        raise D3DError("this op runs on the MI355X only: tensor is on %s (no CPU fallback)" % pcl.device)
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
