"""Levelling and squaring a raw scan.  Every step around the detector takes a cloud whose z is up and whose walls run along
x and y (planes.label_planes classes a plane by its normal's angle to z, primitives.fit_boxes keeps floors upright, the
detector's seven-number boxes have no tilt, voxelize drops what leaves its lattice), while a handheld or RGB-D stream
lives in the frame of its first camera, merge_scans in the frame of its reference scan, and a tripod lidar is level
with an arbitrary heading.  The reference leaves this to whoever prepared the dataset (ScanNet ships an axis-alignment
matrix per scene); here `manhattan_frame` finds that matrix on the GPU from the normals (libd3d_hip, frame.hip).

Semantics (include/d3d_hip.h).  Every normal votes for a candidate up direction u with a truncated quadratic
of the squared sine of its angle to +-u or to the plane across u, as an integer, summed in 64 bits; three passes of a
16 x 16 lattice of tilts, each an eighth as wide as the one before, then two passes of 256 headings over a quarter turn
for the rows the final up direction calls walls.  Candidate tables come from numpy on the host; nothing is read back;
the same set of rows gives the same bits in any order."""
import ctypes
import math

import numpy as np
import torch

from ._cloud import PhaseTimer, gpu_rows, normal_column, number, options, run, scratch
from ._lib import ptr, stream_of
from .pose import apply_pose
from .primitives import FIT_Q, _fit_tables, cloud_min

FRAME_CHUNK = 1024             # frame.hip kChunk: the rows a workgroup of the sweep stages at a time
MAX_TILT = 60.0
MAX_TOL = 20.0
PHASES = ("tilt1", "tilt2", "tilt3", "heading_coarse", "heading_fine")
DEFAULTS = {"max_tilt": 30.0, "tol": 5.0, "up": None}


def _unit(w):
    return w / np.sqrt((w[..., 0:1] * w[..., 0:1] + w[..., 1:2] * w[..., 1:2]) + w[..., 2:3] * w[..., 2:3])


def _rot(v):
    """the smallest rotation that takes (0, 0, 1) to the unit vector v, fp64 [..., 3] -> [..., 3, 3] (d3d_hip.h)"""
    v0, v1, v2 = v[..., 0], v[..., 1], v[..., 2]
    if v.ndim == 1 and v2 == -1.0:
        return np.diag([1.0, -1.0, -1.0])
    a = 1.0 + v2
    x = -(v0 * v1) / a
    rows = [np.stack([1.0 - (v0 * v0) / a, x, v0], -1), np.stack([x, 1.0 - (v1 * v1) / a, v1], -1),
            np.stack([-v0, -v1, v2], -1)]
    return np.stack(rows, -2) + 0.0       # + 0: entry 136 is the identity bit for bit


def tilt_steps(max_tilt):
    """the lattice steps of the three tilt passes, degrees"""
    s1 = float(max_tilt) / 8.0
    return [s1, s1 / 8.0, s1 / 8.0 / 8.0]


def tilt_tables(max_tilt):
    """fp64 [3, 256, 3, 3]: M_k[16 i + j] takes z to the direction of ((j - 8) t, (i - 8) t, 1), t = tan(step_k)"""
    j = (np.arange(256) % 16 - 8).astype(np.float64)
    i = (np.arange(256) // 16 - 8).astype(np.float64)
    out = []
    for st in tilt_steps(max_tilt):
        t = math.tan(math.radians(st))
        out.append(_rot(_unit(np.stack([j * t, i * t, np.ones(256)], -1))))
    return np.stack(out)


def _s2(deg):
    return float(np.float32(math.sin(math.radians(deg)) ** 2))


_TABLES = {}     # (device, max_tilt) -> fp64 [3, 256, 9] on the device


def _device_tables(dev, max_tilt):
    key = (dev, max_tilt)
    t = _TABLES.get(key)
    if t is None:
        if len(_TABLES) > 64:
            _TABLES.clear()
        t = _TABLES[key] = torch.from_numpy(tilt_tables(max_tilt).reshape(3, 256, 9)).to(dev)
    return t


def _check_args(max_tilt, tol, up):
    """-> (max_tilt, tol, B_0 as a row-major fp64 numpy [9] or None)"""
    max_tilt, tol = number(max_tilt, "max_tilt", 0.0, MAX_TILT), number(tol, "tol", 0.0, MAX_TOL, lo_open=True)
    if up is None:
        return max_tilt, tol, None
    try:
        u = np.asarray(up.detach().cpu() if isinstance(up, torch.Tensor) else up, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"up must be a 3-vector, got {up!r}") from None
    if u.shape != (3,) or not np.isfinite(u).all() or not (u * u).sum() > 0.0:
        raise ValueError(f"up must be a finite 3-vector that is not zero, got {up!r}")
    return max_tilt, tol, np.ascontiguousarray(_rot(_unit(u)).reshape(9))


def align_kwargs(align):
    """The `align=` keyword of Preparation and BuildingPipeline: None -> None; True or 'manhattan' -> manhattan_frame's
    defaults; a dict with keys among max_tilt, tol, up -> a checked copy."""
    if align is None or align is False:
        return None
    if align is True or align == "manhattan":
        return dict(DEFAULTS)
    kw = dict(DEFAULTS)
    kw.update(options(align, "align", tuple(DEFAULTS), "None, True, 'manhattan'"))
    _check_args(kw["max_tilt"], kw["tol"], kw["up"])
    return kw


def parse_align(spec):
    """--align[=MAX_TILT,TOL] -> align_kwargs' dict; None -> None, '' -> the defaults"""
    if spec is None:
        return None
    if spec == "":
        return align_kwargs(True)
    parts = spec.split(",")
    if len(parts) != 2:
        raise ValueError(f"--align takes MAX_TILT,TOL in degrees, got {spec!r}")
    try:
        return align_kwargs({"max_tilt": float(parts[0]), "tol": float(parts[1])})
    except ValueError as e:
        raise ValueError(f"--align {spec!r}: {e}") from None


class Frame:
    """What manhattan_frame returns.  pose fp64 [4, 4] (aligned <- scan, zero translation), choice int32 [5] (the winning
    candidate of the three tilt and two heading passes), score int64 [5] (its score) and support int32 [2] (the rows that
    voted, the rows the final up direction calls walls) stay on the device; the properties read them back on first use.
    phases: the dict of milliseconds, when asked for."""

    def __init__(self, pose, choice, score, support, phases=None):
        self.pose, self.choice, self.score, self.support, self.phases = pose, choice, score, support, phases
        self._host = None

    def _read(self):
        if self._host is None:
            R = self.pose[:3, :3].cpu()
            ia, ib = (int(v) for v in self.choice[3:].cpu())
            t = 128 * ia + ib - 128
            if t >= 16384:
                t -= 32768
            tilt = math.degrees(math.acos(max(-1.0, min(1.0, float(R[2, 2])))))
            self._host = (tilt, math.degrees(t * FIT_Q), [int(v) for v in self.support.cpu()])
        return self._host

    @property
    def tilt_deg(self):
        """the angle between the scan's z and the level frame's"""
        return self._read()[0]

    @property
    def yaw_deg(self):
        """the heading of the walls in the levelled scan, in [-45, 45)"""
        return self._read()[1]

    @property
    def supported(self):
        """some row was called a wall: the heading means something"""
        return self._read()[2][1] > 0

    def __repr__(self):
        tilt, yaw, sup = self._read()
        return f"Frame(tilt_deg={tilt:.4g}, yaw_deg={yaw:.4g}, support={sup})"


def manhattan_frame(normals, max_tilt=30.0, tol=5.0, up=None, phases=False):
    """normals fp32 [N, 3] on the GPU, unit length with any sign; a column slice such as cloud[:, 6:9] is read in place
    -> Frame: the rotation from the scan's frame to a level, wall-aligned one.  max_tilt (degrees, at most 60; 0 turns the
    tilt search off): how far from `up` (default (0, 0, 1)) the scan's vertical may lean; tol (degrees, in (0, 20]): how far
    a normal may be from a direction it supports.  Of the four equal headings the one within 45 degrees of the scan's own
    is taken.  A building that is not Manhattan shows in Frame.score and Frame.supported; it is not handled.  Runs on the
    current stream without a read-back; bad arguments raise ValueError before any GPU work.  phases: Frame.phases is a
    dict of milliseconds per pass, timed with events inside the library; synchronises."""
    max_tilt, tol, b0 = _check_args(max_tilt, tol, up)
    nrm, n, stride = gpu_rows(normals, "normals", exact=True)
    dev = nrm.device
    steps = tilt_steps(max_tilt)
    s2 = (ctypes.c_float * 4)(*([_s2(max(tol, st)) for st in steps] + [_s2(tol)]))
    b0_c = None if b0 is None else (ctypes.c_double * 9)(*b0.tolist())
    tables = _device_tables(dev, max_tilt) if max_tilt > 0 else None
    coarse, fine = _fit_tables(dev)
    pose = torch.empty((4, 4), dtype=torch.float64, device=dev)
    choice = torch.empty((5,), dtype=torch.int32, device=dev)
    score = torch.empty((5,), dtype=torch.int64, device=dev)
    support = torch.empty((2,), dtype=torch.int32, device=dev)
    buf, nbytes = scratch(dev, "d3d_manhattan_frame_scratch_bytes")
    timer = PhaseTimer(PHASES, phases)
    run(dev, "d3d_manhattan_frame", ptr(nrm), n, stride, ptr(tables), b0_c, s2, ptr(coarse), ptr(fine), ptr(pose),
        ptr(choice), ptr(score), ptr(support), ptr(buf), nbytes, stream_of(dev), timer.ms)
    return Frame(pose, choice, score, support, timer.read())


def align_cloud(pcl, normal_col="auto", **kw):
    """pcl fp32 [N, C] on the GPU with its normals in columns normal_col .. normal_col + 2 ('auto': 6 of a nine-column
    cloud) -> (cloud, Frame): the cloud through register.apply_pose with manhattan_frame(normals, **kw).pose, positions
    and normals rotated, no read-back."""
    if not isinstance(pcl, torch.Tensor) or pcl.dim() != 2 or pcl.shape[1] < 3:
        raise ValueError("align_cloud: a tensor [N, >= 3]")
    nc = normal_column(normal_col, pcl.shape[1])
    if nc < 0:
        raise ValueError(f"align_cloud: a cloud of {pcl.shape[1]} columns carries no normals; estimate them first "
                         "(normals.with_normals, or normals='estimate' in Preparation / BuildingPipeline)")
    frame = manhattan_frame(pcl[:, nc:nc + 3], **kw)
    return apply_pose(pcl, frame.pose, normal_col), frame


def detector_pose(frame, aligned_cloud):
    """detector frame <- scan frame, fp64 [4, 4] on the device: frame.pose with the translation -cloud_min(aligned_cloud),
    the shift voxelize applies to the aligned cloud"""
    pose = frame.pose.clone()
    pose[:3, 3] = -cloud_min(aligned_cloud).to(pose.device)
    return pose


def _pose64(pose, device):
    T = pose.detach() if isinstance(pose, torch.Tensor) else torch.as_tensor(np.asarray(pose, dtype=np.float64))
    if T.shape != (4, 4):
        raise ValueError(f"pose: a 4 x 4 matrix, got shape {tuple(T.shape)}")
    return T.to(device, torch.float64)


def _boxes7(boxes):
    if not isinstance(boxes, torch.Tensor) or boxes.dim() != 2 or boxes.shape[1] != 7 or not boxes.dtype.is_floating_point:
        raise ValueError("boxes must be a floating-point tensor [K, 7] (yx_zb)")
    return boxes.detach()


def box_corners_in_scan_frame(boxes, pose):
    """boxes [K, 7] yx_zb in the detector's frame, pose 4 x 4 detector <- scan (detector_pose) -> [K, 8, 3]: the corners in
    the scan's frame, x = R^T (x' - t), corner 4 a + 2 b + c at lx = -+d3 / 2, ly = -+d4 / 2, lz = 0 or dz (points_in_boxes.hip's
    box frame).  fp64 arithmetic, one rounding to the boxes' type; plain torch, CPU tensors too."""
    b = _boxes7(boxes).to(torch.float64)
    T = _pose64(pose, b.device)
    c, s = torch.cos(b[:, 6]), torch.sin(b[:, 6])
    sign = torch.tensor([-0.5, 0.5], dtype=torch.float64, device=b.device)
    lx = (b[:, 3, None] * sign)[:, :, None, None].expand(-1, 2, 2, 2)
    ly = (b[:, 4, None] * sign)[:, None, :, None].expand(-1, 2, 2, 2)
    lz = (b[:, 5, None] * (sign + 0.5))[:, None, None, :].expand(-1, 2, 2, 2)
    c, s = c[:, None, None, None], s[:, None, None, None]
    x = b[:, 0, None, None, None] + c * lx + s * ly
    y = b[:, 1, None, None, None] - s * lx + c * ly
    z = b[:, 2, None, None, None] + lz
    p = torch.stack([x, y, z], -1).reshape(-1, 8, 3)
    return ((p - T[:3, 3]) @ T[:3, :3]).to(boxes.dtype)


def boxes_in_scan_frame(boxes, pose):
    """boxes [K, 7] yx_zb in the detector's frame -> [K, 7] in the scan's, for a pose without tilt (third row and column of
    the rotation exactly (0, 0, 1)); a tilted pose has no seven-number form and raises: take box_corners_in_scan_frame."""
    b = _boxes7(boxes).to(torch.float64)
    T = _pose64(pose, b.device)
    R = T[:3, :3]
    if R[2].tolist() != [0.0, 0.0, 1.0] or R[:, 2].tolist() != [0.0, 0.0, 1.0]:
        raise ValueError("boxes_in_scan_frame: the pose tilts the scan, and a yx_zb box cannot lean; take "
                         "box_corners_in_scan_frame for the eight corners")
    out = b.clone()
    out[:, :3] = (b[:, :3] - T[:3, 3]) @ R
    yaw = b[:, 6] + torch.atan2(R[1, 0], R[0, 0])
    out[:, 6] = yaw - torch.floor(yaw / math.pi + 0.5) * math.pi
    return out.to(boxes.dtype)
