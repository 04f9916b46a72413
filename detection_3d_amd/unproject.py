"""From posed depth frames to the detector's input cloud.  The reference renders depth images and back-projects every
frame on the CPU in numpy fp64 (data3d/suncg_utils/suncg_preprocess.py:790-832, depth_2_pcl), then concatenates the
frames and voxel-down-samples them (gen_pcl, :718-764); here a batch of frames is one call on the GPU (libd3d_hip,
unproject.hip), which also gives every point a normal from its neighbouring pixels, facing the camera that saw it: no
neighbour search, and correct for a cloud merged from many viewpoints, where estimate_normals(orient=...) has one.

Semantics (include/d3d_hip.h): a restatement of depth_2_pcl that is not pinned against a run of the
reference (its module imports open3d).  Two deliberate differences: the kept pixels come in row-major order (f, v, u),
where the reference flattens every image column by column, and a pixel needs min_depth <= z <= max_depth and a finite z
besides the reference's z > 0.  The same input gives the same bits.

Out of scope: reading PNG, JPG or .sens files (bring tensors); lens distortion (undistort first); chunking scans whose
F H W rows do not fit in memory (`step` is the knob: it keeps one pixel in step x step).  fuse_frames merges frames by
the voxel mean alone; tsdf.fuse_frames_tsdf fuses the same frames into a signed-distance volume and returns its surface."""
import ctypes
import math

import numpy as np
import torch

from ._cloud import need_gpu, number, options, run, scratch, whole
from ._lib import DepthFramesDesc, ptr, stream_of
from .downsample import DEFAULT_MAX_POINTS, DEFAULT_VOXEL, apply_downsample, downsample_kwargs

PIXEL_LIMIT = 1 << 31
COLUMNS = (3, 6, 9)
UNPROJECT_KEYS = ("columns", "step", "min_depth", "max_depth", "edge", "color_div")


class DepthFrames(object):
    """F posed frames of one scan.
    depth: uint16 (z = d * depth_scale, 0.001: millimetres) or float32 (z = d) [F, H, W] on the GPU; 0, a negative, NaN
    or inf marks a pixel without a measurement.
    color: uint8 or float32 [F, H, W, 3], or None.
    intrinsics: [F, 4] or [4] (one camera for all frames) as (fx, fy, cx, cy) in pixels.
    extrinsics: [F, 3, 4] or [F, 4, 4], camera to world, the camera looking along +z with x to the right and y down.
    Intrinsics and extrinsics may be anything torch.as_tensor takes; they are kept on the device as fp64.  Image tensors
    that are not contiguous are copied."""

    def __init__(self, depth, intrinsics, extrinsics, color=None, depth_scale=0.001):
        if not isinstance(depth, torch.Tensor) or depth.dim() != 3:
            raise ValueError("DepthFrames: depth is a tensor [F, H, W]")
        if depth.dtype not in (torch.uint16, torch.float32):
            raise ValueError(f"DepthFrames: depth is uint16 or float32, got {depth.dtype}")
        f, h, w = depth.shape
        if f > 0 and (h < 1 or w < 1):
            raise ValueError(f"DepthFrames: frames of {h} x {w} pixels")
        if color is not None:
            if not isinstance(color, torch.Tensor) or tuple(color.shape) != (f, h, w, 3):
                raise ValueError(f"DepthFrames: color is a tensor [{f}, {h}, {w}, 3] like the depth, got "
                                 f"{tuple(getattr(color, 'shape', ()))}")
            if color.dtype not in (torch.uint8, torch.float32):
                raise ValueError(f"DepthFrames: color is uint8 or float32, got {color.dtype}")
        intrinsics = torch.as_tensor(intrinsics).to(torch.float64)
        if tuple(intrinsics.shape) == (4,):
            intrinsics = intrinsics.expand(f, 4)
        if tuple(intrinsics.shape) != (f, 4):
            raise ValueError(f"DepthFrames: intrinsics are [{f}, 4] or [4] (fx, fy, cx, cy), got {tuple(intrinsics.shape)}")
        extrinsics = torch.as_tensor(extrinsics).to(torch.float64)
        if tuple(extrinsics.shape) not in ((f, 3, 4), (f, 4, 4)):
            raise ValueError(f"DepthFrames: extrinsics are [{f}, 3, 4] or [{f}, 4, 4], got {tuple(extrinsics.shape)}")
        depth_scale = float(depth_scale)
        if not (depth_scale > 0.0 and math.isfinite(depth_scale)):
            raise ValueError(f"DepthFrames: depth_scale {depth_scale} must be positive and finite")
        if f * h * w >= PIXEL_LIMIT:
            raise ValueError(f"DepthFrames: {f} x {h} x {w} pixels do not fit 31 bits; pass fewer frames per call")
        for t in (depth, color):
            if t is not None:
                need_gpu(t.device)
        if color is not None and color.device != depth.device:
            raise ValueError(f"DepthFrames: depth on {depth.device}, color on {color.device}")
        self.depth = _contiguous(depth.detach())
        self.color = None if color is None else _contiguous(color.detach())
        self.intrinsics = intrinsics.to(depth.device).contiguous()
        self.extrinsics = extrinsics[:, :3, :].to(depth.device).contiguous()
        self.depth_scale = depth_scale
        self.desc = DepthFramesDesc(ptr(self.depth), int(depth.dtype == torch.uint16), ptr(self.color),      # the tensors stay
                                    int(color is not None and color.dtype == torch.uint8), ptr(self.intrinsics),
                                    ptr(self.extrinsics), f, h, w, depth_scale)

    @property
    def shape(self):
        return tuple(self.depth.shape)

    @property
    def device(self):
        return self.depth.device


def _contiguous(t):
    if t.is_contiguous():
        return t
    if t.dtype == torch.uint16:              # copied as int16: the same bits, and a dtype every copy kernel takes
        return t.view(torch.int16).contiguous().view(torch.uint16)
    return t.contiguous()


def unproject_kwargs(unproject):
    """The `unproject=` keyword of BuildingPipeline: None -> {}, or a dict of unproject keywords (columns, step,
    min_depth, max_depth, edge, color_div) -> a checked copy."""
    kw = options(unproject, "unproject", UNPROJECT_KEYS) or {}
    _check_args(**kw)
    return kw


def _check_args(columns=9, step=1, min_depth=0.0, max_depth=math.inf, edge=0.05, color_div=256.0):
    if columns not in COLUMNS:
        raise ValueError(f"unproject: columns is 3 (position), 6 (+ colour) or 9 (+ normal), got {columns!r}")
    step = whole(step, "unproject: step")
    min_depth, max_depth, edge = float(min_depth), float(max_depth), float(edge)
    if math.isnan(min_depth) or math.isnan(max_depth):
        raise ValueError("unproject: min_depth / max_depth is NaN")
    if not edge >= 0.0:                        # inf is allowed, so this is not _cloud.number's check
        raise ValueError(f"unproject: edge {edge} must not be negative")
    color_div = number(color_div, "unproject: color_div", lo_open=True)
    return int(columns), step, min_depth, max_depth, edge, color_div


def unproject(frames, columns=9, step=1, min_depth=0.0, max_depth=math.inf, edge=0.05, color_div=256.0,
              return_pixels=False):
    """frames: DepthFrames -> fp32 [N, columns], one row per kept pixel in ascending (f H + v) W + u: the world position;
    with columns >= 6 the colour (uint8 / color_div, fp32 as it is, zeros without a colour image); with columns == 9 the
    unit normal from the pixel's four neighbours, facing the frame's camera, or (0, 0, 0) where it has none.
    A pixel is kept when its depth z is finite, z > 0, min_depth <= z <= max_depth, and u and v are multiples of `step`.
    edge: a neighbour takes part in the normal when |z_q - z_p| <= edge z_p (a depth discontinuity is no surface).
    return_pixels: also pixel_of_point int32 [N], the index (f H + v) W + u of every row (pixel_labels).
    Runs on the current stream with one host read-back (N); no frame or no kept pixel gives [0, columns] without a
    launch of the row kernel."""
    columns, step, min_depth, max_depth, edge, color_div = _check_args(columns, step, min_depth, max_depth, edge,
                                                                        color_div)
    if not isinstance(frames, DepthFrames):
        raise ValueError(f"unproject: frames is a DepthFrames, got {type(frames).__name__}")
    f, h, w = frames.shape
    dev = frames.device
    info = (ctypes.c_int * 1)(0)
    if f * h * w > 0:
        buf, nbytes = scratch(dev, "d3d_unproject_scratch_bytes", f, h, w, step)
        run(dev, "d3d_unproject_count", frames.desc, step, min_depth, max_depth, ptr(buf), nbytes, info, stream_of(dev))
    n = int(info[0])
    out = torch.empty((n, columns), dtype=torch.float32, device=dev)
    pixels = torch.empty((n,), dtype=torch.int32, device=dev) if return_pixels else None
    if n > 0:
        run(dev, "d3d_unproject_rows", frames.desc, step, min_depth, max_depth, color_div, edge, columns, info, ptr(buf),
            nbytes, ptr(out), ptr(pixels), stream_of(dev))
    return (out, pixels) if return_pixels else out


def suncg_cameras(cam_pos, height, width):
    """The reference's camera files -> (intrinsics [F, 4], extrinsics [F, 3, 4]) as numpy fp64, for DepthFrames.
    cam_pos: rows of 12 numbers (camPos2Extrinsics and camFocus, suncg_preprocess.py:46-88): the centre v, the forward
    direction t, the up direction u, the half fields of view xf and yf, and a score.  fx = fy = 0.5 W / tan(xf) (:85);
    cx = (W - 1) / 2, cy = (H - 1) / 2 (the pixel centres of depth_2_pcl, :801-802); R = [t x u, -u, t] as columns and
    the translation v (:66-67).  Raises ValueError where the reference asserts: the focal lengths from xf and yf differ
    by 1e-3 px or more (:87), or R R^T is off the identity by 1e-2 or more in the sum of magnitudes (:72-73)."""
    cam = np.asarray(cam_pos, dtype=np.float64).reshape(-1, 12)
    height, width = int(height), int(width)
    n = cam.shape[0]
    intr, extr = np.zeros((n, 4)), np.zeros((n, 3, 4))
    for i in range(n):
        v, t, u, xf, yf = cam[i, 0:3], cam[i, 3:6], cam[i, 6:9], cam[i, 9], cam[i, 10]
        fx, fy = 0.5 * width / np.tan(xf), 0.5 * height / np.tan(yf)
        if not abs(fx - fy) < 1e-3:
            raise ValueError(f"suncg_cameras: camera {i}: the focal length is {fx:.6f} px from xf and {fy:.6f} px from yf")
        R = np.stack([np.cross(t, u), -u, t], 1)
        I = R @ R.T
        if not (np.abs(np.diag(I) - 1).sum() < 1e-2 and np.abs(I - np.eye(3)).sum() < 1e-2):
            raise ValueError(f"suncg_cameras: camera {i}: forward {t} and up {u} are not orthonormal")
        intr[i] = (fx, fx, 0.5 * (width - 1), 0.5 * (height - 1))
        extr[i, :, :3], extr[i, :, 3] = R, v
    return intr, extr


def fuse_frames(frames, voxel=DEFAULT_VOXEL, max_points=DEFAULT_MAX_POINTS, seed=0, **unproject_kw):
    """The reference's gen_pcl order on the GPU: unproject(frames, **unproject_kw), then downsample.apply_downsample
    (one point per `voxel`, at most max_points of them; None skips a step).  With columns=9 (the default) the voxel mean
    scales the mean normal back to unit length and ignores the pixels without one: the result is the detector's
    nine-column input, and no neighbour search has run."""
    if unproject_kw.pop("return_pixels", False):
        raise ValueError("fuse_frames: the voxel mean has no pixel of its own (use unproject, then voxel_downsample "
                         "with return_inverse)")
    dkw = downsample_kwargs({"voxel": voxel, "max_points": max_points, "seed": seed})
    return apply_downsample(unproject(frames, **unproject_kw), dkw)


def pixel_labels(values, pixel_of_point, frames, fill=-1):
    """Per-point integers back into the images: values [N] and pixel_of_point [N] (unproject(return_pixels=True), or a
    pipeline result's "point_pixel") -> [F, H, W] of values' dtype, `fill` at the pixels that gave no point.  frames: the
    DepthFrames or its shape (F, H, W).  Plain torch."""
    f, h, w = frames.shape if isinstance(frames, DepthFrames) else tuple(int(s) for s in frames)
    if values.dim() != 1 or pixel_of_point.shape != values.shape:
        raise ValueError(f"pixel_labels: values {tuple(values.shape)} and pixel_of_point {tuple(pixel_of_point.shape)} "
                         "are [N] both")
    if values.dtype.is_floating_point or values.dtype == torch.bool:
        raise ValueError(f"pixel_labels: values are integers, got {values.dtype}")
    img = torch.full((f * h * w,), fill, dtype=values.dtype, device=values.device)
    img[pixel_of_point.long()] = values
    return img.view(f, h, w)
