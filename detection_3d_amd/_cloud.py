"""What every raw-scan wrapper (clean, planes, normals, downsample, register, frame, primitives, unproject, tsdf, render) does
before and around its library call, in one place.  Three rules live here and nowhere else:

rows in place: a cloud is fp32 [N, >= 3] rows read through their row stride (`row_stride_floats` of the C entry points),
so that a column slice of a wider cloud costs no copy; only a transposed or broadcast view is copied;

the check order: type and shape, then float32, then the device, so that an argument fault is a ValueError whatever
device the tensor is on, and D3DError says one thing only: the tensor is fine and not on the GPU;

the call: ask `*_scratch_bytes` for a size, allocate that many bytes on the tensor's device, make the tensor's device
the current one around the launch, and turn the library's return code into an exception.

Imports _lib and torch alone: every raw-scan module imports it at the top."""
import ctypes
import math

import torch

from ._lib import D3DError, check, lib


def in_place(t):
    """t [N, >= 3] -> (the tensor to read, N, its row stride in floats).  Needs no GPU.  A single row has no stride of its
    own, the library still wants one that holds three floats."""
    n = t.shape[0]
    if n > 1 and (t.stride(1) != 1 or t.stride(0) < 3):
        t = t[:, :3].contiguous()        # a transposed or broadcast view: the three columns only
    return t, n, (t.stride(0) if n > 1 else max(3, t.stride(0)))


def need_gpu(device, what="tensor"):
    if device.type != "cuda":
        raise D3DError(f"this op runs on the MI355X only: {what} is on {device} (no CPU fallback)")


def fp32_cloud(t, what="xyz", cols=3, exact=False):
    """`what` is a tensor [N, >= cols] (exact: [N, cols]) and float32 -> it, detached.  On its own where an op has
    further arguments to fault (ValueError) before the first word about a device."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or (t.shape[1] != cols if exact else t.shape[1] < cols):
        raise ValueError(f"{what} must be a tensor [N, {'' if exact else '>= '}{cols}]")
    if t.dtype != torch.float32:
        raise ValueError(f"{what} must be float32, got {t.dtype}")
    return t.detach()


def gpu_cloud(t, what="xyz", cols=3, exact=False):
    """fp32_cloud's check, then the device; for an argument the library reads without a stride (the caller makes it
    contiguous)"""
    t = fp32_cloud(t, what, cols, exact)
    need_gpu(t.device)
    return t


def gpu_rows(t, what="xyz", cols=3, exact=False):
    """gpu_cloud's check, then in_place -> (the tensor to read, N, row stride in floats)"""
    return in_place(gpu_cloud(t, what, cols, exact))


def same_device(**tensors):
    """named tensors (None: not given) -> the device of the first; another one elsewhere raises ValueError"""
    (first, t0), *rest = tensors.items()
    for name, t in rest:
        if t is not None and t.device != t0.device:
            raise ValueError(f"{first} is on {t0.device}, {name} on {t.device}")
    return t0.device


def number(value, what, lo=0.0, hi=math.inf, lo_open=False):
    """-> float(value), finite and in [lo, hi] ((lo, hi] with lo_open; hi = inf: no upper bound); else ValueError"""
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{what} {value!r} must be a number") from None
    if not ((v > lo if lo_open else v >= lo) and v <= hi and math.isfinite(v)):
        if hi == math.inf:
            raise ValueError(f"{what} {v} must be finite and {'>' if lo_open else '>='} {lo:g}")
        raise ValueError(f"{what} {v} outside {'(' if lo_open else '['}{lo:g}, {hi:g}]")
    return v


def whole(value, what, lo=1, hi=None):
    """-> int(value) for an int, or a float with an integer value, in [lo, hi] (hi None: no upper bound); a bool, a
    fraction or anything else raises ValueError"""
    try:
        ok = not isinstance(value, bool) and int(value) == value and lo <= int(value) and (hi is None or int(value) <= hi)
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"{what} {value!r} must be an integer " + (f">= {lo}" if hi is None else f"in [{lo}, {hi}]"))
    return int(value)


def options(value, what, keys, forms="None"):
    """The dict form of a loop keyword such as clean= or downsample=: None -> None, a dict whose keys are among `keys` ->
    a copy; anything else raises ValueError.  forms: the forms the caller takes besides a dict, for the message."""
    if value is None:
        return None
    if not isinstance(value, dict):
        raise ValueError(f"{what} must be {forms} or a dict with keys among {', '.join(keys)}, got {value!r}")
    bad = sorted(set(value) - set(keys))
    if bad:
        raise ValueError(f"{what}: unknown keywords {bad} ({', '.join(keys)})")
    return dict(value)


def normal_column(normal_col, ncols):
    """'auto' (6 of a nine-column cloud, else none), None or a column index -> the first normal column, -1 for none"""
    if isinstance(normal_col, str):
        if normal_col != "auto":
            raise ValueError(f"normal_col must be 'auto', None or a column index, got {normal_col!r}")
        return 6 if ncols == 9 else -1
    if normal_col is None:
        return -1
    nc = int(normal_col)
    if nc < 0 or nc + 3 > ncols:
        raise ValueError(f"normal_col {nc}: three columns inside the {ncols} of the cloud")
    return nc


def scratch(dev, size_fn, *args):
    """-> (uint8 tensor on dev, its size): as many bytes as the library's `size_fn`(*args) asks for.  A fresh buffer per
    call; an op of several library calls passes the one buffer to each."""
    nbytes = getattr(lib(), size_fn)(*args)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


class PhaseTimer:
    """ms: the float array the library fills with one figure per name (it then synchronises), None when off;
    read(): those figures as a dict, None when off"""

    def __init__(self, names, on):
        self.names, self.ms = names, (ctypes.c_float * len(names))() if on else None

    def read(self):
        return None if self.ms is None else dict(zip(self.names, (float(v) for v in self.ms)))


def run(dev, fn, *args):
    """the library's `fn`(*args) with dev the current device; a return code other than 0 raises D3DError"""
    with torch.cuda.device(dev):
        check(getattr(lib(), fn)(*args))
