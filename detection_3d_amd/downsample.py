"""From a raw scan to the detector's input cloud: one point per voxel and a cap on the number of points.  The reference
does both in its data preparation (data3d/suncg_utils/suncg_preprocess.py:748-767, open3d.voxel_down_sample(pcd,
voxel_size=0.02); data3d/indoor_data_util.py:59-71,423, random_sample_pcl(p, 500 000, only_reduce=True)); here they are
calls on the GPU (libd3d_hip, downsample.hip).

Semantics (include/d3d_hip.h; a restatement of open3d's VoxelDownSample that is not pinned against open3d
itself): rows with a non-finite position are dropped; the cell of a point is floor((double(p) - lo) / voxel) per axis
with lo = double(per-axis minimum of the kept rows) - 0.5 voxel; every output column is the voxel's mean (fp64 sum, one
division, one rounding to fp32), the normal columns scaled to unit length afterwards; the voxels come in the order of
their first point in the input.  The cap keeps the k rows with the smallest (key, row), the key an integer mix of
(seed, row), in ascending row order.  The same input gives the same bits, whatever torch's deterministic mode says."""
import ctypes

import torch

from ._cloud import gpu_cloud, need_gpu, normal_column, number, options, run, scratch
from ._lib import ptr, stream_of

MAX_COLS = 16
CELL_LIMIT = 1 << 21
DEFAULT_VOXEL = 0.02
DEFAULT_MAX_POINTS = 500_000


def voxel_downsample(pcl, voxel=DEFAULT_VOXEL, normal_col="auto", return_inverse=False, return_counts=False):
    """pcl fp32 [N, C] on the GPU, 3 <= C <= 16, columns 0:3 the position -> fp32 [M, C], one row per occupied voxel of
    edge `voxel`, every column the mean over the voxel's points.  normal_col: 'auto' (6 when C == 9, else none), a column
    index or None; those three columns are scaled to unit length after the mean (a zero mean stays zero, and so does a
    point that is alone in its voxel: its row is the point, bit for bit).
    return_inverse: also voxel_of_point int32 [N], the output row of every input row, -1 for a row dropped because its
    position is not finite.  return_counts: also the points per voxel, int32 [M].
    Runs on the current stream with one host read-back (M); a cloud wider than 2^21 voxels on an axis raises D3DError."""
    voxel = number(voxel, "voxel", lo_open=True)
    pcl = gpu_cloud(pcl, "pcl").contiguous()
    n, ncols = pcl.shape
    if ncols > MAX_COLS:
        raise ValueError(f"voxel_downsample: 3 to {MAX_COLS} columns, got {ncols}")
    nc = normal_column(normal_col, ncols)
    dev = pcl.device
    info = (ctypes.c_int * 2)(0, 0)
    if n > 0:
        buf, nbytes = scratch(dev, "d3d_voxel_downsample_scratch_bytes", n, ncols)
        run(dev, "d3d_voxel_downsample_cells", ptr(pcl), n, ncols, voxel, ptr(buf), nbytes, info, stream_of(dev))
    m = int(info[0])
    out = torch.empty((m, ncols), dtype=torch.float32, device=dev)
    inverse = torch.empty((n,), dtype=torch.int32, device=dev) if return_inverse else None
    counts = torch.empty((m,), dtype=torch.int32, device=dev) if return_counts else None
    if n > 0:
        run(dev, "d3d_voxel_downsample_rows", ptr(pcl), n, ncols, nc, info, ptr(buf), nbytes, ptr(out), ptr(inverse),
            ptr(counts), stream_of(dev))
    res = (out,) + ((inverse,) if return_inverse else ()) + ((counts,) if return_counts else ())
    return res[0] if len(res) == 1 else res


def sample_rows(n, k, seed, device):
    """The rows a cap of n rows to k keeps: int32 [min(k, n)] on `device`, ascending; the k rows with the smallest
    (key, row), key = the integer mix of (seed, row) of include/d3d_hip.h.  A pure function of (n, k, seed), independent
    of torch's generators.  Runs on the current stream without a host read-back."""
    n, k, seed = int(n), int(k), int(seed)
    if n < 0 or k < 0:
        raise ValueError(f"sample_rows: n {n} and k {k} must not be negative")
    if n >= 1 << 31:
        raise ValueError(f"sample_rows: n {n} does not fit 31 bits")
    device = torch.device(device)
    need_gpu(device, "the device")
    rows = torch.empty((min(k, n),), dtype=torch.int32, device=device)
    if rows.numel() == 0:
        return rows
    buf, nbytes = scratch(device, "d3d_sample_rows_scratch_bytes", n) if k < n else (None, 0)
    run(device, "d3d_sample_rows", n, k, seed & 0xFFFFFFFFFFFFFFFF, ptr(rows), ptr(buf), nbytes, stream_of(device))
    return rows


def cap_points(pcl, max_points=DEFAULT_MAX_POINTS, seed=0, return_rows=False):
    """A uniform random subset of at most max_points rows of pcl without replacement, in the cloud's own order
    (random_sample_pcl(..., only_reduce=True), which returns them shuffled).  A cloud that is small enough is returned
    as it is (the same object); return_rows: also the kept rows, int32, or None when nothing was cut."""
    k = int(max_points)
    if k < 0:
        raise ValueError(f"max_points {k} must not be negative")
    if not isinstance(pcl, torch.Tensor) or pcl.dim() < 1:
        raise ValueError("cap_points: a tensor [N, ...]")
    if k >= pcl.shape[0]:
        return (pcl, None) if return_rows else pcl
    rows = sample_rows(pcl.shape[0], k, seed, pcl.device)
    out = pcl.index_select(0, rows)
    return (out, rows) if return_rows else out


def downsample_kwargs(downsample):
    """The `downsample=` keyword of the loops: None -> None; a voxel size -> {'voxel': v}; a dict with keys among voxel,
    max_points, seed -> a checked copy (voxel None or absent: no voxel step; max_points None or absent: no cap)."""
    if isinstance(downsample, (int, float)) and not isinstance(downsample, bool):
        downsample = {"voxel": downsample}
    kw = options(downsample, "downsample", ("voxel", "max_points", "seed"), "None, a voxel size")
    if kw is None:
        return None
    if kw.get("voxel") is not None:
        kw["voxel"] = number(kw["voxel"], "voxel", lo_open=True)
    if kw.get("max_points") is not None:
        kw["max_points"] = int(kw["max_points"])
        if kw["max_points"] < 1:
            raise ValueError(f"downsample: max_points {kw['max_points']} < 1")
    kw["seed"] = int(kw.get("seed", 0))
    return kw


def parse_downsample(spec):
    """--downsample V[,MAX_POINTS]: None or '' -> None, 'V' -> {'voxel': V}, 'V,K' -> {'voxel': V, 'max_points': K}."""
    if spec is None or not spec.strip():
        return None
    parts = spec.strip().split(",")
    if len(parts) > 2:
        raise ValueError(f"--downsample takes V[,MAX_POINTS], got {spec!r}")
    kw = {"voxel": float(parts[0])}
    if len(parts) == 2:
        kw["max_points"] = int(parts[1])
    return downsample_kwargs(kw)


def apply_downsample(pcl, dkw, return_source=False):
    """The down-sampling steps of a checked `downsample=` (downsample_kwargs) on one raw cloud, on the current stream:
    voxel_downsample, then cap_points.  return_source: also source int32 [N], the row of the result every input row went
    to, -1 for a row that was dropped or capped away (None when dkw is None)."""
    if dkw is None:
        return (pcl, None) if return_source else pcl
    n, source = pcl.shape[0], None
    if dkw.get("voxel") is not None:
        if return_source:
            pcl, source = voxel_downsample(pcl, dkw["voxel"], return_inverse=True)
        else:
            pcl = voxel_downsample(pcl, dkw["voxel"])
    if dkw.get("max_points") is not None:
        m = pcl.shape[0]
        pcl, rows = cap_points(pcl, dkw["max_points"], dkw["seed"], return_rows=True)
        if return_source and rows is not None:
            new_row = torch.full((m + 1,), -1, dtype=torch.int32, device=pcl.device)     # entry m: rows already dropped
            new_row[rows.long()] = torch.arange(rows.shape[0], dtype=torch.int32, device=pcl.device)
            source = new_row[:m] if source is None else new_row[source.long()]
    if return_source and source is None:
        source = torch.arange(n, dtype=torch.int32, device=pcl.device)
    return (pcl, source) if return_source else pcl


def prepare_cloud(pcl, voxel=DEFAULT_VOXEL, max_points=DEFAULT_MAX_POINTS, seed=0, normals=None):
    """A raw scan -> the cloud the detector takes, the three steps of the reference's preparation in its order: one point
    per `voxel` (None: skip), at most max_points of them (None: skip), then, with normals ('estimate' or a dict of
    estimate_normals keywords), normal columns estimated on the down-sampled cloud (normals.with_normals)."""
    from .prepare import Preparation
    dkw = {"voxel": voxel, "max_points": max_points, "seed": seed}
    return Preparation(downsample=dkw, normals=normals).cloud(pcl)[0]
