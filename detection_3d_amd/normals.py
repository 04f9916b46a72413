"""Point normals for clouds that come without them: a lidar, photogrammetry or ScanNet scan carries xyz, or xyz and
colour, while the detector's configs take xyz, colour and normal.  The reference fills the gap in its data preparation
(data3d/indoor_data_util.py:73-76, add_norm: open3d's estimate_normals with a hybrid search of radius 0.1 m and at most
50 neighbours; :395-396 appends the result as columns 6:9); here it is one call on the GPU (libd3d_hip, normals.hip).

Semantics, a restatement of the hybrid search that is not pinned against open3d itself: the neighbours of
a point are all points within `radius` (itself included, distances in fp32), cut to the `max_nn` nearest by (squared
distance, index); fewer than 3 neighbours, or coincident ones, give (0, 0, 1); otherwise the unit eigenvector of the
smallest eigenvalue of the neighbours' covariance.  open3d leaves the sign arbitrary: here the component of largest
magnitude is made positive (ties: the lowest axis), or, with orient=(vx, vy, vz), the normal faces that viewpoint.  The
same input gives the same bits, whatever torch's deterministic mode says."""
import ctypes

import torch

from ._lib import D3DError, check, floats, lib, ptr, stream_of

ESTIMATE = "estimate"


def _check_args(radius, max_nn, orient):
    radius, max_nn = float(radius), int(max_nn)
    if not (radius > 0.0 and radius < float("inf")):
        raise ValueError(f"radius {radius} must be positive and finite")
    if max_nn < 3:
        raise ValueError(f"max_nn {max_nn} < 3: a normal needs three neighbours")
    vp = None
    if orient is not None:
        vp = [float(v) for v in orient]
        if len(vp) != 3:
            raise ValueError(f"orient must be None or a viewpoint (vx, vy, vz), got {orient!r}")
    return radius, max_nn, vp


def estimate_normals(xyz, radius=0.1, max_nn=50, orient=None, return_counts=False):
    """xyz fp32 [N, >= 3] on the GPU, the first three columns being the position; it may be the column slice of a wider
    cloud (`pcl[:, :3]`), which is read in place through its row stride.  -> normals fp32 [N, 3], and with return_counts
    the number of neighbours kept per point, int32 [N] (below 3: the normal is (0, 0, 1)).  Runs on the current stream,
    without a host read-back."""
    radius, max_nn, vp = _check_args(radius, max_nn, orient)
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 2 or xyz.shape[1] < 3:
        raise ValueError("xyz must be a tensor [N, >= 3]")
    if not xyz.is_cuda:
        raise D3DError("this op runs on the MI355X only: tensor is on %s (no CPU fallback)" % xyz.device)
    if xyz.dtype != torch.float32:
        raise ValueError(f"xyz must be float32, got {xyz.dtype}")
    xyz = xyz.detach()
    n = xyz.shape[0]
    if n > 1 and (xyz.stride(1) != 1 or xyz.stride(0) < 3):
        xyz = xyz[:, :3].contiguous()        # a transposed or broadcast view: the three columns only
    stride = xyz.stride(0) if n > 1 else max(3, xyz.stride(0))
    dev = xyz.device
    normals = torch.empty((n, 3), dtype=torch.float32, device=dev)
    counts = torch.empty((n,), dtype=torch.int32, device=dev) if return_counts else None
    if n > 0:
        nbytes = lib().d3d_estimate_normals_scratch_bytes(n, max_nn)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        check(lib().d3d_estimate_normals(ptr(xyz), n, stride, radius, max_nn, floats(vp) if vp else None, ptr(normals),
                                         ptr(counts), ptr(scratch), nbytes, stream_of(dev)))
    return (normals, counts) if return_counts else normals


def estimate_normals_phases(xyz, radius=0.1, max_nn=50):
    """estimate_normals on a contiguous fp32 [N, 3] GPU tensor, timed with events inside the library: -> (normals, dict of
    milliseconds for the cells, sort, table and search phases).  Synchronises; for measurements."""
    radius, max_nn, _ = _check_args(radius, max_nn, None)
    if not xyz.is_cuda:
        raise D3DError("this op runs on the MI355X only: tensor is on %s (no CPU fallback)" % xyz.device)
    n, dev = xyz.shape[0], xyz.device
    normals = torch.empty((n, 3), dtype=torch.float32, device=dev)
    nbytes = lib().d3d_estimate_normals_scratch_bytes(n, max_nn)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ms = (ctypes.c_float * 4)()
    check(lib().d3d_estimate_normals_phases(ptr(xyz), n, xyz.stride(0), radius, max_nn, None, ptr(normals), None,
                                            ptr(scratch), nbytes, stream_of(dev), ms))
    return normals, dict(zip(("cells", "sort", "table", "search"), (float(v) for v in ms)))


def with_normals(pcl, radius=0.1, max_nn=50, orient=None, estimator=estimate_normals):
    """The nine-column cloud (xyz, colour, normal) of a cloud that lacks normals: [N, 3] -> [N, 9] with zero colour,
    [N, 6] -> [N, 9], [N, 9] -> a copy with columns 6:9 replaced; the normals are estimated from columns 0:3.  Any other
    width raises ValueError."""
    if pcl.dim() != 2 or pcl.shape[1] not in (3, 6, 9):
        raise ValueError(f"with_normals: a cloud of 3, 6 or 9 columns, got shape {tuple(pcl.shape)}")
    n, w = pcl.shape
    nrm = estimator(pcl[:, :3], radius=radius, max_nn=max_nn, orient=orient)
    out = torch.empty((n, 9), dtype=pcl.dtype, device=pcl.device)
    out[:, :min(w, 6)] = pcl[:, :min(w, 6)]
    if w == 3:
        out[:, 3:6] = 0
    out[:, 6:9] = nrm
    return out


def normals_kwargs(normals):
    """The `normals=` keyword of the loops: None -> None, 'estimate' -> {}, a dict of estimate_normals keywords ->
    a checked copy."""
    if normals is None:
        return None
    if isinstance(normals, str):
        if normals != ESTIMATE:
            raise ValueError(f"normals must be None, 'estimate' or a dict of estimate_normals keywords, got {normals!r}")
        return {}
    if isinstance(normals, dict):
        bad = sorted(set(normals) - {"radius", "max_nn", "orient"})
        if bad:
            raise ValueError(f"normals: unknown keywords {bad} (radius, max_nn, orient)")
        kw = dict(normals)
        _check_args(kw.get("radius", 0.1), kw.get("max_nn", 50), kw.get("orient"))
        return kw
    raise ValueError(f"normals must be None, 'estimate' or a dict of estimate_normals keywords, got {normals!r}")


def parse_estimate_normals(spec):
    """--estimate-normals[=radius,max_nn]: None (flag absent) -> None, '' (bare flag) -> 'estimate',
    'R' -> {'radius': R}, 'R,K' -> {'radius': R, 'max_nn': K}."""
    if spec is None:
        return None
    spec = spec.strip()
    if not spec:
        return ESTIMATE
    parts = spec.split(",")
    if len(parts) > 2:
        raise ValueError(f"--estimate-normals takes radius[,max_nn], got {spec!r}")
    kw = {"radius": float(parts[0])}
    if len(parts) == 2:
        kw["max_nn"] = int(parts[1])
    return normals_kwargs(kw)
