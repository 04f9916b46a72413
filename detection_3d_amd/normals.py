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
import torch

from ._cloud import PhaseTimer, gpu_rows, number, options, run, scratch, whole
from ._lib import floats, ptr, stream_of

ESTIMATE = "estimate"
PHASES = ("cells", "sort", "table", "search")
_KEYS = ("radius", "max_nn", "orient")


def check_args(radius=0.1, max_nn=50, orient=None):
    """-> (radius, max_nn, the viewpoint as a list or None); a normal needs three neighbours, so max_nn >= 3"""
    radius, max_nn = number(radius, "radius", lo_open=True), whole(max_nn, "max_nn", 3, 2 ** 31 - 1)
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
    normals, counts, _ = _estimate(xyz, radius, max_nn, orient, return_counts, False)
    return (normals, counts) if return_counts else normals


def _estimate(xyz, radius, max_nn, orient, return_counts, phases):
    """-> (normals, counts or None, the dict of milliseconds or None); the untimed entry point of the library enqueues
    and returns, the timed one synchronises"""
    radius, max_nn, vp = check_args(radius, max_nn, orient)
    xyz, n, stride = gpu_rows(xyz)
    dev = xyz.device
    normals = torch.empty((n, 3), dtype=torch.float32, device=dev)
    counts = torch.empty((n,), dtype=torch.int32, device=dev) if return_counts else None
    timer = PhaseTimer(PHASES, phases)
    if n > 0:
        buf, nbytes = scratch(dev, "d3d_estimate_normals_scratch_bytes", n, max_nn)
        run(dev, "d3d_estimate_normals_phases" if phases else "d3d_estimate_normals", ptr(xyz), n, stride, radius,
            max_nn, floats(vp) if vp else None, ptr(normals), ptr(counts), ptr(buf), nbytes, stream_of(dev),
            *((timer.ms,) if phases else ()))
    return normals, counts, timer.read()


def estimate_normals_phases(xyz, radius=0.1, max_nn=50):
    """estimate_normals timed with events inside the library: -> (normals, dict of milliseconds for the cells, sort,
    table and search phases).  Synchronises; for measurements."""
    normals, _, ms = _estimate(xyz, radius, max_nn, None, False, True)
    return normals, ms


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
    if isinstance(normals, str) and normals == ESTIMATE:
        return {}
    kw = options(normals, "normals", _KEYS, "None, 'estimate'")
    if kw is not None:
        check_args(**kw)
    return kw


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
