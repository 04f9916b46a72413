"""Planar patches of a cloud that carries normals, the plane of every patch, and instance ids for an unlabelled scan: the
step between "a cloud with normals" (prepare_cloud, estimate_normals) and "an instance id per point"
(primitives.targets_from_labels).  The detector's classes are planar primitives; the reference's users get instance ids
for them by region growing over normals with open3d or CGAL on the CPU.  Here it is d3d_connected_components with a
narrower edge (planes.hip, include/d3d_hip.h).

Two points are joined when they lie within `radius`, their normals differ by at most `angle` degrees (the sign of a
normal does not matter) and each lies within `offset` of the other's tangent plane; a patch is a component of that
graph.  This is pairwise region growing, not RANSAC: a smoothly curved surface chains into one patch, and the points on
the crease between two planes carry mixed normals and fall into small patches, which `min_points` drops.  The same
input gives the same bits."""
import collections
import ctypes
import math

import torch

from ._cloud import PhaseTimer, gpu_cloud, gpu_rows, number, run, same_device, scratch, whole
from ._lib import ptr, stream_of
from .clean import PHASES
from .config import class_to_label

MAX_PLANES = 4096              # planes.hip kMaxPlanes = box_fit.hip kMaxBoxes
FIT_PHASES = ("moments", "solve")

Planes = collections.namedtuple("Planes", "plane_of_point normal d centroid count rms eigenvalues")


def _check_join(radius, angle, offset):
    """segment_planes' three thresholds: metres, degrees in [0, 90], metres"""
    return number(radius, "radius", lo_open=True), number(angle, "angle", 0.0, 90.0), number(offset, "offset")


def cos_min(angle):
    """the fp32 threshold of segment_planes' normal test: cos(angle) in double, rounded once"""
    return ctypes.c_float(math.cos(angle * math.pi / 180.0)).value


def segment_planes(xyz, normals, radius=0.1, angle=10.0, offset=0.02, phases=False):
    """xyz fp32 [N, >= 3] on the GPU (a column slice of a wider cloud is read in place), normals fp32 [N, 3] on the same
    device -> (label int32 [N], the smallest row index of the point's patch; size int32 [N], that patch's number of
    points).  P and C are joined iff, in fp32 with d = C - P: d2 <= radius^2, |nP . nC| >= cos(angle) and
    max(|nP . d|, |nC . d|) <= offset (the exact arithmetic: include/d3d_hip.h, d3d_segment_planes).  A zero or non-finite
    normal and a NaN position leave the point a patch of its own.  Current stream, no read-back.  phases: also a dict of
    milliseconds (clean.PHASES); synchronises."""
    radius, angle, offset = _check_join(radius, angle, offset)
    xyz, n, stride = gpu_rows(xyz)
    normals = gpu_cloud(normals, "normals", exact=True).contiguous()       # d3d_segment_planes takes no stride for them
    if normals.shape[0] != n:
        raise ValueError(f"normals hold {normals.shape[0]} rows, xyz {n}")
    dev = same_device(xyz=xyz, normals=normals)
    label = torch.empty((n,), dtype=torch.int32, device=dev)
    size = torch.empty((n,), dtype=torch.int32, device=dev)
    timer = PhaseTimer(PHASES, phases)
    if n > 0:
        buf, nbytes = scratch(dev, "d3d_segment_planes_scratch_bytes", n)
        run(dev, "d3d_segment_planes", ptr(xyz), n, stride, ptr(normals), radius, cos_min(angle), offset, ptr(label),
            ptr(size), ptr(buf), nbytes, stream_of(dev), timer.ms)
    return (label, size, timer.read()) if phases else (label, size)


def _plane_lists(label, size, min_points):
    """-> (plane_of_point int32 [N], order int32 [N], offsets int32 [K + 1], K): the patches of at least min_points
    points numbered in ascending order of their label, at most MAX_PLANES of them (the largest, ties to the lower label);
    the rows by (plane, row) with torch's stable sort, as primitives._fit_lists.  One size read-back, for K."""
    n, dev = label.shape[0], label.device
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    head = (label == rows) & (size >= min_points)              # the patch's first row stands for the patch
    k = int(head.sum())                                        # the read-back
    if k > MAX_PLANES:
        cand = torch.nonzero(head).squeeze(1)                  # ascending label
        order = torch.sort(size[cand].to(torch.int64), descending=True, stable=True)[1][:MAX_PLANES]
        head = torch.zeros_like(head)
        head[cand[order]] = True
        k = MAX_PLANES
    number = torch.cumsum(head, 0, dtype=torch.int32) - 1      # plane of every head row
    number = torch.where(head, number, torch.full_like(number, -1))
    pop = number[label.long()] if n else number
    srt, order = torch.sort(torch.where(pop >= 0, pop, torch.full_like(pop, k)).to(torch.int64), stable=True)
    offsets = torch.searchsorted(srt, torch.arange(k + 1, dtype=torch.int64, device=dev)).to(torch.int32)
    return pop, order.to(torch.int32), offsets, k


def fit_planes(xyz, label, size, min_points=100, phases=False):
    """The least-squares plane of every patch of segment_planes (or connected_components) with at least min_points
    points -> Planes(plane_of_point int32 [N] (-1: in no plane), normal fp64 [K, 3], d fp64 [K], centroid fp64 [K, 3],
    count int32 [K], rms fp64 [K], eigenvalues fp64 [K, 3] ascending), planes in ascending order of their label.
    normal . p = d; the normal's component of largest magnitude is positive; rms is the root of the smallest eigenvalue
    of the covariance.  fp64 moments about the patch's first row in an order fixed by the data (include/d3d_hip.h,
    d3d_fit_planes).  A patch of coincident points: normal, d and rms 0.  When more than 4096 patches reach min_points
    the 4096 largest stay (ties to the lower label).  One size read-back, for K.  phases: also a dict of milliseconds
    (FIT_PHASES); synchronises."""
    min_points = whole(min_points, "min_points")
    xyz, n, stride = gpu_rows(xyz)
    for t, what in ((label, "label"), (size, "size")):
        if not isinstance(t, torch.Tensor) or t.shape != (n,) or t.dtype != torch.int32:
            raise ValueError(f"{what} must be an int32 tensor [{n}]")
    dev = same_device(xyz=xyz, label=label, size=size)
    pop, order, offsets, k = _plane_lists(label, size, min_points)
    normal = torch.empty((k, 3), dtype=torch.float64, device=dev)
    d = torch.empty((k,), dtype=torch.float64, device=dev)
    centroid = torch.empty((k, 3), dtype=torch.float64, device=dev)
    count = torch.empty((k,), dtype=torch.int32, device=dev)
    rms = torch.empty((k,), dtype=torch.float64, device=dev)
    eig = torch.empty((k, 3), dtype=torch.float64, device=dev)
    timer = PhaseTimer(FIT_PHASES, phases)
    if k > 0:
        buf, nbytes = scratch(dev, "d3d_fit_planes_scratch_bytes", n, k)
        run(dev, "d3d_fit_planes", ptr(xyz), n, stride, ptr(pop), ptr(order), ptr(offsets), k, ptr(normal), ptr(d),
            ptr(centroid), ptr(count), ptr(rms), ptr(eig), ptr(buf), nbytes, stream_of(dev), timer.ms)
    res = Planes(pop, normal, d, centroid, count, rms, eig)
    return (res, timer.read()) if phases else res


def label_planes(pcl, normals=None, radius=0.1, angle=10.0, offset=0.02, min_points=100, tilt=10.0, classes=None):
    """Pseudo-labels for a scan nobody labelled: pcl fp32 [N, >= 3] on the GPU, normals fp32 [N, 3] or None for columns
    6:9 of a nine-column cloud -> {"instance": int64 [N] (-1: none), "instance_labels": int64 [K]}, the form
    primitives.is_labelled recognises, so that engine.collate, engine.train and targets_from_labels take it as it is.
    The instances are fit_planes' planes of segment_planes' patches.  The class of a plane, on its fitted normal n:
    |n_z| >= cos(tilt) is horizontal, floor when the centroid's z lies below the middle of the cloud's z range and
    ceiling otherwise; |n_z| <= sin(tilt) is wall; anything else gets label 0, which targets_from_labels drops.
    classes: the config's class list (default: background, wall, ceiling, floor); a class it does not hold gets 0."""
    tilt = number(tilt, "tilt", 0.0, 90.0)
    if not isinstance(pcl, torch.Tensor) or pcl.dim() != 2 or pcl.shape[1] < 3:
        raise ValueError("pcl must be a tensor [N, >= 3]")
    if normals is None:
        if pcl.shape[1] < 9:
            raise ValueError(f"normals=None reads columns 6:9, the cloud has {pcl.shape[1]} columns")
        normals = pcl[:, 6:9]
    c2l = class_to_label(("background", "wall", "ceiling", "floor") if classes is None else classes)
    label, size = segment_planes(pcl, normals, radius, angle, offset)
    planes = fit_planes(pcl, label, size, min_points)
    dev = pcl.device
    instance = planes.plane_of_point.to(torch.int64)
    if planes.normal.shape[0] == 0:
        return {"instance": instance, "instance_labels": torch.zeros((0,), dtype=torch.int64, device=dev)}
    z = pcl.detach()[:, 2].to(torch.float64)
    z = z[torch.isfinite(z)]
    middle = (z.min() + z.max()) * 0.5
    nz = planes.normal[:, 2].abs()
    flat = nz >= math.cos(tilt * math.pi / 180.0)
    upright = nz <= math.sin(tilt * math.pi / 180.0)
    low = planes.centroid[:, 2] < middle
    ids = torch.zeros_like(nz, dtype=torch.int64)
    ids = torch.where(flat & low, torch.full_like(ids, c2l.get("floor", 0)), ids)
    ids = torch.where(flat & ~low, torch.full_like(ids, c2l.get("ceiling", 0)), ids)
    ids = torch.where(upright & ~flat, torch.full_like(ids, c2l.get("wall", 0)), ids)
    return {"instance": instance, "instance_labels": ids}


def parse_planes(spec):
    """--planes[=RADIUS,ANGLE,OFFSET,MIN_POINTS]: None -> None (not asked for); '' -> label_planes' defaults; otherwise up
    to four comma-separated values in that order, an empty field keeping its default -> label_planes' keywords."""
    if spec is None:
        return None
    kw = {"radius": 0.1, "angle": 10.0, "offset": 0.02, "min_points": 100}
    parts = [p.strip() for p in spec.split(",")] if spec.strip() else []
    if len(parts) > 4:
        raise ValueError(f"--planes takes at most RADIUS,ANGLE,OFFSET,MIN_POINTS, got {spec!r}")
    for name, value in zip(("radius", "angle", "offset", "min_points"), parts):
        if not value:
            continue
        try:
            kw[name] = int(value) if name == "min_points" else float(value)
        except ValueError:
            raise ValueError(f"--planes: bad value {value!r} for {name}") from None
    kw["radius"], kw["angle"], kw["offset"] = _check_join(kw["radius"], kw["angle"], kw["offset"])
    kw["min_points"] = whole(kw["min_points"], "min_points")
    return kw
