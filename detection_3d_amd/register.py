"""Aligning overlapping scans.  Every other step from raw sensor data to the detector's input (unproject, scan_mesh,
voxel_downsample, clean_cloud, estimate_normals, segment_planes, fit_boxes) takes a cloud that is already in one frame,
while a building is scanned from many stations whose poses are good to a few centimetres and degrees: enough to double
every wall.  The reference's users align the stations with open3d's registration_icp on the CPU; here it is a call on
the GPU (libd3d_hip, register.hip), built on a query of one cloud's cell list by the points of another.

Semantics (include/d3d_hip.h), restatements that are not pinned against open3d itself.  nearest: the cloud
row with the smallest (d2, row) among those with d2 = (dx dx + dy dy) + dz dz <= radius^2 in fp32, estimate_normals'
test.  icp: Gauss-Newton steps on the point-to-plane (or point-to-point) residuals of the pairs nearest finds within
max_dist, sums in fp64 in a fixed order, a 6 x 6 Cholesky solve on the device; pose = [R t; 0 1] with x' = R x + t
mapping source into the target's frame.  The same input gives the same bits, whatever torch's deterministic mode says.

Scans that come without any pose (a tripod lidar moved from room to room, a second session, a BIM export) get their
start from global_align (global_align.hip): each cloud levelled and squared by frame.manhattan_frame, then a
quarter turn, a shift on a lattice and a z shift from integer histograms, their correlations' peaks and a verification
against bird's-eye wall bitmaps; numpy reproduces every output bit for bit (tests/global_ref.py)."""
import ctypes
import math
import warnings

import numpy as np
import torch

from ._cloud import PhaseTimer, fp32_cloud, gpu_rows, number, options, run, same_device, scratch, whole
from ._lib import GlobalAlignDetails, ints, ptr, stream_of
from .clean import PHASES as NEAREST_PHASES
from .downsample import apply_downsample, downsample_kwargs
from .frame import align_cloud, align_kwargs
from .normals import check_args as check_normals_args, estimate_normals
from .pose import apply_pose, check_pose, inverse_pose          # noqa: F401  (apply_pose, inverse_pose: public here)
from .primitives import cloud_min

ICP_PHASES = ("cells", "sort", "table", "transform", "nearest", "accumulate", "solve")
METHODS = {"plane": 0, "point": 1}
HISTORY_COLS = 20
SYSTEM_SIZE = 29
MAX_ITERATIONS = 10000
STATUS = {0: "iterations exhausted", 1: "converged", 2: "degenerate"}


def nearest(query_xyz, cloud_xyz, radius=0.1, return_dist2=False, phases=False):
    """query_xyz fp32 [M, >= 3], cloud_xyz fp32 [N, >= 3] on the GPU (column slices of wider clouds are read in place)
    -> index int32 [M]: the row of the cloud nearest to every query among those within `radius`, ties to the lowest row,
    -1 when there is none or the query is not finite; with return_dist2 also that squared distance, fp32 [M], +inf for
    none.  Current stream, no read-back.  phases: also a dict of milliseconds (cells, sort, table, search, tail), timed
    with events inside the library; synchronises."""
    radius = number(radius, "radius", lo_open=True)
    query, m, qstride = gpu_rows(query_xyz, "query_xyz")
    cloud, n, cstride = gpu_rows(cloud_xyz, "cloud_xyz")
    dev = same_device(query_xyz=query, cloud_xyz=cloud)
    index = torch.empty((m,), dtype=torch.int32, device=dev)
    dist2 = torch.empty((m,), dtype=torch.float32, device=dev) if return_dist2 else None
    timer = PhaseTimer(NEAREST_PHASES, phases)
    if m > 0:
        buf, nbytes = scratch(dev, "d3d_nearest_scratch_bytes", n, m)
        run(dev, "d3d_nearest", ptr(cloud), n, cstride, ptr(query), m, qstride, radius, ptr(index), ptr(dist2), ptr(buf),
            nbytes, stream_of(dev), timer.ms)
    res = (index,) + ((dist2,) if return_dist2 else ()) + ((timer.read(),) if phases else ())
    return res[0] if len(res) == 1 else res


class Registration:
    """What icp returns.  pose fp64 [4, 4], state int32 [2] = (steps, status) and history fp64 [iterations, 20] (per
    executed step the pose after it, the pairs c, the squared error e, |w|, |v|; NaN past `steps`) stay on the device;
    the properties read them back on first use.  With return_details also last_index int32 [M] (the target row of every
    source row in the last executed step, -1: none) and last_system fp64 [29] (its A, b, e, c); phases: the dict of
    milliseconds, when asked for."""

    def __init__(self, pose, state, history, last_index=None, last_system=None, phases=None):
        self.pose, self.state, self.history = pose, state, history
        self.last_index, self.last_system, self.phases = last_index, last_system, phases
        self._host = None

    def _read(self):
        if self._host is None:
            steps, status = (int(v) for v in self.state.cpu())
            last = self.history[steps - 1].cpu().tolist() if steps > 0 else None
            self._host = (steps, status, last)
        return self._host

    @property
    def steps(self):
        return self._read()[0]

    @property
    def status(self):
        """0: the iterations ran out, 1: converged, 2: degenerate (fewer than 6 pairs, or a vanished pivot)"""
        return self._read()[1]

    @property
    def converged(self):
        return self._read()[1] == 1

    @property
    def inliers(self):
        """the pairs of the last executed step"""
        last = self._read()[2]
        return int(last[16]) if last else 0

    @property
    def rmse(self):
        """sqrt(e / c) of the last executed step, at the pose before it; NaN without a pair"""
        last = self._read()[2]
        return math.sqrt(last[17] / last[16]) if last and last[16] > 0 else float("nan")

    def __repr__(self):
        steps, status, _ = self._read()
        return f"Registration(steps={steps}, status={status} ({STATUS.get(status)}), inliers={self.inliers}, rmse={self.rmse:.6g})"


def _check_icp(max_dist, iterations, tol, method, init):
    max_dist = number(max_dist, "max_dist", lo_open=True)
    iterations = whole(iterations, "iterations", 1, MAX_ITERATIONS)
    tol = number(tol, "tol")
    if method not in METHODS:
        raise ValueError(f"method {method!r}: 'plane' or 'point'")
    pose = torch.eye(4, dtype=torch.float64) if init is None else check_pose(init, "init")
    return max_dist, iterations, tol, method, pose


def icp(source, target, target_normals=None, init=None, max_dist=0.1, iterations=30, tol=1e-6, method="plane",
        normal_radius=0.1, max_nn=50, return_details=False, phases=False):
    """source fp32 [M, >= 3], target fp32 [N, >= 3] on the GPU -> Registration: the pose that maps source onto target,
    from `init` (4 x 4, default identity) by at most `iterations` Gauss-Newton steps over the pairs within max_dist;
    stops when the step's rotation vector and translation are both at most `tol` long (status 1) or the system is
    degenerate (status 2, the pose stays).  method 'plane' needs the target's normals: target_normals fp32 [N, >= 3], or
    columns 6:9 of a nine-column target, or estimate_normals(target, normal_radius, max_nn).  All steps are enqueued on
    the current stream at once and nothing is read back.  Bad arguments raise ValueError before any GPU work."""
    max_dist, iterations, tol, method, pose = _check_icp(max_dist, iterations, tol, method, init)
    if method == "plane" and target_normals is None:
        check_normals_args(normal_radius, max_nn)
    fp32_cloud(target, "target")             # its faults come before the first word about the source's device
    src, m, sstride = gpu_rows(source, "source")
    tgt, n, tstride = gpu_rows(target, "target")
    dev = same_device(source=src, target=tgt)
    nrm, nstride = None, 3
    if method == "plane":
        if target_normals is not None:
            nrm, nn, nstride = gpu_rows(target_normals, "target_normals")
            if nn != n or nrm.device != dev:
                raise ValueError(f"icp: target_normals [{nn}, ..] on {nrm.device} for a target of {n} rows on {dev}")
        elif target.shape[1] == 9:
            nrm, _, nstride = gpu_rows(target[:, 6:9], "target")
        else:
            nrm = estimate_normals(tgt, normal_radius, max_nn)
    pose = pose.to(dev)
    state = torch.zeros((2,), dtype=torch.int32, device=dev)
    history = torch.full((iterations, HISTORY_COLS), float("nan"), dtype=torch.float64, device=dev)
    last_index = torch.full((m,), -1, dtype=torch.int32, device=dev) if return_details else None
    last_system = torch.zeros((SYSTEM_SIZE,), dtype=torch.float64, device=dev) if return_details else None
    timer = PhaseTimer(ICP_PHASES, phases)
    buf, nbytes = scratch(dev, "d3d_icp_scratch_bytes", n, m)
    run(dev, "d3d_icp", ptr(src), m, sstride, ptr(tgt), n, tstride, ptr(nrm), nstride, max_dist, METHODS[method],
        iterations, tol, ptr(pose), ptr(history), ptr(state), ptr(last_index), ptr(last_system), ptr(buf), nbytes,
        stream_of(dev), timer.ms)
    return Registration(pose, state, history, last_index, last_system, timer.read())


GLOBAL_PHASES = ("rows", "cells", "correlate", "peaks", "verify", "pick")
MAX_LATTICE = 4096
MAX_PEAKS = 64
MAX_SEP = 64
MAX_TOL = 20.0
MARGIN_MAX = 0.98     # merge_scans: a runner-up this close to the best is taken for an ambiguous building


def _check_global(bin, lattice, tol, peaks, sep, frame):
    """-> (bin, (L, L, Lz), c2, peaks, sep, manhattan_frame's keywords)"""
    bin, tol = number(bin, "bin", 0.0, 1e6, lo_open=True), number(tol, "tol", 0.0, MAX_TOL, lo_open=True)
    try:
        lattice = tuple(lattice)
    except TypeError:
        raise ValueError(f"lattice {lattice!r} must be (Lx, Ly, Lz)") from None
    if len(lattice) != 3:
        raise ValueError(f"lattice {lattice!r} must be (Lx, Ly, Lz)")
    lattice = (whole(lattice[0], "lattice: Lx", 32, MAX_LATTICE), whole(lattice[1], "lattice: Ly", 32, MAX_LATTICE),
               whole(lattice[2], "lattice: Lz", 1, MAX_LATTICE))
    if lattice[0] != lattice[1] or lattice[0] % 32:
        raise ValueError(f"lattice {lattice}: Lx == Ly, a multiple of 32")
    peaks = whole(peaks, "peaks", 1, MAX_PEAKS)
    sep = whole(sep, "sep", 0, MAX_SEP)
    frame_kw = align_kwargs(True if frame is None else frame)
    if frame_kw is None:
        raise ValueError(f"frame {frame!r}: a dict of manhattan_frame's keywords (max_tilt, tol, up)")
    c2 = float(np.float32(math.cos(math.radians(tol)) ** 2))
    return bin, lattice, c2, peaks, sep, frame_kw


class Alignment:
    """What global_align returns.  pose fp64 [4, 4] (source frame -> target frame), lattice_pose (the same between the two
    levelled frames), source_frame and target_frame (the Frames of align_cloud), choice int32 [4] = (q, sx, sy, sz), score
    int64 [6] (the best score of each quarter turn, the best of all, the runner-up), support int32 [4] (rows used and
    dropped, source then target) and state int32 [1] stay on the device; the properties read them back on first use.
    details (return_details): the tables of the call as device tensors; phases: the dict of milliseconds, when asked for."""

    def __init__(self, pose, lattice_pose, source_frame, target_frame, choice, score, support, state, details=None,
                 phases=None):
        self.pose, self.lattice_pose, self.source_frame, self.target_frame = pose, lattice_pose, source_frame, target_frame
        self.choice, self.score, self.support, self.state = choice, score, support, state
        self.details, self.phases = details, phases
        self._host = None

    def _read(self):
        if self._host is None:
            self._host = (int(self.state.cpu()[0]), [int(v) for v in self.score.cpu()], [int(v) for v in self.choice.cpu()])
        return self._host

    @property
    def status(self):
        """0: fine; 1: no wall of the source met a wall of the target, the pose is the origins' shift alone"""
        return self._read()[0]

    @property
    def heading_scores(self):
        """the best score of each quarter turn"""
        return self._read()[1][:4]

    @property
    def best(self):
        return self._read()[1][4]

    @property
    def margin(self):
        """runner-up over best: near 1 the building looks the same under another turn or shift (inf for status 1)"""
        sc = self._read()[1]
        return max(sc[5], 0) / sc[4] if sc[4] > 0 else float("inf")

    @property
    def quarter_turns(self):
        return self._read()[2][0]

    def __repr__(self):
        status, sc, ch = self._read()
        return f"Alignment(status={status}, choice={ch}, best={sc[4]}, margin={self.margin:.3g})"


def _with_normals(cloud, normals, normal_radius, max_nn, what):
    """-> fp32 [N, 6]: position and normal of every row, the normals resolved as icp resolves its target's"""
    xyz, n, _ = gpu_rows(cloud, what)
    if normals is not None:
        nrm, nn, _ = gpu_rows(normals, f"{what}_normals")
        if nn != n or nrm.device != xyz.device:
            raise ValueError(f"global_align: {what}_normals [{nn}, ..] on {nrm.device} for {n} rows on {xyz.device}")
    elif cloud.shape[1] == 9:
        nrm = cloud.detach()[:, 6:9]
    else:
        nrm = estimate_normals(xyz, normal_radius, max_nn)
    return torch.cat([xyz[:, :3], nrm[:, :3]], 1)


def lattice_align(source, source_normals, source_origin, target, target_normals, target_origin, bin=0.05,
                  lattice=(2048, 2048, 256), tol=5.0, peaks=64, sep=2, return_details=False, phases=False):
    """d3d_global_align as it stands (include/d3d_hip.h): two clouds that are levelled and squared already, fp32 [rows, >= 3]
    positions and normals on the GPU (column slices are read in place), and per cloud an origin, fp64 [3] on the device
    (primitives.cloud_min) -> Alignment whose pose is the one between the two levelled frames.  Current stream, no
    read-back."""
    bin, lattice, c2, peaks, sep, _ = _check_global(bin, lattice, tol, peaks, sep, None)
    src, m, sstride = gpu_rows(source, "source")
    snrm, sm, snstride = gpu_rows(source_normals, "source_normals")
    tgt, n, tstride = gpu_rows(target, "target")
    tnrm, tn, tnstride = gpu_rows(target_normals, "target_normals")
    dev = src.device
    if sm != m or tn != n or any(t.device != dev for t in (snrm, tgt, tnrm)):
        raise ValueError(f"lattice_align: {m} / {sm} source and {n} / {tn} target rows and normals, on one device")
    origins = []
    for o in (source_origin, target_origin):
        if not isinstance(o, torch.Tensor) or o.shape != (3,) or o.dtype != torch.float64 or o.device != dev:
            raise ValueError("lattice_align: an origin is a float64 tensor [3] on the clouds' device")
        origins.append(o.detach().contiguous())
    L, Lz, K = lattice[0], lattice[2], peaks
    A = torch.empty((4, 4), dtype=torch.float64, device=dev)
    choice = torch.empty((4,), dtype=torch.int32, device=dev)
    score = torch.empty((6,), dtype=torch.int64, device=dev)
    support = torch.empty((4,), dtype=torch.int32, device=dev)
    state = torch.empty((1,), dtype=torch.int32, device=dev)
    details, det = None, None
    if return_details:
        i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
        details = {"hist": torch.empty((2, 2 * L + Lz), **i32), "cells": torch.empty((2, max(1, min(m, L * L))), **i32),
                   "cell_count": torch.empty((2,), **i32), "target_bits": torch.empty((2, L * L // 32), **i32),
                   "corr": torch.empty((9, 2 * max(L, Lz) - 1), **i64), "peak_value": torch.empty((9, K), **i64),
                   "peak_shift": torch.empty((9, K), **i32), "scores": torch.empty((4, K, K), **i32)}
        det = GlobalAlignDetails(*(ptr(details[k]) for k, _ in GlobalAlignDetails._fields_))
    lat = ints(lattice)
    buf, nbytes = scratch(dev, "d3d_global_align_scratch_bytes", m, lat, K)
    timer = PhaseTimer(GLOBAL_PHASES, phases)
    run(dev, "d3d_global_align", ptr(src), m, sstride, ptr(snrm), snstride, ptr(origins[0]), ptr(tgt), n, tstride,
        ptr(tnrm), tnstride, ptr(origins[1]), bin, lat, c2, K, sep, ptr(A), ptr(choice), ptr(score), ptr(support),
        ptr(state), ctypes.byref(det) if det is not None else None, ptr(buf), nbytes, stream_of(dev), timer.ms)
    return Alignment(A, A, None, None, choice, score, support, state, details, timer.read())


def global_align(source, target, bin=0.05, lattice=(2048, 2048, 256), tol=5.0, peaks=64, sep=2, frame=None,
                 normal_radius=0.1, max_nn=50, return_details=False, phases=False, source_normals=None,
                 target_normals=None):
    """source fp32 [M, >= 3], target fp32 [N, >= 3] on the GPU, each in a frame of its own with no pose between them ->
    Alignment: the coarse pose that maps source onto target, for icp(init=...) to refine.  Both clouds are levelled and
    squared (frame.align_cloud with the keywords in `frame`); what is left is one of four quarter turns, a shift on a
    lattice of `bin` metres (`lattice` cells per axis from each cloud's minimum, Lx == Ly a multiple of 32, at most 4096)
    and a z shift.  Walls (normals within `tol` degrees of x or y) and floors vote by integer histograms; the `peaks`
    best shifts per axis and turn, more than `sep` bins apart, are verified against bird's-eye bitmaps of the walls.
    Normals: *_normals fp32 [rows, >= 3], or columns 6:9 of a nine-column cloud, or estimate_normals(cloud,
    normal_radius, max_nn).  Limits: overlap is maximised and free space costs nothing, so on a point-symmetric building
    seen through a small overlap the half turn can win (Alignment.margin near 1 and heading_scores show it); z is the one
    strongest floor / ceiling peak, a storey off in a multi-storey partial overlap; the accuracy is half a bin per axis
    and the frames' heading error.  return_details: Alignment.details holds every table of the call (histograms, cell
    lists, the target's bitmaps, correlations, peak tables, the [4, K, K] scores) as device tensors; phases:
    Alignment.phases, the milliseconds of d3d_global_align's six phases (GLOBAL_PHASES), which synchronises.  Current
    stream, no read-back; bad arguments raise ValueError before any GPU work."""
    bin, lattice, _, peaks, sep, frame_kw = _check_global(bin, lattice, tol, peaks, sep, frame)
    check_normals_args(normal_radius, max_nn)
    same_device(source=fp32_cloud(source, "source"), target=fp32_cloud(target, "target"))
    six_s = _with_normals(source, source_normals, normal_radius, max_nn, "source")
    six_t = _with_normals(target, target_normals, normal_radius, max_nn, "target")
    with torch.cuda.device(source.device):
        src, fs = align_cloud(six_s, 3, **frame_kw)
        tgt, ft = align_cloud(six_t, 3, **frame_kw)
        found = lattice_align(src, src[:, 3:], cloud_min(src), tgt, tgt[:, 3:], cloud_min(tgt), bin, lattice, tol, peaks, sep,
                              return_details, phases)
        found.pose = inverse_pose(ft.pose) @ found.lattice_pose @ fs.pose
    found.source_frame, found.target_frame = fs, ft
    return found


def merge_scans(clouds, init_poses=None, reference=0, voxel=0.02, max_points=None, seed=0, global_kw=None, **icp_kw):
    """clouds: fp32 [N_i, C] GPU tensors of one width, each in its own frame; init_poses: None or one 4 x 4 (or None) per
    cloud, its rough pose in the reference's frame -> (cloud, poses).  The scans are taken in order; each one is
    registered (icp, **icp_kw) to the voxel-down-sampled union of the reference and the scans placed so far, moved with
    apply_pose and added to the union.  cloud: the union through apply_downsample(voxel, max_points, seed), ready for
    prepare_cloud / BuildingPipeline.map; poses: fp64 [4, 4] device tensors, the identity for the reference.  One
    read-back per registration (its state); a registration that does not converge raises a warning and its pose is
    used as it stands.  init_poses='global': the scans come without poses, and each one's start is global_align(scan,
    union so far, **global_kw)'s; when that finds no walls (status 1) or its margin exceeds MARGIN_MAX (0.98: another
    turn or shift fits as well) a warning is raised and the scan is registered from the identity."""
    clouds = list(clouds)
    if not clouds:
        raise ValueError("merge_scans: no clouds")
    use_global = isinstance(init_poses, str)
    if use_global and init_poses != "global":
        raise ValueError(f"merge_scans: init_poses {init_poses!r}: None, 'global' or one pose per cloud")
    if global_kw is not None and not use_global:
        raise ValueError("merge_scans: global_kw goes with init_poses='global'")
    global_kw = options(global_kw or {}, "merge_scans: global_kw",
                        ("bin", "lattice", "tol", "peaks", "sep", "frame", "normal_radius", "max_nn"))
    if use_global:
        init_poses = None
        _check_global(global_kw.get("bin", 0.05), global_kw.get("lattice", (2048, 2048, 256)), global_kw.get("tol", 5.0),
                      global_kw.get("peaks", 64), global_kw.get("sep", 2), global_kw.get("frame"))
    reference = whole(reference, "merge_scans: reference", 0, len(clouds) - 1)
    if init_poses is None:
        init_poses = [None] * len(clouds)
    init_poses = list(init_poses)
    if len(init_poses) != len(clouds):
        raise ValueError(f"merge_scans: {len(init_poses)} poses for {len(clouds)} clouds")
    init_poses = [None if p is None else check_pose(p, "merge_scans: init_poses") for p in init_poses]
    for c in clouds:
        if not isinstance(c, torch.Tensor) or c.dim() != 2 or c.shape[1] != clouds[0].shape[1] or c.shape[1] < 3:
            raise ValueError("merge_scans: tensors [N, C >= 3] of one width")
    # not target_normals and init: the target and the start differ per scan
    options(icp_kw, "merge_scans: icp's", ("max_dist", "iterations", "tol", "method", "normal_radius", "max_nn"))
    _check_icp(icp_kw.get("max_dist", 0.1), icp_kw.get("iterations", 30), icp_kw.get("tol", 1e-6),
               icp_kw.get("method", "plane"), None)
    model_kw = downsample_kwargs({"voxel": voxel})
    final_kw = downsample_kwargs({"voxel": voxel, "max_points": max_points, "seed": seed})
    union = clouds[reference]
    dev = union.device
    poses = [None] * len(clouds)
    poses[reference] = torch.eye(4, dtype=torch.float64, device=dev)
    for i, scan in enumerate(clouds):
        if i == reference:
            continue
        model = apply_downsample(union, model_kw)
        init = init_poses[i]
        if use_global:
            found = global_align(scan, model, **global_kw)
            if found.status != 0 or found.margin > MARGIN_MAX:
                warnings.warn(f"merge_scans: scan {i} has no clear global alignment ({found!r}); registering it from "
                              "the identity")
            else:
                init = found.pose
        reg = icp(scan, model, init=init, **icp_kw)
        if not reg.converged:
            warnings.warn(f"merge_scans: scan {i} did not converge ({STATUS.get(reg.status)} after {reg.steps} steps, "
                          f"{reg.inliers} pairs)")
        poses[i] = reg.pose
        union = torch.cat([union, apply_pose(scan, reg.pose)])
    return apply_downsample(union, final_kw), poses
