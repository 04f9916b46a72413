"""Several buildings in flight on one GPU (inference throughput).

One building at batch size 1 leaves the GPU under-occupied for a good part of its pass: building the grids and
rulebooks is a chain of small kernels with one host read-back per strided grid, the coarse FPN levels launch
convolutions over a few hundred rows, the detector tail reads two counts back and sweeps NMS with a single wave.
`BuildingPipeline` overlaps these phases of *consecutive* buildings, every building still an independent bs=1 pass:

    stage 1  geometry  (voxelize, input layer, all grids + rulebooks; read-backs)     thread "geometry"
    stage 2  features  (sparse-conv FPN; enqueue only, never waits for the GPU)       the calling thread
    stage 3  tail      (RPN decode + NMS, RoIAlign, box head, per-class NMS)          thread "tail"

Building i owns slot i % in_flight: a HIP stream for its geometry and tail stages (chains of small dependent kernels
whose latency sets the pipeline's rate; normal queue priority -- high priority, round 2's choice, helped on some boxes and
held the other building's convolutions back on others) and a stream for its feature pass, chained by events; its own metadata arena and scratch
(SCN._scratch_key), so no two buildings share mutable state; a semaphore bounds the buildings in flight.  While one
building's large convolutions run, the next one's geometry kernels and the previous one's tail fill the idle CUs and
hide their read-back latencies.  Results are
bit-identical to the serial loop (tests/test_detector_gpu.py); the reference has no counterpart (its test loop,
maskrcnn_benchmark/engine/inference.py:17-40 `compute_on_dataset`, is serial).
"""
import os
import queue
import threading

import torch

from .prepare import Preparation, point_ownership
from .voxelize import voxelize


class BuildingPipeline(object):
    """normals: None (clouds arrive with every column the config takes), 'estimate' or a dict of estimate_normals
    keywords: every raw cloud ([N, 3], [N, 6] or [N, 9]) gets its normal columns from normals.with_normals before it is
    voxelised, on its slot's geometry stream.
    point_owner: every result dict gets two more entries, computed on its slot's tail stream with
    primitives.points_in_boxes(cloud, detections, origin='min'): "point_owner" int32, one entry per row of the input
    cloud = the index of the first detection (the dict's order: descending score per class group) that holds the point,
    -1 for none, and "point_count" int32, the number of points in each detection.
    downsample: None, a voxel size, or a dict with keys among voxel, max_points, seed: every raw cloud is reduced to one
    point per voxel and capped (downsample.voxel_downsample, cap_points) on its slot's geometry stream, before the
    normals.  point_owner keeps one entry per row of the RAW cloud: the owner of the down-sampled point the row went
    into, -1 for a row that was dropped (position not finite) or capped away; "point_count" then counts the
    down-sampled points of each detection.
    clean: None, or a dict of clean.clean_cloud keywords (radius, min_neighbors, statistical, min_component): outliers and
    small detached components are removed on the slot's geometry stream after the down-sampling and before the normals.
    point_owner still has one entry per row of the RAW cloud, -1 for a row that was cleaned away.
    unproject: None or a dict of unproject.unproject keywords (columns, step, min_depth, max_depth, edge, color_div) for
    the inputs that are unproject.DepthFrames: such an input becomes a cloud on its slot's geometry stream first, and
    the steps above follow as for a cloud ("raw cloud" then means the unprojected one).  With point_owner its result also
    carries "point_pixel" int32, the pixel (f H + v) W + u of every row of that cloud (unproject.pixel_labels paints
    point_owner into the frames with it).
    align: None, True / 'manhattan', or a dict of frame.manhattan_frame keywords (max_tilt, tol, up): every cloud is
    levelled and squared to its walls by its normals (frame.align_cloud) on its slot's geometry stream, after the normals
    and before it is voxelised, for scans that arrive in a camera's or a reference station's frame.  The detections live in
    the aligned cloud's min-shifted frame; every result dict carries "frame_pose", fp64 [4, 4] on the device: that frame <-
    the input cloud's frame (frame.detector_pose; frame.box_corners_in_scan_frame takes the boxes back).  point_owner
    tests the points in the aligned frame.  Without align nothing changes and the key is absent.
    rooms: None, True, or a dict with keys among cell, grow, min_area, reach, max_rooms (floorplan.rooms_kwargs): every
    result dict gets the floor plan of its detections (floorplan.floorplan_of with the config's classes), computed on its
    slot's tail stream after the detections and before point_owner: "rooms" {"bbox3d" fp32 [max_rooms, 7], "area" fp64
    [max_rooms], "count" int32 [1]} and "box_rooms" int32 [detections, 2], what lies on either side of every detection.
    The lattice is explicit (floorplan.detector_lattice: the detections' min-shifted frame at `cell`), so nothing is read
    back.  With point_owner also "point_room" int32, one entry per row of the RAW cloud: floorplan.room_of_points of the
    point the row went into, floorplan.NONE for a row that went nowhere.  With rooms=None nothing is imported, launched
    or added."""

    def __init__(self, model, cfg, in_flight=2, device=None, normals=None, point_owner=False, downsample=None,
                 unproject=None, clean=None, align=None, rooms=None):
        self.prepare = Preparation(unproject=unproject, downsample=downsample, normals=normals, clean=clean, align=align)
        self.model, self.cfg = model, cfg
        self.point_owner = bool(point_owner)
        self.rooms = self.rooms_lattice = None
        if rooms is not None and rooms is not False:
            from .floorplan import detector_lattice, rooms_kwargs
            self.rooms = rooms_kwargs(rooms)
            self.rooms_lattice = detector_lattice(cfg, self.rooms["cell"])
        self.device = device if device is not None else next(model.parameters()).device
        self.in_flight = max(1, int(in_flight))
        # streams live as long as the pipeline: metadata arenas and scratch buffers are recycled per stream
        # (normal queue priority: as high-priority streams the geometry / tail stages held back the other building's feature
        #  pass on some boxes -- 203-208 against 204-216 buildings/s in pairs of runs; D3D_PIPE_PRIORITY=-1 restores it)
        prio = int(os.environ.get("D3D_PIPE_PRIORITY", "0"))
        self.hi = [torch.cuda.Stream(device=self.device, priority=prio) for _ in range(self.in_flight)]
        self.lo = [torch.cuda.Stream(device=self.device) for _ in range(self.in_flight)]

    def map(self, clouds):
        """clouds: list of float32 [N, F] point clouds resident on the device, or unproject.DepthFrames -> list of
        detection dicts, in order.
        The caller's stream is made to wait for the results (no device-wide synchronisation)."""
        clouds = list(clouds)
        n = len(clouds)
        if n == 0:
            return []
        s3d = self.cfg.SPARSE3D
        caller = torch.cuda.current_stream(self.device)
        ready = torch.cuda.Event()
        ready.record(caller)
        for st in self.hi:
            st.wait_event(ready)
        results, errors = [None] * n, []
        kept = [None] * n           # with point_owner or align: what the tail adds to the result, only until it has run
        slots = threading.Semaphore(self.in_flight)
        q_feat, q_tail = queue.Queue(), queue.Queue()
        stop = threading.Event()

        def slot(i):
            return self.hi[i % self.in_flight], self.lo[i % self.in_flight]

        def guarded(fn, downstream):
            def run():
                try:
                    torch.cuda.set_device(self.device)
                    with torch.no_grad():
                        fn()
                except BaseException as e:      # noqa: BLE001 - re-raised in the caller
                    errors.append(e)
                    stop.set()
                    for _ in range(self.in_flight + 1):
                        slots.release()
                finally:
                    if downstream is not None:
                        downstream.put(None)
            return run

        def geometry():
            for i in range(n):
                slots.acquire()
                if stop.is_set():
                    return
                hi, lo = slot(i)
                with torch.cuda.stream(hi):
                    hi.wait_stream(lo)      # the slot's previous building has left its arena and allocator blocks
                    pcl, kept[i] = self.prepare.cloud(clouds[i], keep=self.point_owner)
                    coords, feats = voxelize(pcl, s3d.VOXEL_SCALE, s3d.VOXEL_FULL_SCALE)
                    net = self.model.stage_geometry([coords, feats])
                    lo.wait_stream(hi)
                q_feat.put((i, net))

        def features():
            while True:
                item = q_feat.get()
                if item is None or stop.is_set():
                    return
                i, net = item
                hi, lo = slot(i)
                with torch.cuda.stream(lo):
                    feats = self.model.stage_features(net)
                    hi.wait_stream(lo)
                q_tail.put((i, feats))
                del net, feats, item

        def tail():
            while True:
                item = q_tail.get()
                if item is None or stop.is_set():
                    return
                i, feats = item
                with torch.cuda.stream(slot(i)[0]):
                    results[i] = r = self.model.stage_tail(feats)
                    k, kept[i] = kept[i], None
                    if self.rooms is not None:
                        from .floorplan import floorplan_of, point_rooms
                        plan = floorplan_of(r, self.cfg.INPUT.CLASSES, lattice=self.rooms_lattice, **self.rooms)
                        r["rooms"], r["box_rooms"] = plan["rooms"], plan["box_rooms"]
                        if k is not None and self.point_owner:
                            r["point_room"] = point_rooms(k, clouds[i], plan["plan"])
                        del plan
                    if k is not None and self.point_owner:
                        r["point_owner"], r["point_count"] = point_ownership(k, clouds[i], r["bbox3d"])
                        if k.pixels is not None:
                            r["point_pixel"] = k.pixels
                    if k is not None and k.pose is not None:
                        r["frame_pose"] = k.pose
                    del k
                del feats, item
                slots.release()

        threads = [threading.Thread(target=guarded(geometry, q_feat), name="d3d-geometry"),
                   threading.Thread(target=guarded(tail, None), name="d3d-tail")]
        for th in threads:
            th.start()
        guarded(features, q_tail)()
        for th in threads:
            th.join()
        if errors:
            raise errors[0]
        for st in self.hi:
            caller.wait_stream(st)
        for r in results:
            for v in list(r.values()) + list(r["rooms"].values() if self.rooms is not None else ()):
                if torch.is_tensor(v) and v.is_cuda:
                    v.record_stream(caller)
        return results
