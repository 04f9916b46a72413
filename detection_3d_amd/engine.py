"""Loops around the detector: the reference's `inference` (maskrcnn_benchmark/engine/inference_3d.py:16-36,
compute_on_dataset + gather + evaluate) and `do_train` (engine/trainer_sparse3d.py:42-160), composed from this package's
pieces so that one process per GPU feeds itself:

    ScenePrefetcher (files[rank::world], pinned host buffers, copy on a side stream)
      -> d3d_voxelize -> SparseRCNN -> pack_detections / gather_detections (one all_gather of padded tensors)
      -> eval_detection_suncg on rank 0

There is no collective on the inference data path; training adds DistributedDataParallel's bucketed gradient all-reduce
(RCCL over xGMI) and the small loss `reduce` for logging."""
import os
import time

import torch
import torch.distributed as dist

from . import training as T
from .distributed import agree_capacity, gather_detections, pack_detections
from .prepare import Preparation
from .scene_io import ScenePrefetcher


def _hip_voxelize(pcl, cfg):
    from .voxelize import voxelize          # d3d_voxelize: needs the GPU library
    return voxelize(pcl, cfg.SPARSE3D.VOXEL_SCALE, cfg.SPARSE3D.VOXEL_FULL_SCALE)


def collate(scenes, cfg, voxelize_fn=_hip_voxelize, augment=None, normals=None, crop=None, downsample=None, clean=None,
            fit=None):
    """data3d/data.py:15,23-35 (batch collation) for the detector: every scene [(pcl, targets), ...] is voxelised on its own
    (shifted by its own minimum, as the dataset does per scene), gets its example index as a 4th coordinate column, and
    the examples are listed one after the other.  -> (points = [coords int64 [N, 4], feats [N, F], B], [targets]).
    augment (augment.Augment): every example is augmented on its own with its own draws, in place of `voxelize_fn`;
    its targets must then be in the file's frame (ScenePrefetcher(shift_targets=False)).
    normals (None, 'estimate' or a dict of estimate_normals keywords): the raw cloud's normal columns are estimated on
    the GPU first (normals.with_normals), before voxelisation and before `augment`, which then flips and rotates them
    with the points; its elastic distortion comes after the estimate and does not bend them.
    crop ((sx, sy) in metres, or a primitives.RandomCrop): every scene is first cut to a random window of that size and
    its boxes are cropped to the points that remain or dropped (primitives.crop_scene), before the normals, the
    voxelisation and `augment`.  Like `augment` it needs the targets in the file's frame; without `augment` they are
    shifted afterwards as scene_targets(shift=True) shifts them.
    downsample (None, a voxel size, or a dict with keys among voxel, max_points, seed): every raw cloud is reduced to one
    point per voxel and capped (downsample.voxel_downsample, cap_points) after the crop and before the normals, so that
    the order is crop -> down-sample -> cap -> estimated normals -> voxelise or augment.  The detector's frame is the
    minimum of the cloud that is voxelised, which the raw cloud's minimum misses by up to a voxel: like `crop`,
    `downsample` needs the targets in the file's frame and shifts them afterwards.
    clean (None, or a dict with keys among radius, min_neighbors, statistical, min_component: clean.clean_cloud's
    keywords): outliers and small detached components are removed after the cap and before the normals
    (clean.clean_cloud), so that a stray return does not move the frame; the minimum moves, so the targets are treated
    as with `downsample`.
    A scene whose targets are {"instance": int [N], "instance_labels": int64 [K]} (an instance id per point and a label id
    per instance, no boxes) gets its boxes fitted on the GPU first, before the crop (primitives.targets_from_labels); they
    are in the file's frame and are shifted like those of `crop`.  fit (None or a dict with keys among min_points,
    min_size): that function's keywords."""
    return _collate(scenes, cfg, Preparation(crop=crop, downsample=downsample, normals=normals, augment=augment,
                                             voxelize_fn=voxelize_fn, clean=clean, fit=fit))


def _collate(scenes, cfg, chain):
    cs, fs, tgs = [], [], []
    for b, (pcl, tg) in enumerate(scenes):
        c, f, tg = chain.scene(pcl, tg, cfg)
        cs.append(torch.cat([c, torch.full((c.shape[0], 1), b, dtype=c.dtype, device=c.device)], 1))
        fs.append(f)
        tgs.append(tg)
    if not cs:
        raise ValueError("collate: no scene")
    return [torch.cat(cs), torch.cat(fs), len(cs)], tgs


def group_batches(items, n):
    """consecutive items in groups of `n` (the last group may be shorter)"""
    if n < 1:
        raise ValueError(f"batch size {n} < 1")
    group = []
    for it in items:
        group.append(it)
        if len(group) == n:
            yield group
            group = []
    if group:
        yield group


def _rank_world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def inference(model, cfg, files, device, depth=2, max_det=None, voxelize_fn=_hip_voxelize, normals=None,
              downsample=None, clean=None):
    """Detections of every building in `files`, sharded over the ranks of the default process group.
    -> on rank 0: ({file index: detections dict}, {file index: targets dict of the building in the detector's frame});
    None on the other ranks.  Targets travel with the detections so that rank 0 can evaluate without re-reading files.
    normals, downsample, clean: as in `collate` (files that hold xyz, or xyz and colour, get their normal columns
    estimated); with downsample or clean the targets are read in the file's frame and shifted by the minimum of the cloud
    that is voxelised."""
    chain = Preparation(downsample=downsample, normals=normals, voxelize_fn=voxelize_fn, clean=clean)
    rank, world = _rank_world()
    max_det = max_det or int(cfg.MODEL.ROI_HEADS.DETECTIONS_PER_IMG) * max(1, len(cfg.MODEL.SEPARATE_CLASSES_ID) + 1)
    pre = ScenePrefetcher(files, cfg.INPUT.CLASSES, cfg.SPARSE3D.VOXEL_SCALE, device=device, rank=rank, world=world,
                          depth=depth, shift_targets=not chain.targets_in_file_frame)
    was_training = model.training
    model.eval()
    results, truths = [], []
    with torch.no_grad():
        for i, (pcl, tg, _path) in enumerate(pre):
            coords, feats, tg = chain.scene(pcl, tg, cfg)
            results.append((rank + i * world, model([coords, feats])))
            truths.append({"bbox3d": tg["bbox3d"], "labels": tg["labels"],
                           "scores": torch.ones(tg["bbox3d"].shape[0], device=tg["bbox3d"].device)})
    model.train(was_training)
    # capacities from the data (one MAX all-reduce each): a building with more ground-truth boxes -- or, with ties at the
    # cut, more detections -- than DETECTIONS_PER_IMG x groups keeps all of them
    cap_det = agree_capacity([r["bbox3d"].shape[0] for _, r in results], max_det, device)
    cap_gt = agree_capacity([t["bbox3d"].shape[0] for t in truths], 1, device)
    local = [pack_detections(sid, r, cap_det) for sid, r in results]
    local_gt = [pack_detections(sid, t, cap_gt) for (sid, _), t in zip(results, truths)]
    n = len(files)
    # a rank without buildings still takes part in the gathers, with an empty contribution on ITS device
    dets = gather_detections(local, n, cap_det, device=device)
    gts = gather_detections(local_gt, n, cap_gt, device=device)
    if rank != 0:
        return None
    return dets, {k: {"bbox3d": v["bbox3d"], "labels": v["labels"]} for k, v in gts.items()}


def evaluate(cfg, dets, gts):
    """data3d/evaluation/suncg/suncg_eval.py:714-966 on gathered results (rank 0): AP (VOC-07), AIoU, recall tables."""
    from .evaluation import eval_detection_suncg

    def host(d):
        return {k: v.detach().cpu().numpy() for k, v in d.items()}

    ids = sorted(dets.keys())
    return eval_detection_suncg([host(dets[i]) for i in ids], [host(gts[i]) for i in ids], cfg)


def _cycled_scenes(files, cfg, device, rank, world, depth, shift_targets=True):
    """the rank's buildings, prefetched, cycled epoch after epoch; `files` may also hold scenes that are already in
    memory, (pcl, targets) pairs on the device, which are cycled as they are"""
    if len(files) and not isinstance(files[0], (str, os.PathLike)):
        mine = list(files)[rank::world]
        if not mine:
            raise ValueError(f"rank {rank} of {world} has no building: {len(files)} scenes")
        while True:
            for pcl, tg in mine:
                yield pcl, tg
    while True:
        pre = ScenePrefetcher(files, cfg.INPUT.CLASSES, cfg.SPARSE3D.VOXEL_SCALE, device=device, rank=rank,
                              world=world, depth=depth, shift_targets=shift_targets)
        if len(pre) == 0:
            raise ValueError(f"rank {rank} of {world} has no building: {len(files)} files")
        for pcl, tg, _path in pre:
            yield pcl, tg


def train(model, cfg, files, device, steps, local_rank=None, log_every=0, depth=2, voxelize_fn=_hip_voxelize,
          ims_per_gpu=1, augment=None, normals=None, crop=None, downsample=None, clean=None, fit=None):
    """`steps` iterations of data-parallel training over `files[rank::world]` (cycled): `ims_per_gpu` consecutive
    buildings per rank and step (one batch through `collate` when > 1; the global batch world x ims_per_gpu is the
    reference's IMS_PER_BATCH).  `model` must already sit on `device`; it is wrapped in DistributedDataParallel when a
    process group with more than one rank exists.  augment, normals, crop, downsample, clean: as in `collate`, for every
    building (prepare.Preparation), rank r drawing with seed + 1000003 r in `augment` and `crop`; with any of augment,
    crop, downsample and clean the targets are read in the file's frame and follow the cloud that is voxelised.  fit: as
    in `collate`, for scenes that carry instance ids instead of boxes; such scenes are given in memory: `files` may be a
    list of (pcl, targets) pairs on `device` in place of paths (with augment, crop, downsample or clean their boxes, if
    they have any, must be in the file's frame).
    -> dict(buildings_per_s (examples/s), ms_per_step, last reduced losses)."""
    chain = Preparation(crop=crop, downsample=downsample, normals=normals, augment=augment, voxelize_fn=voxelize_fn,
                        clean=clean, fit=fit)
    rank, world = _rank_world()
    ims = int(ims_per_gpu)
    if ims < 1:
        raise ValueError(f"ims_per_gpu {ims_per_gpu} < 1")
    model.train()
    opt = T.make_optimizer(cfg, model)
    ddp = T.wrap_ddp(model, local_rank) if world > 1 else model
    if world == 1:
        T.freeze_unused(model)
    if ims == 1:
        sched = T.make_lr_scheduler(cfg, opt, examples_per_epoch=max(len(files), 1))
    else:                                   # iterations per epoch counted with the global batch (defaults.py:299-301)
        sched_cfg = cfg.clone()
        sched_cfg.SOLVER.IMS_PER_BATCH = world * ims
        sched = T.make_lr_scheduler(sched_cfg, opt, examples_per_epoch=max(len(files), 1))
    chain = chain.for_rank(rank, cfg.INPUT.CLASSES)
    it, t0, reduced = 0, None, {}
    scenes = _cycled_scenes(files, cfg, device, rank, world, depth, not chain.targets_in_file_frame)
    for batch in group_batches(scenes, ims):
        if it == 1:                          # the first iteration pays allocations and the bucket build
            if device is not None:
                torch.cuda.synchronize(device)
            t0 = time.perf_counter()
        if ims == 1:
            coords, feats, tg = chain.scene(*batch[0], cfg)
            _, reduced = T.train_step(ddp, opt, sched, [coords, feats], tg)
        else:
            points, tgs = _collate(batch, cfg, chain)
            _, reduced = T.train_step(ddp, opt, sched, points, tgs)
        it += 1
        if log_every and rank == 0 and it % log_every == 0:
            print(f"iter {it}: " + "  ".join(f"{k} {float(v):.4f}" for k, v in sorted(reduced.items())), flush=True)
        if it >= steps:
            break
    if device is not None:
        torch.cuda.synchronize(device)
    dt = time.perf_counter() - (t0 if t0 is not None else time.perf_counter())
    timed = max(steps - 1, 0)
    t = torch.tensor([dt], dtype=torch.float64, device=device if device is not None else "cpu")
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    return {"buildings_per_s": (world * ims * timed / dt) if dt > 0 and timed else None,
            "ms_per_step": (1e3 * dt / timed) if timed else None, "steps_timed": timed, "world": world,
            "ims_per_gpu": ims,
            "losses": {k: float(v.detach()) for k, v in reduced.items()}}
