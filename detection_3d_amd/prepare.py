"""From a raw input to what the detector takes, the one place that knows the order of the steps:

    unproject (serving, DepthFrames only) | crop (training) -> down-sample -> cap -> clean -> estimated normals
      -> align (serving: levelled and squared to the walls by the normals, frame.align_cloud)
      -> voxelise + targets shifted into the voxelised cloud's frame | augment

engine.collate / inference / train and serving.BuildingPipeline all go through it.  Every step runs on the caller's
current stream; a step whose option is None issues no kernel, allocates nothing and reads nothing back.  `align` is
for clouds without targets: a training scene's boxes cannot take a tilt, so `scene` refuses it."""
import copy
from collections import namedtuple

import torch

from .clean import apply_clean, clean_kwargs, compose_sources
from .downsample import apply_downsample, downsample_kwargs
from .frame import align_cloud, align_kwargs, detector_pose
from .normals import normals_kwargs, with_normals
from .primitives import (as_crop, fit_kwargs, is_labelled, points_in_boxes, shift_targets,
                         targets_from_labels)
from .unproject import DepthFrames, unproject, unproject_kwargs

# what point_ownership needs of one served input: the cloud the owners are found in (None: the input itself), raw row ->
# its row of that cloud (None: the same rows), the pixel of every unprojected row (None: the input was a cloud), and with
# `align` the detector's frame <- the raw cloud's frame, fp64 [4, 4] on the device (frame.detector_pose; None: not aligned)
Kept = namedtuple("Kept", "cloud source pixels pose", defaults=(None,))


class Preparation(object):
    """The keywords of the loops (unproject_kwargs, as_crop, downsample_kwargs, clean_kwargs, normals_kwargs, fit_kwargs,
    align_kwargs; an augment.Augment; voxelize_fn(pcl, cfg) -> (coords, feats)), checked here before anything touches a
    config, a model or a device."""

    def __init__(self, unproject=None, crop=None, downsample=None, normals=None, augment=None, voxelize_fn=None,
                 clean=None, fit=None, align=None):
        self.align = align_kwargs(align)
        self.fit = fit_kwargs(fit)
        self.unproject = unproject_kwargs(unproject)
        self.crop = as_crop(crop)
        self.downsample = downsample_kwargs(downsample)
        self.clean = clean_kwargs(clean)
        self.normals = normals_kwargs(normals)
        self.augment, self.voxelize_fn = augment, voxelize_fn

    @property
    def targets_in_file_frame(self):
        """crop, down-sample, clean and augment each move the detector's frame (the cloud's minimum):
        ScenePrefetcher(shift_targets=False) feeds `scene`"""
        return (self.crop is not None or self.downsample is not None or self.clean is not None or
                self.augment is not None)

    def for_rank(self, rank, classes):
        """the same chain drawing with seed + 1000003 rank in `augment` (checked against the classes) and `crop`"""
        chain = copy.copy(self)
        if self.augment is not None:
            chain.augment = self.augment.for_rank(rank)
            chain.augment.check_classes(classes)
        if self.crop is not None:
            chain.crop = self.crop.for_rank(rank)
        return chain

    def cloud(self, raw, keep=False):
        """raw: a cloud or a DepthFrames -> (the cloud to voxelise, None); with keep the second entry is the Kept that
        point_ownership takes.  With every option None the cloud is `raw` itself.  With `align` the cloud is the aligned
        one, and so is Kept.cloud (the detections live in its frame); the second entry is then a Kept without keep
        too, with nothing but its pose."""
        pcl, source, pixels = raw, None, None
        if isinstance(raw, DepthFrames):
            pcl = unproject(raw, return_pixels=keep, **self.unproject)
            if keep:
                pcl, pixels = pcl
        pcl = apply_downsample(pcl, self.downsample, return_source=keep)
        if keep:
            pcl, source = pcl
        pcl = apply_clean(pcl, self.clean, return_source=keep)
        if keep:
            pcl, cleaned = pcl
            source = compose_sources(source, cleaned)
        kept = Kept(None if pcl is raw else pcl, source, pixels) if keep else None
        if self.normals is not None:
            pcl = with_normals(pcl, **self.normals)
        if self.align is not None:
            pcl, frame = align_cloud(pcl, **self.align)
            pose = detector_pose(frame, pcl)
            kept = Kept(pcl, source, pixels, pose) if keep else Kept(None, None, None, pose)
        return pcl, kept

    def scene(self, pcl, tg, cfg):
        """one training or evaluation scene -> (coords, feats, targets in the frame of coords).  Targets of the form
        {"instance", "instance_labels"} (a scan with an id per point) become boxes first (primitives.targets_from_labels,
        `fit`): in the file's frame, whatever the other options say, so they are shifted after voxelisation."""
        if self.align is not None:
            raise ValueError("Preparation.scene: align is for clouds without targets (a yx_zb box cannot take a tilt); "
                             "align the scan before it is labelled")
        fitted = is_labelled(tg)
        if fitted:
            tg = targets_from_labels(pcl, tg["instance"], tg["instance_labels"], classes=cfg.INPUT.CLASSES, **self.fit)
        if self.crop is not None:
            pcl, tg = self.crop(pcl, tg)
        pcl, _ = self.cloud(pcl)
        if self.augment is not None:
            return self.augment(pcl, tg, cfg)
        coords, feats = self.voxelize_fn(pcl, cfg)
        if self.targets_in_file_frame or fitted:
            tg = shift_targets(pcl, tg, cfg.SPARSE3D.VOXEL_SCALE)
        return coords, feats, tg


def point_ownership(kept, raw, boxes):
    """-> (point_owner int32, one entry per row of the raw cloud (`raw`, or the unprojected one): the first box that
    holds the point it went into, -1 for none or for a row that went nowhere; point_count int32 per box)"""
    owner, count, _, _ = points_in_boxes(raw if kept.cloud is None else kept.cloud, boxes.to(torch.float32), origin="min")
    if kept.source is not None:
        # entry M of the table: the rows that went nowhere (source -1 indexes it from the end)
        table = torch.cat([owner, torch.full((1,), -1, dtype=owner.dtype, device=owner.device)])
        owner = table[kept.source.long()]
    return owner, count
