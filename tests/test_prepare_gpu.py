"""detection_3d_amd.prepare with every option on at once, through engine.collate and serving.BuildingPipeline, against the
steps called by hand in the documented order.  Everything is compared bit for bit: both sides issue the same library
calls on the same inputs, and every step gives the same bits for the same input."""
import numpy as np
import pytest
import torch

from tests.points_ref import room_scene
from tests.unproject_ref import room_scene as rendered_room

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny(dev):
    """the model of tests/test_unproject_gpu.py"""
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.detector import build_detection_model
    cfg = get_cfg("4c_Fpn432")
    torch.manual_seed(1)
    model = build_detection_model(cfg).to(dev).eval()
    with torch.no_grad():
        model.rpn.head.cls_logits.weight.mul_(60)
        model.rpn.head.bbox_pred.weight.mul_(20)
        model.roi_heads.box.predictor.cls_score.weight.mul_(40)
        model.roi_heads.box.predictor.bbox_pred.weight.mul_(100)
    return cfg, model


def test_collate_with_every_option_is_the_steps_in_order(tiny, dev):
    from detection_3d_amd import engine
    from detection_3d_amd.augment import Augment
    from detection_3d_amd.downsample import apply_downsample, downsample_kwargs
    from detection_3d_amd.normals import with_normals
    from detection_3d_amd.primitives import RandomCrop
    cfg = tiny[0]
    scenes = []
    for seed in (0, 1):
        pcl, boxes, labels = room_scene(seed)              # rows in random order: the first 20 000 cover every wall
        scenes.append((torch.from_numpy(pcl[:20000, :6].copy()).to(dev),
                       {"bbox3d": torch.from_numpy(boxes), "labels": torch.from_numpy(labels)}))
    aug_kw = dict(rotate="free", flip_x=True, scale_jitter=0.1, origin_offset=True, elastic=True, color_noise=0.02, seed=5)
    dkw = {"voxel": 0.05, "max_points": 5000}
    points, tgs = engine.collate(scenes, cfg, augment=Augment(**aug_kw), normals="estimate",
                                 crop=RandomCrop((4, 4), seed=3), downsample=dkw)
    crop, aug = RandomCrop((4, 4), seed=3), Augment(**aug_kw)
    coords, feats, rows = [], [], []
    for b, (pcl, tg) in enumerate(scenes):
        pcl, tg = crop(pcl, tg)
        cropped = pcl.shape[0]
        pcl = apply_downsample(pcl, downsample_kwargs(dkw))
        assert 0 < pcl.shape[0] <= min(cropped, 5000) and cropped < 20000 and pcl.shape[1] == 6
        pcl = with_normals(pcl)
        c, f, tg = aug(pcl, tg, cfg)
        assert 0 < c.shape[0] <= 5000 and f.shape[1] == 9 and 0 < tg["bbox3d"].shape[0] <= 5
        coords.append(torch.cat([c, torch.full((c.shape[0], 1), b, dtype=c.dtype, device=dev)], 1))
        feats.append(f)
        assert torch.equal(tgs[b]["bbox3d"], tg["bbox3d"]) and torch.equal(tgs[b]["labels"], tg["labels"])
        rows.append((cropped, pcl.shape[0], c.shape[0]))
    print(f"collate: (rows after the crop, after the down-sampling, voxels) {rows}, {[int(t['bbox3d'].shape[0]) for t in tgs]} boxes")
    assert points[2] == 2 and len(tgs) == 2
    assert torch.equal(points[0], torch.cat(coords)) and torch.equal(points[1], torch.cat(feats))


def test_pipeline_with_every_option_is_the_steps_in_order(tiny, dev):
    from detection_3d_amd.downsample import apply_downsample, downsample_kwargs, voxel_downsample
    from detection_3d_amd.normals import with_normals
    from detection_3d_amd.serving import BuildingPipeline
    from detection_3d_amd.unproject import DepthFrames, suncg_cameras, unproject
    cfg, model = tiny
    depth, cams = rendered_room()
    intr, extr = suncg_cameras(cams, depth.shape[1], depth.shape[2])
    color = np.random.RandomState(9).randint(0, 256, depth.shape + (3,)).astype(np.uint8)
    frames = DepthFrames(torch.from_numpy(depth).to(dev), intr, extr, color=torch.from_numpy(color).to(dev))
    kw = {"edge": 0.1, "min_depth": 1.7}
    raw, pixels = unproject(frames, return_pixels=True, **kw)
    voxels = voxel_downsample(raw, 0.05).shape[0]
    assert 0 < voxels < raw.shape[0] < depth.size
    dkw = {"voxel": 0.05, "max_points": voxels // 2, "seed": 4}
    with torch.no_grad():
        got = BuildingPipeline(model, cfg, in_flight=2, device=dev, unproject=kw, downsample=dkw, normals="estimate",
                               point_owner=True).map([frames])[0]
        small, source = apply_downsample(raw, downsample_kwargs(dkw), return_source=True)
        assert small.shape[0] == voxels // 2 and source.shape == (raw.shape[0],) and bool((source < 0).any())
        want = BuildingPipeline(model, cfg, in_flight=2, device=dev, point_owner=True).map([with_normals(small)])[0]
    torch.cuda.synchronize()
    owner = torch.cat([want["point_owner"], torch.full((1,), -1, dtype=torch.int32, device=dev)])[source.long()]
    want = dict(want, point_owner=owner, point_pixel=pixels)
    print(f"pipeline: {raw.shape[0]} pixels -> {small.shape[0]} points -> {want['bbox3d'].shape[0]} detections, "
          f"{int((owner >= 0).sum())} rows owned")
    assert set(got) == set(want) == {"bbox3d", "scores", "labels", "point_owner", "point_count", "point_pixel"}
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    assert want["bbox3d"].shape[0] > 0 and bool((owner >= 0).any())
