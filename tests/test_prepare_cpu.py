"""detection_3d_amd.prepare without a GPU: the order of the steps with recording fakes in their places, the keyword
checks, the frame rule and the ownership lookup on hand-made tensors."""
import itertools
from types import SimpleNamespace

import pytest
import torch

from detection_3d_amd import prepare
from detection_3d_amd.prepare import Kept, Preparation, point_ownership
from detection_3d_amd.primitives import RandomCrop
from detection_3d_amd.unproject import DepthFrames

CFG = SimpleNamespace(SPARSE3D=SimpleNamespace(VOXEL_SCALE=50), INPUT=SimpleNamespace(CLASSES=["wall"]))
OPTIONS = {"crop": (4, 4), "downsample": {"voxel": 0.05, "max_points": 9}, "normals": "estimate", "augment": True}


class _Crop(RandomCrop):
    def __init__(self, calls, seed=0):
        super().__init__((4, 4), seed)
        self.calls = calls

    def for_rank(self, rank):
        return _Crop(self.calls, self.seed + 1000003 * rank)

    def __call__(self, pcl, tg):
        self.calls.append(("crop", self.seed))
        return pcl + 1, dict(tg, cropped=True)


class _Augment(object):
    def __init__(self, calls, seed=0):
        self.calls, self.seed = calls, seed

    def for_rank(self, rank):
        return _Augment(self.calls, self.seed + 1000003 * rank)

    def check_classes(self, classes):
        self.calls.append(("check_classes", list(classes)))

    def __call__(self, pcl, tg, cfg):
        self.calls.append(("augment", self.seed, pcl.shape[1]))
        return "coords", "feats", dict(tg, augmented=True)


def _chain(monkeypatch, calls, crop=None, downsample=None, normals=None, augment=None, unproject=None):
    """a chain whose every step records its call and passes a cloud on that shows which steps it went through"""
    def fake_unproject(frames, return_pixels=False, **kw):
        calls.append(("unproject", return_pixels, kw))
        return (torch.zeros((5, 3)), "pixels") if return_pixels else torch.zeros((5, 3))

    def fake_downsample(pcl, dkw, return_source=False):
        if dkw is None:                      # what apply_downsample does without the option: nothing
            return (pcl, None) if return_source else pcl
        calls.append(("downsample", dkw, return_source))
        return (pcl[:4], "source") if return_source else pcl[:4]

    def fake_voxelize(pcl, cfg):
        calls.append(("voxelize", tuple(pcl.shape)))
        return "coords", "feats"

    def fake_shift(pcl, tg, scale):
        calls.append(("shift_targets", tuple(pcl.shape), scale))
        return dict(tg, shifted=True)

    def fake_estimator(xyz, radius, max_nn, orient):
        calls.append(("normals", xyz.shape[0]))
        return torch.ones((xyz.shape[0], 3))

    monkeypatch.setattr(prepare, "unproject", fake_unproject)
    monkeypatch.setattr(prepare, "apply_downsample", fake_downsample)
    monkeypatch.setattr(prepare, "shift_targets", fake_shift)
    chain = Preparation(unproject=unproject, crop=_Crop(calls) if crop else None, downsample=downsample, normals=normals,
                        augment=_Augment(calls) if augment else None, voxelize_fn=fake_voxelize)
    if chain.normals is not None:
        chain.normals["estimator"] = fake_estimator
    return chain


def _names(calls):
    return [c[0] for c in calls]


def test_training_side_every_option_on(monkeypatch):
    calls = []
    chain = _chain(monkeypatch, calls, **OPTIONS).for_rank(2, CFG.INPUT.CLASSES)
    assert calls == [("check_classes", ["wall"])]
    del calls[:]
    out = chain.scene(torch.zeros((6, 3)), {"bbox3d": "b"}, CFG)
    assert _names(calls) == ["crop", "downsample", "normals", "augment"]
    assert calls[0] == ("crop", 2000006) and calls[3] == ("augment", 2000006, 9)      # the rank's draws; nine columns
    assert calls[1] == ("downsample", {"voxel": 0.05, "max_points": 9, "seed": 0}, False) and calls[2] == ("normals", 4)
    assert out == ("coords", "feats", {"bbox3d": "b", "cropped": True, "augmented": True})


def test_every_option_off_touches_nothing(monkeypatch):
    calls = []
    pcl, tg = torch.zeros((6, 3)), {"bbox3d": "b"}
    assert Preparation().cloud(pcl) == (pcl, None) and Preparation().cloud(pcl)[0] is pcl        # the real steps
    chain = _chain(monkeypatch, calls)
    for keep in (False, True):
        cloud, kept = chain.cloud(pcl, keep=keep)
        assert cloud is pcl and calls == []
        assert kept == (Kept(None, None, None) if keep else None)
    coords, feats, out = chain.scene(pcl, tg, CFG)
    assert out is tg and calls == [("voxelize", (6, 3))]
    rank = chain.for_rank(3, CFG.INPUT.CLASSES)
    assert (rank.crop, rank.downsample, rank.normals, rank.augment) == (None, None, None, None) and len(calls) == 1


@pytest.mark.parametrize("option,want", [
    ("crop", ["crop", "voxelize", "shift_targets"]),
    ("downsample", ["downsample", "voxelize", "shift_targets"]),
    ("normals", ["normals", "voxelize"]),
    ("augment", ["augment"]),
])
def test_training_side_each_option_alone(monkeypatch, option, want):
    calls = []
    chain = _chain(monkeypatch, calls, **{option: OPTIONS[option]})
    _, _, tg = chain.scene(torch.zeros((6, 3)), {"bbox3d": "b"}, CFG)
    assert _names(calls) == want
    assert tg.get("shifted", False) == ("shift_targets" in want) and tg.get("augmented", False) == (option == "augment")
    if "shift_targets" in want:             # by the minimum of the cloud that was voxelised, at the config's scale
        assert calls[-1] == ("shift_targets", calls[-2][1], 50)


def test_serving_side(monkeypatch):
    frames = object.__new__(DepthFrames)
    calls = []
    chain = _chain(monkeypatch, calls, unproject={"step": 2}, downsample=0.05, normals={"radius": 0.2})
    cloud, kept = chain.cloud(frames, keep=True)
    assert calls == [("unproject", True, {"step": 2}), ("downsample", {"voxel": 0.05, "seed": 0}, True), ("normals", 4)]
    assert cloud.shape == (4, 9) and kept.cloud.shape == (4, 3) and (kept.source, kept.pixels) == ("source", "pixels")
    del calls[:]
    cloud, kept = chain.cloud(frames)
    assert _names(calls) == ["unproject", "downsample", "normals"] and calls[0][1] is False and calls[1][2] is False
    assert cloud.shape == (4, 9) and kept is None
    # each option alone; a cloud is never unprojected, frames always are
    for option, on_cloud in (("unproject", []), ("downsample", ["downsample"]), ("normals", ["normals"])):
        on_frames = ["unproject"] + on_cloud
        for raw, want in ((torch.zeros((6, 3)), on_cloud), (frames, on_frames)):
            del calls[:]
            value = {"step": 2} if option == "unproject" else OPTIONS[option]
            cloud, kept = _chain(monkeypatch, calls, **{option: value}).cloud(raw, keep=True)
            assert _names(calls) == want
            if option == "unproject" and raw is not frames:
                assert cloud is raw and kept == Kept(None, None, None)
            elif option != "downsample":     # frames and nothing down-sampled: the unprojected cloud is what the tail needs
                assert kept.source is None and (kept.cloud is None) == (raw is not frames)
                assert (kept.pixels == "pixels") == (raw is frames)


def test_bad_keywords_raise_before_the_config_is_touched():
    from detection_3d_amd import engine
    from detection_3d_amd.serving import BuildingPipeline
    bad = [{"unproject": {"voxel": 1}}, {"unproject": "estimate"}, {"crop": (1.0,)}, {"crop": "4"},
           {"downsample": {"size": 1}}, {"downsample": -1.0}, {"normals": "maybe"}, {"normals": {"max_nn": 2}}]
    for kw in bad:
        with pytest.raises(ValueError):
            Preparation(**kw)
        (name, value), = kw.items()
        if name != "unproject":
            with pytest.raises(ValueError):
                engine.collate([((), {})], None, **kw)
            with pytest.raises(ValueError):
                engine.train(None, None, [], None, 1, **kw)
        if name in ("downsample", "normals"):
            with pytest.raises(ValueError):
                engine.inference(None, None, [], None, **kw)
        if name != "crop":
            with pytest.raises(ValueError):
                BuildingPipeline(None, None, device="cpu", **kw)


def test_targets_in_file_frame_exactly_with_crop_downsample_or_augment():
    values = {"crop": (4, 4), "downsample": 0.05, "augment": _Augment([]), "normals": "estimate", "unproject": {"step": 2}}
    for on in itertools.product((False, True), repeat=len(values)):
        kw = {k: v for (k, v), flag in zip(values.items(), on) if flag}
        assert Preparation(**kw).targets_in_file_frame == any(k in kw for k in ("crop", "downsample", "augment")), kw


def test_point_ownership_lookup(monkeypatch):
    owner = torch.tensor([2, -1, 0, 1], dtype=torch.int32)
    count = torch.tensor([1, 1, 1], dtype=torch.int32)
    seen = []

    def fake(xyz, boxes, origin=None):
        seen.append((xyz, boxes.dtype, origin))
        return owner, count, None, None

    monkeypatch.setattr(prepare, "points_in_boxes", fake)
    raw, reduced, boxes = torch.zeros((7, 3)), torch.zeros((4, 3)), torch.zeros((3, 7), dtype=torch.float64)
    got, cnt = point_ownership(Kept(None, None, None), raw, boxes)
    assert got is owner and cnt is count and seen[-1][0] is raw and seen[-1][1:] == (torch.float32, "min")
    source = torch.tensor([3, -1, 0, 0, 1, -1, 2], dtype=torch.int32)
    got, cnt = point_ownership(Kept(reduced, source, None), raw, boxes)
    assert seen[-1][0] is reduced and cnt is count
    assert got.dtype == torch.int32 and got.tolist() == [1, -1, 2, 2, -1, -1, 0]
    got, _ = point_ownership(Kept(reduced, None, "pixels"), raw, boxes)          # unprojected, nothing down-sampled
    assert got is owner and seen[-1][0] is reduced
