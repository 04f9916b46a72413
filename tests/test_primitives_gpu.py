"""d3d_points_in_boxes on the GPU against the fp64 restatement of tests/points_ref.py, and its plumbing through
primitives.crop_scene, serving.BuildingPipeline(point_owner=True) and engine.collate(crop=...)."""
import math

import numpy as np
import pytest
import torch

from tests.points_ref import lattice_case, points_in_boxes_ref, room_scene, sampled_wall, scene

pytestmark = pytest.mark.gpu

_CACHE = {}


def _case(seed, n, k, grow):
    """scene and reference, computed once per case and shared (nothing modifies them)"""
    key = (seed, n, k, grow)
    if key not in _CACHE:
        xyz, boxes = scene(seed, n, k)
        _CACHE[key] = (xyz, boxes, points_in_boxes_ref(xyz, boxes, grow))
    return _CACHE[key]


def _run(dev, xyz, boxes, **kw):
    from detection_3d_amd.primitives import points_in_boxes
    out = points_in_boxes(torch.as_tensor(xyz).to(dev), torch.as_tensor(boxes).to(dev), **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _check(got, ref, what):
    owner, count, lo, hi = got
    sure = ~ref["doubtful"]
    print(f"{what}: {int(ref['doubtful'].sum())} doubtful of {len(sure)} points, "
          f"{int((owner[sure] != ref['owner'][sure]).sum())} owners differ, "
          f"count - certain in [{int((count - ref['count_certain']).min(initial=0))}, "
          f"{int((count - ref['count_certain']).max(initial=0))}]")
    assert owner.dtype == np.int32 and count.dtype == np.int32 and lo.dtype == np.float32 and hi.dtype == np.float32
    assert np.array_equal(owner[sure], ref["owner"][sure]), what
    assert (count >= ref["count_certain"]).all() and (count <= ref["count_possible"]).all(), what
    # an extent lies between that of the certain members and that of every possible member, widened by 1e-4 m; a box
    # without certain members may be empty (+inf / -inf)
    assert (lo >= ref["lo_out"] - 1e-4).all() and (lo <= ref["lo_in"] + 1e-4).all(), what
    assert (hi <= ref["hi_out"] + 1e-4).all() and (hi >= ref["hi_in"] - 1e-4).all(), what


@pytest.mark.parametrize("grow", [(0.0, 0.0), (0.5, 2.0)])
def test_exact_on_a_lattice_closed_faces_and_grow(dev, grow):
    xyz, boxes = lattice_case(grow)
    ref = points_in_boxes_ref(xyz, boxes, grow)
    assert ref["count"][3] == 0 and (ref["count"][:3] >= 125).all()
    owner, count, lo, hi = _run(dev, xyz, boxes, grow=grow)
    assert np.array_equal(owner, ref["owner"])
    assert np.array_equal(count, ref["count"])
    for got, want in ((lo, ref["lo"]), (hi, ref["hi"])):
        assert np.array_equal(got.view(np.int32), want.astype(np.float32).view(np.int32))
    assert np.isposinf(lo[3]).all() and np.isneginf(hi[3]).all() and count[3] == 0      # the box without members


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("grow", [(0.0, 0.0), (0.3, 0.3)])
def test_random_scene_matches_where_not_doubtful(dev, seed, grow):
    xyz, boxes, ref = _case(seed, 20000, 48, grow)
    assert ref["doubtful"].mean() <= 0.0025
    _check(_run(dev, xyz, boxes, grow=grow), ref, f"seed {seed} grow {grow}")


@pytest.mark.parametrize("n,k", [(0, 48), (1, 48), (63, 48), (64, 48), (65, 48), (20000, 0), (20000, 1), (5000, 600),
                                 (0, 0)])
def test_sizes(dev, n, k):
    xyz, boxes, ref = _case(2, n, k, (0.0, 0.0))
    got = _run(dev, xyz, boxes)
    assert got[0].shape == (n,) and got[1].shape == (k,) and got[2].shape == (k, 3) and got[3].shape == (k, 3)
    _check(got, ref, f"n {n} k {k}")
    if n == 0:
        assert (got[1] == 0).all() and np.isposinf(got[2]).all() and np.isneginf(got[3]).all()
    if k == 0:
        assert (got[0] == -1).all()


def test_stride_nan_origin_and_reproducibility(dev):
    from detection_3d_amd.primitives import points_in_boxes
    xyz, boxes, _ = _case(0, 20000, 48, (0.0, 0.0))
    rng = np.random.RandomState(7)
    cloud9 = torch.from_numpy(np.concatenate([xyz, rng.rand(len(xyz), 6).astype(np.float32)], 1)).to(dev)
    b = torch.from_numpy(boxes).to(dev)
    want = points_in_boxes(cloud9[:, :3].contiguous(), b)
    for view in (cloud9, cloud9[:, :3]):                   # read in place through the row stride
        got = points_in_boxes(view, b)
        assert all(torch.equal(g, w) for g, w in zip(got, want))
    again = points_in_boxes(cloud9, b)
    assert all(torch.equal(g.view(torch.int32), w.view(torch.int32)) for g, w in zip(again, want))

    # a NaN row belongs to nothing and leaves every other answer alone
    inside = int(torch.nonzero(want[0] >= 0)[0])
    holed = cloud9.clone()
    holed[inside, 1] = float("nan")
    got = points_in_boxes(holed, b)
    assert int(got[0][inside]) == -1
    keep = torch.arange(len(xyz), device=dev) != inside
    assert torch.equal(got[0][keep], want[0][keep])
    assert int((want[1] - got[1]).sum()) >= 1 and bool((got[1] <= want[1]).all())

    # origin='min' is the fp64 minimum subtracted by hand; a vector origin is taken as given
    shift = torch.tensor([300.0, -41.5, 0.0], dtype=torch.float64, device=dev)
    far = (cloud9[:, :3].double() + shift).float()
    mn = far.double().amin(0)
    by_hand = (far.double() - mn).float()
    bm = b.clone()
    bm[:, :3] = (b[:, :3].double() + shift - mn).float()
    want_m = points_in_boxes(by_hand, bm, grow=(0.3, 0.3))
    for origin in ("min", mn, mn.cpu().tolist()):
        got_m = points_in_boxes(far, bm, grow=(0.3, 0.3), origin=origin)
        assert all(torch.equal(g.view(torch.int32), w.view(torch.int32)) for g, w in zip(got_m, want_m))
    assert int((want_m[0] >= 0).sum()) > 5000


def test_too_many_boxes_and_wrong_devices(dev):
    from detection_3d_amd._lib import D3DError, check, lib, ptr, stream_of
    from detection_3d_amd.primitives import points_in_boxes
    xyz = torch.zeros((8, 3), device=dev)
    with pytest.raises(ValueError):
        points_in_boxes(xyz, torch.zeros((4097, 7), device=dev))
    with pytest.raises(D3DError):
        points_in_boxes(xyz, torch.zeros((2, 7)))
    owner = torch.empty(8, dtype=torch.int32, device=dev)
    for n, stride, k in ((-1, 3, 0), (8, 2, 0), (8, 3, 4097), (8, 3, -1)):
        with pytest.raises(D3DError):
            check(lib().d3d_points_in_boxes(ptr(xyz), n, stride, None, ptr(xyz), k, 0.0, 0.0, ptr(owner), ptr(owner),
                                            ptr(xyz), ptr(xyz), stream_of(dev)))


def test_point_lists_of_a_gpu_result(dev):
    from detection_3d_amd.primitives import point_lists, points_in_boxes
    xyz, boxes, ref = _case(0, 20000, 48, (0.0, 0.0))
    owner = points_in_boxes(torch.from_numpy(xyz).to(dev), torch.from_numpy(boxes).to(dev))[0]
    offsets, index = point_lists(owner, 48)
    own = owner.cpu().numpy()
    offsets, index = offsets.cpu().numpy(), index.cpu().numpy()
    for b in range(48):
        assert np.array_equal(index[offsets[b]:offsets[b + 1]], np.nonzero(own == b)[0])
    assert offsets[-1] == (own >= 0).sum()


def test_crop_scene_cuts_a_wall_and_drops_the_box_outside(dev):
    from detection_3d_amd.primitives import crop_scene
    boxes = np.array([[5.0, 3.0, 0.0, 0.2, 10.0, 2.6, math.pi / 2],       # a 10 m wall along x, x in [0, 10]
                      [8.0, 7.0, 0.0, 0.2, 3.0, 2.6, math.pi / 2],        # wholly outside the window
                      [2.0, 6.5, 0.0, 0.2, 3.0, 2.6, 0.0]], np.float32)   # along y, wholly inside
    xyz = np.concatenate([sampled_wall(b) for b in boxes]).astype(np.float32)
    rng = np.random.RandomState(0)
    pcl = np.zeros((len(xyz), 9), np.float32)
    pcl[:, :3] = xyz[rng.permutation(len(xyz))]
    pcl[:, 3] = np.arange(len(xyz))                          # a tag that shows the order of the rows that remain
    window = (-1.0, 0.0, 4.0, 10.0)
    mask = (pcl[:, 0] >= -1.0) & (pcl[:, 0] < 4.0) & (pcl[:, 1] >= 0.0) & (pcl[:, 1] < 10.0)
    tg = {"bbox3d": torch.from_numpy(boxes), "labels": torch.tensor([1, 2, 3])}
    out, tg2 = crop_scene(torch.from_numpy(pcl).to(dev), tg, window)
    assert out.shape == (int(mask.sum()), 9) and np.array_equal(out.cpu().numpy(), pcl[mask])
    got = tg2["bbox3d"]
    assert got.device == tg["bbox3d"].device and got.dtype == torch.float32
    assert tg2["labels"].tolist() == [1, 3]                  # labels follow the boxes
    wall, inner = got[0].numpy(), got[1].numpy()
    assert abs(wall[4] - 4.0) <= 0.05 and abs(wall[0] - 2.0) <= 0.03 and abs(wall[1] - 3.0) <= 1e-5
    assert np.array_equal(wall[[2, 3, 5, 6]], boxes[0, [2, 3, 5, 6]])
    assert np.allclose(inner, boxes[2], atol=1e-5)
    # targets on the device stay there
    _, tg3 = crop_scene(torch.from_numpy(pcl).to(dev), {k: v.to(dev) for k, v in tg.items()}, window)
    assert tg3["bbox3d"].is_cuda and torch.equal(tg3["bbox3d"].cpu(), got) and tg3["labels"].tolist() == [1, 3]


@pytest.fixture(scope="module")
def tiny(dev):
    """the model and scene of tests/test_detector_gpu.py"""
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.detector import build_detection_model
    from detection_3d_amd.synthetic import make_scene as make_building
    cfg = get_cfg("4c_Fpn432")
    torch.manual_seed(1)
    model = build_detection_model(cfg).to(dev).eval()
    with torch.no_grad():
        model.rpn.head.cls_logits.weight.mul_(60)
        model.rpn.head.bbox_pred.weight.mul_(20)
        model.roi_heads.box.predictor.cls_score.weight.mul_(40)
        model.roi_heads.box.predictor.bbox_pred.weight.mul_(100)
    return cfg, model, torch.from_numpy(make_building(3, 40000)).to(dev)


def test_pipeline_reports_point_owners(tiny, dev):
    from detection_3d_amd.primitives import points_in_boxes
    from detection_3d_amd.serving import BuildingPipeline
    cfg, model, cloud = tiny
    clouds = [cloud, cloud[:30000].contiguous()]
    with torch.no_grad():
        on = BuildingPipeline(model, cfg, in_flight=2, device=dev, point_owner=True).map(clouds)
        off = BuildingPipeline(model, cfg, in_flight=2, device=dev).map(clouds)
    torch.cuda.synchronize()
    for c, r, plain in zip(clouds, on, off):
        assert set(plain) == {"bbox3d", "scores", "labels"}
        assert set(r) == set(plain) | {"point_owner", "point_count"}
        assert all(torch.equal(r[k], plain[k]) for k in plain)
        assert r["bbox3d"].shape[0] > 0
        assert r["point_owner"].shape == (c.shape[0],) and r["point_owner"].dtype == torch.int32
        assert r["point_count"].shape == (r["bbox3d"].shape[0],) and r["point_count"].dtype == torch.int32
        owner, count, _, _ = points_in_boxes(c, r["bbox3d"], origin="min")
        assert torch.equal(r["point_owner"], owner) and torch.equal(r["point_count"], count)
        assert int(r["point_owner"].max()) < r["bbox3d"].shape[0]


def test_collate_crops_scenes_and_their_boxes(tiny, dev):
    from detection_3d_amd import engine
    from detection_3d_amd.primitives import RandomCrop, points_in_boxes
    cfg = tiny[0]
    scenes = []
    for seed in (0, 1):
        pcl, boxes, labels = room_scene(seed)
        scenes.append((torch.from_numpy(pcl).to(dev), {"bbox3d": torch.from_numpy(boxes), "labels": torch.from_numpy(labels)}))
    whole, _ = engine.collate(scenes, cfg)
    points, tgs = engine.collate(scenes, cfg, crop=(4, 4))
    assert points[2] == 2 and 0 < points[0].shape[0] < whole[0].shape[0]
    for b, tg in enumerate(tgs):
        rows = points[0][:, 3] == b
        assert 0 < int(rows.sum()) < int((whole[0][:, 3] == b).sum())
        xyz = points[1][rows][:, :3].contiguous()          # the voxelised cloud's metric coordinates: the targets' frame
        assert float(xyz.max()) <= 4.0 + 0.02 + 1e-3 and float(xyz.min()) >= 0.0
        boxes = tg["bbox3d"].to(dev)
        assert boxes.shape[0] == tg["labels"].shape[0] and 0 < boxes.shape[0] <= 5
        count = points_in_boxes(xyz, boxes, grow=(0.3, 0.3))[1]
        assert int(count.min()) > 10
        assert float(boxes[:, 4].max()) <= 4.0 + 0.05
    # the same seed draws the same windows; crop composes with augment's frame condition (targets in the file's frame)
    a, ta = engine.collate(scenes, cfg, crop=RandomCrop((4, 4), seed=3))
    b_, tb = engine.collate(scenes, cfg, crop=RandomCrop((4, 4), seed=3))
    assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1])
    assert all(torch.equal(x["bbox3d"], y["bbox3d"]) for x, y in zip(ta, tb))
