"""detection_3d_amd.primitives without a GPU: the fp64 reference's own doubtful share on the test scenes, and the
plain-torch parts (crop_boxes, point_lists, random_window, argument checks)."""
import math
import warnings

import numpy as np
import pytest
import torch

from tests.points_ref import DOUBTFUL_CAP, points_in_boxes_ref, scene


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("grow", [(0.0, 0.0), (0.3, 0.3)])
def test_reference_scenes_have_few_doubtful_points(seed, grow):
    xyz, boxes = scene(seed)
    ref = points_in_boxes_ref(xyz, boxes, grow)
    share = ref["doubtful"].mean()
    inside = (ref["owner"] >= 0).mean()
    print(f"seed {seed} grow {grow}: doubtful {int(ref['doubtful'].sum())} of {len(xyz)}, inside {inside:.3f}, "
          f"min members {int(ref['count'].min())}")
    assert share <= DOUBTFUL_CAP
    assert 0.15 < inside < 0.6                  # the scene exercises both answers
    assert ref["count"].min() > 0


def _wall(yaw, d4=4.0):
    return torch.tensor([[10.0, 5.0, 0.1, 0.2, d4, 2.5, yaw]], dtype=torch.float32)


def _stats(count, lo_y, hi_y):
    k = len(count)
    lo = torch.zeros((k, 3), dtype=torch.float32)
    hi = torch.zeros((k, 3), dtype=torch.float32)
    lo[:, 1], hi[:, 1] = torch.tensor(lo_y), torch.tensor(hi_y)
    lo[:, 0], hi[:, 0], hi[:, 2] = -0.15, 0.15, 2.5
    return torch.tensor(count, dtype=torch.int32), lo, hi


@pytest.mark.parametrize("yaw", [0.0, math.pi / 4])
def test_crop_boxes_shortens_a_wall_to_its_points(yaw):
    from detection_3d_amd.primitives import crop_boxes
    boxes = _wall(yaw)
    out, keep = crop_boxes(boxes, *_stats([500], [-1.0], [0.5]))
    assert keep.tolist() == [True] and out.dtype == boxes.dtype
    assert abs(float(out[0, 4]) - 1.5) < 1e-6
    # the centre moves by the midpoint -0.25 along the length direction (sin yaw, cos yaw)
    assert abs(float(out[0, 0]) - (10.0 + math.sin(yaw) * -0.25)) < 1e-5
    assert abs(float(out[0, 1]) - (5.0 + math.cos(yaw) * -0.25)) < 1e-5
    assert torch.equal(out[0, [2, 3, 5, 6]], boxes[0, [2, 3, 5, 6]])


def test_crop_boxes_drop_rules_and_clipping():
    from detection_3d_amd.primitives import crop_boxes
    boxes = _wall(0.0).repeat(6, 1)
    boxes[4, 4], boxes[4, 5] = 0.5, 1.0          # 10 d4 dz = 5: the count < 10 rule decides
    #                 many     few (<= min(10*4*2.5, 200) = 100)  short   beyond   small box, 9 pts   exactly at need
    count, lo, hi = _stats([500, 100, 500, 500, 9, 101], [-1.0, -1.0, 0.3, -7.0, -0.25, -2.0], [0.5, 0.5, 0.5, 9.0, 0.25, 2.0])
    out, keep = crop_boxes(boxes, count, lo, hi)
    assert keep.tolist() == [True, False, False, True, False, True]
    assert torch.equal(out[3], boxes[3])                                  # extents beyond the box are clipped to it
    assert torch.equal(out[1], boxes[1]) and torch.equal(out[2], boxes[2])  # dropped rows hold the input box
    # min_points overrides the area rule; min_length is a strict bound
    _, keep = crop_boxes(boxes, count, lo, hi, min_points=50)
    assert keep.tolist() == [True, True, False, True, False, True]
    _, keep = crop_boxes(boxes, count, lo, hi, min_length=1.5)
    assert keep.tolist() == [False, False, False, True, False, True]
    _, keep = crop_boxes(boxes, count, lo, hi, min_length=0.1)
    assert keep.tolist() == [True, False, True, True, False, True]


def test_crop_boxes_empty_boxes_without_warnings_or_nan():
    from detection_3d_amd.primitives import crop_boxes
    boxes = _wall(0.3).repeat(2, 1)
    count = torch.tensor([0, 500], dtype=torch.int32)
    lo = torch.tensor([[math.inf] * 3, [-0.1, -1.0, 0.0]], dtype=torch.float32)
    hi = torch.tensor([[-math.inf] * 3, [0.1, 1.0, 2.0]], dtype=torch.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out, keep = crop_boxes(boxes, count, lo, hi)
    assert keep.tolist() == [False, True]
    assert torch.isfinite(out).all() and torch.equal(out[0], boxes[0])
    out0, keep0 = crop_boxes(boxes[:0], count[:0], lo[:0], hi[:0])
    assert out0.shape == (0, 7) and keep0.shape == (0,)


def test_point_lists_are_grouped_by_box_in_point_order():
    from detection_3d_amd.primitives import point_lists
    owner = torch.tensor([2, -1, 0, 2, 0, -1, 3, 0], dtype=torch.int32)
    offsets, index = point_lists(owner, 5)
    assert offsets.dtype == torch.int64 and index.dtype == torch.int64
    assert offsets.tolist() == [0, 3, 3, 5, 6, 6]
    assert index.tolist() == [2, 4, 7, 0, 3, 6]
    offsets, index = point_lists(torch.zeros(0, dtype=torch.int32), 2)
    assert offsets.tolist() == [0, 0, 0] and index.numel() == 0
    offsets, index = point_lists(torch.full((4,), -1, dtype=torch.int32), 0)
    assert offsets.tolist() == [0] and index.numel() == 0


def test_random_window_stays_inside_the_extent():
    from detection_3d_amd.primitives import random_window
    rng = np.random.RandomState(0)
    pcl = torch.from_numpy((rng.rand(1000, 3) * [25.0, 3.0, 2.7] + [-4.0, 7.0, 0.0]).astype(np.float32))
    lo, hi = pcl[:, :2].amin(0), pcl[:, :2].amax(0)
    gen = torch.Generator().manual_seed(5)
    starts = set()
    for _ in range(50):
        x0, y0, x1, y1 = random_window(pcl, (6.0, 4.0), gen)
        assert float(lo[0]) <= x0 and x1 <= float(hi[0]) and abs((x1 - x0) - 6.0) < 1e-9
        # the cloud is 3 m deep, the window 4 m: the whole extent, half open, so one float32 step above the maximum
        assert y0 == float(lo[1]) and y1 == float(torch.nextafter(hi[1], torch.tensor(math.inf)))
        assert bool(((pcl[:, 1] >= y0) & (pcl[:, 1] < y1)).all())
        starts.add(round(x0, 6))
    assert len(starts) > 40
    a = random_window(pcl, (6.0, 4.0), torch.Generator().manual_seed(9))
    b = random_window(pcl, (6.0, 4.0), torch.Generator().manual_seed(9))
    assert a == b


def test_argument_validation():
    from detection_3d_amd import primitives as P
    boxes, (count, lo, hi) = _wall(0.0), _stats([500], [-1.0], [0.5])
    with pytest.raises(ValueError):
        P.crop_boxes(boxes[:, :6], count, lo, hi)
    with pytest.raises(ValueError):
        P.crop_boxes(boxes, count, lo[:, :2], hi)
    with pytest.raises(ValueError):
        P.crop_boxes(boxes, count, lo, hi, min_points=-1)
    with pytest.raises(ValueError):
        P.crop_boxes(boxes, count, lo, hi, min_length=-0.1)
    with pytest.raises(ValueError):
        P.point_lists(torch.tensor([0, 3]), 3)
    with pytest.raises(ValueError):
        P.point_lists(torch.tensor([0.0, 1.0]), 3)
    with pytest.raises(ValueError):
        P.point_lists(torch.tensor([0, 1]), -1)
    with pytest.raises(ValueError):
        P.random_window(torch.zeros(4, 3), (0.0, 1.0))
    with pytest.raises(ValueError):
        P.random_window(torch.zeros(0, 3), (1.0, 1.0))
    xyz = torch.zeros(4, 3)
    for bad in [dict(grow=(0.1,)), dict(grow=(-0.1, 0.0)), dict(grow=(0.0, math.inf)), dict(grow=0.3)]:
        with pytest.raises(ValueError):
            P.points_in_boxes(xyz, boxes, **bad)
    with pytest.raises(ValueError):
        P.points_in_boxes(xyz[:, :2], boxes)
    with pytest.raises(ValueError):
        P.points_in_boxes(xyz, boxes[:, :5])
    with pytest.raises(ValueError):
        P.crop_scene(xyz, {"bbox3d": boxes, "labels": torch.ones(1)}, (0.0, 0.0, 0.0, 1.0))
    for bad in [(1.0,), (1.0, -2.0), "4", (1.0, 2.0, 3.0)]:
        with pytest.raises(ValueError):
            P.as_crop(bad)
    with pytest.raises(ValueError):
        P.parse_crop("4")
    assert P.as_crop(None) is None and P.parse_crop("") is None
    assert P.as_crop((4, 4)) is P.as_crop((4.0, 4.0)) and P.parse_crop("4,3", seed=2).size_xy == (4.0, 3.0)
    assert P.RandomCrop((4, 4), seed=1).for_rank(2).seed == 1 + 2 * 1000003


def test_points_in_boxes_refuses_cpu_tensors():
    from detection_3d_amd._lib import D3DError
    from detection_3d_amd.primitives import crop_scene, points_in_boxes
    with pytest.raises(D3DError):
        points_in_boxes(torch.zeros(4, 3), _wall(0.0))
    with pytest.raises(D3DError):
        crop_scene(torch.zeros(4, 3), {"bbox3d": _wall(0.0), "labels": torch.ones(1)}, (0.0, 0.0, 1.0, 1.0))


def test_the_loops_take_crop():
    import inspect
    from detection_3d_amd import engine
    assert inspect.signature(engine.collate).parameters["crop"].default is None
    assert inspect.signature(engine.train).parameters["crop"].default is None
