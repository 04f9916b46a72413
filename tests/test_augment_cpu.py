"""Host side of detection_3d_amd.augment (no GPU): parameter draws, the linear part, the boxes' transform against their
BEV corners, zero-yaw classes, and the numpy elastic oracle of tests/augment_ref.py against scipy's form of elastic()."""
import math

import numpy as np
import pytest
import torch

from tests import augment_ref as ref


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def test_same_seed_same_params_and_other_seed_differs():
    from detection_3d_amd.augment import Augment
    kw = dict(rotate="free", flip_x=True, scale_jitter=0.2, origin_offset=True, elastic=True, color_noise=0.05)
    a, b, c = Augment(seed=7, **kw), Augment(seed=7, **kw), Augment(seed=8, **kw)
    for _ in range(5):
        pa, pb, pc = a.sample_params(), b.sample_params(), c.sample_params()
        for x, y in zip(pa, pb):
            assert np.array_equal(np.asarray(x), np.asarray(y))
        assert pa.theta != pc.theta and not np.array_equal(pa.u1, pc.u1)
    assert a.for_rank(0).seed == 7 and a.for_rank(3).seed == 7 + 3 * 1000003


def test_ranges_quarter_angles_and_identity():
    from detection_3d_amd.augment import linear_part, normal_matrix, sample_params
    g = _gen(0)
    flips, ks = set(), set()
    for _ in range(400):
        p = sample_params(g, "quarter", True, 0.15, True, 0.1)
        flips.add(p.flip)
        ks.add(p.k)
        assert 0.85 <= p.scale <= 1.15
        assert p.k in (0, 1, 2, 3) and p.theta == p.k * (math.pi / 2)
        assert np.all((p.u1 >= 0) & (p.u1 < 1)) and np.all((p.u2 >= 0) & (p.u2 < 1))
        r = linear_part(p, 50)[:2, :2] / (p.scale * 50)
        assert set(np.abs(r).ravel().tolist()) <= {0.0, 1.0}          # exact quarter turns
    assert flips == {1.0, -1.0} and ks == {0, 1, 2, 3}
    for _ in range(200):
        p = sample_params(g, "free")
        assert 0 <= p.theta < 2 * math.pi and p.flip == 1.0 and p.scale == 1.0
    p = sample_params(g)                                               # all off
    assert p.flip == 1.0 and p.scale == 1.0 and p.theta == 0.0
    assert not p.u1.any() and not p.u2.any() and not p.color.any()
    assert np.array_equal(linear_part(p, 50), np.diag([50.0, 50.0, 50.0]))
    assert np.array_equal(normal_matrix(p), np.eye(3))
    with pytest.raises(ValueError):
        sample_params(g, "half")


def _in_box_transform(b, p, m, off, scale):
    """corners of b moved like points: (corner . m[:2, :2]) / scale + off / scale"""
    c = ref.bev_corners(b)
    moved = np.stack([(c[..., 0] * m[0, j] + c[..., 1] * m[1, j]) for j in range(2)], -1)
    return moved / scale + off[None, None, :2] / scale


@pytest.mark.parametrize("flip", [1.0, -1.0])
@pytest.mark.parametrize("rot", ["none", "q0", "q1", "q2", "q3", "free"])
@pytest.mark.parametrize("s", [1.0, 0.87, 1.13])
def test_box_corners_follow_the_points(flip, rot, s):
    from detection_3d_amd.augment import Params, linear_part, transform_boxes
    rng = np.random.RandomState(int(s * 100) + 7 * ["none", "q0", "q1", "q2", "q3", "free"].index(rot) + int(flip > 0))
    n = 64
    b = np.zeros((n, 7), np.float32)
    b[:, 0:2] = rng.rand(n, 2) * 25
    b[:, 2] = rng.rand(n)
    b[:, 3:6] = 0.1 + rng.rand(n, 3) * 4
    b[:, 6] = (rng.rand(n) - 0.5) * np.pi
    k = int(rot[1]) if rot.startswith("q") else (0 if rot == "none" else -1)
    theta = k * math.pi / 2 if k >= 0 else rng.rand() * 2 * math.pi
    p = Params(flip, s, k, theta, np.zeros(3), np.zeros(3), np.zeros(3), 0)
    m = linear_part(p, 50)
    off = np.array([1234.5, 987.25, 3.0])
    out = transform_boxes(b, np.zeros(n, bool), p, m, off, 50)
    assert out.dtype == np.float32
    assert np.all(out[:, 6] >= -np.float32(np.pi / 2)) and np.all(out[:, 6] < np.float32(np.pi / 2))
    got, want = ref.bev_corners(out), _in_box_transform(b, p, m, off, 50)
    for i in range(n):
        d = np.linalg.norm(got[i][:, None, :] - want[i][None, :, :], axis=-1)
        assert d.min(1).max() < 1e-5 and d.min(0).max() < 1e-5, (i, d)
    np.testing.assert_allclose(out[:, 3:6], b[:, 3:6] * s, rtol=1e-6)
    np.testing.assert_allclose(out[:, 2], (b[:, 2] * s * 50 + off[2]) / 50, rtol=1e-6)


def test_zero_yaw_classes_stay_zero_with_swapped_dims():
    from detection_3d_amd.augment import Augment, Params, linear_part, transform_boxes
    b = np.array([[3.0, 4.0, 0.0, 6.0, 2.0, 0.1, 0.0], [5.0, 1.0, 0.0, 8.0, 3.0, 0.1, 0.0]], np.float32)
    for k in range(4):
        p = Params(1.0, 1.0, k, k * math.pi / 2, np.zeros(3), np.zeros(3), np.zeros(3), 0)
        out = transform_boxes(b, np.array([True, True]), p, linear_part(p, 50), np.zeros(3), 50)
        assert np.all(out[:, 6] == 0)
        want = b[:, [4, 3]] if k % 2 else b[:, [3, 4]]
        assert np.array_equal(out[:, 3:5], want), (k, out)
    Augment(rotate="quarter").check_classes(["background", "wall", "ceiling", "floor"])
    Augment(rotate="free").check_classes(["background", "wall", "door", "window"])
    with pytest.raises(ValueError, match="zero-yaw"):
        Augment(rotate="free").check_classes(["background", "wall", "ceiling", "floor"])


def test_unaugmented_boxes_equal_scene_targets_bits():
    """identity parameters: the boxes in the file's frame, moved by the points' offset, are scene_targets' bits"""
    from detection_3d_amd.augment import Params, linear_part, transform_boxes
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.scene_io import scene_targets
    from detection_3d_amd.synthetic import make_scene, make_targets, yx_zb_to_standard
    cfg = get_cfg("4c_Fpn432")
    classes = cfg.INPUT.CLASSES
    pcl = make_scene(3, 20000)
    bx, lb = make_targets(3)
    std = {classes[int(l)]: yx_zb_to_standard(bx[lb == l]) for l in np.unique(lb)}
    want = scene_targets(pcl, std, classes, 50)
    raw = scene_targets(pcl, std, classes, 50, shift=False)
    p = Params(1.0, 1.0, 0, 0.0, np.zeros(3), np.zeros(3), np.zeros(3), 0)
    m = linear_part(p, 50)
    off = -ref.affine(pcl, m).min(0)
    got = transform_boxes(raw["bbox3d"], np.zeros(len(raw["labels"]), bool), p, m, off, 50)
    assert np.array_equal(got, want["bbox3d"]) and np.array_equal(raw["labels"], want["labels"])


def test_element_columns():
    from detection_3d_amd.augment import element_columns
    assert element_columns(["xyz", "color", "normal"]) == {"xyz": 0, "color": 3, "normal": 6}
    assert element_columns(["xyz", "normal"]) == {"xyz": 0, "normal": 3}


def test_elastic_oracle_equals_scipy_form():
    pytest.importorskip("scipy")
    from detection_3d_amd.augment import elastic_displace  # noqa: F401 -- the GPU pass this oracle checks
    rng = np.random.RandomState(0)
    a = (rng.rand(3000, 3) * np.array([900.0, 700.0, 130.0])) - np.array([20.0, 10.0, 5.0])
    for gran, mag in ((6, 40.0), (20, 160.0)):
        bb = ref.grid_dims(a, gran)
        raw = [rng.randn(*bb).astype(np.float32) for _ in range(3)]
        want, noise = ref.elastic_scipy(a, raw, gran, mag)
        blurred = [ref.blur(f) for f in raw]
        for x, y in zip(blurred, noise):
            assert y.dtype == np.float32 and np.array_equal(x.view(np.int32), y.view(np.int32))
        got = ref.elastic_pass(a, blurred, gran, mag)
        assert np.array_equal(got.view(np.int64), want.view(np.int64))
        # outside the grid: no displacement
        far = np.array([[1e6, 0.0, 0.0]])
        assert np.array_equal(ref.elastic_pass(far, blurred, gran, mag), far)
        a = got


def test_parse_augment_spec():
    from detection_3d_amd.augment import parse_augment
    assert parse_augment("") is None
    a = parse_augment("flip,rotate=quarter,scale=0.1,offset,elastic,color=0.02", seed=4)
    assert (a.flip_x, a.rotate, a.scale_jitter, a.origin_offset, a.elastic, a.color_noise, a.seed) == \
        (True, "quarter", 0.1, True, True, 0.02, 4)
    assert parse_augment("rotate").rotate == "free"
    with pytest.raises(ValueError):
        parse_augment("flip,mirror")
    with pytest.raises(ValueError):
        parse_augment("rotate=half")
