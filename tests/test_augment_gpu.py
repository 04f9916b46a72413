"""Augmentation on the MI355X (detection_3d_amd.augment, csrc/augment.hip) against the numpy oracle of tests/augment_ref.py:
identity = voxelize + scene_targets bit for bit; the affine path bit for bit; points in a box stay in the moved box; the
elastic blur and displacement; determinism; training with augmentation."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import augment_ref as ref

pytestmark = pytest.mark.gpu


def _cfg(name="4c_Fpn432"):
    from detection_3d_amd.config import get_cfg
    return get_cfg(name)


def _scene(seed, n, cfg):
    from detection_3d_amd.scene_io import scene_targets
    from detection_3d_amd.synthetic import make_scene, make_targets, yx_zb_to_standard
    classes = cfg.INPUT.CLASSES
    pcl = make_scene(seed, n)
    bx, lb = make_targets(seed)
    std = {classes[int(l)]: yx_zb_to_standard(bx[lb == l]) for l in np.unique(lb)}
    return pcl, std


def _fixed(aug, p):
    aug.sample_params = lambda: p
    return aug


def test_identity_equals_voxelize_and_scene_targets(dev):
    from detection_3d_amd.augment import Augment
    from detection_3d_amd.scene_io import scene_targets
    from detection_3d_amd.voxelize import voxelize
    cfg = _cfg()
    pcl, std = _scene(1, 300000, cfg)
    x = torch.from_numpy(pcl).to(dev)
    c0, f0 = voxelize(x, cfg.SPARSE3D.VOXEL_SCALE, cfg.SPARSE3D.VOXEL_FULL_SCALE)
    t0 = scene_targets(pcl, std, cfg.INPUT.CLASSES, cfg.SPARSE3D.VOXEL_SCALE)
    raw = scene_targets(pcl, std, cfg.INPUT.CLASSES, cfg.SPARSE3D.VOXEL_SCALE, shift=False)
    tg = {"bbox3d": torch.from_numpy(raw["bbox3d"]).to(dev), "labels": torch.from_numpy(raw["labels"]).to(dev)}
    c1, f1, t1 = Augment(seed=5)(x, tg, cfg)
    assert torch.equal(c0, c1) and torch.equal(f0.view(torch.int32), f1.view(torch.int32))
    assert np.array_equal(t1["bbox3d"].cpu().numpy(), t0["bbox3d"])
    assert np.array_equal(t1["labels"].cpu().numpy(), t0["labels"])


def test_affine_matches_oracle_bits(dev):
    from detection_3d_amd.augment import Augment, Params, linear_part, normal_matrix
    cfg = _cfg()
    pcl, _ = _scene(2, 500000, cfg)
    p = Params(-1.0, 1.0731, -1, 0.7321, np.array([0.3, 0.6, 0.1]), np.array([0.9, 0.2, 0.5]),
               np.array([0.013, -0.021, 0.004]), 0)
    aug = _fixed(Augment(rotate="free", flip_x=True, scale_jitter=0.1, origin_offset=True, color_noise=0.02), p)
    empty = {"bbox3d": torch.zeros((0, 7)), "labels": torch.zeros((0,), dtype=torch.int64)}
    c, f, _ = aug(torch.from_numpy(pcl).to(dev), empty, cfg)
    m, nrm = linear_part(p, 50), normal_matrix(p)
    wc, wf, _, keep = ref.augment_voxelize(pcl, m, 50, cfg.SPARSE3D.VOXEL_FULL_SCALE, nrm, p.color, p.u1, p.u2, 3, 6)
    assert keep.sum() > 0.99 * pcl.shape[0]
    assert np.array_equal(c.cpu().numpy(), wc)
    assert np.array_equal(f.cpu().numpy().view(np.int32), wf.view(np.int32))


def test_points_in_a_box_stay_in_the_moved_box(dev):
    from detection_3d_amd.augment import Augment
    from detection_3d_amd.synthetic import make_targets
    cfg = _cfg()
    rng = np.random.RandomState(4)
    bx, lb = make_targets(4)
    bx[:, 0:2] += 3.0                                           # keep every box away from the cloud's minimum
    per, margin = 400, 5e-4
    pts, owner = [], []
    for i, b in enumerate(bx):
        q = (rng.rand(per, 3) - 0.5) * (b[[3, 4, 5]] - 2 * margin)
        c, s = math.cos(b[6]), math.sin(b[6])
        x = q[:, 0] * c + q[:, 1] * s + b[0]                   # orc_bev_corners: R(-yaw)
        y = -q[:, 0] * s + q[:, 1] * c + b[1]
        z = q[:, 2] + b[2] + b[5] * 0.5
        pts.append(np.stack([x, y, z], 1))
        owner.append(np.full(per, i))
    clutter = rng.rand(20000, 3) * np.array([31.0, 25.0, 3.0])
    xyz = np.concatenate(pts + [clutter]).astype(np.float32)
    owner = np.concatenate(owner + [np.full(clutter.shape[0], -1)])
    pcl = np.concatenate([xyz, rng.rand(xyz.shape[0], 3), np.tile([[0, 0, 1]], (xyz.shape[0], 1))], 1).astype(np.float32)
    tg = {"bbox3d": torch.from_numpy(bx).to(dev), "labels": torch.from_numpy(lb).to(dev)}
    for seed in range(4):
        aug = Augment(rotate="free", flip_x=True, scale_jitter=0.2, origin_offset=True, seed=seed)
        coords, feats, out = aug(torch.from_numpy(pcl).to(dev), tg, cfg)
        assert coords.shape[0] == pcl.shape[0]                 # nothing dropped: rows are the input rows
        f = feats.cpu().numpy().astype(np.float64)
        ob = out["bbox3d"].cpu().numpy().astype(np.float64)
        for i, b in enumerate(ob):
            p = f[owner == i, 0:3]
            dx, dy = p[:, 0] - b[0], p[:, 1] - b[1]
            c, s = math.cos(b[6]), math.sin(b[6])
            qx, qy = c * dx - s * dy, s * dx + c * dy
            assert np.all(np.abs(qx) <= b[3] / 2) and np.all(np.abs(qy) <= b[4] / 2), (seed, i)
            assert np.all(p[:, 2] >= b[2]) and np.all(p[:, 2] <= b[2] + b[5]), (seed, i)


def test_elastic_blur_and_displacement_match_oracle(dev):
    from detection_3d_amd import _lib
    from detection_3d_amd.augment import Augment, Params, _params_struct, element_columns, linear_part
    cfg = _cfg()
    lib = _lib.lib()
    rng = np.random.RandomState(5)
    pcl, _ = _scene(5, 200000, cfg)
    p = Params(1.0, 0.95, -1, 1.1, np.zeros(3), np.zeros(3), np.zeros(3), 0)
    st, m = _params_struct(p, 50, element_columns(cfg.INPUT.ELEMENTS), 0.0)
    x = torch.from_numpy(pcl).to(dev)
    n = pcl.shape[0]
    scratch = torch.empty(lib.d3d_augment_scratch_bytes(n), dtype=torch.uint8, device=dev)
    pts = torch.empty((n, 3), dtype=torch.float64, device=dev)
    mm = (ctypes.c_double * 6)()
    _lib.check(lib.d3d_augment_transform(_lib.ptr(x), n, 9, ctypes.byref(st), _lib.ptr(pts), mm, _lib.ptr(scratch),
                                         scratch.numel(), _lib.stream_of()))
    a = ref.affine(pcl, m)
    assert np.array_equal(pts.cpu().numpy(), a)
    assert np.array_equal(np.array(mm[:]), np.concatenate([a.min(0), a.max(0)]))
    for gran, mag in ((6, 40.0), (20, 160.0)):
        bb = ref.grid_dims(a, gran)
        raw = rng.randn(3, *bb).astype(np.float32)
        fields = torch.from_numpy(raw).to(dev)
        tmp = torch.empty_like(fields)
        _lib.check(lib.d3d_elastic_blur(_lib.ptr(fields), 3, _lib.ints(bb), _lib.ptr(tmp), _lib.stream_of()))
        want_f = np.stack([ref.blur(f) for f in raw])
        assert np.array_equal(fields.cpu().numpy().view(np.int32), want_f.view(np.int32))      # the same fp64 operations
        _lib.check(lib.d3d_elastic_apply(_lib.ptr(pts), n, _lib.ptr(fields), _lib.ints(bb), float(gran), float(mag), mm,
                                         _lib.ptr(scratch), scratch.numel(), _lib.stream_of()))
        a = ref.elastic_pass(a, want_f, gran, mag)
        got = pts.cpu().numpy()
        assert np.array_equal(got.view(np.int64), a.view(np.int64))
        assert np.allclose(np.array(mm[:]), np.concatenate([got.min(0), got.max(0)]), rtol=0, atol=0)
        assert np.abs(got - ref.affine(pcl, m)).max() > 1.0                # the distortion moves points
    coords = torch.empty((n, 3), dtype=torch.int64, device=dev)
    feats = torch.empty((n, 9), dtype=torch.float32, device=dev)
    kept, off = ctypes.c_int(0), (ctypes.c_double * 3)()
    _lib.check(lib.d3d_augment_voxelize(_lib.ptr(x), n, 9, _lib.ptr(pts), ctypes.byref(st), 50.0,
                                        _lib.ints(cfg.SPARSE3D.VOXEL_FULL_SCALE), _lib.ptr(coords), _lib.ptr(feats),
                                        ctypes.byref(kept), off, _lib.ptr(scratch), scratch.numel(), _lib.stream_of()))
    wc, wf, woff, keep = ref.augment_voxelize(pcl, m, 50, cfg.SPARSE3D.VOXEL_FULL_SCALE, points=a)
    assert kept.value == wc.shape[0]
    assert np.array_equal(np.array(off[:]), woff)
    assert np.array_equal(coords[:kept.value].cpu().numpy(), wc)                 # every row
    assert np.array_equal(feats[:kept.value].cpu().numpy()[:, :3].view(np.int32), wf[:, :3].view(np.int32))
    np.testing.assert_allclose(feats[:kept.value].cpu().numpy()[:, :3], wf[:, :3], rtol=0, atol=1e-6)
    # the whole call with elastic on
    aug = Augment(rotate="quarter", flip_x=True, scale_jitter=0.1, origin_offset=True, elastic=True, color_noise=0.02)
    c2, f2, _ = aug(x, {"bbox3d": torch.zeros((0, 7)), "labels": torch.zeros((0,), dtype=torch.int64)}, cfg)
    assert c2.shape[0] > 0.95 * n and bool(torch.isfinite(f2).all())
    full = torch.tensor(cfg.SPARSE3D.VOXEL_FULL_SCALE, device=dev)
    assert bool((c2 >= 0).all()) and bool((c2 < full).all())


def test_same_seed_same_bits_other_seed_differs(dev):
    from detection_3d_amd.augment import Augment
    from detection_3d_amd.scene_io import scene_targets
    cfg = _cfg()
    pcl, std = _scene(6, 200000, cfg)
    raw = scene_targets(pcl, std, cfg.INPUT.CLASSES, 50, shift=False)
    tg = {"bbox3d": torch.from_numpy(raw["bbox3d"]).to(dev), "labels": torch.from_numpy(raw["labels"]).to(dev)}
    x = torch.from_numpy(pcl).to(dev)
    kw = dict(rotate="free", flip_x=True, scale_jitter=0.1, origin_offset=True, elastic=True, color_noise=0.02)
    outs = [Augment(seed=s, **kw)(x, tg, cfg) for s in (11, 11, 12)]
    (ca, fa, ta), (cb, fb, tb), (cc, fc, tc) = outs
    assert torch.equal(ca, cb) and torch.equal(fa.view(torch.int32), fb.view(torch.int32))
    assert torch.equal(ta["bbox3d"], tb["bbox3d"])
    assert ca.shape != cc.shape or not torch.equal(ca, cc)
    assert not torch.equal(ta["bbox3d"], tc["bbox3d"])


@pytest.fixture(scope="module")
def scene_files_4c(tmp_path_factory):
    from detection_3d_amd.synthetic import write_scene_file
    d = tmp_path_factory.mktemp("aug_scenes")
    cfg = _cfg()
    return [write_scene_file(str(d / f"scene_{i}.npz"), 90 + i, 200000, cfg.INPUT.CLASSES) for i in range(3)]


def _train(cfg, files, dev, steps, aug, ims=1):
    from detection_3d_amd import engine
    from detection_3d_amd.detector import build_detection_model
    torch.manual_seed(0)
    model = build_detection_model(cfg).to(dev)
    return engine.train(model, cfg, files, dev, steps=steps, ims_per_gpu=ims, augment=aug)


def test_deterministic_training_with_augmentation(dev, scene_files_4c):
    from detection_3d_amd.augment import Augment
    cfg = _cfg()
    kw = dict(rotate="free", flip_x=True, scale_jitter=0.1, origin_offset=True, elastic=True, color_noise=0.02, seed=3)
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        a = _train(cfg, scene_files_4c, dev, 2, Augment(**kw))
        b = _train(cfg, scene_files_4c, dev, 2, Augment(**kw))
    finally:
        torch.use_deterministic_algorithms(was)
    assert a["losses"] == b["losses"] and all(np.isfinite(v) for v in a["losses"].values())


def test_training_4c_all_on_free(dev, scene_files_4c):
    from detection_3d_amd.augment import Augment
    aug = Augment(rotate="free", flip_x=True, scale_jitter=0.1, origin_offset=True, elastic=True, color_noise=0.02)
    out = _train(_cfg(), scene_files_4c, dev, 3, aug, ims=2)
    assert out["steps_timed"] == 2 and all(np.isfinite(v) for v in out["losses"].values())


def test_training_6c_quarter(dev, tmp_path):
    from detection_3d_amd.augment import Augment
    from detection_3d_amd.synthetic import write_scene_file
    cfg = _cfg("6c_Fpn4321")
    files = [write_scene_file(str(tmp_path / f"s{i}.npz"), 40 + i, 60000, cfg.INPUT.CLASSES) for i in range(2)]
    with pytest.raises(ValueError, match="zero-yaw"):
        _train(cfg, files, dev, 1, Augment(rotate="free"))
    aug = Augment(rotate="quarter", flip_x=True, scale_jitter=0.1, origin_offset=True, elastic=True, color_noise=0.02)
    out = _train(cfg, files, dev, 3, aug, ims=2)
    assert out["steps_timed"] == 2 and all(np.isfinite(v) for v in out["losses"].values())
