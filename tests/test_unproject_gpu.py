"""detection_3d_amd.unproject (unproject.hip) against the numpy restatement of its semantics in tests/unproject_ref.py,
and its plumbing through fuse_frames and serving.BuildingPipeline.

Bounds, derived: N, pixel_of_point and the order are integers and must be exact.  Positions and colours are the same
IEEE fp64 operations in the same order on both sides (no contraction, correctly rounded division) and one rounding to
fp32: bit for bit.  The normals add an fp64 sqrt and three divisions by it; should the device's differ in the last bit
from numpy's, the single fp32 rounding of a value of magnitude <= 1 moves by at most one ulp <= 2^-24, so every
component is within 2^-23 of the restatement."""
import numpy as np
import pytest
import torch

from tests.unproject_ref import (PLANE, ROOM, angle_to, holes_scene, plane_angle_bound, plane_scene, room_face_distance,
                                 room_scene, unproject_ref, walls_scene)

pytestmark = pytest.mark.gpu

SHAPES = [(3, 37, 53), (2, 96, 131)]
_REF = {}


def _scene(shape, float_depth=False):
    key = ("scene", shape, float_depth)
    if key not in _REF:
        _REF[key] = holes_scene(*shape, float_depth=float_depth)
    return _REF[key]


def _ref(shape, float_depth=False, float_color=False, **kw):
    """the restatement at 9 columns, computed once per case (fewer columns are its leading ones)"""
    key = ("ref", shape, float_depth, float_color, tuple(sorted(kw.items())))
    if key not in _REF:
        depth, color, intr, extr = _scene(shape, float_depth)
        _REF[key] = unproject_ref(depth, intr, extr, color=_color(color, float_color), columns=9, **kw)
    return _REF[key]


def _color(color, as_float):
    """fp32 colours with a few bit patterns an arithmetic copy would change"""
    if not as_float:
        return color
    c = (color.astype(np.float32) / np.float32(255.0)).copy()
    c[0, 0, 0] = (np.float32(-0.0), np.float32(np.nan), np.float32(1e-42))
    return c


def _frames(dev, depth, intr, extr, color=None, **kw):
    from detection_3d_amd.unproject import DepthFrames
    return DepthFrames(torch.from_numpy(depth).to(dev), intr, extr,
                       color=None if color is None else torch.from_numpy(color).to(dev), **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(dev, shape, columns, float_depth=False, float_color=False, intr_of=None, extr_of=None, **kw):
    from detection_3d_amd.unproject import unproject
    depth, color, intr, extr = _scene(shape, float_depth)
    r_rows, r_pix, r_has = _ref(shape, float_depth, float_color, **kw)
    fr = _frames(dev, depth, intr if intr_of is None else intr_of(intr), extr if extr_of is None else extr_of(extr),
                 color=_color(color, float_color))
    rows, pix = unproject(fr, columns=columns, return_pixels=True, **kw)
    assert rows.dtype == torch.float32 and pix.dtype == torch.int32
    rows, pix = rows.cpu().numpy(), pix.cpu().numpy()
    what = (shape, columns, float_depth, float_color, kw)
    assert rows.shape == (r_rows.shape[0], columns), what
    assert np.array_equal(pix, r_pix), what
    k = min(columns, 6)
    assert np.array_equal(_bits(rows[:, :k]), _bits(r_rows[:, :k])), what
    if columns == 9:
        zero = (rows[:, 6:9] == 0).all(1)
        assert np.array_equal(zero, ~r_has), what
        err = np.abs(rows[:, 6:9].astype(np.float64) - r_rows[:, 6:9].astype(np.float64))
        print(f"{what}: {rows.shape[0]} rows, {int(zero.sum())} without a normal; {int((err > 0).sum())} of {err.size} "
              f"normal components differ, largest {err.max():.3e} (bound {2.0 ** -23:.3e})")
        assert (err <= 2.0 ** -23).all(), what
    return rows, pix


@pytest.mark.parametrize("columns", [3, 6, 9])
@pytest.mark.parametrize("shape", SHAPES)
def test_uint16_depth_uint8_colour(dev, shape, columns):
    """tests 1 and 2 of the issue: exact positions, colours and order; normals against the restatement"""
    depth = _scene(shape)[0]
    assert depth[0, 0, 0] > 0 and depth[-1, -1, -1] > 0 and 0.25 < (depth == 0).mean() < 0.7
    assert shape[0] < 3 or not depth[1].any()
    _check(dev, shape, columns)


@pytest.mark.parametrize("columns", [3, 6, 9])
@pytest.mark.parametrize("shape", SHAPES)
def test_float_depth_with_nan_inf_negative_and_out_of_range(dev, shape, columns):
    depth = _scene(shape, True)[0]
    assert np.isnan(depth).any() and np.isinf(depth).any() and (depth < 0).any()
    assert ((depth > 0) & (depth < 0.5)).any() and ((depth > 6.0) & np.isfinite(depth)).any()
    _check(dev, shape, columns, float_depth=True, min_depth=0.5, max_depth=6.0)


@pytest.mark.parametrize("columns", [6, 9])
@pytest.mark.parametrize("shape", SHAPES)
def test_float_colour_is_copied_bit_for_bit(dev, shape, columns):
    _check(dev, shape, columns, float_color=True)


@pytest.mark.parametrize("step", [2, 3])
@pytest.mark.parametrize("columns", [3, 6, 9])
@pytest.mark.parametrize("shape", SHAPES)
def test_step_keeps_the_lattice_and_normals_use_raw_neighbours(dev, shape, columns, step):
    rows, pix = _check(dev, shape, columns, step=step)
    F, H, W = shape
    assert (pix % W % step == 0).all() and (pix // W % H % step == 0).all() and 0 < rows.shape[0]


@pytest.mark.parametrize("shape", SHAPES)
def test_broadcast_intrinsics_and_4x4_extrinsics(dev, shape):
    from detection_3d_amd.unproject import unproject
    depth, color, intr, extr = _scene(shape)
    F = shape[0]
    bottom = np.tile(np.array([[[0.0, 0.0, 0.0, 1.0]]]), (F, 1, 1))
    # [F, 4, 4] extrinsics against the restatement
    _check(dev, shape, 9, extr_of=lambda e: torch.from_numpy(np.concatenate([e, bottom], 1)))
    # [4] intrinsics: the same as the row repeated
    one = _frames(dev, depth, intr[0], np.concatenate([extr, bottom], 1), color=color)
    rep = _frames(dev, depth, np.tile(intr[0], (F, 1)), extr, color=color)
    assert torch.equal(unproject(one), unproject(rep))
    r_rows, r_pix, _ = unproject_ref(depth, intr[0], extr, color=color, columns=6)
    got = unproject(one, columns=6).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(r_rows))


def test_plane(dev):
    """A tilted plane n . X = d seen through f = 300 px at 60 x 80 pixels, the depth computed analytically per pixel and
    rounded to fp32.  Bound on the angle between an interior pixel's normal and n: a sample's depth is off by eps z,
    eps <= 2^-24, which moves the point along its ray by eps C, that is by eps (n . C) = eps d out of the plane.  A central
    difference of two samples is a = a0 + alpha n with a0 in the plane and |alpha| <= 2 eps |d|, likewise b = b0 + beta n.
    Then a x b = |a0| |b0| sin(phi) n + alpha (n x b0) + beta (a0 x n), the last two terms in the plane, so
    tan(angle) <= (|alpha| / |a0| + |beta| / |b0|) / sin(phi) <= 2 eps |d| (1 / |a0| + 1 / |b0|) / sin(phi), with
    |a0| ~ 2 z / f the pixel baseline and sin(phi) set by the tilt.  The bound is evaluated from the exact points (their
    in-plane perturbation changes it by eps z / |a0| ~ 1e-5 relative: the factor 1 + 1e-3), plus 2^-24 for the fp32
    rounding of the components; fp64 arithmetic is 2^-29 of eps and negligible (tests/unproject_ref.py,
    plane_angle_bound)."""
    from detection_3d_amd.unproject import unproject
    depth, intr, extr, points = plane_scene()
    H, W = PLANE["H"], PLANE["W"]
    rows = unproject(_frames(dev, depth, intr, extr)).cpu().numpy()
    assert rows.shape == (H * W, 9) and (rows[:, 3:6] == 0).all()          # no colour image: zeros
    n = rows[:, 6:9].reshape(H, W, 3)[1:-1, 1:-1].reshape(-1, 3)
    C = rows[:, 0:3].reshape(H, W, 3)[1:-1, 1:-1].reshape(-1, 3).astype(np.float64)      # identity extrinsics
    assert (n != 0).any(1).all()
    assert ((n.astype(np.float64) * C).sum(1) < 0).all()
    ang = angle_to(n, PLANE["normal"])
    bound = plane_angle_bound(points)
    print(f"plane: largest angle to the true normal {ang.max():.3e} rad, bound {bound:.3e} rad")
    assert ang.max() <= bound


def test_depth_edge(dev):
    from detection_3d_amd.unproject import unproject
    depth, intr, extr, col = walls_scene()
    H, W = depth.shape[1:]
    fr = _frames(dev, depth, intr, extr)
    n = unproject(fr, edge=0.05).cpu().numpy()[:, 6:9]
    assert n.shape == (H * W, 3) and (n == np.array([0.0, 0.0, -1.0], np.float32)).all()
    n = unproject(fr, edge=1.0).cpu().numpy()[:, 6:9].reshape(H, W, 3)
    at_step = np.zeros(W, bool)
    at_step[[col - 1, col]] = True
    assert (n[:, ~at_step] == np.array([0.0, 0.0, -1.0], np.float32)).all()
    assert (n[:, at_step] != np.array([0.0, 0.0, -1.0], np.float32)).any(-1).all()


def test_edge_cases(dev):
    from detection_3d_amd.unproject import DepthFrames, unproject
    # no frame, and a batch without a valid pixel
    empty = DepthFrames(torch.zeros(0, 4, 5, dtype=torch.uint16, device=dev), [1.0, 1.0, 0.0, 0.0], np.zeros((0, 3, 4)))
    rows, pix = unproject(empty, columns=6, return_pixels=True)
    assert rows.shape == (0, 6) and pix.shape == (0,) and rows.dtype == torch.float32 and pix.dtype == torch.int32
    dead = torch.full((2, 9, 11), float("nan"), device=dev)
    dead[1] = -1.0
    rows = unproject(DepthFrames(dead, [10.0, 10.0, 5.0, 4.0], np.zeros((2, 3, 4))))
    assert rows.shape == (0, 9)
    # one row or one column of pixels: positions right, no normals
    rs = np.random.RandomState(5)
    for shape in ((2, 1, 300), (2, 300, 1)):
        depth = (1.0 + rs.rand(*shape)).astype(np.float32)
        intr = np.array([50.0, 55.0, 0.5 * (shape[2] - 1), 0.5 * (shape[1] - 1)])
        extr = np.concatenate([np.eye(3), np.ones((3, 1))], 1)[None].repeat(2, 0)
        r_rows, r_pix, r_has = unproject_ref(depth, intr, extr)
        rows, pix = unproject(_frames(dev, depth, intr, extr), return_pixels=True)
        assert not r_has.any() and np.array_equal(pix.cpu().numpy(), r_pix)
        assert np.array_equal(_bits(rows.cpu().numpy()), _bits(r_rows)) and (rows[:, 6:9] == 0).all()
    # a non-contiguous depth view (every other column of a wider image), uint16 and fp32
    shape = SHAPES[0]
    depth, color, intr, extr = _scene(shape)
    wide = np.zeros((shape[0], shape[1], 2 * shape[2]), depth.dtype)
    wide[:, :, ::2] = depth
    wide[:, :, 1::2] = 1234
    for cast in (lambda a: a, lambda a: a.astype(np.float32) * np.float32(0.001)):
        view = torch.from_numpy(cast(wide)).to(dev)[:, :, ::2]
        assert not view.is_contiguous()
        whole = torch.from_numpy(cast(depth)).to(dev)
        got = unproject(DepthFrames(view, intr, extr))
        want = unproject(DepthFrames(whole, intr, extr))
        assert got.shape[0] > 0 and torch.equal(got, want)
    # two runs give the same bits
    fr = _frames(dev, depth, intr, extr, color=color)
    a, b = unproject(fr), unproject(fr)
    assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))


@pytest.fixture(scope="module")
def room(dev):
    from detection_3d_amd.unproject import suncg_cameras
    depth, cams = room_scene()
    intr, extr = suncg_cameras(cams, depth.shape[1], depth.shape[2])
    rs = np.random.RandomState(9)
    color = rs.randint(0, 256, depth.shape + (3,)).astype(np.uint8)
    return _frames(dev, depth, intr, extr, color=color)


def test_fuse_frames_is_unproject_then_downsample(dev, room):
    """The room of tests/unproject_ref.py: every rendered point lies on a face, so a voxel's mean lies within the voxel's
    edge of the face its points came from; the cameras are inside the convex room, so a normal facing its camera points
    into the room."""
    from detection_3d_amd.downsample import apply_downsample, downsample_kwargs
    from detection_3d_amd.unproject import fuse_frames, unproject
    voxel = 0.1
    for max_points in (500_000, 1000):
        fused = fuse_frames(room, voxel=voxel, max_points=max_points, seed=3, edge=0.05)
        want = apply_downsample(unproject(room, edge=0.05),
                                downsample_kwargs({"voxel": voxel, "max_points": max_points, "seed": 3}))
        assert fused.shape == want.shape and fused.shape[1] == 9
        assert np.array_equal(_bits(fused.cpu().numpy()), _bits(want.cpu().numpy()))
    assert fused.shape[0] == 1000
    fused = fuse_frames(room, voxel=voxel).cpu().numpy()
    raw = unproject(room)
    assert 1000 < fused.shape[0] < raw.shape[0] == room.depth.numel()
    dist = room_face_distance(fused[:, 0:3])
    n = fused[:, 6:9].astype(np.float64)
    has = (n != 0).any(1)
    inward = (n * (0.5 * ROOM - fused[:, 0:3].astype(np.float64))).sum(1)
    print(f"room: {raw.shape[0]} pixels -> {fused.shape[0]} points, farthest from a face {dist.max():.4f} m (voxel {voxel}), "
          f"{int(has.sum())} normals, smallest inward component {inward[has].min():.3f} m")
    assert dist.max() <= voxel + 1e-5
    assert has.sum() > 0.9 * fused.shape[0] and (inward[has] > 0).all()
    assert (np.abs(np.sqrt((n[has] ** 2).sum(1)) - 1.0) < 2.0 ** -22).all()


@pytest.fixture(scope="module")
def tiny(dev):
    """the model of tests/test_downsample_gpu.py"""
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


def _same(a, b):
    return all(a[k].shape == b[k].shape and torch.equal(a[k], b[k]) for k in ("bbox3d", "scores", "labels"))


def test_pipeline_takes_frames(tiny, room, dev):
    from detection_3d_amd.serving import BuildingPipeline
    from detection_3d_amd.unproject import pixel_labels, unproject
    cfg, model = tiny
    kw = {"edge": 0.1, "min_depth": 1.7}
    cloud, pixel_of_point = unproject(room, return_pixels=True, **kw)
    assert 0 < cloud.shape[0] < room.depth.numel()
    with torch.no_grad():
        pipe = BuildingPipeline(model, cfg, in_flight=2, device=dev, point_owner=True, unproject=kw)
        got = pipe.map([room, cloud, room])
        want = BuildingPipeline(model, cfg, in_flight=2, device=dev, point_owner=True).map([cloud])[0]
        plain = BuildingPipeline(model, cfg, in_flight=2, device=dev, unproject=kw).map([room])[0]
    torch.cuda.synchronize()
    print(f"pipeline: {cloud.shape[0]} points -> {want['bbox3d'].shape[0]} detections")
    assert _same(got[0], want) and _same(got[1], want) and _same(got[2], want) and _same(plain, want)
    assert "point_pixel" not in plain and "point_pixel" not in got[1] and "point_pixel" not in want
    for r in (got[0], got[2]):
        assert torch.equal(r["point_pixel"], pixel_of_point)
        assert torch.equal(r["point_owner"], want["point_owner"]) and torch.equal(r["point_count"], want["point_count"])
    img = pixel_labels(got[0]["point_owner"], got[0]["point_pixel"], room)
    assert img.shape == room.depth.shape and img.dtype == torch.int32
    dropped = torch.ones(room.depth.numel(), dtype=torch.bool, device=dev)
    dropped[pixel_of_point.long()] = False
    marked = pixel_labels(got[0]["point_owner"] + 1, got[0]["point_pixel"], room)       # owners -1 .. become 0 ..
    assert torch.equal((marked == -1).view(-1), dropped) and bool(dropped.any())
    assert torch.equal(img.view(-1)[pixel_of_point.long()], got[0]["point_owner"])
