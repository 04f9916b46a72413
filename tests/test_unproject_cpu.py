"""Host side of detection_3d_amd.unproject: the camera convention, the argument checks, and the consistency of the
numpy restatement (tests/unproject_ref.py) the GPU tests compare against.  No GPU."""
import numpy as np
import pytest
import torch

from tests.unproject_ref import (PLANE, angle_to, holes_scene, plane_angle_bound, plane_scene, unproject_ref,
                                 walls_scene)


def _cam(centre=(38.0, 1.25, 41.5), yaw=0.4, pitch=-0.2, xf=0.55, H=480, W=640):
    t = np.array([np.cos(yaw) * np.cos(pitch), np.sin(pitch), np.sin(yaw) * np.cos(pitch)])
    right = np.cross(t, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    u = np.cross(right, t)
    yf = np.arctan(np.tan(xf) * H / W)
    return np.concatenate([centre, t, u, [xf, yf, 14.2]])


def test_suncg_cameras_axis_and_right():
    from detection_3d_amd.unproject import suncg_cameras
    H, W = 480, 640
    cam = _cam(H=H, W=W)
    intr, extr = suncg_cameras(np.stack([cam, _cam(yaw=2.0, pitch=0.1)]), H, W)
    assert intr.shape == (2, 4) and extr.shape == (2, 3, 4) and intr.dtype == np.float64
    v, t, u = cam[0:3], cam[3:6], cam[6:9]
    fx, fy, cx, cy = intr[0]
    assert fx == fy == 0.5 * W / np.tan(cam[9]) and cx == 319.5 and cy == 239.5
    R, trans = extr[0, :, :3], extr[0, :, 3]
    # a point on the optical axis at depth z: camera (0, 0, z) -> v + z t
    z = 3.25
    assert np.allclose(R @ [0.0, 0.0, z] + trans, v + z * t, rtol=0, atol=1e-12)
    # a pixel right of the centre moves along t x u, one below it along -u
    du = 10.0
    C = np.array([(cx + du - cx) * z / fx, 0.0, z])
    assert np.allclose(R @ C + trans - (v + z * t), np.cross(t, u) * du * z / fx, rtol=0, atol=1e-12)
    C = np.array([0.0, 7.0 * z / fy, z])
    assert np.allclose(R @ C + trans - (v + z * t), -u * 7.0 * z / fy, rtol=0, atol=1e-12)
    assert abs(np.linalg.det(R) - 1.0) < 1e-9


def test_suncg_cameras_refuses_what_the_reference_asserts():
    from detection_3d_amd.unproject import suncg_cameras
    cam = _cam()
    bad = cam.copy()
    bad[10] *= 1.01                      # the focal length from yf is off by pixels
    with pytest.raises(ValueError, match="focal"):
        suncg_cameras(bad, 480, 640)
    bad = cam.copy()
    bad[6:9] = bad[6:9] * 1.05           # up is not a unit vector
    with pytest.raises(ValueError, match="orthonormal"):
        suncg_cameras(bad, 480, 640)
    bad = cam.copy()
    bad[6:9] = bad[6:9] + 0.05 * bad[3:6]    # up leans into forward
    with pytest.raises(ValueError, match="orthonormal"):
        suncg_cameras(bad, 480, 640)
    suncg_cameras(cam, 480, 640)


def test_depthframes_argument_checks():
    from detection_3d_amd._lib import D3DError
    from detection_3d_amd.unproject import DepthFrames
    F, H, W = 2, 5, 7
    depth = torch.zeros(F, H, W, dtype=torch.uint16)
    K, E = [300.0, 300.0, 3.0, 2.0], np.zeros((F, 3, 4))
    for bad in (torch.zeros(F, H, W, dtype=torch.float64), torch.zeros(F, H, W, dtype=torch.int32),
                torch.zeros(H, W, dtype=torch.uint16), np.zeros((F, H, W), np.float32)):
        with pytest.raises(ValueError, match="depth"):
            DepthFrames(bad, K, E)
    for bad in (torch.zeros(F, H, W, 3, dtype=torch.float64), torch.zeros(F, H, W, 4, dtype=torch.uint8),
                torch.zeros(F, H, W + 1, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="color"):
            DepthFrames(depth, K, E, color=bad)
    for bad in (np.zeros((F, 3)), np.zeros((F + 1, 4)), np.zeros(3)):
        with pytest.raises(ValueError, match="intrinsics"):
            DepthFrames(depth, bad, E)
    for bad in (np.zeros((F, 3, 3)), np.zeros((F + 1, 3, 4)), np.zeros((3, 4))):
        with pytest.raises(ValueError, match="extrinsics"):
            DepthFrames(depth, K, bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="depth_scale"):
            DepthFrames(depth, K, E, depth_scale=bad)
    # 2 x 32768 x 32768 = 2^31 pixels (an expanded view: no memory behind it)
    huge = torch.zeros(1, 1, 1, dtype=torch.uint16).expand(2, 32768, 32768)
    with pytest.raises(ValueError, match="31 bits"):
        DepthFrames(huge, K, np.zeros((2, 3, 4)))
    # well-formed, but on the CPU: no fallback
    with pytest.raises(D3DError):
        DepthFrames(depth, K, E)
    with pytest.raises(D3DError):
        DepthFrames(torch.zeros(F, H, W), np.zeros((F, 4)), np.zeros((F, 4, 4)), color=torch.zeros(F, H, W, 3))


def test_unproject_argument_checks():
    from detection_3d_amd.unproject import fuse_frames, pixel_labels, unproject, unproject_kwargs
    for kw in ({"columns": 4}, {"columns": 12}, {"step": 0}, {"step": 1.5}, {"edge": -0.1}, {"edge": float("nan")},
               {"color_div": 0.0}, {"min_depth": float("nan")}):
        with pytest.raises(ValueError):
            unproject(None, **kw)
        with pytest.raises(ValueError):
            unproject_kwargs(kw)
    with pytest.raises(ValueError, match="DepthFrames"):
        unproject(torch.zeros(2, 5, 7))
    with pytest.raises(ValueError, match="unknown"):
        unproject_kwargs({"voxel": 0.02})
    with pytest.raises(ValueError):
        unproject_kwargs("estimate")
    assert unproject_kwargs(None) == {} and unproject_kwargs({"step": 2, "columns": 6}) == {"step": 2, "columns": 6}
    with pytest.raises(ValueError, match="pixel"):
        fuse_frames(None, return_pixels=True)
    img = pixel_labels(torch.tensor([4, 5, 6]), torch.tensor([0, 7, 11], dtype=torch.int32), (2, 2, 3))
    assert img.tolist() == [[[4, -1, -1], [-1, -1, -1]], [[-1, 5, -1], [-1, -1, 6]]]
    with pytest.raises(ValueError):
        pixel_labels(torch.tensor([0.5]), torch.tensor([0]), (1, 1, 1))


def test_pipeline_checks_its_unproject_keywords():
    from detection_3d_amd.serving import BuildingPipeline
    with pytest.raises(ValueError, match="unknown"):
        BuildingPipeline(None, None, device=torch.device("cpu"), unproject={"voxel": 1})


def _normal_checks(rows, has, C_of_row, what):
    """lengths within 2^-23 of 0 or 1; non-zero exactly where `has`; every non-zero normal faces its camera"""
    n = rows[:, 6:9].astype(np.float64)
    length = np.sqrt((n * n).sum(1))
    zero = (rows[:, 6:9] == 0).all(1)
    assert np.array_equal(~zero, has), what
    assert (np.abs(length[has] - 1.0) <= 2.0 ** -23).all(), (what, np.abs(length[has] - 1.0).max())
    assert ((n * C_of_row).sum(1)[has] < 0).all(), what


def _camera_points(rows, pix, intr, extr, shape):
    """the camera-frame direction of every row's own camera to the point, in world axes: X - t"""
    F, H, W = shape
    f = pix // (H * W)
    return rows[:, 0:3].astype(np.float64) - np.asarray(extr)[f, :3, 3]


def test_reference_is_consistent_on_the_plane():
    depth, intr, extr, points = plane_scene()
    rows, pix, has = unproject_ref(depth, intr, extr, columns=9)
    H, W = PLANE["H"], PLANE["W"]
    assert rows.shape == (H * W, 9) and np.array_equal(pix, np.arange(H * W))
    _normal_checks(rows, has, _camera_points(rows, pix, intr, extr, depth.shape), "plane")
    assert has.all()                       # the border pixels take one-sided differences
    interior = np.zeros((H, W), bool)
    interior[1:-1, 1:-1] = True
    ang = angle_to(rows[:, 6:9], PLANE["normal"])[interior.ravel()]
    bound = plane_angle_bound(points)
    print(f"plane (restatement): largest angle to the true normal {ang.max():.3e} rad, bound {bound:.3e} rad")
    assert ang.max() <= bound


def test_reference_is_consistent_on_the_walls():
    depth, intr, extr, col = walls_scene()
    rows, pix, has = unproject_ref(depth, intr, extr, columns=9, edge=0.05)
    _normal_checks(rows, has, _camera_points(rows, pix, intr, extr, depth.shape), "walls")
    assert has.all() and (rows[:, 6:9] == np.array([0.0, 0.0, -1.0], np.float32)).all()
    rows, _, has = unproject_ref(depth, intr, extr, columns=9, edge=1.0)
    n = rows[:, 6:9].reshape(depth.shape[1], depth.shape[2], 3)
    at_step = np.zeros(depth.shape[2], bool)
    at_step[[col - 1, col]] = True
    assert (n[:, ~at_step] == np.array([0.0, 0.0, -1.0], np.float32)).all()
    assert (n[:, at_step, 2] > -0.9).all() and has.all()


@pytest.mark.parametrize("shape", [(3, 37, 53), (2, 96, 131)])
def test_reference_zero_normals_are_the_pixels_without_a_neighbour_pair(shape):
    depth, color, intr, extr = holes_scene(*shape)
    edge = 0.05
    rows, pix, has = unproject_ref(depth, intr, extr, color=color, columns=9, edge=edge)
    _normal_checks(rows, has, _camera_points(rows, pix, intr, extr, shape), "holes")
    # the definition again, pixel by pixel in plain Python
    F, H, W = shape
    z = depth.astype(np.float64) * 0.001
    want = np.zeros(pix.shape[0], bool)
    for i, p in enumerate(pix):
        f, v, u = p // (H * W), (p // W) % H, p % W

        def usable(vv, uu):
            return 0 <= vv < H and 0 <= uu < W and z[f, vv, uu] > 0 and abs(z[f, vv, uu] - z[f, v, u]) <= edge * z[f, v, u]
        want[i] = (usable(v, u + 1) or usable(v, u - 1)) and (usable(v + 1, u) or usable(v - 1, u))
    assert 0 < want.sum() < want.shape[0]
    assert np.array_equal(has, want)
    assert (depth.reshape(-1)[pix] > 0).all() and pix.shape[0] == int((depth > 0).sum())
    assert pix[0] == 0 and pix[-1] == F * H * W - 1
