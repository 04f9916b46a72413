"""frame.manhattan_frame without a GPU: the numpy restatement of its definition (tests/frame_ref.py) recovers a known
rotation, the candidate tables, the box helpers on hand-made boxes, and the argument checks."""
import math

import numpy as np
import pytest
import torch

from tests.frame_ref import heading_error_deg, manhattan_frame_ref, tilt_tables, tilted_room, up_error_deg

# (tilt, azimuth, yaw) of the scans: tilt <= 25 degrees, any yaw
SCANS = [(25.0, 10.0, 10.0), (13.0, 200.0, 44.0), (20.0, 300.0, 46.0), (5.0, 77.0, 80.0), (24.0, 123.0, 271.0),
         (0.0, 0.0, 0.0), (17.0, 250.0, 135.0)]


def test_tilt_tables_are_rotations_and_entry_136_is_the_identity():
    from detection_3d_amd.frame import tilt_tables as package_tables
    for max_tilt in (30.0, 60.0, 7.0):
        T = tilt_tables(max_tilt)
        assert T.shape == (3, 256, 3, 3)
        assert np.abs(T @ np.swapaxes(T, -1, -2) - np.eye(3)).max() <= 1e-14
        assert np.abs(np.linalg.det(T) - 1.0).max() <= 1e-14
        for k in range(3):
            assert np.array_equal(T[k, 136].view(np.uint64), np.eye(3).view(np.uint64))
        # candidate 16 i + j leans towards ((j - 8) t, (i - 8) t, 1)
        t = math.tan(math.radians(max_tilt / 8.0))
        up = T[0, 16 * 3 + 12, :, 2]
        assert np.allclose(up[:2] / up[2], [4 * t, -5 * t], atol=1e-14)
        # the package hands the device the tables of the definition
        assert np.array_equal(package_tables(max_tilt).view(np.uint64), T.view(np.uint64))


@pytest.mark.parametrize("seed,scan", list(enumerate(SCANS)))
def test_restatement_recovers_the_rotation_without_noise(seed, scan):
    nm, R = tilted_room(20000, *scan, noise=0.0, clutter=0.25, seed=seed)
    res = manhattan_frame_ref(nm)
    up, head = up_error_deg(res, R), heading_error_deg(res, R)
    print(f"scan {scan}: up {up:.4f} deg, heading {head:.4f} deg, choice {res['choice']}")
    assert up <= 30.0 / 512.0             # one third-pass step; the nearest lattice node is within 0.041
    assert head <= 0.01
    assert res["support"][0] == 20000 and 0.4 * 20000 < res["support"][1] < 0.55 * 20000
    P = res["pose"]
    assert np.abs(P[:3, :3] @ P[:3, :3].T - np.eye(3)).max() <= 1e-13 and abs(np.linalg.det(P[:3, :3]) - 1) <= 1e-13
    assert np.array_equal(P[3], [0, 0, 0, 1]) and np.array_equal(P[:3, 3], [0, 0, 0])


@pytest.mark.parametrize("seed,scan", list(enumerate(SCANS)))
def test_restatement_recovers_the_rotation_with_two_degrees_of_noise(seed, scan):
    """measured with these seeds: up 0.000-0.067 degrees (three of seven above 0.05: 0.058, 0.051, 0.067), heading
    0.004-0.035; the bound is 0.1 for both"""
    nm, R = tilted_room(20000, *scan, noise=2.0, clutter=0.25, seed=100 + seed)
    res = manhattan_frame_ref(nm)
    up, head = up_error_deg(res, R), heading_error_deg(res, R)
    print(f"scan {scan}: up {up:.4f} deg, heading {head:.4f} deg")
    assert up <= 0.1 and head <= 0.1


def test_degenerate_inputs():
    nm, R = tilted_room(5000, 12.0, 40.0, 20.0, seed=3)
    res = manhattan_frame_ref(nm, max_tilt=0.0)                        # the up axis is left alone
    assert np.array_equal(res["B3"], np.eye(3)) and list(res["choice"][:3]) == [136] * 3 and list(res["score"][:3]) == [0] * 3
    assert np.array_equal(res["pose"][2, :3], [0, 0, 1]) and np.array_equal(res["pose"][:3, 2], [0, 0, 1])
    hint = manhattan_frame_ref(nm, max_tilt=0.0, up=(0.1, -0.2, 1.0))
    assert np.allclose(hint["B3"][:, 2], np.array([0.1, -0.2, 1.0]) / math.sqrt(1.05), atol=1e-15)
    empty = manhattan_frame_ref(np.zeros((0, 3), np.float32))
    assert np.array_equal(empty["pose"], np.eye(4)) and list(empty["choice"]) == [136, 136, 136, 0, 128]
    assert list(empty["score"]) == [0] * 5 and list(empty["support"]) == [0, 0]
    floor = np.tile(np.array([[0, 0, 1], [0, 0, -1]], np.float32), (50, 1))
    res = manhattan_frame_ref(floor)
    assert list(res["support"]) == [100, 0] and list(res["choice"][3:]) == [0, 128] and list(res["score"][3:]) == [0, 0]
    assert np.array_equal(res["pose"], np.eye(4)) and res["score"][0] > 0
    junk = np.full((7, 3), np.nan, np.float32)
    junk[3] = 0.0
    junk[4] = np.inf
    assert np.array_equal(manhattan_frame_ref(junk)["pose"], np.eye(4))


@pytest.mark.parametrize("yaw", [10.0, 44.0, 46.0, 80.0])
def test_heading_is_the_one_within_45_degrees_of_the_scans_own(yaw):
    nm, R = tilted_room(8000, 0.0, 0.0, yaw, seed=int(yaw))
    res = manhattan_frame_ref(nm)
    got = res["t"] * 180.0 / 65536.0
    want = yaw if yaw < 45 else yaw - 90
    assert -45.0 <= got < 45.0 and abs(got - want) <= 0.01
    # pose maps the scan's wall normals onto the axes, and turns the scan by less than 45 degrees
    P = res["pose"][:3, :3]
    assert abs(math.degrees(math.atan2(P[1, 0], P[0, 0])) + want) <= 0.01
    assert np.abs(np.abs(P @ R) - np.abs(np.round(P @ R))).max() <= 1e-3 and heading_error_deg(res, R) <= 0.01


def _corners(box):
    """analytic corners of one yx_zb box, corner 4 a + 2 b + c"""
    xc, yc, zb, d3, d4, dz, yaw = box
    c, s = math.cos(yaw), math.sin(yaw)
    out = []
    for lx in (-d3 / 2, d3 / 2):
        for ly in (-d4 / 2, d4 / 2):
            for lz in (0.0, dz):
                out.append([xc + c * lx + s * ly, yc - s * lx + c * ly, zb + lz])
    return np.array(out)


BOXES = [[3.0, 4.0, 0.5, 0.2, 5.0, 2.5, 0.3], [10.0, -2.0, 0.0, 0.1, 2.0, 2.7, -math.pi / 2],
         [0.0, 0.0, 1.0, 4.0, 6.0, 0.05, 0.0], [7.5, 7.5, 0.2, 0.3, 3.0, 1.0, 1.5]]


def _pose(R, t):
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, t
    return torch.from_numpy(P)


def test_box_helpers_under_a_pure_yaw():
    from detection_3d_amd.frame import box_corners_in_scan_frame, boxes_in_scan_frame
    phi, t = math.radians(30.0), np.array([1.0, 2.0, 3.0])
    R = np.array([[math.cos(phi), -math.sin(phi), 0.0], [math.sin(phi), math.cos(phi), 0.0], [0.0, 0.0, 1.0]])
    boxes = torch.tensor(BOXES, dtype=torch.float64)
    corners = box_corners_in_scan_frame(boxes, _pose(R, t))
    assert corners.shape == (4, 8, 3) and corners.dtype == torch.float64
    for b, got in zip(BOXES, corners.numpy()):
        want = (_corners(b) - t) @ R                                   # x = R^T (x' - t)
        assert np.abs(got - want).max() <= 1e-13
    moved = boxes_in_scan_frame(boxes, _pose(R, t))
    assert moved.shape == (4, 7) and torch.equal(moved[:, 3:6], boxes[:, 3:6])
    assert (moved[:, 6] >= -math.pi / 2).all() and (moved[:, 6] < math.pi / 2).all()
    for b, m, got in zip(BOXES, moved.numpy(), corners.numpy()):
        assert abs(((m[6] - b[6] - phi + math.pi / 2) % math.pi) - math.pi / 2) <= 1e-13       # yaw + phi, modulo pi
        mine = _corners(m)                     # the same eight corners; a yaw that wrapped by pi lists them in another order
        for c in got:
            assert np.abs(mine - c).sum(1).min() <= 1e-12
    # the identity leaves boxes alone; fp32 boxes come back as fp32
    inner = boxes[[0, 2, 3]].float()           # (box 1's yaw sits on the wrap)
    same = boxes_in_scan_frame(inner, torch.eye(4, dtype=torch.float64))
    assert same.dtype == torch.float32 and torch.allclose(same, inner, atol=1e-6)


def test_box_helpers_under_a_pure_tilt():
    from detection_3d_amd.frame import box_corners_in_scan_frame, boxes_in_scan_frame
    th = math.radians(6.0)
    R = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(th), -math.sin(th)], [0.0, math.sin(th), math.cos(th)]])
    t = np.array([-0.5, 0.25, 2.0])
    boxes = torch.tensor(BOXES, dtype=torch.float64)
    corners = box_corners_in_scan_frame(boxes, _pose(R, t)).numpy()
    for b, got in zip(BOXES, corners):
        assert np.abs(got - (_corners(b) - t) @ R).max() <= 1e-13
    # by hand, the first corner of box 0: R^T turns about x by -6 degrees
    x, y, z = _corners(BOXES[0])[0] - t
    assert np.allclose(corners[0, 0], [x, math.cos(th) * y + math.sin(th) * z, -math.sin(th) * y + math.cos(th) * z], atol=1e-13)
    with pytest.raises(ValueError, match="box_corners_in_scan_frame"):
        boxes_in_scan_frame(boxes, _pose(R, t))
    with pytest.raises(ValueError):
        boxes_in_scan_frame(boxes[:, :6], torch.eye(4))
    with pytest.raises(ValueError):
        box_corners_in_scan_frame(boxes, torch.eye(3))


def test_arguments_are_checked_before_any_device_call():
    from detection_3d_amd._lib import D3DError
    from detection_3d_amd.frame import align_cloud, align_kwargs, manhattan_frame, parse_align
    from detection_3d_amd.prepare import Preparation
    from detection_3d_amd.serving import BuildingPipeline
    nm = torch.zeros((4, 3))
    for kw in ({"tol": 0}, {"tol": 21}, {"tol": float("nan")}, {"max_tilt": -1}, {"max_tilt": 61}, {"max_tilt": "x"},
               {"up": (0, 0)}, {"up": (0, 0, 0)}, {"up": (1, 2, 3, 4)}, {"up": (0, float("nan"), 1)}, {"up": "z"}):
        with pytest.raises(ValueError):
            manhattan_frame(nm, **kw)
        with pytest.raises(ValueError):
            align_kwargs(kw)
        with pytest.raises(ValueError):
            Preparation(align=kw)
        with pytest.raises(ValueError):
            BuildingPipeline(None, None, device="cpu", align=kw)
    for bad in (torch.zeros((4, 4)), torch.zeros(4), torch.zeros((4, 3), dtype=torch.float64), [[0, 0, 1]]):
        with pytest.raises(ValueError):
            manhattan_frame(bad)
    with pytest.raises(D3DError):
        manhattan_frame(nm)
    with pytest.raises(ValueError):
        align_kwargs({"max_tilt": 10, "radius": 1})
    with pytest.raises(ValueError):
        align_kwargs("level")
    with pytest.raises(ValueError, match="estimate"):
        align_cloud(torch.zeros((4, 3)))
    with pytest.raises(ValueError, match="estimate"):
        align_cloud(torch.zeros((4, 6)))
    assert align_kwargs(None) is None and Preparation().align is None
    assert align_kwargs(True) == align_kwargs("manhattan") == {"max_tilt": 30.0, "tol": 5.0, "up": None}
    assert align_kwargs({"tol": 3})["tol"] == 3 and align_kwargs({"max_tilt": 0})["max_tilt"] == 0
    assert parse_align(None) is None and parse_align("") == align_kwargs(True)
    assert parse_align("20,4") == {"max_tilt": 20.0, "tol": 4.0, "up": None}
    for bad in ("20", "20,4,1", "a,b", "20,0"):
        with pytest.raises(ValueError):
            parse_align(bad)


def test_training_scenes_refuse_align():
    from types import SimpleNamespace
    from detection_3d_amd.prepare import Kept, Preparation
    chain = Preparation(align={"max_tilt": 10}, voxelize_fn=lambda pcl, cfg: ("coords", "feats"))
    assert chain.align == {"max_tilt": 10, "tol": 5.0, "up": None} and not chain.targets_in_file_frame
    cfg = SimpleNamespace(SPARSE3D=SimpleNamespace(VOXEL_SCALE=50), INPUT=SimpleNamespace(CLASSES=["wall"]))
    with pytest.raises(ValueError, match="align"):
        chain.scene(torch.zeros((6, 9)), {"bbox3d": torch.zeros((0, 7)), "labels": torch.zeros(0)}, cfg)
    assert Kept(1, 2, 3) == Kept(1, 2, 3, None) and Kept(1, 2, 3).pose is None          # the new field has a default
