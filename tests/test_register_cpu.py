"""tests/register_ref.py checked against itself and against brute force, and the parts of detection_3d_amd.register that
need no GPU: apply_pose and the argument checks."""
import numpy as np
import pytest
import torch

from tests import register_ref as rr


def test_nearest_ref_equals_a_brute_force_fp32_argmin():
    """300 queries against 400 points in a 0.5 m cube, some of either not finite, a duplicated cloud row and queries
    that coincide with cloud rows: the (bits, row) minimum over ALL rows in fp32, bit for bit."""
    rs = np.random.RandomState(0)
    cloud = (rs.rand(400, 3) * 0.5 + np.array([13.7, -4.2, 1.1])).astype(np.float32)
    query = (rs.rand(300, 3) * 0.6 - 0.05 + np.array([13.7, -4.2, 1.1])).astype(np.float32)
    cloud[17] = cloud[5]                                  # a tie: the lower row wins
    cloud[33, 1] = np.nan
    cloud[34, 0] = np.inf
    query[:20] = cloud[:20]                               # d2 = 0, and row 5 rather than 17
    query[40, 2] = np.nan
    query[41, 0] = -np.inf
    for radius in (0.03, 0.1):
        index, dist2 = rr.nearest_ref(query, cloud, radius)
        d2 = rr.d2_f32(cloud[None, :, :], query[:, None, :])                     # [300, 400]
        bits = d2.view(np.uint32).astype(np.int64)
        bits[bits > rr.r2_bits(radius)] = 1 << 40
        bits[~np.isfinite(query).all(1)] = 1 << 40
        best = bits.argmin(1)                             # the first minimum: the lowest row
        none = bits[np.arange(300), best] == 1 << 40
        want_i = np.where(none, -1, best).astype(np.int32)
        want_d = np.where(none, np.float32(np.inf), d2[np.arange(300), best]).astype(np.float32)
        assert np.array_equal(index, want_i)
        assert np.array_equal(dist2.view(np.uint32), want_d.view(np.uint32))
        assert index[5] == 5 and index[17] == 5 and index[40] == -1 and index[41] == -1
        assert none.sum() > 2 and (~none).sum() > 50      # both outcomes are there at either radius


def _corner():
    """three faces of a 1 m cube's corner on a 10 cm lattice, without noise, and their exact normals"""
    g = np.arange(0.05, 1.0, 0.1)
    u, v = [a.ravel() for a in np.meshgrid(g, g)]
    z = np.zeros_like(u)
    pts = np.concatenate([np.stack([u, v, z], 1), np.stack([z, u, v], 1), np.stack([u, z, v], 1)])
    nrm = np.concatenate([np.tile([0.0, 0.0, 1.0], (u.size, 1)), np.tile([1.0, 0.0, 0.0], (u.size, 1)),
                          np.tile([0.0, 1.0, 0.0], (u.size, 1))])
    return pts.astype(np.float32), nrm.astype(np.float32)


@pytest.mark.parametrize("method", ["plane", "point"])
def test_step_ref_recovers_a_small_motion_on_exact_pairs(method):
    """Source = the corner moved by the inverse of a 1 degree / 1 cm motion about its centre, pairs within 5 cm: every
    source point finds its own counterpart (the lattice is 10 cm wide, the motion moves a point by less than 3 cm).
    Measured on the CPU against the true motion, (rotation in rad, centre in m): after ONE step plane (1.1e-6, 4.6e-5),
    point (2.2e-5, 8.3e-5), what the linearisation leaves of a 1.7e-2 rad rotation; after the loop's convergence at tol
    1e-9, 3 steps, plane (1.7e-11, 6.5e-11), point (3.4e-9, 1.1e-9), the fp32 rounding of the moved source.  The bounds
    are those figures times 10."""
    tgt, nrm = _corner()
    centre = tgt.astype(np.float64).mean(0)
    shift = 0.01 * np.array([1.0, -2.0, 0.5]) / np.linalg.norm([1.0, -2.0, 0.5])
    truth = rr.motion_about(centre, (0.3, -0.5, 0.8), np.deg2rad(1.0), shift)
    src = rr.move(np.linalg.inv(truth), tgt)
    one = rr.step_ref(np.eye(4), src, tgt, nrm, 0.05, method)
    assert np.array_equal(one["index"], np.arange(tgt.shape[0]))
    assert one["c"] == tgt.shape[0] and one["status"] == 0
    rot, pos = rr.pose_errors(one["pose"], truth, centre)
    print(method, "one step:", rot, pos)
    bound = {"plane": (1.1e-5, 4.6e-4), "point": (2.2e-4, 8.3e-4)}[method]
    assert rot <= bound[0] and pos <= bound[1]
    pose, steps, status, _ = rr.icp_ref(src, tgt, nrm, None, 0.05, 30, 1e-9, method)
    rot, pos = rr.pose_errors(pose, truth, centre)
    print(method, "loop:", steps, status, rot, pos)
    bound = {"plane": (1.7e-10, 6.5e-10), "point": (3.4e-8, 1.1e-8)}[method]
    assert status == 1 and steps <= 5
    assert rot <= bound[0] and pos <= bound[1]


def test_step_ref_flags_a_degenerate_system():
    tgt, nrm = _corner()
    face = slice(0, 100)                                  # one plane: the rotation about its normal is free
    s = rr.step_ref(np.eye(4), tgt[face], tgt[face], nrm[face], 0.05, "plane")
    assert s["c"] == 100 and s["status"] == 2 and np.array_equal(s["pose"], np.eye(4))
    s = rr.step_ref(np.eye(4), tgt[:5], tgt, nrm, 0.05, "plane")
    assert s["c"] == 5 and s["status"] == 2               # fewer than 6 pairs


def test_apply_pose_round_trips_and_rotates_normals():
    from detection_3d_amd.register import apply_pose, inverse_pose
    rs = np.random.RandomState(1)
    pose = torch.from_numpy(rr.motion_about((13.0, -4.0, 1.0), (0.2, 0.1, 0.9), 0.4, (0.3, -0.2, 0.1)))
    nrm = rs.randn(200, 3)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    pcl = torch.from_numpy(np.concatenate([rs.rand(200, 3) * 2 + np.array([13.0, -4.0, 1.0]), rs.rand(200, 3), nrm],
                                          1).astype(np.float32))
    moved = apply_pose(pcl, pose)
    assert moved.dtype == torch.float32 and moved.shape == pcl.shape and moved.data_ptr() != pcl.data_ptr()
    R, t = pose[:3, :3], pose[:3, 3]
    assert torch.equal(moved[:, :3], (pcl[:, :3].double() @ R.T + t).float())
    assert torch.equal(moved[:, 3:6], pcl[:, 3:6])                               # colour stays
    assert torch.equal(moved[:, 6:9], (pcl[:, 6:9].double() @ R.T).float())
    assert float((moved[:, 6:9].double().norm(dim=1) - 1).abs().max()) < 1e-6
    back = apply_pose(moved, inverse_pose(pose))
    # two roundings to fp32 at coordinates below 16 m: 2 * 2^-24 * 16 = 1.9e-6 m per axis, and as much again through R
    assert float((back[:, :3] - pcl[:, :3]).abs().max()) < 4e-6
    assert float((back[:, 6:9] - pcl[:, 6:9]).abs().max()) < 3e-7
    assert torch.allclose(inverse_pose(pose) @ pose, torch.eye(4, dtype=torch.float64), atol=1e-14)
    six = apply_pose(pcl[:, :6], pose)                                           # no normal columns: only xyz moves
    assert torch.equal(six[:, :3], moved[:, :3]) and torch.equal(six[:, 3:], pcl[:, 3:6])
    keep = apply_pose(pcl, pose, normal_col=None)
    assert torch.equal(keep[:, 6:9], pcl[:, 6:9])
    with pytest.raises(ValueError):
        apply_pose(pcl, torch.eye(3))
    with pytest.raises(ValueError):
        apply_pose(pcl[:, 0], pose)
    with pytest.raises(ValueError):
        apply_pose(pcl, pose, normal_col=8)


def test_argument_errors_come_before_any_gpu_call():
    from detection_3d_amd._lib import D3DError
    from detection_3d_amd.register import icp, merge_scans, nearest
    a = torch.zeros((10, 3))
    for kw in (dict(radius=0.0), dict(radius=float("nan")), dict(radius="wide")):
        with pytest.raises(ValueError):
            nearest(a, a, **kw)
    with pytest.raises(ValueError):
        nearest(a[:, :2], a)
    for kw in (dict(max_dist=-1.0), dict(iterations=0), dict(iterations=2.5), dict(iterations=10 ** 6), dict(tol=-1e-6),
               dict(tol=float("inf")), dict(method="colour"), dict(init=torch.eye(3)), dict(init=torch.full((4, 4), float("nan"))),
               dict(init=torch.ones(4, 4)), dict(max_nn=2), dict(normal_radius=0.0)):
        with pytest.raises(ValueError):
            icp(a, a, **kw)
    with pytest.raises(ValueError):
        icp(a, a[:, :2])
    with pytest.raises(ValueError):
        merge_scans([])
    with pytest.raises(ValueError):
        merge_scans([a, a], reference=2)
    with pytest.raises(ValueError):
        merge_scans([a, a], init_poses=[None])
    with pytest.raises(ValueError):
        merge_scans([a, a], colour=True)
    with pytest.raises(ValueError):
        merge_scans([a, torch.zeros((4, 6))])
    # CPU tensors: no fallback
    with pytest.raises(D3DError):
        nearest(a, a)
    with pytest.raises(D3DError):
        icp(a, a)
    with pytest.raises(D3DError):
        icp(a, a, method="point")
