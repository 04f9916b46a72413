"""fit_boxes without a GPU: the numpy restatement of its definition (tests/fit_ref.py) recovers rectangles and does not
depend on the order of the rows; scene_io.yx_zb_to_standard inverts standard_to_yx_zb; argument checks that fail before
any device call."""
import math

import numpy as np
import pytest
import torch

from tests.fit_ref import FINE_STEP, box_points, fit_boxes_ref, fit_one, random_rectangle, yaw_distance


def test_restatement_recovers_random_rectangles():
    """corners plus up to 300 interior points of 400 wall-like boxes (thickness 0.05-0.4 m, length 0.5-12 m, centres up to
    60 m).  The best candidate lies within half a fine step of the box's yaw; the bound is one step (doubled for the fp32
    rotations), and the thickness may grow by the length times that angle plus 1e-4 m of fp32 rounding at 60 m."""
    rng = np.random.RandomState(0)
    worst_yaw = worst_d3 = 0.0
    for _ in range(400):
        b = random_rectangle(rng)
        p = box_points(rng, b, rng.randint(0, 300))
        got = fit_one(p[rng.permutation(len(p))].astype(np.float32))[0].astype(np.float64)
        dyaw = float(yaw_distance(got[6], b[6]))
        worst_yaw, worst_d3 = max(worst_yaw, dyaw), max(worst_d3, abs(got[3] - b[3]))
        assert dyaw <= 4.8e-5, (b, got)
        assert abs(got[3] - b[3]) <= b[4] * 4.8e-5 + 1e-4, (b, got)
        assert abs(got[4] - b[4]) <= 1e-3 and np.abs(got[[0, 1]] - b[[0, 1]]).max() <= 1e-3
        assert abs(got[2] - b[2]) <= 1e-6 and abs(got[5] - b[5]) <= 1e-6
        assert got[3] <= got[4] and -math.pi / 2 <= got[6] < math.pi / 2
    print(f"worst yaw error {worst_yaw:.3g} rad (step {FINE_STEP:.3g}), worst thickness error {worst_d3:.3g} m")


def test_restatement_does_not_depend_on_the_order_of_the_rows():
    rng = np.random.RandomState(1)
    pts, ids = [], []
    for g in range(12):
        p = box_points(rng, random_rectangle(rng), rng.randint(0, 200))
        pts.append(p)
        ids.append(np.full(len(p), g))
    xyz, inst = np.concatenate(pts).astype(np.float32), np.concatenate(ids)
    free = rng.uniform(size=13) < 0.7
    want = fit_boxes_ref(xyz, inst, 13, free)
    perm = rng.permutation(len(xyz))
    got = fit_boxes_ref(xyz[perm], inst[perm], 13, free)
    for w, g in zip(want, got):
        assert w.tobytes() == g.tobytes()
    assert want[1][12] == 0 and (want[2][12] == -1).all() and not want[0][12].any()
    assert np.array_equal(want[2][:12][~free[:12]], np.tile([0, 128], ((~free[:12]).sum(), 1)))
    assert (want[0][~free, 6] == 0).all()


def _ulp(v):
    return float(np.spacing(np.float32(v)))


def test_yx_zb_to_standard_inverts_standard_to_yx_zb():
    from detection_3d_amd.scene_io import set_yaw_zero, standard_to_yx_zb, yx_zb_to_standard
    rng = np.random.RandomState(2)
    b = np.stack([rng.uniform(-80, 80, 500), rng.uniform(-80, 80, 500), rng.uniform(-3, 3, 500),
                  rng.uniform(0.05, 0.4, 500), rng.uniform(0.5, 12, 500), rng.uniform(0.1, 3, 500),
                  rng.uniform(-math.pi / 2, math.pi / 2, 500)], 1).astype(np.float32)
    b[0, 6], b[1, 6], b[2, 6] = -np.float32(math.pi / 2), np.nextafter(np.float32(math.pi / 2), np.float32(0)), 0.0
    std = yx_zb_to_standard(b)
    assert std.dtype == np.float32 and std.shape == (500, 7)
    assert np.array_equal(std[:, 3], b[:, 4]) and np.array_equal(std[:, 4], b[:, 3])      # x size = length, y size = thickness
    assert (std[:, 6] >= 0).all() and (std[:, 6] <= np.float32(math.pi)).all()
    back = standard_to_yx_zb(std)
    assert np.array_equal(back[:, [0, 1, 3, 4, 5]], b[:, [0, 1, 3, 4, 5]])
    for r, w in zip(back.astype(np.float64), b.astype(np.float64)):
        assert abs(r[2] - w[2]) <= 2 * _ulp(max(abs(w[2]), w[5]))
        assert float(yaw_distance(r[6], w[6])) <= 2 * _ulp(math.pi)
    # fixed-yaw boxes (floor, ceiling, room): yaw 0 comes back as 0 and set_yaw_zero leaves the sizes where they were
    fixed = b.copy()
    fixed[:, 6] = 0
    fixed[:, [3, 4]] = b[:, [4, 3]]                        # sizes along x and y in any order
    again = set_yaw_zero(standard_to_yx_zb(yx_zb_to_standard(fixed)))
    assert np.array_equal(again[:, [0, 1, 3, 4, 5, 6]], fixed[:, [0, 1, 3, 4, 5, 6]])


def test_fit_boxes_checks_its_arguments_before_any_device_call():
    from detection_3d_amd import primitives as P
    xyz, inst = torch.zeros(6, 3), torch.zeros(6, dtype=torch.int64)
    for bad_xyz in (torch.zeros(6, 2), torch.zeros(6), "cloud"):
        with pytest.raises(ValueError):
            P.fit_boxes(bad_xyz, inst, k=1)
    for bad_inst in (torch.zeros(6), torch.zeros(5, dtype=torch.int64), torch.zeros(6, 1, dtype=torch.int32),
                     torch.zeros(6, dtype=torch.bool), [0] * 6):
        with pytest.raises(ValueError):
            P.fit_boxes(xyz, bad_inst, k=1)
    for bad_k in (-1, P.MAX_BOXES + 1):
        with pytest.raises(ValueError):
            P.fit_boxes(xyz, inst, k=bad_k)
    for bad_free in (torch.ones(2, dtype=torch.bool), torch.ones(1), torch.ones(1, 1, dtype=torch.bool)):
        with pytest.raises(ValueError):
            P.fit_boxes(xyz, inst, k=1, yaw_free=bad_free)
    with pytest.raises(ValueError):
        P.fit_boxes(xyz.double(), inst, k=1)
    for bad_origin in ("max", (0.0, 1.0)):
        with pytest.raises(ValueError):
            P.fit_boxes(xyz, inst, k=1, origin=bad_origin)
    assert P.FIT_CHUNK % 256 == 0 and P.FIT_CHUNK >= 256


def test_targets_from_labels_checks_its_arguments_before_any_device_call():
    from detection_3d_amd import primitives as P
    xyz, inst = torch.zeros(6, 9), torch.zeros(6, dtype=torch.int64)
    labels = torch.ones(1, dtype=torch.int64)
    for bad in ({"min_size": (0, 0)}, {"min_size": (0, 0, -1)}, {"min_size": 0.1}, {"min_size": (0, 0, float("inf"))},
                {"min_points": -1}):
        with pytest.raises(ValueError):
            P.targets_from_labels(xyz, inst, labels, **bad)
    for bad_labels in (torch.ones(1), torch.ones(1, 1, dtype=torch.int64), torch.ones(P.MAX_BOXES + 1, dtype=torch.int64)):
        with pytest.raises(ValueError):
            P.targets_from_labels(xyz, inst, bad_labels)


def test_fit_boxes_refuses_cpu_tensors():
    from detection_3d_amd._lib import D3DError
    from detection_3d_amd.primitives import fit_boxes, targets_from_labels
    xyz, inst = torch.zeros(6, 3), torch.zeros(6, dtype=torch.int64)
    with pytest.raises(D3DError):
        fit_boxes(xyz, inst, k=1)
    with pytest.raises(D3DError):
        fit_boxes(xyz, inst)
    with pytest.raises(D3DError):
        targets_from_labels(xyz, inst, torch.ones(1, dtype=torch.int64), classes=["background", "wall", "floor"])


def test_preparation_checks_fit():
    from detection_3d_amd.prepare import Preparation
    from detection_3d_amd.primitives import MIN_POINTS_ANY
    assert Preparation().fit == {"min_points": MIN_POINTS_ANY, "min_size": (0.0, 0.0, 0.0)}
    chain = Preparation(fit={"min_size": (0.1, 0, 0.5)})
    assert chain.fit == {"min_points": MIN_POINTS_ANY, "min_size": (0.1, 0.0, 0.5)}
    assert Preparation(fit={"min_points": 3}).fit["min_points"] == 3
    assert not chain.targets_in_file_frame               # fitting alone moves no frame
    for bad in ({"min_pts": 3}, {"min_points": -1}, {"min_size": (1, 2)}, {"min_size": (0, 0, -0.1)}, 5, "fit"):
        with pytest.raises(ValueError):
            Preparation(fit=bad)
