"""What tests/test_planes_gpu.py rests on, checked without a GPU: on every cloud whose GPU labelling is compared with the
reference, the reference's tightened and loosened labellings agree (a condition, so that no GPU test can pass by leaving
cases out); what the reference finds in the room; argument validation of detection_3d_amd.planes before any GPU call."""
import numpy as np
import pytest
import torch

from tests import planes_ref


@pytest.mark.parametrize("name", sorted(planes_ref.CASES))
def test_the_two_labellings_of_the_reference_agree(name):
    (l0, s0), (l1, s1) = planes_ref.case(name)[5:7]
    assert np.array_equal(l0, l1) and np.array_equal(s0, s1), name


def test_what_the_reference_finds_in_the_clouds():
    def patches(name):
        return planes_ref.case(name)[5]
    assert np.unique(patches("sheets")[0]).size == 2 and np.unique(patches("sheets_wide")[0]).size == 1
    assert np.unique(patches("fold8")[0]).size == 1 and np.unique(patches("fold30")[0]).size == 2
    assert np.unique(patches("chains")[0]).size == 2 and (patches("chains_half")[1] == 1).all()
    assert (patches("dense")[1] == 1500).all()
    l, s = patches("bad")
    n0 = planes_ref.BAD_SHEET
    assert (l[:n0] == 0).all() and np.array_equal(l[n0:n0 + 8], np.arange(n0, n0 + 8))
    assert l[n0 + 8] == l[n0 + 9] == n0 + 8 and s[n0 + 9] == 2
    for n in (1, 2, 63, 64, 65):
        assert (patches(f"line{n}")[1] == n).all()


@pytest.mark.parametrize("seed", [0, 1])
def test_purity_and_coverage_of_the_reference_in_the_room(seed):
    xyz, nrm, face = planes_ref.make_room(12000, seed)
    assert np.array_equal(xyz, planes_ref.case(f"room{seed}")[0])
    label, size = planes_ref.case(f"room{seed}")[5]
    pairs = planes_ref.edges_ref(xyz, nrm, 0.1, 10.0, 0.02)[0]
    assert 30000 <= pairs.shape[0] <= 45000
    for head in np.unique(label[size >= 20]):                   # every patch of 20 or more points lies in one face
        assert np.unique(face[label == head]).size == 1, head
    cover = []
    for f in range(7):                                          # the largest patch of a face holds most of the face
        rows = face == f
        cover.append(np.unique(label[rows], return_counts=True)[1].max() / rows.sum())
    print(f"room {seed}: {pairs.shape[0]} pairs, {np.unique(label).size} patches, coverage {np.round(cover, 3)}")
    assert min(cover) >= 0.9
    pop, heads = planes_ref.plane_lists_ref(label, size, 100)
    assert heads.size == 7 and np.unique(face[pop >= 0]).size == 7


def test_plane_lists_of_the_reference():
    label = np.int32([0, 0, 2, 2, 2, 5, 0])
    size = np.int32([3, 3, 3, 3, 3, 1, 3])
    pop, heads = planes_ref.plane_lists_ref(label, size, 2)
    assert heads.tolist() == [0, 2] and pop.tolist() == [0, 0, 1, 1, 1, -1, 0]
    pop, heads = planes_ref.plane_lists_ref(label, size, 1, cap=2)           # ties to the lower label
    assert heads.tolist() == [0, 2] and pop.tolist() == [0, 0, 1, 1, 1, -1, 0]


def test_bad_arguments_raise_before_any_gpu_call():
    from detection_3d_amd._lib import D3DError
    from detection_3d_amd.planes import fit_planes, label_planes, segment_planes
    xyz, nrm = torch.zeros((4, 3)), torch.zeros((4, 3))
    for kw in ({"radius": 0.0}, {"radius": float("inf")}, {"radius": "wide"}, {"angle": -1.0}, {"angle": 90.5},
               {"angle": float("nan")}, {"offset": -0.01}, {"offset": float("inf")}, {"offset": float("nan")}):
        with pytest.raises(ValueError):
            segment_planes(xyz, nrm, **kw)
    with pytest.raises(D3DError):
        segment_planes(xyz, nrm)
    with pytest.raises(D3DError):
        fit_planes(xyz, torch.zeros(4, dtype=torch.int32), torch.ones(4, dtype=torch.int32))
    for min_points in (0, -3, 2.5, True, "many"):
        with pytest.raises(ValueError):
            fit_planes(xyz, torch.zeros(4, dtype=torch.int32), torch.ones(4, dtype=torch.int32), min_points)
    with pytest.raises(ValueError):
        segment_planes(torch.zeros((4, 2)), nrm)
    with pytest.raises(ValueError):
        label_planes(xyz, tilt=91.0)
    with pytest.raises(ValueError):
        label_planes(torch.zeros((4, 6)))                       # normals=None needs nine columns
    with pytest.raises(D3DError):
        label_planes(torch.zeros((4, 9)))


def test_cos_min_is_rounded_once():
    import math
    from detection_3d_amd.planes import cos_min
    assert cos_min(0.0) == 1.0 and 0.0 < cos_min(90.0) < 1e-16
    assert cos_min(10.0) == float(np.float32(math.cos(10.0 * math.pi / 180.0)))


def test_the_planes_spec_of_label_scene():
    from detection_3d_amd.planes import parse_planes
    assert parse_planes(None) is None
    default = {"radius": 0.1, "angle": 10.0, "offset": 0.02, "min_points": 100}
    assert parse_planes("") == default and parse_planes(" ") == default
    assert parse_planes("0.05") == dict(default, radius=0.05)
    assert parse_planes("0.2,15,0.03,250") == {"radius": 0.2, "angle": 15.0, "offset": 0.03, "min_points": 250}
    assert parse_planes(",,0.05") == dict(default, offset=0.05)
    for bad in ("0.1,10,0.02,100,7", "wide", "0.1,100", "0.1,10,-1", "0.1,10,0.02,0", "0.1,10,0.02,2.5", "-1"):
        with pytest.raises(ValueError):
            parse_planes(bad)
