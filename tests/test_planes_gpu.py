"""detection_3d_amd.planes (planes.hip) against the fp64 restatement of its semantics in tests/planes_ref.py.

Bounds.  Labels and sizes are integers: on every cloud of planes_ref.CASES the reference's tightened and loosened
labellings agree (tests/test_planes_cpu.py asserts it without a GPU), so the fp32 kernel must give exactly that labelling.
fit_planes: plane_of_point, count and the order of the planes are exact.  The moments are fp64 sums of m <= 1e5 terms
about an origin inside the patch, |dC| <~ m 2^-53 4 l2; with 3x for the solver the angle between the fitted and the
reference line is at most 1e-9 / gap, gap = (l1 - l0) / l2 (as in test_normals_gpu.py); the centroid is within 1e-12,
d within angle_bound |centroid| + 1e-12, rms within 1e-9 relative plus 1e-12; an eigenvalue moves by at most |dC| (Weyl):
1e-9 l2.  The boxes of label_planes' room lie within 5 cm of their faces: 2 mm of noise plus the point spacing."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import clean_ref, planes_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _segment(dev, xyz, nrm, radius, angle, offset):
    from detection_3d_amd.planes import segment_planes
    label, size = segment_planes(_gpu(dev, xyz), _gpu(dev, nrm), radius, angle, offset)
    assert label.dtype == torch.int32 and size.dtype == torch.int32 and label.shape == size.shape == (xyz.shape[0],)
    return label.cpu().numpy(), size.cpu().numpy()


@pytest.mark.parametrize("name", sorted(planes_ref.CASES))
def test_patches_equal_the_reference(dev, name):
    xyz, nrm, radius, angle, offset, (l0, s0), (l1, s1) = planes_ref.case(name)
    assert np.array_equal(l0, l1) and np.array_equal(s0, s1), f"{name}: the reference's two labellings differ"
    label, size = _segment(dev, xyz, nrm, radius, angle, offset)
    print(f"{name}: {xyz.shape[0]} points, {np.unique(l0).size} patches, largest {s0.max()}, label mismatches "
          f"{int((label != l0).sum())}, size mismatches {int((size != s0).sum())}")
    assert np.array_equal(label, l0) and np.array_equal(size, s0), name


def test_what_the_clouds_are_there_for(dev):
    def patches(name):
        xyz, nrm, radius, angle, offset = planes_ref.case(name)[:5]
        return _segment(dev, xyz, nrm, radius, angle, offset)
    l, s = patches("sheets")                                  # the offset test alone keeps the two sheets apart
    assert np.unique(l).size == 2 and (s == 1500).all()
    assert np.unique(patches("sheets_wide")[0]).size == 1
    assert np.unique(patches("fold8")[0]).size == 1 and np.unique(patches("fold30")[0]).size == 2
    l, s = patches("chains")                                  # a union 3000 deep
    assert np.unique(l).size == 2 and (s == 3000).all()
    l, s = patches("chains_half")
    assert np.array_equal(l, np.arange(6000)) and (s == 1).all()
    # the unstaged form is actually taken: every neighbourhood of the dense patch is past the staging budget
    assert clean_ref.neighbors_ref(planes_ref.case("dense")[0], 0.1)[0].min() > 1024
    assert (patches("dense")[1] == 1500).all()
    l, s = patches("bad")
    n0 = planes_ref.BAD_SHEET
    assert (l[:n0] == 0).all() and (s[:n0] == n0).all()                                  # the neighbours are unaffected
    assert np.array_equal(l[n0:n0 + 8], np.arange(n0, n0 + 8)) and (s[n0:n0 + 8] == 1).all()
    assert l[n0 + 8] == l[n0 + 9] == n0 + 8 and s[n0 + 8] == s[n0 + 9] == 2


def test_edge_sizes_and_a_strided_view(dev):
    from detection_3d_amd.planes import segment_planes
    label, size = segment_planes(torch.zeros((0, 3), device=dev), torch.zeros((0, 3), device=dev))
    assert label.shape == size.shape == (0,) and label.dtype == torch.int32
    xyz, nrm = planes_ref.case("room0")[:2]
    pcl = np.zeros((xyz.shape[0], 9), np.float32)
    pcl[:, :3], pcl[:, 6:9] = xyz, nrm
    pcl = _gpu(dev, pcl)
    a = segment_planes(pcl[:, :3], pcl[:, 6:9])
    b = segment_planes(_gpu(dev, xyz), _gpu(dev, nrm))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = segment_planes(pcl[:, :3], pcl[:, 6:9])                # two runs give the same bits
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    label, size, ms = segment_planes(pcl[:, :3], pcl[:, 6:9], phases=True)
    assert torch.equal(label, a[0]) and set(ms) == {"cells", "sort", "table", "search", "tail"}


@pytest.mark.parametrize("name", ["room0", "bad", "dense"])
def test_a_permutation_of_the_rows_gives_the_same_partition(dev, name):
    xyz, nrm, radius, angle, offset, (l0, s0), _ = planes_ref.case(name)
    n = xyz.shape[0]
    perm = np.random.RandomState(11).permutation(n)            # new row j holds old row perm[j]
    label, size = _segment(dev, xyz[perm], nrm[perm], radius, angle, offset)
    new_row = np.empty(n, np.int64)
    new_row[perm] = np.arange(n)
    first = np.full(n, n, np.int64)                            # per old label: the smallest new row of its patch
    np.minimum.at(first, l0, new_row)
    assert np.array_equal(label, first[l0[perm]]) and np.array_equal(size, s0[perm])


def test_a_right_angle_and_a_huge_offset_are_connected_components(dev):
    from detection_3d_amd.clean import connected_components
    from detection_3d_amd.planes import segment_planes
    for name in ("room0", "dense"):
        xyz, nrm = planes_ref.case(name)[:2]
        xyz, nrm = _gpu(dev, xyz), _gpu(dev, nrm)
        for radius in (0.05, 0.1):
            got = segment_planes(xyz, nrm, radius, 90.0, 1e30)
            want = connected_components(xyz, radius)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (name, radius)


# ---- fit_planes ----
def _angle(a, b):
    """between the lines of two unit vectors, from the cross product (no acos near 1)"""
    return np.arcsin(np.minimum(1.0, np.linalg.norm(np.cross(a, b), axis=-1)))


def _check_fit(planes, ref, what):
    normal, d, centroid = planes.normal.cpu().numpy(), planes.d.cpu().numpy(), planes.centroid.cpu().numpy()
    count, rms, eig = planes.count.cpu().numpy(), planes.rms.cpu().numpy(), planes.eigenvalues.cpu().numpy()
    assert planes.normal.dtype == planes.d.dtype == planes.rms.dtype == torch.float64 and planes.count.dtype == torch.int32
    assert np.array_equal(count, ref["count"])
    some = np.isfinite(ref["gap"])                             # the largest eigenvalue is positive
    ok = some & (ref["gap"] > 1e-3)                            # and there is a normal to find (not: two points, a line)
    assert ok.any()
    ang = _angle(normal[ok], ref["normal"][ok])
    bound = 1e-9 / ref["gap"][ok]
    dc = np.abs(centroid - ref["centroid"]).max()
    dd = np.abs(d - ref["d"])[ok] - bound * np.linalg.norm(ref["centroid"][ok], axis=1)
    rel = np.abs(rms - ref["rms"])[ok] / ref["rms"][ok]
    de = (np.abs(eig - ref["eigenvalues"])[some] / ref["eigenvalues"][some][:, 2:]).max()
    print(f"{what}: {int(ok.sum())} planes of up to {count.max()} points, worst angle x gap {np.max(ang * ref['gap'][ok]):.3e} "
          f"(bound 1e-9), centroid {dc:.3e} (1e-12), d beyond the angle's share {dd.max():.3e} (1e-12), rms relative "
          f"{rel.max():.3e} (1e-9), eigenvalues / l2 {de:.3e} (1e-9)")
    assert (ang <= bound).all() and dc <= 1e-12 and dd.max() <= 1e-12
    assert (np.abs(rms - ref["rms"])[ok] <= 1e-9 * ref["rms"][ok] + 1e-12).all() and de <= 1e-9
    assert (np.diff(eig, axis=1) >= 0).all()
    lead = np.take_along_axis(normal[ok], np.argmax(np.abs(normal[ok]), 1)[:, None], 1)        # the sign rule
    assert (lead > 0).all() and np.abs(np.linalg.norm(normal[ok], axis=1) - 1).max() <= 1e-14
    assert np.abs(np.linalg.norm(normal[some], axis=1) - 1).max() <= 1e-14
    flat = ~some & (count > 0)
    assert not normal[flat].any() and not d[flat].any() and not rms[flat].any() and not eig[flat].any()


@pytest.mark.parametrize("name,min_points", [("room0", 100), ("room1", 1)])
def test_fitted_planes_against_fsum_and_eigh(dev, name, min_points):
    from detection_3d_amd.planes import fit_planes, segment_planes
    xyz, nrm, radius, angle, offset, (l0, s0), _ = planes_ref.case(name)
    g = _gpu(dev, xyz)
    label, size = segment_planes(g, _gpu(dev, nrm), radius, angle, offset)
    planes = fit_planes(g, label, size, min_points)
    pop, heads = planes_ref.plane_lists_ref(l0, s0, min_points)
    assert planes.plane_of_point.dtype == torch.int32 and np.array_equal(planes.plane_of_point.cpu().numpy(), pop)
    assert planes.normal.shape == (heads.size, 3) and (heads.size == 7 if name == "room0" else heads.size > 7)
    _check_fit(planes, planes_ref.fit_ref(xyz, pop, heads.size), name)
    again = fit_planes(g, label, size, min_points)
    for a, b in zip(planes, again):                            # the same bits
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                           b.view(torch.int64) if b.dtype == torch.float64 else b)


def test_a_tilted_plane_a_single_point_and_coincident_points(dev):
    from detection_3d_amd.planes import fit_planes
    rs = np.random.RandomState(4)
    m = 3000                                                    # three chunks of the moments' launch
    uv = rs.rand(m, 2)
    nv = np.array([-0.6, 0.48, -0.64])                          # its largest component is negative: the sign is turned
    e1 = np.cross(nv, [0, 0, 1.0])
    e1 /= np.linalg.norm(e1)
    tilted = uv[:, :1] * e1 + uv[:, 1:] * np.cross(nv, e1) + rs.randn(m, 1) * 0.003 * nv + np.array(planes_ref.SHIFT)
    xyz = np.concatenate([tilted, [[1.5, 2.5, 3.5]], np.tile([[7.25, -1.5, 0.125]], (5, 1))]).astype(np.float32)
    label = np.concatenate([np.zeros(m), [m], np.full(5, m + 1)]).astype(np.int32)
    size = np.concatenate([np.full(m, m), [1], np.full(5, 5)]).astype(np.int32)
    planes = fit_planes(_gpu(dev, xyz), _gpu(dev, label), _gpu(dev, size), min_points=1)
    pop, heads = planes_ref.plane_lists_ref(label, size, 1)
    assert heads.tolist() == [0, m, m + 1] and np.array_equal(planes.plane_of_point.cpu().numpy(), pop)
    ref = planes_ref.fit_ref(xyz, pop, 3)
    assert np.isinf(ref["gap"][1:]).all()
    _check_fit(planes, ref, "tilted")
    n0 = planes.normal[0].cpu().numpy()
    assert n0[2] > 0 and _angle(n0, -nv) < 1e-3
    assert planes.count.tolist() == [m, 1, 5]
    assert np.array_equal(planes.centroid[1:].cpu().numpy(), xyz[[m, m + 1]].astype(np.float64))
    assert fit_planes(_gpu(dev, xyz), _gpu(dev, label), _gpu(dev, size), min_points=2).count.tolist() == [m, 5]
    none = fit_planes(_gpu(dev, xyz), _gpu(dev, label), _gpu(dev, size), min_points=m + 1)
    assert none.normal.shape == (0, 3) and (none.plane_of_point == -1).all()


def test_more_patches_than_planes(dev):
    from detection_3d_amd.planes import MAX_PLANES, fit_planes
    rs = np.random.RandomState(6)
    small, big = 4200, 10                                       # patches of 3 points, then patches of 4
    n = 3 * small + 4 * big
    xyz = rs.rand(n, 3).astype(np.float32)
    label = np.concatenate([np.repeat(np.arange(small) * 3, 3), 3 * small + np.repeat(np.arange(big) * 4, 4)]).astype(np.int32)
    size = np.concatenate([np.full(3 * small, 3), np.full(4 * big, 4)]).astype(np.int32)
    perm = rs.permutation(n)                                    # patches scattered over the rows
    new_row = np.empty(n, np.int64)
    new_row[perm] = np.arange(n)
    first = np.full(n, n, np.int64)
    np.minimum.at(first, label, new_row)
    label, size, xyz = first[label[perm]].astype(np.int32), size[perm], xyz[perm]
    planes = fit_planes(_gpu(dev, xyz), _gpu(dev, label), _gpu(dev, size), min_points=3)
    pop, heads = planes_ref.plane_lists_ref(label, size, 3)
    assert heads.size == MAX_PLANES == planes.normal.shape[0]
    assert np.array_equal(planes.plane_of_point.cpu().numpy(), pop)
    assert (pop[size == 4] >= 0).all() and (pop < 0).sum() == 3 * (small + big - MAX_PLANES)    # the largest stay
    count = planes.count.cpu().numpy()
    assert np.array_equal(count, size[heads])
    ref = planes_ref.fit_ref(xyz, pop, 64)                      # the first planes are enough for the values
    assert np.abs(planes.centroid[:64].cpu().numpy() - ref["centroid"]).max() <= 1e-12


# ---- labels for an unlabelled scan ----
def _room_cloud(dev, extra=None):
    xyz, nrm = planes_ref.case("room0")[:2]
    pcl = np.zeros((xyz.shape[0], 9), np.float32)
    pcl[:, :3], pcl[:, 6:9] = xyz, nrm
    if extra is not None:
        pcl = np.concatenate([pcl, extra])
    return _gpu(dev, pcl)


def test_label_planes_on_the_room(dev):
    from detection_3d_amd.config import class_to_label, get_cfg
    from detection_3d_amd.planes import label_planes
    from detection_3d_amd.primitives import is_labelled, targets_from_labels
    cfg = get_cfg("6c_Fpn4321")
    c2l = class_to_label(cfg.INPUT.CLASSES)
    # a 45 degree ramp of 1 x 1 m inside the room, 2500 points: neither horizontal nor a wall
    rs = np.random.RandomState(8)
    st = rs.rand(2500, 2)
    ramp = np.zeros((2500, 9), np.float32)
    ramp[:, :3] = np.column_stack([0.5 + st[:, 0] * math.sqrt(0.5), 1.0 + st[:, 1], 0.5 + st[:, 0] * math.sqrt(0.5)]) + \
        np.array(planes_ref.SHIFT)
    ramp[:, 6:9] = [-math.sqrt(0.5), 0.0, math.sqrt(0.5)]
    pcl = _room_cloud(dev, ramp)
    tg = label_planes(pcl, classes=cfg.INPUT.CLASSES)
    assert is_labelled(tg) and tg["instance"].dtype == tg["instance_labels"].dtype == torch.int64
    assert tg["instance"].shape == (pcl.shape[0],) and tg["instance"].is_cuda
    ids = tg["instance_labels"].cpu().numpy()
    assert sorted(ids.tolist()) == sorted([c2l["floor"], c2l["ceiling"]] + [c2l["wall"]] * 5 + [0])
    ramp_plane = tg["instance"][-2500:].unique().tolist()
    assert len(ramp_plane) == 1 and ids[ramp_plane[0]] == 0
    same = label_planes(pcl[:, :3], pcl[:, 6:9].contiguous(), classes=cfg.INPUT.CLASSES)
    assert torch.equal(same["instance"], tg["instance"]) and torch.equal(same["instance_labels"], tg["instance_labels"])
    assert (label_planes(pcl, classes=["background", "wall"])["instance_labels"] <= c2l["wall"]).all()

    out = targets_from_labels(pcl, tg["instance"], tg["instance_labels"], classes=cfg.INPUT.CLASSES)
    boxes, labels = out["bbox3d"].cpu().numpy().astype(np.float64), out["labels"].cpu().numpy()
    assert boxes.shape == (7, 7)
    shift = np.array(planes_ref.SHIFT)
    worst = 0.0
    for f, (o, u, v, nv) in enumerate(planes_ref.room_faces()):
        o, u, v = np.asarray(o, float) + shift, np.asarray(u, float), np.asarray(v, float)
        mid = o + 0.5 * (u + v)
        j = int(np.argmin(np.linalg.norm(boxes[:, :2] - mid[:2], axis=1) + np.abs(boxes[:, 2] + 0.5 * boxes[:, 5] - mid[2])))
        b = boxes[j]
        if f < 2:                                               # floor, ceiling: yaw 0, sizes along x and y, no height
            assert labels[j] == c2l["floor" if f == 0 else "ceiling"] and b[6] == 0
            want = [mid[0], mid[1], o[2], u[0], v[1], 0.0]
        else:                                                   # a wall: thin, as long as the face, as high as the room
            assert labels[j] == c2l["wall"]
            want = [mid[0], mid[1], o[2], 0.0, np.linalg.norm(u), v[2]]
        err = np.abs(b[:6] - np.array(want)).max()
        worst = max(worst, err)
        assert err <= 0.05, (f, b, want)
    print(f"label_planes on the room: 7 boxes, worst distance of a centre or size from its face {worst:.4f} m (bound 0.05)")


def test_collate_takes_label_planes_targets(dev):
    from detection_3d_amd import engine
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.planes import label_planes
    cfg = get_cfg("6c_Fpn4321")
    pcl = _room_cloud(dev)
    tg = label_planes(pcl, classes=cfg.INPUT.CLASSES)
    points, targets = engine.collate([(pcl, tg)], cfg)
    assert points[2] == 1 and targets[0]["bbox3d"].shape == (7, 7) and sorted(targets[0]["labels"].tolist()) == [1] * 5 + [4, 5]      # wall, floor, ceiling


def test_label_scene_script_labels_a_cloud_without_instances(dev, tmp_path):
    from detection_3d_amd.scene_io import load_scene
    pcl = _room_cloud(dev).cpu().numpy()
    src, dst = str(tmp_path / "unlabelled.npz"), str(tmp_path / "scene.npz")
    np.savez(src, pcl=pcl)
    script = os.path.join(ROOT, "scripts", "label_scene.py")
    p = subprocess.run([sys.executable, script, src, dst, "--config", "6c_Fpn4321", "--planes=0.1,10,0.02,100"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got_pcl, std = load_scene(dst)
    assert np.array_equal(got_pcl, pcl) and {c: len(b) for c, b in std.items()} == {"wall": 5, "ceiling": 1, "floor": 1}
    np.savez(src, pcl=pcl, instance=np.zeros(pcl.shape[0], np.int32), instance_class=np.array(["wall"]))
    p = subprocess.run([sys.executable, script, src, dst, "--planes"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "instance" in p.stderr          # a labelled input keeps its own labels
