"""What the TSDF definition (tests/tsdf_ref.py) gives on the analytic room of tests/unproject_ref.py, and the
argument checks of detection_3d_amd.tsdf.  No GPU.

A prototype of the definition on room_scene(96, 128) with voxel 0.1, trunc 0.4 and origin (-0.5, -0.5, -0.5) gave 7788
rows, every one within 0.30 voxel of a face, a normal on 97 % of them and, on the rows farther than 3 voxels from the
second-nearest face, an inward normal component >= 0.93; the bounds below leave a margin over those figures."""
import math

import numpy as np
import pytest
import torch

from tests.tsdf_ref import ROOM, TsdfRef, room_frames
from tests.unproject_ref import room_face_distance, unproject_ref

VOXEL, TRUNC, ORIGIN = 0.1, 0.4, (-0.5, -0.5, -0.5)


@pytest.fixture(scope="module")
def room():
    depth, intr, extr = room_frames(96, 128)
    ref = TsdfRef(VOXEL, TRUNC, ORIGIN, color=False).integrate(depth, intr, extr)
    return depth, intr, extr, ref.surface_points(9)


def test_surface_lies_on_the_faces(room):
    rows, voxels, has = room[3]
    assert rows.shape[0] > 5000 and voxels.shape == (rows.shape[0], 3)
    d = room_face_distance(rows[:, :3]) / VOXEL
    print(f"{rows.shape[0]} rows, farthest from a face {d.max():.3f} voxel")
    assert d.max() <= 0.5


def test_normals_are_unit_or_zero_and_point_inwards(room):
    rows, _, has = room[3]
    n = rows[:, 6:9].astype(np.float64)
    length = np.linalg.norm(n, axis=1)
    assert (np.abs(length[has] - 1.0) <= 1e-6).all()
    assert (rows[~has, 6:9] == 0).all()
    print(f"{has.mean():.4f} of the rows have a normal")
    assert has.mean() >= 0.9
    # away from the room's edges (more than 3 voxels from the second-nearest face) the normal is the face's, inwards
    xyz = rows[:, :3].astype(np.float64)
    dist = np.concatenate([np.abs(xyz), np.abs(xyz - ROOM)], 1)            # to the faces x=0, y=0, z=0, x=4, y=3, z=2.5
    face = dist.argmin(1)
    away = has & (np.sort(dist, 1)[:, 1] > 3 * VOXEL)
    inward = np.where(face < 3, 1.0, -1.0) * n[np.arange(len(n)), face % 3]
    print(f"{int(away.sum())} rows away from edges, smallest inward component {inward[away].min():.3f}")
    assert away.sum() > 3000 and (inward[away] >= 0.85).all()


def _project(points, intr, extr):
    """camera-frame depth and pixel of world points [N, 3] in one frame"""
    d = points - extr[:, 3]
    c = d @ extr[:, :3]
    with np.errstate(all="ignore"):
        return c[:, 2], np.floor(c[:, 0] * intr[0] / c[:, 2] + intr[2] + 0.5), np.floor(c[:, 1] * intr[1] / c[:, 2] + intr[3] + 0.5)


def test_free_space_outvotes_a_wrong_measurement(room):
    """A patch of one frame reads 1.0 m where two or more other frames look straight through: the volume has no surface
    there, the plain unprojection of the same frames keeps the points."""
    depth, intr, extr, _ = room
    F, H, W = depth.shape
    size, found = 6, None
    for f in range(F):
        for v0 in range(0, H - size, size):
            for u0 in range(0, W - size, size):
                if not (depth[f, v0:v0 + size, u0:u0 + size] > 1.0 + 2 * TRUNC).all():
                    continue
                v, u = np.mgrid[v0:v0 + size, u0:u0 + size]
                cam = np.stack([(u.ravel() - intr[f, 2]) / intr[f, 0], (v.ravel() - intr[f, 3]) / intr[f, 1],
                                np.ones(size * size)], 1) * 1.0
                pts = cam @ extr[f, :, :3].T + extr[f, :, 3]
                votes = np.zeros(len(pts), int)
                for o in range(F):
                    if o == f:
                        continue
                    z, pu, pv = _project(pts, intr[o], extr[o])
                    inside = (z > 0) & (pu >= 2) & (pu < W - 2) & (pv >= 2) & (pv < H - 2)
                    seen = depth[o][np.where(inside, pv, 0).astype(int), np.where(inside, pu, 0).astype(int)]
                    votes += inside & (seen - z > 2 * TRUNC)               # in front of what that frame sees, by a margin
                if (votes >= 2).all():
                    found = (f, v0, u0, pts)
                    break
            if found:
                break
        if found:
            break
    assert found, "no patch of the room is crossed by two other frames' free space"
    f, v0, u0, pts = found
    wrong = depth.copy()
    wrong[f, v0:v0 + size, u0:u0 + size] = 1.0
    rows, _, _ = TsdfRef(VOXEL, TRUNC, ORIGIN, color=False).integrate(wrong, intr, extr).surface_points(3)
    gap = np.linalg.norm(rows[:, None, :3].astype(np.float64) - pts[None], axis=2).min()
    cloud, _, _ = unproject_ref(wrong, intr, extr, columns=3)
    kept = np.linalg.norm(cloud[:, None, :3].astype(np.float64) - pts[None], axis=2).min(0)
    print(f"patch of frame {f} at ({v0}, {u0}): nearest surface row {gap / VOXEL:.2f} voxel away; the unprojection has a "
          f"point within {kept.max():.2e} m of each")
    assert gap > 2 * VOXEL
    assert kept.max() < 1e-5
    # and it is the other frames that remove it: the wrong frame alone puts a surface through the patch
    alone, _, _ = TsdfRef(VOXEL, TRUNC, ORIGIN, color=False).integrate(wrong[f:f + 1], intr[f:f + 1],
                                                                       extr[f:f + 1]).surface_points(3)
    assert np.linalg.norm(alone[:, None, :3].astype(np.float64) - pts[None], axis=2).min(0).max() < VOXEL


def test_argument_checks_raise_value_error():
    from detection_3d_amd.tsdf import TsdfVolume, fuse_frames_tsdf
    for kw in (dict(voxel=0.0), dict(voxel=math.nan), dict(voxel="x"), dict(trunc=0.0), dict(trunc=-1.0),
               dict(trunc=math.inf), dict(voxel=0.01, trunc=10.0), dict(origin=(0, 0)), dict(origin=(0, 0, math.nan)),
               dict(origin=3.0), dict(max_blocks=0), dict(max_blocks=1.5), dict(max_blocks=(1 << 22) + 1),
               dict(max_blocks=True)):
        with pytest.raises(ValueError):
            TsdfVolume(**kw)
    vol = TsdfVolume(0.05, origin=(1, 2, 3))
    assert vol.trunc == 4 * 0.05 and vol.origin == (1.0, 2.0, 3.0) and vol.n_blocks == 0 and not vol.clipped
    for kw in (dict(step=0), dict(step=1.5), dict(min_depth=math.nan), dict(max_depth=math.nan), dict(color_div=0.0),
               dict(color_div=math.inf)):
        with pytest.raises(ValueError):
            vol.integrate(None, **kw)
        with pytest.raises(ValueError):
            fuse_frames_tsdf(None, **kw)
    with pytest.raises(ValueError, match="DepthFrames"):
        vol.integrate(torch.zeros(1, 4, 4))
    with pytest.raises(ValueError, match="DepthFrames"):
        TsdfVolume.around(torch.zeros(1, 4, 4))
    with pytest.raises(ValueError, match="DepthFrames"):
        fuse_frames_tsdf(torch.zeros(1, 4, 4))
    with pytest.raises(ValueError):
        fuse_frames_tsdf(None, batch=0)
    for kw in (dict(columns=4), dict(min_weight=-1), dict(min_weight=math.nan)):
        with pytest.raises(ValueError):
            vol.surface_points(**kw)


def test_cpu_tensors_raise_d3d_error():
    from detection_3d_amd._lib import D3DError
    from detection_3d_amd.tsdf import TsdfVolume
    from detection_3d_amd.unproject import DepthFrames
    with pytest.raises(D3DError):
        TsdfVolume(device="cpu")
    with pytest.raises(D3DError):                      # the frames are fine, and on the CPU
        DepthFrames(torch.ones(1, 4, 4), [4.0, 4.0, 1.5, 1.5], torch.eye(4)[None])
    vol = TsdfVolume()
    for call in (vol.surface_points, vol.blocks):      # nothing integrated: the volume has no GPU to answer from
        with pytest.raises(D3DError):
            call()
