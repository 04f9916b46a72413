"""The mesh definition (tests/tsdf_mesh_ref.py) on an analytic sphere and on the analytic room, the library's
case table against the one derived here, and the argument checks of TsdfVolume.mesh, TsdfVolume.from_blocks and
fuse_frames_mesh.  No GPU.

Sphere: D = clip((|x - c| - r) / trunc, -1, 1) with r = 4.2 voxels, c at voxel (8.3, 8.6, 8.45), trunc = 4 voxels, over
the eight blocks (0..1)^3.  A vertex is the linear interpolation of a convex distance along an edge of length at most
sqrt(3) h, so it lies within 3 h^2 / (8 (r - sqrt(3) h)) = 0.152 voxel of the sphere; a prototype measured 0.089.

Room: tests/unproject_ref.py's room at 48 x 64 from four cameras, voxel 0.1, trunc 0.4.  DESIGN 6q's bound for the axis
edges is 0.5 voxel; with the diagonal edges included the restatement measures 0.494 voxel over the referenced vertices,
so 0.5 is asserted here too."""
import math

import numpy as np
import pytest
import torch

from tests.tsdf_mesh_ref import (SPHERE, SWAPPED, edge_census, euler_characteristic, mesh_ref, sphere_blocks,
                                 sphere_distance, table_array)
from tests.tsdf_ref import TsdfRef, room_frames
from tests.unproject_ref import room_face_distance

SPHERE_BOUND = 3.0 / (8.0 * (SPHERE["r"] - math.sqrt(3.0)))


def test_library_table_equals_the_derived_one():
    from detection_3d_amd._lib import lib
    got = np.full((6, 16, 13), 99, np.int8)
    assert lib().d3d_tsdf_mesh_table(got.ctypes.data) == 0
    want = table_array()
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    # the derivation agrees with the two lists the definition states
    assert sorted(m for (s, m), v in SWAPPED.items() if s > 0 and v) == [2, 5, 8, 10, 11, 14]
    assert sorted(m for (s, m), v in SWAPPED.items() if s < 0 and v) == [1, 3, 4, 6, 7, 9, 12, 13]
    assert want[:, 0, 0].tolist() == [0] * 6 and want[:, 15, 0].tolist() == [0] * 6
    assert sorted(want[0, 1:15, 0].tolist()) == [1] * 8 + [2] * 6


@pytest.fixture(scope="module")
def sphere():
    return mesh_ref(sphere_blocks(), 1.0, (0.0, 0.0, 0.0))


def test_sphere_is_a_closed_oriented_manifold(sphere):
    vertices, triangles, color, edges = sphere
    assert len(triangles) > 1000 and color.shape == vertices.shape and edges.shape == (len(vertices), 4)
    most, unpaired = edge_census(triangles)
    assert most == 1 and unpaired == 0             # every directed edge once, and its reverse once
    assert euler_characteristic(triangles) == 2


def test_sphere_vertices_lie_on_the_sphere_and_normals_point_outwards(sphere):
    vertices, triangles, _, _ = sphere
    d = sphere_distance(vertices[np.unique(triangles)])
    print(f"{len(vertices)} vertices, {len(triangles)} triangles, farthest from the sphere {d.max():.4f} voxel "
          f"(bound {SPHERE_BOUND:.4f})")
    assert d.max() <= SPHERE_BOUND
    tv = vertices[triangles].astype(np.float64)
    normal = np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0])
    outward = (normal * (tv.mean(1) - np.array(SPHERE["c"]))).sum(1)
    assert (outward >= 0).all()                    # no triangle faces the centre: D < 0 is inside the sphere


def test_kinds_0_to_2_are_the_surface_rows():
    blocks = sphere_blocks()
    ref = TsdfRef(1.0, SPHERE["trunc"], (0.0, 0.0, 0.0))
    ref.coords, ref.D, ref.W = blocks[0].astype(np.int64), blocks[1].reshape(8, 512), blocks[2].reshape(8, 512)
    ref.C, ref.CW = blocks[3].reshape(8, 512, 3), blocks[4].reshape(8, 512)
    rows, voxels, _ = ref.surface_points(6)
    vertices, _, color, edges = mesh_ref(blocks, 1.0, (0.0, 0.0, 0.0))
    axis = edges[:, 3] < 3
    assert np.array_equal(edges[axis, :3], voxels)
    assert np.array_equal(vertices[axis].view(np.uint32), rows[:, :3].view(np.uint32))
    assert np.array_equal(color[axis].view(np.uint32), rows[:, 3:6].view(np.uint32))


def test_room_vertices_lie_on_the_faces():
    depth, intr, extr = room_frames(48, 64)
    voxel, origin = 0.1, (-0.5, -0.5, -0.5)
    ref = TsdfRef(voxel, 0.4, origin, color=False).integrate(depth, intr, extr)
    coords, D, W, _, _ = ref.blocks()
    vertices, triangles, color, edges = mesh_ref((coords, D, W, None, None), voxel, origin)
    assert color is None and len(triangles) > 20000
    used = np.unique(triangles)
    d = room_face_distance(vertices[used]) / voxel
    print(f"{len(coords)} blocks, {len(vertices)} vertices ({len(vertices) - len(used)} unreferenced), {len(triangles)} "
          f"triangles, farthest referenced vertex from a face {d.max():.3f} voxel")
    assert d.max() <= 0.5
    assert edge_census(triangles)[0] == 1          # an open surface, but no directed edge twice


def test_argument_checks_raise_value_error():
    from detection_3d_amd.tsdf import TsdfVolume, fuse_frames_mesh
    vol = TsdfVolume(0.05)
    for kw in (dict(min_weight=-1), dict(min_weight=math.nan), dict(min_weight="x"), dict(min_weight=math.inf)):
        with pytest.raises(ValueError):
            vol.mesh(**kw)
        with pytest.raises(ValueError):
            fuse_frames_mesh(None, **kw)
    for kw in (dict(step=0), dict(min_depth=math.nan), dict(color_div=0.0), dict(batch=0), dict(voxel=0.0), dict(trunc=-1.0)):
        with pytest.raises(ValueError):
            fuse_frames_mesh(None, **kw)
    with pytest.raises(ValueError, match="DepthFrames"):
        fuse_frames_mesh(torch.zeros(1, 4, 4))
    with pytest.raises(TypeError):
        fuse_frames_mesh(None, max_points=3)

    coords = torch.tensor([[0, 0, 0], [0, 0, 1]], dtype=torch.int32)
    d, w = torch.zeros(2, 8, 8, 8), torch.ones(2, 8, 8, 8)
    c, cw = torch.zeros(2, 8, 8, 8, 3), torch.ones(2, 8, 8, 8)
    bad = [((coords.long(), d, w), {}), ((coords[:, :2], d, w), {}), ((coords.tolist(), d, w), {}),
           ((coords, d.double(), w), {}), ((coords, d[:1], w), {}), ((coords, d, w.reshape(2, 512)), {}),
           ((coords, d, w, c), {}), ((coords, d, w, None, cw), {}), ((coords, d, w, c[..., :2], cw), {}),
           ((coords, d, w, c, cw[:1]), {}), ((coords, d, w, c.half(), cw), {}),
           ((torch.tensor([[0, 0, 0], [0, 0, 0]], dtype=torch.int32), d, w), {}),               # twice
           ((torch.tensor([[0, 0, 0], [0, -1, 0]], dtype=torch.int32), d, w), {}),
           ((torch.tensor([[0, 0, 0], [65536, 0, 0]], dtype=torch.int32), d, w), {}),
           ((coords, d, w), dict(voxel=0.0)), ((coords, d, w), dict(trunc=math.nan)), ((coords, d, w), dict(origin=(0, 0))),
           ((coords, d, w), dict(max_blocks=1)), ((coords, d, w), dict(max_blocks=0)), ((coords, d, w), dict(max_blocks=2.5))]
    for args, kw in bad:
        with pytest.raises(ValueError):
            TsdfVolume.from_blocks(*args, **kw)
    if torch.cuda.is_available():
        with pytest.raises(ValueError):                # mixed devices: before any word about the CPU
            TsdfVolume.from_blocks(coords.cuda(), d, w.cuda())


def test_cpu_tensors_raise_d3d_error():
    from detection_3d_amd._lib import D3DError
    from detection_3d_amd.tsdf import TsdfVolume
    with pytest.raises(D3DError):                      # nothing integrated: the volume has no GPU to answer from
        TsdfVolume().mesh()
    coords = torch.tensor([[0, 0, 0], [0, 0, 1]], dtype=torch.int32)
    with pytest.raises(D3DError):                      # the blocks are fine, and on the CPU
        TsdfVolume.from_blocks(coords, torch.zeros(2, 8, 8, 8), torch.ones(2, 8, 8, 8))
    with pytest.raises(D3DError):
        TsdfVolume.from_blocks(coords[:0], torch.zeros(0, 8, 8, 8), torch.ones(0, 8, 8, 8))
