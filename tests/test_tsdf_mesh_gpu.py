"""TsdfVolume.mesh, TsdfVolume.from_blocks and fuse_frames_mesh (tsdf_mesh.hip) against the numpy restatement of their
semantics in tests/tsdf_mesh_ref.py.

Tolerance: none.  The device computes the same fp64 operations in the same order, there is no sqrt on this path and the
one division is the one surface_points already matches bit for bit: V, T, the vertices, the colours, the triangles and
the edges of return_edges are compared bit for bit.  The one geometric bound is the rendered sphere's: a vertex lies
within 0.152 voxel of the sphere (tests/test_tsdf_mesh_cpu.py), a chord between vertices on it sags by at most 3 h^2 / (8 r)
= 0.089 voxel, so a point of a triangle lies within 0.3 voxel."""
import numpy as np
import pytest
import torch

from tests.tsdf_mesh_ref import SPHERE, edge_census, mesh_ref, sphere_blocks, sphere_distance
from tests.tsdf_ref import TsdfRef, room_colors, room_frames

pytestmark = pytest.mark.gpu

VOXEL, ORIGIN = 0.05, (0.3, -1.2, 2.0)
ROOM_VOLUME = dict(voxel=0.1, trunc=0.4, origin=(-0.5, -0.5, -0.5))
_REF = {}


def _ref(key, build):
    """a restatement computed once and shared, never changed afterwards"""
    if key not in _REF:
        _REF[key] = build()
    return _REF[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _volume(dev, blocks, order=None, **kw):
    """TsdfVolume.from_blocks of numpy blocks, given in `order`"""
    from detection_3d_amd.tsdf import TsdfVolume
    order = np.arange(len(blocks[0])) if order is None else order
    put = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a[order])).to(dev)
    return TsdfVolume.from_blocks(*[put(a) for a in blocks], **kw)


def _same_mesh(vol, want, what, **mesh_kw):
    """vol.mesh(return_edges=True, **mesh_kw) against want = mesh_ref(...) -> (vertices, triangles) as numpy"""
    r_vertices, r_triangles, r_color, r_edges = want
    mesh, edges = vol.mesh(return_edges=True, **mesh_kw)
    assert mesh.vertices.dtype == torch.float32 and mesh.triangles.dtype == torch.int32 and edges.dtype == torch.int32
    vertices, triangles, edges = mesh.vertices.cpu().numpy(), mesh.triangles.cpu().numpy(), edges.cpu().numpy()
    print(f"{what}: {vol.n_blocks} blocks, {len(vertices)} vertices, {len(triangles)} triangles")
    assert vertices.shape == r_vertices.shape and triangles.shape == r_triangles.shape, what
    assert np.array_equal(edges, r_edges), what
    assert np.array_equal(_bits(vertices), _bits(r_vertices)), what
    assert np.array_equal(triangles, r_triangles), what
    if r_color is None:
        assert mesh.vertex_color is None, what
    else:
        assert mesh.vertex_color.dtype == torch.float32
        assert np.array_equal(_bits(mesh.vertex_color.cpu().numpy()), _bits(r_color)), what
    plain = vol.mesh(**mesh_kw)                            # without the edges: the same mesh
    assert torch.equal(plain.vertices.view(torch.int32), mesh.vertices.view(torch.int32))
    assert torch.equal(plain.triangles, mesh.triangles)
    return vertices, triangles


def _sphere():
    return _ref("sphere", lambda: (sphere_blocks(), mesh_ref(sphere_blocks(), VOXEL, ORIGIN)))


def test_sphere_from_shuffled_blocks(dev):
    blocks, want = _sphere()
    assert (blocks[4] == 0).sum() > 100                    # voxels without colour
    vol = _volume(dev, blocks, np.random.RandomState(1).permutation(8), voxel=VOXEL, origin=ORIGIN, max_blocks=64)
    assert vol.n_blocks == 8 and vol.color
    vertices, triangles = _same_mesh(vol, want, "sphere")
    assert edge_census(triangles) == (1, 0)
    assert sphere_distance(vertices[np.unique(triangles)], VOXEL, ORIGIN).max() <= 0.152


def test_sphere_with_a_missing_block_and_unseen_voxels(dev):
    """block (1, 1, 1) left out, five voxels near the surface with W = 0, W in {1, 2, 3} and min_weight 2: the mesh has a
    boundary, and still no directed edge occurs twice"""
    def build():
        rs = np.random.RandomState(2)
        coords, D, W, C, CW = [a[:7].copy() for a in sphere_blocks()]
        W = rs.randint(1, 4, W.shape).astype(np.float32)
        near = np.argwhere(np.abs(D) < 0.2)
        for j in rs.choice(len(near), 5, replace=False):
            W[tuple(near[j])] = 0
        blocks = (coords, D, W, C, CW)
        return blocks, mesh_ref(blocks, VOXEL, ORIGIN, min_weight=2)

    blocks, want = _ref("holed sphere", build)
    vol = _volume(dev, blocks, np.random.RandomState(3).permutation(7), voxel=VOXEL, origin=ORIGIN, max_blocks=7)
    _, triangles = _same_mesh(vol, want, "holed sphere", min_weight=2)
    most, unpaired = edge_census(triangles)
    assert most == 1 and unpaired > 0 and len(triangles) > 0    # a cell is emitted when all eight are seen: (2 / 3)^8 of them


def test_blocks_at_the_end_of_the_coordinate_range(dev):
    """two blocks at x = 65534 and 65535 with a plane through them: the neighbour beyond the range is absent"""
    def build():
        coords = np.array([(65534, 5, 7), (65535, 5, 7)], np.int32)
        l = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).astype(np.float64)
        D = np.stack([np.clip(((l[..., 2] - 3.4) + 0.21 * (l[..., 0] + 8 * j - 8) + 0.13 * l[..., 1]) / 4.0, -1, 1)
                      for j in range(2)]).astype(np.float32)
        blocks = (coords, D, np.ones_like(D), None, None)
        return blocks, mesh_ref(blocks, 0.02, (-10485.0, 0.5, 0.25))

    blocks, want = _ref("range end", build)
    vol = _volume(dev, blocks, np.array([1, 0]), voxel=0.02, origin=(-10485.0, 0.5, 0.25), max_blocks=4)
    assert not vol.color
    vertices, triangles = _same_mesh(vol, want, "range end")
    assert len(triangles) > 100 and edge_census(triangles)[0] == 1


def test_no_crossing_and_no_block_give_an_empty_mesh(dev):
    from detection_3d_amd.tsdf import TsdfVolume
    coords = np.array([(0, 0, 0), (0, 0, 1)], np.int32)
    ones = np.ones((2, 8, 8, 8), np.float32)
    vol = _volume(dev, (coords, ones, ones, None, None))
    mesh, edges = vol.mesh(return_edges=True)
    assert mesh.vertices.shape == (0, 3) and mesh.triangles.shape == (0, 3) and edges.shape == (0, 4)
    assert mesh.vertex_color is None
    empty = TsdfVolume(device=dev)                         # no block at all, and a device
    mesh = empty.mesh()
    assert mesh.vertices.shape == (0, 3) and mesh.triangles.shape == (0, 3) and mesh.vertex_color.shape == (0, 3)
    none = _volume(dev, tuple(a[:0] for a in (coords, ones, ones)) + (None, None))
    assert none.n_blocks == 0 and none.mesh().triangles.shape == (0, 3)


def _room():
    def build():
        depth, intr, extr = room_frames(48, 64, near_wall=True)
        return depth, intr, extr, room_colors(depth)
    return _ref("room", build)


def _room_ref(calls, with_color=True):
    def build():
        depth, intr, extr, col = _room()
        ref = TsdfRef(color=with_color, **ROOM_VOLUME)
        for a, b in calls:
            ref.integrate(depth[a:b], intr[a:b], extr[a:b], col[a:b])
        return ref
    return _ref(("room ref", calls, with_color), build)


def _room_mesh_ref(calls, min_weight=1, with_color=True, color=True):
    def build():
        coords, D, W, C, CW = _room_ref(calls, with_color).blocks()
        blocks = (coords, D, W, C, CW) if with_color else (coords, D, W, None, None)
        return mesh_ref(blocks, ROOM_VOLUME["voxel"], ROOM_VOLUME["origin"], min_weight, color)
    return _ref(("room mesh", calls, min_weight, with_color, color), build)


def _frames(dev, first=0, last=None):
    from detection_3d_amd.unproject import DepthFrames
    depth, intr, extr, col = _room()
    s = slice(first, last)
    return DepthFrames(torch.from_numpy(depth[s]).to(dev), intr[s], extr[s], color=torch.from_numpy(col[s]).to(dev))


def _room_volume(dev, calls, with_color=True):
    from detection_3d_amd.tsdf import TsdfVolume
    vol = TsdfVolume(max_blocks=1024, color=with_color, **ROOM_VOLUME)
    for a, b in calls:
        vol.integrate(_frames(dev, a, b))
    return vol


def test_room_through_integrate(dev):
    """five frames with uint8 colour in one call; then a second call; then min_weight 2"""
    vol = _room_volume(dev, ((0, 2),))
    _, t1 = _same_mesh(vol, _room_mesh_ref(((0, 2),)), "room, frames 0-1")
    vol.integrate(_frames(dev, 2, 5))
    _, t2 = _same_mesh(vol, _room_mesh_ref(((0, 2), (2, 5))), "room, then frames 2-4")
    _, t3 = _same_mesh(vol, _room_mesh_ref(((0, 2), (2, 5)), 2), "room, min_weight 2", min_weight=2)
    assert 0 < len(t1) < len(t2) and 0 < len(t3) < len(t2)
    one = _room_volume(dev, ((0, 5),))
    _same_mesh(one, _room_mesh_ref(((0, 5),)), "room, one call")


def test_without_colour(dev):
    vol = _room_volume(dev, ((0, 5),))
    _same_mesh(vol, _room_mesh_ref(((0, 5),), color=False), "color=False", color=False)
    plain = _room_volume(dev, ((0, 5),), with_color=False)
    _same_mesh(plain, _room_mesh_ref(((0, 5),), with_color=False), "a volume without colour")


def test_kinds_0_to_2_are_the_surface_rows(dev):
    vol = _room_volume(dev, ((0, 5),))
    for min_weight in (1, 2):
        mesh, edges = vol.mesh(min_weight, return_edges=True)
        rows, voxels = vol.surface_points(6, min_weight, return_voxels=True)
        axis = edges[:, 3] < 3
        assert 0 < int(axis.sum()) == rows.shape[0] < edges.shape[0]
        assert torch.equal(edges[axis][:, :3], voxels)
        assert torch.equal(mesh.vertices[axis].view(torch.int32), rows[:, :3].contiguous().view(torch.int32))
        assert torch.equal(mesh.vertex_color[axis].view(torch.int32), rows[:, 3:6].contiguous().view(torch.int32))


def test_from_blocks_is_the_inverse_of_blocks(dev):
    from detection_3d_amd.tsdf import TsdfVolume
    vol = _room_volume(dev, ((0, 2),))
    blocks = vol.blocks()
    back = TsdfVolume.from_blocks(*blocks, max_blocks=1024, **ROOM_VOLUME)
    assert back.n_blocks == vol.n_blocks and back.color
    for a, b in zip(back.blocks(), blocks):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for a, b in zip(back.surface_points(9, return_voxels=True), vol.surface_points(9, return_voxels=True)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # integrate finds the inserted blocks, adds its own and carries on: equal to the restatement that went on from there
    back.integrate(_frames(dev, 2, 5))
    ref = _room_ref(((0, 2), (2, 5)))
    assert back.n_blocks == len(ref.coords) > vol.n_blocks
    for a, b in zip(back.blocks(), ref.blocks()):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.astype(a.cpu().numpy().dtype))), "integrate after from_blocks"
    _same_mesh(back, _room_mesh_ref(((0, 2), (2, 5))), "from_blocks, then frames 2-4")
    # a coordinate twice is refused before anything is inserted
    twice = torch.cat([blocks[0], blocks[0][:1]])
    with pytest.raises(ValueError, match="twice"):
        TsdfVolume.from_blocks(twice, *[torch.cat([t, t[:1]]) for t in blocks[1:]], **ROOM_VOLUME)


def test_two_runs_give_the_same_bits(dev):
    outs = []
    for _ in range(2):
        vol = _room_volume(dev, ((0, 2), (2, 5)))
        mesh, edges = vol.mesh(return_edges=True)
        outs.append([t.cpu().numpy() for t in (mesh.vertices, mesh.triangles, mesh.vertex_color, edges)])
    for a, b in zip(*outs):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_fuse_frames_mesh_is_around_integrate_mesh(dev):
    from detection_3d_amd.tsdf import TsdfVolume, frames_slice, fuse_frames_mesh
    fr = _frames(dev)
    got = fuse_frames_mesh(fr, voxel=0.1, batch=2, min_weight=2, max_blocks=1024, step=2)
    vol = TsdfVolume.around(fr, 0.1, max_blocks=1024)
    for a in (0, 2, 4):
        vol.integrate(frames_slice(fr, a, min(a + 2, 5)), step=2)
    want = vol.mesh(2)
    assert got.triangles.shape[0] > 1000 and torch.equal(got.triangles, want.triangles)
    assert torch.equal(got.vertices.view(torch.int32), want.vertices.view(torch.int32))
    assert torch.equal(got.vertex_color.view(torch.int32), want.vertex_color.view(torch.int32))


def test_rendered_sphere_lies_on_the_sphere_and_scan_mesh_takes_the_mesh(dev):
    from detection_3d_amd.render import look_at, render_depth, scan_mesh
    blocks, _ = _sphere()
    mesh = _volume(dev, blocks, voxel=VOXEL, origin=ORIGIN, max_blocks=8).mesh()
    centre = np.array(ORIGIN) + np.array(SPHERE["c"]) * VOXEL
    H, W = 48, 64
    intr = np.array([[70.0, 70.0, 0.5 * (W - 1), 0.5 * (H - 1)]])
    extr = look_at(centre + np.array([-1.0, 0.25, 0.15]), centre)[None]
    fr = render_depth(mesh, intr, extr, H, W)
    z = fr.depth[0].cpu().numpy().astype(np.float64)
    v, u = np.nonzero(z > 0)
    assert len(v) > 300                                    # a disc of about 15 pixels' radius
    cam = np.stack([(u - intr[0, 2]) / intr[0, 0] * z[v, u], (v - intr[0, 3]) / intr[0, 1] * z[v, u], z[v, u]], 1)
    world = cam @ np.asarray(extr[0])[:, :3].T + np.asarray(extr[0])[:, 3]
    d = sphere_distance(world, VOXEL, ORIGIN)
    print(f"{len(v)} pixels hit the sphere, farthest from it {d.max():.4f} voxel (bound 0.3)")
    assert d.max() <= 0.3
    assert fr.color is not None and fr.color.dtype == torch.float32
    cloud = scan_mesh(mesh, intr, extr, H, W, voxel=0.01)
    assert cloud.shape[0] > 100 and cloud.shape[1] == 9
