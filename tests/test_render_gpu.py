"""detection_3d_amd.render (render.hip) against the numpy restatement of its semantics in tests/render_ref.py, and its
composition with unproject, fuse_frames, voxelize and points_in_boxes.

Bounds, derived: `tri` is an integer and must be exact.  Depth and colour are the same IEEE fp64 operations in the same
order on both sides (no contraction, correctly rounded division, rint to even) and one rounding to the output type: bit
for bit, at every pixel."""
import numpy as np
import pytest
import torch

from tests.render_ref import (BESIDE, HIDDEN, building, check_exact_scene, exact_scene, plane_expectation, plane_grid,
                              render_ref)
from tests.unproject_ref import PLANE, ROOM, angle_to, plane_angle_bound, room_face_distance, room_scene

pytestmark = pytest.mark.gpu

SHAPES = [(3, 37, 53), (2, 96, 131)]
_REF = {}


def _scene(shape, uint8_color=False, coincident=True):
    key = ("scene", shape, uint8_color, coincident)
    if key not in _REF:
        _REF[key] = exact_scene(*shape, uint8_color=uint8_color, coincident=coincident)
    return _REF[key]


def _ref(shape, uint8_color=False, coincident=True, uint16_depth=False):
    key = ("ref", shape, uint8_color, coincident, uint16_depth)
    if key not in _REF:
        sc = _scene(shape, uint8_color, coincident)
        _REF[key] = render_ref(sc["vertices"], sc["triangles"], sc["intr"], sc["extr"], shape[1], shape[2],
                               vertex_color=sc["color"], depth_dtype=np.uint16 if uint16_depth else np.float32)
        check_exact_scene(sc, _REF[key][1], shape[1], shape[2])
    return _REF[key]


def _mesh(dev, vertices, triangles, color=None):
    from detection_3d_amd.render import TriangleMesh
    return TriangleMesh(torch.from_numpy(vertices).to(dev), torch.from_numpy(triangles).to(dev),
                        None if color is None else torch.from_numpy(color).to(dev))


def _np(t):
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _render(dev, sc, shape, uint16_depth=False, **kw):
    from detection_3d_amd.render import render_depth
    frames, tri = render_depth(_mesh(dev, sc["vertices"], sc["triangles"], sc["color"]), sc["intr"], sc["extr"], shape[1],
                               shape[2], depth_dtype=torch.uint16 if uint16_depth else torch.float32,
                               return_triangles=True, **kw)
    assert tri.dtype == torch.int32 and tuple(tri.shape) == tuple(shape) == frames.shape
    assert tuple(frames.color.shape) == tuple(shape) + (3,)
    return _np(frames.depth), _np(tri), _np(frames.color)


@pytest.mark.parametrize("uint16_depth", [False, True])
@pytest.mark.parametrize("uint8_color", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_exact(dev, shape, uint8_color, uint16_depth):
    """test 1 of the issue: every pixel of every frame, the triangle, the depth bits and the colour bits"""
    sc = _scene(shape, uint8_color)
    r_depth, r_tri, r_color, _ = _ref(shape, uint8_color, uint16_depth=uint16_depth)
    depth, tri, color = _render(dev, sc, shape, uint16_depth)
    what = (shape, uint8_color, uint16_depth)
    assert depth.dtype == r_depth.dtype and color.dtype == r_color.dtype and tri.shape == r_tri.shape, what
    print(f"{what}: {int((r_tri >= 0).sum())} of {r_tri.size} pixels hit, {int((tri != r_tri).sum())} triangles, "
          f"{int((_bits(depth) != _bits(r_depth)).sum())} depths and {int((_bits(color) != _bits(r_color)).sum())} colour "
          f"components differ")
    assert np.array_equal(tri, r_tri), what
    assert np.array_equal(_bits(depth), _bits(r_depth)), what
    assert np.array_equal(_bits(color), _bits(r_color)), what
    if uint16_depth:
        assert (depth[r_tri >= 0] > 0).all()


def test_watertight_plane(dev):
    """test 2: 512 jittered triangles of mixed winding on z_w = 0, seen at ~70 degrees incidence at 64 x 80: no pixel
    centre is lost between them, and z is the analytic ray-plane depth to 1e-9 relative"""
    from detection_3d_amd.render import look_at, render_depth
    n, H, W = 16, 64, 80
    v, t = plane_grid(n)
    assert t.shape == (512, 3)
    eye, target = np.array([8.0, -1.5, 2.2]), np.array([8.0, 4.5, 0.0])
    incidence = np.degrees(np.arctan2(np.linalg.norm((target - eye)[:2]), eye[2]))
    assert 65.0 < incidence < 75.0
    intr, extr = np.array([70.0, 70.0, 0.5 * (W - 1), 0.5 * (H - 1)]), look_at(eye, target)
    inside, want = plane_expectation(intr, extr, H, W, n)
    assert inside.mean() > 0.5
    # fp32 depth rounds z; the fp64 z itself is compared through the restatement, which the device equals bit for bit
    r_depth, r_tri, _, r_z = render_ref(v, t, intr, extr[None], H, W)
    frames, tri = render_depth(_mesh(dev, v, t), intr, extr[None], H, W, return_triangles=True)
    tri, depth = _np(tri)[0], _np(frames.depth)[0]
    assert np.array_equal(tri, r_tri[0]) and np.array_equal(_bits(depth), _bits(r_depth[0]))
    err = np.abs(r_z[0][inside] - want[inside]) / want[inside]
    print(f"plane: {int(inside.sum())} pixels inside the outline, {int((tri[inside] < 0).sum())} without a hit, largest "
          f"relative depth error {err.max():.3e} (bound 1e-9), {np.unique(tri[inside]).size} triangles seen")
    assert (tri[inside] >= 0).all()
    assert (err <= 1e-9).all()
    assert (np.abs(depth[inside].astype(np.float64) - want[inside]) <= (1e-9 + 2.0 ** -24) * want[inside]).all()


def test_order_independence(dev):
    """test 3: a permuted triangle array gives the same depth and colour bits and the permuted indices (the scene
    without the coincident pair: no exact ties between different triangles but on shared edges, which this scene's
    cameras may meet; there the depth is equal and the index may differ), and two runs give the same bits"""
    shape = SHAPES[0]
    sc = _scene(shape, coincident=False)
    depth, tri, color = _render(dev, sc, shape)
    again = _render(dev, sc, shape)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip((depth, tri, color), again))
    perm = np.random.RandomState(4).permutation(sc["triangles"].shape[0])      # new index i is old triangle perm[i]
    moved = dict(sc, triangles=np.ascontiguousarray(sc["triangles"][perm]))
    p_depth, p_tri, p_color = _render(dev, moved, shape)
    assert np.array_equal(_bits(p_depth), _bits(depth))
    back = np.where(p_tri >= 0, perm[np.maximum(p_tri, 0)], -1)
    same = back == tri
    # where the index differs, two triangles tie exactly: the restatement with the other triangle alone gives that depth
    print(f"order: {int((~same).sum())} pixels at exact ties of {same.size}")
    assert (~same).sum() <= 0.01 * same.size and ((tri >= 0) == (p_tri >= 0)).all()
    assert np.array_equal(_bits(p_color[same]), _bits(color[same]))
    for f, v, u in zip(*np.nonzero(~same)):
        one = sc["triangles"][[back[f, v, u]]]
        z = render_ref(sc["vertices"], one, sc["intr"][f], sc["extr"][f][None], shape[1], shape[2])[0][0, v, u]
        assert z == depth[f, v, u]


def test_chunking(dev):
    """test 4: one frame per chunk gives the bits of one chunk; a budget below a frame's need names the need"""
    from detection_3d_amd.render import frame_scratch_bytes, last_chunks
    shape = SHAPES[1]
    sc = dict(_scene(shape))
    sc["extr"] = np.concatenate([sc["extr"], sc["extr"][::-1]])               # four frames that all see the room
    sc["intr"] = np.concatenate([sc["intr"], sc["intr"][::-1]])
    shape = (4,) + shape[1:]
    whole = _render(dev, sc, shape)
    assert last_chunks() == [(0, 4)]
    need = frame_scratch_bytes(_mesh(dev, sc["vertices"], sc["triangles"]), sc["intr"], sc["extr"], shape[1], shape[2])
    assert len(need) == 4 and need[0] == need[3] and need[1] == need[2] and min(need) > 4 * 100
    split = _render(dev, sc, shape, max_scratch_bytes=max(need))
    assert last_chunks() == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(whole, split))
    with pytest.raises(ValueError, match=str(max(need))):
        _render(dev, sc, shape, max_scratch_bytes=max(need) - 1)
    with pytest.raises(ValueError, match="needs"):
        _render(dev, sc, shape, max_scratch_bytes=64)


def test_round_trip_through_unproject(dev):
    """test 5: the room of tests/unproject_ref.py as a box mesh, 48 x 64 from its 4 cameras.  Every point is within
    1e-5 m of a face (one fp32 rounding of z <= 12 m, 7e-7 m, and one of the position).  A pixel whose four neighbours
    show its own face has the face's normal within the bound of tests/unproject_ref.py's plane test: plane_angle_bound
    is evaluated on the exact points of the face's plane over the rectangle of pixels around those that show it, and its
    rounding term (all but the final 2^-24), which is linear in the plane's distance |d| from the camera, is scaled from
    PLANE's |d| to the face's."""
    from detection_3d_amd.render import box_mesh, render_depth
    from detection_3d_amd.unproject import suncg_cameras, unproject
    H, W = 48, 64
    ref_depth, cams = room_scene(H, W)
    intr, extr = suncg_cameras(cams, H, W)
    v, t = box_mesh([[2.0, 1.5, 0.0, 4.0, 3.0, 2.5, 0.0]])
    frames, tri = render_depth(_mesh(dev, v, t), intr, extr, H, W, return_triangles=True)
    depth, tri = _np(frames.depth), _np(tri)
    assert (tri >= 0).all() and np.abs(depth - ref_depth).max() < 1e-5
    rows = unproject(frames, edge=1.0).cpu().numpy()       # every neighbour on the pixel's own face is usable
    assert rows.shape == (4 * H * W, 9)
    dist = room_face_distance(rows[:, :3])
    print(f"round trip: farthest point from a face {dist.max():.3e} m (bound 1e-5)")
    assert dist.max() <= 1e-5
    normals = rows[:, 6:9].reshape(4, H, W, 3)
    face = tri // 2                                       # box_mesh: two triangles per face, x-, x+, y-, y+, z-, z+
    face_normal = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])   # inwards
    face_offset = np.array([0.0, ROOM[0], 0.0, ROOM[1], 0.0, ROOM[2]])
    vv, uu = np.mgrid[0:H, 0:W].astype(np.float64)
    checked, worst = 0, 0.0
    for f in range(4):
        fx, fy, cx, cy = intr[f]
        R, eye = extr[f][:, :3], extr[f][:, 3]
        rays = np.stack([(uu - cx) / fx, (vv - cy) / fy, np.ones_like(uu)], -1)
        own = np.zeros((H, W), bool)
        own[1:-1, 1:-1] = ((face[f, 1:-1, 1:-1] == face[f, 1:-1, :-2]) & (face[f, 1:-1, 1:-1] == face[f, 1:-1, 2:])
                           & (face[f, 1:-1, 1:-1] == face[f, :-2, 1:-1]) & (face[f, 1:-1, 1:-1] == face[f, 2:, 1:-1]))
        for k in range(6):
            sel = own & (face[f] == k)
            if not sel.any():
                continue
            n_cam = R.T @ face_normal[k]
            d = abs(eye[k // 2] - face_offset[k])          # the plane's distance from the camera
            r0, r1 = np.nonzero(sel.any(1))[0][[0, -1]]
            c0, c1 = np.nonzero(sel.any(0))[0][[0, -1]]
            patch = rays[r0 - 1:r1 + 2, c0 - 1:c1 + 2]
            points = patch * (-d / (patch @ n_cam))[..., None]
            assert (points[..., 2] > 0).all()
            bound = (plane_angle_bound(points) - 2.0 ** -24) * d / abs(PLANE["d"]) + 2.0 ** -24
            ang = angle_to(normals[f][sel], face_normal[k])
            assert (normals[f][sel] != 0).any(-1).all()
            checked += int(sel.sum())
            worst = max(worst, float((ang / bound).max()))
            assert ang.max() <= bound, (f, k, ang.max(), bound)
    print(f"round trip: {checked} of {4 * H * W} normals checked, largest angle / bound {worst:.3f}")
    assert checked > 0.8 * 4 * H * W


def test_scan_mesh(dev):
    """test 6: walls, floor, ceiling and a cupboard from six cameras at 64 x 64 -> the detector's cloud.  The extent
    allows 1e-4 m: the fp32 roundings of a depth and a position below 50 m are under 1e-5 m, and a voxel mean lies in
    the hull of its points."""
    from detection_3d_amd.primitives import points_in_boxes
    from detection_3d_amd.render import scan_mesh
    from detection_3d_amd.voxelize import voxelize
    v, t, lo, hi, intr, extr = building()
    color = np.random.RandomState(2).randint(0, 256, v.shape).astype(np.uint8)
    cloud = scan_mesh(_mesh(dev, v, t, color), intr, extr, 64, 64, voxel=0.05, max_points=500_000, seed=1)
    assert cloud.dtype == torch.float32 and cloud.dim() == 2 and cloud.shape[1] == 9 and cloud.shape[0] > 1000
    assert bool(torch.isfinite(cloud).all())
    c = cloud.cpu().numpy().astype(np.float64)
    assert (c[:, :3] >= lo - 1e-4).all() and (c[:, :3] <= hi + 1e-4).all()
    length = np.sqrt((c[:, 6:9] ** 2).sum(1))
    assert ((length == 0) | (np.abs(length - 1.0) < 2.0 ** -22)).all() and (length > 0).mean() > 0.5
    out = voxelize(cloud)
    assert out[0].shape[0] == cloud.shape[0] and out[1].shape == cloud.shape
    slabs = torch.from_numpy(np.stack([HIDDEN, BESIDE]).astype(np.float32)).to(dev)
    count = points_in_boxes(cloud, slabs)[1].cpu().numpy()
    print(f"scan_mesh: {cloud.shape[0]} points; behind the cupboard {count[0]}, beside it {count[1]}")
    assert count[0] == 0 and count[1] > 0
    capped = scan_mesh(_mesh(dev, v, t, color), intr, extr, 64, 64, voxel=0.05, max_points=500, seed=1, max_depth=6.0)
    assert capped.shape == (500, 9)


def test_degenerate_inputs(dev):
    """test 7: no frame, no triangle, no vertex: zero images of the right shapes; CPU tensors and bad cameras raise"""
    from detection_3d_amd._lib import D3DError
    from detection_3d_amd.render import TriangleMesh, last_chunks, render_depth
    sc = _scene(SHAPES[0], uint8_color=True)
    full = _mesh(dev, sc["vertices"], sc["triangles"], sc["color"])
    frames, tri = render_depth(full, sc["intr"][:0], sc["extr"][:0], 9, 11, return_triangles=True)
    assert frames.shape == (0, 9, 11) and tri.shape == (0, 9, 11) and frames.color.shape == (0, 9, 11, 3)
    no_tri = _mesh(dev, sc["vertices"], sc["triangles"][:0], sc["color"])
    no_vertex = _mesh(dev, sc["vertices"][:0], sc["triangles"], sc["color"][:0])
    for mesh in (no_tri, no_vertex):
        for dtype in (torch.float32, torch.uint16):
            frames, tri = render_depth(mesh, sc["intr"], sc["extr"], 9, 11, depth_dtype=dtype, return_triangles=True)
            assert last_chunks() == []
            assert frames.shape == (3, 9, 11) and frames.depth.dtype == dtype and not _np(frames.depth).any()
            assert frames.color.dtype == torch.uint8 and not bool(frames.color.any()) and bool((tri == -1).all())
    assert render_depth(no_tri, sc["intr"], sc["extr"], 9, 11).color is not None
    # a mesh of which no triangle can be hit runs the kernels and gives the same
    dead = dict(sc, triangles=np.array([[0, 1, sc["vertices"].shape[0]], [-5, 0, 1]], np.int32))
    depth, tri, color = _render(dev, dead, SHAPES[0])
    assert not depth.any() and (tri == -1).all() and not color.any()
    # uint16 depth at 10 um: every z above 0.65535 m is "no measurement", the triangle stays
    r_depth, r_tri = render_ref(sc["vertices"], sc["triangles"], sc["intr"], sc["extr"], SHAPES[0][1], SHAPES[0][2],
                                depth_dtype=np.uint16, depth_scale=1e-5)[:2]
    depth, tri, _ = _render(dev, sc, SHAPES[0], uint16_depth=True, depth_scale=1e-5)
    assert ((r_depth == 0) & (r_tri >= 0)).any() and (r_depth > 0).any()
    assert np.array_equal(depth, r_depth) and np.array_equal(tri, r_tri)
    with pytest.raises(D3DError):
        TriangleMesh(torch.from_numpy(sc["vertices"]), torch.from_numpy(sc["triangles"]).to(dev))
    with pytest.raises(ValueError):
        render_depth(full, sc["intr"][:2], sc["extr"], 9, 11)
    with pytest.raises(ValueError):
        render_depth(full, sc["intr"], sc["extr"][:, :2], 9, 11)
    with pytest.raises(ValueError):
        render_depth(full, sc["intr"], sc["extr"], 1 << 16, 1 << 14)
