"""The host side of detection_3d_amd.render and the numpy restatement of its kernel's semantics (tests/render_ref.py) on
known answers.  No GPU."""
import numpy as np
import pytest
import torch

from tests.render_ref import (camera_space, check_exact_scene, exact_scene, moller_trumbore, plane_expectation, plane_grid,
                              render_ref,
                              room_cameras)


def test_wall_facing_the_camera_has_its_distance_at_every_covered_pixel():
    """an axis-aligned wall at distance d in front of the identity camera: z == d exactly (D = d S in exact products of
    small binary fractions), and the covered pixels are those whose ray meets the rectangle"""
    from detection_3d_amd.render import box_mesh
    H, W, f, d = 21, 30, 16.0, 2.5
    v = np.array([[-1.0, -0.5, d], [1.0, -0.5, d], [1.0, 0.75, d], [-1.0, 0.75, d]], np.float32)
    t = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    intr = np.array([f, f, 14.0, 10.0])
    extr = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None]
    depth, tri, color, z = render_ref(v, t, intr, extr, H, W)
    vv, uu = np.mgrid[0:H, 0:W]
    x, y = (uu - 14.0) / f * d, (vv - 10.0) / f * d
    covered = (np.abs(x) <= 1.0) & (y >= -0.5) & (y <= 0.75)
    assert covered.sum() > 50 and np.array_equal(tri[0] >= 0, covered)
    assert (z[0][covered] == d).all() and (depth[0][covered] == np.float32(d)).all() and (depth[0][~covered] == 0).all()
    # the shared diagonal goes to the lower index, and uint16 depth is millimetres
    assert (tri[0][covered & (np.abs(y + 0.5 - (x + 1.0) * 0.625) < 1e-12)] == 0).all()
    d16 = render_ref(v, t, intr, extr, H, W, depth_dtype=np.uint16)[0]
    assert d16.dtype == np.uint16 and (d16[0][covered] == 2500).all() and (d16[0][~covered] == 0).all()
    assert (render_ref(v, t, intr, extr, H, W, max_depth=2.0)[1] == -1).all()
    assert box_mesh(np.zeros((0, 7)))[0].shape == (0, 3)


def test_restatement_agrees_with_moller_trumbore_away_from_edges():
    """the exactness scene: every hit whose barycentric coordinates are at least 1e-6 from an edge has the depth and the
    weights of an independent intersection routine to 1e-12 relative; the special triangles do what they are there for"""
    F, H, W = 3, 37, 53
    sc = exact_scene(F, H, W)
    depth, tri, color, z = render_ref(sc["vertices"], sc["triangles"], sc["intr"], sc["extr"], H, W, vertex_color=sc["color"])
    check_exact_scene(sc, tri, H, W)
    assert 50 <= sc["triangles"].shape[0] <= 80
    checked, worst = 0, 0.0
    for f in range(F):
        P = camera_space(sc["vertices"], sc["extr"][f])
        fx, fy, cx, cy = sc["intr"][f]
        for v in range(H):
            for u in range(W):
                t = tri[f, v, u]
                if t < 0:
                    continue
                a, b, c = P[sc["triangles"][t]]
                d = np.array([(u - cx) / fx, (v - cy) / fy, 1.0])
                tt, bu, bv = moller_trumbore(np.zeros(3), d, a, b, c)
                if not min(bu, bv, 1.0 - bu - bv) > 1e-6:
                    continue
                checked += 1
                worst = max(worst, abs(tt - z[f, v, u]) / tt)
                want = (1.0 - bu - bv) * sc["color"][sc["triangles"][t][0]] + bu * sc["color"][sc["triangles"][t][1]] \
                    + bv * sc["color"][sc["triangles"][t][2]]
                assert np.abs(want - color[f, v, u]).max() < 1e-6
    print(f"{checked} pixels against Moller-Trumbore, largest relative depth difference {worst:.3e}")
    assert checked > 0.5 * 2 * H * W and worst <= 1e-12


def test_watertight_plane_in_the_restatement():
    from detection_3d_amd.render import look_at
    v, t = plane_grid(4)
    assert t.shape == (32, 3) and (v[:, 2] == 0).all()
    intr, extr = [30.0, 30.0, 15.5, 11.5], look_at([2.0, -3.0, 2.0], [2.0, 2.0, 0.0])
    tri, _, z = render_ref(v, t, intr, extr[None], 24, 32)[1:]
    inside, want = plane_expectation(intr, extr, 24, 32, 4)
    assert inside.sum() > 30 and (tri[0][inside] >= 0).all()
    assert (np.abs(z[0][inside] - want[inside]) <= 1e-9 * want[inside]).all()


def test_box_mesh_corners_and_closed_faces():
    from detection_3d_amd.render import box_mesh
    boxes = np.array([[1.0, 2.0, 0.5, 0.2, 3.0, 2.5, 0.0], [-3.0, 4.0, 1.0, 0.5, 2.0, 1.5, 0.6]])
    v, t = box_mesh(boxes)
    assert v.dtype == np.float32 and t.dtype == np.int32 and v.shape == (16, 3) and t.shape == (24, 3)
    # yaw 0: the thickness d3 runs along x, the length d4 along y (primitives' lx, ly)
    assert np.allclose(v[:8].min(0), [0.9, 0.5, 0.5]) and np.allclose(v[:8].max(0), [1.1, 3.5, 3.0])
    # a rotated box: every corner maps back to (+-d3/2, +-d4/2, 0 or dz) in the box frame of primitives.points_in_boxes
    b = boxes[1]
    c, s = np.cos(b[6]), np.sin(b[6])
    dx, dy = v[8:, 0].astype(np.float64) - b[0], v[8:, 1].astype(np.float64) - b[1]
    lx, ly, lz = c * dx - s * dy, s * dx + c * dy, v[8:, 2] - b[2]
    got = sorted(zip(np.round(lx, 5), np.round(ly, 5), np.round(lz, 5)))
    want = sorted((i * 0.25, j * 1.0, l * 1.5) for i in (-1, 1) for j in (-1, 1) for l in (0, 1))
    assert np.allclose(got, want, atol=1e-5)
    for k in range(2):
        tk = t[12 * k:12 * k + 12]
        assert tk.min() == 8 * k and tk.max() == 8 * k + 7
        edges = {}
        for a, b_, c_ in tk:
            for e in ((a, b_), (b_, c_), (c_, a)):
                edges.setdefault(frozenset(e), []).append(e)
        assert len(edges) == 18
        # closed and consistently wound: every edge is used by exactly two triangles, once in each direction
        assert all(len(u) == 2 and u[0] == u[1][::-1] for u in edges.values())
        # wound outwards: the signed volume is that of the box
        p = v[tk].astype(np.float64) - v[8 * k:8 * k + 8].astype(np.float64).mean(0)
        vol = np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0
        assert abs(vol - boxes[k, 3] * boxes[k, 4] * boxes[k, 5]) < 1e-5


def test_look_at_has_the_rotation_of_suncg_cameras():
    from detection_3d_amd.render import look_at
    from detection_3d_amd.unproject import suncg_cameras
    eye, target = np.array([1.0, -2.0, 1.5]), np.array([4.0, 3.0, 0.5])
    extr = look_at(eye, target, up=(0.1, 0.2, 1.0))
    R = extr[:, :3]
    t, u = R[:, 2], -R[:, 1]
    assert np.allclose(t, (target - eye) / np.linalg.norm(target - eye)) and u @ np.array([0.1, 0.2, 1.0]) > 0
    cam = np.concatenate([eye, t, u, [0.62, np.arctan(np.tan(0.62) * 48 / 64), 1.0]])
    want = suncg_cameras(cam[None], 48, 64)[1][0]
    assert np.abs(want - extr).max() < 1e-15
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and np.linalg.det(R) > 0
    assert np.array_equal(extr[:, 3], eye)
    assert np.array_equal(room_cameras(1)[0][:, :3], np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]))
    with pytest.raises(ValueError):
        look_at(eye, eye)
    with pytest.raises(ValueError):
        look_at(eye, eye + [0.0, 0.0, 2.0])


def test_argument_errors():
    from detection_3d_amd._lib import D3DError
    from detection_3d_amd.render import TriangleMesh, render_depth, scan_mesh
    v, t = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(D3DError):
        TriangleMesh(v, t)
    for bad in ((v[:, :2], t), (v, t[:, :2]), (v.double(), t), (v, t.long()), (v.numpy(), t)):
        with pytest.raises(ValueError):
            TriangleMesh(*bad)
    with pytest.raises(ValueError):
        TriangleMesh(v, t, vertex_color=torch.zeros(3, 3))
    with pytest.raises(ValueError):
        TriangleMesh(v, t, vertex_color=torch.zeros(4, 3, dtype=torch.float64))
    extr = np.zeros((1, 3, 4))
    with pytest.raises(ValueError):
        render_depth("mesh", [1.0, 1.0, 0.0, 0.0], extr, 4, 4)
    for kw in (dict(height=0), dict(width=2.5), dict(min_depth=float("nan")), dict(depth_dtype=torch.float64),
               dict(depth_scale=0.0), dict(max_scratch_bytes=0)):
        args = dict(height=4, width=4)
        args.update(kw)
        with pytest.raises(ValueError, match="render_depth"):
            render_depth("mesh", [1.0, 1.0, 0.0, 0.0], extr, **args)
    with pytest.raises(ValueError):
        scan_mesh(None, [1.0, 1.0, 0.0, 0.0], extr, 4, 4)
