"""detection_3d_amd.tsdf (tsdf.hip) against the numpy restatement of its semantics in tests/tsdf_ref.py.

Tolerance: the device computes the same fp64 operations in the same order, so the block coordinates, weight,
color_weight, tsdf, color, the number of rows, the positions, the colours, the voxels of return_voxels and the set of
rows without a normal agree bit for bit.  The normal is m / sqrt(l2) per component: where the device's fp64 sqrt or
division differs from numpy's in the last place, the single fp32 rounding of a value of magnitude <= 1 moves by at most
one ulp <= 2^-24, so every component agrees within 2^-23 (the bound of tests/test_unproject_gpu.py); each case prints
how many components differ at all.  The restatement has no cull, so a cull that changed a result would show."""
import numpy as np
import pytest
import torch

from tests.tsdf_ref import TsdfRef, holes_scene, room_colors, room_frames

pytestmark = pytest.mark.gpu

ROOM_VOLUME = dict(voxel=0.1, trunc=0.4, origin=(-0.5, -0.5, -0.5))
_REF = {}


def _room(H, W, color):
    """the room's five frames (the fifth 0.3 m from a wall); color: 'u8', 'f32' or None"""
    key = ("room", H, W, color)
    if key not in _REF:
        depth, intr, extr = room_frames(H, W, near_wall=True)
        col = None if color is None else room_colors(depth)
        if color == "f32":
            col = (col.astype(np.float32) / np.float32(255.0)).copy()
        _REF[key] = (depth, intr, extr, col)
    return _REF[key]


def _ref(key, build):
    """a restatement computed once and shared, never changed afterwards"""
    if key not in _REF:
        _REF[key] = build()
    return _REF[key]


def _frames(dev, depth, intr, extr, color=None, first=0, last=None):
    from detection_3d_amd.unproject import DepthFrames
    s = slice(first, last)
    return DepthFrames(torch.from_numpy(depth[s]).to(dev), intr[s], extr[s],
                       color=None if color is None else torch.from_numpy(color[s]).to(dev))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_blocks(vol, ref, what):
    coords, tsdf, weight, color, cweight = vol.blocks()
    r_coords, r_tsdf, r_weight, r_color, r_cweight = ref.blocks()
    assert coords.dtype == torch.int32 and tsdf.dtype == torch.float32
    assert vol.n_blocks == len(r_coords), what
    assert np.array_equal(coords.cpu().numpy(), r_coords), what
    assert np.array_equal(_bits(weight.cpu().numpy()), _bits(r_weight)), what
    assert np.array_equal(_bits(tsdf.cpu().numpy()), _bits(r_tsdf)), what
    if vol.color:
        assert np.array_equal(_bits(cweight.cpu().numpy()), _bits(r_cweight)), what
        assert np.array_equal(_bits(color.cpu().numpy()), _bits(r_color)), what
    else:
        assert color is None and cweight is None
    assert vol.clipped == ref.clipped, what


def _same_surface(vol, ref, what, columns=(3, 6, 9), min_weight=1):
    n = None
    for c in columns:
        rows, voxels = vol.surface_points(c, min_weight, return_voxels=True)
        assert rows.dtype == torch.float32 and voxels.dtype == torch.int32
        rows, voxels = rows.cpu().numpy(), voxels.cpu().numpy()
        r_rows, r_voxels, r_has = ref.surface_points(c, min_weight)
        assert rows.shape == r_rows.shape, (what, c)
        assert np.array_equal(voxels, r_voxels), (what, c)
        k = min(c, 6)
        assert np.array_equal(_bits(rows[:, :k]), _bits(r_rows[:, :k])), (what, c)
        if c == 9:
            zero = (rows[:, 6:9] == 0).all(1)
            assert np.array_equal(zero, ~r_has), what
            err = np.abs(rows[:, 6:9].astype(np.float64) - r_rows[:, 6:9].astype(np.float64))
            print(f"{what}: {vol.n_blocks} blocks, {rows.shape[0]} rows, {int(zero.sum())} without a normal; "
                  f"{int((err > 0).sum())} of {err.size} normal components differ, largest "
                  f"{err.max() if err.size else 0.0:.3e} (bound {2.0 ** -23:.3e})")
            assert (err <= 2.0 ** -23).all(), what
        n = rows.shape[0]
    return n


def _room_case(dev, H, W, color, volume=ROOM_VOLUME, calls=((0, None),), with_color=True, **int_kw):
    """integrates the room's frames in `calls` (first, last) on the device and in the restatement -> (volume, ref)"""
    from detection_3d_amd.tsdf import TsdfVolume
    depth, intr, extr, col = _room(H, W, color)

    def build():
        ref = TsdfRef(color=with_color, **volume)
        for a, b in calls:
            ref.integrate(depth[a:b], intr[a:b], extr[a:b], None if col is None else col[a:b], **int_kw)
        return ref

    ref = _ref(("room ref", H, W, color, tuple(sorted(volume.items())), calls, with_color, tuple(sorted(int_kw.items()))),
               build)
    vol = TsdfVolume(max_blocks=1024, color=with_color, **volume)
    for a, b in calls:
        assert vol.integrate(_frames(dev, depth, intr, extr, col, a, b), **int_kw) is vol
    return vol, ref


@pytest.mark.parametrize("color", ["u8", "f32", None])
@pytest.mark.parametrize("size", [(48, 64), (96, 128)])
def test_room(dev, size, color):
    """five cameras, one of them inside the culling sphere of the blocks around it; blocks, every column count, and
    min_weight 2"""
    what = ("room", size, color)
    vol, ref = _room_case(dev, *size, color, with_color=color is not None)
    _same_blocks(vol, ref, what)
    n1 = _same_surface(vol, ref, what)
    n2 = _same_surface(vol, ref, what + ("min_weight 2",), columns=(9,), min_weight=2)
    assert 0 < n2 < n1


def test_room_frames_without_colour_leave_a_colour_volume_untouched(dev):
    vol, ref = _room_case(dev, 48, 64, None, with_color=True)
    _same_blocks(vol, ref, "no colour image")
    assert float(vol.blocks()[4].abs().max()) == 0.0
    _same_surface(vol, ref, "no colour image", columns=(6,))


@pytest.mark.parametrize("step", [1, 2])
def test_step_and_depth_range(dev, step):
    """step thins the allocation only; min_depth and max_depth cut both passes"""
    what = ("step", step)
    vol, ref = _room_case(dev, 48, 64, "u8", step=step, min_depth=0.5, max_depth=3.0)
    _same_blocks(vol, ref, what)
    _same_surface(vol, ref, what, columns=(9,))


def test_single_frame(dev):
    vol, ref = _room_case(dev, 48, 64, "u8", calls=((4, 5),))
    _same_blocks(vol, ref, "F = 1")
    _same_surface(vol, ref, "F = 1", columns=(9,))


def test_two_calls_add_blocks_and_update_old_ones(dev):
    what = "frames 0-1, then 2-4"
    vol, ref = _room_case(dev, 48, 64, "u8", calls=((0, 2), (2, 5)))
    one, _ = _room_case(dev, 48, 64, "u8", calls=((0, 2),))
    assert one.n_blocks < vol.n_blocks                   # the second call allocated blocks of its own
    _same_blocks(vol, ref, what)
    _same_surface(vol, ref, what, columns=(9,))


@pytest.mark.parametrize("float_depth", [False, True])
def test_holes_scene_through_around(dev, float_depth):
    """uint16 depth with ~30 % holes and one empty frame, or fp32 depth with NaN, inf, negatives and values outside the
    depth range; uint8 colour; random poses tens of metres out, the origin from TsdfVolume.around"""
    from detection_3d_amd.tsdf import TsdfVolume
    what = ("holes", float_depth)
    depth, color, intr, extr = holes_scene(3, 37, 53, float_depth=float_depth)
    kw = dict(min_depth=0.5, max_depth=6.0) if float_depth else {}
    fr = _frames(dev, depth, intr, extr, color)
    vol = TsdfVolume.around(fr, 0.05, max_blocks=1 << 14, **kw)
    assert vol.trunc == 4.0 * 0.05
    ref = TsdfRef(0.05, None, vol.origin).integrate(depth, intr, extr, color, **kw)
    vol.integrate(fr, **kw)
    assert not vol.clipped and vol.n_blocks > 0
    _same_blocks(vol, ref, what)
    assert _same_surface(vol, ref, what) > 0


def test_clipped(dev):
    """part of the room lies below coordinate 0 of the volume: those samples are dropped, the rest is the same"""
    volume = dict(ROOM_VOLUME, origin=(1.3, -0.5, 0.9))
    vol, ref = _room_case(dev, 48, 64, "u8", volume=volume)
    assert vol.clipped and ref.clipped
    _same_blocks(vol, ref, "clipped")
    assert _same_surface(vol, ref, "clipped", columns=(9,)) > 0
    roomy, ref = _room_case(dev, 48, 64, "u8", volume=dict(ROOM_VOLUME, origin=(-0.9, -0.9, -0.9)))
    assert not roomy.clipped and not ref.clipped and vol.n_blocks < roomy.n_blocks


def test_full_volume_raises_until_reset(dev):
    """16 blocks do not hold the room: a bounds check by construction (no block past max_blocks has storage and the table
    walk is bounded), reported after the call's one read-back"""
    from detection_3d_amd._lib import D3DError
    from detection_3d_amd.tsdf import TsdfVolume
    depth, intr, extr, col = _room(48, 64, "u8")
    fr = _frames(dev, depth, intr, extr, col)
    vol = TsdfVolume(max_blocks=16, **ROOM_VOLUME)
    with pytest.raises(D3DError, match="16 blocks"):
        vol.integrate(fr)
    for call in (lambda: vol.integrate(fr), vol.surface_points, vol.blocks):
        with pytest.raises(D3DError, match="reset"):
            call()
    assert vol.reset() is vol and vol.n_blocks == 0 and not vol.clipped
    assert vol.surface_points(9).shape == (0, 9)
    # what the near-wall camera sees within 0.6 m fits
    ref = TsdfRef(**ROOM_VOLUME).integrate(depth[4:], intr[4:], extr[4:], col[4:], max_depth=0.6)
    assert 0 < len(ref.coords) <= 16
    vol.integrate(_frames(dev, depth, intr, extr, col, 4), max_depth=0.6)
    _same_blocks(vol, ref, "after reset")
    _same_surface(vol, ref, "after reset", columns=(9,))
    # and a volume with enough blocks holds all of it
    vol, ref = _room_case(dev, 48, 64, "u8")
    _same_blocks(vol, ref, "enough blocks")


def test_two_runs_give_the_same_bits(dev):
    outs = []
    for _ in range(2):
        vol, _ = _room_case(dev, 96, 128, "u8", calls=((0, 2), (2, 5)))
        rows, voxels = vol.surface_points(9, return_voxels=True)
        outs.append([t.cpu().numpy() for t in vol.blocks()] + [rows.cpu().numpy(), voxels.cpu().numpy()])
    for a, b in zip(*outs):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_fuse_frames_tsdf_is_around_integrate_surface_cap(dev):
    from detection_3d_amd.downsample import cap_points
    from detection_3d_amd.tsdf import TsdfVolume, frames_slice, fuse_frames_tsdf
    depth, intr, extr, col = _room(48, 64, "u8")
    fr = _frames(dev, depth, intr, extr, col)
    out = fuse_frames_tsdf(fr, voxel=0.1, max_points=3000, seed=5, batch=2, max_blocks=1024, step=2)
    vol = TsdfVolume.around(fr, 0.1, max_blocks=1024)
    for a in (0, 2, 4):
        vol.integrate(frames_slice(fr, a, min(a + 2, 5)), step=2)
    cloud = vol.surface_points(9)
    assert cloud.shape[0] > 3000
    want = cap_points(cloud, 3000, 5)
    assert out.shape == (3000, 9) and torch.equal(out.view(torch.int32), want.view(torch.int32))
    uncut = fuse_frames_tsdf(fr, voxel=0.1, max_points=None, batch=2, min_weight=2, max_blocks=1024, step=2)
    seen_twice = vol.surface_points(9, 2)
    assert 0 < seen_twice.shape[0] < cloud.shape[0]
    assert torch.equal(uncut.view(torch.int32), seen_twice.view(torch.int32))
