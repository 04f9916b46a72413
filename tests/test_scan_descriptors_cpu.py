"""The descriptors of the raw-scan chain (d3d_depth_frames, d3d_tsdf_volume, d3d_triangle_mesh of include/d3d_hip.h) at
the thirteen entry points that take them: a NULL descriptor, a descriptor with exactly one bad field, and a valid
descriptor of an empty batch, volume or mesh.  No GPU: an argument fault returns before any HIP call, and so does a call
that has nothing to do.  Every pointer here is a made-up address that nothing reads.

The expected texts are those of the entry points as they were with loose arguments (ABI 2), so a case fails when a check
was lost or reworded, and, because each case faults on one named field whose value the text repeats, when a
ctypes.Structure of detection_3d_amd/_lib.py and its C struct disagree on the order, type or padding of the fields: the
cases reach the first, a middle and the last field of each struct.

Not here: d3d_tsdf_touch on an empty batch (it still reads the state words back, which needs the device)."""
import ctypes
import math

import pytest

FAKE = 0x10000                                   # a device address that is never read
INF, NAN = math.inf, math.nan


def _frames(**over):
    from detection_3d_amd._lib import DepthFramesDesc
    d = DepthFramesDesc(FAKE, 1, FAKE, 1, FAKE, FAKE, 2, 3, 4, 0.001)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _volume(**over):
    from detection_3d_amd._lib import TsdfVolumeDesc
    d = TsdfVolumeDesc(0.125, 0.5, (0.0, 0.0, 0.0), FAKE, 1024, FAKE, 64, 3, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _mesh(**over):
    from detection_3d_amd._lib import TriangleMeshDesc
    d = TriangleMeshDesc(FAKE, 8, FAKE, 12, FAKE, 1)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _call(name, frames, volume, mesh, min_depth=0.0, ncols=9, rows=1):
    """the entry point with its descriptors and otherwise valid arguments; scratch of 0 bytes, so a call that passes every
    argument check of its descriptors still ends before a launch ("scratch too small")"""
    from detection_3d_amd._lib import lib
    L = lib()
    i32 = (ctypes.c_int * 3)(rows, rows, 0)
    i64 = (ctypes.c_int64 * 2)(rows, 0)
    args = {
        "d3d_unproject_count": (frames, 1, min_depth, INF, FAKE, 0, i32, None),
        "d3d_unproject_rows": (frames, 1, min_depth, INF, 256.0, 0.05, ncols, i32, FAKE, 0, FAKE, None, None),
        "d3d_tsdf_touch": (frames, 1, min_depth, INF, volume, 4, i32, None),
        "d3d_tsdf_integrate": (frames, min_depth, INF, 256.0, volume, 0, None, None),
        "d3d_tsdf_surface_count": (volume, 1.0, FAKE, 0, i32, None),
        "d3d_tsdf_surface_rows": (volume, 1.0, ncols, i32, FAKE, 0, FAKE, None, None),
        "d3d_tsdf_mesh_count": (volume, 1.0, FAKE, 0, i32, None),
        "d3d_tsdf_mesh_vertices": (volume, i32, FAKE, 0, FAKE, None, None, None),
        "d3d_tsdf_mesh_triangles": (volume, i32, FAKE, 0, FAKE, None),
        "d3d_tsdf_insert_blocks": (FAKE, 3, volume, None),
        "d3d_render_bin": (mesh, frames, FAKE, 0, i64, None),
        "d3d_render_fill": (mesh, frames, i64, FAKE, 0, FAKE, None),
        "d3d_render_tiles": (mesh, frames, min_depth, INF, i64, FAKE, 0, FAKE, None, None),
    }[name]
    rc = getattr(L, name)(*args)
    return rc, (L.d3d_last_error() or b"").decode(), i32, i64


FRAMES_READ = ("d3d_unproject_count", "d3d_unproject_rows", "d3d_tsdf_touch", "d3d_tsdf_integrate", "d3d_render_tiles")
FRAMES_SHAPE = FRAMES_READ + ("d3d_render_bin", "d3d_render_fill")
GEOMETRY = ("d3d_tsdf_touch", "d3d_tsdf_integrate", "d3d_tsdf_surface_rows", "d3d_tsdf_mesh_vertices")
GROW = ("d3d_tsdf_touch", "d3d_tsdf_insert_blocks")
LOOKUP = ("d3d_tsdf_surface_count", "d3d_tsdf_surface_rows", "d3d_tsdf_mesh_count", "d3d_tsdf_mesh_vertices",
          "d3d_tsdf_mesh_triangles")
VOLUME = GEOMETRY + GROW[1:] + LOOKUP[:1] + LOOKUP[2:3] + LOOKUP[4:]
RENDER = ("d3d_render_bin", "d3d_render_fill", "d3d_render_tiles")

# (entry points, which descriptor, the one bad field, the text that names the entry point (%s) and the faulty quantity)
BAD = [
    (FRAMES_SHAPE, "frames", dict(frames=-1), "%s: -1 frames of 3 x 4 pixels"),
    (FRAMES_SHAPE, "frames", dict(width=0), "%s: 2 frames of 3 x 0 pixels"),
    (FRAMES_SHAPE, "frames", dict(height=32768, width=32768), "%s: 2 x 32768 x 32768 = 2147483648 pixels do not fit 31 bits"),
    (FRAMES_READ, "frames", dict(depth_scale=0.0), "%s: depth_scale 0 must be positive and finite"),
    (FRAMES_READ, "frames", dict(depth=None), "%s: null pointer"),
    (FRAMES_READ[1:], "frames", dict(extrinsics=None), "%s: null pointer"),
    (GEOMETRY, "volume", dict(voxel=0.0), "%s: voxel 0 must be positive and finite"),
    (GEOMETRY, "volume", dict(origin=(0.0, INF, 0.0)), "%s: origin[1] = inf must be finite"),
    (GEOMETRY[1:2], "volume", dict(trunc=-1.0), "%s: trunc -1 must be positive and finite"),
    (GROW, "volume", dict(table_slots=1000), "%s: the table has d3d_tsdf_table_slots(max_blocks) slots; null pointer"),
    (GROW, "volume", dict(max_blocks=600), "%s: the table has d3d_tsdf_table_slots(max_blocks) slots; null pointer"),
    (GROW, "volume", dict(max_blocks=0), "%s: max_blocks 0 outside [1, 2^22]"),
    (GROW, "volume", dict(state=None), "%s: the table has d3d_tsdf_table_slots(max_blocks) slots; null pointer"),
    (LOOKUP, "volume", dict(table_slots=1000), "%s: null pointer, or a table of fewer than two slots per block"),
    (LOOKUP, "volume", dict(n_blocks=600), "%s: null pointer, or a table of fewer than two slots per block"),
    (LOOKUP, "volume", dict(order=None), "%s: null pointer, or a table of fewer than two slots per block"),
    (LOOKUP + GEOMETRY[1:2], "volume", dict(n_blocks=-1), "%s: -1 blocks"),
    (("d3d_tsdf_surface_rows", "d3d_tsdf_mesh_vertices"), "volume", dict(color_weight=None),
     "%s: colour and colour weight go together"),
    (("d3d_tsdf_surface_rows", "d3d_tsdf_mesh_vertices"), "volume", dict(color_state=None),
     "%s: colour and colour weight go together"),
    (("d3d_tsdf_integrate",), "volume", dict(color_weight=None), "%s: a colour image and a volume without colour"),
    (RENDER, "mesh", dict(n_vertices=-1), "%s: -1 vertices, 12 triangles"),
    (RENDER, "mesh", dict(n_triangles=-5), "%s: 8 vertices, -5 triangles"),
    (RENDER[2:], "mesh", dict(vertex_color=None), "%s: a colour image needs vertex colours and the reverse"),
    (RENDER[2:], "frames", dict(color=None), "%s: a colour image needs vertex colours and the reverse"),
]


@pytest.mark.parametrize("names,which,fields,text", BAD, ids=[f"{b[1]}-{'-'.join(b[2])}-{i}" for i, b in enumerate(BAD)])
def test_one_bad_field(names, which, fields, text):
    for name in names:
        desc = dict(frames=_frames(), volume=_volume(), mesh=_mesh())
        desc[which] = dict(frames=_frames, volume=_volume, mesh=_mesh)[which](**fields)
        rc, err, _, _ = _call(name, **desc)
        assert rc != 0 and (text % name) in err, (name, fields, rc, err)


def test_the_baseline_passes_every_descriptor_check():
    """what the cases above change one field of is valid: every entry point gets as far as its scratch, or, where it has
    none, is left out (d3d_tsdf_touch, _integrate and _insert_blocks would launch)"""
    for name in FRAMES_SHAPE + LOOKUP:
        if name in ("d3d_tsdf_touch", "d3d_tsdf_integrate"):
            continue
        rc, err, _, _ = _call(name, _frames(), _volume(), _mesh())
        assert rc != 0 and err == f"{name}: scratch too small", (name, rc, err)


@pytest.mark.parametrize("name", FRAMES_SHAPE + tuple(v for v in VOLUME if v not in FRAMES_SHAPE))
def test_null_descriptor(name):
    for which in ("frames", "volume", "mesh"):
        desc = dict(frames=_frames(), volume=_volume(), mesh=_mesh())
        takes = dict(frames=name in FRAMES_SHAPE, volume=name in VOLUME, mesh=name in RENDER)[which]
        if not takes:
            continue
        desc[which] = None
        rc, err, _, _ = _call(name, **desc)
        assert rc != 0 and f"{name}: null pointer" in err, (name, which, rc, err)


@pytest.mark.parametrize("name", FRAMES_READ)
def test_nan_depth_range(name):
    rc, err, _, _ = _call(name, _frames(), _volume(), _mesh(), min_depth=NAN)
    assert rc != 0 and f"{name}: min_depth / max_depth is NaN" in err, (rc, err)


@pytest.mark.parametrize("name", ["d3d_unproject_rows", "d3d_tsdf_surface_rows"])
def test_four_columns(name):
    rc, err, _, _ = _call(name, _frames(), _volume(), _mesh(), ncols=4)
    assert rc != 0 and f"{name}: 4 columns (3, 6 or 9)" in err, (rc, err)


def test_empty_batch_volume_and_mesh_are_fine():
    no_frames, no_blocks = _frames(frames=0), _volume(n_blocks=0)
    for name in FRAMES_SHAPE:
        if name == "d3d_tsdf_touch":
            continue
        frames, volume = (_frames(), no_blocks) if name == "d3d_tsdf_integrate" else (no_frames, _volume())
        rc, err, i32, i64 = _call(name, frames, volume, _mesh(), rows=0)
        assert rc == 0, (name, rc, err)
        assert i32[0] == 0 and i64[0] == 0, name
    for name in LOOKUP:
        rc, err, i32, _ = _call(name, _frames(), no_blocks, _mesh(), rows=0)
        assert rc == 0 and i32[0] == 0 and i32[1] == 0, (name, rc, err)
    for name in ("d3d_render_bin", "d3d_render_fill"):
        rc, err, _, i64 = _call(name, _frames(), _volume(), _mesh(n_triangles=0))
        assert rc == 0, (name, rc, err)
    from detection_3d_amd._lib import lib
    assert lib().d3d_tsdf_insert_blocks(None, 0, _volume(), None) == 0
