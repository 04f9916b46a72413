"""detection_3d_amd._cloud without a GPU: the stride rule on CPU tensors, the one check order of every raw-scan op (type
and shape, float32, device), the number and option-dict checks, and the import order of frame and register."""
import math
import os
import subprocess
import sys

import pytest
import torch

from detection_3d_amd import _cloud
from detection_3d_amd._lib import D3DError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wide():
    return torch.arange(45, dtype=torch.float32).reshape(5, 9)


STRIDE_CASES = [
    # name, the argument, read in place (the same tensor) or copied, n, row stride in floats
    ("contiguous", lambda: torch.zeros(5, 3), True, 5, 3),
    ("columns 0:3 of nine", lambda: _wide()[:, :3], True, 5, 9),
    ("columns 6:9 of nine", lambda: _wide()[:, 6:9], True, 5, 9),
    ("transposed", lambda: torch.zeros(3, 5).T, False, 5, 3),
    ("a broadcast row", lambda: torch.zeros(1, 3).expand(5, 3), False, 5, 3),
    ("one row of nine", lambda: _wide()[:1, :3], True, 1, 9),
    ("one broadcast row", lambda: torch.zeros(3).expand(1, 3), True, 1, 3),
    ("no row", lambda: torch.zeros(0, 3), True, 0, 3),
    ("no row of nine", lambda: torch.zeros(0, 9)[:, :3], True, 0, 9),
]


@pytest.mark.parametrize("name,make,in_place,n,stride", STRIDE_CASES, ids=[c[0] for c in STRIDE_CASES])
def test_stride_rule(name, make, in_place, n, stride):
    t = make()
    got, got_n, got_stride = _cloud.in_place(t)
    assert (got_n, got_stride) == (n, stride)
    assert got.shape[0] == n and got.shape[1] >= 3
    if in_place:
        assert got.data_ptr() == t.data_ptr() and got is t            # read where it lies, storage offset included
    else:
        assert got.data_ptr() != t.data_ptr() and got.is_contiguous() and tuple(got.shape) == (n, 3)
        assert torch.equal(got, t[:, :3])
    if name == "columns 6:9 of nine":
        assert got.storage_offset() == 6


def test_the_stride_rule_copies_three_columns_only():
    t = torch.arange(45, dtype=torch.float32).reshape(9, 5).T           # [5, 9], transposed storage
    got, n, stride = _cloud.in_place(t)
    assert tuple(got.shape) == (5, 3) and (n, stride) == (5, 3) and torch.equal(got, t[:, :3])


def test_rows_check_order():
    x = torch.zeros(4, 3)
    for bad in ([[0.0, 0.0, 1.0]], torch.zeros(12), torch.zeros(4, 2)):
        with pytest.raises(ValueError):
            _cloud.gpu_rows(bad)
    with pytest.raises(ValueError):
        _cloud.gpu_rows(torch.zeros(4, 4), "normals", exact=True)       # exact: four columns are one too many
    with pytest.raises(ValueError, match="normals"):
        _cloud.gpu_rows(torch.zeros(4, 2), "normals")
    with pytest.raises(ValueError, match="float32"):
        _cloud.gpu_rows(x.double())                                     # the dtype comes before the device
    with pytest.raises(D3DError):
        _cloud.gpu_rows(x)
    with pytest.raises(D3DError):
        _cloud.gpu_rows(torch.zeros(4, 9))
    assert not issubclass(D3DError, ValueError)                         # the two outcomes above are distinct


def _boxes():
    return torch.tensor([[0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0]])


def _ops():
    from detection_3d_amd.clean import radius_neighbors
    from detection_3d_amd.frame import manhattan_frame
    from detection_3d_amd.normals import estimate_normals
    from detection_3d_amd.planes import segment_planes
    from detection_3d_amd.primitives import points_in_boxes
    from detection_3d_amd.register import nearest
    return {"radius_neighbors": radius_neighbors, "segment_planes": lambda x: segment_planes(x, torch.zeros(4, 3)),
            "estimate_normals": estimate_normals, "nearest": lambda x: nearest(x, torch.zeros(4, 3)),
            "manhattan_frame": manhattan_frame, "points_in_boxes": lambda x: points_in_boxes(x, _boxes())}


@pytest.mark.parametrize("op", ["radius_neighbors", "segment_planes", "estimate_normals", "nearest", "manhattan_frame",
                                "points_in_boxes"])
def test_every_module_checks_the_dtype_before_the_device(op):
    fn = _ops()[op]
    with pytest.raises(ValueError):
        fn(torch.zeros(4, 3, dtype=torch.float64))                      # on the CPU and not float32: the argument fault
    with pytest.raises(D3DError):
        fn(torch.zeros(4, 3))


def test_same_device():
    a, b = torch.zeros(1), torch.zeros(1, device="meta")
    assert _cloud.same_device(xyz=a, normals=a, size=None) == a.device
    with pytest.raises(ValueError, match="xyz is on cpu, normals on meta"):
        _cloud.same_device(xyz=a, normals=b)


NOT_NUMBERS = ("wide", None, [1.0], float("nan"), float("inf"), -float("inf"))
NUMBER_CASES = [
    # keywords of number, accepted boundary, rejected boundary
    (dict(lo_open=True), 5e-324, 0.0),                                  # positive and finite
    (dict(), 0.0, -5e-324),                                             # finite and not negative
    (dict(lo=0.0, hi=90.0), 90.0, 90.00000000000001),                   # [0, 90]
    (dict(lo=0.0, hi=90.0), 0.0, -1e-300),
    (dict(lo=0.0, hi=20.0, lo_open=True), 20.0, 0.0),                   # (0, 20]
]


@pytest.mark.parametrize("kw,good,bad", NUMBER_CASES)
def test_number(kw, good, bad):
    got = _cloud.number(good, "radius", **kw)
    assert got == good and type(got) is float
    for value in (bad,) + NOT_NUMBERS:
        with pytest.raises(ValueError, match="radius"):
            _cloud.number(value, "radius", **kw)
    # float() decides what a number is, as every copy of this check did: a bool is 1.0 or 0.0, an int is its value
    assert _cloud.number(True, "radius", **kw) == 1.0 and _cloud.number(1, "radius", **kw) == 1.0


def test_number_names_the_range():
    for kw, text in ((dict(lo_open=True), "> 0"), (dict(), ">= 0"), (dict(hi=90.0), "[0, 90]"),
                     (dict(hi=20.0, lo_open=True), "(0, 20]")):
        with pytest.raises(ValueError) as e:
            _cloud.number(-1.0, "tol", **kw)
        assert "tol" in str(e.value) and text in str(e.value)


def test_whole():
    assert _cloud.whole(1, "k") == 1 and _cloud.whole(2.0, "k") == 2 and type(_cloud.whole(2.0, "k")) is int
    assert _cloud.whole(10 ** 12, "k") == 10 ** 12                      # hi=None: no upper bound
    assert _cloud.whole(0, "k", 0) == 0 and _cloud.whole(32, "k", 32, 4096) == 32 and _cloud.whole(4096, "k", 32, 4096) == 4096
    for bad in (0, -3, 2.5, True, False, "2", "many", None, float("nan"), float("inf"), [1]):
        with pytest.raises(ValueError, match="k"):
            _cloud.whole(bad, "k")
    for bad in (31, 4097, 64.5, True):
        with pytest.raises(ValueError) as e:
            _cloud.whole(bad, "lattice: Lx", 32, 4096)
        assert "lattice: Lx" in str(e.value) and "[32, 4096]" in str(e.value)
    with pytest.raises(ValueError, match=">= 1"):
        _cloud.whole(0, "k")


def test_options():
    keys = ("radius", "max_nn")
    assert _cloud.options(None, "normals", keys) is None
    given = {"radius": 0.2}
    got = _cloud.options(given, "normals", keys)
    assert got == given and got is not given
    assert _cloud.options({}, "normals", keys) == {}
    with pytest.raises(ValueError) as e:
        _cloud.options({"radius": 0.2, "size": 1, "colour": 2}, "normals", keys)
    assert "unknown keywords ['colour', 'size']" in str(e.value) and "radius, max_nn" in str(e.value)
    for bad in (0.2, "estimate", [("radius", 0.2)], True):
        with pytest.raises(ValueError) as e:
            _cloud.options(bad, "normals", keys, "None, 'estimate'")
        assert "normals must be None, 'estimate' or a dict with keys among radius, max_nn" in str(e.value)


def test_the_kwargs_functions_keep_their_special_forms():
    from detection_3d_amd.clean import clean_kwargs
    from detection_3d_amd.downsample import downsample_kwargs
    from detection_3d_amd.frame import align_kwargs
    from detection_3d_amd.normals import normals_kwargs
    from detection_3d_amd.primitives import MIN_POINTS_ANY, fit_kwargs
    from detection_3d_amd.unproject import unproject_kwargs
    assert clean_kwargs(None) is None and clean_kwargs({}) == {"radius": 0.1}
    assert normals_kwargs(None) is None and normals_kwargs("estimate") == {} and normals_kwargs({"max_nn": 9}) == {"max_nn": 9}
    assert downsample_kwargs(None) is None and downsample_kwargs(0.05) == {"voxel": 0.05, "seed": 0}
    assert align_kwargs(None) is None and align_kwargs(False) is None
    assert align_kwargs(True) == align_kwargs("manhattan") == {"max_tilt": 30.0, "tol": 5.0, "up": None}
    assert unproject_kwargs(None) == {} and unproject_kwargs({"step": 2}) == {"step": 2}
    assert fit_kwargs(None) == {"min_points": MIN_POINTS_ANY, "min_size": (0.0, 0.0, 0.0)}
    assert fit_kwargs({"min_points": 0})["min_points"] == 0
    for fn, what in ((clean_kwargs, "clean"), (normals_kwargs, "normals"), (downsample_kwargs, "downsample"),
                     (align_kwargs, "align"), (unproject_kwargs, "unproject"), (fit_kwargs, "fit")):
        with pytest.raises(ValueError) as e:
            fn({"colour": 1})
        assert f"{what}: unknown keywords ['colour']" in str(e.value)
        with pytest.raises(ValueError) as e:
            fn([1])
        assert f"{what} must be None" in str(e.value) and "or a dict with keys among" in str(e.value)


def test_clean_cloud_validates_through_clean_kwargs():
    from detection_3d_amd.clean import clean_cloud, clean_kwargs
    pcl = torch.zeros(4, 3)
    for bad in ({"statistical": (0, 1.0)}, {"statistical": (3, -1.0)}, {"statistical": 3}, {"min_neighbors": 0},
                {"min_component": 1.5}, {"radius": 0.0}):
        with pytest.raises(ValueError) as by_keyword:
            clean_kwargs(bad)
        with pytest.raises(ValueError) as by_call:
            clean_cloud(pcl, **bad)
        assert str(by_keyword.value) == str(by_call.value)
    assert clean_cloud(pcl) is pcl and clean_cloud(pcl, return_source=True) == (pcl, None)


@pytest.mark.parametrize("module", ["frame", "register", "_cloud"])
def test_each_module_imports_on_its_own(module):
    """a fresh interpreter, one module: no import cycle hides behind the order in which a caller happens to import, and
    importing does not load the GPU library"""
    code = (f"import sys, detection_3d_amd.{module}, detection_3d_amd._lib as L; "
            "assert L._lib is None; print(sorted(m for m in sys.modules if "
            "m.startswith('detection_3d_amd.')))")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    loaded = out.stdout
    if module == "frame":
        assert "detection_3d_amd.register" not in loaded                # frame needs pose, not register
    if module == "_cloud":
        assert loaded.strip() == "['detection_3d_amd._cloud', 'detection_3d_amd._lib']"


def test_register_still_exports_the_pose_helpers():
    from detection_3d_amd import pose, register
    assert register.apply_pose is pose.apply_pose and register.inverse_pose is pose.inverse_pose
    assert math.isclose(float(register.inverse_pose(torch.eye(4))[0, 0]), 1.0)
