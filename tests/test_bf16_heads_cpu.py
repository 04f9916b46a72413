"""bf16 heads without a GPU: the new C-ABI symbols, their size queries and argument checks, the validation of
SparseRCNN.head_dtype, and the --bf16-heads option of scripts/train_ddp.py."""
import ctypes
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("d3d_rpn_head_bf16", "d3d_roi_align_rotated_3d_sparse_forward_bf16",
       "d3d_roi_align_rotated_3d_sparse_forward_levels_bf16", "d3d_roi_align_rotated_3d_sparse_backward_bf16",
       "d3d_roi_align_rotated_3d_sparse_backward_bf16_scratch_bytes",
       "d3d_roi_align_rotated_3d_sparse_backward_deterministic_bf16",
       "d3d_roi_align_rotated_3d_sparse_backward_deterministic_bf16_scratch_bytes")


@pytest.fixture(scope="module")
def lib():
    from detection_3d_amd import _lib
    from detection_3d_amd.build import build_library
    build_library()
    return _lib.lib()


def test_new_symbols_declared_exported_bound(lib):
    from detection_3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "d3d_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(handle, name), name
        assert name in integration or name.replace("_scratch_bytes", "") in integration, name


def test_size_queries_answer(lib):
    assert lib.d3d_roi_align_rotated_3d_sparse_backward_bf16_scratch_bytes(128, 1000) >= 128 * 1000 * 4
    assert lib.d3d_roi_align_rotated_3d_sparse_backward_bf16_scratch_bytes(128, 0) > 0
    assert lib.d3d_roi_align_rotated_3d_sparse_backward_bf16_scratch_bytes(0, 10) == 0
    assert lib.d3d_roi_align_rotated_3d_sparse_backward_bf16_scratch_bytes(128, -1) == 0
    args = (512, 128, 7, 7, 3, 2, 100000)
    det = lib.d3d_roi_align_rotated_3d_sparse_backward_deterministic_bf16_scratch_bytes(*args)
    assert det > 0 and det == lib.d3d_roi_align_rotated_3d_sparse_backward_deterministic_scratch_bytes(*args)
    assert lib.d3d_roi_align_rotated_3d_sparse_backward_deterministic_bf16_scratch_bytes(512, 128, 7, 7, 3, 0, 10) == 0


def _err(rc):
    from detection_3d_amd import _lib
    assert rc != 0
    return _lib.lib().d3d_last_error().decode()


def test_bf16_entry_points_refuse_bad_arguments(lib):
    """argument checks that return before anything touches a device"""
    vp = ctypes.c_void_p
    dummy = vp(4096)
    rows = (ctypes.c_int * 1)(64)
    maps = (vp * 1)(dummy)
    # rpn head: channels, map count, the one-tile-per-wave gate, null weights, misaligned weights
    assert "channels" in _err(lib.d3d_rpn_head_bf16(maps, rows, 1, 192, dummy, dummy, dummy, dummy, 4, dummy, dummy, None))
    assert "maps" in _err(lib.d3d_rpn_head_bf16(maps, rows, 0, 128, dummy, dummy, dummy, dummy, 4, dummy, dummy, None))
    assert "output columns" in _err(lib.d3d_rpn_head_bf16(maps, rows, 1, 128, dummy, dummy, dummy, dummy, 17, dummy,
                                                          dummy, None))
    assert "bad arguments" in _err(lib.d3d_rpn_head_bf16(maps, rows, 1, 128, None, dummy, dummy, dummy, 4, dummy, dummy,
                                                         None))
    assert "aligned" in _err(lib.d3d_rpn_head_bf16(maps, rows, 1, 128, vp(4098), dummy, dummy, dummy, 4, dummy, dummy,
                                                   None))
    size = (ctypes.c_int * 3)(8, 8, 8)
    crop = (ctypes.c_int * 3)(8, 8, 8)
    # RoI forward / backward: null metadata, bad shapes, levels, scratch
    assert _err(lib.d3d_roi_align_rotated_3d_sparse_forward_bf16(None, size, dummy, 128, crop, dummy, 4, 0.5, 7, 7, 3, 2,
                                                                 None, 0, 1, dummy, None))
    feats = (vp * 5)(*([dummy] * 5))
    scales = (ctypes.c_float * 5)(*([1.0] * 5))
    assert "levels" in _err(lib.d3d_roi_align_rotated_3d_sparse_forward_levels_bf16(
        dummy, 5, size, feats, 128, scales, dummy, 4, 7, 7, 3, 2, dummy, 1, dummy, None))
    assert "bad arguments" in _err(lib.d3d_roi_align_rotated_3d_sparse_backward_bf16(
        dummy, size, dummy, 128, crop, dummy, 4, 0.5, 7, 7, 3, 2, dummy, -1, dummy, 1 << 20, None))
    assert "scratch" in _err(lib.d3d_roi_align_rotated_3d_sparse_backward_bf16(
        dummy, size, dummy, 128, crop, dummy, 4, 0.5, 7, 7, 3, 2, dummy, 1000, dummy, 16, None))
    assert "sampling_ratio" in _err(lib.d3d_roi_align_rotated_3d_sparse_backward_deterministic_bf16(
        dummy, size, dummy, 128, crop, dummy, 4, 0.5, 7, 7, 3, 0, dummy, 1000, dummy, 1 << 30, None))
    assert "scratch" in _err(lib.d3d_roi_align_rotated_3d_sparse_backward_deterministic_bf16(
        dummy, size, dummy, 128, crop, dummy, 4, 0.5, 7, 7, 3, 2, dummy, 1000, dummy, 16, None))


def test_head_dtype_other_than_fp32_or_bf16_raises():
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.detector import SparseRCNN
    model = SparseRCNN(get_cfg("4c_Fpn432")).eval()
    assert model.head_dtype == torch.float32 and model.backbone.head_dtype == torch.float32
    for bad in (torch.float16, torch.float64, "bfloat16"):
        model.head_dtype = bad
        with pytest.raises(ValueError, match="head_dtype"):
            model([torch.zeros((4, 3), dtype=torch.int64), torch.zeros((4, 9))])
        with pytest.raises(ValueError, match="head_dtype"):
            model.stage_features(None)
    model.head_dtype = torch.bfloat16
    model._pass_head_dtype()
    assert model.backbone.head_dtype == torch.bfloat16


def test_train_ddp_bf16_heads_option():
    spec = importlib.util.spec_from_file_location("train_ddp_bf16_heads_under_test",
                                                  os.path.join(ROOT, "scripts", "train_ddp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.parse_args(["--config", "6c_Fpn4321"])
    assert a.bf16_heads is False
    b = mod.parse_args(["--bf16-heads", "--bf16", "--ims-per-gpu", "2", "--deterministic"])
    assert b.bf16_heads is True and b.bf16 is True and b.ims_per_gpu == 2 and b.deterministic is True
