"""The C-ABI library loads (no GPU needed) and exports every symbol include/d3d_hip.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "d3d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(d3d_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported_and_bound():
    from detection_3d_amd import _lib
    from detection_3d_amd.build import build_library
    build_library()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) >= 30
    for n in names:
        assert hasattr(handle, n), f"{n} declared in d3d_hip.h but not exported"
    assert set(names) == set(_lib.EXPORTED_SYMBOLS), set(names) ^ set(_lib.EXPORTED_SYMBOLS)
    lib = _lib.lib()
    assert lib.d3d_abi_version() == 3
    # pure host-side helpers are callable without a GPU
    assert lib.d3d_packed_weight_bytes(27, 9, 32, 0) == 27 * 16 * 32 * 4
    assert lib.d3d_packed_weight_bytes(8, 128, 128, 0) == 8 * 128 * 128 * 4
    assert lib.d3d_packed_weight_bytes(1, 300, 128, 0) == 0
    assert lib.d3d_nms_scratch_bytes(2000) >= 2000 * 32 * 8


def test_fp32_only_twins_are_gone():
    """ABI 2: the _dt entry points serve every storage type; their fp32-only twins are not exported, declared or bound"""
    from detection_3d_amd import _lib
    from detection_3d_amd.build import build_library
    build_library()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    declared = _declared()
    for n in ("d3d_packed_weight_floats", "d3d_pack_conv_weight", "d3d_pack_conv_weight_transposed",
              "d3d_subm_conv_forward", "d3d_conv_forward", "d3d_deconv_forward", "d3d_subm_conv_backward",
              "d3d_conv_backward", "d3d_deconv_backward", "d3d_bn_batch_invstd", "d3d_bn_apply", "d3d_bn_forward",
              "d3d_bn_backward"):
        assert not hasattr(handle, n), f"{n} is still exported"
        assert n not in declared, f"{n} is still declared in d3d_hip.h"
        assert n not in _lib.EXPORTED_SYMBOLS and not hasattr(_lib.lib(), n), f"{n} is still bound"


def test_ops_refuse_cpu_tensors():
    import torch
    from detection_3d_amd import _lib, box_ops
    with pytest.raises(_lib.D3DError):
        box_ops.rotate_iou_gpu_eval(torch.zeros(2, 5), torch.zeros(2, 5))
