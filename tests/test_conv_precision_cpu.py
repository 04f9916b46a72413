"""torch's fp32 matmul precision setting -> d3d_dtype of the sparse convolutions (no GPU needed).

'highest' / 'ieee' / unset keep D3D_F32 (today's calls); 'high' / 'medium' / 'tf32' select D3D_F32_X3 (bf16x3
products, include/d3d_hip.h); bf16 storage stays D3D_BF16 whatever the setting."""
import pytest
import torch


@pytest.fixture(autouse=True)
def _restore_precision():
    """every test here changes the setting: both of torch's knobs are put back afterwards"""
    matmul, generic = torch.backends.cuda.matmul.fp32_precision, torch.backends.fp32_precision
    try:
        yield
    finally:
        torch.backends.fp32_precision = generic
        torch.backends.cuda.matmul.fp32_precision = matmul


def _code(dtype=torch.float32):
    from detection_3d_amd.sparseconvnet import SCN
    return SCN.conv_dtype_code(dtype)


def test_packed_weight_bytes_of_x3():
    from detection_3d_amd import _lib
    from detection_3d_amd.build import build_library
    build_library()
    lib = _lib.lib()
    assert lib.d3d_packed_weight_bytes(27, 128, 128, 2) == 27 * 128 * 128 * 4
    assert lib.d3d_packed_weight_bytes(8, 64, 256, 2) == 8 * 64 * 256 * 4
    # shapes the bf16x3 kernel does not serve pack as fp32 for k_conv: the same bytes as D3D_F32
    assert lib.d3d_packed_weight_bytes(27, 9, 32, 2) == lib.d3d_packed_weight_bytes(27, 9, 32, 0) == 27 * 16 * 32 * 4
    assert lib.d3d_packed_weight_bytes(1, 300, 128, 2) == 0


def test_codes():
    from detection_3d_amd.sparseconvnet import SCN
    assert (SCN.F32, SCN.BF16, SCN.F32_X3) == (0, 1, 2)


def test_unset_is_exact():
    torch.backends.fp32_precision = "none"
    torch.backends.cuda.matmul.fp32_precision = "none"
    assert _code() == 0


@pytest.mark.parametrize("level,want", [("high", 2), ("medium", 2), ("highest", 0)])
def test_legacy_api(level, want):
    torch.set_float32_matmul_precision(level)
    assert _code() == want
    assert _code(torch.bfloat16) == 1


@pytest.mark.parametrize("value,want", [("tf32", 2), ("ieee", 0)])
def test_new_api(value, want):
    torch.backends.cuda.matmul.fp32_precision = value
    assert _code() == want
    assert _code(torch.bfloat16) == 1


def test_generic_setting_when_matmul_is_none():
    torch.backends.cuda.matmul.fp32_precision = "none"
    torch.backends.fp32_precision = "tf32"
    assert _code() == 2


def test_mixed_apis_never_raise():
    """torch.get_float32_matmul_precision() raises once both APIs were used; the mapping does not"""
    torch.set_float32_matmul_precision("high")
    torch.backends.cuda.matmul.fp32_precision = "ieee"
    assert _code() == 0
    torch.set_float32_matmul_precision("medium")
    assert _code() == 2
    torch.backends.cuda.matmul.fp32_precision = "tf32"
    torch.set_float32_matmul_precision("highest")
    assert _code() == 0


def test_cudnn_conv_flag_is_not_read():
    torch.backends.cuda.matmul.fp32_precision = "ieee"
    assert torch.backends.cudnn.conv.fp32_precision == "tf32"     # torch's default
    assert _code() == 0


def test_other_dtypes_refused():
    from detection_3d_amd import _lib
    with pytest.raises(_lib.D3DError):
        _code(torch.float16)
