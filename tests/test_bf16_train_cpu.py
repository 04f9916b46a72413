"""bf16 training without a GPU: the new C-ABI symbols, their host-side size queries and argument checks, the dtype guards
of the backward wrappers, and the --bf16 option of scripts/train_ddp.py."""
import importlib.util
import os
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("d3d_subm_conv_backward_dt", "d3d_conv_backward_dt", "d3d_deconv_backward_dt",
       "d3d_pack_conv_weight_transposed_dt", "d3d_bn_forward_dt", "d3d_bn_backward_dt")


@pytest.fixture(scope="module")
def lib():
    from detection_3d_amd import _lib
    from detection_3d_amd.build import build_library
    build_library()
    return _lib.lib()


def test_new_symbols_declared_exported_bound(lib):
    import ctypes
    from detection_3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "d3d_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(handle, name), name


def test_size_queries_answer_for_bf16(lib):
    from detection_3d_amd.sparseconvnet import SCN
    # W^T of the detector's layers in bf16 storage: Cin' = Cout, Cout' = Cin
    for fv, cin, cout in ((27, 32, 32), (8, 32, 64), (1, 32, 128), (1, 256, 128), (8, 128, 256), (27, 256, 256)):
        assert lib.d3d_packed_weight_bytes(fv, cout, cin, SCN.BF16) == fv * cout * cin * 2
    assert lib.d3d_packed_weight_bytes(27, 9, 32, SCN.BF16) == 27 * 16 * 32 * 2      # the first layer: 9 -> 16
    assert lib.d3d_packed_weight_bytes(27, 300, 32, SCN.BF16) == 0
    # the fixed-order dW partials are fp32 of the weight's size, whatever the storage type
    assert lib.d3d_conv_dw_scratch_bytes(27, 9, 32) == 32 * 27 * 9 * 32 * 4
    assert lib.d3d_bn_backward_scratch_bytes(128) > 0 and lib.d3d_bn_scratch_bytes(128) > 0


def test_bf16_entry_points_refuse_before_launch(lib):
    from detection_3d_amd import _lib
    ints = _lib.ints
    p = 0x1000          # placeholders: every call below fails its checks before it touches memory
    size, filt = ints([8, 8, 8]), ints([3, 3, 3])
    # unsupported bf16 shapes: D3D_ERR_UNSUPPORTED (-5)
    assert lib.d3d_subm_conv_backward_dt(None, size, filt, p, 48, 48, None, 32, p, None, p, 1, None) == -5
    assert lib.d3d_subm_conv_backward_dt(None, size, filt, p, 32, 32, None, 48, p, None, p, 1, None) == -5
    assert lib.d3d_subm_conv_backward_dt(None, size, filt, p, 32, 9, None, 32, p, None, p, 1, None) == -5   # 9 -> 16
    assert lib.d3d_subm_conv_backward_dt(None, size, filt, p, 16, 9, p, 32, p, p, p, 1, None) == -5        # no dInput
    assert lib.d3d_conv_backward_dt(None, size, size, filt, filt, p, 512, 512, None, 32, p, None, p, 1, None) == -5
    assert lib.d3d_deconv_backward_dt(None, size, size, filt, filt, p, 32, 32, None, 16, p, None, p, 1, None) == -5
    assert lib.d3d_pack_conv_weight_transposed_dt(p, 27, 9, 32, 1, p, 1, None) == -5
    # unknown storage types and bad arguments: D3D_ERR_ARG (-1)
    assert lib.d3d_subm_conv_backward_dt(None, size, filt, p, 32, 32, None, 32, p, None, p, 2, None) == -1
    assert lib.d3d_subm_conv_backward_dt(None, size, filt, p, 16, 9, None, 32, p, None, p, 0, None) == -1  # fp32: cs == cin
    assert lib.d3d_bn_forward_dt(p, p, 10, 32, None, None, None, None, None, None, 1e-4, 0.9, 1, 0.0, p, 1 << 20, 2,
                                 None) == -1
    assert lib.d3d_bn_backward_dt(p, p, p, p, 10, 32, p, p, None, None, None, 0.0, p, 1 << 20, 2, None) == -1


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append(name)
            return 0
        return f


def test_backward_wrappers_guard_dtypes(monkeypatch):
    """float16 rows, and rows / gradients of different storage types, raise D3DError before any library call; bf16 rows
    reach the _dt entry points with their stored width and the weight's Cin"""
    from detection_3d_amd._lib import D3DError
    from detection_3d_amd.sparseconvnet import SCN
    rec = _Recorder()
    monkeypatch.setattr(SCN, "lib", lambda: rec)
    monkeypatch.setattr(SCN, "require_gpu", lambda *t: None)
    monkeypatch.setattr(SCN, "stream_of", lambda: None)
    m = types.SimpleNamespace(_h=None)
    w = torch.zeros(27, 1, 32, 32)
    bad = ((torch.zeros(5, 32, dtype=torch.float16), torch.zeros(5, 32, dtype=torch.float16)),
           (torch.zeros(5, 32, dtype=torch.bfloat16), torch.zeros(5, 32)),
           (torch.zeros(5, 32), torch.zeros(5, 32, dtype=torch.bfloat16)))
    for feats, d_out in bad:
        with pytest.raises(D3DError):
            SCN.SubmanifoldConvolution_backward([8, 8, 8], [3, 3, 3], m, feats, None, d_out, w, torch.zeros_like(w), None,
                                                want_d_input=False)
        with pytest.raises(D3DError):
            SCN.Convolution_backward([8, 8, 8], [4, 4, 4], [2, 2, 2], [2, 2, 2], m, feats, None, d_out, w[:8],
                                     torch.zeros_like(w[:8]), None, want_d_input=False)
        with pytest.raises(D3DError):
            SCN.Deconvolution_backward([4, 4, 4], [8, 8, 8], [2, 2, 2], [2, 2, 2], m, feats, None, d_out, w[:8],
                                       torch.zeros_like(w[:8]), None, want_d_input=False)
        with pytest.raises(D3DError):
            SCN.BatchNormalization_backward(feats, feats.new_empty(0), feats, d_out, torch.zeros(32), torch.ones(32),
                                            None, None, None, None, None, None, 0.0)
    assert rec.calls == []
    # the first layer in bf16: 9 channels stored as 16, dWeight only
    w9 = torch.zeros(27, 1, 9, 32)
    SCN.SubmanifoldConvolution_backward([8, 8, 8], [3, 3, 3], m, torch.zeros(5, 16, dtype=torch.bfloat16), None,
                                        torch.zeros(5, 32, dtype=torch.bfloat16), w9, torch.zeros_like(w9), None,
                                        want_d_input=False)
    assert rec.calls == ["d3d_subm_conv_backward_dt"]
    with pytest.raises(D3DError):      # rows stored narrower than the weight expects
        SCN.SubmanifoldConvolution_backward([8, 8, 8], [3, 3, 3], m, torch.zeros(5, 9, dtype=torch.bfloat16), None,
                                            torch.zeros(5, 32, dtype=torch.bfloat16), w9, torch.zeros_like(w9), None,
                                            want_d_input=False)


def _train_ddp():
    spec = importlib.util.spec_from_file_location("train_ddp_bf16_under_test", os.path.join(ROOT, "scripts", "train_ddp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_ddp_bf16_option():
    mod = _train_ddp()
    a = mod.parse_args(["--config", "6c_Fpn4321"])
    assert a.bf16 is False
    b = mod.parse_args(["--bf16", "--ims-per-gpu", "4", "--deterministic", "--seed", "3"])
    assert b.bf16 is True and b.ims_per_gpu == 4 and b.deterministic is True and b.seed == 3
