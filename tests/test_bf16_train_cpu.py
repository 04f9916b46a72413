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


def test_fp32_rows_refused_as_by_the_fp32_only_forms(lib):
    """dtype 0 (D3D_F32) through the _dt entry points: what the removed fp32-only twins refused with D3D_ERR_ARG (-1) is
    still refused with it, and their empty calls still return D3D_OK, all before any launch"""
    from detection_3d_amd import _lib
    ints = _lib.ints
    p = 0x1000          # placeholder: never dereferenced
    size, filt = ints([8, 8, 8]), ints([3, 3, 3])
    # convolutions, forward and backward: null metadata, null sizes
    assert lib.d3d_subm_conv_forward_dt(None, size, filt, p, 32, p, 32, None, p, 0, None, None, None) == -1
    assert lib.d3d_subm_conv_forward_dt(p, None, filt, p, 32, p, 32, None, p, 0, None, None, None) == -1
    assert lib.d3d_conv_forward_dt(None, size, size, filt, filt, p, 32, p, 32, p, 0, None, None, None) == -1
    assert lib.d3d_conv_forward_dt(p, size, size, filt, None, p, 32, p, 32, p, 0, None, None, None) == -1
    assert lib.d3d_deconv_forward_dt(None, size, size, filt, filt, p, 32, p, 32, None, p, 0, None, None, None) == -1
    assert lib.d3d_deconv_forward_dt(p, size, None, filt, filt, p, 32, p, 32, None, p, 0, None, None, None) == -1
    assert lib.d3d_subm_conv_backward_dt(None, size, filt, p, 32, 32, p, 32, p, p, p, 0, None) == -1
    assert lib.d3d_subm_conv_backward_dt(p, size, None, p, 32, 32, p, 32, p, p, p, 0, None) == -1
    assert lib.d3d_conv_backward_dt(None, size, size, filt, filt, p, 32, 32, p, 32, p, p, p, 0, None) == -1
    assert lib.d3d_conv_backward_dt(p, size, size, filt, None, p, 32, 32, p, 32, p, p, p, 0, None) == -1
    assert lib.d3d_deconv_backward_dt(None, size, size, filt, filt, p, 32, 32, p, 32, p, p, p, 0, None) == -1
    assert lib.d3d_deconv_backward_dt(p, size, None, filt, filt, p, 32, 32, p, 32, p, p, p, 0, None) == -1
    # packing: null pointers, no filter, no output channel, Cin (W^T: Cout) past 256
    assert lib.d3d_pack_conv_weight_dt(None, 27, 32, 32, p, 0, None) == -1
    assert lib.d3d_pack_conv_weight_dt(p, 27, 32, 32, None, 0, None) == -1
    assert lib.d3d_pack_conv_weight_dt(p, 0, 32, 32, p, 0, None) == -1
    assert lib.d3d_pack_conv_weight_dt(p, 27, 32, 0, p, 0, None) == -1
    assert lib.d3d_pack_conv_weight_dt(p, 27, 300, 32, p, 0, None) == -1
    assert lib.d3d_pack_conv_weight_transposed_dt(None, 27, 32, 32, 1, p, 0, None) == -1
    assert lib.d3d_pack_conv_weight_transposed_dt(p, 27, 32, 32, 1, None, 0, None) == -1
    assert lib.d3d_pack_conv_weight_transposed_dt(p, 0, 32, 32, 1, p, 0, None) == -1
    assert lib.d3d_pack_conv_weight_transposed_dt(p, 27, 0, 32, 1, p, 0, None) == -1
    assert lib.d3d_pack_conv_weight_transposed_dt(p, 27, 32, 300, 1, p, 0, None) == -1
    # BatchNorm statistics and apply: null pointers, no rows, no planes; an empty apply is D3D_OK
    assert lib.d3d_bn_batch_invstd_dt(None, 10, 32, 1e-4, p, p, p, 1 << 20, 0, None) == -1
    assert lib.d3d_bn_batch_invstd_dt(p, 10, 32, 1e-4, None, p, p, 1 << 20, 0, None) == -1
    assert lib.d3d_bn_batch_invstd_dt(p, 10, 32, 1e-4, p, None, p, 1 << 20, 0, None) == -1
    assert lib.d3d_bn_batch_invstd_dt(p, 0, 32, 1e-4, p, p, p, 1 << 20, 0, None) == -1
    assert lib.d3d_bn_batch_invstd_dt(p, 10, 30, 1e-4, p, p, p, 1 << 20, 0, None) == -1      # planes % 4
    assert lib.d3d_bn_batch_invstd_dt(p, 10, 32, 1e-4, p, p, None, 0, 0, None) == -1         # no scratch
    assert lib.d3d_bn_apply_dt(None, None, 0, 32, None, None, None, None, 0.0, 0, None) == 0
    assert lib.d3d_bn_apply_dt(None, p, 10, 32, p, p, None, None, 0.0, 0, None) == -1
    assert lib.d3d_bn_apply_dt(p, None, 10, 32, p, p, None, None, 0.0, 0, None) == -1
    assert lib.d3d_bn_apply_dt(p, p, 10, 32, None, p, None, None, 0.0, 0, None) == -1
    assert lib.d3d_bn_apply_dt(p, p, 10, 32, p, None, None, None, 0.0, 0, None) == -1
    assert lib.d3d_bn_apply_dt(p, p, 10, 0, p, p, None, None, 0.0, 0, None) == -1
    assert lib.d3d_bn_apply_dt(p, p, -1, 32, p, p, None, None, 0.0, 0, None) == -1
    # BatchNorm forward and backward: null statistics, no planes, negative rows, null features; no rows is D3D_OK
    def fwd(i, o, rows, planes, save_mean):
        return lib.d3d_bn_forward_dt(i, o, rows, planes, save_mean, p, p, p, None, None, 1e-4, 0.9, 1, 0.0, p, 1 << 20, 0, None)

    assert fwd(p, p, 10, 32, None) == -1
    assert fwd(p, p, 10, 0, p) == -1
    assert fwd(p, p, -1, 32, p) == -1
    assert fwd(None, None, 0, 32, p) == 0
    assert fwd(None, p, 10, 32, p) == -1
    assert fwd(p, None, 10, 32, p) == -1

    def bwd(i, o, g, d, rows, planes, save_mean, scratch, nbytes):
        return lib.d3d_bn_backward_dt(i, o, g, d, rows, planes, save_mean, p, None, None, None, 0.0, scratch, nbytes, 0, None)

    assert bwd(p, p, p, p, 10, 0, p, p, 1 << 20) == -1
    assert bwd(p, p, p, p, -1, 32, p, p, 1 << 20) == -1
    assert bwd(p, p, p, p, 10, 32, None, p, 1 << 20) == -1
    assert bwd(None, None, None, None, 0, 32, p, p, 1 << 20) == 0
    assert bwd(None, p, p, p, 10, 32, p, p, 1 << 20) == -1
    assert bwd(p, p, p, None, 10, 32, p, p, 1 << 20) == -1
    assert bwd(p, p, p, p, 10, 48, p, p, 1 << 20) == -1                                     # 256 % planes
    assert bwd(p, p, p, p, 10, 32, p, None, 0) == -1                                        # no scratch


class _Recorder:
    def __init__(self):
        self.calls = []
        self.args = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append(name)
            self.args.append(args)
            return 0
        return f


@pytest.mark.parametrize("transposed", [False, True])
def test_pack_paths_make_one_call_per_storage_type(monkeypatch, transposed):
    """pack_weight / pack_weight_transposed: the size query, a buffer whose element type names the d3d_dtype, the _dt pack
    call -- and for a contiguous fp32 parameter no copy of it, whatever the code"""
    from detection_3d_amd.sparseconvnet import SCN

    class Rec(_Recorder):
        def d3d_packed_weight_bytes(self, fv, cin, cout, code):
            self.calls.append("d3d_packed_weight_bytes")
            self.args.append((fv, cin, cout, code))
            return fv * cin * cout * (2 if code == SCN.BF16 else 4)

    monkeypatch.setattr(SCN, "require_gpu", lambda *t: None)
    monkeypatch.setattr(SCN, "stream_of", lambda: None)
    w = torch.nn.Parameter(torch.zeros(27, 1, 32, 64))
    entry = "d3d_pack_conv_weight_transposed_dt" if transposed else "d3d_pack_conv_weight_dt"
    for code, elem in ((SCN.F32, torch.float32), (SCN.BF16, torch.bfloat16), (SCN.F32_X3, torch.int16)):
        rec = Rec()
        monkeypatch.setattr(SCN, "lib", lambda: rec)
        dtype = torch.bfloat16 if code == SCN.BF16 else torch.float32
        packed = SCN.pack_weight_transposed(w, True, dtype, code) if transposed else SCN.pack_weight(w, dtype, code)
        assert rec.calls == ["d3d_packed_weight_bytes", entry]
        assert rec.args[0] == ((27, 64, 32, code) if transposed else (27, 32, 64, code))
        assert packed.dtype == elem and packed.numel() * packed.element_size() == 27 * 32 * 64 * (2 if code == SCN.BF16 else 4)
        assert SCN._packed_code(packed) == code
        call = rec.args[1]
        assert call[0].value == w.data_ptr()                      # the parameter itself: no cast, no copy, no launch
        assert call[1:4] == (27, 32, 64) and call[-2] == code
        assert (call[5] if transposed else call[4]).value == packed.data_ptr()


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
