"""Deterministic mode without a GPU: the torch-flag dispatch of the Python wrappers, the new C-ABI symbols and their
argument checks, and the --deterministic option of scripts/train_ddp.py."""
import importlib.util
import os
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def flag():
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    yield
    torch.use_deterministic_algorithms(was, warn_only=warn)


@pytest.fixture(scope="module")
def lib():
    from detection_3d_amd import _lib
    from detection_3d_amd.build import build_library
    build_library()
    return _lib.lib()


def test_deterministic_follows_the_torch_flag(flag):
    from detection_3d_amd import _lib
    torch.use_deterministic_algorithms(False)
    assert not _lib.deterministic()
    torch.use_deterministic_algorithms(True)
    assert _lib.deterministic()
    with pytest.raises(RuntimeError, match="my_op does not have a deterministic implementation"):
        _lib.alert_not_deterministic("my_op")
    torch.use_deterministic_algorithms(True, warn_only=True)
    with pytest.warns(UserWarning, match="my_op"):
        _lib.alert_not_deterministic("my_op")


class _Recorder:
    """stands in for the HIP library: records the calls, returns 0 (no GPU needed)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append(name)
            if name.endswith("scratch_bytes"):
                return 4096
            return 0
        return f


def _fake_ctx(grad_shape, sampling_ratio=2):
    meta = types.SimpleNamespace(_h=None)
    rois = torch.zeros((grad_shape[0], 8))
    ctx = types.SimpleNamespace(saved_tensors=(rois,),
                                args=(meta, [8, 8, 8], [8, 8, 8], 0.25, 4, 5, 3, sampling_ratio, (10, grad_shape[1])))
    return ctx


@pytest.mark.parametrize("on", [False, True])
def test_sparse_roi_backward_dispatch(monkeypatch, flag, on):
    from detection_3d_amd import roi_align_rotated_3d as R
    rec = _Recorder()
    monkeypatch.setattr(R, "lib", lambda: rec)
    monkeypatch.setattr(R, "stream_of", lambda: None)
    torch.use_deterministic_algorithms(on)
    d = R._RoiSparseFn.backward(_fake_ctx((3, 4, 4, 5, 3)), torch.zeros((3, 4, 4, 5, 3)))[0]
    assert d.shape == (10, 4)
    if on:
        assert rec.calls == ["d3d_roi_align_rotated_3d_sparse_backward_deterministic_scratch_bytes",
                             "d3d_roi_align_rotated_3d_sparse_backward_deterministic"]
    else:
        assert rec.calls == ["d3d_roi_align_rotated_3d_sparse_backward"]


def test_sparse_roi_backward_adaptive_sampling_raises(monkeypatch, flag):
    """adaptive sampling (sampling_ratio <= 0) has no fixed-order form: raise, or warn and use the atomic form"""
    from detection_3d_amd import roi_align_rotated_3d as R
    rec = _Recorder()
    monkeypatch.setattr(R, "lib", lambda: rec)
    monkeypatch.setattr(R, "stream_of", lambda: None)
    torch.use_deterministic_algorithms(True)
    with pytest.raises(RuntimeError, match="sampling_ratio <= 0"):
        R._RoiSparseFn.backward(_fake_ctx((3, 4, 4, 5, 3), 0), torch.zeros((3, 4, 4, 5, 3)))
    torch.use_deterministic_algorithms(True, warn_only=True)
    with pytest.warns(UserWarning):
        R._RoiSparseFn.backward(_fake_ctx((3, 4, 4, 5, 3), 0), torch.zeros((3, 4, 4, 5, 3)))
    assert rec.calls == ["d3d_roi_align_rotated_3d_sparse_backward"]


def test_dense_roi_backward_raises_in_deterministic_mode(monkeypatch, flag):
    from detection_3d_amd import roi_align_rotated_3d as R
    torch.use_deterministic_algorithms(True)
    with pytest.raises(RuntimeError, match=r"roi_align_rotated_3d_backward \(dense input\) does not have a deterministic"):
        R.roi_align_rotated_3d_backward(torch.zeros(1, 2, 4, 5, 3), torch.zeros(1, 8), 0.25, 4, 5, 3, 1, 2, 8, 8, 4, 2)


@pytest.mark.parametrize("on", [False, True])
def test_conv_backward_dw_mode_per_call(monkeypatch, flag, on):
    """the conv backward wrappers switch the library's per-thread fixed-order dW on around the call (scratch from
    torch) and off after it, also when the call fails; with the flag off they make no extra call"""
    from detection_3d_amd.sparseconvnet import SCN
    rec = _Recorder()
    monkeypatch.setattr(SCN, "lib", lambda: rec)
    monkeypatch.setattr(SCN, "require_gpu", lambda *t: None)
    monkeypatch.setattr(SCN, "stream_of", lambda: None)
    torch.use_deterministic_algorithms(on)
    m = types.SimpleNamespace(_h=None)
    w = torch.zeros(8, 1, 32, 64)
    SCN.Convolution_backward([8, 8, 8], [4, 4, 4], [2, 2, 2], [2, 2, 2], m, torch.zeros(5, 32), None, torch.zeros(3, 64), w,
                             torch.zeros_like(w), None, want_d_input=False)
    if on:
        assert rec.calls == ["d3d_conv_dw_scratch_bytes", "d3d_conv_dw_thread_mode", "d3d_conv_backward_dt",
                             "d3d_conv_dw_thread_mode"]
    else:
        assert rec.calls == ["d3d_conv_backward_dt"]
    # an error inside the call still switches the mode off
    rec.calls.clear()
    monkeypatch.setattr(SCN, "check", lambda rc: (_ for _ in ()).throw(RuntimeError("boom")))
    with pytest.raises(RuntimeError, match="boom"):
        SCN.Convolution_backward([8, 8, 8], [4, 4, 4], [2, 2, 2], [2, 2, 2], m, torch.zeros(5, 32), None, torch.zeros(3, 64), w,
                                 torch.zeros_like(w), None, want_d_input=False)
    assert rec.calls[-1] == ("d3d_conv_dw_thread_mode" if on else "d3d_conv_backward_dt")


def test_new_symbols_and_argument_checks(lib):
    import ctypes
    from detection_3d_amd import _lib
    for name in ("d3d_roi_align_rotated_3d_sparse_backward_deterministic",
                 "d3d_roi_align_rotated_3d_sparse_backward_deterministic_scratch_bytes",
                 "d3d_conv_dw_thread_mode", "d3d_conv_dw_scratch_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS
    q = lib.d3d_roi_align_rotated_3d_sparse_backward_deterministic_scratch_bytes
    small = q(10, 32, 4, 5, 3, 2, 1000)
    assert small > 10 * 60 * 64 * 4 * 6                    # six record arrays of K x NB x 64
    assert q(20, 32, 4, 5, 3, 2, 1000) > small             # grows with K, C, n_rows
    assert q(10, 64, 4, 5, 3, 2, 1000) > small
    assert q(10, 32, 4, 5, 3, 2, 100000) > small
    assert q(0, 32, 4, 5, 3, 2, 1000) > 0                  # K = 0: valid
    for bad in ((10, 32, 4, 5, 3, 0, 1000), (10, 0, 4, 5, 3, 2, 1000), (-1, 32, 4, 5, 3, 2, 1000),
                (10, 32, 0, 5, 3, 2, 1000), (10, 32, 4, 5, 3, 2, -1), (100000, 256, 7, 7, 3, 4, 1000)):
        assert q(*bad) == 0, bad                          # out of range (adaptive sampling, too many records)
    f = lib.d3d_roi_align_rotated_3d_sparse_backward_deterministic
    ints = _lib.ints
    # argument errors come before any device work (D3D_ERR_ARG = -1)
    assert f(None, ints([8, 8, 8]), None, 32, ints([8, 8, 8]), None, 1, 0.25, 4, 5, 3, 2, None, 10, None, 0, None) == -1
    # dW: scratch query and the per-thread mode
    n = 27 * 64 * 64 * 4
    assert lib.d3d_conv_dw_scratch_bytes(27, 64, 64) == 32 * n           # small layers: all 32 partials
    assert lib.d3d_conv_dw_scratch_bytes(27, 256, 256) == 9 * 27 * 256 * 256 * 4   # large ones: within 64 MB
    assert lib.d3d_conv_dw_scratch_bytes(0, 64, 64) == 0
    assert lib.d3d_conv_dw_thread_mode(-1, None, 0) == 0
    assert lib.d3d_conv_dw_thread_mode(1, None, 0) == -1                  # fixed order needs a buffer
    # the mode is per thread: set it in a thread of its own (a placeholder address that no kernel ever sees), so that
    # a failing assert cannot leave it on for this one
    import threading
    seen = []

    def other():
        try:
            seen.append(lib.d3d_conv_dw_thread_mode(1, ctypes.c_void_p(4096), 4096))
            seen.append(lib.d3d_conv_dw_thread_mode(-1, None, 0))
        finally:
            seen.append(lib.d3d_conv_dw_thread_mode(0, None, 0))
    th = threading.Thread(target=other)
    th.start()
    th.join()
    assert seen == [0, 1, 1]
    assert lib.d3d_conv_dw_thread_mode(-1, None, 0) == 0                  # this thread: untouched


def _train_ddp():
    spec = importlib.util.spec_from_file_location("train_ddp_under_test", os.path.join(ROOT, "scripts", "train_ddp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_ddp_deterministic_option(flag):
    mod = _train_ddp()
    a = mod.parse_args(["--config", "4c_Fpn432", "--steps", "4"])
    assert a.deterministic is False and a.seed == 0 and a.steps == 4
    b = mod.parse_args(["--deterministic", "--seed", "7"])
    assert b.deterministic is True and b.seed == 7
    with pytest.raises(SystemExit):
        mod.parse_args(["--seed", "x"])
    torch.use_deterministic_algorithms(False)
    mod.seed_everything(a)                                 # default: the flag stays off, weights seeded with 0
    assert not torch.are_deterministic_algorithms_enabled()
    x = torch.rand(4)
    torch.manual_seed(0)
    assert torch.equal(x, torch.rand(4))
    fill = torch.utils.deterministic.fill_uninitialized_memory
    mod.seed_everything(b)
    assert torch.utils.deterministic.fill_uninitialized_memory == fill      # torch's own setting is left alone
    assert torch.are_deterministic_algorithms_enabled()
    y = torch.rand(4)
    torch.manual_seed(7)
    assert torch.equal(y, torch.rand(4))
