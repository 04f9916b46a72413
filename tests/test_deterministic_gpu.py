"""torch.use_deterministic_algorithms(True) on the MI355X: the fixed-order RoIAlignRotated3D backward
(d3d_roi_align_rotated_3d_sparse_backward_deterministic), the fixed-order dWeight of the sparse convolutions selected
per call, and whole training steps that give the same bits in every run."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


class _flag:
    """torch.use_deterministic_algorithms(on) for a block; restores the previous setting"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.was = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(self.on)

    def __exit__(self, *exc):
        torch.use_deterministic_algorithms(self.was)
        return False


def _sparse_map(dev, sizes, C, seed):
    """one sparse map of len(sizes) examples: example b holds sizes[b] random sites"""
    from detection_3d_amd import sparseconvnet as scn
    rng = np.random.RandomState(seed)
    size = (48, 40, 12)
    coords = []
    for b, n in enumerate(sizes):
        c = np.unique(np.stack([rng.randint(0, s, n) for s in size], 1), axis=0)
        coords.append(np.concatenate([c, np.full((c.shape[0], 1), b)], 1))
    coords = np.concatenate(coords).astype(np.int64)
    feats = rng.randn(coords.shape[0], C).astype(np.float32)
    t = scn.InputLayer(3, size, mode=4)([torch.from_numpy(coords), torch.from_numpy(feats).to(dev)])
    loc = t.get_spatial_locations().cpu().numpy()
    return t, loc, (loc[:, :3].max(0) + 1).tolist()


def _random_rois(rng, K, crop, n_examples):
    rois = np.zeros((K, 8), np.float32)
    rois[:, 0] = np.arange(K) % n_examples
    rois[:, 1] = rng.rand(K) * crop[1] * 4
    rois[:, 2] = rng.rand(K) * crop[0] * 4
    rois[:, 3] = rng.rand(K) * crop[2] * 4
    rois[:, 4:7] = 4 + rng.rand(K, 3) * np.array([60, 40, 20])
    rois[:, 7] = rng.rand(K) * 180
    return rois


def _sparse_grad(t, rois, grad, crop, deterministic, pooled=(4, 5, 3), scale=0.25):
    from detection_3d_amd import sparseconvnet as scn
    from detection_3d_amd.roi_align_rotated_3d import roi_align_rotated_3d_sparse
    f = t.features.detach().clone().requires_grad_(True)
    tt = scn.SparseConvNetTensor(f, t.metadata, t.spatial_size)
    with _flag(deterministic):
        out = roi_align_rotated_3d_sparse(tt, rois, scale, *pooled, 2, crop=crop)
        out.backward(grad)
    return f.grad


def _check_sparse(dev, t, loc, crop, rois_np, grad_np, n_examples, expect_nonzero=True):
    C = t.features.shape[1]
    rois = torch.from_numpy(rois_np).to(dev)
    g = torch.from_numpy(grad_np).to(dev)
    runs = [_sparse_grad(t, rois, g, crop, True) for _ in range(3)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])          # the same bits in every call
    got = runs[0].cpu().numpy()
    atomic = _sparse_grad(t, rois, g, crop, False).cpu().numpy()
    dense = oracle.roi_align_rotated_3d_backward(grad_np, rois_np, 0.25, 4, 5, 3, 2,
                                                 (n_examples, C, crop[0], crop[1], crop[2]))
    want = dense[loc[:, 3], :, loc[:, 0], loc[:, 1], loc[:, 2]]
    if not expect_nonzero:
        assert not np.abs(want).any() and not np.abs(got).any() and not np.abs(atomic).any()
        return got
    assert np.abs(want).max() > 0
    assert rel(got, want) < 1e-4                       # the oracle, as test_roi_align_sparse_backward
    assert rel(got, atomic) <= 1e-5                    # the atomic kernel: only the summation order differs
    return got


@pytest.mark.parametrize("sizes", [(2500,), (2500, 1800)])
def test_sparse_roi_backward_deterministic(dev, sizes):
    t, loc, crop = _sparse_map(dev, sizes, 32, 2 + len(sizes))
    rng = np.random.RandomState(7)
    rois = _random_rois(rng, 40, crop, len(sizes))
    g = rng.randn(40, 32, 4, 5, 3).astype(np.float32)
    got = _check_sparse(dev, t, loc, crop, rois, g, len(sizes))
    if len(sizes) == 2:
        assert np.abs(got[loc[:, 3] == 1]).max() > 0


def test_sparse_roi_backward_deterministic_channels(dev):
    """C = 300: more than one pass of 256 channels over a chunk, and a channel count that is not a multiple of 64"""
    t, loc, crop = _sparse_map(dev, (3000,), 300, 11)
    rng = np.random.RandomState(8)
    rois = _random_rois(rng, 24, crop, 1)
    _check_sparse(dev, t, loc, crop, rois, rng.randn(24, 300, 4, 5, 3).astype(np.float32), 1)


def test_sparse_roi_backward_deterministic_empty_and_outside(dev):
    t, loc, crop = _sparse_map(dev, (2000,), 32, 5)
    rng = np.random.RandomState(9)
    # K = 0
    got = _sparse_grad(t, torch.zeros((0, 8), device=dev), torch.zeros((0, 32, 4, 5, 3), device=dev), crop, True)
    assert got.shape == t.features.shape and not got.abs().any()
    # RoIs wholly outside the grid: zeros
    rois = _random_rois(rng, 12, crop, 1)
    rois[:, 1:3] += 5000
    _check_sparse(dev, t, loc, crop, rois, rng.randn(12, 32, 4, 5, 3).astype(np.float32), 1, expect_nonzero=False)


def test_sparse_roi_backward_deterministic_hot_cells(dev):
    """hundreds of identical RoIs: every cell under them has hundreds of records, far past the chunk length of 64.
    The exact gradient is the one RoI's backward of the fp64 sum of the top gradients."""
    t, loc, crop = _sparse_map(dev, (2500,), 32, 6)
    rng = np.random.RandomState(10)
    K = 400
    rois = np.repeat(_random_rois(rng, 1, crop, 1), K, 0)
    rois[0, 4:7] = [30, 25, 12]
    rois[:] = rois[0]
    g = (0.5 + 0.5 * rng.rand(K, 32, 4, 5, 3)).astype(np.float32)    # one sign: no cancellation in the reference
    runs = [_sparse_grad(t, torch.from_numpy(rois).to(dev), torch.from_numpy(g).to(dev), crop, True) for _ in range(3)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    g64 = g.astype(np.float64).sum(0, keepdims=True)
    scale = float(np.abs(g64).max())
    dense = oracle.roi_align_rotated_3d_backward((g64 / scale).astype(np.float32), rois[:1], 0.25, 4, 5, 3, 2,
                                                 (1, 32, crop[0], crop[1], crop[2])).astype(np.float64) * scale
    want = dense[loc[:, 3], :, loc[:, 0], loc[:, 1], loc[:, 2]]
    got = runs[0].cpu().numpy()
    assert np.abs(want).max() > 0
    assert rel(got, want) < 1e-5


def test_sparse_roi_backward_deterministic_errors(dev):
    """absent grid: D3D_ERR_STATE as in the atomic form; scratch too small: an argument error"""
    from detection_3d_amd import _lib
    t, loc, crop = _sparse_map(dev, (500,), 32, 12)
    lib = _lib.lib()
    n = t.features.shape[0]
    g = torch.zeros((2, 32, 4, 5, 3), device=dev)
    r = torch.zeros((2, 8), device=dev)
    d = torch.zeros((n, 32), device=dev)
    nbytes = lib.d3d_roi_align_rotated_3d_sparse_backward_deterministic_scratch_bytes(2, 32, 4, 5, 3, 2, n)
    s = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    args = lambda size, nb: (t.metadata._h, _lib.ints(size), _lib.ptr(g), 32, _lib.ints(crop), _lib.ptr(r), 2, 0.25,
                             4, 5, 3, 2, _lib.ptr(d), n, _lib.ptr(s), nb, _lib.stream_of())
    assert lib.d3d_roi_align_rotated_3d_sparse_backward_deterministic(*args([7, 7, 7], nbytes)) == -4
    assert lib.d3d_roi_align_rotated_3d_sparse_backward_deterministic(*args(list(t.spatial_size.tolist()),
                                                                            nbytes - 1024)) == -1
    assert lib.d3d_roi_align_rotated_3d_sparse_backward_deterministic(*args(list(t.spatial_size.tolist()),
                                                                            nbytes)) == 0


def test_dense_roi_backward_raises_in_deterministic_mode(dev):
    """the dense-input backward keeps its fp32 atomics: in deterministic mode it raises as torch's ops do, and with
    warn_only=True it warns and still matches the oracle"""
    from detection_3d_amd.roi_align_rotated_3d import roi_align_rotated_3d_forward
    rng = np.random.RandomState(4)
    x = torch.from_numpy(rng.randn(1, 8, 16, 16, 6).astype(np.float32)).to(dev).requires_grad_(True)
    rois = torch.from_numpy(_random_rois(rng, 6, (16, 16, 6), 1)).to(dev)
    g = torch.from_numpy(rng.randn(6, 8, 4, 5, 3).astype(np.float32)).to(dev)
    with _flag(True):
        out = roi_align_rotated_3d_forward(x, rois, 0.25, 4, 5, 3, 2)
        with pytest.raises(RuntimeError, match="roi_align_rotated_3d_backward.*deterministic"):
            out.backward(g)
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        out = roi_align_rotated_3d_forward(x, rois, 0.25, 4, 5, 3, 2)
        with pytest.warns(UserWarning, match="deterministic"):
            out.backward(g)
    finally:
        torch.use_deterministic_algorithms(was)
    want = oracle.roi_align_rotated_3d_backward(g.cpu().numpy(), rois.cpu().numpy(), 0.25, 4, 5, 3, 2, (1, 8, 16, 16, 6))
    assert rel(x.grad.cpu().numpy(), want) < 1e-4


# ---------------------------------------------------------------------------------------------------------------------
def _conv_setup(dev, cin, cout, n_points):
    from detection_3d_amd import sparseconvnet as scn
    from tests.helpers import small_scene
    size = (128, 128, 32)
    rng = np.random.RandomState(cin + cout)
    _, coords, _ = small_scene(5, n_points, (2.5, 2.0, 0.6), size)
    feats = torch.from_numpy(rng.randn(coords.shape[0], cin).astype(np.float32)).to(dev)
    torch.manual_seed(3)
    sub = scn.SubmanifoldConvolution(3, cin, cout, 3, False).to(dev)
    down = scn.Convolution(3, cin, cout, [2, 2, 2], [2, 2, 2], False).to(dev)
    up = scn.Deconvolution(3, cout, cin, [2, 2, 2], [2, 2, 2], False).to(dev)

    def grads(deterministic):
        for m in (sub, down, up):
            m.weight.grad = None
        with _flag(deterministic):
            t = scn.InputLayer(3, size, mode=4)([torch.from_numpy(coords), feats])
            y = sub(t).features
            y.backward(torch.ones_like(y) * 0.5 + y.detach() * 0.1)
            u = up(down(t)).features
            u.backward(torch.ones_like(u) * 0.25 + u.detach() * 0.1)
        return [m.weight.grad.clone() for m in (sub, down, up)]
    return grads


@pytest.mark.parametrize("cin,cout,n_points", [(32, 32, 60000), (64, 128, 3000), (256, 256, 300)])
def test_conv_dw_follows_torch_flag(dev, cin, cout, n_points):
    from detection_3d_amd._lib import lib
    grads = _conv_setup(dev, cin, cout, n_points)
    before = lib().d3d_conv_dw_deterministic(-1)
    atomic = grads(False)
    a, b = grads(True), grads(True)
    assert lib().d3d_conv_dw_deterministic(-1) == before          # the process-wide switch is not touched
    assert lib().d3d_conv_dw_thread_mode(-1, None, 0) == 0         # nor left on for the thread
    for x, y, z in zip(a, b, atomic):
        assert torch.isfinite(x).all() and float(x.abs().max()) > 0
        assert torch.equal(x, y)
        assert float((x - z).abs().max()) <= 1e-5 * float(z.abs().max())
    # the process-wide switch gives the same bits as the per-call mode (same partials: same plan, same budget)
    was = lib().d3d_conv_dw_deterministic(1)
    try:
        c = grads(False)
    finally:
        lib().d3d_conv_dw_deterministic(was)
    for x, y in zip(a, c):
        assert torch.equal(x, y)


def test_conv_dw_deterministic_small_arena(dev, monkeypatch):
    """metadata whose feature lane (a third of 96 MB) cannot hold 32 partials of a 256 x 256 layer (7 MB each): the
    fixed-order dW completes with fewer partials, under the torch flag (partials in a torch buffer) and under the
    process-wide switch (partials in the feature lane), with the same bits as with a large arena"""
    from detection_3d_amd import _lib
    from detection_3d_amd.sparseconvnet import SCN
    n = 27 * 256 * 256 * 4
    assert 32 * n > (96 << 20) // 3
    assert _lib.lib().d3d_conv_dw_scratch_bytes(27, 256, 256) <= (64 << 20) < 32 * n
    grads = _conv_setup(dev, 256, 256, 20000)
    ref = grads(True)
    monkeypatch.setattr(SCN, "arena_bytes_for", lambda n_points: 96 << 20)
    a, b = grads(True), grads(True)
    was = _lib.lib().d3d_conv_dw_deterministic(1)
    try:
        c = grads(False)
    finally:
        _lib.lib().d3d_conv_dw_deterministic(was)
    for x, y, z, w in zip(a, b, ref, c):
        assert torch.equal(x, y) and torch.equal(x, z) and torch.equal(x, w)


def test_backbone_takes_the_side_stream_pass_in_deterministic_mode(dev, monkeypatch):
    """Under the flag, with torch's NaN fill of new tensors on, a GPU input goes through the side-stream pass
    (FPN_Net._forward_async_geometry), whose input layer orders its side-stream write behind the fill: every map is
    finite and equal to the bit to the one-stream pass's under the same flag."""
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.detector import build_detection_model
    from detection_3d_amd.sparseconvnet import fpn_net
    from detection_3d_amd.synthetic import make_scene
    from detection_3d_amd.voxelize import voxelize
    assert torch.utils.deterministic.fill_uninitialized_memory
    cfg = get_cfg("4c_Fpn432")
    torch.manual_seed(0)
    model = build_detection_model(cfg).to(dev).eval()
    calls = []
    real = fpn_net.FPN_Net._forward_async_geometry
    monkeypatch.setattr(fpn_net.FPN_Net, "_forward_async_geometry", lambda self, net0: calls.append(1) or real(self, net0))
    c, f = voxelize(torch.from_numpy(make_scene(8, 60000)).to(dev), cfg.SPARSE3D.VOXEL_SCALE,
                    cfg.SPARSE3D.VOXEL_FULL_SCALE)
    maps = {}
    with torch.no_grad(), _flag(True):
        for side in (True, False):
            monkeypatch.setattr(fpn_net, "SIDE_STREAMS", side)
            rpn, roi = model.backbone([c, f])
            torch.cuda.synchronize()
            maps[side] = [m.features.clone() for m in rpn + roi]
    assert len(calls) == 1
    assert len(maps[True]) == len(maps[False]) > 0
    for a, b in zip(maps[True], maps[False]):
        assert a.shape == b.shape and a.shape[0] > 0 and torch.isfinite(a).all() and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
def _scene(dev, seed, n_points, extent):
    from detection_3d_amd.synthetic import make_scene, make_targets
    pcl = torch.from_numpy(make_scene(seed, n_points, extent)).to(dev)
    b, l = make_targets(seed, extent)
    return pcl, {"bbox3d": torch.from_numpy(b).to(dev), "labels": torch.from_numpy(l).to(dev)}


def _step_case(dev, name, scenes):
    """-> (model, initial state, batch): the model in training mode and a collated batch of the given scenes"""
    from detection_3d_amd import engine, training as T
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.detector import build_detection_model
    cfg = get_cfg(name)
    torch.manual_seed(0)
    model = build_detection_model(cfg).to(dev).train()
    T.freeze_unused(model)
    items = [_scene(dev, *s) for s in scenes]
    points, tgs = engine.collate(items, cfg)
    if len(items) == 1:
        points, tgs = [points[0][:, :3].contiguous(), points[1]], tgs[0]
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return cfg, model, state, points, tgs


def _fwd_bwd(model, state, points, tgs):
    model.load_state_dict(state)
    model.zero_grad(set_to_none=True)
    torch.manual_seed(1234)                               # the samplers' permutations
    losses = model(points, tgs)
    sum(losses.values()).backward()
    return ({k: v.detach().clone() for k, v in losses.items()},
            {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None})


def _two_sgd_steps(cfg, model, state, points, tgs):
    from detection_3d_amd import training as T
    model.load_state_dict(state)
    opt = T.make_optimizer(cfg, model)
    for it in range(2):
        torch.manual_seed(99 + it)
        opt.zero_grad(set_to_none=True)
        losses = model(points, tgs)
        sum(losses.values()).backward()
        opt.step()
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


STEP_CASES = {
    "4c_b1": ("4c_Fpn432", [(5, 60000, (25.0, 19.0, 2.7))]),
    "4c_b2": ("4c_Fpn432", [(5, 60000, (25.0, 19.0, 2.7)), (6, 25000, (12.0, 9.0, 2.7))]),
    "3G6c_b1": ("3G6c_Fpn4321", [(7, 60000, (25.0, 19.0, 2.7))]),
    "6c_500k": ("6c_Fpn4321", [(0, 500000, (25.0, 19.0, 2.7))]),
}


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_training_step_bit_reproducible(dev, case):
    """Under torch.use_deterministic_algorithms(True): two forward + backward passes from the same weights and seed give
    equal losses and equal gradients of every parameter, and two SGD steps give equal weights.  The gradients also
    agree with the default (atomic) mode within the bound of test_duplicated_batch_equals_single_example.
    torch's defaults hold: in this mode it fills every new tensor with NaN, so a read of memory no kernel wrote, or a
    write that races with the fill, shows up here."""
    assert torch.utils.deterministic.fill_uninitialized_memory
    name, scenes = STEP_CASES[case]
    cfg, model, state, points, tgs = _step_case(dev, name, scenes)
    with _flag(True):
        l1, g1 = _fwd_bwd(model, state, points, tgs)
        l2, g2 = _fwd_bwd(model, state, points, tgs)
    assert set(l1) == set(l2) and len(l1) >= 4
    for k in l1:
        assert torch.equal(l1[k], l2[k]), (k, float(l1[k]), float(l2[k]))
    assert set(g1) == set(g2) and len(g1) > 50
    diff = [k for k in g1 if not torch.equal(g1[k], g2[k])]
    assert not diff, diff[:10]
    l0, g0 = _fwd_bwd(model, state, points, tgs)           # flag off
    for k in l1:
        assert abs(float(l0[k]) - float(l1[k])) <= 1e-5 * max(abs(float(l0[k])), 1e-12), k
    flat0 = torch.cat([g0[k].reshape(-1) for k in sorted(g1)])
    flat1 = torch.cat([g1[k].reshape(-1) for k in sorted(g1)])
    assert (flat0 - flat1).norm().item() <= 1e-4 * flat0.norm().item()
    if case == "6c_500k":
        return                                             # (the SGD steps: on the smaller cases)
    with _flag(True):
        w1 = _two_sgd_steps(cfg, model, state, points, tgs)
        w2 = _two_sgd_steps(cfg, model, state, points, tgs)
    diff = [k for k in w1 if not torch.equal(w1[k], w2[k])]
    assert not diff, diff[:10]
