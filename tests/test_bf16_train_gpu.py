"""Training in bf16 storage: the backbone's rows and their gradients are bf16, accumulation, parameters, their gradients
and the BatchNorm statistics fp32.

Oracle: the fp32 CPU oracle on the SAME bf16-rounded inputs, weights and upstream gradients (as test_bf16_gpu.py).
Products of bf16 values are exact in fp32, so dWeight (fp32 out) differs from the oracle only by summation order: the
fp32 tests' 2e-4 of the largest magnitude.  dInput and BatchNorm outputs are rounded once to bf16: 1e-2."""
import numpy as np
import pytest
import torch

import oracle
from tests.helpers import nbr_to_rules, small_scene

pytestmark = pytest.mark.gpu
TOL = 1e-2


@pytest.fixture(autouse=True)
def _bf16_backward_built():
    """fails in Python, before anything is launched, on a library without the bf16 backward entry points"""
    from detection_3d_amd import _lib
    assert hasattr(_lib.lib(), "d3d_conv_backward_dt")


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def bf16_round(x):
    return torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).float().numpy()


def _bf16_grad(rng, shape, dev):
    """a random upstream gradient in bf16 and its exact fp32 values"""
    g = torch.from_numpy(rng.randn(*shape).astype(np.float32)).to(torch.bfloat16)
    return g.to(dev), g.float().numpy()


def _input_bf16(dev, cin, seed, n_points=6000, size=(64, 64, 16), requires_grad=True):
    """sparse tensor with bf16 rows (zero padded to the stored width) -> (tensor, exact fp32 rows [n, cin], sites)"""
    from detection_3d_amd import sparseconvnet as scn
    from detection_3d_amd.sparseconvnet import SCN
    rng = np.random.RandomState(seed + cin)
    _, coords, _ = small_scene(seed, n_points, (1.2, 1.0, 0.3), size)
    feats = rng.randn(coords.shape[0], cin).astype(np.float32)
    t = scn.InputLayer(3, size, mode=4)([torch.from_numpy(coords), torch.from_numpy(feats).to(dev)])
    width = SCN.stored_planes(cin, torch.bfloat16)
    f = torch.nn.functional.pad(t.features, (0, width - cin)).to(torch.bfloat16)
    t.features = f.requires_grad_(requires_grad)
    _, loc = oracle.input_sites(coords)
    return t, f.detach().float().cpu().numpy()[:, :cin], loc


@pytest.fixture(params=[1, 2, 4])
def row_blocks(request):
    """dInput runs through k_conv_bf16: each of its weight-sharing widths, forced on for every launch size"""
    from detection_3d_amd._lib import check, lib
    check(lib().d3d_conv_bf16_tuning(request.param, 0))
    yield request.param
    check(lib().d3d_conv_bf16_tuning(2, -1))


def _w(m, k, cin, cout):
    return bf16_round(m.weight.detach().cpu().numpy().reshape(k, cin, cout))


@pytest.mark.parametrize("cin,cout", [(32, 32), (32, 64), (64, 64), (64, 128), (128, 128), (256, 128), (128, 256),
                                      (256, 256)])
def test_conv_backward_bf16(dev, cin, cout, row_blocks):
    from detection_3d_amd import sparseconvnet as scn
    t, x, loc = _input_bf16(dev, cin, 4)
    rng = np.random.RandomState(cin + 3 * cout)
    torch.manual_seed(1)
    # submanifold 3^3
    conv = scn.SubmanifoldConvolution(3, cin, cout, 3, False).to(dev)
    y = conv(t).features
    assert y.dtype == torch.bfloat16
    g, gn = _bf16_grad(rng, y.shape, dev)
    y.backward(g)
    assert t.features.grad.dtype == torch.bfloat16 and conv.weight.grad.dtype == torch.float32
    nbr, _ = oracle.subm_nbr(loc, [3, 3, 3])
    d_x, d_w = oracle.rule_conv_backward(x, _w(conv, 27, cin, cout), nbr_to_rules(nbr), gn)
    assert rel_err(conv.weight.grad.cpu().numpy().reshape(27, cin, cout), d_w) < 2e-4
    assert rel_err(t.features.grad.float().cpu().numpy(), d_x) < TOL
    # strided conv 2/2 (dInput through the deconvolution plan)
    t.features.grad = None
    down = scn.Convolution(3, cin, cout, [2, 2, 2], [2, 2, 2], False).to(dev)
    d = down(t)
    g, gn = _bf16_grad(rng, d.features.shape, dev)
    d.features.backward(g)
    lo, ru = oracle.conv_rules(loc, [2, 2, 2], [2, 2, 2], [32, 32, 8])
    d_x, d_wd = oracle.rule_conv_backward(x, _w(down, 8, cin, cout), ru, gn)
    assert rel_err(down.weight.grad.cpu().numpy().reshape(8, cin, cout), d_wd) < 2e-4
    assert rel_err(t.features.grad.float().cpu().numpy(), d_x) < TOL
    # its deconvolution cout -> cin (dInput through the convolution plan)
    mid = d.features.detach().requires_grad_(True)
    up = scn.Deconvolution(3, cout, cin, [2, 2, 2], [2, 2, 2], False).to(dev)
    u = up(scn.SparseConvNetTensor(mid, d.metadata, d.spatial_size)).features
    g, gn = _bf16_grad(rng, u.shape, dev)
    u.backward(g)
    d_mid, d_wu = oracle.rule_conv_backward(mid.detach().float().cpu().numpy(), _w(up, 8, cout, cin), ru, gn,
                                            deconv=True)
    assert rel_err(up.weight.grad.cpu().numpy().reshape(8, cout, cin), d_wu) < 2e-4
    assert rel_err(mid.grad.float().cpu().numpy(), d_mid) < TOL


def test_first_layer_weight_grad_bf16(dev):
    """Cin = 9 stored as 16 bf16 channels: dWeight only, written for the 9 real channels ([27, 9, 32])"""
    from detection_3d_amd import sparseconvnet as scn
    t, x, loc = _input_bf16(dev, 9, 2, requires_grad=False)
    assert t.features.shape[1] == 16
    conv = scn.SubmanifoldConvolution(3, 9, 32, 3, False).to(dev)
    y = conv(t).features
    g, gn = _bf16_grad(np.random.RandomState(2), y.shape, dev)
    y.backward(g)
    nbr, _ = oracle.subm_nbr(loc, [3, 3, 3])
    _, d_w = oracle.rule_conv_backward(x, _w(conv, 27, 9, 32), nbr_to_rules(nbr), gn)
    assert conv.weight.grad.shape == (27, 1, 9, 32)
    assert rel_err(conv.weight.grad.cpu().numpy().reshape(27, 9, 32), d_w) < 2e-4


@pytest.mark.parametrize("cin,cout,n_points", [(32, 32, 60000), (64, 128, 20000), (256, 256, 3000)])
def test_conv_backward_bf16_deterministic_dw(dev, cin, cout, n_points):
    """the fixed-order dW form (d3d_conv_dw_deterministic): the same bits in every call, the atomic form up to the
    summation order (1e-5 of the tensor's magnitude)"""
    from detection_3d_amd import sparseconvnet as scn
    from detection_3d_amd._lib import lib
    size = (128, 128, 32)
    rng = np.random.RandomState(cin + cout)
    _, coords, _ = small_scene(5, n_points, (2.5, 2.0, 0.6), size)
    feats = torch.from_numpy(rng.randn(coords.shape[0], cin).astype(np.float32)).to(dev)
    torch.manual_seed(3)
    sub = scn.SubmanifoldConvolution(3, cin, cout, 3, False).to(dev)
    down = scn.Convolution(3, cin, cout, [2, 2, 2], [2, 2, 2], False).to(dev)
    up = scn.Deconvolution(3, cout, cin, [2, 2, 2], [2, 2, 2], False).to(dev)

    def grads():
        for m in (sub, down, up):
            m.weight.grad = None
        t = scn.InputLayer(3, size, mode=4)([torch.from_numpy(coords), feats])
        t.features = t.features.to(torch.bfloat16)
        y = sub(t).features
        y.backward((torch.ones_like(y) * 0.5 + y.detach() * 0.1).to(torch.bfloat16))
        u = up(down(t)).features
        u.backward((torch.ones_like(u) * 0.25 + u.detach() * 0.1).to(torch.bfloat16))
        return [m.weight.grad.clone() for m in (sub, down, up)]

    atomic = grads()
    was = lib().d3d_conv_dw_deterministic(1)
    try:
        a = grads()
        b = grads()
    finally:
        lib().d3d_conv_dw_deterministic(was)
    for x, y, z in zip(a, b, atomic):
        assert torch.isfinite(x).all() and float(x.abs().max()) > 0
        assert torch.equal(x, y)
        assert float((x - z).abs().max()) <= 1e-5 * float(z.abs().max())


@pytest.mark.parametrize("C", [32, 128, 256])
@pytest.mark.parametrize("leak", [0.0, 0.333])
def test_batchnorm_train_bf16(dev, C, leak):
    # every launch form against exact fp64 results, with per-element bounds: tests/test_bn_forms_gpu.py
    from detection_3d_amd import sparseconvnet as scn
    from detection_3d_amd.sparseconvnet import SCN
    rng = np.random.RandomState(C + int(leak * 1000))
    xt = torch.from_numpy((rng.randn(4000, C) * 2 + 0.5).astype(np.float32)).to(torch.bfloat16).to(dev)
    x = xt.float().cpu().numpy()
    bn = scn.BatchNormLeakyReLU(C, momentum=0.95, leakiness=leak).to(dev).train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-0.2, 0.2)
        bn.running_var.uniform_(0.8, 1.2)
    gamma, beta = bn.weight.detach().cpu().numpy(), bn.bias.detach().cpu().numpy()
    rm0, rv0 = bn.running_mean.cpu().numpy().copy(), bn.running_var.cpu().numpy().copy()
    want, sm, si, rm, rv = oracle.bn_forward(x, rm0, rv0, gamma, beta, 1e-4, 0.95, True, leak)
    # the entry point itself: fp32 save_mean / save_invstd and running statistics
    out = xt.new_empty(0)
    save_mean, save_invstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    r_mean, r_var = bn.running_mean.clone(), bn.running_var.clone()
    with torch.no_grad():
        SCN.BatchNormalization_updateOutput(xt, out, save_mean, save_invstd, r_mean, r_var, bn.weight, bn.bias, 1e-4,
                                            0.95, True, leak)
    assert out.dtype == torch.bfloat16
    assert rel_err(out.float().cpu().numpy(), want) < TOL
    assert rel_err(save_mean.cpu().numpy(), sm) < 1e-5 and rel_err(save_invstd.cpu().numpy(), si) < 1e-5
    assert rel_err(r_mean.cpu().numpy(), rm) < 1e-5 and rel_err(r_var.cpu().numpy(), rv) < 1e-5
    # the module in training mode: autograd through _BatchNormFn
    xg = xt.clone().requires_grad_(True)
    y = bn(scn.SparseConvNetTensor(xg, None, torch.tensor([8, 8, 8]))).features
    assert y.dtype == torch.bfloat16 and y.grad_fn is not None
    assert rel_err(bn.running_mean.cpu().numpy(), rm) < 1e-5 and rel_err(bn.running_var.cpu().numpy(), rv) < 1e-5
    g, gn = _bf16_grad(rng, y.shape, dev)
    y.backward(g)
    yk = y.detach().float().cpu().numpy()                   # the kernel's own y decides the leaky mask
    d_in, d_w, d_b = oracle.bn_backward(x, yk, gn, sm, si, gamma, leak)
    assert xg.grad.dtype == torch.bfloat16
    assert rel_err(xg.grad.float().cpu().numpy(), d_in) < TOL
    assert rel_err(bn.weight.grad.cpu().numpy(), d_w) < 5e-4
    assert rel_err(bn.bias.grad.cpu().numpy(), d_b) < 5e-4


def test_backward_wrappers_refuse_other_dtypes(dev):
    """float16 rows, or rows and gradient of different types, raise D3DError before anything is launched"""
    from detection_3d_amd._lib import D3DError
    from detection_3d_amd.sparseconvnet import SCN
    w = torch.zeros(27, 1, 32, 32, device=dev)
    dw = torch.zeros_like(w)
    f32 = torch.zeros(10, 32, device=dev)
    for feats, d_out in ((f32.half(), f32.half()), (f32.to(torch.bfloat16), f32), (f32, f32.to(torch.bfloat16))):
        with pytest.raises(D3DError):
            SCN.SubmanifoldConvolution_backward([8, 8, 8], [3, 3, 3], None, feats, feats.new_empty(0), d_out, w, dw,
                                                None)
        with pytest.raises(D3DError):
            SCN.Convolution_backward([8, 8, 8], [4, 4, 4], [2, 2, 2], [2, 2, 2], None, feats, feats.new_empty(0), d_out,
                                     w[:8], dw[:8], None)
        with pytest.raises(D3DError):
            SCN.Deconvolution_backward([4, 4, 4], [8, 8, 8], [2, 2, 2], [2, 2, 2], None, feats, feats.new_empty(0),
                                       d_out, w[:8], dw[:8], None)
        with pytest.raises(D3DError):
            SCN.BatchNormalization_backward(feats, feats.new_empty(0), feats, d_out, w[0, 0, 0], w[0, 0, 0], None, None,
                                            None, None, None, None, 0.0)


# ---------------------------------------------------------------------------------------------------------------------
def _model(dev, name):
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.detector import build_detection_model
    cfg = get_cfg(name)
    torch.manual_seed(0)
    return cfg, build_detection_model(cfg).to(dev).train()


def _scene(dev, seed, n_points, extent=(25.0, 19.0, 2.7)):
    from detection_3d_amd.synthetic import make_scene, make_targets
    pcl = torch.from_numpy(make_scene(seed, n_points, extent)).to(dev)
    b, l = make_targets(seed, extent)
    return pcl, {"bbox3d": torch.from_numpy(b).to(dev), "labels": torch.from_numpy(l).to(dev)}


def _backbone_grads(model, coords, feats, proj):
    model.zero_grad(set_to_none=True)
    rpn_maps, _ = model.backbone([coords, feats])
    loss = sum((m.features * p).sum() for m, p in zip(rpn_maps, proj) if m is not None)
    loss.backward()
    return {k: p.grad.detach().clone() for k, p in model.backbone.named_parameters() if p.grad is not None}


def _cos(x, y):
    x, y = x.reshape(-1).double(), y.reshape(-1).double()
    return float(x @ y / (x.norm() * y.norm()))


def test_backbone_grads_bf16_vs_fp32(dev):
    """Same weights and scene (4c, ~200 k points), loss = a fixed random projection of the maps the RPN consumes: the
    same parameters receive a gradient, and the bf16 gradients stay within a fixed multiple of how far the fp32
    gradients themselves move when nothing but the input rows are rounded to bf16 once (`ref`).

    Measured on MI355X (this scene): all gradients together cos 0.9798 for bf16 against 0.9947 for `ref`; per
    parameter min 0.9449 (m_downs.2.0.0.bias, a BatchNorm bias in front of a strided convolution) against 0.9877.  The
    issue's first guess of >= 0.999 / >= 0.99 does not hold for any storage with 8 mantissa bits here: at
    initialisation with this loss the down path amplifies perturbations -- one rounding of the 9 input channels costs
    cos 0.9947 overall and 0.98-0.99 on every m_downs layer, and bf16 rounds after every layer of ~30 forward and ~30
    backward ones.  Parameters near the loss (convs_pro2d, m_mergeds, m_ups.2-3, m_shortcuts.4-5) agree to 0.9998.
    Bounds: 1 - cos <= 8 (1 - cos_ref) (measured ratio <= 4.5 on every down-path parameter) and cos >= 0.95 overall;
    per parameter cos >= 0.9, and either cos >= 0.999 (the parameters near the loss, which one input rounding does not
    reach) or the same 8x bound.
    Parameters whose fp32 gradient norm is below 1e-3 of the largest are not compared one by one: at the coarsest
    levels BatchNorm sees one or two sites, and those gradients are rounding noise."""
    from detection_3d_amd.voxelize import voxelize
    cfg, model = _model(dev, "4c_Fpn432")
    pcl, _ = _scene(dev, 5, 200000)
    coords, feats = voxelize(pcl, 50, cfg.SPARSE3D.VOXEL_FULL_SCALE)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        maps, _ = model.backbone([coords, feats])
    gen = torch.Generator(device=dev).manual_seed(7)
    proj = [None if m is None else torch.randn(m.features.shape, device=dev, generator=gen) for m in maps]

    def grads(dtype, f):
        model.load_state_dict(state)
        model.backbone.compute_dtype = dtype
        try:
            return _backbone_grads(model, coords, f, proj)
        finally:
            model.backbone.compute_dtype = torch.float32

    g32 = grads(torch.float32, feats)
    ref = grads(torch.float32, feats.to(torch.bfloat16).float())
    g16 = grads(torch.bfloat16, feats)
    nz32 = {k for k, g in g32.items() if g.abs().sum() > 0}
    nz16 = {k for k, g in g16.items() if g.abs().sum() > 0}
    assert nz32 == nz16 and len(nz32) > 20, nz32 ^ nz16
    keys = sorted(nz32)
    assert all(g16[k].dtype == torch.float32 and torch.isfinite(g16[k]).all() for k in keys)
    flat = {n: torch.cat([g[k].reshape(-1) for k in keys]) for n, g in (("32", g32), ("16", g16), ("ref", ref))}
    cos_all, cos_ref = _cos(flat["32"], flat["16"]), _cos(flat["32"], flat["ref"])
    big = max(g32[k].norm().item() for k in keys)
    per = {k: (_cos(g32[k], g16[k]), _cos(g32[k], ref[k])) for k in keys if g32[k].norm().item() >= 1e-3 * big}
    worst = min(per, key=lambda k: per[k][0])
    print(f"bf16 vs fp32 backbone gradients: all {cos_all:.5f} (ref {cos_ref:.5f}), per-parameter min "
          f"{per[worst][0]:.5f} (ref {per[worst][1]:.5f}, {worst}), {len(per)} of {len(keys)} compared")
    assert cos_all >= 0.95 and 1 - cos_all <= 8 * (1 - cos_ref), (cos_all, cos_ref)
    bad = {k: v for k, v in per.items() if v[0] < 0.9 or (v[0] < 0.999 and 1 - v[0] > 8 * (1 - v[1]))}
    assert not bad, bad


@pytest.mark.parametrize("name", ["4c_Fpn432", "6c_Fpn4321"])
def test_train_steps_bf16(dev, name):
    """four bf16 steps on one building: finite losses that fall, gradients where test_train_steps expects them"""
    from detection_3d_amd import training as T
    from detection_3d_amd.voxelize import voxelize
    cfg, model = _model(dev, name)
    model.backbone.compute_dtype = torch.bfloat16
    pcl, targets = _scene(dev, 5, 60000)
    coords, feats = voxelize(pcl, 50, cfg.SPARSE3D.VOXEL_FULL_SCALE)
    opt = T.make_optimizer(cfg, model)
    torch.manual_seed(1)
    totals = []
    for it in range(4):
        losses = model([coords, feats], targets)
        total = sum(losses.values())
        assert torch.isfinite(total), losses
        opt.zero_grad()
        total.backward()
        if it == 0:
            got = {k for k, p in model.named_parameters() if p.grad is not None and p.grad.abs().sum() > 0}
            none = {k for k, p in model.named_parameters() if p.grad is None}
            assert "backbone.layers_in.1.weight" in got and "backbone.m_downs.8.1.1.3.weight" in got
            assert "rpn.head.conv.weight" in got and "roi_heads.box.feature_extractor.fc6.weight" in got
            n_up = max(cfg.MODEL.RPN.RPN_SCALES_FROM_TOP + list(cfg.MODEL.ROI_BOX_HEAD.POOLER_SCALES_FROM_TOP))
            assert f"backbone.m_mergeds.{n_up - 1}.weight" in got
            if n_up < 8:
                assert f"backbone.m_mergeds.{n_up}.weight" in none and "backbone.m_ups.7.1.weight" in none
            assert all(p.dtype == torch.float32 for p in model.parameters())
            assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
        opt.step()
        totals.append(total.item())
    assert totals[-1] < totals[0], totals


def test_3g6c_step_bf16(dev):
    from detection_3d_amd import training as T
    from detection_3d_amd.voxelize import voxelize
    cfg, model = _model(dev, "3G6c_Fpn4321")
    model.backbone.compute_dtype = torch.bfloat16
    pcl, targets = _scene(dev, 7, 60000)
    coords, feats = voxelize(pcl, 50, cfg.SPARSE3D.VOXEL_FULL_SCALE)
    opt = T.make_optimizer(cfg, model)
    losses = model([coords, feats], targets)
    total = sum(losses.values())
    assert torch.isfinite(total), losses
    opt.zero_grad()
    total.backward()
    grads = [p.grad for p in model.backbone.parameters() if p.grad is not None]
    assert len(grads) > 20 and all(torch.isfinite(g).all() for g in grads)
    opt.step()


def test_heterogeneous_batch_bf16(dev):
    from detection_3d_amd import engine, training as T
    cfg, model = _model(dev, "4c_Fpn432")
    model.backbone.compute_dtype = torch.bfloat16
    opt = T.make_optimizer(cfg, model)
    points, tgs = engine.collate([_scene(dev, 5, 60000), _scene(dev, 6, 25000, (12.0, 9.0, 2.7))], cfg)
    assert points[2] == 2
    losses = model(points, tgs)
    total = sum(losses.values())
    assert torch.isfinite(total), losses
    opt.zero_grad()
    total.backward()
    grads = [p.grad for p in model.backbone.parameters() if p.grad is not None]
    assert len(grads) > 20 and all(torch.isfinite(g).all() for g in grads)
    opt.step()


class _flag:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.was = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(self.on)

    def __exit__(self, *exc):
        torch.use_deterministic_algorithms(self.was)


@pytest.mark.parametrize("batch", [1, 2])
def test_bf16_step_bit_reproducible(dev, batch):
    """under torch.use_deterministic_algorithms(True): two seeded bf16 SGD steps give the same losses and weights"""
    from detection_3d_amd import engine, training as T
    cfg, model = _model(dev, "4c_Fpn432")
    T.freeze_unused(model)
    model.backbone.compute_dtype = torch.bfloat16
    items = [_scene(dev, 5, 60000), _scene(dev, 6, 25000, (12.0, 9.0, 2.7))][:batch]
    points, tgs = engine.collate(items, cfg)
    if batch == 1:
        points, tgs = [points[0][:, :3].contiguous(), points[1]], tgs[0]
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}

    def run():
        model.load_state_dict(state)
        opt = T.make_optimizer(cfg, model)
        losses = []
        for it in range(2):
            torch.manual_seed(99 + it)
            opt.zero_grad(set_to_none=True)
            l = model(points, tgs)
            total = sum(l.values())
            total.backward()
            opt.step()
            losses.append(total.detach().clone())
        return losses, {k: v.detach().clone() for k, v in model.state_dict().items()}

    with _flag(True):
        l1, w1 = run()
        l2, w2 = run()
    assert all(torch.isfinite(x) for x in l1)
    assert all(torch.equal(a, b) for a, b in zip(l1, l2)), (l1, l2)
    diff = [k for k in w1 if not torch.equal(w1[k], w2[k])]
    assert not diff, diff[:10]
