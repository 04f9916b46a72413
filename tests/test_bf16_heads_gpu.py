"""bf16 heads (SparseRCNN.head_dtype = torch.bfloat16): the RPN head, RoI pooling and the box head on bf16 operands.

Kernels: d3d_rpn_head_bf16 against an fp64 reference built from the same bf16 operands (t rounded to bf16 as the kernel
rounds it); the bf16 RoIAlign forward bit for bit against the fp32 kernel on the widened map, rounded; the bf16
fixed-order backward bit for bit against the fp32 fixed-order backward into zeros, rounded; the bf16 atomic backward
within one bf16 ulp of that.  Detector: inference and training against the fp32-head model from the same weights."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(autouse=True)
def _bf16_heads_built():
    """fails in Python, before anything is launched, on a library without the bf16 head entry points"""
    from detection_3d_amd import _lib
    assert hasattr(_lib.lib(), "d3d_rpn_head_bf16")


class _flag:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.was = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(self.on)

    def __exit__(self, *exc):
        torch.use_deterministic_algorithms(self.was)


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------------
# RPN head
def _rpn_reference(head, feats):
    """fp64 reference from the bf16 operands: t = bf16(relu(x W1^T + b1)), out = t W2^T + b2; -> (obj, reg, bound)"""
    c = head.conv.weight.shape[0]
    w1 = head.conv.weight.detach().view(c, c).to(BF).double()
    w2 = torch.cat([head.cls_logits.weight.detach().view(-1, c), head.bbox_pred.weight.detach().view(-1, c)]).to(BF).double()
    b1 = head.conv.bias.detach().double()
    b2 = torch.cat([head.cls_logits.bias.detach(), head.bbox_pred.bias.detach()]).double()
    x = torch.cat(feats).double()
    t = torch.relu(x @ w1.t() + b1).float().to(BF).double()
    out = t @ w2.t() + b2
    mag = t.abs() @ w2.abs().t()
    # bf16 rounding of t (2^-8 of each |t| |w| term) + fp32 accumulation
    bound = 2.0 ** -8 * mag + 2e-5 * (mag + b2.abs()) + 1e-30
    a = head.num_anchors_per_location * head.seperate_rpn
    return out[:, :a], out[:, a:], bound[:, :a], bound[:, a:]


def _rpn_head(dev, config, channels, anchors):
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.detector import RPNHead
    cfg = get_cfg(config)
    torch.manual_seed(channels + anchors)
    head = RPNHead(cfg, channels, anchors).to(dev).eval()
    with torch.no_grad():
        for p in head.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return head


@pytest.mark.parametrize("channels", [128, 256])
@pytest.mark.parametrize("rows,anchors", [([1000, 333, 37], 4), ([5], 4), ([64, 0, 31], 1), ([0], 4),
                                          ([700, 129, 64, 1, 33, 0], 4), ([97, 40], "gate")])
def test_rpn_head_bf16_kernel(dev, channels, rows, anchors):
    a = channels // 8 if anchors == "gate" else anchors          # "gate": the widest head the fused kernel takes
    head = _rpn_head(dev, "4c_Fpn432", channels, a)
    assert head.num_anchors_per_location * head.seperate_rpn * 8 <= channels
    feats = [torch.randn(n, channels, device=dev).to(BF) for n in rows]
    with torch.no_grad():
        assert head._fused_ok(feats)
        obj, reg = head(feats)
    assert obj.dtype == reg.dtype == torch.float32
    wo, wr, bo, br = _rpn_reference(head, feats)
    assert obj.shape == (sum(rows) * head.num_anchors_per_location, head.seperate_rpn)
    assert (obj.reshape(wo.shape).double() - wo).abs().le(bo).all()
    assert (reg.reshape(wr.shape).double() - wr).abs().le(br).all()
    # the weights are re-packed after an update
    with torch.no_grad():
        head.conv.weight.mul_(2)
        obj2, _ = head(feats)
    wo2, _, bo2, _ = _rpn_reference(head, feats)
    assert (obj2.reshape(wo2.shape).double() - wo2).abs().le(bo2).all()


def test_rpn_head_3g6c_groups_bf16(dev):
    """three class groups: 96 output columns (three tiles) of a 128-channel head"""
    head = _rpn_head(dev, "3G6c_Fpn4321", 128, 4)
    assert head.seperate_rpn == 3
    feats = [torch.randn(n, 128, device=dev).to(BF) for n in (513, 64, 1)]
    with torch.no_grad():
        assert head._fused_ok(feats)
        obj, reg = head(feats)
    wo, wr, bo, br = _rpn_reference(head, feats)
    assert (obj.reshape(wo.shape).double() - wo).abs().le(bo).all()
    assert (reg.reshape(wr.shape).double() - wr).abs().le(br).all()


@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_rpn_head_wider_than_the_gate_falls_back(dev, dtype):
    """8a > C: the library GEMMs in both types (before the gate the fp32 launch raised D3DError)"""
    head = _rpn_head(dev, "4c_Fpn432", 128, 17)
    feats = [torch.randn(n, 128, device=dev).to(dtype) for n in (100, 7)]
    with torch.no_grad():
        assert not head._fused_ok(feats)
        obj, reg = head(feats)
    assert obj.dtype == reg.dtype == torch.float32
    x = torch.cat(feats).float()
    t = torch.relu(x @ head.conv.weight.view(128, 128).t().float() + head.conv.bias)
    wo = (t @ head.cls_logits.weight.view(-1, 128).t() + head.cls_logits.bias).reshape(obj.shape)
    tol = 1e-4 if dtype == torch.float32 else 3e-2
    assert (obj - wo).abs().max() <= tol * wo.abs().max()


# ---------------------------------------------------------------------------------------------------------------------
# RoI pooling
@pytest.fixture(scope="module")
def maps(dev):
    """the roi maps of a two-example batch of 4c (fp32, one metadata; example ids in the coordinates)"""
    from detection_3d_amd import engine
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.detector import build_detection_model
    from detection_3d_amd.synthetic import make_scene, make_targets
    cfg = get_cfg("4c_Fpn432")
    torch.manual_seed(3)
    model = build_detection_model(cfg).to(dev).eval()
    scenes = []
    for seed, n, ext in ((4, 40000, (25.0, 19.0, 2.7)), (5, 20000, (12.0, 9.0, 2.7))):
        b, l = make_targets(seed, ext)
        scenes.append((torch.from_numpy(make_scene(seed, n, ext)).to(dev),
                       {"bbox3d": torch.from_numpy(b).to(dev), "labels": torch.from_numpy(l).to(dev)}))
    points, _ = engine.collate(scenes, cfg)
    with torch.no_grad():
        _, roi_maps = model.backbone(points[:2])
    return cfg, model, roi_maps


def _rois(maps_, K, seed, scale, batch=2):
    rng = np.random.RandomState(seed)
    loc = maps_.get_spatial_locations().cpu().numpy()
    crop = loc[:, :3].max(0) + 1
    r = np.zeros((K, 8), np.float32)
    r[:, 0] = rng.randint(0, batch, K)
    r[:, 1] = rng.rand(K) * crop[1] / scale
    r[:, 2] = rng.rand(K) * crop[0] / scale
    r[:, 3] = rng.rand(K) * crop[2] / scale
    r[:, 4] = (1 + rng.rand(K) * 6) / scale
    r[:, 5] = (1 + rng.rand(K) * 6) / scale
    r[:, 6] = (1 + rng.rand(K) * 3) / scale
    r[:, 7] = rng.rand(K) * 180
    return torch.from_numpy(r).to(maps_.features.device), [int(c) for c in crop]


def _bf16_map(m):
    from detection_3d_amd import sparseconvnet as scn
    return scn.SparseConvNetTensor(m.features.to(BF), m.metadata, m.spatial_size)


def _up(m):
    from detection_3d_amd import sparseconvnet as scn
    return scn.SparseConvNetTensor(m.features.float(), m.metadata, m.spatial_size)


@pytest.mark.parametrize("K", [0, 1, 300])
@pytest.mark.parametrize("channels_inner", [False, True])
@pytest.mark.parametrize("crop", [False, True])
def test_roi_forward_bf16_single_level(maps, K, channels_inner, crop):
    from detection_3d_amd.roi_align_rotated_3d import roi_align_rotated_3d_sparse_into
    _, _, roi_maps = maps
    m16 = _bf16_map(roi_maps[0])
    scale = 1.0 / 4
    rois, cr = _rois(m16, K, 11 + K, scale)
    shape = (K, 7, 7, 128, 3) if channels_inner else (K, 128, 7, 7, 3)
    got = torch.full(shape, 7.0, dtype=BF, device=rois.device)
    want = torch.full(shape, 7.0, dtype=torch.float32, device=rois.device)
    kw = dict(crop=cr if crop else None, channels_inner=channels_inner)
    roi_align_rotated_3d_sparse_into(got, m16, rois, scale, 2, **kw)
    roi_align_rotated_3d_sparse_into(want, _up(m16), rois, scale, 2, **kw)
    assert torch.equal(_bits(got), _bits(want.to(BF)))
    if K > 1:
        assert got.float().abs().max() > 0


@pytest.mark.parametrize("channels_inner", [False, True])
def test_roi_forward_bf16_levels(maps, channels_inner):
    from detection_3d_amd.roi_align_rotated_3d import roi_align_rotated_3d_sparse_levels_into
    cfg, _, roi_maps = maps
    scales = cfg.MODEL.ROI_BOX_HEAD.POOLER_SCALES_SPATIAL
    assert len(roi_maps) >= 2
    m16 = [_bf16_map(m) for m in roi_maps]
    K = 257
    rois, _ = _rois(m16[0], K, 5, scales[0])
    levels = torch.from_numpy(np.random.RandomState(1).randint(-1, len(m16), K).astype(np.int32)).to(rois.device)
    ph, pw, pz = cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION
    shape = (K, ph, pw, 128, pz) if channels_inner else (K, 128, ph, pw, pz)
    got = torch.full(shape, 3.0, dtype=BF, device=rois.device)
    want = torch.full(shape, 3.0, dtype=torch.float32, device=rois.device)
    roi_align_rotated_3d_sparse_levels_into(got, m16, rois, scales, 2, levels, channels_inner=channels_inner)
    roi_align_rotated_3d_sparse_levels_into(want, [_up(m) for m in m16], rois, scales, 2, levels,
                                            channels_inner=channels_inner)
    assert torch.equal(_bits(got), _bits(want.to(BF)))
    assert (got[levels.long() == -1] == 3.0).all()


def _pool_grad(m, rois, scale, g, deterministic):
    from detection_3d_amd import sparseconvnet as scn
    from detection_3d_amd.roi_align_rotated_3d import roi_align_rotated_3d_sparse
    f = m.features.detach().clone().requires_grad_(True)
    with _flag(deterministic):
        out = roi_align_rotated_3d_sparse(scn.SparseConvNetTensor(f, m.metadata, m.spatial_size), rois, scale, 7, 7, 3, 2)
        assert out.dtype == f.dtype
        out.backward(g.to(out.dtype))
    assert f.grad.dtype == f.dtype and f.grad.shape == f.shape
    return f.grad


@pytest.mark.parametrize("K", [0, 200])
def test_roi_backward_bf16(maps, K):
    _, _, roi_maps = maps
    m16 = _bf16_map(roi_maps[0])
    scale = 1.0 / 4
    rois, _ = _rois(m16, K, 21, scale)
    g = torch.randn((K, 128, 7, 7, 3), device=rois.device).to(BF)
    ref = _pool_grad(_up(m16), rois, scale, g.float(), True)        # fp32 fixed-order form into zeros
    det = _pool_grad(m16, rois, scale, g, True)
    assert torch.equal(_bits(det), _bits(ref.to(BF)))
    det2 = _pool_grad(m16, rois, scale, g, True)
    assert torch.equal(_bits(det), _bits(det2))
    atom = _pool_grad(m16, rois, scale, g, False)
    r = ref.to(BF).float()
    ulp = torch.where(r == 0, torch.zeros_like(r), 2.0 ** (torch.floor(torch.log2(r.abs().clamp_min(1e-38))) - 7))
    assert ((atom.float() - r).abs() <= ulp + 1e-6 * ref.abs().max()).all()
    untouched = (ref == 0).all(1)
    assert (det[untouched] == 0).all() and (atom[untouched] == 0).all()
    if K:
        assert untouched.any() and not untouched.all()
    else:
        assert untouched.all()


# ---------------------------------------------------------------------------------------------------------------------
# detector
def _model(dev, name, train):
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.detector import build_detection_model
    cfg = get_cfg(name)
    torch.manual_seed(0)
    model = build_detection_model(cfg).to(dev)
    return cfg, (model.train() if train else model.eval())


def _batch(dev, cfg, B, n=40000):
    from detection_3d_amd import engine
    from detection_3d_amd.synthetic import make_scene, make_targets
    scenes = []
    for seed, ext in ((5, (25.0, 19.0, 2.7)), (6, (12.0, 9.0, 2.7)))[:B]:
        b, l = make_targets(seed, ext)
        scenes.append((torch.from_numpy(make_scene(seed, n, ext)).to(dev),
                       {"bbox3d": torch.from_numpy(b).to(dev), "labels": torch.from_numpy(l).to(dev)}))
    points, tgs = engine.collate(scenes, cfg)
    if B == 1:
        return [points[0][:, :3].contiguous(), points[1]], tgs[0]
    return points, tgs


@pytest.mark.parametrize("name", ["4c_Fpn432", "3G6c_Fpn4321"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("backbone", [torch.float32, BF])
def test_inference_bf16_heads(dev, name, B, backbone):
    """RPN outputs within 2^-6 of the largest |output| of the fp32-head run (bf16 operands of a 128-channel head, the
    t rounding: measured <= 2^-8 here); the box head on the SAME proposals (at random initialisation the objectness of
    ~1 M anchors has near-ties, and top-k / NMS may keep other proposals for differences far below any bf16 bound):
    at least 95 % of the fp32-head detections with score > 0.5 have a bf16-head detection of their label whose box
    agrees to 5e-2 in every coordinate (metres, radians: the same proposal, a regression that moved by far less) and
    whose score is within 2e-2 (measured: <= 2e-3).  The rest are near-ties that NMS or the per-image top-k cut
    resolves the other way (a displaced detection's nearest same-label bf16 box was 1.2-2.7 m away).  With a bf16 backbone the maps reach the heads as bf16 (no fp32 copy)."""
    cfg, model = _model(dev, name, False)
    model.backbone.compute_dtype = backbone
    with torch.no_grad():                     # spread scores (no near-ties for NMS to order), some above 0.5
        model.roi_heads.box.predictor.cls_score.weight.mul_(40)
        model.roi_heads.box.predictor.cls_score.bias[1] += 1.0
        model.rpn.head.cls_logits.weight.mul_(30)
    points, _ = _batch(dev, cfg, B)
    seen = {}

    def record(module, args):
        seen.setdefault(model.head_dtype, args[0][0].dtype)

    hook = model.rpn.head.register_forward_pre_hook(record)
    res32, mid32 = model(points, return_intermediates=True)
    model.head_dtype = BF
    res16, mid16 = model(points, return_intermediates=True)
    hook.remove()
    assert seen[torch.float32] == torch.float32 and seen[BF] == BF
    if backbone == BF:
        # the very tensors of the backbone's maps: no copy in front of the heads
        for m in mid16["rpn_features"] + mid16["roi_features"]:
            assert m is None or m.features.dtype == BF
    # RPN head outputs on the two runs' maps (same maps up to the bf16 rounding of an fp32 backbone's rows)
    with torch.no_grad():
        o32, r32 = model.rpn.head([m.features for m in mid32["rpn_features"]])
        o16, r16 = model.rpn.head([m.features for m in mid16["rpn_features"]])
    assert o16.dtype == torch.float32
    assert (o16 - o32).abs().max() <= 2.0 ** -6 * o32.abs().max()
    assert (r16 - r32).abs().max() <= 2.0 ** -6 * r32.abs().max()
    # box head + post-processing on the fp32 run's proposals
    box = model.roi_heads.box
    props = mid32["proposals"]
    kw = dict(sep_id=mid32["sep_id"], example_id=mid32["example_id"], n_examples=B)
    with torch.no_grad():
        d32 = box(mid32["roi_features"], props, **kw)
        d16 = box(mid16["roi_features"], props, **kw)
    d32, d16 = (d32, d16) if B > 1 else ([d32], [d16])
    n_conf, n_matched = 0, 0
    for a, b in zip(d32, d16):
        conf = a["scores"] > 0.5
        n_conf += int(conf.sum())
        for i in torch.nonzero(conf).view(-1).tolist():
            same = torch.nonzero(b["labels"] == a["labels"][i]).view(-1)
            dist = (b["bbox3d"][same] - a["bbox3d"][i]).abs().max(1)[0]      # metres / radians
            n_matched += int(((dist <= 5e-2) & ((b["scores"][same] - a["scores"][i]).abs() <= 2e-2)).any())
    print(f"{name} B={B} backbone={backbone}: {n_matched} of {n_conf} detections with score > 0.5 matched")
    assert n_conf > 0 and n_matched >= 0.95 * n_conf, (n_matched, n_conf)
    r16 = res16 if B > 1 else [res16]
    assert all(r["scores"].dtype == torch.float32 and torch.isfinite(r["bbox3d"]).all() for r in r16)


def _step(model, points, tgs, seed=99):
    model.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    losses = model(points, tgs)
    total = sum(losses.values())
    total.backward()
    return ({k: v.detach().clone() for k, v in losses.items()},
            {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None})


def _cos(x, y):
    x, y = x.reshape(-1).double(), y.reshape(-1).double()
    return float(x @ y / (x.norm() * y.norm()))


@pytest.mark.parametrize("name", ["4c_Fpn432", "6c_Fpn4321", "3G6c_Fpn4321"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("backbone", [torch.float32, BF])
def test_training_step_bf16_heads(dev, name, B, backbone):
    """one step from the same weights and batch, fp32 heads against bf16 heads, under the torch flag (both runs sample
    the same RoIs when their proposals agree): finite losses within 5e-2 relative of the fp32-head step in total,
    fp32 parameter gradients with cosine >= 0.99 over all parameters together"""
    from detection_3d_amd import training as T
    cfg, model = _model(dev, name, True)
    T.freeze_unused(model)
    model.backbone.compute_dtype = backbone
    points, tgs = _batch(dev, cfg, B, 30000)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    with _flag(True):
        l32, g32 = _step(model, points, tgs)
        model.load_state_dict(state)
        model.head_dtype = BF
        l16, g16 = _step(model, points, tgs)
    assert set(l16) == set(l32) and set(g16) == set(g32)
    t32, t16 = sum(float(v) for v in l32.values()), sum(float(v) for v in l16.values())
    assert all(torch.isfinite(v) for v in l16.values()), l16
    print(f"{name} B={B} backbone={backbone}: total loss fp32 heads {t32:.6f}, bf16 heads {t16:.6f}; per loss "
          + ", ".join(f"{k} {float(l32[k]):.5f}/{float(l16[k]):.5f}" for k in sorted(l32)))
    assert abs(t16 - t32) <= 5e-2 * abs(t32)
    assert all(g.dtype == torch.float32 and torch.isfinite(g).all() for g in g16.values())
    keys = sorted(g32)
    cos = _cos(torch.cat([g32[k].reshape(-1) for k in keys]), torch.cat([g16[k].reshape(-1) for k in keys]))
    print(f"  gradient cosine {cos:.5f}")
    assert cos >= 0.99


@pytest.mark.parametrize("backbone", [torch.float32, BF])
def test_bf16_heads_step_bit_reproducible(dev, backbone):
    from detection_3d_amd import training as T
    cfg, model = _model(dev, "4c_Fpn432", True)
    T.freeze_unused(model)
    model.backbone.compute_dtype = backbone
    model.head_dtype = BF
    points, tgs = _batch(dev, cfg, 2, 30000)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}

    def run():
        model.load_state_dict(state)
        opt = T.make_optimizer(cfg, model)
        l, g = _step(model, points, tgs)
        opt.step()
        return l, g, {k: v.detach().clone() for k, v in model.state_dict().items()}

    with _flag(True):
        l1, g1, w1 = run()
        l2, g2, w2 = run()
    assert all(torch.equal(l1[k], l2[k]) for k in l1)
    assert all(torch.equal(g1[k], g2[k]) for k in g1)
    assert all(torch.equal(w1[k], w2[k]) for k in w1)


def test_default_head_dtype_unchanged(dev):
    """head_dtype = torch.float32 set explicitly gives the bits of a model whose attribute was never touched"""
    cfg, model = _model(dev, "4c_Fpn432", False)
    points, _ = _batch(dev, cfg, 1)
    assert model.head_dtype == torch.float32
    r1 = model(points)
    model.head_dtype = torch.float32
    r2 = model(points)
    assert all(torch.equal(r1[k], r2[k]) for k in r1)
    cfg, model = _model(dev, "4c_Fpn432", True)
    points, tgs = _batch(dev, cfg, 1, 30000)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    with _flag(True):
        l1, g1 = _step(model, points, tgs)
        model.load_state_dict(state)
        model.head_dtype = torch.float32
        l2, g2 = _step(model, points, tgs)
    assert all(torch.equal(l1[k], l2[k]) for k in l1)
    assert all(torch.equal(g1[k], g2[k]) for k in g1)
