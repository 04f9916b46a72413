"""The whole detector on a tiny synthetic building with the grouped top-down path (fpn_net.GROUP_CONVS) on and off:
every RPN map, every RoI map and the detections must be bit-identical."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_grouped_top_down_path_is_bit_identical(dev):
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.detector import build_detection_model
    from detection_3d_amd.sparseconvnet import fpn_net
    from detection_3d_amd.synthetic import make_scene
    from detection_3d_amd.voxelize import voxelize
    cfg = get_cfg("4c_Fpn432")
    torch.manual_seed(1)
    model = build_detection_model(cfg).to(dev).eval()
    with torch.no_grad():                       # spread the scores so that NMS / thresholds bite
        model.rpn.head.cls_logits.weight.mul_(60)
        model.rpn.head.bbox_pred.weight.mul_(20)
        model.roi_heads.box.predictor.cls_score.weight.mul_(40)
        model.roi_heads.box.predictor.bbox_pred.weight.mul_(100)
    pcl = torch.from_numpy(make_scene(3, 20000)).to(dev)
    coords, feats = voxelize(pcl, cfg.SPARSE3D.VOXEL_SCALE, cfg.SPARSE3D.VOXEL_FULL_SCALE)
    was = fpn_net.GROUP_CONVS
    runs = {}
    try:
        for on in (True, False):
            fpn_net.GROUP_CONVS = on
            with torch.no_grad():
                runs[on] = model([coords, feats], return_intermediates=True)
    finally:
        fpn_net.GROUP_CONVS = was
    (res_a, mid_a), (res_b, mid_b) = runs[True], runs[False]
    for key in ("rpn_features", "roi_features"):
        assert len(mid_a[key]) == len(mid_b[key]) > 0
        for a, b in zip(mid_a[key], mid_b[key]):
            assert a.spatial_size.tolist() == b.spatial_size.tolist()
            assert a.features.shape[0] > 0 and torch.equal(a.features, b.features)
    assert res_a["bbox3d"].shape[0] > 0
    for key in ("bbox3d", "scores", "labels"):
        assert torch.equal(res_a[key], res_b[key]), key
