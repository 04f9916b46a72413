"""Shared test helpers: small synthetic scenes and a numpy composition of the FPN backbone out of
oracle ops (the checker for the HIP backbone)."""
import numpy as np

import oracle


def small_scene(seed, n_points, extent, full_scale, scale=50):
    from detection_3d_amd.synthetic import make_scene
    pcl = make_scene(seed, n_points, extent)
    coords, feats = oracle.voxelize(pcl, scale, full_scale)
    return pcl, coords, feats


def canon_rules(trip):
    """sorted (offset, in, out) rows of an (in, out, offset) triple list"""
    t = np.asarray(trip, np.int64).reshape(-1, 3)
    order = np.lexsort((t[:, 1], t[:, 0], t[:, 2]))
    return t[order]


def nbr_to_rules(nbr):
    n, K = nbr.shape
    out_ids, ks = np.nonzero(nbr >= 0)
    return np.stack([nbr[out_ids, ks], out_ids, ks], 1)


from oracle.detector_port import OracleDetector, OracleFPN  # noqa: E402,F401


def sort_by_loc(feats, loc):
    loc = np.asarray(loc)
    order = np.lexsort((loc[:, 2], loc[:, 1], loc[:, 0], loc[:, 3]))
    return feats[order], loc[order]


def label_differences_sit_on_thresholds(lab_a, lab_b, q_a, q_b, low, high, eps=1e-6):
    """Matcher labels from two IoU matrices q_a / q_b [M gt, N] (both already yaw-masked) may differ only where an IoU sits on
    one of the Matcher's thresholds (modeling/matcher.py:84-100,131-158): the low / high thresholds on a column's
    maximum, a gt's best quality (the ties that become low-quality matches) and its ignore threshold max(0.02,
    best - 0.05).  -> (number of differing columns, list of unexplained column indices)."""
    lab_a, lab_b = np.asarray(lab_a), np.asarray(lab_b)
    diff = np.nonzero(lab_a != lab_b)[0]
    bad = []
    if not len(diff):
        return 0, bad
    q_a, q_b = np.asarray(q_a, np.float64), np.asarray(q_b, np.float64)
    best = np.stack([q_a.max(1), q_b.max(1)])                                   # [2, M]
    ign = np.maximum(0.02, best - 0.05)
    for j in diff:
        ok = False
        for q in (q_a, q_b):
            col = q[:, j]
            m = col.max()
            ok |= min(abs(m - low), abs(m - high)) <= eps
            ok |= bool((np.abs(col[None] - best) <= eps).any()) or bool((np.abs(col[None] - ign) <= eps).any())
        if not ok:
            bad.append(int(j))
    return len(diff), bad


def rpn_targets_reference(lossf, anchors, gt_boxes):
    """What d3d_match_segments fuses, in tensor ops, for one RPN segment (rpn/loss_3d.py:88-109,178-213):
    boxes_iou_3d + Matcher (yaw mask, low-quality rule) + box_encode.  lossf: training.RPNLoss.
    -> labels fp32 [N] (1 pos, 0 neg, -1 ignored), regression targets [N, 7]."""
    import math
    import torch
    from detection_3d_amd import box_ops, training as T
    if gt_boxes.shape[0] == 0:
        return torch.zeros(anchors.shape[0], device=anchors.device), torch.zeros_like(anchors)
    q = box_ops.boxes_iou_3d(gt_boxes, anchors, lossf.aug, criterion=2, flag='rpn_label_generation')
    yaw_diff = torch.abs(box_ops.limit_period(gt_boxes[:, -1].view(-1, 1) - anchors[:, -1].view(1, -1), 0.5, math.pi))
    matched = lossf.matcher(q, yaw_diff=yaw_diff)
    labels = (matched >= 0).to(torch.float32)
    labels[matched == T.Matcher.BETWEEN_THRESHOLDS] = -1
    return labels, T.box_encode(gt_boxes[matched.clamp(min=0)], anchors)


def roi_subsample_reference(lossf, proposals, gt_boxes, gt_labels):
    """The same for one RoI segment plus its sampling (box_head_3d/loss.py:66-160): boxes_iou_3d + Matcher + box_encode,
    then lossf.sampler.  lossf: training.ROILoss.  -> (sampled proposals, labels int64, regression targets), in row
    order."""
    import torch
    from detection_3d_amd import box_ops, training as T
    if gt_boxes.shape[0] == 0:
        labels = torch.zeros(proposals.shape[0], dtype=torch.int64, device=proposals.device)
        reg = torch.zeros_like(proposals)
    else:
        q = box_ops.boxes_iou_3d(gt_boxes, proposals, lossf.aug, criterion=-1, flag='roi_label_generation')
        matched = lossf.matcher(q)
        labels = gt_labels[matched.clamp(min=0)].to(torch.int64)
        labels[matched == T.Matcher.BELOW_LOW_THRESHOLD] = 0
        labels[matched == T.Matcher.BETWEEN_THRESHOLDS] = -1
        reg = T.box_encode(gt_boxes[matched.clamp(min=0)], proposals, lossf.weights)
    pos, neg = lossf.sampler(labels)
    keep = torch.sort(torch.cat([pos, neg]))[0]
    return proposals[keep], labels[keep], reg[keep]
