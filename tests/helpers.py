"""Shared test helpers: small synthetic scenes and a numpy composition of the FPN backbone out of
oracle ops (the checker for the HIP backbone)."""
import contextlib

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


def rules_conv64(x, w, rules, n_out):
    """fp64: y, sum_k |x||w|, ||x o w||_2 and the products of bf16-rounded operands, per output element (an output
    meets an offset at most once in these rulebooks, so a fancy-indexed add per offset is exact)"""
    import torch
    K, cin, cout = w.shape
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    xb = torch.from_numpy(x).to(torch.bfloat16).double().numpy()
    wb = torch.from_numpy(w).to(torch.bfloat16).double().numpy()
    y, a, s2, yb = (np.zeros((n_out, cout)) for _ in range(4))
    for k in range(K):
        sel = rules[:, 2] == k
        i, o = rules[sel, 0], rules[sel, 1]
        assert np.unique(o).size == o.size
        y[o] += x64[i] @ w64[k]
        a[o] += np.abs(x64[i]) @ np.abs(w64[k])
        s2[o] += (x64[i] ** 2) @ (w64[k] ** 2)
        yb[o] += xb[i] @ wb[k]
    return y, a, np.sqrt(s2), yb


def saved_precision():
    """torch's fp32 matmul precision, both APIs' state (the legacy level read while the two agree, as they do between
    tests)"""
    import torch
    return (torch.get_float32_matmul_precision(), torch.backends.cuda.matmul.fp32_precision,
            torch.backends.fp32_precision)


def restore_precision(saved):
    import torch
    legacy, matmul, generic = saved
    torch.set_float32_matmul_precision(legacy)
    torch.backends.fp32_precision = generic
    torch.backends.cuda.matmul.fp32_precision = matmul


@contextlib.contextmanager
def precision(value):
    """'tf32' -> set_float32_matmul_precision('high'), 'ieee' -> 'highest' for the block, restored afterwards (fp32
    sparse convolutions run as bf16x3 under 'tf32')"""
    import torch
    saved = saved_precision()
    torch.set_float32_matmul_precision("high" if value == "tf32" else "highest")
    try:
        yield
    finally:
        restore_precision(saved)
