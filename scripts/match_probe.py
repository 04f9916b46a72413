"""Development probe: label assignment of a 2-example batch (configs/6c fpn4321, 2 x 500k-point synthetic buildings).

    python scripts/match_probe.py --mode {none,batch,loop} [--reps 20]
    rocprofv3 --kernel-trace --stats -d OUT -o match -- python scripts/match_probe.py --mode batch

Setup (identical in every mode): voxelise + collate both buildings, backbone, RPN head, anchors, training proposal selection
per example, GT boxes added.  Then `reps` times:
    batch: RPNLoss.prepare_targets_segments over all anchors of the batch + the ROI matching of all proposals, each ONE
           d3d_match_segments launch set (k_match_pass1 / k_match_pass2)
    loop:  the same calls once per example (one segment each): one d3d_match_segments launch set per example and stage
    none:  nothing (the setup's kernels, to subtract)
Prints one JSON line (host wall time per rep of the phase, with a device synchronisation around it)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                               # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("none", "batch", "loop"), default="batch")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=500_000)
    args = ap.parse_args()
    from detection_3d_amd import box_ops, engine, training as T
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.detector import build_detection_model
    from detection_3d_amd.synthetic import make_scene, make_targets
    dev = torch.device("cuda:0")
    cfg = get_cfg("6c_Fpn4321")
    torch.manual_seed(0)
    model = build_detection_model(cfg).to(dev).train()
    scenes = []
    for seed in (0, 1):
        b, l = make_targets(seed)
        scenes.append((torch.from_numpy(make_scene(seed, args.points)).to(dev),
                       {"bbox3d": torch.from_numpy(b).to(dev), "labels": torch.from_numpy(l).to(dev)}))
    points, tgs = engine.collate(scenes, cfg)
    rpn = model.rpn
    with torch.no_grad():
        rpn_feats, _ = model.backbone(points[:2])
        obj, reg = rpn.head([f.features for f in rpn_feats])
        anchors = rpn.anchor_generator.forward_cat(rpn_feats)
        A = rpn.anchor_generator.num_anchors_per_location()
        example = torch.cat([f.get_spatial_locations()[:, 3].repeat_interleave(A) for f in rpn_feats])
        segs = rpn.select_proposals_segments(obj, reg, anchors, example, 2, True)
        props = [torch.cat([p, t["bbox3d"]]) for (p, _), t in zip(segs, tgs)]
        props = [p.clone() for p in props]
        for p in props:
            p[:, 3:6] = torch.clamp(p[:, 3:6], min=0.001)
    prop_all = torch.cat(props)
    prop_seg = torch.cat([torch.full((p.shape[0],), i, dtype=torch.int64, device=dev) for i, p in enumerate(props)])
    ex32 = example.to(torch.int32).contiguous()
    rpn_l, roi_l = rpn.loss_evaluator, model.roi_heads.box.loss_evaluator
    gts = [t["bbox3d"] for t in tgs]

    def batch():
        rpn_l.prepare_targets_segments(anchors, ex32, gts)
        gt, offs = T.segment_offsets(gts)
        m = roi_l.matcher
        box_ops.match_segments(gt, offs, prop_all, prop_seg.to(torch.int32), roi_l.aug, criterion=-1,
                               high=m.high_threshold, low=m.low_threshold, encode_weights=roi_l.weights)

    def loop():
        m = roi_l.matcher
        for b in range(2):
            rows = example == b
            a_b = anchors[rows]
            rpn_l.prepare_targets_segments(a_b, torch.zeros(a_b.shape[0], dtype=torch.int32, device=dev), [gts[b]])
            box_ops.match_segments(gts[b], [0, gts[b].shape[0]], props[b],
                                   torch.zeros(props[b].shape[0], dtype=torch.int32, device=dev), roi_l.aug,
                                   criterion=-1, high=m.high_threshold, low=m.low_threshold,
                                   encode_weights=roi_l.weights)

    fn = {"batch": batch, "loop": loop, "none": lambda: None}[args.mode]
    with torch.no_grad():
        fn()                                                     # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    print(json.dumps({"mode": args.mode, "reps": args.reps, "anchors": int(anchors.shape[0]),
                      "proposals": [int(p.shape[0]) for p in props], "gt": [int(g.shape[0]) for g in gts],
                      "ms_per_rep": 1e3 * dt / max(args.reps, 1)}), flush=True)


if __name__ == "__main__":
    main()
