"""fp32 heads against bf16 heads (SparseRCNN.head_dtype), interleaved, in one process; prints one JSON line.

    python scripts/heads_bf16_probe.py [--reps 7] [--infer-points 1000000 --infer-batch 4] [--train-points 500000]

Workloads: (1) the bench's bf16 region -- 4c, a batch of `--infer-batch` buildings of `--infer-points` points, backbone in
bf16 storage, one inference pass (voxelisation outside the timed span); (2) one 6c training step (forward, backward, SGD)
on a building of `--train-points` points, fp32 backbone.  Each repetition times fp32 heads and bf16 heads back to back
(alternating which goes first), after one untimed warm-up pass of each; medians of wall time with a device
synchronisation on both ends."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--infer-points", type=int, default=1_000_000)
    ap.add_argument("--infer-batch", type=int, default=4)
    ap.add_argument("--train-points", type=int, default=500_000)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    from detection_3d_amd import engine, training as T
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.detector import build_detection_model
    from detection_3d_amd.synthetic import make_scene, make_targets
    from detection_3d_amd.voxelize import voxelize
    dev = torch.device("cuda:0")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def interleaved(run):
        """run(dtype) -> None; medians (ms) of fp32 and bf16 heads, alternating the order"""
        for dt in (torch.float32, torch.bfloat16):
            run(dt)
        ms = {torch.float32: [], torch.bfloat16: []}
        for r in range(args.reps):
            order = (torch.float32, torch.bfloat16) if r % 2 == 0 else (torch.bfloat16, torch.float32)
            for dt in order:
                ms[dt].append(timed(lambda: run(dt)))
        return {"fp32_heads_ms": statistics.median(ms[torch.float32]),
                "bf16_heads_ms": statistics.median(ms[torch.bfloat16]),
                "fp32_heads_all_ms": [round(v, 3) for v in ms[torch.float32]],
                "bf16_heads_all_ms": [round(v, 3) for v in ms[torch.bfloat16]]}

    # (1) inference, bf16 backbone, 4 x 1 M points
    cfg = get_cfg("4c_Fpn432")
    torch.manual_seed(args.seed)
    model = build_detection_model(cfg).to(dev).eval()
    model.backbone.compute_dtype = torch.bfloat16
    B = args.infer_batch
    cs, fs = [], []
    for b in range(B):
        pcl = torch.from_numpy(make_scene(500 + b, args.infer_points, (35.0, 27.0, 2.7))).to(dev)
        c, f = voxelize(pcl, cfg.SPARSE3D.VOXEL_SCALE, cfg.SPARSE3D.VOXEL_FULL_SCALE)
        cs.append(torch.cat([c, torch.full((c.shape[0], 1), b, dtype=torch.int64, device=dev)], 1))
        fs.append(f)
    points = [torch.cat(cs), torch.cat(fs), B]

    def infer(dt):
        model.head_dtype = dt
        model(points)

    out = {"inference_4c_bf16_backbone": dict(interleaved(infer), batch=B, points_per_building=args.infer_points)}
    del model

    # (2) training step, 6c, fp32 backbone
    cfg = get_cfg("6c_Fpn4321")
    torch.manual_seed(args.seed)
    model = build_detection_model(cfg).to(dev).train()
    T.freeze_unused(model)
    opt = T.make_optimizer(cfg, model)
    bx, lb = make_targets(7)
    scene = (torch.from_numpy(make_scene(7, args.train_points)).to(dev),
             {"bbox3d": torch.from_numpy(bx).to(dev), "labels": torch.from_numpy(lb).to(dev)})
    pts, tgs = engine.collate([scene], cfg)
    pts, tgs = [pts[0][:, :3].contiguous(), pts[1]], tgs[0]
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}

    def train(dt):
        model.load_state_dict(state)           # every step from the same weights
        model.head_dtype = dt
        torch.manual_seed(args.seed + 1)
        opt.zero_grad(set_to_none=True)
        sum(model(pts, tgs).values()).backward()
        opt.step()

    out["train_6c_fp32_backbone"] = dict(interleaved(train), points_per_building=args.train_points)
    out.update(reps=args.reps, seed=args.seed, unit="ms (median wall time per pass)")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
