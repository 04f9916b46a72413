"""Cost of the on-device augmentation (detection_3d_amd.augment) against plain voxelize, and of a 6c training step with
and without it.

    python scripts/augment_probe.py [--calls 60] [--train-steps 12] [--out FILE]

Per case: warm calls first, then `calls` rounds that each time one plain voxelize and one augmented call with events
(interleaved, so that clocks and caches drift alike); the medians are reported.  Cases: 500 k points of the 25 x 19 m
synthetic building, 500 k points of a 50 x 50 m one, and 4 buildings of 1 M points in a row -- each with elastic off
and on.  Then engine.train on the 6c config, augment=None against everything on (rotate='quarter').  One JSON line per
result."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def probe_calls(cfg, dev, clouds, elastic, calls, warm=5):
    from detection_3d_amd.augment import Augment
    from detection_3d_amd.voxelize import voxelize
    aug = Augment(rotate="quarter", flip_x=True, scale_jitter=0.1, origin_offset=True, elastic=elastic,
                  color_noise=0.02, seed=1)
    empty = {"bbox3d": torch.zeros((0, 7)), "labels": torch.zeros((0,), dtype=torch.int64)}
    scale, full = cfg.SPARSE3D.VOXEL_SCALE, cfg.SPARSE3D.VOXEL_FULL_SCALE

    def plain():
        for x in clouds:
            voxelize(x, scale, full)

    def augmented():
        for x in clouds:
            aug(x, empty, cfg)

    for _ in range(warm):
        plain()
        augmented()
    tp, ta = [], []
    for _ in range(calls):
        tp.append(_timed(plain))
        ta.append(_timed(augmented))
    return statistics.median(tp), statistics.median(ta)


def probe_train(cfg, dev, steps, augment):
    from detection_3d_amd import engine
    from detection_3d_amd.detector import build_detection_model
    from detection_3d_amd.synthetic import write_scene_file
    d = tempfile.mkdtemp(prefix="d3d_aug_probe_")
    files = [write_scene_file(os.path.join(d, f"s{i}.npz"), i, 500_000, cfg.INPUT.CLASSES) for i in range(4)]
    torch.manual_seed(0)
    model = build_detection_model(cfg).to(dev)
    return engine.train(model, cfg, files, dev, steps=steps, augment=augment)["ms_per_step"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--train-steps", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from detection_3d_amd import _lib
    from detection_3d_amd.augment import Augment
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.synthetic import make_scene
    _lib.lib()
    dev = torch.device("cuda:0")
    cfg = get_cfg("6c_Fpn4321")
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    cases = [("500k_25x19m", [make_scene(0, 500_000)]),
             ("500k_50x50m", [make_scene(1, 500_000, extent=(50.0, 50.0, 2.7))]),
             ("4x1M_25x19m", [make_scene(2 + i, 1_000_000) for i in range(4)])]
    for name, clouds in cases:
        xs = [torch.from_numpy(c).to(dev) for c in clouds]
        for elastic in (False, True):
            tp, ta = probe_calls(cfg, dev, xs, elastic, args.calls)
            emit({"case": name, "elastic": elastic, "voxelize_ms": round(tp, 4), "augment_ms": round(ta, 4),
                  "ratio": round(ta / tp, 3), "calls": args.calls})
        del xs
    base = probe_train(cfg, dev, args.train_steps, None)
    aug = Augment(rotate="quarter", flip_x=True, scale_jitter=0.1, origin_offset=True, elastic=True, color_noise=0.02)
    on = probe_train(cfg, dev, args.train_steps, aug)
    emit({"case": "train_6c_500k", "augment_none_ms_per_step": round(base, 3), "augment_all_ms_per_step": round(on, 3),
          "steps": args.train_steps})
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
