"""A labelled scan -> an ordinary scene file: fits the box of every instance on the GPU (primitives.targets_from_labels)
and writes the cloud with those boxes as scene_io.save_scene does, so that load_scene, ScenePrefetcher and
scripts/train_ddp.py read it like any other scene.

    python scripts/label_scene.py labelled.npz scene.npz --config 6c_Fpn4321 [--min-points 10] [--min-size 0.05,0.05,0.1]

The input is an .npz without pickled members: `pcl` float32 [N, >= 3], `instance` an integer id in [0, K) per row
(negative: none), `instance_class` a string array [K] with the class name of every instance.  Instances of a class the
config does not list are left out."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("labelled")
    ap.add_argument("scene")
    ap.add_argument("--config", default="6c_Fpn4321")
    ap.add_argument("--min-points", type=int, default=None)
    ap.add_argument("--min-size", default="0,0,0", help="D3,D4,DZ in metres: smaller boxes are widened to these")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    from detection_3d_amd.config import class_to_label, get_cfg
    from detection_3d_amd.primitives import MIN_POINTS_ANY, targets_from_labels
    from detection_3d_amd.scene_io import save_scene, yx_zb_to_standard
    cfg = get_cfg(args.config)
    with np.load(args.labelled, allow_pickle=False) as d:
        pcl = np.ascontiguousarray(d["pcl"], dtype=np.float32)
        instance = np.asarray(d["instance"])
        names = [str(n) for n in d["instance_class"]]
    if instance.dtype.kind not in "iu" or instance.shape != (pcl.shape[0],):
        raise SystemExit(f"instance must be an integer array [{pcl.shape[0]}], got {instance.dtype} {instance.shape}")
    c2l = class_to_label(cfg.INPUT.CLASSES)
    l2c = {l: c for c, l in c2l.items()}
    labels = torch.tensor([c2l.get(n, 0) for n in names], dtype=torch.int64)
    dev = torch.device(args.device)
    tg = targets_from_labels(torch.from_numpy(pcl).to(dev), torch.from_numpy(instance.astype(np.int64)).to(dev), labels,
                             min_points=MIN_POINTS_ANY if args.min_points is None else args.min_points,
                             min_size=[float(v) for v in args.min_size.split(",")], classes=cfg.INPUT.CLASSES)
    boxes, kept = tg["bbox3d"].cpu().numpy(), tg["labels"].cpu().numpy()
    per_class = {l2c[int(l)]: yx_zb_to_standard(boxes[kept == l]) for l in np.unique(kept)}
    save_scene(args.scene, pcl, per_class)
    print(f"{args.scene}: {pcl.shape[0]} points, " + ", ".join(f"{len(v)} {c}" for c, v in per_class.items()))


if __name__ == "__main__":
    main()
