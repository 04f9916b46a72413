"""A labelled scan -> an ordinary scene file: fits the box of every instance on the GPU (primitives.targets_from_labels)
and writes the cloud with those boxes as scene_io.save_scene does, so that load_scene, ScenePrefetcher and
scripts/train_ddp.py read it like any other scene.

    python scripts/label_scene.py labelled.npz scene.npz --config 6c_Fpn4321 [--min-points 10] [--min-size 0.05,0.05,0.1]

    python scripts/label_scene.py unlabelled.npz scene.npz --planes[=RADIUS,ANGLE,OFFSET,MIN_POINTS]

The input is an .npz without pickled members: `pcl` float32 [N, >= 3], `instance` an integer id in [0, K) per row
(negative: none), `instance_class` a string array [K] with the class name of every instance.  Instances of a class the
config does not list are left out.

--planes is for a scan nobody labelled: `pcl` float32 [N, 9] with normals in columns 6:9 and no `instance`.  The
instances are then the planar patches of planes.label_planes (region growing over the normals on the GPU; defaults
0.1 m, 10 degrees, 0.02 m, 100 points), classed floor, ceiling or wall by their fitted normal.

--align[=MAX_TILT,TOL] (degrees, defaults 30 and 5) is for a scan that is not level or not square to its walls: the
cloud (`pcl` [N, 9]) is first turned into its Manhattan frame by its normals (frame.align_cloud), so that --planes
classes by the angle to the true vertical and the boxes are upright; the scene file holds the aligned cloud.

--rooms[=CELL,MIN_AREA] (metres and square metres, defaults 0.05 and 1.0) is for a config that lists the class `room`:
a labelled scan has no room nodes, so one room box per room of the floor plan between the fitted walls, windows and
doors is appended (floorplan.room_targets; z from the walls).  Nothing is added when the scan labels rooms itself."""
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
    ap.add_argument("--planes", nargs="?", const="", default=None, metavar="RADIUS,ANGLE,OFFSET,MIN_POINTS",
                    help="no `instance` in the input: label the planar patches of the cloud (planes.label_planes)")
    ap.add_argument("--align", nargs="?", const="", default=None, metavar="MAX_TILT,TOL",
                    help="level the cloud and square it to its walls by its normals first (frame.align_cloud)")
    ap.add_argument("--rooms", nargs="?", const="", default=None, metavar="CELL,MIN_AREA",
                    help="append one `room` box per room of the floor plan between the fitted walls (floorplan.room_targets)")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    from detection_3d_amd.config import class_to_label, get_cfg
    from detection_3d_amd.floorplan import parse_rooms, room_targets
    from detection_3d_amd.frame import align_cloud, parse_align
    from detection_3d_amd.planes import label_planes, parse_planes
    from detection_3d_amd.primitives import MIN_POINTS_ANY, targets_from_labels
    from detection_3d_amd.scene_io import save_scene, yx_zb_to_standard
    cfg = get_cfg(args.config)
    try:
        planes = parse_planes(args.planes)
        align = parse_align(args.align)
        rooms = parse_rooms(args.rooms)
    except ValueError as e:
        raise SystemExit(str(e))
    with np.load(args.labelled, allow_pickle=False) as d:
        pcl = np.ascontiguousarray(d["pcl"], dtype=np.float32)
        if planes is not None and "instance" in d.files:
            raise SystemExit("--planes is for an input without `instance`; this one carries its own labels")
        instance = None if planes is not None else np.asarray(d["instance"])
        names = None if planes is not None else [str(n) for n in d["instance_class"]]
    c2l = class_to_label(cfg.INPUT.CLASSES)
    l2c = {l: c for c, l in c2l.items()}
    dev = torch.device(args.device)
    cloud = torch.from_numpy(pcl).to(dev)
    if align is not None:
        if pcl.ndim != 2 or pcl.shape[1] != 9:
            raise SystemExit(f"--align reads the normals from columns 6:9, pcl is {pcl.shape}")
        cloud, frame = align_cloud(cloud, **align)
        pcl = cloud.cpu().numpy()
        print(f"aligned: {frame!r}")
    if planes is not None:
        if pcl.ndim != 2 or pcl.shape[1] < 9:
            raise SystemExit(f"--planes reads the normals from columns 6:9, pcl is {pcl.shape}")
        found = label_planes(cloud, classes=cfg.INPUT.CLASSES, **planes)
        inst, labels = found["instance"], found["instance_labels"]
    else:
        if instance.dtype.kind not in "iu" or instance.shape != (pcl.shape[0],):
            raise SystemExit(f"instance must be an integer array [{pcl.shape[0]}], got {instance.dtype} {instance.shape}")
        inst = torch.from_numpy(instance.astype(np.int64)).to(dev)
        labels = torch.tensor([c2l.get(n, 0) for n in names], dtype=torch.int64)
    tg = targets_from_labels(cloud, inst, labels,
                             min_points=MIN_POINTS_ANY if args.min_points is None else args.min_points,
                             min_size=[float(v) for v in args.min_size.split(",")], classes=cfg.INPUT.CLASSES)
    if rooms is not None:
        if "room" not in c2l:
            raise SystemExit(f"--rooms: the config {args.config} does not list the class `room`")
        tg = room_targets(tg, cfg.INPUT.CLASSES, **rooms)
    boxes, kept = tg["bbox3d"].cpu().numpy(), tg["labels"].cpu().numpy()
    per_class = {l2c[int(l)]: yx_zb_to_standard(boxes[kept == l]) for l in np.unique(kept)}
    save_scene(args.scene, pcl, per_class)
    print(f"{args.scene}: {pcl.shape[0]} points, " + ", ".join(f"{len(v)} {c}" for c, v in per_class.items()))


if __name__ == "__main__":
    main()
