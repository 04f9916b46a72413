"""Inference at torch's default fp32 matmul precision against 'tf32' (the sparse convolutions as bf16x3, D3D_F32_X3).

On a seeded 4c scene (500 k points by default) it alternates N passes of each mode and reports, as one JSON line:
  - the median ms per pass (voxelize + detector) of each mode;
  - the largest relative difference (max |a - b| / max |b|) over the backbone maps, and per map;
  - how the detections agree: counts, and the 3-D IoU of each default detection's best same-label match.
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` with --mode to select one mode:
    python scripts/precision_probe.py --passes 20                       (timing + agreement)
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/precision_probe.py --passes 10 --mode tf32
--layers replays every sparse convolution of one pass on its own (same rows, rulebooks and fused BatchNorm), both
modes alternated, and prints a JSON line per launch (Cin, Cout, filter volume, output rows, median us per mode):
inside a pass the launches overlap the geometry stream's kernels, which blurs per-launch kernel times.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def set_mode(mode):
    # the legacy call sets both of torch's APIs; the new one alone leaves them disagreeing on torch 2.10, and torch's
    # own matmuls then raise
    torch.set_float32_matmul_precision("high" if mode == "tf32" else "highest")


def flatten(maps):
    out = []
    for m in maps:
        if isinstance(m, (list, tuple)):
            out += flatten(m)
        elif m is not None and hasattr(m, "features"):
            out.append(m)
    return out


def agreement(r0, r3):
    import oracle
    d0 = r0[0] if isinstance(r0, (list, tuple)) else r0
    d3 = r3[0] if isinstance(r3, (list, tuple)) else r3
    b0, l0 = d0["bbox3d"].cpu().numpy(), d0["labels"].cpu().numpy()
    b3, l3 = d3["bbox3d"].cpu().numpy(), d3["labels"].cpu().numpy()
    ious = []
    for lab in np.unique(l0):
        p, q = b0[l0 == lab], b3[l3 == lab]
        if len(p) and len(q):
            ious += list(np.asarray(oracle.boxes_iou_3d(q, p)).reshape(len(q), len(p)).max(0))
        else:
            ious += [0.0] * len(p)
    return {"n_default": int(len(b0)), "n_tf32": int(len(b3)), "matched_iou_min": float(min(ious, default=1.0)),
            "matched_iou_median": float(np.median(ious)) if ious else 1.0,
            "matched_above_0.9": int(sum(i > 0.9 for i in ious))}


def replay_layers(model, pcl, cfg, reps=10):
    from detection_3d_amd.sparseconvnet import SCN
    from detection_3d_amd.voxelize import voxelize
    names = ("SubmanifoldConvolution_updateOutput", "Convolution_updateOutput", "Deconvolution_updateOutput")
    calls, orig = [], {n: getattr(SCN, n) for n in names}

    def recorder(n):
        def f(*args, **kw):
            calls.append((n, args, kw))
            return orig[n](*args, **kw)
        return f
    for n in names:
        setattr(SCN, n, recorder(n))
    try:
        set_mode("default")
        coords, feats = voxelize(pcl, cfg.SPARSE3D.VOXEL_SCALE, cfg.SPARSE3D.VOXEL_FULL_SCALE)
        maps = model.backbone([coords, feats])
        torch.cuda.synchronize()
    finally:
        for n in names:
            setattr(SCN, n, orig[n])
    rows = []
    for n, args, kw in calls:
        i = 3 if n == "SubmanifoldConvolution_updateOutput" else 5      # (input, output, weight) positions
        feats_in, out, weight = args[i], args[i + 1], args[i + 2]
        packed = {}
        for m in ("default", "tf32"):
            set_mode(m)
            packed[m] = SCN.pack_weight(weight, feats_in.dtype)
        times = {"default": [], "tf32": []}
        for r in range(reps + 1):
            for m in ("default", "tf32"):
                set_mode(m)
                k = dict(kw, packed=packed[m])
                if isinstance(kw.get("stats"), list):
                    k["stats"] = []
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                orig[n](*args, **k)
                e1.record()
                e1.synchronize()
                if r:
                    times[m].append(1e3 * e0.elapsed_time(e1))
        fv, _, cin, cout = weight.shape
        rows.append({"kind": n.split("_")[0], "cin": int(cin), "cout": int(cout), "fv": int(fv),
                     "rows_in": int(feats_in.shape[0]), "rows_out": int(out.shape[0]),
                     "us": {m: float(np.median(v)) for m, v in times.items()}})
    del maps
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=500000)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", choices=["both", "default", "tf32"], default="both")
    ap.add_argument("--layers", action="store_true", help="replay each convolution of one pass alone, both modes")
    args = ap.parse_args()
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.detector import build_detection_model
    from detection_3d_amd.synthetic import make_scene
    from detection_3d_amd.voxelize import voxelize
    dev = torch.device("cuda:0")
    cfg = get_cfg("4c_Fpn432")
    torch.manual_seed(0)
    model = build_detection_model(cfg).to(dev).eval()
    pcl = torch.from_numpy(make_scene(0, args.points)).to(dev)
    modes = ["default", "tf32"] if args.mode == "both" else [args.mode]
    was = torch.get_float32_matmul_precision()

    def one_pass():
        coords, feats = voxelize(pcl, cfg.SPARSE3D.VOXEL_SCALE, cfg.SPARSE3D.VOXEL_FULL_SCALE)
        return model([coords, feats])

    if args.layers:
        try:
            with torch.no_grad():
                set_mode("default")
                one_pass()                                # warm-up: code objects, allocator, rulebook paths
                for r in replay_layers(model, pcl, cfg):
                    print(json.dumps(r), flush=True)
        finally:
            torch.set_float32_matmul_precision(was)
        return
    times = {m: [] for m in modes}
    try:
        with torch.no_grad():
            for it in range(args.warmup + args.passes):
                for m in modes:                           # the modes alternate pass by pass
                    set_mode(m)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    one_pass()
                    torch.cuda.synchronize()
                    if it >= args.warmup:
                        times[m].append(1e3 * (time.perf_counter() - t0))
            out = {"points": args.points, "passes": args.passes,
                   "ms_median": {m: float(np.median(v)) for m, v in times.items()},
                   "ms_spread": {m: [float(np.percentile(v, 10)), float(np.percentile(v, 90))] for m, v in times.items()}}
            if len(modes) == 2:
                maps, res = {}, {}
                for m in modes:
                    set_mode(m)
                    coords, feats = voxelize(pcl, cfg.SPARSE3D.VOXEL_SCALE, cfg.SPARSE3D.VOXEL_FULL_SCALE)
                    maps[m] = flatten(model.backbone([coords, feats]))
                    res[m] = model([coords, feats])
                rel = [float((a.features - b.features).abs().max()) / max(float(b.features.abs().max()), 1e-30)
                       for a, b in zip(maps["tf32"], maps["default"])]
                out["maps"] = len(rel)
                out["map_rel_diff"] = rel
                out["map_rel_diff_max"] = max(rel)
                out["detections"] = agreement(res["default"], res["tf32"])
    finally:
        torch.set_float32_matmul_precision(was)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
