"""Cost of estimating point normals on the GPU (detection_3d_amd.normals) on the synthetic buildings, beside
d3d_voxelize on the same cloud, the full building pass, and a CPU reference for context.

    python scripts/normals_probe.py [--reps 30] [--warm 5] [--no-cpu] [--no-pass] [--out FILE]

Per cloud (500 k and 1 M points of the 25 x 19 m building, radius 0.1 m, max_nn 50): warm calls, then `reps` rounds that
each time one estimate_normals and one voxelize with events, interleaved so that clocks and caches drift alike; median,
min, max and the interquartile range are reported.  The library's own events split a call into its phases (cell
coordinates, sort, cell table, search).  The building pass is voxelize + the 6c detector in eval mode, timed the same
way.  The CPU reference is the k-d tree query plus batched numpy.linalg.eigh on at most 16 threads, once.  One JSON line
per result."""
import argparse
import json
import os
import statistics
import sys
import time

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


def _spread(ts):
    q = statistics.quantiles(ts, n=4)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "iqr_ms": round(q[2] - q[0], 4)}


def cpu_reference(xyz, radius, max_nn, workers=16):
    """k-d tree neighbours within `radius`, the `max_nn` nearest of them, batched eigh -> (seconds, median count)"""
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    p = xyz.astype(np.float64)
    d, j = cKDTree(p).query(p, k=max_nn, distance_upper_bound=radius, workers=workers)
    ok = np.isfinite(d)
    q = np.where(ok[..., None], p[np.minimum(j, p.shape[0] - 1)] - p[:, None, :], 0.0)
    m = ok.sum(1)
    mean = q.sum(1) / m[:, None]
    c = np.einsum("nki,nkj->nij", q, q) / m[:, None, None] - mean[:, :, None] * mean[:, None, :]
    np.linalg.eigh(c)
    return time.perf_counter() - t0, float(np.median(m))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--radius", type=float, default=0.1)
    ap.add_argument("--max-nn", type=int, default=50)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-pass", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from detection_3d_amd import _lib
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.normals import estimate_normals, estimate_normals_phases
    from detection_3d_amd.synthetic import make_scene
    from detection_3d_amd.voxelize import voxelize
    _lib.lib()
    dev = torch.device("cuda:0")
    cfg = get_cfg("6c_Fpn4321")
    scale, full = cfg.SPARSE3D.VOXEL_SCALE, cfg.SPARSE3D.VOXEL_FULL_SCALE
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    model = None
    if not args.no_pass:
        from detection_3d_amd.detector import build_detection_model
        torch.manual_seed(0)
        model = build_detection_model(cfg).to(dev).eval()
    for name, n_points in (("500k_25x19m", 500_000), ("1M_25x19m", 1_000_000)):
        host = make_scene(0, n_points)
        pcl = torch.from_numpy(host).to(dev)
        xyz = pcl[:, :3]

        def est():
            estimate_normals(xyz, args.radius, args.max_nn)

        def vox():
            voxelize(pcl, scale, full)

        def building():
            with torch.no_grad():
                c, f = voxelize(pcl, scale, full)
                model([c, f])

        for _ in range(args.warm):
            est()
            vox()
        te, tv = [], []
        for _ in range(args.reps):
            te.append(_timed(est))
            tv.append(_timed(vox))
        _, counts = estimate_normals(xyz, args.radius, args.max_nn, return_counts=True)
        counts = counts.cpu().numpy()
        emit({"case": name, "what": "estimate_normals", "reps": args.reps, "radius": args.radius, "max_nn": args.max_nn,
              "median_count": float(np.median(counts)), "capped_share": round(float((counts == args.max_nn).mean()), 4),
              **_spread(te)})
        emit({"case": name, "what": "voxelize", "reps": args.reps, **_spread(tv)})
        xyz_c = xyz.contiguous()
        ph = [estimate_normals_phases(xyz_c, args.radius, args.max_nn)[1] for _ in range(args.reps)]
        emit({"case": name, "what": "phases_median_ms",
              **{k: round(statistics.median(p[k] for p in ph), 4) for k in ("cells", "sort", "table", "search")}})
        if model is not None:
            for _ in range(args.warm):
                building()
            emit({"case": name, "what": "building_pass_6c", "reps": args.reps,
                  **_spread([_timed(building) for _ in range(args.reps)])})
        if not args.no_cpu:
            sec, med = cpu_reference(host[:, :3], args.radius, args.max_nn)
            emit({"case": name, "what": "cpu_kdtree_eigh_16_threads", "seconds": round(sec, 3), "median_count": med})
        del pcl, xyz, xyz_c
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
