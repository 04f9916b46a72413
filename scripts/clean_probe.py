"""Cost of cleaning a cloud on the GPU (detection_3d_amd.clean), beside the same filters on the CPU of the same machine.

    python scripts/clean_probe.py [--reps 20] [--warm 3] [--no-cpu] [--out FILE]

Two clouds of the synthetic 25 x 19 m building: the raw one of 2 M points, and its down-sampled form (one point per 2 cm
voxel, capped to 500 k).  Per cloud: every filter alone (radius_outliers, statistical_outliers, connected_components) and
clean_cloud with all three, timed with events around the call (median, min, max, interquartile range over `reps` rounds
after `warm` warm calls), and the library's own events split each filter into its phases (cell coordinates, sorts, cell
table, search, tail: the statistics and the keep mask, or the flatten and label passes).  The CPU side runs the same
filters once with scipy.spatial.cKDTree (workers=16) and scipy.sparse.csgraph.connected_components and the ratio to the
GPU median is reported.  One JSON line per result."""
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

RADIUS, MIN_NEIGHBORS, STATISTICAL, MIN_COMPONENT = 0.1, 8, (20, 2.0), 0.01


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


def cpu_radius(p, workers=16):
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    count = cKDTree(p).query_ball_point(p, RADIUS, workers=workers, return_length=True)
    keep = count >= MIN_NEIGHBORS
    return time.perf_counter() - t0, int(keep.sum())


def cpu_statistical(p, workers=16):
    from scipy.spatial import cKDTree
    k, ratio = STATISTICAL
    t0 = time.perf_counter()
    d, _ = cKDTree(p).query(p, k=k + 1, distance_upper_bound=RADIUS, workers=workers)
    full = np.isfinite(d[:, k])
    mean = d[full].sum(1) / k
    keep = mean <= mean.mean() + ratio * mean.std(ddof=1)
    return time.perf_counter() - t0, int(keep.sum())


def cpu_components(p):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    pairs = cKDTree(p).query_pairs(RADIUS, output_type="ndarray")
    n = p.shape[0]
    g = coo_matrix((np.ones(pairs.shape[0], np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    _, comp = connected_components(g, directed=False)
    keep = np.bincount(comp)[comp] >= MIN_COMPONENT * n
    return time.perf_counter() - t0, int(keep.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from detection_3d_amd import _lib
    from detection_3d_amd.clean import (clean_cloud, connected_components, knn_mean_distance, radius_neighbors,
                                        radius_outliers, statistical_outliers)
    from detection_3d_amd.downsample import prepare_cloud
    from detection_3d_amd.synthetic import make_scene
    _lib.lib()
    dev = torch.device("cuda:0")
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    raw = torch.from_numpy(make_scene(0, 2_000_000)).to(dev)
    clouds = (("500k_downsampled", prepare_cloud(raw, voxel=0.02, max_points=500_000)), ("2M_raw", raw))
    k, ratio = STATISTICAL
    for name, pcl in clouds:
        xyz = pcl[:, :3]
        n = pcl.shape[0]
        calls = {
            "radius_outliers": lambda: radius_outliers(xyz, RADIUS, MIN_NEIGHBORS),
            "statistical_outliers": lambda: statistical_outliers(xyz, k, ratio, RADIUS),
            "connected_components": lambda: connected_components(xyz, RADIUS),
            "clean_cloud_all_three": lambda: clean_cloud(pcl, RADIUS, MIN_NEIGHBORS, STATISTICAL, MIN_COMPONENT),
        }
        phased = {
            "radius_outliers": lambda: radius_neighbors(xyz, RADIUS, phases=True)[-1],
            "statistical_outliers": lambda: knn_mean_distance(xyz, k, ratio, RADIUS, phases=True)[-1],
            "connected_components": lambda: connected_components(xyz, RADIUS, phases=True)[-1],
        }
        count = radius_neighbors(xyz, RADIUS)
        kept = clean_cloud(pcl, RADIUS, MIN_NEIGHBORS, STATISTICAL, MIN_COMPONENT).shape[0]
        emit({"case": name, "points": n, "radius": RADIUS, "median_count": float(count.float().median()),
              "max_count": int(count.max()), "kept_by_all_three": kept})
        gpu_ms = {}
        for what, fn in calls.items():
            for _ in range(args.warm):
                fn()
            ts = [_timed(fn) for _ in range(args.reps)]
            gpu_ms[what] = statistics.median(ts)
            emit({"case": name, "what": what, "reps": args.reps, **_spread(ts)})
            if what in phased:
                ph = [phased[what]() for _ in range(args.reps)]
                emit({"case": name, "what": what + "_phases_median_ms",
                      **{key: round(statistics.median(p[key] for p in ph), 4) for key in ph[0]}})
        if not args.no_cpu:
            p = xyz.cpu().numpy().astype(np.float64)
            for what, fn in (("radius_outliers", cpu_radius), ("statistical_outliers", cpu_statistical),
                             ("connected_components", cpu_components)):
                sec, cpu_kept = fn(p)
                emit({"case": name, "what": "cpu_" + what, "seconds": round(sec, 3), "kept": cpu_kept,
                      "ratio_to_gpu": round(sec * 1e3 / gpu_ms[what], 1)})
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
