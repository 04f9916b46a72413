"""Cost of segmenting a cloud into planar patches on the GPU (detection_3d_amd.planes), beside connected_components on the
same cloud and radius (the same walk with the cheaper edge: the difference is the price of the normals) and beside the
scipy restatement on the CPU of the same machine.

    python scripts/planes_probe.py [--reps 20] [--warm 3] [--cpu] [--out FILE]

Two clouds of the synthetic 25 x 19 m building, down-sampled to one point per 2 cm voxel and capped to 500 k and to 1 M
points; their normal columns are the voxel means of the synthetic normals.  Per cloud: segment_planes and
connected_components timed with events around the call (median, min, max, interquartile range over `reps` rounds after
`warm` warm calls) and split into phases by the library's own events; fit_planes whole, its two library phases and the
share of the point lists (torch's stable sort and what goes with it); label_planes whole.  --cpu runs the restatement
once on the first cloud: cKDTree.query_pairs (scipy has no threaded pair search; one thread), the three edge tests in
numpy and scipy.sparse.csgraph.connected_components.  One JSON line per result."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RADIUS, ANGLE, OFFSET, MIN_POINTS = 0.1, 10.0, 0.02, 100


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


def cpu_planes(p, nr):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    pairs = cKDTree(p).query_pairs(RADIUS, output_type="ndarray")
    t1 = time.perf_counter()
    a, b = pairs[:, 0], pairs[:, 1]
    d = p[b] - p[a]
    c = np.abs(np.einsum("ij,ij->i", nr[a], nr[b]))
    e = np.maximum(np.abs(np.einsum("ij,ij->i", nr[a], d)), np.abs(np.einsum("ij,ij->i", nr[b], d)))
    sel = (c >= math.cos(math.radians(ANGLE))) & (e <= OFFSET)
    n = p.shape[0]
    g = coo_matrix((np.ones(int(sel.sum()), np.int8), (a[sel], b[sel])), shape=(n, n))
    count, comp = connected_components(g, directed=False)
    t2 = time.perf_counter()
    return {"pairs": int(pairs.shape[0]), "edges": int(sel.sum()), "patches": int(count), "pair_search_s": round(t1 - t0, 3),
            "seconds": round(t2 - t0, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--sizes", default="500000,1000000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from detection_3d_amd import _lib
    from detection_3d_amd.clean import connected_components
    from detection_3d_amd.downsample import prepare_cloud
    from detection_3d_amd.planes import _plane_lists, fit_planes, label_planes, segment_planes
    from detection_3d_amd.synthetic import make_scene
    _lib.lib()
    dev = torch.device("cuda:0")
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    def measure(name, what, fn, phased=None):
        for _ in range(args.warm):
            fn()
        ts = [_timed(fn) for _ in range(args.reps)]
        emit({"case": name, "what": what, "reps": args.reps, **_spread(ts)})
        if phased is not None:
            ph = [phased() for _ in range(args.reps)]
            emit({"case": name, "what": what + "_phases_median_ms",
                  **{key: round(statistics.median(p[key] for p in ph), 4) for key in ph[0]}})
        return statistics.median(ts)

    emit({"library": _lib.LIB_PATH})
    raw = torch.from_numpy(make_scene(0, 4_000_000)).to(dev)
    for i, cap in enumerate(int(v) for v in args.sizes.split(",")):
        pcl = prepare_cloud(raw, voxel=0.02, max_points=cap)
        xyz, nrm = pcl[:, :3], pcl[:, 6:9].contiguous()
        n = pcl.shape[0]
        name = f"{n // 1000}k"
        label, size = segment_planes(xyz, nrm, RADIUS, ANGLE, OFFSET)
        planes = fit_planes(xyz, label, size, MIN_POINTS)
        heads = label == torch.arange(n, dtype=torch.int32, device=dev)
        emit({"case": name, "points": n, "radius": RADIUS, "angle": ANGLE, "offset": OFFSET, "patches": int(heads.sum()),
              "planes": int(planes.normal.shape[0]), "largest": int(size.max()),
              "points_in_planes": int((planes.plane_of_point >= 0).sum()),
              "components": int((connected_components(xyz, RADIUS)[0] == torch.arange(n, dtype=torch.int32, device=dev)).sum())})
        seg = measure(name, "segment_planes", lambda: segment_planes(xyz, nrm, RADIUS, ANGLE, OFFSET),
                      lambda: segment_planes(xyz, nrm, RADIUS, ANGLE, OFFSET, phases=True)[-1])
        measure(name, "connected_components", lambda: connected_components(xyz, RADIUS),
                lambda: connected_components(xyz, RADIUS, phases=True)[-1])
        measure(name, "fit_planes", lambda: fit_planes(xyz, label, size, MIN_POINTS),
                lambda: fit_planes(xyz, label, size, MIN_POINTS, phases=True)[-1])
        measure(name, "fit_planes_point_lists", lambda: _plane_lists(label, size, MIN_POINTS))
        measure(name, "label_planes", lambda: label_planes(pcl, None, RADIUS, ANGLE, OFFSET, MIN_POINTS))
        if args.cpu and i == 0:
            r = cpu_planes(xyz.cpu().numpy().astype(np.float64), nrm.cpu().numpy().astype(np.float64))
            emit({"case": name, "what": "cpu_segment_planes", **r, "ratio_to_gpu": round(r["seconds"] * 1e3 / seg, 1)})
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
