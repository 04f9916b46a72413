"""Cost of detection_3d_amd.register on the GPU, beside a k-d tree and the numpy step on the CPU of the same machine.

    python scripts/register_probe.py [--sizes 500000,2000000] [--reps 15] [--warm 3] [--no-cpu] [--out FILE]

Per size two scans of the synthetic building's mesh through render.scan_mesh, from two sets of cameras (two stations);
the second one is moved by 0.2 degrees (4 cm at the far walls) and 3 cm about the building's centre and registered to
the first, max_dist 0.1 m, point to plane on the normals scan_mesh delivers.  Timed with events around the call, after `warm` warm calls, median
and quartiles over `reps` rounds; forms that are compared alternate within a round:
  nearest             the whole call, and its phases from the library's own events (cells, sort, table, search);
  nearest_shuffled    the same queries in a random order: what the scan order's locality is worth to the search;
  radius_neighbors    clean.radius_neighbors on the target: its search phase is the sorted self-walk with staged cells,
                      an upper mark for what sorting the queries could give (per query, it also counts every neighbour);
  icp_1               one step by phase (transform, nearest, accumulate, solve);
  icp_30              icp(iterations=30, tol=1e-6) as a user calls it, and with tol=0 so that all 30 steps execute;
  cpu                 cKDTree(target) build, query(k=1, distance_upper_bound, workers=16) and the numpy normal equations
                      and solve of one step, once.
One JSON line per result."""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

MAX_DIST = 0.1


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _spread(ts):
    q = statistics.quantiles(ts, n=4)
    return {"median_ms": round(statistics.median(ts), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4),
            "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def _median_phases(ph):
    return {key: round(statistics.median(p[key] for p in ph), 4) for key in ph[0]}


def motion(centre, degrees, shift):
    a = np.array([0.1, -0.2, 1.0]) / np.linalg.norm([0.1, -0.2, 1.0])
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    t = math.radians(degrees)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)
    T[:3, 3] = centre - T[:3, :3] @ centre + np.asarray(shift)
    return T


def cpu_step(src, tgt, nrm, workers=16):
    """one point-to-plane step from the identity on the host -> seconds of (tree build, query, normal equations + solve)"""
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    tree = cKDTree(tgt)
    t1 = time.perf_counter()
    d, j = tree.query(src, k=1, distance_upper_bound=MAX_DIST, workers=workers)
    t2 = time.perf_counter()
    ok = np.isfinite(d)
    p, q, n = src[ok].astype(np.float64), tgt[j[ok]].astype(np.float64), nrm[j[ok]].astype(np.float64)
    r = ((p - q) * n).sum(1)
    J = np.concatenate([np.cross(p, n), n], 1)
    x = np.linalg.solve(J.T @ J, -(J.T @ r))
    t3 = time.perf_counter()
    return t1 - t0, t2 - t1, t3 - t2, int(ok.sum()), float(np.linalg.norm(x[:3])), float(np.linalg.norm(x[3:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500000,2000000")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from render_probe import make_cameras, make_mesh
    from detection_3d_amd import _lib
    from detection_3d_amd.clean import radius_neighbors
    from detection_3d_amd.register import apply_pose, icp, inverse_pose, nearest
    from detection_3d_amd.render import scan_mesh
    _lib.lib()
    dev = torch.device("cuda:0")
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    mesh, lo, hi = make_mesh(0, dev)
    centre = 0.5 * (lo + hi)
    for size in (int(s) for s in args.sizes.split(",")):
        voxel = 0.02 if size <= 500_000 else 0.01
        scans = []
        for seed in (0, 1):
            intr, extr = make_cameras(args.frames, args.image, lo, hi, seed)
            scans.append(scan_mesh(mesh, intr, extr, args.image, args.image, voxel=voxel, max_points=size, seed=seed))
        target = scans[0]
        truth = motion(centre, 0.2, (0.02, -0.02, 0.01))
        source = apply_pose(scans[1], inverse_pose(torch.from_numpy(truth)))
        case = f"{size // 1000}k"
        n, m = target.shape[0], source.shape[0]
        q, c = source[:, :3], target[:, :3]
        shuffled = q[torch.randperm(m, device=dev, generator=torch.Generator(dev).manual_seed(0))].contiguous()
        index = nearest(q, c, MAX_DIST)
        emit({"case": case, "target_points": n, "source_points": m, "voxel": voxel, "max_dist": MAX_DIST,
              "paired_at_start": int((index >= 0).sum())})
        forms = {"nearest": lambda: nearest(q, c, MAX_DIST), "nearest_shuffled": lambda: nearest(shuffled, c, MAX_DIST),
                 "radius_neighbors": lambda: radius_neighbors(c, MAX_DIST)}
        phased = {"nearest": lambda: nearest(q, c, MAX_DIST, phases=True)[-1],
                  "nearest_shuffled": lambda: nearest(shuffled, c, MAX_DIST, phases=True)[-1],
                  "radius_neighbors": lambda: radius_neighbors(c, MAX_DIST, phases=True)[-1]}
        for fn in forms.values():
            for _ in range(args.warm):
                fn()
        ts, ph = {k: [] for k in forms}, {k: [] for k in forms}
        for _ in range(args.reps):                       # the forms alternate within a round
            for k, fn in forms.items():
                ts[k].append(_timed(fn))
            for k, fn in phased.items():
                ph[k].append(fn())
        for k in forms:
            med = _median_phases(ph[k])
            emit({"case": case, "what": k, "reps": args.reps, **_spread(ts[k])})
            emit({"case": case, "what": k + "_phases_median_ms", **med,
                  "search_ns_per_query": round(med["search"] * 1e6 / (n if k == "radius_neighbors" else m), 2)})
        for _ in range(args.warm):
            icp(source, target, max_dist=MAX_DIST, iterations=1)
        one = [icp(source, target, max_dist=MAX_DIST, iterations=1, phases=True).phases for _ in range(args.reps)]
        emit({"case": case, "what": "icp_1_phases_median_ms", **_median_phases(one)})
        for what, tol in (("icp_30", 1e-6), ("icp_30_all_steps", 0.0)):
            call = lambda: icp(source, target, max_dist=MAX_DIST, iterations=30, tol=tol)
            for _ in range(args.warm):
                call()
            t = [_timed(call) for _ in range(args.reps)]
            reg = call()
            pose = reg.pose.cpu().numpy()
            dR = pose[:3, :3] @ truth[:3, :3].T
            emit({"case": case, "what": what, "reps": args.reps, **_spread(t), "steps": reg.steps, "status": reg.status,
                  "pairs": reg.inliers, "rmse_m": round(reg.rmse, 6),
                  "rotation_error_rad": float(math.acos(max(-1.0, min(1.0, 0.5 * (np.trace(dR) - 1.0))))),
                  "centre_error_m": float(np.linalg.norm(pose[:3, :3] @ centre + pose[:3, 3] - (truth[:3, :3] @ centre + truth[:3, 3])))})
        if not args.no_cpu:
            build, query, solve, pairs, wn, vn = cpu_step(q.cpu().numpy(), c.contiguous().cpu().numpy(),
                                                          target[:, 6:9].contiguous().cpu().numpy())
            gpu = statistics.median(ts["nearest"])
            emit({"case": case, "what": "cpu_step", "tree_build_s": round(build, 3), "query_s": round(query, 3),
                  "equations_and_solve_s": round(solve, 3), "pairs": pairs, "w": wn, "v": vn,
                  "build_and_query_over_gpu_nearest": round((build + query) * 1e3 / gpu, 1),
                  "query_over_gpu_nearest": round(query * 1e3 / gpu, 1)})
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
