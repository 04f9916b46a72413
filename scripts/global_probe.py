"""Cost of register.global_align (d3d_global_align) against the numpy restatement of tests/global_ref.py on the host.

    python scripts/global_probe.py [--sizes 500000,2000000] [--reps 15] [--warm 3] [--no-cpu] [--out FILE]

Per size two scans of the synthetic building's mesh through render.scan_mesh, from two sets of cameras (two stations);
the second one is delivered a quarter turn, 0.3 degrees and metres away from the first, without a pose.  Timed with events
around the call after `warm` warm calls, median and quartiles over `reps` rounds; the forms alternate within a round:
  global_align      the whole call: the normals' frames (align_cloud twice), cloud_min twice, d3d_global_align, the pose;
  lattice_align     d3d_global_align alone on the levelled clouds, and its phases from the library's own events (rows,
                    cells, correlate, peaks, verify, pick);
  probes_per_s      the verification's bitmap probes, valid candidates x listed source cells, over its phase;
  numpy             the restatement on the host for the same levelled clouds, once, with whether every output equals the
                    kernel's bits, and the ratio to lattice_align;
  coarse, icp_after the pose found against the truth (rotation angle, distance at the building's centre), and where icp
                    ends from it, in how many steps; icp_from_truth: where icp ends when it starts at the truth, the
                    floor that the two stations' different samples set.
One JSON line per row."""
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
    from detection_3d_amd.frame import align_cloud
    from detection_3d_amd.primitives import cloud_min
    from detection_3d_amd.register import GLOBAL_PHASES, apply_pose, global_align, icp, inverse_pose, lattice_align
    from tests import global_ref
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
            scans.append(scan_mesh_of(mesh, intr, extr, args.image, voxel, size, seed))
        target = scans[0]
        a = math.radians(90.3)
        truth = np.eye(4)
        truth[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]
        truth[:3, 3] = [7.5, -12.25, 0.6]
        source = apply_pose(scans[1], inverse_pose(torch.from_numpy(truth)))
        case = f"{size // 1000}k"
        src, _ = align_cloud(source)
        tgt, _ = align_cloud(target)
        o_s, o_t = cloud_min(src), cloud_min(tgt)
        lat = lambda **kw: lattice_align(src, src[:, 6:9], o_s, tgt, tgt[:, 6:9], o_t, **kw)
        forms = {"global_align": lambda: global_align(source, target), "lattice_align": lat}
        for fn in forms.values():
            for _ in range(args.warm):
                fn()
        ts, ph = {k: [] for k in forms}, []
        for _ in range(args.reps):
            for k, fn in forms.items():
                ts[k].append(_timed(fn))
            ph.append(lat(phases=True).phases)
        found = global_align(source, target)
        det = lat(return_details=True)
        counts = [int(v) for v in det.details["cell_count"].cpu()]
        valid = int((det.details["scores"] >= 0).sum())
        phases = {k: round(statistics.median(p[k] for p in ph), 4) for k in GLOBAL_PHASES}
        c = np.asarray(centre, np.float64)
        inv = np.linalg.inv(truth)
        c_src = inv[:3, :3] @ c + inv[:3, 3]

        def errors(pose):
            P = pose.cpu().numpy()
            dR = P[:3, :3] @ truth[:3, :3].T
            return {"rotation_rad": round(math.acos(max(-1.0, min(1.0, 0.5 * (np.trace(dR) - 1.0)))), 7),
                    "centre_m": round(float(np.linalg.norm(P[:3, :3] @ c_src + P[:3, 3] - c)), 5)}

        reg = icp(source, target, init=found.pose, max_dist=0.1, iterations=30)
        best = icp(source, target, init=truth, max_dist=0.1, iterations=30)
        emit({"case": case, "source_points": source.shape[0], "target_points": target.shape[0], "voxel": voxel,
              "alignment": repr(found), "heading_scores": found.heading_scores, "support": found.support.tolist(),
              "source_cells": counts, "valid_candidates": valid,
              "global_align": _spread(ts["global_align"]), "lattice_align": _spread(ts["lattice_align"]),
              "phase_ms": phases,
              "probes_per_s": round(valid * sum(counts) / (phases["verify"] * 1e-3), 0) if phases["verify"] > 0 else None,
              "coarse": errors(found.pose),
              "icp_after": dict(errors(reg.pose), steps=reg.steps, status=reg.status),
              "icp_from_truth": dict(errors(best.pose), steps=best.steps, status=best.status)})
        if not args.no_cpu:
            s, t = src.cpu().numpy(), tgt.cpu().numpy()
            t0 = time.perf_counter()
            ref = global_ref.global_ref(s[:, :3], s[:, 6:9], o_s.cpu().numpy(), t[:, :3], t[:, 6:9], o_t.cpu().numpy())
            host_ms = (time.perf_counter() - t0) * 1e3
            same = all(np.array_equal(det.details[k].cpu().numpy(), ref[k].view(det.details[k].cpu().numpy().dtype))
                       for k in ("hist", "corr", "peak_value", "peak_shift", "scores", "target_bits"))
            same = same and np.array_equal(det.choice.cpu().numpy(), ref["choice"]) and \
                np.array_equal(det.score.cpu().numpy(), ref["score"]) and \
                np.array_equal(det.pose.cpu().numpy().view(np.uint64), ref["pose"].view(np.uint64))
            emit({"case": case, "numpy_ms": round(host_ms, 1), "equal_bits": bool(same),
                  "numpy_over_lattice_align": round(host_ms / statistics.median(ts["lattice_align"]), 1)})
        del scans, source, target, src, tgt
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def scan_mesh_of(mesh, intr, extr, image, voxel, size, seed):
    from detection_3d_amd.render import scan_mesh
    return scan_mesh(mesh, intr, extr, image, image, voxel=voxel, max_points=size, seed=seed)


if __name__ == "__main__":
    main()
