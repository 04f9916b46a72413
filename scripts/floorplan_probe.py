"""Cost of the phases of detection_3d_amd.floorplan (floorplan.hip) on the GPU, each set against the numpy / scipy
restatement of tests/floorplan_ref.py on the host at the same size (run once), with the outputs compared.

    python scripts/floorplan_probe.py [--calls 20] [--case detector|max|all] [--out FILE]

Cases: `detector`, the six-room plan scaled to the detector's 81.92 m lattice at 5 cm (1643 x 1643 cells with the
margin) with its walls cut into 196 boxes; `max`, 4096 x 4096 cells with 4096 random walls.  Both place 500 k points.
Phases: table (box_table, torch), raster (d3d_floorplan_raster alone), rooms (d3d_floorplan_rooms; its own five phases
from one more call with the library's events), sides, points.  Warm calls first, then `calls` timed calls of each phase
between device events; medians are reported.  The labelling's traffic: `bytes_compulsory` is the bitmap read once and
the label map written once; `bytes_moved` counts what its kernels read and write per cell as they are written (the
parents, the per-root word, the flags and the scan on top of that), chains and atomics not counted.  One JSON line per
case."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

# per cell, int32 words: runs (par w), roots (par r, label w, info clear), flags (label r, info r, flag w), scan (r, w,
# r + w), write (label r + w); per bitmap word: runs 1, links 4, roots 1
CELL_WORDS, BITMAP_WORDS = 13, 6


def _median_ms(fn, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def _host(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def detector_case(ref):
    scale = 81.92 / 14.0
    rows = []
    for wl in ref.six_rooms(scale):
        xc, yc, zb, d3, d4, dz, yaw = (float(v) for v in wl)
        n = 28
        for i in range(n):                                   # the wall cut into n boxes along its length (s, c)
            m = (i + 0.5) / n * d4 - d4 / 2
            rows.append([xc + math.sin(yaw) * m, yc + math.cos(yaw) * m, zb, 0.1, d4 / n, dz, yaw])
    return np.array(rows, dtype=np.float32), ((-0.1, -0.1), (1643, 1643)), 6


def max_case(ref):
    rs = np.random.RandomState(1)
    k, ext = 4096, 4096 * 0.05
    a = rs.choice([0.0, math.pi / 2], k) + (rs.rand(k) < 0.2) * rs.uniform(0, math.pi, k)
    rows = np.stack([rs.uniform(2, ext - 2, k), rs.uniform(2, ext - 2, k), np.zeros(k), np.full(k, 0.1), rs.uniform(1, 12, k),
                     np.full(k, 2.5), a], 1)
    return rows.astype(np.float32), ((0.0, 0.0), (4096, 4096)), None


def run_case(name, calls, dev):
    import floorplan_ref as ref
    from detection_3d_amd import floorplan as fp
    from detection_3d_amd._cloud import run
    from detection_3d_amd._lib import ptr, stream_of
    boxes_np, (origin, shape), want_rooms = {"detector": detector_case, "max": max_case}[name](ref)
    cell, grow, lat = 0.05, 0.1, fp.Lattice(origin, shape)
    h, w = shape
    boxes = torch.from_numpy(boxes_np).to(dev)
    k = boxes.shape[0]
    rs = np.random.RandomState(2)
    pts_np = np.stack([rs.uniform(origin[0] - 1, origin[0] + w * cell + 1, 500000),
                       rs.uniform(origin[1] - 1, origin[1] + h * cell + 1, 500000), rs.uniform(0, 3, 500000)], 1).astype(np.float32)
    pts = torch.from_numpy(pts_np).to(dev)
    table = fp.box_table(boxes, grow)
    words = torch.empty((h, (w + 31) // 32), dtype=torch.int32, device=dev)
    bitmap = fp.Bitmap(words, lat, cell)

    def raster():
        run(dev, "d3d_floorplan_raster", ptr(table), None, k, cell, origin[0], origin[1], h, w, ptr(words), stream_of(dev))

    ms = {"table": _median_ms(lambda: fp.box_table(boxes, grow), calls), "raster": _median_ms(raster, calls),
          "rooms": _median_ms(lambda: fp.label_rooms(bitmap), calls)}
    plan = fp.label_rooms(bitmap, return_phases=True)
    ms["sides"] = _median_ms(lambda: fp.box_sides(plan, boxes), calls)
    ms["points"] = _median_ms(lambda: fp.room_of_points(pts, plan), calls)
    sides, room = fp.box_sides(plan, boxes), fp.room_of_points(pts, plan)
    torch.cuda.synchronize()
    # the host restatement, once, from the device's table
    t_np, t0_np = table.cpu().numpy(), fp.box_table(boxes, 0.0).cpu().numpy()
    host = {}
    host["table"], _ = _host(lambda: ref.box_table(boxes_np, grow))
    host["raster"], blk = _host(lambda: ref.blocked(t_np, None, cell, origin, shape))
    host["rooms"], (label, r, cells, bounds, seed) = _host(lambda: ref.rooms(blk, plan.min_cells, plan.max_rooms))
    host["sides"], want_sides = _host(lambda: ref.sides(t0_np, label, cell, origin, 0.5))
    host["points"], want_room = _host(lambda: ref.room_of_points(pts_np, label, cell, origin))
    same = {"bitmap": bool(np.array_equal(bitmap.blocked.cpu().numpy(), blk)),
            "label": bool(np.array_equal(plan.label.cpu().numpy(), label)), "count": plan.count == r,
            "tables": bool(np.array_equal(plan.cells.cpu().numpy(), cells) and np.array_equal(plan.bounds.cpu().numpy(), bounds)
                           and np.array_equal(plan.seed.cpu().numpy(), seed)),
            "sides": bool(np.array_equal(sides.cpu().numpy(), want_sides)),
            "points": bool(np.array_equal(room.cpu().numpy(), want_room))}
    if want_rooms is not None and r != want_rooms:
        raise SystemExit(f"{name}: {r} rooms, expected {want_rooms}")
    nw = (w + 31) // 32
    compulsory = h * nw * 4 + h * w * 4
    moved = h * w * 4 * CELL_WORDS + h * nw * 4 * BITMAP_WORDS
    return {"case": name, "lattice": [h, w], "boxes": k, "points": int(pts.shape[0]), "rooms": r,
            "blocked_share": round(float(blk.mean()), 4), "gpu_ms": {p: round(v, 4) for p, v in ms.items()},
            "rooms_phases_ms": {p: round(v, 4) for p, v in plan.phase_ms.items()},
            "host_ms": {p: round(v, 2) for p, v in host.items()}, "equal_to_host": same,
            "rooms_bytes_compulsory": compulsory, "rooms_bytes_moved": moved,
            "rooms_gbps_of_moved": round(moved / (ms["rooms"] * 1e-3) / 1e9, 1),
            "rooms_gbps_of_compulsory": round(compulsory / (ms["rooms"] * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--case", default="all", choices=("detector", "max", "all"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("floorplan_probe measures on the GPU: none found")
    dev = torch.device("cuda:0")
    lines = [json.dumps(run_case(c, args.calls, dev)) for c in (("detector", "max") if args.case == "all" else (args.case,))]
    for line in lines:
        print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
