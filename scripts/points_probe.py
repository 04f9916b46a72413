"""Cost of primitives.points_in_boxes (d3d_points_in_boxes) against a chunked torch expression of the same definition on
the same GPU.

    python scripts/points_probe.py [--calls 30] [--chunk 65536] [--out FILE]

Cases: 500 k points x 200 boxes and 1 M points x 600 boxes (points of synthetic.make_scene, wall-like boxes of
synthetic.make_boxes, grow (0.3, 0.3)).  The baseline builds the [chunk, K] membership mask in fp32 torch ops and
reduces it to the same four outputs.  Warm calls first, then `calls` rounds that each time one call of either with
events, interleaved so that clocks and caches drift alike; medians are reported, with the number of points whose owner
and of boxes whose count differ between the two (fp32 evaluation order differs at faces).  One JSON line per case."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def torch_points_in_boxes(xyz, boxes, grow, chunk):
    """the definition of include/d3d_hip.h in torch ops, `chunk` points at a time -> owner, count, lo, hi"""
    n, k = xyz.shape[0], boxes.shape[0]
    c = torch.cos(boxes[:, 6].double()).float()
    s = torch.sin(boxes[:, 6].double()).float()
    hx = torch.clamp(boxes[:, 3], min=grow[0]) * 0.5
    hy = torch.clamp(boxes[:, 4], min=grow[0]) * 0.5
    hz = torch.clamp(boxes[:, 5], min=grow[1])
    owner = torch.empty(n, dtype=torch.int32, device=xyz.device)
    count = torch.zeros(k, dtype=torch.int32, device=xyz.device)
    lo = torch.full((k, 3), float("inf"), device=xyz.device)
    hi = torch.full((k, 3), float("-inf"), device=xyz.device)
    inf = torch.tensor(float("inf"), device=xyz.device)
    ids = torch.arange(k, dtype=torch.int32, device=xyz.device)
    for o in range(0, n, chunk):
        p = xyz[o:o + chunk]
        dx, dy = p[:, None, 0] - boxes[None, :, 0], p[:, None, 1] - boxes[None, :, 1]
        local = (c * dx - s * dy, s * dx + c * dy, p[:, None, 2] - boxes[None, :, 2])
        m = (local[0].abs() <= hx) & (local[1].abs() <= hy) & (local[2] >= 0) & (local[2] <= hz)
        owner[o:o + chunk] = torch.where(m, ids, torch.tensor(k, dtype=torch.int32, device=xyz.device)).amin(1)
        count += m.sum(0, dtype=torch.int32)
        for d in range(3):
            lo[:, d] = torch.minimum(lo[:, d], torch.where(m, local[d], inf).amin(0))
            hi[:, d] = torch.maximum(hi[:, d], torch.where(m, local[d], -inf).amax(0))
    owner[owner == k] = -1
    return owner, count, lo, hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from detection_3d_amd import _lib
    from detection_3d_amd.primitives import points_in_boxes
    from detection_3d_amd.synthetic import make_boxes, make_scene
    _lib.lib()
    dev = torch.device("cuda:0")
    grow = (0.3, 0.3)
    rows = []
    for n, k in ((500_000, 200), (1_000_000, 600)):
        cloud = torch.from_numpy(make_scene(n % 7, n)).to(dev)           # [n, 9], read in place
        boxes = torch.from_numpy(make_boxes(k, k)[0]).to(dev)

        def kernel():
            return points_in_boxes(cloud, boxes, grow)

        def baseline():
            return torch_points_in_boxes(cloud, boxes, grow, args.chunk)

        for _ in range(3):
            kernel()
            baseline()
        tk, tb = [], []
        for _ in range(args.calls):
            t, got = _timed(kernel)
            tk.append(t)
            t, want = _timed(baseline)
            tb.append(t)
        row = {"points": n, "boxes": k, "kernel_ms": round(statistics.median(tk), 4),
               "torch_chunked_ms": round(statistics.median(tb), 4), "chunk": args.chunk, "calls": args.calls,
               "owners_differ": int((got[0] != want[0]).sum()), "counts_differ": int((got[1] != want[1]).sum()),
               "members": int(got[1].sum()), "owned": int((got[0] >= 0).sum())}
        row["torch_over_kernel"] = round(row["torch_chunked_ms"] / row["kernel_ms"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del cloud, boxes
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
