"""Cost of primitives.fit_boxes (d3d_fit_boxes) against a chunked torch expression of the same definition on the same GPU.

    python scripts/fit_probe.py [--calls 30] [--chunk 65536] [--no-cpu] [--out FILE]

Cases: 500 k points x 200 instances and 1 M x 600: wall-like boxes of synthetic.make_boxes, points drawn inside them, the
instance of every point found by primitives.points_in_boxes.  Reported per case, medians over `calls` rounds with the
10th and 90th percentile, every round timing each variant once with device events, interleaved so that clocks and caches
drift alike, after three warm rounds:
  fit_boxes_ms          the whole call (Python, lists, six launches);
  lists_ms              the sort / offset plumbing in torch;
  pass1_ms, pass2_ms    accumulator fill, sweep and pick of each pass, between events inside the library;
  torch_chunked_ms      the same definition in torch: per chunk of rows the [rows, 256] rotations and scatter_reduce_
                        amin / amax into [K, 256], an fp64 argmin per pass; with the number of instances whose choice or
                        extents differ from the kernel's bits;
  cpu_ref_s             tests/fit_ref.py in numpy on the host, once, for context only.
One JSON line per case."""
import argparse
import ctypes
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
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _stats(v):
    v = sorted(v)
    return [round(statistics.median(v), 4), round(v[len(v) // 10], 4), round(v[(len(v) * 9) // 10], 4)]


def _sweep(x, y, ids, c, s, k, chunk):
    """extents [4][k, 256] of u = c x - s y, v = s x + c y; c, s [256] or per instance [k, 256]"""
    dev = x.device
    acc = [torch.full((k, 256), float("inf"), device=dev), torch.full((k, 256), float("-inf"), device=dev),
           torch.full((k, 256), float("inf"), device=dev), torch.full((k, 256), float("-inf"), device=dev)]
    for o in range(0, x.shape[0], chunk):
        g = ids[o:o + chunk]
        cc, ss = (c[None], s[None]) if c.dim() == 1 else (c[g], s[g])
        xs, ys = x[o:o + chunk, None], y[o:o + chunk, None]
        u = (cc * xs - ss * ys) + 0.0
        v = (ss * xs + cc * ys) + 0.0
        idx = g[:, None].expand(-1, 256)
        acc[0].scatter_reduce_(0, idx, u, "amin")
        acc[1].scatter_reduce_(0, idx, u, "amax")
        acc[2].scatter_reduce_(0, idx, v, "amin")
        acc[3].scatter_reduce_(0, idx, v, "amax")
    return acc


def torch_fit(xyz, inst, k, coarse, fine, chunk):
    """-> choice int64 [k, 2], extent fp32 [k, 4] of the definition of include/d3d_hip.h in torch ops (all instances free,
    every instance non-empty)"""
    ok = (inst >= 0) & (inst < k) & torch.isfinite(xyz[:, :3]).all(1)
    x, y, ids = xyz[ok, 0], xyz[ok, 1], inst[ok].long()
    e = _sweep(x, y, ids, coarse[:, 0].float(), coarse[:, 1].float(), k, chunk)
    a = ((e[1].double() - e[0].double()) * (e[3].double() - e[2].double())).argmin(1)
    ca, sa = coarse[a, 0][:, None], coarse[a, 1][:, None]
    c = (ca * fine[None, :, 0] - sa * fine[None, :, 1]).float()
    s = (sa * fine[None, :, 0] + ca * fine[None, :, 1]).float()
    e = _sweep(x, y, ids, c, s, k, chunk)
    i = ((e[1].double() - e[0].double()) * (e[3].double() - e[2].double())).argmin(1)
    return torch.stack([a, i], 1), torch.stack([v.gather(1, i[:, None])[:, 0] for v in e], 1)


def make_case(n, k, dev):
    from detection_3d_amd.primitives import points_in_boxes
    from detection_3d_amd.synthetic import make_boxes
    scale = max(1.0, (k / 200.0) ** 0.5)
    boxes = make_boxes(k, k, extent=(25.0 * scale, 19.0 * scale, 2.7))[0].astype(np.float64)
    rng = np.random.RandomState(n % 7)
    j = rng.randint(0, k, n)
    u = rng.uniform(-0.5, 0.5, (n, 3)) * boxes[j, 3:6]
    c, s = np.cos(boxes[j, 6]), np.sin(boxes[j, 6])
    pcl = np.zeros((n, 9), np.float32)
    pcl[:, 0] = c * u[:, 0] + s * u[:, 1] + boxes[j, 0]
    pcl[:, 1] = -s * u[:, 0] + c * u[:, 1] + boxes[j, 1]
    pcl[:, 2] = boxes[j, 2] + 0.5 * boxes[j, 5] + u[:, 2]
    cloud = torch.from_numpy(pcl).to(dev)                     # [n, 9], read in place
    owner = points_in_boxes(cloud, torch.from_numpy(boxes.astype(np.float32)).to(dev), grow=(1e-3, 1e-3))[0]
    return cloud, owner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from detection_3d_amd import _lib
    from detection_3d_amd import primitives as P
    _lib.lib()
    dev = torch.device("cuda:0")
    rows = []
    for n, k in ((500_000, 200), (1_000_000, 600)):
        cloud, owner = make_case(n, k, dev)
        inst = owner.long()
        coarse, fine = P._fit_tables(dev)
        phases = (ctypes.c_float * 2)()

        def whole():
            return P.fit_boxes(cloud, owner, k=k, return_details=True)

        def lists():
            return P._fit_lists(cloud, inst, k, None)

        def baseline():
            return torch_fit(cloud, inst, k, coarse, fine, args.chunk)

        t = {"fit_boxes_ms": [], "lists_ms": [], "pass1_ms": [], "pass2_ms": [], "torch_chunked_ms": []}
        for r in range(3 + args.calls):
            tw, got = _timed(whole)
            tl, (order, srt, offsets) = _timed(lists)
            P._fit_call(cloud, None, order, srt, offsets, k, None, phases)
            tb, want = _timed(baseline)
            if r >= 3:
                for key, v in zip(t, (tw, tl, phases[0], phases[1], tb)):
                    t[key].append(v)
        some = got[1] > 0
        row = {"points": n, "instances": k, "labelled": int((owner >= 0).sum()), "non_empty": int(some.sum()),
               "chunk": args.chunk, "calls": args.calls}
        for key, v in t.items():
            row[key] = _stats(v)                              # median, 10th, 90th percentile
        row["choice_differ"] = int((got[2][some].long() != want[0][some]).any(1).sum())
        row["extent_differ"] = int((got[3][some][:, :4].view(torch.int32) != want[1][some].view(torch.int32)).any(1).sum())
        row["torch_over_fit_boxes"] = round(row["torch_chunked_ms"][0] / row["fit_boxes_ms"][0], 2)
        row["torch_over_passes"] = round(row["torch_chunked_ms"][0] / (row["pass1_ms"][0] + row["pass2_ms"][0]), 2)
        if not args.no_cpu:
            from tests.fit_ref import fit_boxes_ref
            xyz_h, inst_h = cloud[:, :3].cpu().numpy(), owner.cpu().numpy()
            t0 = time.perf_counter()
            ref = fit_boxes_ref(xyz_h, inst_h, k)
            row["cpu_ref_s"] = round(time.perf_counter() - t0, 2)
            row["cpu_ref_bits_differ"] = int((got[0].cpu().numpy().view(np.uint32) != ref[0].view(np.uint32)).any(1).sum())
        rows.append(row)
        print(json.dumps(row), flush=True)
        del cloud, owner, inst
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
