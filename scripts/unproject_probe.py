"""Cost of unproject.unproject and unproject.fuse_frames against what a user writes today, on the same GPU.

    python scripts/unproject_probe.py [--frames 100] [--height 480] [--width 640] [--rounds 15] [--inner 4] [--out FILE]

Workload: `frames` posed frames of uint16 depth (a smooth surface 1 .. 5 m away in millimetres, ~15 % of the pixels
zero) and uint8 colour, cameras scattered through a 20 m building.  Baselines, never the code under test:
(a) the same back-projection as a torch fp64 expression (meshgrid, mask, boolean index), six columns, without the
finite / min / max tests of the contract, which this workload does not need (so (a) does a little less than the
kernel); (b) for nine columns that expression plus normals.estimate_normals(radius 0.1, max_nn 50) on its output, the
only way to normals today, `--normal-calls` times.

Timing: warm calls first, then `rounds` rounds over the cases, interleaved so that clocks drift alike.  A round times
every case twice, `inner` calls each.  "cold": a 1 GiB buffer is rewritten before every call and each call has its own
pair of events, so the 154 MB of input, which would fit the 256 MB Infinity Cache, come from HBM; the figure is the mean
of the round's calls.  "warm": the calls run back to back between one pair of events, as a caller looping over the same
frames would see them; then part of the input is still in the cache, and the rate is not an HBM rate.  Medians over
the rounds with the quartile spread.  A call of unproject is two kernels, a scan and the read-back of N; its rate is
the compulsory traffic over the call's time: 2 B of depth and 3 B of colour read per pixel, 4 columns B (+ 4 B with
return_pixels) written per kept pixel.  One JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, inner=1, evict=None):
    """ms per call over `inner` calls (evict: a buffer to rewrite before each call, outside the timed span), last result"""
    if evict is None:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / inner, out
    ms = 0.0
    for _ in range(inner):
        evict.add_(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms += a.elapsed_time(b)
    return ms / inner, out


def _stats(ms):
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [min(ms), statistics.median(ms), max(ms)]
    return {"median_ms": round(statistics.median(ms), 3), "q1_ms": round(q[0], 3), "q3_ms": round(q[2], 3)}


def make_frames(F, H, W, dev, seed=0):
    from detection_3d_amd.unproject import DepthFrames
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    v, u = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    f = torch.arange(F, device=dev)[:, None, None]
    z = 3.0 + 1.2 * torch.sin(u / 97.0 + f) + 0.7 * torch.cos(v / 61.0 - f)
    z = z + 0.003 * torch.randn((F, H, W), device=dev, generator=g)
    mm = (z * 1000.0).round().to(torch.int32)
    mm[torch.rand((F, H, W), device=dev, generator=g) < 0.15] = 0
    depth = mm.to(torch.int16).view(torch.uint16)            # below 2^15 mm: the same bits
    color = torch.randint(0, 256, (F, H, W, 3), device=dev, generator=g, dtype=torch.uint8)
    yaw = torch.rand(F, generator=g, device=dev).double() * 6.283
    c, s, o, l = torch.cos(yaw), torch.sin(yaw), torch.zeros_like(yaw), torch.ones_like(yaw)
    R = torch.stack([torch.stack([s, o, c], 1), torch.stack([-c, o, s], 1), torch.stack([o, -l, o], 1)], 1)   # z up
    t = torch.rand((F, 3), generator=g, device=dev).double() * torch.tensor([20.0, 20.0, 1.0], device=dev, dtype=torch.float64)
    extr = torch.cat([R, t[:, :, None]], 2)
    intr = torch.tensor([0.9 * W, 0.9 * W, 0.5 * (W - 1), 0.5 * (H - 1)], dtype=torch.float64)
    return DepthFrames(depth, intr, extr, color=color), mm


def torch_unproject(mm, fr):
    """the contract of include/d3d_hip.h as a torch fp64 expression -> fp32 [N, 6] (mm: the depth as int32)"""
    F, H, W = mm.shape
    z = mm.double() * fr.depth_scale
    K, E = fr.intrinsics, fr.extrinsics
    v, u = torch.meshgrid(torch.arange(H, device=mm.device, dtype=torch.float64),
                          torch.arange(W, device=mm.device, dtype=torch.float64), indexing="ij")
    fx, fy, cx, cy = (K[:, j, None, None] for j in range(4))
    x, y = (u - cx) * (z / fx), (v - cy) * (z / fy)
    mask = z > 0
    cols = [(((E[:, k, 0, None, None] * x + E[:, k, 1, None, None] * y) + E[:, k, 2, None, None] * z)
             + E[:, k, 3, None, None])[mask] for k in range(3)]
    rgb = fr.color[mask].double() / 256.0
    return torch.cat([torch.stack(cols, 1), rgb], 1).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--normal-calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from detection_3d_amd import _lib
    from detection_3d_amd.normals import estimate_normals
    from detection_3d_amd.unproject import fuse_frames, unproject
    _lib.lib()
    dev = torch.device("cuda:0")
    fr, mm = make_frames(args.frames, args.height, args.width, dev)
    P = mm.numel()
    cases = {"unproject6": lambda: unproject(fr, columns=6), "unproject9": lambda: unproject(fr, columns=9),
             "unproject9_pixels": lambda: unproject(fr, columns=9, return_pixels=True),
             "unproject9_step2": lambda: unproject(fr, columns=9, step=2),
             "torch_fp64_6": lambda: torch_unproject(mm, fr), "fuse_frames": lambda: fuse_frames(fr)}
    for _ in range(2):
        for fn in cases.values():
            fn()
    evict = torch.zeros(1 << 28, dtype=torch.int32, device=dev)
    times, warm = {k: [] for k in cases}, {k: [] for k in cases}
    outs = {}
    for _ in range(args.rounds):
        for k, fn in cases.items():
            outs.pop(k, None)
            t, _ = _timed(fn, args.inner)
            warm[k].append(t)
            t, outs[k] = _timed(fn, args.inner, evict)
            times[k].append(t)
    N = int(outs["unproject6"].shape[0])
    row = {"frames": args.frames, "height": args.height, "width": args.width, "pixels": P, "kept": N,
           "valid_share": round(N / P, 4), "rounds": args.rounds, "inner": args.inner}
    for k in cases:
        row[k] = _stats(times[k])
        row[k]["warm"] = _stats(warm[k])
    for k, cols, extra, n in (("unproject6", 6, 0, N), ("unproject9", 9, 0, N), ("unproject9_pixels", 9, 4, N),
                              ("unproject9_step2", 9, 0, int(outs["unproject9_step2"].shape[0]))):
        nbytes = 5 * P + (4 * cols + extra) * n
        row[k]["compulsory_MB"] = round(nbytes / 1e6, 1)
        row[k]["call_TBps"] = round(nbytes / (row[k]["median_ms"] * 1e-3) / 1e12, 3)
        row[k]["warm"]["call_TBps"] = round(nbytes / (row[k]["warm"]["median_ms"] * 1e-3) / 1e12, 3)
    row["fused_points"] = int(outs["fuse_frames"].shape[0])
    base = outs["torch_fp64_6"]
    row["rows_equal_torch"] = int(base.shape[0]) == N
    row["largest_difference_to_torch"] = float((base - outs["unproject6"]).abs().max()) if row["rows_equal_torch"] else None
    row["torch_over_kernel_6"] = round(row["torch_fp64_6"]["median_ms"] / row["unproject6"]["median_ms"], 2)
    del outs, evict
    torch.cuda.empty_cache()
    print(json.dumps(dict(row, partial=True)), flush=True)
    tn = []
    for _ in range(args.normal_calls):
        t, _ = _timed(lambda: estimate_normals(base))
        tn.append(t)
    row["estimate_normals_on_torch_output"] = _stats(tn)
    row["torch_plus_normals_over_kernel_9"] = round((row["torch_fp64_6"]["median_ms"] + statistics.median(tn)) /
                                                    row["unproject9"]["median_ms"], 2)
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
