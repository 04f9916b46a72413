"""Cost of downsample.voxel_downsample and downsample.sample_rows against torch expressions of the same definitions on the
same GPU, and what down-sampling first saves normals.estimate_normals.

    python scripts/downsample_probe.py [--calls 9] [--sizes 2000000,10000000] [--per-voxel 4,20] [--out FILE]

Clouds: synthetic.make_scene with n / p points, every point repeated p times with a uniform jitter of +-5 mm, so that
voxels of 2 cm hold about p points (the measured mean is reported); nine columns.  Baselines, never the code under test:
cells by the same fp64 formula, torch.unique(cells, dim=0, return_inverse=True), fp64 index_add_ and a division (rows in
cell order, which costs the baseline nothing extra); for the cap the k smallest of torch.rand keys by topk and a sort of
the indices.  Warm calls first, then `calls` rounds that time one call of each with events, interleaved so that clocks
and caches drift alike; medians with the quartile spread.  estimate_normals (radius 0.1, max_nn 50) is timed on the raw
cloud and on the down-sampled one, `--normal-calls` times each.  One JSON line per case."""
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


def _stats(ms):
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [min(ms), statistics.median(ms), max(ms)]
    return {"median_ms": round(statistics.median(ms), 3), "q1_ms": round(q[0], 3), "q3_ms": round(q[2], 3)}


def torch_voxel_downsample(pcl, voxel, normal_col=6):
    """the definition of include/d3d_hip.h in torch ops -> (rows fp32 [M, C] in cell order, inverse, counts)"""
    p = pcl[:, :3].double()
    lo = p.amin(0) - 0.5 * voxel
    cells = torch.floor((p - lo) / voxel).long()
    uniq, inv = torch.unique(cells, dim=0, return_inverse=True)
    m = uniq.shape[0]
    sums = torch.zeros((m, pcl.shape[1]), dtype=torch.float64, device=pcl.device).index_add_(0, inv, pcl.double())
    cnt = torch.bincount(inv, minlength=m)
    mean = sums / cnt[:, None].double()
    v = mean[:, normal_col:normal_col + 3]
    length = torch.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    scale = torch.where((length > 0) & (cnt > 1), length, torch.ones_like(length))
    mean[:, normal_col:normal_col + 3] = v / scale[:, None]
    return mean.float(), inv, cnt


def torch_sample_rows(n, k, generator):
    keys = torch.rand(n, device=generator.device, generator=generator)
    return keys.topk(k, largest=False, sorted=False).indices.sort().values


def make_cloud(n, per_voxel, dev):
    from detection_3d_amd.synthetic import make_scene
    base = torch.from_numpy(make_scene(per_voxel, n // per_voxel)).to(dev)
    cloud = base.repeat_interleave(per_voxel, 0)
    g = torch.Generator(device=dev)
    g.manual_seed(n + per_voxel)
    cloud[:, :3] += (torch.rand((cloud.shape[0], 3), device=dev, generator=g) - 0.5) * 0.01
    return cloud[torch.randperm(cloud.shape[0], device=dev, generator=g)].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--normal-calls", type=int, default=3)
    ap.add_argument("--sizes", default="2000000,10000000")
    ap.add_argument("--per-voxel", default="4,20")
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--cap", type=int, default=500_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from detection_3d_amd import _lib
    from detection_3d_amd.downsample import sample_rows, voxel_downsample
    from detection_3d_amd.normals import estimate_normals
    _lib.lib()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    rows = []
    for n in (int(v) for v in args.sizes.split(",")):
        for p in (int(v) for v in args.per_voxel.split(",")):
            cloud = make_cloud(n, p, dev)
            n = cloud.shape[0]

            def kernel():
                return voxel_downsample(cloud, args.voxel, return_inverse=True, return_counts=True)

            def baseline():
                return torch_voxel_downsample(cloud, args.voxel)

            def cap():
                return sample_rows(n, args.cap, 0, dev)

            def cap_baseline():
                return torch_sample_rows(n, args.cap, gen)

            for _ in range(2):
                kernel(), baseline(), cap(), cap_baseline()
            tk, tb, tc, tcb = [], [], [], []
            for _ in range(args.calls):
                t, got = _timed(kernel)
                tk.append(t)
                t, want = _timed(baseline)
                tb.append(t)
                t, picked = _timed(cap)
                tc.append(t)
                t, _ = _timed(cap_baseline)
                tcb.append(t)
            small, _, counts = got
            same_counts = bool(torch.equal(counts.long().sort().values, want[2].sort().values))
            # rows in cell order on both sides: the baseline's order is the lexicographic order of the cells
            row = {"points": n, "per_voxel_target": p, "voxels": int(small.shape[0]),
                   "points_per_voxel": round(n / max(int(small.shape[0]), 1), 2), "largest_voxel": int(counts.max()),
                   "voxel_downsample": _stats(tk), "torch_unique_index_add": _stats(tb),
                   "sample_rows": _stats(tc), "torch_rand_topk": _stats(tcb), "cap": args.cap, "calls": args.calls,
                   "voxels_equal": int(want[0].shape[0]) == int(small.shape[0]), "counts_equal": same_counts,
                   "cap_rows": int(picked.shape[0])}
            row["torch_over_kernel"] = round(row["torch_unique_index_add"]["median_ms"] /
                                             row["voxel_downsample"]["median_ms"], 2)
            row["topk_over_sample_rows"] = round(row["torch_rand_topk"]["median_ms"] / row["sample_rows"]["median_ms"], 2)
            del got, want
            tr, ts = [], []
            estimate_normals(small)
            for _ in range(args.normal_calls):
                t, _ = _timed(lambda: estimate_normals(cloud))
                tr.append(t)
                t, _ = _timed(lambda: estimate_normals(small))
                ts.append(t)
            row["estimate_normals_raw"] = _stats(tr)
            row["estimate_normals_downsampled"] = _stats(ts)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del cloud, small, counts
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
