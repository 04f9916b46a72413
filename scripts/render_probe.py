"""Cost of render.render_depth and render.scan_mesh per phase, and against a torch fp64 expression of the same
brute-force semantics, on the same GPU.

    python scripts/render_probe.py [--frames 100] [--size 640] [--rounds 9] [--levels 1 5] [--out FILE]

Scenes: synthetic.make_targets' boxes with a floor and a ceiling slab as a mesh (render.box_mesh), every triangle split
into 4^level by its edge midpoints: level 1 is about 10^3 large triangles, level 5 about 3 10^5 small ones.  `frames`
cameras 1.3 m above the floor at seeded positions inside the mesh's extent, looking level in seeded directions, at
size x size pixels (the reference's gen_cam_images renders 640 x 640).

Phases, each between its own pair of events, one chunk of all frames at a time as render_depth runs them: "bin"
(d3d_render_bin: rectangles, tile counts, scan, and the host read-back of the list length), "fill" (d3d_render_fill) and
"tiles" (d3d_render_tiles); "render_depth" is the whole call and "scan_mesh" the chain to at most 500 000 points.  Two warm
calls first, then `rounds` rounds over the cases in turn; medians with the quartiles.  List lengths per (frame, tile)
are read from the tile counts (the second 256-byte slot of the scratch, render.hip's carve).
Baseline, never the code under test: the semantics of include/d3d_hip.h as a torch fp64 expression over [F, H, W, T]
in chunks of triangles, at a size it can finish (--base-frames 4 at --base-size 160 on the level-1 mesh); render_depth
runs at that same size beside it, and the two results are compared.  One JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

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


def _stats(ms):
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [min(ms), statistics.median(ms), max(ms)]
    return {"median_ms": round(statistics.median(ms), 3), "q1_ms": round(q[0], 3), "q3_ms": round(q[2], 3)}


def make_mesh(level, dev):
    from detection_3d_amd.render import TriangleMesh, box_mesh
    from detection_3d_amd.synthetic import make_targets
    boxes = make_targets(0)[0].astype(np.float64)
    v = box_mesh(boxes)[0]
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    ctr, size = 0.5 * (lo + hi), hi - lo
    slabs = [[ctr[0], ctr[1], lo[2] - 0.1, size[0], size[1], 0.1, 0.0], [ctr[0], ctr[1], hi[2], size[0], size[1], 0.1, 0.0]]
    v, t = box_mesh(np.concatenate([boxes, np.array(slabs)]))
    p = v[t].astype(np.float64)                                 # [T, 3, 3]: the corners of every triangle
    for _ in range(level):
        a, b, c = p[:, 0], p[:, 1], p[:, 2]
        ab, bc, ca = 0.5 * (a + b), 0.5 * (b + c), 0.5 * (c + a)
        p = np.concatenate([np.stack(q, 1) for q in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))])
    vertices = torch.from_numpy(p.reshape(-1, 3).astype(np.float32)).to(dev)
    triangles = torch.arange(vertices.shape[0], dtype=torch.int32, device=dev).view(-1, 3)
    color = torch.randint(0, 256, vertices.shape, dtype=torch.uint8, device=dev)
    return TriangleMesh(vertices, triangles, color), lo, hi


def make_cameras(F, size, lo, hi, seed=0):
    from detection_3d_amd.render import look_at
    rs = np.random.RandomState(seed)
    extr = []
    for _ in range(F):
        eye = np.array([rs.uniform(lo[0] + 1, hi[0] - 1), rs.uniform(lo[1] + 1, hi[1] - 1), 1.3])
        yaw = rs.uniform(0, 2 * math.pi)
        extr.append(look_at(eye, eye + [math.cos(yaw), math.sin(yaw), 0.0]))
    return np.array([0.9 * size, 0.9 * size, 0.5 * (size - 1), 0.5 * (size - 1)]), np.stack(extr)


def torch_render(mesh, intr, extr, H, W, chunk=128):
    """the contract of include/d3d_hip.h as a torch fp64 expression -> (z fp64 [F, H, W] (inf: no hit), tri int64)"""
    dev = mesh.device
    K = torch.as_tensor(intr, dtype=torch.float64, device=dev).expand(extr.shape[0], 4)
    E = torch.as_tensor(extr, dtype=torch.float64, device=dev)
    x = mesh.vertices.double()
    d = [x[None, :, k] - E[:, k, 3, None] for k in range(3)]
    P = torch.stack([(E[:, 0, k, None] * d[0] + E[:, 1, k, None] * d[1]) + E[:, 2, k, None] * d[2] for k in range(3)], 2)
    u = torch.arange(W, dtype=torch.float64, device=dev)[None, None, :, None]
    v = torch.arange(H, dtype=torch.float64, device=dev)[None, :, None, None]
    dx, dy = (u - K[:, 2, None, None, None]) / K[:, 0, None, None, None], (v - K[:, 3, None, None, None]) / K[:, 1, None, None, None]
    F = E.shape[0]
    zbest = torch.full((F, H, W), math.inf, dtype=torch.float64, device=dev)
    tbest = torch.full((F, H, W), -1, dtype=torch.int64, device=dev)

    def cross(p, q):
        return (p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1], p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2],
                p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0])
    T = mesh.triangles.shape[0]
    for t0 in range(0, T, chunk):
        idx = mesh.triangles[t0:t0 + chunk].long()
        a, b, c = (P[:, idx[:, j]] for j in range(3))                       # [F, C, 3]
        n = [cross(b, c), cross(c, a), cross(a, b)]
        D = (a[..., 0] * n[0][0] + a[..., 1] * n[0][1]) + a[..., 2] * n[0][2]
        e = [(dx * m[0][:, None, None, :] + dy * m[1][:, None, None, :]) + m[2][:, None, None, :] for m in n]
        S = (e[0] + e[1]) + e[2]
        inside = ((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0))
        z = D[:, None, None, :] / S
        z = torch.where(inside & (S != 0) & torch.isfinite(z) & (z > 0), z, torch.full_like(z, math.inf))
        zc, tc = z.min(3)                                                   # the first minimum: the lowest index
        better = zc < zbest
        zbest = torch.where(better, zc, zbest)
        tbest = torch.where(better, tc + t0, tbest)
    return zbest, tbest


def phases(mesh, intr, extr, size, rounds):
    """render_depth's chunk loop with every library call between its own events -> (stats, list statistics)"""
    from detection_3d_amd._lib import check, lib, ptr, stream_of
    from detection_3d_amd.render import _Call, _cameras
    K, E = _cameras("probe", intr, extr)
    F, dev = E.shape[0], mesh.device
    depth = torch.empty((F, size, size), dtype=torch.float32, device=dev)
    color = torch.empty((F, size, size, 3), dtype=torch.uint8, device=dev)
    call = _Call(mesh, K, E, size, size, depth, color, 0.001)
    ms = {"bin": [], "fill": [], "tiles": []}
    for r in range(rounds + 2):
        t_bin, (scratch, entries) = _timed(lambda: call.bin(0, F))
        lists = torch.empty(max(entries, 1), dtype=torch.int32, device=dev)
        s, views = stream_of(dev), call.frames(0, F)
        t_fill, _ = _timed(lambda: check(lib().d3d_render_fill(mesh.desc, views, call.info, ptr(scratch), scratch.numel(),
                                                                ptr(lists), s)))
        t_tiles, _ = _timed(lambda: check(lib().d3d_render_tiles(mesh.desc, views, 0.0, math.inf, call.info, ptr(scratch),
                                                                  scratch.numel(), ptr(lists), None, s)))
        if r >= 2:
            ms["bin"].append(t_bin), ms["fill"].append(t_fill), ms["tiles"].append(t_tiles)
    n_tiles = F * ((size + 15) // 16) ** 2
    counts = scratch[256:256 + 4 * n_tiles].view(torch.int32)
    info = {"list_entries": entries, "n_tiles": n_tiles, "mean_list": round(entries / n_tiles, 1),
            "max_list": int(counts.max()), "hit_share": round(float((depth > 0).double().mean()), 4)}
    return {k: _stats(v) for k, v in ms.items()}, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--levels", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--base-frames", type=int, default=4)
    ap.add_argument("--base-size", type=int, default=160)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from detection_3d_amd import _lib
    from detection_3d_amd.render import render_depth, scan_mesh
    _lib.lib()
    dev = torch.device("cuda:0")
    row = {"frames": args.frames, "size": args.size, "rounds": args.rounds, "scenes": {}}
    for level in args.levels:
        mesh, lo, hi = make_mesh(level, dev)
        intr, extr = make_cameras(args.frames, args.size, lo, hi)
        cases = {"render_depth": lambda: render_depth(mesh, intr, extr, args.size, args.size),
                 "scan_mesh": lambda: scan_mesh(mesh, intr, extr, args.size, args.size)}
        for fn in cases.values():
            fn(), fn()
        times = {k: [] for k in cases}
        for _ in range(args.rounds):
            for k, fn in cases.items():
                t, out = _timed(fn)
                times[k].append(t)
        sc = {"triangles": int(mesh.triangles.shape[0]), "points": int(out.shape[0])}
        sc.update({k: _stats(v) for k, v in times.items()})
        ph, info = phases(mesh, intr, extr, args.size, args.rounds)
        sc.update(ph)
        sc.update(info)
        row["scenes"][f"level{level}"] = sc
        print(json.dumps({"partial": True, f"level{level}": sc}), flush=True)
        del mesh, out
        torch.cuda.empty_cache()
    mesh, lo, hi = make_mesh(min(args.levels), dev)
    intr, extr = make_cameras(args.base_frames, args.base_size, lo, hi)
    cases = {"torch_fp64": lambda: torch_render(mesh, intr, extr, args.base_size, args.base_size),
             "render_depth": lambda: render_depth(mesh, intr, extr, args.base_size, args.base_size, return_triangles=True)}
    outs, times = {}, {k: [] for k in cases}
    for k, fn in cases.items():
        fn()
    for _ in range(args.rounds):
        for k, fn in cases.items():
            t, outs[k] = _timed(fn)
            times[k].append(t)
    z, tri = outs["torch_fp64"]
    frames, got = outs["render_depth"]
    base = {"frames": args.base_frames, "size": args.base_size, "triangles": int(mesh.triangles.shape[0])}
    base.update({k: _stats(v) for k, v in times.items()})
    base["triangles_equal"] = bool((tri == got.long()).all())
    base["depth_equal"] = bool((torch.where(tri >= 0, z, torch.zeros_like(z)).float() == frames.depth).all())
    base["torch_over_kernel"] = round(base["torch_fp64"]["median_ms"] / base["render_depth"]["median_ms"], 1)
    row["baseline"] = base
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
