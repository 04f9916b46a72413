"""Cost and effect of tsdf.TsdfVolume and tsdf.fuse_frames_tsdf on the GPU, against what is there today.

    python scripts/tsdf_probe.py [--frames 100] [--height 480] [--width 640] [--voxel 0.02] [--rounds 9] [--out FILE]

Workload: `frames` posed frames of fp32 depth and uint8 colour rendered (render.render_depth) from the synthetic
building of scripts/render_probe.py, cameras scattered through it.

Timed, each on its own: the allocation pass on an empty volume ("touch_insert": every block is inserted) and on a volume
that holds the blocks already ("touch_found": plain loads only; both include the call's read-back), the integration pass
over all blocks, and the extraction (block sort, count, scan, read-back, rows; nine columns).  Warm calls first, then
Beside the extraction, on the same volume, the mesh ("mesh": block sort, count, two scans, read-back, vertices with
colours, triangles; TsdfVolume.mesh), with its vertex and triangle counts and scratch bytes.
`rounds` rounds over the cases, interleaved.  "cold": a 1 GiB buffer is rewritten before the call, so that inputs and
voxel state come from HBM; "warm": calls back to back.  Medians with quartiles.  Beside them fuse_frames and
fuse_frames_tsdf as a user calls them.

Checked: a chunked torch fp64 expression of the same integration over the same blocks gives the same bits (tsdf and
weight), and is timed once.  Counted: blocks, bytes held, and the share of (block, frame) pairs the cull removes.

Effect: with Gaussian noise of `--noise` metres on every depth, the RMS distance to the mesh of a sample of the points
of fuse_frames_tsdf and of fuse_frames.  One JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def _timed(fn, evict=None):
    if evict is not None:
        evict.add_(1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _stats(ms):
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [min(ms), statistics.median(ms), max(ms)]
    return {"median_ms": round(statistics.median(ms), 3), "q1_ms": round(q[0], 3), "q3_ms": round(q[2], 3)}


def torch_integrate(vol, fr, chunk=4096):
    """the integration of include/d3d_hip.h as a torch fp64 expression over vol's blocks in their coordinate order, from
    zero state -> (tsdf, weight) fp32 [B, 512]"""
    coords = vol.blocks()[0].long()
    dev = coords.device
    F, H, W = fr.shape
    z = fr.depth.double() if fr.depth.dtype == torch.float32 else \
        (fr.depth.view(torch.int16).int() & 0xFFFF).double() * fr.depth_scale
    valid = torch.isfinite(z) & (z > 0)
    l = torch.stack(torch.meshgrid(*[torch.arange(8, device=dev)] * 3, indexing="ij"), -1).view(512, 3)
    origin = torch.tensor(vol.origin, dtype=torch.float64, device=dev)
    K, E = fr.intrinsics, fr.extrinsics
    out_d, out_w = [], []
    for b0 in range(0, coords.shape[0], chunk):
        g = 8 * coords[b0:b0 + chunk, None, :] + l[None]
        X = origin + g.double() * vol.voxel
        S = torch.zeros(g.shape[:2], dtype=torch.float64, device=dev)
        n = torch.zeros(g.shape[:2], dtype=torch.float64, device=dev)
        for f in range(F):
            d = X - E[f, :, 3]
            c = [(E[f, 0, j] * d[..., 0] + E[f, 1, j] * d[..., 1]) + E[f, 2, j] * d[..., 2] for j in range(3)]
            pu = torch.floor((c[0] * K[f, 0] / c[2] + K[f, 2]) + 0.5)
            pv = torch.floor((c[1] * K[f, 1] / c[2] + K[f, 3]) + 0.5)
            ok = (c[2] > 0) & (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
            iu, iv = torch.where(ok, pu, 0.0).long(), torch.where(ok, pv, 0.0).long()
            zp = z[f][iv, iu]
            sdf = zp - c[2]
            ok = ok & valid[f][iv, iu] & ~(sdf < -vol.trunc)
            q = sdf / vol.trunc
            S = torch.where(ok, S + torch.where(q > 1.0, 1.0, q), S)
            n = n + ok
        out_d.append(torch.where(n > 0, S / n, 0.0).float())       # from zero state: (0 * 0 + S) / (0 + n)
        out_w.append(n.float())
    return torch.cat(out_d), torch.cat(out_w)


def mesh_distance(points, mesh, chunk=1024):
    """distance of points fp32 [P, 3] to the nearest triangle of the mesh (fp64, all pairs in chunks)"""
    tri = mesh.vertices.double()[mesh.triangles.long()]                       # [T, 3, 3]
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    nrm = torch.linalg.cross(b - a, c - a)
    nrm = nrm / nrm.norm(dim=-1, keepdim=True)

    def segment(p, s, e):
        se = e - s
        t = (((p - s) * se).sum(-1) / (se * se).sum(-1).clamp_min(1e-300)).clamp(0.0, 1.0)
        return (p - (s + t[..., None] * se)).norm(dim=-1)

    out = []
    for p0 in range(0, points.shape[0], chunk):
        p = points[p0:p0 + chunk, None, :].double()
        h = ((p - a) * nrm).sum(-1)
        q = p - h[..., None] * nrm
        inside = torch.ones_like(h, dtype=torch.bool)
        for s, e in ((a, b), (b, c), (c, a)):
            inside &= (torch.linalg.cross(e - s, q - s) * nrm).sum(-1) >= 0
        d = torch.where(inside, h.abs(), torch.full_like(h, float("inf")))
        for s, e in ((a, b), (b, c), (c, a)):
            d = torch.minimum(d, segment(p, s, e))
        out.append(d.min(1).values)
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--max-blocks", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--sample", type=int, default=20000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from render_probe import make_cameras, make_mesh
    from detection_3d_amd import _lib
    from detection_3d_amd.downsample import cap_points
    from detection_3d_amd.render import render_depth
    from detection_3d_amd.tsdf import TsdfVolume, fuse_frames_tsdf
    from detection_3d_amd.unproject import DepthFrames, fuse_frames
    _lib.lib()
    dev = torch.device("cuda:0")
    mesh, lo, hi = make_mesh(0, dev)
    intr, extr = make_cameras(args.frames, args.width, lo, hi)
    intr[3] = 0.5 * (args.height - 1)
    fr = render_depth(mesh, intr, extr, args.height, args.width)
    F, H, W = fr.shape
    row = {"frames": F, "height": H, "width": W, "voxel": args.voxel, "rounds": args.rounds,
           "valid_share": round(float((fr.depth > 0).float().mean()), 4)}

    vol = TsdfVolume.around(fr, args.voxel, max_blocks=args.max_blocks)
    vol.count_cull = True
    vol.integrate(fr)
    torch.cuda.synchronize()
    row.update(blocks=vol.n_blocks, state_MB=round(vol.state_bytes / 1e6, 1), clipped=vol.clipped,
               culled_pair_share=round(vol.culled_pairs / max(vol.pairs, 1), 4))
    vol.count_cull = False
    # the same integration as a torch expression: equal bits
    t_ms, (t_d, t_w) = _timed(lambda: torch_integrate(vol, fr))
    _, k_d, k_w, _, _ = vol.blocks()
    row["torch_fp64_integrate_ms"] = round(t_ms, 1)
    row["torch_equal_bits"] = bool(torch.equal(t_d.view(torch.int32), k_d.reshape(-1, 512).view(torch.int32)) and
                                   torch.equal(t_w, k_w.reshape(-1, 512)))
    del t_d, t_w, k_d, k_w

    n = vol.n_blocks
    kw = (0.0, float("inf"))

    def touch_insert():
        vol.reset()
        return vol._touch(fr, 1, *kw)

    cases = {"touch_insert": touch_insert, "touch_found": lambda: vol._touch(fr, 1, *kw),
             "integrate": lambda: vol._update(fr, n, 0, *kw, 256.0),       # from zero state: the ids above are new ones
             "extract9": lambda: (setattr(vol, "_order", None), vol.surface_points(9))[1],
             "mesh": lambda: (setattr(vol, "_order", None), vol.mesh())[1],
             "fuse_frames": lambda: fuse_frames(fr, voxel=args.voxel),
             "fuse_frames_tsdf": lambda: fuse_frames_tsdf(fr, voxel=args.voxel, max_blocks=args.max_blocks)}
    for fn in cases.values():
        fn()
    evict = torch.zeros(1 << 28, dtype=torch.int32, device=dev)
    cold, warm = {k: [] for k in cases}, {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, fn in cases.items():
            warm[k].append(_timed(fn)[0])
            cold[k].append(_timed(fn, evict)[0])
    for k in cases:
        row[k] = dict(_stats(cold[k]), warm=_stats(warm[k]))
    row["surface_rows"] = int(vol.surface_points(3).shape[0])
    fused = vol.mesh()
    row.update(mesh_vertices=int(fused.vertices.shape[0]), mesh_triangles=int(fused.triangles.shape[0]),
               mesh_scratch_MB=round(_lib.lib().d3d_tsdf_mesh_scratch_bytes(n) / 1e6, 1),
               mesh_referenced_vertices=int(torch.unique(fused.triangles).numel()))
    del fused
    row["torch_over_kernel_integrate"] = round(row["torch_fp64_integrate_ms"] / row["integrate"]["median_ms"], 1)
    del evict, vol
    torch.cuda.empty_cache()
    print(json.dumps(dict(row, partial=True)), flush=True)

    # the claim: averaging across frames brings noisy points closer to the surface than the voxel mean does
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    noisy = torch.where(fr.depth > 0, fr.depth + args.noise * torch.randn(fr.depth.shape, device=dev, generator=g), fr.depth)
    nf = DepthFrames(noisy, fr.intrinsics, fr.extrinsics, color=fr.color)
    for name, cloud in (("tsdf", fuse_frames_tsdf(nf, voxel=args.voxel, max_points=None, max_blocks=args.max_blocks)),
                        ("voxel_mean", fuse_frames(nf, voxel=args.voxel, max_points=None)),
                        ("tsdf_clean", fuse_frames_tsdf(fr, voxel=args.voxel, max_points=None, max_blocks=args.max_blocks)),
                        ("voxel_mean_clean", fuse_frames(fr, voxel=args.voxel, max_points=None))):
        d = mesh_distance(cap_points(cloud, args.sample, 1)[:, :3], mesh)
        row["noise_" + name] = {"points": int(cloud.shape[0]), "rms_mm": round(float((d * d).mean().sqrt()) * 1e3, 3),
                                "median_mm": round(float(d.median()) * 1e3, 3),
                                "p95_mm": round(float(d.quantile(0.95)) * 1e3, 3)}
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
