"""Cost of frame.manhattan_frame (d3d_manhattan_frame) against a chunked torch expression of the same votes on the same GPU.

    python scripts/frame_probe.py [--calls 30] [--chunk 65536] [--out FILE]

Cases: 500 k and 2 M normals of a synthetic room (30 % floor and ceiling, 45 % walls in two directions, 25 % clutter,
random signs, 2 degrees of noise per component), tilted by 14 degrees and turned by 63, read in place from columns 6:9 of
a nine-column cloud.  Reported per case, medians over `calls` rounds with the 10th and 90th percentile, every round
timing each variant once with device events, interleaved so that clocks and caches drift alike, after three warm rounds:
  manhattan_frame_ms    the whole call (Python, eleven launches);
  phase_ms              the five passes (sweep and pick each), between events inside the library;
  torch_chunked_ms      the same definition in torch: per chunk of rows the [rows, 256] votes as int64 and their column
                        sums, the frames composed in fp64 on the device, no read-back; with whether its choices, scores
                        and pose equal the kernel's bits;
  align_cloud_ms        manhattan_frame and register.apply_pose on the [N, 9] cloud.
One JSON line per case."""
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


def _stats(v):
    v = sorted(v)
    return [round(statistics.median(v), 4), round(v[len(v) // 10], 4), round(v[(len(v) * 9) // 10], 4)]


def make_case(n, dev, seed=0):
    """[n, 9] cloud whose columns 6:9 are the normals of a tilted, turned room"""
    from detection_3d_amd.frame import _rot
    rng = np.random.RandomState(seed)
    kind = rng.uniform(size=n)
    nm = rng.normal(size=(n, 3)) * math.radians(2.0)
    nm[kind < 0.3, 2] += 1.0
    nm[(kind >= 0.3) & (kind < 0.525), 0] += 1.0
    nm[(kind >= 0.525) & (kind < 0.75), 1] += 1.0
    junk = kind >= 0.75
    nm[junk] = rng.normal(size=(int(junk.sum()), 3))
    nm /= np.linalg.norm(nm, axis=1, keepdims=True)
    nm *= np.where(rng.uniform(size=(n, 1)) < 0.5, -1.0, 1.0)
    ti, az, ya = math.radians(14.0), math.radians(200.0), math.radians(63.0)
    T = _rot(np.array([math.sin(ti) * math.cos(az), math.sin(ti) * math.sin(az), math.cos(ti)]))
    Z = np.array([[math.cos(ya), -math.sin(ya), 0.0], [math.sin(ya), math.cos(ya), 0.0], [0.0, 0.0, 1.0]])
    pcl = np.zeros((n, 9), np.float32)
    pcl[:, :3] = rng.uniform(0, 20, (n, 3))
    pcl[:, 6:9] = nm @ (T @ Z).T
    return torch.from_numpy(pcl).to(dev)


def _mul(B, M):
    return (B[:, 0, None] * M[None, 0, :] + B[:, 1, None] * M[None, 1, :]) + B[:, 2, None] * M[None, 2, :]


def _winner(sc, default):
    idx = torch.arange(256, device=sc.device)
    best = sc.max()
    at = torch.where(sc == best, idx, torch.full_like(idx, 256)).min()
    return torch.where(best > 0, at, torch.full_like(at, default)), best


def torch_frame(nrm, max_tilt, tol, chunk):
    """-> pose fp64 [4, 4], choice int64 [5], score int64 [5] of the definition of include/d3d_hip.h in torch ops"""
    from detection_3d_amd import frame as F
    from detection_3d_amd.primitives import _fit_tables
    dev = nrm.device
    tables = F._device_tables(dev, max_tilt).reshape(3, 256, 3, 3)
    coarse, fine = _fit_tables(dev)
    n0, n1, n2 = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    m = (n0 * n0 + n1 * n1) + n2 * n2
    ok = (m >= 0.5) & (m <= 2.0)
    n0, n1, n2, m = n0[ok, None], n1[ok, None], n2[ok, None], m[ok, None]
    B = torch.eye(3, dtype=torch.float64, device=dev)
    choice, score = [], []
    for k, st in enumerate(F.tilt_steps(max_tilt)):
        s2 = F._s2(max(tol, st))
        u = ((B[:, 0, None] * tables[k, :, 0, 2][None] + B[:, 1, None] * tables[k, :, 1, 2][None]) +
             B[:, 2, None] * tables[k, :, 2, 2][None]).float()               # [3, 256]: the candidates' up directions
        sc = torch.zeros(256, dtype=torch.int64, device=dev)
        for o in range(0, n0.shape[0], chunk):
            d = (n0[o:o + chunk] * u[0][None] + n1[o:o + chunk] * u[1][None]) + n2[o:o + chunk] * u[2][None]
            a2 = d * d
            r = torch.minimum(a2, torch.clamp_min(m[o:o + chunk] - a2, 0.0))
            sc += (torch.clamp_min(s2 - r, 0.0) * 1073741824.0).long().sum(0)
        at, best = _winner(sc, 136)
        choice.append(at)
        score.append(best)
        B = _mul(B, tables[k][at])
    s2 = F._s2(tol)
    B32 = B.float()
    d = (n0 * B32[0, 2] + n1 * B32[1, 2]) + n2 * B32[2, 2]
    wall = (d * d <= s2)[:, 0]
    p = ((n0 * B32[0, 0] + n1 * B32[1, 0]) + n2 * B32[2, 0])[wall]
    q = ((n0 * B32[0, 1] + n1 * B32[1, 1]) + n2 * B32[2, 1])[wall]
    cd, sd = coarse[:, 0], coarse[:, 1]
    for k in (3, 4):
        if k == 4:
            ca, sa = coarse[choice[3], 0], coarse[choice[3], 1]
            cd, sd = ca * fine[:, 0] - sa * fine[:, 1], sa * fine[:, 0] + ca * fine[:, 1]
        c, s = cd.float()[None], sd.float()[None]
        sc = torch.zeros(256, dtype=torch.int64, device=dev)
        for o in range(0, p.shape[0], chunk):
            pp, qq = p[o:o + chunk], q[o:o + chunk]
            d1, d2 = c * pp + s * qq, c * qq - s * pp
            r = torch.minimum(d1 * d1, d2 * d2)
            sc += (torch.clamp_min(s2 - r, 0.0) * 1073741824.0).long().sum(0)
        at, best = _winner(sc, 0 if k == 3 else 128)
        choice.append(at)
        score.append(best)
    C, S = cd[choice[4]], sd[choice[4]]
    far = 128 * choice[3] + choice[4] - 128 >= 16384
    C, S = torch.where(far, S, C), torch.where(far, -C, S)
    zero, one = torch.zeros_like(C), torch.ones_like(C)
    Rz = torch.stack([torch.stack([C, -S, zero]), torch.stack([S, C, zero]), torch.stack([zero, zero, one])])
    pose = torch.eye(4, dtype=torch.float64, device=dev)
    pose[:3, :3] = _mul(B, Rz).T
    return pose, torch.stack(choice), torch.stack(score)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from detection_3d_amd import _lib
    from detection_3d_amd.frame import PHASES, align_cloud, manhattan_frame
    _lib.lib()
    dev = torch.device("cuda:0")
    rows = []
    for n in (500_000, 2_000_000):
        cloud = make_case(n, dev)
        nrm = cloud[:, 6:9]
        t = {"manhattan_frame_ms": [], "torch_chunked_ms": [], "align_cloud_ms": []}
        ph = {k: [] for k in PHASES}
        for r in range(3 + args.calls):
            tw, got = _timed(lambda: manhattan_frame(nrm))
            timed = manhattan_frame(nrm, phases=True)
            tb, want = _timed(lambda: torch_frame(nrm, 30.0, 5.0, args.chunk))
            ta, _ = _timed(lambda: align_cloud(cloud))
            if r >= 3:
                for key, v in zip(t, (tw, tb, ta)):
                    t[key].append(v)
                for k in PHASES:
                    ph[k].append(timed.phases[k])
        row = {"normals": n, "chunk": args.chunk, "calls": args.calls, "tilt_deg": round(got.tilt_deg, 4),
               "yaw_deg": round(got.yaw_deg, 4), "support": got.support.tolist(), "choice": got.choice.tolist()}
        for key, v in t.items():
            row[key] = _stats(v)                              # median, 10th, 90th percentile
        row["phase_ms"] = {k: _stats(v) for k, v in ph.items()}
        row["passes_ms"] = round(sum(statistics.median(v) for v in ph.values()), 4)
        row["choice_equal"] = bool(torch.equal(got.choice.long(), want[1]))
        row["score_equal"] = bool(torch.equal(got.score, want[2]))
        row["pose_bits_equal"] = bool(torch.equal(got.pose.view(torch.int64), want[0].view(torch.int64)))
        row["torch_over_call"] = round(row["torch_chunked_ms"][0] / row["manhattan_frame_ms"][0], 2)
        row["torch_over_passes"] = round(row["torch_chunked_ms"][0] / row["passes_ms"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del cloud, nrm
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
