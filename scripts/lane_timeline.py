"""Where the streams of one building's pass are, level by level (timeline marks of FPN_Net._forward_async_geometry): for
every pyramid level the times -- ms since the caller's stream started the pass -- at which the host enters and leaves
the level and the caller's stream arrives at it and goes on; then the pass's other marks (input grid, level-0 rulebook,
point lists and input means, the ends of the down and the top-down path).
  python scripts/lane_timeline.py [points]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from detection_3d_amd.config import get_cfg
from detection_3d_amd.detector import build_detection_model
from detection_3d_amd import timeline
from detection_3d_amd.synthetic import make_scene
from detection_3d_amd.voxelize import voxelize

n_points = int(sys.argv[1]) if len(sys.argv) > 1 else 500000
dev = torch.device("cuda:0")
cfg = get_cfg("4c_Fpn432")
torch.manual_seed(0)
model = build_detection_model(cfg).to(dev).eval()
clouds = [torch.from_numpy(make_scene(i, n_points)).to(dev) for i in range(4)]
with torch.no_grad():
    for i in range(8):
        model(list(voxelize(clouds[i % 4], 50, cfg.SPARSE3D.VOXEL_FULL_SCALE)))
    torch.cuda.synchronize()
    rows = {}
    for rep in range(6):
        inp = list(voxelize(clouds[rep % 4], 50, cfg.SPARSE3D.VOXEL_FULL_SCALE))
        torch.cuda.synchronize()
        timeline.MARKS = []
        start = torch.cuda.Event(enable_timing=True)
        start.record()
        h0 = time.perf_counter()
        model(inp)
        end = torch.cuda.Event(enable_timing=True)
        end.record()
        torch.cuda.synchronize()
        marks, timeline.MARKS = timeline.MARKS, None
        for label, k, ev, host in marks:
            t = (host - h0) * 1e3 if ev is None else start.elapsed_time(ev)
            rows.setdefault((k, label + (" (host clock)" if ev is None and k < 0 else "")), []).append(t)
            if ev is not None and k < 0:
                rows.setdefault((k, label + " [host enqueued]"), []).append((host - h0) * 1e3)
        rows.setdefault((-1, "pass done"), []).append(start.elapsed_time(end))
labels = ["host enters", "main arrives", "main continues", "host leaves"]
print("median of 6 passes, ms since the pass started")
print("level " + " ".join(f"{l[:15]:>15}" for l in labels))
for k in sorted({k for k, _ in rows if k >= 0}):
    cells = []
    for l in labels:
        v = rows.get((k, l))
        cells.append(f"{sorted(v)[len(v) // 2]:15.2f}" if v else " " * 15)
    print(f"{k:5d} " + " ".join(cells))
print("caller's stream after the levels:")
for (k, l), v in sorted(((kl, v) for kl, v in rows.items() if kl[0] < 0), key=lambda t: sorted(t[1])[len(t[1]) // 2]):
    print(f"  {l:40s} {sorted(v)[len(v) // 2]:7.2f}")
