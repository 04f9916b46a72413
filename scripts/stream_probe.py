import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from detection_3d_amd.config import get_cfg
from detection_3d_amd.detector import build_detection_model
from detection_3d_amd.synthetic import make_scene
from detection_3d_amd.voxelize import voxelize
dev = torch.device("cuda:0")
cfg = get_cfg("4c_Fpn432")
torch.manual_seed(0)
model = build_detection_model(cfg).to(dev).eval()
clouds = [torch.from_numpy(make_scene(i, 500000)).to(dev) for i in range(4)]
def loop(tag, n=24):
    with torch.no_grad():
        for i in range(4):
            model(list(voxelize(clouds[i % 4], 50, cfg.SPARSE3D.VOXEL_FULL_SCALE)))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for i in range(n):
            model(list(voxelize(clouds[i % 4], 50, cfg.SPARSE3D.VOXEL_FULL_SCALE)))
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
    print(f"{tag}: {1e3 * dt / n:.2f} ms per building", flush=True)
loop("fresh process")
streams = [torch.cuda.Stream(device=dev) for _ in range(8)]
for s in streams:
    with torch.cuda.stream(s):
        torch.zeros(10, device=dev)
torch.cuda.synchronize()
loop("after creating 8 more streams")
bufs = [torch.empty(5_000_000, dtype=torch.float32).pin_memory() for _ in range(12)]
loop("after pinning 240 MB")
import threading
def idle():
    time.sleep(3)
ts = [threading.Thread(target=idle, daemon=True) for _ in range(4)]
[t.start() for t in ts]
loop("with 4 sleeping threads")
import tempfile
from detection_3d_amd.scene_io import ScenePrefetcher
from detection_3d_amd.synthetic import write_scene_file
from detection_3d_amd import engine
d = tempfile.mkdtemp()
files = [write_scene_file(os.path.join(d, f"s{i}.npz"), i, 500000, cfg.INPUT.CLASSES) for i in range(4)]
for pcl, tg, p in ScenePrefetcher(files * 2, cfg.INPUT.CLASSES, 50, device=dev):
    pass
torch.cuda.synchronize()
loop("after one prefetcher pass")
engine.inference(model, cfg, files, dev)
loop("after engine.inference")
torch.cuda.synchronize(); t0 = time.perf_counter()
engine.inference(model, cfg, files * 6, dev)
torch.cuda.synchronize(); print(f"engine.inference: {1e3 * (time.perf_counter() - t0) / 24:.2f} ms per building")
