"""Data-parallel training of the detector, one process per GPU (BASELINE.json configs[3]: configs/3G6c fpn4321 bs=1 x N,
RCCL gradient all-reduce over xGMI; tools/train_net_sparse3d.py:52-57,170-177 + engine/trainer_sparse3d.py).

    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        scripts/train_ddp.py --config 3G6c_Fpn4321 --steps 20 [--data DIR | --scenes 8 --points 500000] [--ims-per-gpu 2]
        [--deterministic [--seed S]] [--bf16] [--bf16-heads] [--augment flip,rotate[=quarter|free],scale=Z,offset,...]
        [--estimate-normals[=radius,max_nn]] [--downsample V[,MAX_POINTS]] [--clean SPEC]

Every rank reads its own buildings (files[rank::world]) through scene_io.ScenePrefetcher, runs forward + backward (DDP
all-reduces ~128 MB of fp32 gradients bucket by bucket during the backward pass; the never-used top-down modules are
frozen so that no per-step graph search is needed), SGD step, LR schedule; the 4-12 loss scalars are reduced to rank 0
for logging.  Rank 0 prints one JSON line: buildings/s over all ranks (max-over-ranks time), ms per step, last losses.
The process group is created BEFORE anything touches the GPU."""
import argparse
import json
import os
import sys
import tempfile

WORLD = max(1, int(os.environ.get("WORLD_SIZE", "1")))
os.environ.setdefault("OMP_NUM_THREADS", str(max(1, min(8, (os.cpu_count() or 1) // WORLD))))   # ranks share the host

import torch                               # noqa: E402
import torch.distributed as dist           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="3G6c_Fpn4321")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--data", default=None, help="directory of scene files (.pth / .npz); default: synthetic scenes")
    ap.add_argument("--scenes", type=int, default=0, help="synthetic scenes to write (default: 2 per rank)")
    ap.add_argument("--points", type=int, default=500_000)
    ap.add_argument("--log-every", type=int, default=0)
    ap.add_argument("--ims-per-gpu", type=int, default=1,
                    help="buildings per rank and step (IMS_PER_BATCH = ranks x this; the LR schedule counts with it)")
    ap.add_argument("--verify", action="store_true",
                    help="after the steps: compare the weights of all ranks and gather the detections of every scene")
    ap.add_argument("--deterministic", action="store_true",
                    help="torch.use_deterministic_algorithms(True): the same losses and weights in every run of the "
                         "same world size (the library's backward ops take their fixed-order forms)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the weights and of the samplers")
    ap.add_argument("--bf16", action="store_true",
                    help="train the sparse backbone in bf16 storage (fp32 accumulation, fp32 weights, statistics and "
                         "optimizer state; the heads stay fp32 unless --bf16-heads)")
    ap.add_argument("--bf16-heads", action="store_true",
                    help="run the RPN head, RoI pooling and box head on bf16 operands (model.head_dtype; fp32 weights, "
                         "statistics, outputs of the heads and losses); combinable with --bf16")
    ap.add_argument("--augment", default="",
                    help="augment every training building on the GPU (detection_3d_amd.augment): a comma list of flip, "
                         "rotate[=quarter|free], scale=Z, offset, elastic, color=S; seeded from --seed (+ 1000003 x rank)")
    ap.add_argument("--estimate-normals", nargs="?", const="", default=None, metavar="RADIUS[,MAX_NN]",
                    help="estimate the normal columns of every building on the GPU before it is voxelised and augmented "
                         "(detection_3d_amd.normals; files that hold xyz, or xyz and colour); default 0.1,50")
    ap.add_argument("--crop", default="", metavar="SX,SY",
                    help="cut every training building to a random window of SX x SY metres on the GPU and crop or drop its "
                         "boxes by the points that remain (detection_3d_amd.primitives); seeded from --seed (+ 1000003 x rank)")
    ap.add_argument("--downsample", default=None, metavar="V[,MAX_POINTS]",
                    help="reduce every raw building to one point per voxel of V metres on the GPU and, with MAX_POINTS, "
                         "to a random subset of at most that many (detection_3d_amd.downsample), before the normals; "
                         "the cap is seeded from --seed")
    ap.add_argument("--clean", default=None, metavar="SPEC",
                    help="remove outliers and small detached components of every building on the GPU after the "
                         "down-sampling and before the normals (detection_3d_amd.clean): comma-separated radius=R, "
                         "neighbors=M, statistical=K:RATIO, component=C (points, or a share with a decimal point)")
    args = ap.parse_args(argv)
    from detection_3d_amd.clean import parse_clean
    from detection_3d_amd.downsample import parse_downsample
    from detection_3d_amd.normals import parse_estimate_normals
    args.normals = parse_estimate_normals(args.estimate_normals)
    args.downsample = parse_downsample(args.downsample)
    args.clean = parse_clean(args.clean)
    if args.downsample is not None:
        args.downsample["seed"] = int(getattr(args, "seed", 0) or 0)
    return args


def seed_everything(args):
    """Before the model is built: the torch flag (with --deterministic) and the seeds of the initial weights and of
    the samplers (torch.randperm on the device draws from torch's generator)."""
    if args.deterministic:
        torch.use_deterministic_algorithms(True)
    torch.manual_seed(args.seed)          # same initial weights on every rank (DDP also broadcasts rank 0's)


def main():
    args = parse_args()
    rank, local_rank = int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group(backend=os.environ.get("D3D_DIST_BACKEND", "nccl"), init_method="env://", rank=rank,
                            world_size=WORLD)     # nccl = RCCL; gloo: rehearsals of N ranks on one GPU
    local_rank %= max(1, torch.cuda.device_count())     # (several ranks on one GPU only in gloo rehearsals)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    torch.set_num_threads(int(os.environ["OMP_NUM_THREADS"]))

    from detection_3d_amd import _lib, engine
    _lib.lib()
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.detector import build_detection_model
    from detection_3d_amd.synthetic import write_scene_file

    cfg = get_cfg(args.config)
    if args.data:
        files = sorted(os.path.join(args.data, f) for f in os.listdir(args.data) if f.endswith((".pth", ".npz")))
    else:
        n = args.scenes or 2 * WORLD * max(1, args.ims_per_gpu)
        tmp = os.path.join(tempfile.gettempdir(), f"d3d_train_scenes_{os.environ.get('MASTER_PORT', '0')}")
        files = [os.path.join(tmp, f"scene_{i}.npz") for i in range(n)]
        if rank == 0:
            os.makedirs(tmp, exist_ok=True)
            for i, f in enumerate(files):
                if not os.path.exists(f):
                    write_scene_file(f, i, args.points, cfg.INPUT.CLASSES)
        dist.barrier()
    from detection_3d_amd.augment import parse_augment
    augment = parse_augment(args.augment, args.seed)
    from detection_3d_amd.primitives import parse_crop
    crop = parse_crop(args.crop, args.seed)
    seed_everything(args)
    model = build_detection_model(cfg).to(dev)
    if args.bf16:
        model.backbone.compute_dtype = torch.bfloat16
    if args.bf16_heads:
        model.head_dtype = torch.bfloat16
    out = engine.train(model, cfg, files, dev, args.steps, local_rank=local_rank, log_every=args.log_every,
                       ims_per_gpu=args.ims_per_gpu, augment=augment, normals=args.normals, crop=crop,
                       downsample=args.downsample, clean=args.clean)
    if args.verify:
        # (1) the averaged-gradient steps leave every rank with the same weights (fingerprint: sum and sum of squares of
        # every parameter in fp64); (2) the sharded inference loop returns every scene's detections on rank 0
        with torch.no_grad():
            fp = torch.stack([torch.stack([p.detach().double().sum(), (p.detach().double() ** 2).sum()])
                              for p in model.parameters()]).reshape(-1)
        if dist.get_backend() == "gloo":
            fp = fp.cpu()
        fps = [torch.empty_like(fp) for _ in range(WORLD)]
        dist.all_gather(fps, fp)
        out["weights_equal"] = bool(all(torch.equal(fps[0], f) for f in fps))
        res = engine.inference(model, cfg, files, dev, normals=args.normals, downsample=args.downsample,
                               clean=args.clean)
        if rank == 0:
            dets, gts = res
            out["scenes_gathered"] = sorted(int(k) for k in dets)
            out["detections_per_scene"] = [int(dets[k]["bbox3d"].shape[0]) for k in sorted(dets)]
            out["gt_per_scene"] = [int(gts[k]["bbox3d"].shape[0]) for k in sorted(gts)]
    if rank == 0:
        out.update(config=args.config, n_gpus=WORLD, deterministic=args.deterministic, bf16=args.bf16,
                   bf16_heads=args.bf16_heads, augment=repr(augment) if augment is not None else None,
                   normals=args.normals, downsample=args.downsample, clean=args.clean, crop=repr(crop) if crop is not None else None,
                   points_per_building=args.points if not args.data else None,
                   unit="buildings/s", metric="training buildings/sec (forward + backward + SGD, DDP)")
        print(json.dumps(out), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
