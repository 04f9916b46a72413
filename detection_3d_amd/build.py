"""Builds libd3d_hip.so (gfx950) in-tree: python -m detection_3d_amd.build"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libd3d_hip.so")
SOURCES = ["grid.hip", "grid_chain.hip", "plan.hip", "geometry_async.hip", "grid_views.hip", "scan_sort.hip", "voxelize.hip",
           "conv.hip", "conv_ws.hip", "conv_bf16.hip", "conv_dw.hip", "bn.hip", "bn_backward.hip", "box_match.hip", "nms.hip", "box_tail.hip",
           "roi_forward.hip", "roi_backward.hip", "roi_backward_det.hip", "rpn_head.hip", "topk.hip",
           "augment.hip", "celllist.hip", "normals.hip", "points_in_boxes.hip", "box_fit.hip", "floorplan.hip", "frame.hip", "downsample.hip", "unproject.hip", "tsdf.hip", "tsdf_mesh.hip", "render.hip", "clean.hip", "planes.hip", "register.hip", "global_align.hip"]
# -ffp-contract=off: the box geometry (box_geometry.inc) shares an arithmetic contract with the CPU oracle
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-std=c++17"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_library(force=False, verbose=False):
    os.makedirs(LIBDIR, exist_ok=True)
    objdir = os.path.join(LIBDIR, "obj")
    os.makedirs(objdir, exist_ok=True)
    headers = [os.path.join(CSRC, "d3d_internal.h"), os.path.join(CSRC, "grid_internal.h"), os.path.join(CSRC, "conv_block.inc"),
               os.path.join(CSRC, "cell_walk.inc"), os.path.join(CSRC, "union_find.inc"), os.path.join(CSRC, "eigen3.inc"), os.path.join(CSRC, "box_geometry.inc"),
               os.path.join(CSRC, "roi_geometry.inc"), os.path.join(CSRC, "depth_frames.inc"), os.path.join(CSRC, "tsdf_volume.inc"),
               os.path.join(HERE, "..", "include", "d3d_hip.h")]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

    def compile_one(src):
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace(".hip", ".o"))
        if force or _stale(o, [s] + headers):
            cmd = [hipcc] + FLAGS + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
        return o

    with ThreadPoolExecutor(max_workers=4) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    if force or _stale(LIB, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", LIB]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv, verbose=True))
