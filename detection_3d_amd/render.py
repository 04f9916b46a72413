"""From a triangle mesh to posed depth frames.  The reference builds its dataset in five steps (gen_house_obj,
gen_cam_images and gen_pcl of data3d/suncg_utils/suncg_preprocess.py): the house mesh, the camera poses, the depth and
colour images, their back-projection and the voxel merge.  It leaves the images to an external OpenGL tool (scn2img);
here `render_depth` is that step on the GPU (libd3d_hip, render.hip): a tile-binned rasteriser whose output is a
DepthFrames, so that unproject, fuse_frames and the serving pipeline take it as they take a scanner's frames, and
`scan_mesh` is the whole chain from a mesh to the detector's nine-column cloud: only the surfaces a camera sees, holes
behind furniture, density falling with distance.

Semantics (include/d3d_hip.h): the pixel-triangle test in homogeneous form, fp64 in a fixed order, two-sided
with closed edges; the smallest z-depth wins a pixel, then the lowest triangle index.  Triangles that cross the camera
plane need no clipping, two triangles sharing an edge lose no pixel centre between them, and the same input gives the
same bits, whatever the order of the triangles and however the frames are split into chunks.

Out of scope: reading .obj, .ply or .json house files (bring tensors); textures and materials; anti-aliasing; sensor
noise; camera placement (scn2cam's heuristics); lens distortion; meshes that do not fit in memory."""
import ctypes
import math

import numpy as np
import torch

from ._cloud import need_gpu, number, run, scratch, whole
from ._lib import DepthFramesDesc, TriangleMeshDesc, lib, ptr, stream_of
from .downsample import DEFAULT_MAX_POINTS, DEFAULT_VOXEL
from .unproject import PIXEL_LIMIT, DepthFrames, fuse_frames

RENDER_KEYS = ("min_depth", "max_depth", "depth_dtype", "depth_scale", "max_scratch_bytes")
_LAST_CHUNKS = []


class TriangleMesh(object):
    """vertices fp32 [V, 3] in world coordinates, triangles int32 [T, 3], vertex_color fp32 or uint8 [V, 3] or None, all on
    one GPU.  An index outside [0, V) or a non-finite vertex is not an error: such a triangle is never hit."""

    def __init__(self, vertices, triangles, vertex_color=None):
        if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
            raise ValueError("TriangleMesh: vertices is a tensor [V, 3]")
        if not isinstance(triangles, torch.Tensor) or triangles.dim() != 2 or triangles.shape[1] != 3:
            raise ValueError("TriangleMesh: triangles is a tensor [T, 3]")
        if vertices.dtype != torch.float32:
            raise ValueError(f"TriangleMesh: vertices are float32, got {vertices.dtype}")
        if triangles.dtype != torch.int32:
            raise ValueError(f"TriangleMesh: triangles are int32, got {triangles.dtype}")
        if vertex_color is not None:
            if not isinstance(vertex_color, torch.Tensor) or tuple(vertex_color.shape) != tuple(vertices.shape):
                raise ValueError(f"TriangleMesh: vertex_color is a tensor [{vertices.shape[0]}, 3] like the vertices, got "
                                 f"{tuple(getattr(vertex_color, 'shape', ()))}")
            if vertex_color.dtype not in (torch.uint8, torch.float32):
                raise ValueError(f"TriangleMesh: vertex_color is uint8 or float32, got {vertex_color.dtype}")
        for t in (vertices, triangles, vertex_color):
            if t is not None:
                need_gpu(t.device)
        for t in (triangles, vertex_color):
            if t is not None and t.device != vertices.device:
                raise ValueError(f"TriangleMesh: vertices on {vertices.device}, another tensor on {t.device}")
        self.vertices = vertices.detach().contiguous()
        self.triangles = triangles.detach().contiguous()
        self.vertex_color = None if vertex_color is None else vertex_color.detach().contiguous()
        vc = self.vertex_color
        self.desc = TriangleMeshDesc(ptr(self.vertices), self.vertices.shape[0], ptr(self.triangles), self.triangles.shape[0],
                                     ptr(vc), int(vc is not None and vc.dtype == torch.uint8))

    @property
    def device(self):
        return self.vertices.device


def _cameras(who, intrinsics, extrinsics):
    extrinsics = torch.as_tensor(extrinsics).to(torch.float64)
    if extrinsics.dim() != 3 or tuple(extrinsics.shape[1:]) not in ((3, 4), (4, 4)):
        raise ValueError(f"{who}: extrinsics are [F, 3, 4] or [F, 4, 4], got {tuple(extrinsics.shape)}")
    f = extrinsics.shape[0]
    intrinsics = torch.as_tensor(intrinsics).to(torch.float64)
    if tuple(intrinsics.shape) == (4,):
        intrinsics = intrinsics.expand(f, 4)
    if tuple(intrinsics.shape) != (f, 4):
        raise ValueError(f"{who}: intrinsics are [{f}, 4] or [4] (fx, fy, cx, cy), got {tuple(intrinsics.shape)}")
    return intrinsics, extrinsics[:, :3, :]


def _check_args(who, mesh, height, width, min_depth, max_depth, depth_dtype, depth_scale, max_scratch_bytes):
    height, width = whole(height, f"{who}: height"), whole(width, f"{who}: width")
    min_depth, max_depth = float(min_depth), float(max_depth)
    if math.isnan(min_depth) or math.isnan(max_depth):
        raise ValueError(f"{who}: min_depth / max_depth is NaN")
    if depth_dtype not in (torch.float32, torch.uint16):
        raise ValueError(f"{who}: depth_dtype is torch.float32 or torch.uint16, got {depth_dtype!r}")
    depth_scale = number(depth_scale, f"{who}: depth_scale", lo_open=True)
    max_scratch_bytes = whole(max_scratch_bytes, f"{who}: max_scratch_bytes")
    if not isinstance(mesh, TriangleMesh):
        raise ValueError(f"{who}: mesh is a TriangleMesh, got {type(mesh).__name__}")
    return height, width, min_depth, max_depth, depth_scale, max_scratch_bytes


class _Call(object):
    """the arguments the three library calls share, for frames [f0, f1)"""

    def __init__(self, mesh, intrinsics, extrinsics, height, width, depth=None, color=None, depth_scale=0.0):
        self.mesh, self.h, self.w, self.dev = mesh, height, width, mesh.device
        self.intr = intrinsics.to(self.dev).contiguous()
        self.extr = extrinsics.to(self.dev).contiguous()
        self.depth, self.color, self.depth_scale = depth, color, depth_scale
        self.info = (ctypes.c_int64 * 1)(0)

    def frames(self, f0, f1):
        """the d3d_depth_frames the calls fill: the cameras and the shape, and for d3d_render_tiles the images"""
        depth, color = (None if t is None else t[f0:f1] for t in (self.depth, self.color))
        return DepthFramesDesc(ptr(depth), int(depth is not None and depth.dtype == torch.uint16), ptr(color),
                               int(color is not None and color.dtype == torch.uint8), ptr(self.intr[f0:f1]),
                               ptr(self.extr[f0:f1]), f1 - f0, self.h, self.w, self.depth_scale)

    def bin(self, f0, f1):
        """-> (scratch, all list entries of the frames)"""
        buf, nbytes = scratch(self.dev, "d3d_render_scratch_bytes", f1 - f0, self.h, self.w)
        run(self.dev, "d3d_render_bin", self.mesh.desc, self.frames(f0, f1), ptr(buf), nbytes, self.info,
            stream_of(self.dev))
        return buf, int(self.info[0])


def frame_scratch_bytes(mesh, intrinsics, extrinsics, height, width):
    """What every frame needs on its own: a list of F byte counts (the tile tables plus 4 bytes per (tile, triangle) list
    entry).  render_depth's max_scratch_bytes must be at least the largest; one read-back per frame."""
    height, width = _check_args("frame_scratch_bytes", mesh, height, width, 0.0, math.inf, torch.float32, 0.001, 1)[:2]
    intrinsics, extrinsics = _cameras("frame_scratch_bytes", intrinsics, extrinsics)
    f = extrinsics.shape[0]
    fixed = lib().d3d_render_scratch_bytes(1, height, width)
    if mesh.vertices.shape[0] == 0 or mesh.triangles.shape[0] == 0:
        return [fixed] * f
    call = _Call(mesh, intrinsics, extrinsics, height, width)
    return [fixed + 4 * call.bin(i, i + 1)[1] for i in range(f)]


def last_chunks():
    """the frame ranges [(f0, f1), ..] the most recent render_depth of this process ran as"""
    return list(_LAST_CHUNKS)


def render_depth(mesh, intrinsics, extrinsics, height, width, min_depth=0.0, max_depth=math.inf,
                 depth_dtype=torch.float32, depth_scale=0.001, return_triangles=False, max_scratch_bytes=1 << 30):
    """mesh: TriangleMesh; intrinsics [F, 4] or [4] (fx, fy, cx, cy) and extrinsics [F, 3, 4] or [F, 4, 4] (camera to
    world, +z forward, x right, y down) as for DepthFrames -> DepthFrames of F images of height x width pixels:
    depth: float32 (the z-depth; 0 where nothing was hit) or uint16 (rint(z / depth_scale); 0 also where that is above
    65535); color, when the mesh has vertex colours: their perspective-correct interpolation, of their type.
    A hit counts when z is finite, z > 0 and min_depth <= z <= max_depth (max_depth: the reference's kinect_max_depth).
    return_triangles: also tri int32 [F, H, W], the triangle every pixel shows, -1 for none: with unproject's
    pixel_of_point it carries a per-face label to every point of the cloud.
    The frames are rendered in chunks of whole frames whose scratch (tile tables and (tile, triangle) lists) stays within
    max_scratch_bytes, with one host read-back per chunk; the result does not depend on the split.  A frame that needs
    more on its own raises ValueError.  No frame, no triangle or no vertex gives empty images without a launch of the
    tile kernel."""
    height, width, min_depth, max_depth, depth_scale, budget = _check_args(
        "render_depth", mesh, height, width, min_depth, max_depth, depth_dtype, depth_scale, max_scratch_bytes)
    intrinsics, extrinsics = _cameras("render_depth", intrinsics, extrinsics)
    f, dev = extrinsics.shape[0], mesh.device
    if f * height * width >= PIXEL_LIMIT:
        raise ValueError(f"render_depth: {f} x {height} x {width} pixels do not fit 31 bits; pass fewer frames per call")
    vc = mesh.vertex_color
    del _LAST_CHUNKS[:]
    if f == 0 or mesh.vertices.shape[0] == 0 or mesh.triangles.shape[0] == 0:
        depth = _zeros((f, height, width), depth_dtype, dev)
        color = None if vc is None else torch.zeros((f, height, width, 3), dtype=vc.dtype, device=dev)
        tri = torch.full((f, height, width), -1, dtype=torch.int32, device=dev)
    else:
        depth = _empty((f, height, width), depth_dtype, dev)
        color = None if vc is None else torch.empty((f, height, width, 3), dtype=vc.dtype, device=dev)
        tri = torch.empty((f, height, width), dtype=torch.int32, device=dev) if return_triangles else None
        call = _Call(mesh, intrinsics, extrinsics, height, width, depth, color, depth_scale)
        scratch_of = lib().d3d_render_scratch_bytes
        if scratch_of(1, height, width) > budget:
            raise ValueError(f"render_depth: one frame of {height} x {width} pixels needs {scratch_of(1, height, width)} "
                             f"bytes of tile tables, max_scratch_bytes is {budget}")
        step = f                                   # frames per chunk: the tables take at most half of the budget ...
        while step > 1 and 2 * scratch_of(step, height, width) > budget:
            step = (step + 1) // 2
        f0 = 0
        while f0 < f:
            f1 = min(f, f0 + step)
            buf, entries = call.bin(f0, f1)
            need = buf.numel() + 4 * entries
            if need > budget or entries >= (1 << 31):
                if f1 - f0 == 1:
                    raise ValueError(f"render_depth: frame {f0} needs {need} bytes of scratch ({entries} list entries of 4 "
                                     f"bytes), max_scratch_bytes is {budget}")
                step = (f1 - f0) // 2              # ... and the lists decide the rest: halve and bin again
                continue
            lists = torch.empty(max(entries, 1), dtype=torch.int32, device=dev)
            s, views = stream_of(dev), call.frames(f0, f1)
            run(dev, "d3d_render_fill", mesh.desc, views, call.info, ptr(buf), buf.numel(), ptr(lists), s)
            run(dev, "d3d_render_tiles", mesh.desc, views, min_depth, max_depth, call.info, ptr(buf), buf.numel(), ptr(lists),
                ptr(None if tri is None else tri[f0:f1]), s)
            _LAST_CHUNKS.append((f0, f1))
            f0 = f1
    frames = DepthFrames(depth, intrinsics, extrinsics, color=color, depth_scale=depth_scale)
    return (frames, tri) if return_triangles else frames


def _empty(shape, dtype, dev):
    if dtype == torch.uint16:                    # allocated as int16: the same bytes, and a dtype every fill takes
        return torch.empty(shape, dtype=torch.int16, device=dev).view(torch.uint16)
    return torch.empty(shape, dtype=dtype, device=dev)


def _zeros(shape, dtype, dev):
    if dtype == torch.uint16:
        return torch.zeros(shape, dtype=torch.int16, device=dev).view(torch.uint16)
    return torch.zeros(shape, dtype=dtype, device=dev)


def scan_mesh(mesh, intrinsics, extrinsics, height, width, voxel=DEFAULT_VOXEL, max_points=DEFAULT_MAX_POINTS, seed=0,
              **render_and_unproject_kw):
    """fuse_frames(render_depth(mesh, ...)): the reference's scn2img, depth_2_pcl and voxel_down_sample in one call ->
    the detector's nine-column cloud fp32 [N, 9] (position, colour, normal facing the camera that saw the point).
    Keywords of render_depth (min_depth, max_depth, depth_dtype, depth_scale, max_scratch_bytes) go to it, the rest to
    unproject; min_depth and max_depth go to both."""
    rkw = {k: render_and_unproject_kw.pop(k) for k in RENDER_KEYS if k in render_and_unproject_kw}
    if "return_triangles" in render_and_unproject_kw:
        raise ValueError("scan_mesh: the voxel mean has no triangle of its own (use render_depth, then unproject)")
    frames = render_depth(mesh, intrinsics, extrinsics, height, width, **rkw)
    for k in ("min_depth", "max_depth"):
        if k in rkw:
            render_and_unproject_kw[k] = rkw[k]
    return fuse_frames(frames, voxel=voxel, max_points=max_points, seed=seed, **render_and_unproject_kw)


_BOX_FACES = ((0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3))


def box_mesh(boxes_yx_zb):
    """Rotated boxes [K, 7] yx_zb (xc, yc, z_bot, d3, d4, dz, yaw; the convention of scene_io and primitives: in the box
    frame lx = c (X - xc) - s (Y - yc) runs along d3 and ly = s (X - xc) + c (Y - yc) along d4) -> (vertices float32
    [8 K, 3], triangles int32 [12 K, 3]) as numpy arrays.  Vertex 8 k + 4 i + 2 j + l of box k is the corner
    (lx, ly, lz) = ((i - 1/2) d3, (j - 1/2) d4, l dz); every face is two triangles wound to face outwards, and every
    box is closed: each of its 18 edges belongs to exactly two triangles.  synthetic.make_targets' walls plus a floor
    and a ceiling slab are a building."""
    b = np.asarray(boxes_yx_zb, dtype=np.float64).reshape(-1, 7)
    k = b.shape[0]
    c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
    vertices = np.zeros((k, 8, 3))
    for i in range(2):
        for j in range(2):
            for l in range(2):
                lx, ly = (i - 0.5) * b[:, 3], (j - 0.5) * b[:, 4]
                vertices[:, 4 * i + 2 * j + l] = np.stack([b[:, 0] + c * lx + s * ly, b[:, 1] - s * lx + c * ly,
                                                           b[:, 2] + l * b[:, 5]], 1)
    one = np.array([t for q in _BOX_FACES for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], dtype=np.int64)
    triangles = (one[None] + 8 * np.arange(k)[:, None, None]).reshape(-1, 3)
    return vertices.reshape(-1, 3).astype(np.float32), triangles.astype(np.int32)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """The camera at `eye` looking at `target` with `up` upwards in the image -> extrinsics fp64 [3, 4] (camera to world)
    in the DepthFrames convention.  With t the unit forward direction and u the unit up direction orthogonal to it, the
    rotation is what suncg_cameras builds from the same two vectors: the columns t x u, -u, t."""
    eye, target, up = (np.asarray(v, dtype=np.float64).reshape(3) for v in (eye, target, up))
    t = target - eye
    n = np.linalg.norm(t)
    if not n > 0.0:
        raise ValueError("look_at: eye and target coincide")
    t = t / n
    right = np.cross(t, up)
    n = np.linalg.norm(right)
    if not n > 0.0:
        raise ValueError("look_at: up is parallel to the viewing direction")
    right = right / n
    u = np.cross(right, t)
    out = np.zeros((3, 4))
    out[:, :3] = np.stack([np.cross(t, u), -u, t], 1)
    out[:, 3] = eye
    return out
