"""Surface fusion of posed depth frames: a truncated signed-distance volume (TSDF) on the GPU and the cloud of its zero
crossing.  `fuse_frames` merges frames by the voxel mean, which averages inside a cell and never across cells: depth
noise thickens a wall to several voxels, and a wrong measurement (a flying pixel, a return through a window) stays in
the cloud however many frames looked straight through that spot.  Here every voxel near a measured surface keeps the
mean, over the frames that saw it, of min(1, (depth at its pixel - its own depth) / trunc): noise averages out across
frames, free space outvotes a stray return, and the gradient of the volume gives each point a normal that faces the
cameras.  KinectFusion-style projective fusion; the reference has nothing like it.

Semantics (include/d3d_hip.h): fp64 arithmetic in a stated order, stored once as fp32, so that the numpy
restatement of tests/tsdf_ref.py gives the same bits.  The voxels live in 8 x 8 x 8 blocks found through a hash; block
ids depend on scheduling, every output is ordered by block coordinate and so does not.  One call of F frames and F calls
of one frame may differ in the last bit (the mean is folded into fp32 once per call).  Weights count observations, exact
up to 2^24 per voxel.

Out of scope: weights other than 1 per observation; a weight cap for moving scenes; ray-exact block allocation (a block
that the voxel-spaced samples of every ray miss is not allocated); growing max_blocks (a volume that runs full raises
and wants reset()).

TsdfVolume.mesh() gives the zero crossing as a render.TriangleMesh (marching tetrahedra; the restatement is
tests/tsdf_mesh_ref.py), TsdfVolume.from_blocks() is the inverse of blocks(), fuse_frames_mesh() is around, integrate,
mesh.  Out of scope there: writing .ply or .obj files, mesh simplification, vertex normals, dropping the vertices that
no triangle refers to."""
import ctypes
import math

import torch

from ._cloud import need_gpu, number, run, same_device, scratch, whole
from ._lib import D3DError, DepthFramesDesc, TsdfVolumeDesc, lib, ptr, stream_of
from .downsample import DEFAULT_MAX_POINTS, DEFAULT_VOXEL, cap_points
from .render import TriangleMesh
from .unproject import COLUMNS, DepthFrames

MAX_BLOCKS = 1 << 22
MAX_REACH = 256
BLOCK_VOXELS = 512


def _check_integrate(step=1, min_depth=0.0, max_depth=math.inf, color_div=256.0):
    step = whole(step, "tsdf: step")
    min_depth, max_depth = float(min_depth), float(max_depth)
    if math.isnan(min_depth) or math.isnan(max_depth):
        raise ValueError("tsdf: min_depth / max_depth is NaN")
    return step, min_depth, max_depth, number(color_div, "tsdf: color_div", lo_open=True)


def _check_volume(voxel, trunc):
    voxel = number(voxel, "tsdf: voxel", lo_open=True)
    trunc = 4.0 * voxel if trunc is None else number(trunc, "tsdf: trunc", lo_open=True)
    if not math.ceil(trunc / voxel) <= MAX_REACH:
        raise ValueError(f"tsdf: trunc {trunc} is more than {MAX_REACH} voxels of {voxel}")
    return voxel, trunc


def _need_frames(frames, who):
    if not isinstance(frames, DepthFrames):
        raise ValueError(f"{who}: frames is a DepthFrames, got {type(frames).__name__}")


class TsdfVolume(object):
    """A volume of voxel edge `voxel` whose voxel (0, 0, 0) sits at `origin`; trunc: the truncation distance, default
    4 voxel; max_blocks: the storage, in blocks of 8^3 voxels, allocated as the volume fills; color: keep a mean colour
    per voxel (frames without a colour image leave it untouched).  Block coordinates are 16 bits per axis: the volume
    spans 65536 x 8 voxels from the origin, and what falls outside is dropped and sets `clipped`."""

    def __init__(self, voxel=DEFAULT_VOXEL, trunc=None, origin=(0.0, 0.0, 0.0), max_blocks=1 << 18, color=True, device=None):
        self.voxel, self.trunc = _check_volume(voxel, trunc)
        try:
            origin = tuple(origin)
        except TypeError:
            origin = ()
        if len(origin) != 3:
            raise ValueError("tsdf: origin is three numbers")
        self.origin = tuple(number(o, "tsdf: origin", lo=-math.inf) for o in origin)
        self.max_blocks = whole(max_blocks, "tsdf: max_blocks", 1, MAX_BLOCKS)
        self.color = bool(color)
        self.device = None if device is None else torch.device(device)
        if self.device is not None:
            need_gpu(self.device, "the volume")
        self.count_cull = False                  # scripts/tsdf_probe.py: count the (block, frame) pairs the cull removes
        self._table = None
        self.reset()

    def reset(self):
        """An empty volume again; also what a volume that ran full needs before its next call."""
        self.n_blocks, self.clipped, self._full, self._order = 0, False, False, None
        self.culled_pairs = self.pairs = 0
        if self._table is not None:
            self._table.fill_(0xFF)
            self._state.zero_()
        return self

    # ---- storage ----
    def _on(self, dev):
        if self.device is not None and (self.device.type != dev.type or self.device.index not in (None, dev.index)):
            raise ValueError(f"tsdf: the volume is on {self.device}, the frames on {dev}")
        self.device = dev
        if self._table is None:
            self._slots = lib().d3d_tsdf_table_slots(self.max_blocks)
            self._table = torch.full((self._slots, 16), 0xFF, dtype=torch.uint8, device=dev)
            self._state = torch.zeros(4, dtype=torch.int32, device=dev)
            self._coords = torch.empty((self.max_blocks, 3), dtype=torch.int32, device=dev)
            self._tsdf = self._weight = self._color = self._cweight = None
            self._cap = 0
        return dev

    def _reserve(self, n):
        """room for n blocks of voxel state; the first n_blocks blocks keep theirs"""
        if n <= self._cap:
            return
        cap, keep, dev = min(self.max_blocks, max(n, 2 * self._cap, 64)), self.n_blocks, self.device

        def grown(old, *tail):
            new = torch.empty((cap, BLOCK_VOXELS) + tail, dtype=torch.float32, device=dev)
            if old is not None and keep:
                new[:keep] = old[:keep]
            return new

        self._tsdf, self._weight = grown(self._tsdf), grown(self._weight)
        if self.color:
            self._color, self._cweight = grown(self._color, 3), grown(self._cweight)
        self._cap = cap

    def _desc(self, n_blocks=None, order=None):
        """the library's d3d_tsdf_volume of the state as it is now; n_blocks: the count a pass is about to commit"""
        return TsdfVolumeDesc(self.voxel, self.trunc, self.origin, ptr(self._table), self._slots, ptr(self._coords),
                              self.max_blocks, self.n_blocks if n_blocks is None else n_blocks, ptr(self._state),
                              ptr(order), ptr(self._tsdf), ptr(self._weight), ptr(self._color), ptr(self._cweight))

    def _alive(self, who):
        if self._full:
            raise D3DError(f"{who}: the volume ran out of its {self.max_blocks} blocks; its contents are unspecified "
                           "until reset() (pass a larger max_blocks or voxel)")

    # ---- fusion ----
    def integrate(self, frames, step=1, min_depth=0.0, max_depth=math.inf, color_div=256.0):
        """Fuses a batch of frames (DepthFrames) and returns the volume.  Allocates the blocks within trunc of every kept
        pixel's measurement along its ray (a pixel is kept as in unproject: valid depth, u and v multiples of `step`), then
        updates every voxel of every block, old and new, from every valid pixel of the frames in order (step plays no
        part there).  A voxel that from_blocks() gave a tsdf of NaN or +-inf keeps it: (w NaN + S) / (w + n).  One host
        read-back (the block count).  Raises D3DError when the blocks run out; the volume then
        raises on every call until reset()."""
        step, min_depth, max_depth, color_div = _check_integrate(step, min_depth, max_depth, color_div)
        _need_frames(frames, "tsdf.integrate")
        self._alive("tsdf.integrate")
        if frames.depth.numel() == 0:
            return self
        first_new = self.n_blocks
        n = self._touch(frames, step, min_depth, max_depth)
        self._update(frames, n, first_new, min_depth, max_depth, color_div)
        return self

    def _touch(self, frames, step, min_depth, max_depth):
        """the allocation pass and the call's read-back -> the number of blocks now allocated"""
        dev = self._on(frames.device)
        info = (ctypes.c_int * 3)(0, 0, 0)
        reach = int(math.ceil(self.trunc / self.voxel))
        run(dev, "d3d_tsdf_touch", frames.desc, step, min_depth, max_depth, self._desc(), reach, info, stream_of(dev))
        n, clipped, full = int(info[0]), bool(info[1]), bool(info[2])
        self.clipped = self.clipped or clipped
        if full:
            self._full = True
            self._alive("tsdf.integrate")
        return n

    def _update(self, frames, n, first_new, min_depth, max_depth, color_div):
        """the integration pass over blocks [0, n), of which [first_new, n) are new; asynchronous"""
        dev = self.device
        f, h, w = frames.shape
        self._reserve(n)
        color = frames.color if self.color else None
        culled = torch.zeros(1, dtype=torch.int64, device=dev) if self.count_cull else None
        if n > 0:
            desc = frames.desc
            if color is not frames.color:        # a volume without colour does not read the images
                desc = DepthFramesDesc.from_buffer_copy(desc)
                desc.color = None
            run(dev, "d3d_tsdf_integrate", desc, min_depth, max_depth, color_div, self._desc(n), first_new,
                ptr(culled), stream_of(dev))
        self.n_blocks, self._order = n, None
        if culled is not None:
            self.culled_pairs += int(culled.item())
            self.pairs += n * f

    def _sorted(self):
        """the block ids in ascending (x, y, z) of their coordinates, int32 [n_blocks]"""
        if self._order is None:
            dev, n = self.device, self.n_blocks
            order = torch.empty((n,), dtype=torch.int32, device=dev)
            buf, nbytes = scratch(dev, "d3d_tsdf_order_scratch_bytes", n)
            run(dev, "d3d_tsdf_order", ptr(self._coords), n, ptr(order), ptr(buf), nbytes, stream_of(dev))
            self._order = order
        return self._order

    def blocks(self):
        """-> (coords int32 [B, 3] ascending in (x, y, z), tsdf, weight fp32 [B, 8, 8, 8], color fp32 [B, 8, 8, 8, 3],
        color_weight fp32 [B, 8, 8, 8]; the last two None for a volume without colour): copies, indexed [x, y, z] inside a
        block.  A voxel no frame has seen has weight 0."""
        self._alive("tsdf.blocks")
        if self.n_blocks == 0:
            if self.device is None:
                raise D3DError("tsdf.blocks: the volume has seen no frame and has no device yet")
            empty = lambda *s: torch.empty(s, dtype=torch.float32, device=self.device)
            return (torch.empty((0, 3), dtype=torch.int32, device=self.device), empty(0, 8, 8, 8), empty(0, 8, 8, 8),
                    empty(0, 8, 8, 8, 3) if self.color else None, empty(0, 8, 8, 8) if self.color else None)
        order = self._sorted().long()
        pick = lambda t, *tail: None if t is None else t.index_select(0, order).view(-1, 8, 8, 8, *tail)
        return (self._coords.index_select(0, order), pick(self._tsdf), pick(self._weight), pick(self._color, 3),
                pick(self._cweight))

    def surface_points(self, columns=9, min_weight=1, return_voxels=False):
        """The zero crossing as a cloud: fp32 [N, columns], one row per edge between a voxel and its +x, +y or +z
        neighbour, both seen by at least min_weight observations, whose tsdf values differ in sign: the position
        interpolated along the edge; with columns >= 6 the interpolated colour; with columns == 9 the unit gradient of
        the volume at the voxel, which faces the cameras, or (0, 0, 0) where a forward neighbour is missing or
        truncated.  Rows in (block coordinate, voxel, axis) order.  return_voxels: also the voxel g of every row, int32
        [N, 3].  One host read-back (N)."""
        if columns not in COLUMNS:
            raise ValueError(f"tsdf: columns is 3 (position), 6 (+ colour) or 9 (+ normal), got {columns!r}")
        min_weight = number(min_weight, "tsdf: min_weight")
        self._alive("tsdf.surface_points")
        dev, n = self.device, self.n_blocks
        if dev is None:
            raise D3DError("tsdf.surface_points: the volume has seen no frame and has no device yet")
        info = (ctypes.c_int * 1)(0)
        if n > 0:
            order = self._sorted()
            buf, nbytes = scratch(dev, "d3d_tsdf_surface_scratch_bytes", n)
            vol = self._desc(order=order)
            run(dev, "d3d_tsdf_surface_count", vol, min_weight, ptr(buf), nbytes, info, stream_of(dev))
        rows = int(info[0])
        out = torch.empty((rows, int(columns)), dtype=torch.float32, device=dev)
        voxels = torch.empty((rows, 3), dtype=torch.int32, device=dev) if return_voxels else None
        if rows > 0:
            run(dev, "d3d_tsdf_surface_rows", vol, min_weight, int(columns), info, ptr(buf), nbytes, ptr(out), ptr(voxels),
                stream_of(dev))
        return (out, voxels) if return_voxels else out

    def mesh(self, min_weight=1, color=True, return_edges=False):
        """The zero crossing as a render.TriangleMesh: marching tetrahedra on the Kuhn split of every cell whose eight
        voxels are allocated and seen by at least min_weight observations.  One vertex per crossed edge from a voxel g to
        g + e, e one of x, y, z, xy, xz, yz, xyz (kinds 0..6; kinds 0..2 are surface_points' rows), in (block coordinate,
        voxel, kind) order; a vertex none of whose cells is emitted stays in the list, unreferenced.  Triangles int32 [T,
        3] in (block coordinate, voxel, tetrahedron) order, counter-clockwise seen from free space.  vertex_color fp32
        [V, 3], or None for a volume without colour or with color=False.  return_edges: also int32 [V, 4], the voxel g and
        the kind of every vertex.  One host read-back (V and T); D3DError when either is past 2^31 - 1."""
        min_weight = number(min_weight, "tsdf: min_weight")
        self._alive("tsdf.mesh")
        dev, n = self.device, self.n_blocks
        if dev is None:
            raise D3DError("tsdf.mesh: the volume has seen no frame and has no device yet")
        info = (ctypes.c_int * 2)(0, 0)
        if n > 0:
            order = self._sorted()
            buf, nbytes = scratch(dev, "d3d_tsdf_mesh_scratch_bytes", n)
            vol = self._desc(order=order)
            run(dev, "d3d_tsdf_mesh_count", vol, min_weight, ptr(buf), nbytes, info, stream_of(dev))
        nv, nt = int(info[0]), int(info[1])
        vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        triangles = torch.empty((nt, 3), dtype=torch.int32, device=dev)
        colors = torch.empty((nv, 3), dtype=torch.float32, device=dev) if color and self.color else None
        edges = torch.empty((nv, 4), dtype=torch.int32, device=dev) if return_edges else None
        if nv > 0:
            run(dev, "d3d_tsdf_mesh_vertices", vol, info, ptr(buf), nbytes, ptr(vertices), ptr(colors), ptr(edges),
                stream_of(dev))
        if nt > 0:
            run(dev, "d3d_tsdf_mesh_triangles", vol, info, ptr(buf), nbytes, ptr(triangles), stream_of(dev))
        mesh = TriangleMesh(vertices, triangles, colors)
        return (mesh, edges) if return_edges else mesh

    @classmethod
    def from_blocks(cls, coords, tsdf, weight, color=None, color_weight=None, voxel=DEFAULT_VOXEL, trunc=None,
                    origin=(0.0, 0.0, 0.0), max_blocks=None):
        """The inverse of blocks(): a volume that holds the given blocks, in any order.  coords int32 [B, 3] in [0,
        65536), no coordinate twice; tsdf, weight fp32 [B, 8, 8, 8]; color fp32 [B, 8, 8, 8, 3] and color_weight fp32 [B,
        8, 8, 8], both or neither (neither: a volume without colour); all on one GPU.  max_blocks: None for max(B, 2^18).
        integrate() afterwards finds the blocks and carries on.  Any fp32 state is taken as it is; a voxel whose tsdf is
        NaN or +-inf is not seen by surface_points() and mesh() at any min_weight, whatever its weight, and integrate()
        keeps it (the mean of a NaN stays NaN).  The host waits for the checks of the coordinates (two
        torch expressions) and for the insertion's read-back."""
        voxel, trunc = _check_volume(voxel, trunc)

        def need(t, what, shape, dtype):
            if not isinstance(t, torch.Tensor) or t.dim() != len(shape) or \
                    any(s is not None and t.shape[i] != s for i, s in enumerate(shape)):
                raise ValueError(f"tsdf.from_blocks: {what} is a tensor [{', '.join('B' if s is None else str(s) for s in shape)}]")
            if t.dtype != dtype:
                raise ValueError(f"tsdf.from_blocks: {what} is {dtype}, got {t.dtype}")
            return t.detach()

        coords = need(coords, "coords", (None, 3), torch.int32)
        n = coords.shape[0]
        tsdf = need(tsdf, "tsdf", (n, 8, 8, 8), torch.float32)
        weight = need(weight, "weight", (n, 8, 8, 8), torch.float32)
        if (color is None) != (color_weight is None):
            raise ValueError("tsdf.from_blocks: color and color_weight go together")
        if color is not None:
            color = need(color, "color", (n, 8, 8, 8, 3), torch.float32)
            color_weight = need(color_weight, "color_weight", (n, 8, 8, 8), torch.float32)
        same_device(coords=coords, tsdf=tsdf, weight=weight, color=color, color_weight=color_weight)
        max_blocks = max(n, 1 << 18) if max_blocks is None else whole(max_blocks, "tsdf: max_blocks", 1, MAX_BLOCKS)
        if n > max_blocks:
            raise ValueError(f"tsdf.from_blocks: {n} blocks and max_blocks {max_blocks}")
        vol = cls(voxel=voxel, trunc=trunc, origin=origin, max_blocks=max_blocks, color=color is not None)
        if n > 0:
            c = coords.long()
            if bool(((c < 0) | (c > 0xFFFF)).any()):
                raise ValueError("tsdf.from_blocks: a block coordinate outside [0, 65536)")
            if torch.unique((c[:, 0] << 32) | (c[:, 1] << 16) | c[:, 2]).numel() != n:
                raise ValueError("tsdf.from_blocks: a block coordinate is given twice")
        need_gpu(coords.device, "the blocks")
        dev = vol._on(coords.device)
        if n > 0:
            try:
                run(dev, "d3d_tsdf_insert_blocks", ptr(coords.contiguous()), n, vol._desc(), stream_of(dev))
            except D3DError:
                vol.reset()
                raise
            vol._reserve(n)
            vol._tsdf[:n] = tsdf.reshape(n, BLOCK_VOXELS)
            vol._weight[:n] = weight.reshape(n, BLOCK_VOXELS)
            if color is not None:
                vol._color[:n] = color.reshape(n, BLOCK_VOXELS, 3)
                vol._cweight[:n] = color_weight.reshape(n, BLOCK_VOXELS)
            vol.n_blocks = n
        return vol

    @property
    def state_bytes(self):
        """bytes of voxel state, table and coordinates held on the device"""
        held = (self._table, self._coords, self._tsdf, self._weight, self._color, self._cweight) if self._table is not None else ()
        return sum(t.numel() * t.element_size() for t in held if t is not None)

    @classmethod
    def around(cls, frames, voxel=DEFAULT_VOXEL, trunc=None, min_depth=0.0, max_depth=math.inf, **volume_kw):
        """A volume whose origin lies below everything the frames measure: the per-axis minimum of their unprojected
        valid pixels (plain torch, fp64, one host read-back) less trunc and one block.  volume_kw: max_blocks, color."""
        voxel, trunc = _check_volume(voxel, trunc)
        _, min_depth, max_depth, _ = _check_integrate(1, min_depth, max_depth)
        _need_frames(frames, "TsdfVolume.around")
        f, h, w = frames.shape
        dev = frames.device
        lo = torch.full((3,), math.inf, dtype=torch.float64, device=dev)
        u = torch.arange(w, dtype=torch.float64, device=dev)[None, None, :]
        v = torch.arange(h, dtype=torch.float64, device=dev)[None, :, None]
        for a in range(0, f if h * w else 0, 8):
            d = frames.depth[a:a + 8]
            if d.dtype == torch.uint16:
                z = (d.view(torch.int16).to(torch.int32) & 0xFFFF).to(torch.float64) * frames.depth_scale
            else:
                z = d.to(torch.float64)
            valid = torch.isfinite(z) & (z > 0) & (z >= min_depth) & (z <= max_depth)
            fx, fy, cx, cy = (frames.intrinsics[a:a + 8, j][:, None, None] for j in range(4))
            cam = ((u - cx) * (z / fx), (v - cy) * (z / fy), z)
            E = frames.extrinsics[a:a + 8]
            world = torch.stack([sum(E[:, k, j][:, None, None] * cam[j] for j in range(3)) + E[:, k, 3][:, None, None]
                                 for k in range(3)])
            world = torch.where(valid[None], world, torch.full_like(world, math.inf))
            lo = torch.minimum(lo, world.amin(dim=(1, 2, 3)))
        lo = lo.cpu().tolist()
        origin = tuple(x - (trunc + 8.0 * voxel) if math.isfinite(x) else 0.0 for x in lo)
        return cls(voxel=voxel, trunc=trunc, origin=origin, device=dev, **volume_kw)


def frames_slice(frames, first, last):
    """frames [first, last) of a DepthFrames as a DepthFrames (views, no copy)"""
    return DepthFrames(frames.depth[first:last], frames.intrinsics[first:last], frames.extrinsics[first:last],
                       None if frames.color is None else frames.color[first:last], frames.depth_scale)


def fuse_frames_tsdf(frames, voxel=DEFAULT_VOXEL, trunc=None, max_points=DEFAULT_MAX_POINTS, seed=0, batch=None,
                     min_weight=1, max_blocks=1 << 18, **integrate_kw):
    """fuse_frames with a surface in place of the voxel mean: TsdfVolume.around(frames, voxel, trunc), integrate in
    batches of `batch` frames (None: all at once), surface_points(9, min_weight), then downsample.cap_points(max_points,
    seed) (None skips the cap).  The result is the detector's nine-column input, one point per crossed voxel edge.
    integrate_kw: step, min_depth, max_depth, color_div."""
    integrate_kw = dict(zip(("step", "min_depth", "max_depth", "color_div"), _check_integrate(**integrate_kw)))
    _need_frames(frames, "fuse_frames_tsdf")
    f = frames.shape[0]
    batch = f if batch is None else whole(batch, "fuse_frames_tsdf: batch")
    volume = TsdfVolume.around(frames, voxel, trunc, integrate_kw["min_depth"], integrate_kw["max_depth"],
                               max_blocks=max_blocks, color=frames.color is not None)
    for a in range(0, f, max(batch, 1)):
        volume.integrate(frames_slice(frames, a, min(a + batch, f)), **integrate_kw)
    cloud = volume.surface_points(9, min_weight)
    return cloud if max_points is None else cap_points(cloud, max_points, seed)


def fuse_frames_mesh(frames, voxel=DEFAULT_VOXEL, trunc=None, batch=None, min_weight=1, max_blocks=1 << 18, **integrate_kw):
    """Posed depth frames to a surface mesh: TsdfVolume.around(frames, voxel, trunc), integrate in batches of `batch`
    frames (None: all at once), mesh(min_weight) -> a render.TriangleMesh, coloured when the frames are.  integrate_kw:
    step, min_depth, max_depth, color_div."""
    integrate_kw = dict(zip(("step", "min_depth", "max_depth", "color_div"), _check_integrate(**integrate_kw)))
    min_weight = number(min_weight, "tsdf: min_weight")
    _need_frames(frames, "fuse_frames_mesh")
    f = frames.shape[0]
    batch = f if batch is None else whole(batch, "fuse_frames_mesh: batch")
    volume = TsdfVolume.around(frames, voxel, trunc, integrate_kw["min_depth"], integrate_kw["max_depth"],
                               max_blocks=max_blocks, color=frames.color is not None)
    for a in range(0, f, max(batch, 1)):
        volume.integrate(frames_slice(frames, a, min(a + batch, f)), **integrate_kw)
    return volume.mesh(min_weight)
