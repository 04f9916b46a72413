"""Training-time augmentation of a scene on the GPU: x flip, rotation about z, isotropic scale, elastic distortion, a
random origin offset inside the lattice and colour noise -- the knobs of data3d/suncg_utils/suncg_dataset.py:113-142,
which the reference has hard-wired off (:78-83).  The per-point work runs in libd3d_hip (augment.hip), folded into the
passes of d3d_voxelize; the host draws the per-scene parameters and moves the ground-truth boxes.

Deviations from the reference, on purpose:
- zoom is an isotropic scale s ~ U[1 - z, 1 + z]; the reference's `eye + randn * zoom` shears, and boxes could not
  follow it;
- normals are multiplied by F Rz (the reference leaves them unrotated, wrong once rotation is on);
- the boxes follow flip, rotation, scale and shift (the reference moves them by the shift only); they do NOT follow the
  elastic distortion, as in the reference;
- 'quarter' rotations use exact cos / sin (0, +-1), so that a quarter turn maps the lattice onto itself.

Points are in voxel units: a = xyz . M with M = (I f s scale) @ Rz(theta), built in fp64 in that order.
"""
import ctypes
import math
from collections import namedtuple

import numpy as np
import torch

from ._lib import AugmentParams, check, ints, lib, ptr, require_gpu, stream_of
from .config import class_to_label
from .scene_io import _ZERO_YAW_CLASSES, limit_period, set_yaw_zero

ROTATIONS = ("none", "quarter", "free")
# suncg_dataset.py:22,36-37: the file's columns of each element; the prefetcher keeps the sorted selection
_ELEMENT_IDS = {"xyz": [0, 1, 2], "color": [3, 4, 5], "normal": [6, 7, 8]}
_QUARTER = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))      # (cos, sin) of k pi / 2
RANK_SEED_STRIDE = 1000003

Params = namedtuple("Params", "flip scale k theta u1 u2 color elastic_seed")
Params.__doc__ = """One scene's draws: flip (+1 / -1), scale s, quarter index k (-1 unless 'quarter'), theta (rad),
u1 / u2 (origin offset, U[0,1)^3), color (fp64 offsets of the 3 colour columns), elastic_seed (device generator)."""


def element_columns(elements):
    """-> {element: its first column} after the column selection of suncg_dataset.py:36-37,146."""
    ids = sorted(i for e in elements for i in _ELEMENT_IDS[e])
    return {e: ids.index(_ELEMENT_IDS[e][0]) for e in elements}


def sample_params(gen, rotate="none", flip_x=False, scale_jitter=0.0, origin_offset=False, color_noise=0.0):
    """Draws one scene's parameters from the host torch.Generator `gen`.  Every draw is taken whatever is switched on, in
    a fixed order, so that switching one knob leaves the others' values unchanged.  -> Params."""
    if rotate not in ROTATIONS:
        raise ValueError(f"rotate must be one of {ROTATIONS}, got {rotate!r}")
    u = torch.rand(9, dtype=torch.float64, generator=gen).numpy()
    k = int(torch.randint(0, 4, (1,), generator=gen).item())
    c = torch.randn(3, dtype=torch.float64, generator=gen).numpy()
    eseed = int(torch.randint(0, 2 ** 62, (1,), generator=gen, dtype=torch.int64).item())
    flip = -1.0 if (flip_x and u[0] < 0.5) else 1.0
    z = float(scale_jitter)
    s = (1.0 - z) + (2.0 * z) * float(u[1]) if z > 0 else 1.0
    if rotate == "quarter":
        theta = k * (math.pi / 2)
    elif rotate == "free":
        k, theta = -1, float(u[2]) * (2 * math.pi)
    else:
        k, theta = 0, 0.0
    u1, u2 = (u[3:6].copy(), u[6:9].copy()) if origin_offset else (np.zeros(3), np.zeros(3))
    color = c * float(color_noise) if color_noise else np.zeros(3)
    return Params(flip, s, k, theta, u1, u2, color, eseed)


def rotation_z(p):
    """Rz = [[c, s, 0], [-s, c, 0], [0, 0, 1]] (suncg_dataset.py:121), exact for quarter turns."""
    c, s = _QUARTER[p.k] if p.k >= 0 else (math.cos(p.theta), math.sin(p.theta))
    return np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]], np.float64)


def linear_part(p, scale):
    """M = (I f s scale) @ Rz in fp64, in the order of suncg_dataset.py:115-121 (the diagonal times each row of Rz)."""
    d = np.ones(3)
    d[0] *= p.flip
    d *= p.scale
    d *= float(scale)
    return d[:, None] * rotation_z(p)


def normal_matrix(p):
    """F Rz: normals follow flip and rotation, not the scale."""
    return np.array([p.flip, 1.0, 1.0])[:, None] * rotation_z(p)


def transform_boxes(boxes, zero_yaw, p, m, offset, scale):
    """Boxes yx_zb [M, 7] (xc, yc, z_bottom, d3, d4, dz, yaw; in the scene's own frame, unshifted) of the points moved by
    a = xyz . m + offset (voxel units): centre (c . m) / scale + offset / scale in fp64 (c . m in the points' order; the
    unaugmented case is then the arithmetic of scene_io.scene_targets bit for bit), sizes times s,
    yaw' = limit_period(f yaw - theta, 0.5, pi) -- the BEV corners of center_to_corner_box2d rotate by -yaw -- and rows
    of `zero_yaw` (ceiling / floor / room) through set_yaw_zero again after quarter turns.  -> float32 [M, 7]."""
    b = np.array(boxes, dtype=np.float32).reshape(-1, 7)
    if b.shape[0] == 0:
        return b
    c = b[:, 0:3].astype(np.float64)
    cm = np.stack([(c[:, 0] * m[0, j] + c[:, 1] * m[1, j]) + c[:, 2] * m[2, j] for j in range(3)], 1)
    out = b.copy()
    out[:, 0:3] = cm / float(scale) + np.asarray(offset, np.float64)[None, :] / float(scale)
    if p.scale != 1.0:
        out[:, 3:6] = b[:, 3:6].astype(np.float64) * p.scale
    if p.flip != 1.0 or p.theta != 0.0:
        yaw = limit_period(p.flip * b[:, 6].astype(np.float64) - p.theta, 0.5, np.pi).astype(np.float32)
        yaw[yaw >= np.float32(np.pi / 2)] -= np.float32(np.pi)          # fp32 rounding up to pi / 2
        out[:, 6] = yaw
    zy = np.asarray(zero_yaw, bool).reshape(-1)
    if p.k > 0 and zy.any():
        out[zy] = set_yaw_zero(out[zy])
    return out


def _params_struct(p, scale, cols, color_noise):
    st = AugmentParams()
    m, nrm = linear_part(p, scale), normal_matrix(p)
    for i in range(9):
        st.m[i] = float(m.flat[i])
        st.nrm[i] = float(nrm.flat[i])
    for i in range(3):
        st.color[i] = float(p.color[i])
        st.u1[i] = float(p.u1[i])
        st.u2[i] = float(p.u2[i])
    st.origin_offset = int(bool(np.any(p.u1) or np.any(p.u2)))
    # columns only when their transform is not the identity: the unaugmented case copies them, bit for bit
    st.color_col = cols.get("color", -1) if color_noise else -1
    st.normal_col = cols.get("normal", -1) if (p.flip != 1.0 or p.theta != 0.0) else -1
    return st, m


def _minmax(buf):
    return np.array(buf[:], np.float64)


def elastic_displace(points, minmax, gran, mag, generator, scratch):
    """One pass of elastic() (suncg_dataset.py:220-233) on fp64 points [n, 3] on the GPU, in place: the grid
    bb = |a|.max(0) // gran + 3 from the per-axis `minmax` [6] of the points (host), three N(0, 1) fields drawn with the
    device `generator`, the 6-pass box blur (d3d_elastic_blur) and the trilinear displacement (d3d_elastic_apply).
    -> minmax of the displaced points.  `minmax` is taken over the finite coordinates only (d3d_augment_transform,
    d3d_elastic_apply): a NaN or +-Inf row is outside every grid, keeps its value and is dropped by the voxelizer's
    contract; an axis without a finite value (min > max) counts as extent 0."""
    require_gpu(points)
    n = points.shape[0]
    minmax = np.asarray(minmax, np.float64)
    absmax = np.where(minmax[:3] <= minmax[3:], np.maximum(np.abs(minmax[:3]), np.abs(minmax[3:])), 0.0)
    bb = tuple(int(v) for v in (absmax.astype(np.int32) // int(gran) + 3))
    fields = torch.randn((3,) + bb, dtype=torch.float32, device=points.device, generator=generator)
    tmp = torch.empty_like(fields)
    s = stream_of(points.device)
    check(lib().d3d_elastic_blur(ptr(fields), 3, ints(bb), ptr(tmp), s))
    out = (ctypes.c_double * 6)()
    check(lib().d3d_elastic_apply(ptr(points), n, ptr(fields), ints(bb), float(gran), float(mag), out, ptr(scratch),
                                  scratch.numel(), s))
    return _minmax(out)


def parse_augment(spec, seed=0):
    """'flip,rotate[=quarter|free],scale=Z,offset,elastic,color=S' -> Augment (bare 'rotate' is 'free', the
    reference's draw); None or '' -> None."""
    if not spec:
        return None
    kw = {}
    for item in spec.split(","):
        key, _, val = item.strip().partition("=")
        if key == "flip" and not val:
            kw["flip_x"] = True
        elif key == "rotate":
            kw["rotate"] = val or "free"
        elif key == "scale" and val:
            kw["scale_jitter"] = float(val)
        elif key == "offset" and not val:
            kw["origin_offset"] = True
        elif key == "elastic" and not val:
            kw["elastic"] = True
        elif key == "color" and val:
            kw["color_noise"] = float(val)
        else:
            raise ValueError(f"augment: unknown item {item!r} in {spec!r} "
                             "(flip, rotate[=quarter|free], scale=Z, offset, elastic, color=S)")
    return Augment(seed=seed, **kw)


class Augment(object):
    """Random per-scene augmentation for training, applied on the GPU while the scene is voxelised.

    Augment(rotate='none' | 'quarter' | 'free', flip_x, scale_jitter=z, origin_offset, elastic, color_noise=sigma, seed):
    with everything off the result is bit for bit that of voxelize + scene_targets.  One host torch.Generator per
    instance draws every scene's parameters; the elastic fields come from a device generator seeded from it.

    __call__(pcl_dev, targets, cfg) -> (coords int64 [M, 3], feats fp32 [M, F], targets): pcl_dev fp32 [N, F] on the GPU
    with the columns of cfg.INPUT.ELEMENTS; targets {"bbox3d": yx_zb [K, 7], "labels": [K]} in the scene's own frame
    (scene_targets(..., shift=False), ScenePrefetcher(shift_targets=False)); the returned boxes are in the frame of the
    returned coordinates.  The boxes do not follow the elastic distortion (as in the reference).

    Non-finite coordinates follow voxelize's contract, elastic on or off: a point whose transformed coordinate is NaN or
    +Inf is dropped alone (the result is that of the cloud without it), a -Inf one drops the whole cloud; none of them
    sizes an elastic noise grid."""

    def __init__(self, rotate="none", flip_x=False, scale_jitter=0.0, origin_offset=False, elastic=False,
                 color_noise=0.0, seed=0):
        if rotate not in ROTATIONS:
            raise ValueError(f"rotate must be one of {ROTATIONS}, got {rotate!r}")
        if not 0.0 <= float(scale_jitter) < 1.0:
            raise ValueError(f"scale_jitter {scale_jitter} outside [0, 1)")
        if float(color_noise) < 0:
            raise ValueError(f"color_noise {color_noise} < 0")
        self.rotate, self.flip_x, self.scale_jitter = rotate, bool(flip_x), float(scale_jitter)
        self.origin_offset, self.elastic, self.color_noise = bool(origin_offset), bool(elastic), float(color_noise)
        self.seed = int(seed)
        self.generator = torch.Generator()
        self.generator.manual_seed(self.seed)

    def __repr__(self):
        return (f"Augment(rotate={self.rotate!r}, flip_x={self.flip_x}, scale_jitter={self.scale_jitter}, "
                f"origin_offset={self.origin_offset}, elastic={self.elastic}, color_noise={self.color_noise}, "
                f"seed={self.seed})")

    def for_rank(self, rank):
        """the same knobs with seed + 1000003 rank: the ranks of a data-parallel run draw differently"""
        return Augment(self.rotate, self.flip_x, self.scale_jitter, self.origin_offset, self.elastic, self.color_noise,
                       self.seed + RANK_SEED_STRIDE * int(rank))

    def sample_params(self):
        return sample_params(self.generator, self.rotate, self.flip_x, self.scale_jitter, self.origin_offset,
                             self.color_noise)

    def check_classes(self, classes):
        if self.rotate == "free":
            bad = [c for c in classes if c in _ZERO_YAW_CLASSES]
            if bad:
                raise ValueError(f"rotate='free' with zero-yaw classes {bad}: their anchors have no yaw (USE_YAWS = 0); "
                                 "use rotate='quarter'")

    def __call__(self, pcl_dev, targets, cfg):
        classes = list(cfg.INPUT.CLASSES)
        self.check_classes(classes)
        p = self.sample_params()
        scale, full = cfg.SPARSE3D.VOXEL_SCALE, cfg.SPARSE3D.VOXEL_FULL_SCALE
        pcl = pcl_dev.detach().to(torch.float32).contiguous()
        require_gpu(pcl)
        n, nfeat = pcl.shape
        cols = element_columns(cfg.INPUT.ELEMENTS)
        if any(c + 3 > nfeat for c in cols.values()):
            raise ValueError(f"{nfeat} feature columns do not hold the elements {list(cfg.INPUT.ELEMENTS)}")
        st, m = _params_struct(p, scale, cols, self.color_noise)
        dev = pcl.device
        coords = torch.empty((n, 3), dtype=torch.int64, device=dev)
        feats = torch.empty((n, nfeat), dtype=torch.float32, device=dev)
        nbytes = lib().d3d_augment_scratch_bytes(n)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        s = stream_of(dev)
        points = None
        if self.elastic and n > 0:
            points = torch.empty((n, 3), dtype=torch.float64, device=dev)
            mm = (ctypes.c_double * 6)()
            check(lib().d3d_augment_transform(ptr(pcl), n, nfeat, ctypes.byref(st), ptr(points), mm, ptr(scratch),
                                              nbytes, s))
            mm = _minmax(mm)
            gen = torch.Generator(device=dev)
            gen.manual_seed(p.elastic_seed)
            for gran, mag in ((6 * scale // 50, 40 * scale / 50), (20 * scale // 50, 160 * scale / 50)):   # :124-125
                mm = elastic_displace(points, mm, gran, mag, gen, scratch)
        kept = ctypes.c_int(0)
        offset = (ctypes.c_double * 3)()
        check(lib().d3d_augment_voxelize(ptr(pcl), n, nfeat, ptr(points), ctypes.byref(st), float(scale), ints(full),
                                         ptr(coords), ptr(feats), ctypes.byref(kept), offset, ptr(scratch), nbytes, s))
        bx, lb = targets["bbox3d"], targets["labels"]
        bx_h = bx.detach().cpu().numpy() if isinstance(bx, torch.Tensor) else np.asarray(bx)
        lb_h = lb.detach().cpu().numpy() if isinstance(lb, torch.Tensor) else np.asarray(lb)
        c2l = class_to_label(classes)
        zero_ids = [c2l[c] for c in _ZERO_YAW_CLASSES if c in c2l]
        out = transform_boxes(bx_h, np.isin(lb_h, zero_ids), p, m, np.array(offset[:]), scale)
        tb = torch.from_numpy(out)
        if isinstance(bx, torch.Tensor):
            tb = tb.to(bx.device)
        return coords[:kept.value], feats[:kept.value], {"bbox3d": tb, "labels": lb}
