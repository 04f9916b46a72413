"""numpy oracle of detection_3d_amd/csrc/augment.hip: the same fp64 operations in the same order (no contraction), so
that the affine path matches bit for bit; the elastic sampling follows scipy's RegularGridInterpolator step by step."""
import itertools

import numpy as np

BLUR_W = float(np.float32(1) / np.float32(3))          # np.ones(...).astype('float32') / 3, suncg_dataset.py:215-217


def affine(xyz, m):
    """a_j = ((x m0j + y m1j) + z m2j) in fp64"""
    x, y, z = (np.asarray(xyz[:, d], np.float64) for d in range(3))
    return np.stack([(x * m[0, j] + y * m[1, j]) + z * m[2, j] for j in range(3)], 1)


def offset_of(a, full, u1=None, u2=None):
    """suncg_dataset.py:126-132"""
    lo, hi = a.min(0), a.max(0)
    off = -lo
    if u1 is not None:
        q = (np.asarray(full, np.float64) - hi) + lo
        off = off + (np.clip(q - 0.001, 0, None) * u1 + np.clip(q + 0.001, None, 0) * u2)
    return off


def augment_voxelize(pcl, m, scale, full, nrm=None, color=None, u1=None, u2=None, color_col=-1, normal_col=-1,
                     points=None):
    """-> (coords int64 [M,3], feats fp32 [M,F], offset [3], kept mask [N])"""
    a = affine(pcl, m) if points is None else np.asarray(points, np.float64)
    off = offset_of(a, full, u1, u2)
    b = a + off
    keep = np.all((b >= 0) & (b < np.asarray(full, np.float64)), 1)
    bk = b[keep]
    coords = bk.astype(np.int64)
    feats = np.array(pcl[keep], np.float32)
    feats[:, 0:3] = (bk / float(scale)).astype(np.float32)
    if color_col >= 0:
        feats[:, color_col:color_col + 3] = (pcl[keep, color_col:color_col + 3].astype(np.float64) + color).astype(np.float32)
    if normal_col >= 0:
        feats[:, normal_col:normal_col + 3] = affine(pcl[keep, normal_col:normal_col + 3], nrm).astype(np.float32)
    return coords, feats, off, keep


def blur_axis(f, axis):
    """one 3-tap pass, zero padded: ((0 + x[-1] w) + x[0] w) + x[+1] w in fp64, rounded to fp32"""
    x = f.astype(np.float64)
    lo = np.zeros_like(x)
    hi = np.zeros_like(x)
    sl = [slice(None)] * 3
    a, b = list(sl), list(sl)
    a[axis], b[axis] = slice(1, None), slice(None, -1)
    lo[tuple(a)] = x[tuple(b)]                      # x[i - 1]
    hi[tuple(b)] = x[tuple(a)]                      # x[i + 1]
    return (((0.0 + lo * BLUR_W) + x * BLUR_W) + hi * BLUR_W).astype(np.float32)


def blur(f):
    """elastic()'s axes 0, 1, 2, 0, 1, 2"""
    for axis in (0, 1, 2, 0, 1, 2):
        f = blur_axis(f, axis)
    return f


def grid_dims(a, gran):
    """bb = |a|.max(0) // gran + 3 (suncg_dataset.py:221)"""
    return tuple(int(v) for v in (np.abs(a).max(0).astype(np.int32) // int(gran) + 3))


def interpolate(field, gran, pts):
    """RegularGridInterpolator(axes linspace(-(b-1) gran, (b-1) gran, b), field, bounds_error=0, fill_value=0)(pts)"""
    axes = [np.linspace(-(b - 1) * gran, (b - 1) * gran, b) for b in field.shape]
    idx, t, oob = [], [], np.zeros(pts.shape[0], bool)
    for d, g in enumerate(axes):
        x = pts[:, d]
        i = np.clip(np.searchsorted(g, x) - 1, 0, g.size - 2)
        idx.append(i)
        t.append((x - g[i]) / (g[i + 1] - g[i]))
        oob |= (x < g[0]) | (x > g[-1])
    val = np.zeros(pts.shape[0])
    for corner in itertools.product((0, 1), repeat=3):
        w = np.ones(pts.shape[0])
        for d, c in enumerate(corner):
            w = w * (t[d] if c else 1.0 - t[d])
        ii = tuple(np.where(oob, 0, idx[d] + c) for d, c in enumerate(corner))
        val = val + field[ii].astype(np.float64) * w
    val[oob] = 0.0
    return val


def elastic_pass(a, fields, gran, mag):
    """a + g(a) * mag with g the 3 (blurred) fields sampled at a"""
    disp = np.stack([interpolate(f, gran, a) for f in fields], 1)
    return a + disp * mag


def elastic_scipy(a, fields_raw, gran, mag):
    """elastic() of the reference with given raw fields instead of its randn draws: scipy.ndimage.convolve +
    RegularGridInterpolator"""
    import scipy.interpolate
    import scipy.ndimage
    b0 = np.ones((3, 1, 1)).astype("float32") / 3
    b1 = np.ones((1, 3, 1)).astype("float32") / 3
    b2 = np.ones((1, 1, 3)).astype("float32") / 3
    noise = list(fields_raw)
    for w in (b0, b1, b2, b0, b1, b2):
        noise = [scipy.ndimage.convolve(n, w, mode="constant", cval=0) for n in noise]
    ax = [np.linspace(-(b - 1) * gran, (b - 1) * gran, b) for b in noise[0].shape]
    interp = [scipy.interpolate.RegularGridInterpolator(ax, n, bounds_error=0, fill_value=0) for n in noise]
    return a + np.hstack([i(a)[:, None] for i in interp]) * mag, noise


def bev_corners(boxes):
    """orc_bev_corners (center_to_corner_box2d) in fp64: [n, 4, 2]"""
    b = np.asarray(boxes, np.float64)
    nx, ny = np.array([-0.5, -0.5, 0.5, 0.5]), np.array([-0.5, 0.5, 0.5, -0.5])
    c, s = np.cos(b[:, 6])[:, None], np.sin(b[:, 6])[:, None]
    px, py = b[:, 3:4] * nx, b[:, 4:5] * ny
    return np.stack([px * c + py * s + b[:, 0:1], px * (-s) + py * c + b[:, 1:2]], 2)
