"""The definitions of detection_3d_amd.floorplan restated in numpy fp64, with scipy.ndimage.label (4-connected) for the
components.  numpy rounds every product, sum and quotient on its own, which is the contract of floorplan.hip (built with
-ffp-contract=off), so every output is compared bit for bit.  The exact tests hand the device's own box table (read
back) to `blocked`, `sides` and `lattice`; `box_table` itself is compared to 1e-12."""
import math

import numpy as np
from scipy import ndimage

OUTSIDE, BLOCKED, SMALL, NONE = -1, -2, -3, -4
FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])


def box_table(boxes, grow=0.0):
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 7).astype(np.float64)
    return np.stack([b[:, 0], b[:, 1], np.cos(b[:, 6]), np.sin(b[:, 6]), b[:, 3] / 2 + grow, b[:, 4] / 2 + grow], 1)


def lattice(table, select, cell, margin=2):
    """(origin, shape) of lattice=None: around the corners of the selected finite rows"""
    t = np.asarray(table, dtype=np.float64).reshape(-1, 6)
    ok = np.isfinite(t).all(1)
    if select is not None:
        ok &= np.asarray(select, dtype=bool)
    t = t[ok]
    if t.shape[0] == 0:
        x0 = y0 = x1 = y1 = 0.0
    else:
        ex = np.abs(t[:, 2]) * t[:, 4] + np.abs(t[:, 3]) * t[:, 5]
        ey = np.abs(t[:, 3]) * t[:, 4] + np.abs(t[:, 2]) * t[:, 5]
        x0, y0 = float((t[:, 0] - ex).min()), float((t[:, 1] - ey).min())
        x1, y1 = float((t[:, 0] + ex).max()), float((t[:, 1] + ey).max())
    i0, j0 = math.floor(x0 / cell) - margin, math.floor(y0 / cell) - margin
    i1, j1 = math.ceil(x1 / cell) + margin, math.ceil(y1 / cell) + margin
    return (i0 * cell, j0 * cell), (j1 - j0, i1 - i0)


def blocked(table, select, cell, origin, shape):
    """bool [H, W]: the cell's centre lies in at least one selected box, faces closed; a non-finite row blocks nothing"""
    h, w = shape
    ox, oy = (np.float64(v) for v in origin)
    cell = np.float64(cell)
    X = (ox + (np.arange(w, dtype=np.float64) + 0.5) * cell)[None, :]
    Y = (oy + (np.arange(h, dtype=np.float64) + 0.5) * cell)[:, None]
    out = np.zeros((h, w), dtype=bool)
    t = np.asarray(table, dtype=np.float64).reshape(-1, 6)
    for j in range(t.shape[0]):
        if (select is not None and not select[j]) or not np.isfinite(t[j]).all():
            continue
        xc, yc, c, s, hx, hy = t[j]
        # the columns and rows the box can reach, two cells wider: only to keep the loop cheap
        ex, ey = abs(c) * hx + abs(s) * hy, abs(s) * hx + abs(c) * hy
        a0 = int(np.clip(np.floor((xc - ex - ox) / cell) - 2, 0, w))
        a1 = int(np.clip(np.floor((xc + ex - ox) / cell) + 3, 0, w))
        b0 = int(np.clip(np.floor((yc - ey - oy) / cell) - 2, 0, h))
        b1 = int(np.clip(np.floor((yc + ey - oy) / cell) + 3, 0, h))
        if a0 >= a1 or b0 >= b1:
            continue
        dx, dy = X[:, a0:a1] - xc, Y[b0:b1] - yc
        lx = c * dx - s * dy
        ly = s * dx + c * dy
        out[b0:b1, a0:a1] |= (np.abs(lx) <= hx) & (np.abs(ly) <= hy)
    return out


def blocked_full(table, select, cell, origin, shape):
    """`blocked` without the window: every cell against every box (small plans)"""
    h, w = shape
    ox, oy = (np.float64(v) for v in origin)
    cell = np.float64(cell)
    X = (ox + (np.arange(w, dtype=np.float64) + 0.5) * cell)[None, :]
    Y = (oy + (np.arange(h, dtype=np.float64) + 0.5) * cell)[:, None]
    out = np.zeros((h, w), dtype=bool)
    t = np.asarray(table, dtype=np.float64).reshape(-1, 6)
    for j in range(t.shape[0]):
        if (select is not None and not select[j]) or not np.isfinite(t[j]).all():
            continue
        xc, yc, c, s, hx, hy = t[j]
        dx, dy = X - xc, Y - yc
        with np.errstate(all="ignore"):
            lx = c * dx - s * dy
            ly = s * dx + c * dy
            out |= (np.abs(lx) <= hx) & (np.abs(ly) <= hy)
    return out


def min_cells(min_area, cell):
    return max(1, int(math.ceil(float(min_area) / (float(cell) * float(cell)))))


def rooms(blocked_map, min_cells_=1, max_rooms=1024):
    """-> label int32 [H, W], R, cells int32 [max_rooms], bounds int32 [max_rooms, 4], seed int32 [max_rooms]; the rows
    from R on hold 0, (W, H, -1, -1) and -1"""
    blk = np.asarray(blocked_map, dtype=bool)
    h, w = blk.shape
    comp, n = ndimage.label(~blk, structure=FOUR)        # numbered in scan order: by smallest cell id already
    label = np.full((h, w), BLOCKED, dtype=np.int32)
    cells = np.zeros(max_rooms, dtype=np.int32)
    bounds = np.tile(np.array([w, h, -1, -1], dtype=np.int32), (max_rooms, 1))
    seed = np.full(max_rooms, -1, dtype=np.int32)
    if n == 0:
        return label, 0, cells, bounds, seed
    flat = comp.reshape(-1)
    ids = np.arange(h * w)
    first = np.full(n + 1, h * w, dtype=np.int64)
    np.minimum.at(first, flat, ids)
    size = np.bincount(flat, minlength=n + 1)
    edge = np.zeros((h, w), dtype=bool)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
    outside = np.zeros(n + 1, dtype=bool)
    outside[np.unique(comp[edge & ~blk])] = True
    objs = ndimage.find_objects(comp)
    r = 0
    value = np.zeros(n + 1, dtype=np.int32)
    for c in sorted(range(1, n + 1), key=lambda c: first[c]):
        if outside[c]:
            value[c] = OUTSIDE
        elif size[c] < min_cells_:
            value[c] = SMALL
        else:
            value[c] = r
            if r < max_rooms:
                ys, xs = objs[c - 1]
                cells[r], seed[r] = size[c], first[c]
                bounds[r] = (xs.start, ys.start, xs.stop - 1, ys.stop - 1)
            r += 1
    free = ~blk
    label[free] = value[comp[free]]
    return label, r, cells, bounds, seed


def cell_of(x, o, cell, n):
    """the cell index of coordinates x along one axis, -1 off the lattice"""
    with np.errstate(all="ignore"):
        f = np.floor((np.asarray(x, dtype=np.float64) - np.float64(o)) / np.float64(cell))
    ok = (f >= 0) & (f < n)
    return np.where(ok, np.where(ok, f, 0).astype(np.int64), -1)


def sides(table0, label, cell, origin, reach=0.5):
    """table0: the table with grow 0 -> int32 [K, 2], column 0 the -lx side"""
    t = np.asarray(table0, dtype=np.float64).reshape(-1, 6)
    h, w = label.shape
    cell = np.float64(cell)
    n_probe = int(math.ceil(float(reach) / float(cell)))
    out = np.full((t.shape[0], 2), NONE, dtype=np.int32)
    for j in range(t.shape[0]):
        xc, yc, c, s, hx, _ = t[j]
        for e, sign in enumerate((-1.0, 1.0)):
            for k in range(n_probe):
                tt = sign * (hx + (np.float64(k) + 0.5) * cell)
                with np.errstate(all="ignore"):
                    px, py = xc + c * tt, yc - s * tt
                ix, iy = int(cell_of(px, origin[0], cell, w)), int(cell_of(py, origin[1], cell, h))
                if ix < 0 or iy < 0:
                    out[j, e] = OUTSIDE
                    break
                if label[iy, ix] != BLOCKED:
                    out[j, e] = label[iy, ix]
                    break
    return out


def room_of_points(xyz, label, cell, lattice_origin, origin=None):
    p = np.asarray(xyz, dtype=np.float32)[:, :3].astype(np.float64)
    if origin is not None:
        with np.errstate(all="ignore"):
            p = p - np.asarray(origin, dtype=np.float64).reshape(1, 3)
    h, w = label.shape
    ix, iy = cell_of(p[:, 0], lattice_origin[0], cell, w), cell_of(p[:, 1], lattice_origin[1], cell, h)
    out = np.full(p.shape[0], OUTSIDE, dtype=np.int32)
    on = (ix >= 0) & (iy >= 0)
    out[on] = label[iy[on], ix[on]]
    out[~np.isfinite(p).all(1)] = NONE
    return out


def room_boxes(bounds, cell, origin, z_bot=0.0, height=0.0):
    b = np.asarray(bounds, dtype=np.float64).reshape(-1, 4)
    out = np.zeros((b.shape[0], 7), dtype=np.float64)
    out[:, 0] = origin[0] + (b[:, 0] + b[:, 2] + 1) / 2 * cell
    out[:, 1] = origin[1] + (b[:, 1] + b[:, 3] + 1) / 2 * cell
    out[:, 2] = z_bot
    out[:, 3] = (b[:, 2] - b[:, 0] + 1) * cell
    out[:, 4] = (b[:, 3] - b[:, 1] + 1) * cell
    out[:, 5] = height
    return out


def cloud_min(xyz):
    p = np.asarray(xyz, dtype=np.float32)[:, :3]
    p = np.where(np.isnan(p), np.inf, p)
    return p.min(0).astype(np.float64) if p.shape[0] else np.zeros(3)


# ---- hand-built plans (the tests' inputs) ----
def wall(x0, y0, x1, y1, thick=0.1, z_bot=0.0, dz=2.5):
    """the yx_zb row of a wall from (x0, y0) to (x1, y1): d3 = thick across, d4 = the length; +lx = (c, -s) is the
    normal, so a wall along x has yaw pi / 2 and one along y yaw 0"""
    length = math.hypot(x1 - x0, y1 - y0)
    ux, uy = (x1 - x0) / length, (y1 - y0) / length        # the length axis d4 runs along (s, c)
    yaw = math.atan2(ux, uy)
    return [(x0 + x1) / 2, (y0 + y1) / 2, z_bot, thick, length, dz, yaw]


def six_rooms(scale=1.0):
    """walls 0.1 thick at x = 1, 5, 9, 13 and y = 1, 5, 9 (times scale): 2 x 3 rooms"""
    xs, ys = [1.0, 5.0, 9.0, 13.0], [1.0, 5.0, 9.0]
    rows = [wall(x * scale, ys[0] * scale, x * scale, ys[-1] * scale) for x in xs]
    rows += [wall(xs[0] * scale, y * scale, xs[-1] * scale, y * scale) for y in ys]
    return np.array(rows, dtype=np.float32)


def random_plan(seed, n_walls=24, extent=(9.0, 6.5)):
    """axis-aligned and rotated walls inside [0.5, extent]"""
    rs = np.random.RandomState(seed)
    rows = []
    for i in range(n_walls):
        x0, y0 = rs.uniform(0.5, extent[0]), rs.uniform(0.5, extent[1])
        length = rs.uniform(0.5, 5.0)
        kind = rs.randint(3)
        a = (0.0, math.pi / 2)[kind] if kind < 2 else rs.uniform(0, math.pi)
        x1 = float(np.clip(x0 + length * math.cos(a), 0.5, extent[0]))
        y1 = float(np.clip(y0 + length * math.sin(a), 0.5, extent[1]))
        if math.hypot(x1 - x0, y1 - y0) < 0.2:
            continue
        rows.append(wall(x0, y0, x1, y1, thick=rs.uniform(0.05, 0.3)))
    return np.array(rows, dtype=np.float32).reshape(-1, 7)
