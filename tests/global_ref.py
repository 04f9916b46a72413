"""numpy restatement of d3d_global_align (include/d3d_hip.h), a brute-force form of its verification for tiny lattices, and
the scenes its tests use.  Imports nothing from the package; written from the definition, not from the kernels.

Definition, for two clouds that are levelled and squared already.  Row: m = (n0 n0 + n1 n1) + n2 n2 in fp32; it takes part
iff 0.5 <= m <= 2 and its position is finite; cell c_a = floor((double(p_a) - o_a) / bin); a cell outside [0, L_a): dropped,
otherwise used; class = the axis a with n_a n_a >= c2 m (fp32), if any.  Histograms H_a over the rows of class a; wall
bitmaps (classes x, y) over (cx, cy), the target's dilated 3 x 3 inside the lattice.  Quarter turn q about the lattice
centre: (x, y) -> (x, y), (L-1-y, x), (L-1-x, L-1-y), (y, L-1-x), classes x and y swapping for odd q.  Correlations with the
target's histograms smoothed as 2 H[c] + H[c-1] + H[c+1]; peaks: C[s] > 0, nothing >= C[s] in [s - sep, s), nothing > C[s] in
(s, s + sep]; the K largest by (C descending, s ascending).  Candidate (q, i, j): the number of the source's occupied wall
cells whose turned cell plus (sx_i, sy_j) is set in the target's dilated bitmap of the class the turn gives them; -1 with
an unused slot.  Pick: the highest score, the lowest (q, i, j).  Pose: see pose_of."""
import math

import numpy as np

F32 = np.float32


def quantise(xyz, nrm, origin, bin, lattice, c2):
    """-> (hist int32 [2 L + Lz], [cells of class x, of class y] as sorted arrays of cy L + cx, used, dropped)"""
    L, Lz = int(lattice[0]), int(lattice[2])
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    nrm = np.asarray(nrm, F32).reshape(-1, 3)
    o = np.asarray(origin, np.float64).reshape(3)
    with np.errstate(all="ignore"):
        a = nrm * nrm
        m = (a[:, 0] + a[:, 1]) + a[:, 2]
        part = (m >= F32(0.5)) & (m <= F32(2.0)) & np.isfinite(xyz).all(1)
        xyz, a, m = xyz[part], a[part], m[part]
        f = np.floor((xyz.astype(np.float64) - o) / np.float64(bin))
        inside = ((f >= 0) & (f < np.array([L, L, Lz], np.float64))).all(1)
        t = F32(c2) * m
        cls = np.where(a[:, 0] >= t, 0, np.where(a[:, 1] >= t, 1, np.where(a[:, 2] >= t, 2, -1)))
    used, dropped = int(inside.sum()), int((~inside).sum())
    c = f[inside].astype(np.int64)
    cls = cls[inside]
    hist = np.zeros(2 * L + Lz, np.int64)
    for k, (off, length) in enumerate(((0, L), (L, L), (2 * L, Lz))):
        hist[off:off + length] = np.bincount(c[cls == k, k], minlength=length)
    cells = [np.unique(c[cls == k, 1] * L + c[cls == k, 0]) for k in (0, 1)]
    return hist.astype(np.int32), cells, used, dropped


def bitmap_words(image):
    """bool [L, L] indexed [y, x] -> uint32 [L L / 32]: bit (y L + x) mod 32 of word (y L + x) / 32"""
    flat = image.reshape(-1, 32).astype(np.uint64)
    return (flat << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)


def dilate(image):
    out = image.copy()
    p = np.pad(image, 1)
    L = image.shape[0]
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + L, dx:dx + L]
    return out


def turn(q, x, y, L):
    return [(x, y), (L - 1 - y, x), (L - 1 - x, L - 1 - y), (y, L - 1 - x)][q]


def turned_hist(q, axis, hx, hy):
    if axis == 0:
        return [hx, hy[::-1], hx[::-1], hy][q]
    return [hy, hx, hy[::-1], hx[::-1]][q]


def correlate(hs, ht):
    """int64 [2 L - 1], entry s + L - 1: sum_c hs[c] ht~[c + s]; Python integers, so nothing can round"""
    L = len(hs)
    t = np.zeros(L + 2, np.int64)
    t[1:-1] = ht
    smooth = 2 * t[1:-1] + t[:-2] + t[2:]
    assert int(hs.astype(np.int64).sum()) * int(smooth.max(initial=0)) < 2 ** 62
    return np.correlate(smooth.astype(np.int64), hs.astype(np.int64), "full")      # integer arithmetic: exact


def peaks_of(C, L, K, sep):
    """-> (value int64 [K], shift int32 [K]), unused slots (-1, 0)"""
    n = len(C)
    ok = C > 0
    for d in range(1, sep + 1):
        before = np.concatenate([np.full(d, -1, np.int64), C[:-d]]) if d < n else np.full(n, -1, np.int64)
        after = np.concatenate([C[d:], np.full(d, -1, np.int64)]) if d < n else np.full(n, -1, np.int64)
        ok &= ~(before >= C) & ~(after > C)
    at = np.nonzero(ok)[0]
    order = at[np.lexsort((at, -C[at]))][:K]
    value, shift = np.full(K, -1, np.int64), np.zeros(K, np.int32)
    value[:len(order)] = C[order]
    shift[:len(order)] = order - (L - 1)
    return value, shift


def pose_of(q, sx, sy, sz, o_s, o_t, bin, L):
    """x_t = R x_s + t in fp64, every operation as written: u = (o_s,x + bin h, o_s,y + bin h, o_s,z), v = (o_t,x + bin (sx +
    h), o_t,y + bin (sy + h), o_t,z + bin sz), h = L / 2; t = v - Rz(q) u, with Rz(q) u a selection and a sign"""
    b = np.float64(bin)
    o_s, o_t = np.asarray(o_s, np.float64), np.asarray(o_t, np.float64)
    half = L // 2
    hb = b * np.float64(half)
    ux, uy, uz = o_s[0] + hb, o_s[1] + hb, o_s[2]
    vx, vy, vz = o_t[0] + b * np.float64(sx + half), o_t[1] + b * np.float64(sy + half), o_t[2] + b * np.float64(sz)
    wx, wy = [(ux, uy), (-uy, ux), (-ux, -uy), (uy, -ux)][q]
    c, s = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][q]
    pose = np.eye(4)
    pose[0, :2] = [c, 0.0 if s == 0.0 else -s]
    pose[1, :2] = [s, c]
    pose[:3, 3] = [vx - wx, vy - wy, vz - uz]
    return pose


def global_ref(src_xyz, src_nrm, o_s, tgt_xyz, tgt_nrm, o_t, bin=0.05, lattice=(2048, 2048, 256), tol=5.0, peaks=64, sep=2):
    """-> dict with the library's outputs and tables: pose, choice, score, support, status, hist [2, 2 L + Lz], cells (two
    arrays of cy << 16 | cx), target_bits uint32 [2, L L / 32], corr int64 [9, 2 max(L, Lz) - 1], peak_value, peak_shift
    [9, K], scores int32 [4, K, K]"""
    L, Lz, K = int(lattice[0]), int(lattice[2]), int(peaks)
    assert lattice[0] == lattice[1] and L % 32 == 0
    c2 = F32(math.cos(math.radians(tol)) ** 2)
    hs, cells_s, used_s, dropped_s = quantise(src_xyz, src_nrm, o_s, bin, lattice, c2)
    ht, cells_t, used_t, dropped_t = quantise(tgt_xyz, tgt_nrm, o_t, bin, lattice, c2)
    timg = []
    for k in (0, 1):
        img = np.zeros(L * L, bool)
        img[cells_t[k]] = True
        timg.append(dilate(img.reshape(L, L)))
    NS = 2 * max(L, Lz) - 1
    corr = np.zeros((9, NS), np.int64)
    pv, ps = np.zeros((9, K), np.int64), np.zeros((9, K), np.int32)
    for q in range(4):
        for axis in (0, 1):
            k = 2 * q + axis
            corr[k, :2 * L - 1] = correlate(turned_hist(q, axis, hs[:L], hs[L:2 * L]), ht[axis * L:(axis + 1) * L])
            pv[k], ps[k] = peaks_of(corr[k, :2 * L - 1], L, K, sep)
    corr[8, :2 * Lz - 1] = correlate(hs[2 * L:], ht[2 * L:])
    pv[8], ps[8] = peaks_of(corr[8, :2 * Lz - 1], Lz, K, sep)
    scores = np.full((4, K, K), -1, np.int32)
    for q in range(4):
        vi, vj = pv[2 * q] > 0, pv[2 * q + 1] > 0
        scores[q][np.ix_(vi, vj)] = 0
        sy = ps[2 * q + 1][vj].astype(np.int64)
        for k in (0, 1):
            tx, ty = turn(q, cells_s[k] % L, cells_s[k] // L, L)
            flat = timg[k ^ (q & 1)].reshape(-1)
            for i in np.nonzero(vi)[0]:
                x = tx + int(ps[2 * q][i])
                inx = (x >= 0) & (x < L)
                y = ty[inx][None, :] + sy[:, None]
                iny = (y >= 0) & (y < L)
                hit = flat[np.where(iny, y, 0) * L + x[inx][None, :]] & iny
                scores[q, i, vj] += hit.sum(1).astype(np.int32)
    flat = scores.reshape(-1)
    at = int(np.argmax(flat))                          # the first of the equal maxima: the lowest (q, i, j)
    best = int(flat[at])
    score = np.array([int(scores[q].max()) for q in range(4)] + [best, int(np.delete(flat, at).max())], np.int64)
    o_s, o_t = np.asarray(o_s, np.float64), np.asarray(o_t, np.float64)
    if best <= 0:
        status, choice = 1, np.zeros(4, np.int32)
        pose = np.eye(4)
        pose[:3, 3] = o_t - o_s
    else:
        q, i, j = at // (K * K), (at // K) % K, at % K
        sz = int(ps[8, 0]) if pv[8, 0] > 0 else 0
        status, choice = 0, np.array([q, ps[2 * q, i], ps[2 * q + 1, j], sz], np.int32)
        pose = pose_of(q, int(choice[1]), int(choice[2]), sz, o_s, o_t, bin, L)
    return {"pose": pose, "choice": choice, "score": score, "support": np.array([used_s, dropped_s, used_t, dropped_t], np.int32),
            "status": status, "hist": np.stack([hs, ht]),
            "cells": [((c // L) << 16 | (c % L)).astype(np.int32) for c in cells_s],
            "target_bits": np.stack([bitmap_words(t) for t in timg]), "corr": corr, "peak_value": pv, "peak_shift": ps,
            "scores": scores, "margin": (max(int(score[5]), 0) / best if best > 0 else math.inf)}


def brute_scores(src_xyz, src_nrm, o_s, tgt_xyz, tgt_nrm, o_t, bin, lattice, tol):
    """every (q, sx, sy) of a small lattice scored directly from sets of cells -> int [4, 2 L - 1, 2 L - 1], entry
    [q, sx + L - 1, sy + L - 1]; loops and sets, nothing shared with global_ref but quantise"""
    L = int(lattice[0])
    c2 = F32(math.cos(math.radians(tol)) ** 2)
    _, cells_s, _, _ = quantise(src_xyz, src_nrm, o_s, bin, lattice, c2)
    _, cells_t, _, _ = quantise(tgt_xyz, tgt_nrm, o_t, bin, lattice, c2)
    grown = []
    for k in (0, 1):
        g = set()
        for c in cells_t[k].tolist():
            x, y = c % L, c // L
            g.update((x + dx, y + dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if 0 <= x + dx < L and 0 <= y + dy < L)
        grown.append(g)
    out = np.zeros((4, 2 * L - 1, 2 * L - 1), np.int64)
    for q in range(4):
        for k in (0, 1):
            tgt = grown[k ^ (q & 1)]
            for c in cells_s[k].tolist():
                x, y = turn(q, c % L, c // L, L)
                for (gx, gy) in tgt:                 # this source cell meets this target cell under exactly one shift
                    out[q, gx - x + L - 1, gy - y + L - 1] += 1
    return out


# ---- scenes ----------------------------------------------------------------------------------------------------------

SHELL = (25.0, 19.0, 2.7)


def building(seed, n_walls=10):
    """the faces of a 25 x 19 x 2.7 m shell with interior walls at random offsets that span random parts of it -> list of
    (axis of the normal, offset along it, (lo, hi) along the first other axis, (lo, hi) along the second)"""
    rng = np.random.RandomState(1000 + seed)
    X, Y, Z = SHELL
    faces = [(2, 0.0, (0, X), (0, Y)), (2, Z, (0, X), (0, Y)), (0, 0.0, (0, Y), (0, Z)), (0, X, (0, Y), (0, Z)),
             (1, 0.0, (0, X), (0, Z)), (1, Y, (0, X), (0, Z))]
    for _ in range(n_walls):
        axis = int(rng.randint(2))
        along = Y if axis == 0 else X
        off = rng.uniform(1.0, (X if axis == 0 else Y) - 1.0)
        a, b = np.sort(rng.uniform(0, along, 2))
        if b - a < 2.0:
            a, b = max(0.0, a - 1.0), min(along, b + 1.0)
        faces.append((axis, float(off), (float(a), float(b)), (0, Z)))
    return faces


def sample(faces, n, seed, noise=0.003):
    """n points on the faces, by area, with `noise` metres of Gaussian noise on every coordinate and exact normals of a
    random sign -> (xyz fp64 [n, 3], normals fp64 [n, 3])"""
    rng = np.random.RandomState(seed)
    area = np.array([(f[2][1] - f[2][0]) * (f[3][1] - f[3][0]) for f in faces])
    which = rng.choice(len(faces), n, p=area / area.sum())
    xyz, nrm = np.zeros((n, 3)), np.zeros((n, 3))
    u, v = rng.uniform(size=n), rng.uniform(size=n)
    for k, (axis, off, r1, r2) in enumerate(faces):
        sel = which == k
        o1, o2 = [a for a in range(3) if a != axis]
        xyz[sel, axis] = off
        xyz[sel, o1] = r1[0] + u[sel] * (r1[1] - r1[0])
        xyz[sel, o2] = r2[0] + v[sel] * (r2[1] - r2[0])
        nrm[sel, axis] = 1.0
    nrm *= np.where(rng.uniform(size=(n, 1)) < 0.5, -1.0, 1.0)
    return xyz + rng.normal(size=(n, 3)) * noise, nrm


def rigid(yaw_deg, shift):
    a = math.radians(yaw_deg)
    P = np.eye(4)
    P[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]
    P[:3, 3] = shift
    return P


def pair(seed, q, n=120000, target_max_x=20.0, source_min_x=5.0, residual_yaw=0.05, max_shift=20.0):
    """two scans of building(seed), sampled apart: the target keeps x <= target_max_x in the building's frame, the source
    keeps x >= source_min_x and is delivered in a frame of its own, turned by q quarter turns and `residual_yaw` degrees
    and shifted by up to max_shift metres -> (source [.., 6], target [.., 6] fp32 (xyz, normal), truth fp64 [4, 4] with
    x_target = truth x_source)"""
    faces = building(seed)
    rng = np.random.RandomState(5000 + 4 * seed + q)
    tx, tn = sample(faces, n, 2 * seed + 11)
    sx, sn = sample(faces, n, 2 * seed + 12)
    keep_t, keep_s = tx[:, 0] <= target_max_x, sx[:, 0] >= source_min_x
    tx, tn, sx, sn = tx[keep_t], tn[keep_t], sx[keep_s], sn[keep_s]
    shift = np.append(rng.uniform(-max_shift, max_shift, 2), rng.uniform(-1.0, 1.0))
    truth = rigid(90.0 * q + residual_yaw, shift)
    inv = np.linalg.inv(truth)
    sx = sx @ inv[:3, :3].T + inv[:3, 3]
    sn = sn @ inv[:3, :3].T
    return (np.concatenate([sx, sn], 1).astype(F32), np.concatenate([tx, tn], 1).astype(F32), truth)


def origin_of(xyz):
    """the cloud's per-axis minimum over rows without a NaN, as primitives.cloud_min takes it (zeros for no rows)"""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    if len(xyz) == 0:
        return np.zeros(3)
    return np.where(np.isnan(xyz), np.inf, xyz).min(0).astype(np.float64)


def align_ref(source, target, **kw):
    """global_ref on two [.., 6] clouds that are squared already, origins their minima"""
    return global_ref(source[:, :3], source[:, 3:6], origin_of(source[:, :3]), target[:, :3], target[:, 3:6],
                      origin_of(target[:, :3]), **kw)


def shift_error(pose, truth, at):
    """per-axis distance between where the two poses put the point `at`"""
    at = np.asarray(at, np.float64)
    return np.abs((pose[:3, :3] @ at + pose[:3, 3]) - (truth[:3, :3] @ at + truth[:3, 3]))
