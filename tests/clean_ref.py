"""numpy / scipy fp64 restatement of detection_3d_amd/csrc/clean.hip's semantics and the clouds the clean
tests run on, in the style of tests/normals_ref.py.  Neighbours come from a k-d tree at 1.001 r, d2 is recomputed in
fp64 from the fp32 positions, the candidates are ordered by (d2, j) and cut at k + 1.

Edge flags mark the only points where fp32 and fp64 may pick different sets: a candidate within EDGE_REL of r^2
(relative to r^2), and, for the k-nearest cut, a (k+1)-th and (k+2)-th squared distance that differ by at most EDGE_REL
of the latter (relative to the distance itself, normals_ref's tie_scale='cut': an fp32 d2 of an exact offset is off by
at most 1.8e-7 d2, so the order of two distances is only in doubt within 4e-7 d2 and the flag keeps a margin of 25;
measured against r^2 instead, a neighbourhood of a thousand points would flag a quarter of itself)."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components as _cc
from scipy.spatial import cKDTree

from tests.normals_ref import EDGE_REL, dense_patch, make_scene


def _positions(xyz, radius):
    p = np.asarray(xyz, np.float32)[:, :3].astype(np.float64)
    r = float(np.float32(radius))
    return p, r, r * r


def _balls(p, r):
    return cKDTree(p).query_ball_point(p, 1.001 * r) if p.shape[0] else []


def neighbors_ref(xyz, radius=0.1):
    """-> (count int32 [N]: the points with d2 <= r^2, the point itself included; lo, hi int32 [N]: the count with every
    candidate within EDGE_REL r^2 of r^2 left out / taken in; edge bool [N]: lo != hi)"""
    p, r, r2 = _positions(xyz, radius)
    n = p.shape[0]
    count, lo, hi = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i, ball in enumerate(_balls(p, r)):
        q = p[np.asarray(ball, np.int64)] - p[i]
        d2 = (q * q).sum(1)
        count[i] = (d2 <= r2).sum()
        lo[i] = (d2 < r2 * (1.0 - EDGE_REL)).sum()
        hi[i] = (d2 <= r2 * (1.0 + EDGE_REL)).sum()
    return count, lo, hi, lo != hi


def knn_ref(xyz, k=20, radius=0.1):
    """-> (mean fp64 [N]: the sum of the distances to the k + 1 nearest candidates by (d2, j), the point itself among
    them, over k; +inf for a sparse point; found int32 [N]: the kept candidates - 1; edge bool [N])"""
    p, r, r2 = _positions(xyz, radius)
    n = p.shape[0]
    mean, found, edge = np.full(n, np.inf), np.zeros(n, np.int32), np.zeros(n, bool)
    for i, ball in enumerate(_balls(p, r)):
        j = np.asarray(ball, np.int64)
        q = p[j] - p[i]
        d2 = (q * q).sum(1)
        edge[i] = bool(np.any(np.abs(d2 - r2) <= EDGE_REL * r2))
        keep = d2 <= r2
        j, d2 = j[keep], d2[keep]
        order = np.lexsort((j, d2))
        if order.size > k + 1:
            if d2[order[k + 1]] - d2[order[k]] <= EDGE_REL * d2[order[k + 1]]:
                edge[i] = True
            order = order[:k + 1]
        found[i] = order.size - 1
        if found[i] >= k:
            mean[i] = np.sqrt(d2[order]).sum() / k
    return mean, found, edge


def stats_ref(mean):
    """(mu, sigma) of the finite means: the mean, and the square root of the squared deviations over (count - 1)"""
    v = np.asarray(mean, np.float64)
    v = v[np.isfinite(v)]
    if v.size == 0:
        return 0.0, 0.0
    mu = v.sum() / v.size
    return mu, (np.sqrt(((v - mu) ** 2).sum() / (v.size - 1)) if v.size > 1 else 0.0)


def _labels(n, a, b):
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    g = coo_matrix((np.ones(a.size, np.int8), (a, b)), shape=(n, n))
    _, comp = _cc(g, directed=False)
    first = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(first, comp, np.arange(n))
    return first[comp].astype(np.int32), np.bincount(comp)[comp].astype(np.int32)


def components_ref(xyz, radius=0.1):
    """-> ((label, size) with edges d2 <= r^2 (1 - EDGE_REL), (label, size) with edges d2 <= r^2 (1 + EDGE_REL)):
    label int32 [N] the smallest row index of the point's component, size int32 [N] its number of points.  Where the two
    agree, every threshold between them, the fp32 one included, gives the same components."""
    p, r, r2 = _positions(xyz, radius)
    n = p.shape[0]
    pairs = cKDTree(p).query_pairs(1.001 * r, output_type="ndarray") if n else np.zeros((0, 2), np.int64)
    q = p[pairs[:, 0]] - p[pairs[:, 1]]
    d2 = (q * q).sum(1)
    out = []
    for t in (r2 * (1.0 - EDGE_REL), r2 * (1.0 + EDGE_REL)):
        sel = d2 <= t
        out.append(_labels(n, pairs[sel, 0], pairs[sel, 1]))
    return tuple(out)


def make_cloud(seed):
    """normals_ref.make_scene(6000, seed) and a dense_patch of 1500 points: 16 isolated points, a detached patch and a
    neighbourhood of more than 1024 candidates (the unstaged form) -> fp32 [7500, 3]"""
    return np.concatenate([make_scene(6000, seed), dense_patch(1500, seed + 100)])


def make_chains(radius=0.1, m=3000, seed=0):
    """Two parallel lines of m points, spaced 0.9 radius along the line and 1.2 radius apart, rows permuted -> fp32
    [2 m, 3].  At `radius` exactly two components of m points, a union m deep; at half of it 2 m singletons."""
    t = np.arange(m, dtype=np.float64) * 0.9 * radius
    a = np.stack([t, np.zeros(m), np.zeros(m)], 1)
    b = np.stack([t, np.full(m, 1.2 * radius), np.zeros(m)], 1)
    pts = np.concatenate([a, b]) + np.array([3.0, -2.0, 0.5])
    return pts[np.random.RandomState(seed).permutation(2 * m)].astype(np.float32)
