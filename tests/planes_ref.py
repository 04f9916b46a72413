"""numpy / scipy fp64 restatement of detection_3d_amd/csrc/planes.hip's semantics and the clouds the plane
tests run on, in the style of tests/clean_ref.py.  Pairs come from a k-d tree at 1.001 r; the three quantities of an edge
(d2, |nP . nC|, max(|nP . d|, |nC . d|)) are computed in fp64 from the fp32 inputs and two labellings are returned:
"lo" with every threshold tightened and "hi" with every threshold loosened,
    d2 <= r^2 (1 -+ EDGE_REL),   |c| >= cos_min +- 1e-6,   e <= offset (1 -+ EDGE_REL) -+ 1e-7 r.
An fp32 dot of unit vectors is off by under 4e-7 and e by under 4e-7 r, so where lo and hi agree the fp32 kernel must
give exactly that labelling.  tests/test_planes_cpu.py asserts that they agree on every cloud the GPU tests compare."""
import math

import numpy as np
from scipy.spatial import cKDTree

from tests import clean_ref
from tests.normals_ref import EDGE_REL, canonical_sign, dense_patch

SHIFT = (12.5, -7.25, 1.0)
ROOM = (4.0, 3.0, 2.5)


def edges_ref(xyz, normals, radius, angle, offset):
    """-> (pairs int64 [M, 2], lo bool [M], hi bool [M]) over the pairs of finite positions within 1.001 r"""
    p = np.asarray(xyz, np.float32)[:, :3].astype(np.float64)
    nr = np.asarray(normals, np.float32).astype(np.float64)
    r = float(np.float32(radius))
    r2 = r * r
    cm = float(np.float32(math.cos(float(angle) * math.pi / 180.0)))
    off = float(np.float32(offset))
    rows = np.flatnonzero(np.isfinite(p).all(1))
    if rows.size < 2:
        return np.zeros((0, 2), np.int64), np.zeros(0, bool), np.zeros(0, bool)
    pairs = rows[cKDTree(p[rows]).query_pairs(1.001 * r, output_type="ndarray")]
    a, b = pairs[:, 0], pairs[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        d = p[b] - p[a]
        d2 = (d * d).sum(1)
        c = np.abs((nr[a] * nr[b]).sum(1))
        e = np.maximum(np.abs((nr[a] * d).sum(1)), np.abs((nr[b] * d).sum(1)))      # a NaN stays a NaN and fails
        lo = (d2 <= r2 * (1.0 - EDGE_REL)) & (c >= cm + 1e-6) & (e <= off * (1.0 - EDGE_REL) - 1e-7 * r)
        hi = (d2 <= r2 * (1.0 + EDGE_REL)) & (c >= cm - 1e-6) & (e <= off * (1.0 + EDGE_REL) + 1e-7 * r)
    return pairs, lo, hi


def segment_ref(xyz, normals, radius=0.1, angle=10.0, offset=0.02):
    """-> ((label, size) of "lo", (label, size) of "hi"): label int32 [N] the smallest row index of the point's patch, size
    int32 [N] its number of points"""
    n = np.asarray(xyz).shape[0]
    pairs, lo, hi = edges_ref(xyz, normals, radius, angle, offset)
    return tuple(clean_ref._labels(n, pairs[sel, 0], pairs[sel, 1]) for sel in (lo, hi))


def plane_lists_ref(label, size, min_points, cap=4096):
    """-> (plane_of_point int32 [N], the labels of the planes ascending): the patches of at least min_points points, the
    `cap` largest of them (ties to the lower label)"""
    label, size = np.asarray(label), np.asarray(size)
    heads = np.flatnonzero((label == np.arange(label.shape[0])) & (size >= min_points))
    if heads.size > cap:
        heads = np.sort(heads[np.argsort(-size[heads].astype(np.int64), kind="stable")[:cap]])
    number = np.full(label.shape[0] + 1, -1, np.int32)
    number[heads] = np.arange(heads.size, dtype=np.int32)
    return (number[label] if label.shape[0] else number[:0]), heads


def fit_ref(xyz, plane_of_point, k):
    """math.fsum moments about each plane's first row and numpy.linalg.eigh, fp64 -> dict of normal [k, 3] (canonical
    sign), d, centroid [k, 3], count, rms, eigenvalues [k, 3] ascending, gap = (l1 - l0) / l2 (inf: no plane)"""
    p = np.asarray(xyz, np.float32)[:, :3].astype(np.float64)
    out = {"normal": np.zeros((k, 3)), "d": np.zeros(k), "centroid": np.zeros((k, 3)), "count": np.zeros(k, np.int32),
           "rms": np.zeros(k), "eigenvalues": np.zeros((k, 3)), "gap": np.full(k, np.inf)}
    for g in range(k):
        rows = np.flatnonzero(plane_of_point == g)
        m = rows.size
        out["count"][g] = m
        if m == 0:
            continue
        o = p[rows[0]]
        q = p[rows] - o
        mean = np.array([math.fsum(q[:, a]) for a in range(3)]) / m
        out["centroid"][g] = o + mean
        cov = np.array([[math.fsum(q[:, a] * q[:, b]) / m - mean[a] * mean[b] for b in range(3)] for a in range(3)])
        w, v = np.linalg.eigh(cov)
        if not w[2] > 0.0:
            continue
        out["eigenvalues"][g] = w
        out["normal"][g] = canonical_sign(v[:, 0])
        out["d"][g] = float(out["normal"][g] @ out["centroid"][g])
        out["rms"][g] = math.sqrt(max(w[0], 0.0))
        out["gap"][g] = (w[1] - w[0]) / w[2]
    return out


# ---- clouds: (xyz fp32 [N, 3], normals fp32 [N, 3]), every normal synthetic ----
def room_faces():
    """the 7 faces of the room: (origin, edge u, edge v, unit normal), a point of the face is origin + s u + t v"""
    lx, ly, lz = ROOM
    return [((0, 0, 0), (lx, 0, 0), (0, ly, 0), (0, 0, 1)),            # floor
            ((0, 0, lz), (lx, 0, 0), (0, ly, 0), (0, 0, 1)),           # ceiling
            ((0, 0, 0), (0, ly, 0), (0, 0, lz), (1, 0, 0)),            # wall x = 0
            ((lx, 0, 0), (0, ly, 0), (0, 0, lz), (1, 0, 0)),           # wall x = 4
            ((0, 0, 0), (lx, 0, 0), (0, 0, lz), (0, 1, 0)),            # wall y = 0
            ((0, ly, 0), (lx, 0, 0), (0, 0, lz), (0, 1, 0)),           # wall y = 3
            ((2.0, 0, 0), (0, 1.8, 0), (0, 0, lz), (1, 0, 0))]         # interior wall at x = 2, 1.8 m long


def _jittered(rs, m, aspect):
    """m points of the unit square, one at a random place in each of m randomly chosen cells of a grid of about m square
    cells (aspect = the face's length along s over that along t)"""
    a = max(1, int(round(math.sqrt(m * aspect))))
    b = -(-m // a)
    cell = rs.permutation(a * b)[:m]
    return (np.column_stack([cell // b, cell % b]) + rs.rand(m, 2)) / np.array([a, b])


def make_room(n=12000, seed=0):
    """Floor, ceiling, four walls of a 4 x 3 x 2.5 m room and a 1.8 m interior wall at x = 2; points per face by area, one
    per cell of a grid over the face (at this density, 6 neighbours within 0.1 m, a uniform draw sits so close to the
    percolation threshold of the neighbour graph that whether a face stays one patch is a property of the draw), 2 mm
    of Gaussian noise along the face normal; normals: the face normal plus tan(2 deg) randn(3), normalised, with a random
    sign per point; everything shifted by SHIFT, rows permuted -> (xyz fp32 [n, 3], normals fp32 [n, 3], face int [n])"""
    rs = np.random.RandomState(seed)
    faces = room_faces()
    area = np.array([np.linalg.norm(np.cross(u, v)) for _, u, v, _ in faces])
    cnt = np.floor(n * area / area.sum()).astype(int)
    cnt[0] += n - cnt.sum()
    face = np.repeat(np.arange(len(faces)), cnt)
    o, u, v, nv = (np.asarray([f[j] for f in faces], np.float64)[face] for j in range(4))
    st = np.concatenate([_jittered(rs, c, np.linalg.norm(f[1]) / np.linalg.norm(f[2])) for c, f in zip(cnt, faces)])
    pts = o + st[:, :1] * u + st[:, 1:] * v + rs.randn(n, 1) * 0.002 * nv
    nrm = nv + math.tan(math.radians(2.0)) * rs.randn(n, 3)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm *= np.where(rs.rand(n, 1) < 0.5, -1.0, 1.0)
    perm = rs.permutation(n)
    return (pts + np.array(SHIFT))[perm].astype(np.float32), nrm[perm].astype(np.float32), face[perm]


def _up(n):
    return np.tile(np.float32([0, 0, 1]), (n, 1))


def make_sheets(m=1500, seed=2):
    """two parallel 1 x 1 m planes 0.05 m apart with identical normals +z, m points each, rows permuted"""
    rs = np.random.RandomState(seed)
    xy = rs.rand(2 * m, 2)
    z = np.where(np.arange(2 * m) < m, 0.0, 0.05)
    xyz = np.column_stack([xy, z]) + np.array(SHIFT)
    return xyz[rs.permutation(2 * m)].astype(np.float32), _up(2 * m)


def make_fold(degrees, m=1500, seed=3):
    """two 1 x 1 m half-planes meeting along the y axis at `degrees`, exact normals, m points each, rows permuted"""
    rs = np.random.RandomState(seed)
    th = math.radians(degrees)
    a = np.column_stack([-rs.rand(m), rs.rand(m), np.zeros(m)])
    t = rs.rand(m)
    b = np.column_stack([t * math.cos(th), rs.rand(m), t * math.sin(th)])
    nrm = np.concatenate([np.tile([0.0, 0.0, 1.0], (m, 1)), np.tile([-math.sin(th), 0.0, math.cos(th)], (m, 1))])
    perm = rs.permutation(2 * m)
    return (np.concatenate([a, b]) + np.array(SHIFT))[perm].astype(np.float32), nrm[perm].astype(np.float32)


def make_chains(radius=0.1):
    xyz = clean_ref.make_chains(radius)
    return xyz, _up(xyz.shape[0])


def make_dense(m=1500, seed=5):
    xyz = dense_patch(m, seed)
    return xyz, _up(m)


BAD_SHEET = 400     # rows of the sheet in make_bad_rows; the special rows follow


def make_bad_rows():
    """A 20 x 20 sheet of points 5 cm apart with normals +z, then rows 400.. : on the sheet (between its points, the
    fifth in line with a column of it) a zero normal, a NaN normal, (inf, inf, inf), (inf, 0, 0) and (0, 0, inf); a NaN
    position with a good normal; a metre above, two rows at one position with perpendicular normals and two rows at
    another position with equal normals.  -> (xyz, normals); the sheet is one patch, rows 400:408 are singletons, rows
    408 and 409 are joined."""
    g = np.arange(20) * 0.05
    sheet = np.column_stack([np.repeat(g, 20), np.tile(g, 20), np.zeros(400)])
    inf, nan = np.inf, np.nan
    special = [((0.225, 0.225, 0), (0, 0, 0)), ((0.425, 0.225, 0), (nan, 0, 1)), ((0.625, 0.225, 0), (inf, inf, inf)),
               ((0.25, 0.625, 0), (inf, 0, 0)), ((0.625, 0.625, 0), (0, 0, inf)), ((nan, 0.5, 0), (0, 0, 1)),
               ((0.5, 0.5, 1.0), (0, 0, 1)), ((0.5, 0.5, 1.0), (1, 0, 0)),
               ((0.8, 0.5, 1.0), (0, 1, 0)), ((0.8, 0.5, 1.0), (0, 1, 0))]
    xyz = np.concatenate([sheet, np.array([s[0] for s in special], np.float64)]) + np.array(SHIFT)
    nrm = np.concatenate([np.tile([0.0, 0.0, 1.0], (400, 1)), np.array([s[1] for s in special], np.float64)])
    return xyz.astype(np.float32), nrm.astype(np.float32)


def make_line(n):
    """n points 5 cm apart on a line, normals +z: one patch (n = 0: empty)"""
    xyz = np.column_stack([np.arange(n) * 0.05, np.zeros(n), np.zeros(n)]) + np.array(SHIFT)
    return xyz.astype(np.float32).reshape(n, 3), _up(n).reshape(n, 3)


# every (cloud, radius, angle, offset) whose GPU labelling is compared with segment_ref; test_planes_cpu.py asserts
# lo == hi on each
CASES = {
    "room0": (lambda: make_room(12000, 0)[:2], 0.1, 10.0, 0.02),
    "room1": (lambda: make_room(12000, 1)[:2], 0.1, 10.0, 0.02),
    "sheets": (make_sheets, 0.1, 10.0, 0.02),
    "sheets_wide": (make_sheets, 0.1, 10.0, 0.06),
    "fold8": (lambda: make_fold(8.0), 0.1, 10.0, 0.02),
    "fold30": (lambda: make_fold(30.0), 0.1, 10.0, 0.02),
    "chains": (make_chains, 0.1, 10.0, 0.02),
    "chains_half": (make_chains, 0.05, 10.0, 0.02),
    "dense": (make_dense, 0.1, 10.0, 0.02),
    "bad": (make_bad_rows, 0.1, 10.0, 0.02),
    "line1": (lambda: make_line(1), 0.1, 10.0, 0.02),
    "line2": (lambda: make_line(2), 0.1, 10.0, 0.02),
    "line63": (lambda: make_line(63), 0.1, 10.0, 0.02),
    "line64": (lambda: make_line(64), 0.1, 10.0, 0.02),
    "line65": (lambda: make_line(65), 0.1, 10.0, 0.02),
}

_CACHE = {}


def case(name):
    """-> (xyz, normals, radius, angle, offset, (label, size) of lo, (label, size) of hi), computed once"""
    if name not in _CACHE:
        make, radius, angle, offset = CASES[name]
        xyz, nrm = make()
        lo, hi = segment_ref(xyz, nrm, radius, angle, offset)
        _CACHE[name] = (xyz, nrm, radius, angle, offset, lo, hi)
    return _CACHE[name]
