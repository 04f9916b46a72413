"""What the rotated-NMS tests share and a machine without a GPU can check (test_nms_forms_cpu.py): lattice scenes whose
suppression graph is known in exact rational arithmetic, families of hard box pairs with two references, and the
dispatch of d3d_rotate_nms_3d_batched restated -- the record d3d_nms_last_form must give.

Boxes are yx_zb rows (x, y, z0, d3, d4, dz, yaw); d3 is the extent along x at yaw 0.  A later box j is suppressed by a
kept earlier box i iff not (gate <= 0) and polygon IoU >= thr, where gate = fp32 BEV IoU (nms_gpu.py) x z-interval IoU
and the polygon IoU is the fp64 clip of the two fp32 quads (spconv's rotate_non_max_suppression_cpu).

LATTICE SCENES.  yaw = 0 and every coordinate and size a multiple of 1/8, at most 2048 (cells start below 256, so only a
structure longer than that reaches further): corners, differences, areas and the intersection rectangle are exact in
fp32 and in fp64, and below 512 so are the fp32 products of two coordinates.  The decision of a pair cannot depend on
rounding as long as its exact IoU is not thr itself; the builder asserts |IoU - thr| >= 1e-6 for every pair with a
positive intersection (the clip's t = dc / (dc - dn) may round, some 1e-16, hence a margin at all).
Structures: ("path", L) neighbours shifted 1/2 along x (IoU 3/5; next-nearest 1/3), ("cliquez", m <= 8) identical BEV
with z0 in steps of 1/8 (IoU 1, z intervals overlap), ("clique", m) 32 x 32 boxes shifted by multiples of 1/8 in x and
y, ("iso",) one box, ("ztouch",) two boxes of identical BEV whose z intervals only touch (no edge), ("zhalf",) the same
half a dz apart (an edge).  Every structure sits in a cell of its own, at least 8 away from the others in x or y, or 16
in z.  The adjacency is computed with fractions.Fraction from the boxes (all pairs whose integer rectangles and z
intervals overlap -- found with integer arithmetic -- whatever structure they belong to) and the expected keep list
is greedy() over it: neither the oracle nor the library is involved.

HARD PAIRS.  families() generates (A, B, thr, clamp) per family, A scored before B.  Two references:
 * the contract: oracle.nms_pair (gate, polygon IoU) -> pair_decision_oracle;
 * pair_iou_f64: corners from fp64 cos / sin of the fp32 fields, Sutherland-Hodgman clip, shoelace areas, all fp64 numpy.
A pair is doubtful if its fp64 IoU lies within delta of thr; delta = 4 x the largest |oracle IoU - fp64 IoU| over all
finite pairs of all families, measured by measure() on the CPU (the two differ by the fp32 rounding of the oracle's
corners).  Measured with the seeds below (test_nms_forms_cpu.py asserts that a fresh measurement reproduces them):

  delta = 4 x 3.65e-5 = 1.46e-4 (DELTA_RECORDED; the largest difference is a pair of far_200, where an fp32 corner
  carries 1.5e-5 of rounding; without that family it is 2.0e-6, a near-parallel wall)

  family                pairs  thr    doubtful      suppress  gate <= 0 exceptions
  identical              300  0.5      0 (0.00 %)    300    0
  same_below_1e-6        300  0.9      0 (0.00 %)    300    0
  same_above_1e-6        300  0.9      0 (0.00 %)    300    0
  contained              300  0.3      0 (0.00 %)    207    0
  crossing_walls         300  0.01     5 (1.67 %)     41    0
  shared_edge_corner     300  0.01     0 (0.00 %)      0    0
  near_parallel_walls    300  0.45     0 (0.00 %)     82    0
  special_yaw            300  0.5      0 (0.00 %)     30    0
  tiny_sizes             300  0.3      0 (0.00 %)     28    0
  tiny_sizes_clamped     300  0.3      0 (0.00 %)    161    0
  z_intervals            300  0.5      0 (0.00 %)     46    0
  far_200                300  0.45     0 (0.00 %)     84    0
  generic_thr_0.01       300  0.01     0 (0.00 %)    234    0
  generic_thr_0.3        300  0.3      1 (0.33 %)    150    0
  generic_thr_0.45       300  0.45     0 (0.00 %)     66    0
  generic_thr_0.5        300  0.5      0 (0.00 %)     51    0
  generic_thr_0.9        300  0.9      1 (0.33 %)    144    0
  non_finite             252  0.3      0 (0.00 %)     48    0
  non_finite_clamped     252  0.3      0 (0.00 %)     61    0

Outside the band the oracle and the fp64 reference agree on every pair, except pairs whose fp32 gate is <= 0 although
the fp64 intersection is positive (the fp32 polygon of nms_gpu.py collapses: nearly coincident edges cross at no
point, or at a wrong one); the contract is the oracle's decision for them as well.  They are counted against
FAMILY_RECORD: with these seeds there is none (GATE_EXCEPTIONS_RECORDED = 0).  The non-finite families have no fp64 IoU (the reference is the oracle alone: one NaN / +Inf / -Inf field in
A or in B).  What the reference's Python gives there: torch.clamp(min=) keeps a NaN size; iou_one_dim's torch.min /
torch.max make iou_z = overlap / common NaN when a z bound is NaN, z0 = +-Inf gives -inf / inf = NaN, and two equal point
intervals (dz = 0) give 0 / 0 = NaN; the sweep's gate `iou3d <= 0 -> skip` lets a NaN pass, so such a pair is decided
on its BEV polygon alone.  dz = +-Inf gives iou_z = 0 or below and is skipped; NaN or Inf in a BEV field never
suppresses (no polygon with a positive area).  The oracle and the kernels follow that."""
import math
from fractions import Fraction

import numpy as np

# ---------------------------------------------------------------------------------------------------- the record
NMS_FIELDS = ("family", "ncbmax", "ncb", "segments", "n_max", "max_keep", "lds_bytes")
REGS, LDS = 1, 2
MODE_DEFAULT, MODE_REGS, MODE_LDS = 0, 1, 2
N_LIMIT = 4096                  # 1 << kNmsIdxBits
SW_STAGES = 4                   # kSwStages


def expect_form(n_max, mode, segments=1, max_keep=0):
    """d3d_rotate_nms_3d_batched's choice for a launch (n_max > 0, segments > 0)."""
    ncb = (n_max + 63) // 64
    mk = max_keep if max_keep > 0 else n_max
    if mode == MODE_REGS:
        f = (REGS, 0, ncb, segments, n_max, mk, 0)
    else:
        f = (LDS, 16 if ncb <= 16 else 32 if ncb <= 32 else 64, ncb, segments, n_max, mk, 2 * 64 * (ncb + 1) * 8)
    return dict(zip(NMS_FIELDS, f))


# ---------------------------------------------------------------------------------------------------- lattice scenes
U = 8                           # lattice units per metre
CELL_GAP = 8 * U
XY_LIMIT = 256 * U
Z_LAYER = 16 * U


def _struct_boxes(kind, *arg):
    """integer rows (x, y, z0, d3, d4, dz) in units of 1/8, relative to the cell's corner (centres offset so that no
    coordinate is negative), in the structure's natural order"""
    if kind == "path":
        return [(U + i * U // 2, U, 0, 2 * U, U, U) for i in range(arg[0])]
    if kind == "cliquez":
        assert 1 <= arg[0] <= 8
        return [(U, U, k, 2 * U, U, U) for k in range(arg[0])]
    if kind == "clique":
        m, w = arg[0], max(1, int(math.ceil(math.sqrt(arg[0]))))
        return [(16 * U + (k % w), 16 * U + (k // w), 0, 32 * U, 32 * U, U) for k in range(m)]
    if kind == "iso":
        return [(U, U, 0, 2 * U, U, U)]
    if kind == "ztouch":
        return [(U, U, 0, 2 * U, U, U), (U, U, U, 2 * U, U, U)]
    if kind == "zhalf":
        return [(U, U, 0, 2 * U, U, U), (U, U, U // 2, 2 * U, U, U)]
    raise ValueError(kind)


def _exact_edges(q, thr):
    """q int64 [n, 6] lattice rows -> list of (i, j, IoU) for i < j with IoU >= thr, by Fraction; asserts the margin"""
    n = q.shape[0]
    x0, x1 = 2 * q[:, 0] - q[:, 3], 2 * q[:, 0] + q[:, 3]          # doubled: half sizes stay integers
    y0, y1 = 2 * q[:, 1] - q[:, 4], 2 * q[:, 1] + q[:, 4]
    z0, z1 = q[:, 2], q[:, 2] + q[:, 5]
    t = Fraction(float(np.float32(thr)))
    edges = []
    for a in range(0, n, 512):
        s = slice(a, min(a + 512, n))
        ix = np.minimum(x1[s, None], x1[None]) - np.maximum(x0[s, None], x0[None])
        iy = np.minimum(y1[s, None], y1[None]) - np.maximum(y0[s, None], y0[None])
        iz = np.minimum(z1[s, None], z1[None]) - np.maximum(z0[s, None], z0[None])
        ii, jj = np.nonzero((ix > 0) & (iy > 0) & (iz > 0))
        for i, j in zip(ii + a, jj):
            if i >= j:
                continue
            inter = Fraction(int(ix[i - a, j]) * int(iy[i - a, j]), 4 * U * U)
            union = Fraction(int(q[i, 3] * q[i, 4] + q[j, 3] * q[j, 4]), U * U) - inter
            iou = inter / union
            assert abs(iou - t) >= Fraction(1, 10 ** 6), (i, j, iou, thr)
            if iou >= t:
                edges.append((int(i), int(j), iou))
    return edges


def lattice_scene(structs, perm=None, thr=0.5):
    """structs: list of structure tuples; perm[p] = construction index (structures concatenated in their natural order)
    of the box at sweep position p (None: identity).  -> dict: boxes float32 [n, 7] in sweep order, scores float32 [n]
    strictly descending, adj (list of sorted neighbour lists, sweep positions), struct (structure index per sweep
    position), keep (the greedy list), thr."""
    rows, owner = [], []
    cx = cy = cz = 0
    shelf = 0
    for si, st in enumerate(structs):
        b = np.asarray(_struct_boxes(*st), np.int64)
        w = int((b[:, 0] + (b[:, 3] + 1) // 2).max()) + 1
        h = int((b[:, 1] + (b[:, 4] + 1) // 2).max()) + 1
        if cx + w > XY_LIMIT:
            cx, cy, shelf = 0, cy + shelf + CELL_GAP, 0
        if cy + h > XY_LIMIT:
            cx, cy, cz, shelf = 0, 0, cz + Z_LAYER, 0
        b = b.copy()
        b[:, 0] += cx
        b[:, 1] += cy
        b[:, 2] += cz
        rows.append(b)
        owner += [si] * b.shape[0]
        cx += w + CELL_GAP
        shelf = max(shelf, h)
    q = np.concatenate(rows) if rows else np.zeros((0, 6), np.int64)
    n = q.shape[0]
    assert q[:, :3].max(initial=0) <= 2048 * U
    perm = np.arange(n) if perm is None else np.asarray(perm)
    assert sorted(perm.tolist()) == list(range(n))
    q = q[perm]
    boxes = np.zeros((n, 7), np.float32)
    boxes[:, :6] = q.astype(np.float64) / U                   # exact
    scores = (1.0 - np.arange(n, dtype=np.float64) / (2.0 * max(n, 1))).astype(np.float32)
    assert n < 2 or np.all(np.diff(scores) < 0)
    adj = [[] for _ in range(n)]
    for i, j, _ in _exact_edges(q, thr):
        adj[i].append(j)
        adj[j].append(i)
    adj = [sorted(a) for a in adj]
    return dict(boxes=boxes, scores=scores, adj=adj, struct=np.asarray(owner, np.int64)[perm], keep=greedy(adj), thr=thr)


def greedy(adj, cap=None):
    """the survivors of a greedy sweep over positions 0, 1, ... of a suppression graph; at most `cap` of them"""
    removed, keep = [False] * len(adj), []
    for i in range(len(adj)):
        if removed[i]:
            continue
        keep.append(i)
        for j in adj[i]:
            if j > i:
                removed[j] = True
    return keep if cap is None else keep[:cap]


def mixed_structs(n, seed):
    """paths, cliques and isolated boxes with exactly n boxes in all"""
    rng = np.random.RandomState(seed)
    out, left = [], n
    menu = [("path", 2), ("path", 3), ("path", 5), ("path", 9), ("path", 17), ("path", 70), ("cliquez", 2), ("cliquez", 8),
            ("clique", 3), ("clique", 20), ("iso",), ("iso",), ("iso",), ("ztouch",), ("zhalf",)]
    while left > 0:
        st = menu[rng.randint(len(menu))]
        size = len(_struct_boxes(*st))
        if size > left:
            st = ("path", left) if left > 1 else ("iso",)
            size = left
        out.append(st)
        left -= size
    return out


def mixed_scene(n, seed, thr=0.5):
    st = mixed_structs(n, seed)
    return lattice_scene(st, np.random.RandomState(seed + 1).permutation(n), thr)


def place(n, chosen, seed=0):
    """a permutation for lattice_scene that puts construction index chosen[k][1] at sweep position chosen[k][0] and the
    rest in random order"""
    pos = dict(chosen)
    assert len(set(pos.values())) == len(pos)
    rest = [c for c in np.random.RandomState(seed).permutation(n).tolist() if c not in set(pos.values())]
    perm, it = [], iter(rest)
    for p in range(n):
        perm.append(pos[p] if p in pos else next(it))
    return np.asarray(perm)


def shuffled_with_ties(scene, seed):
    """the scene as d3d_rotate_nms_3d takes it: boxes in a random input order and scores with ties (runs of three equal
    values) whose defined order -- descending score, equal scores: lower input index first -- is the scene's sweep order.
    -> boxes [n, 7], scores [n], slot (input index of every sweep position)"""
    n = scene["boxes"].shape[0]
    slot = np.random.RandomState(seed).permutation(n)
    for a in range(0, n, 3):
        slot[a:a + 3] = np.sort(slot[a:a + 3])
    boxes = np.zeros_like(scene["boxes"])
    scores = np.zeros(n, np.float32)
    boxes[slot] = scene["boxes"]
    scores[slot] = (1.0 - (np.arange(n) // 3) / (2.0 * max(n, 1))).astype(np.float32)
    return boxes, scores, slot


SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 193, 256, 320, 1023, 1024, 1025, 2047, 2048, 2049, 4032, 4033, 4096)
_SCENES = {}


def size_scene(n):
    """the size-edge scene of n boxes: paths, cliques and isolated boxes in a random permutation (built once)"""
    if ("size", n) not in _SCENES:
        _SCENES[("size", n)] = mixed_scene(n, 1000 + n)
    return _SCENES[("size", n)]


def restrict(scene, sel):
    """the scene of the boxes at sweep positions sel, swept in that order: (boxes, adjacency, greedy keep)"""
    pos = {int(b): p for p, b in enumerate(sel)}
    adj = [sorted(pos[j] for j in scene["adj"][int(b)] if j in pos) for b in sel]
    return scene["boxes"][np.asarray(sel, np.int64)], adj, greedy(adj)


def structure_scene(name):
    """the structure cases (built once): name -> scene, with the keep list the case is about in scene['want'] where it
    has a closed form"""
    if ("st", name) in _SCENES:
        return _SCENES[("st", name)]
    if name == "path64":                      # one chunk, in sweep order: 64 fixed-point steps
        sc = lattice_scene([("path", 64)])
        sc["want"] = list(range(0, 64, 2))
    elif name == "path64_reversed":
        sc = lattice_scene([("path", 64)], np.arange(64)[::-1])
        sc["want"] = list(range(0, 64, 2))
    elif name == "path128":                   # the chain crosses the chunk boundary
        sc = lattice_scene([("path", 128)])
        sc["want"] = list(range(0, 128, 2))
    elif name == "clique64":
        sc = lattice_scene([("clique", 64)])
        sc["want"] = [0]
    elif name == "clique_every_chunk":        # n = 2049: 33 chunks, the last one holds one box, a clique member
        n, m = 2049, 33
        st = [("clique", m)] + mixed_structs(n - m, 7)
        chosen = [(64 * k + (17 * k) % 64 if k < 32 else 2048, k) for k in range(m)]
        sc = lattice_scene(st, place(n, chosen, 8))
        assert all(p in sc["adj"][chosen[0][0]] for p, _ in chosen[1:])
        assert chosen[0][0] in sc["keep"] and not any(p in sc["keep"] for p, _ in chosen[1:])
    elif name == "chunk_all_suppressed":      # chunk 1 = the partners of chunk 0, chunk 2 isolated
        st = [("path", 2)] * 64 + [("iso",)] * 64
        perm = [2 * p for p in range(64)] + [2 * p + 1 for p in range(64)] + list(range(128, 192))
        sc = lattice_scene(st, perm)
        sc["want"] = list(range(64)) + list(range(128, 192))
    elif name == "all_isolated":              # 5 chunks; the count after chunk c is exactly 64 (c + 1)
        sc = lattice_scene([("iso",)] * 320)
        sc["want"] = list(range(320))
    elif name == "mixed1100":
        sc = mixed_scene(1100, 31)
    else:
        raise ValueError(name)
    if "want" in sc:
        assert sc["keep"] == sc["want"], name
    _SCENES[("st", name)] = sc
    return sc


STRUCTURES = ("path64", "path64_reversed", "path128", "clique64", "clique_every_chunk", "chunk_all_suppressed",
              "all_isolated", "mixed1100")


def identical_at_one(n=64):
    """pairs of identical lattice boxes for thr = 1.0: all arithmetic on them is exact (no edge of the clip is crossed, so
    no quotient is formed), IoU == 1.0 == thr in every arithmetic, and `>=` suppresses.  The one place where a lattice
    IoU equals thr; the margin rule of lattice_scene does not apply to it.  -> boxes [2 n, 7], pair p = rows 2p, 2p + 1"""
    rng = np.random.RandomState(5)
    b = np.zeros((n, 7), np.float32)
    b[:, 0:2] = rng.randint(0, 64 * U, (n, 2)) / U
    b[:, 2] = rng.randint(0, 4 * U, n) / U
    b[:, 3:5] = rng.randint(1, 8 * U, (n, 2)) / U
    b[:, 5] = rng.randint(1, 2 * U, n) / U
    two = np.repeat(b, 2, axis=0)
    two[1::2, 2] += (rng.randint(0, 2, n) * (b[:, 5] * U // 2) / U).astype(np.float32)     # same BEV, z moved by < dz
    return two


# ---------------------------------------------------------------------------------------------------- hard pairs
THRS = (0.01, 0.3, 0.45, 0.5, 0.9)
DELTA_RECORDED = 1.46e-4
FAMILY_RECORD = {        # name: (pairs, thr, doubtful pairs, pairs the oracle suppresses)
    "identical": (300, 0.5, 0, 300),
    "same_below_1e-6": (300, 0.9, 0, 300),
    "same_above_1e-6": (300, 0.9, 0, 300),
    "contained": (300, 0.3, 0, 207),
    "crossing_walls": (300, 0.01, 5, 41),
    "shared_edge_corner": (300, 0.01, 0, 0),
    "near_parallel_walls": (300, 0.45, 0, 82),
    "special_yaw": (300, 0.5, 0, 30),
    "tiny_sizes": (300, 0.3, 0, 28),
    "tiny_sizes_clamped": (300, 0.3, 0, 161),
    "z_intervals": (300, 0.5, 0, 46),
    "far_200": (300, 0.45, 0, 84),
    "generic_thr_0.01": (300, 0.01, 0, 234),
    "generic_thr_0.3": (300, 0.3, 1, 150),
    "generic_thr_0.45": (300, 0.45, 0, 66),
    "generic_thr_0.5": (300, 0.5, 0, 51),
    "generic_thr_0.9": (300, 0.9, 1, 144),
    "non_finite": (252, 0.3, 0, 48),
    "non_finite_clamped": (252, 0.3, 0, 61),
}
GATE_EXCEPTIONS_RECORDED = 0    # pairs outside the band on which the two references differ (all would have gate <= 0)
DOUBTFUL_CAP = 0.02


def clamp_sizes(b, clamp):
    b = np.array(b, np.float32, copy=True)
    b[:, 3:5] = np.maximum(b[:, 3:5], np.float32(clamp[0]))          # np.maximum keeps a NaN, as torch.clamp does
    b[:, 5] = np.maximum(b[:, 5], np.float32(clamp[1]))
    return b


def _corners64(b):
    c, s = math.cos(float(b[6])), math.sin(float(b[6]))
    xd, yd = float(b[3]), float(b[4])
    return [(c * px + s * py + float(b[0]), -s * px + c * py + float(b[1]))
            for px, py in ((-xd / 2, -yd / 2), (-xd / 2, yd / 2), (xd / 2, yd / 2), (xd / 2, -yd / 2))]


def _shoelace(p):
    return 0.5 * abs(sum(p[i][0] * p[(i + 1) % len(p)][1] - p[(i + 1) % len(p)][0] * p[i][1] for i in range(len(p))))


def _clip(subject, clipper):
    """Sutherland-Hodgman: convex `subject` cut by the half-planes of convex `clipper` (either orientation)"""
    sgn = 1.0 if sum(clipper[i][0] * clipper[(i + 1) % 4][1] - clipper[(i + 1) % 4][0] * clipper[i][1]
                     for i in range(4)) >= 0 else -1.0
    out = list(subject)
    for e in range(4):
        (x1, y1), (x2, y2) = clipper[e], clipper[(e + 1) % 4]
        src, out = out, []
        for i in range(len(src)):
            cur, nxt = src[i], src[(i + 1) % len(src)]
            dc = sgn * ((x2 - x1) * (cur[1] - y1) - (y2 - y1) * (cur[0] - x1))
            dn = sgn * ((x2 - x1) * (nxt[1] - y1) - (y2 - y1) * (nxt[0] - x1))
            if dc >= 0:
                out.append(cur)
            if (dc >= 0) != (dn >= 0):
                t = dc / (dc - dn)
                out.append((cur[0] + t * (nxt[0] - cur[0]), cur[1] + t * (nxt[1] - cur[1])))
        if not out:
            break
    return out


def pair_iou_f64(a, b):
    """(BEV IoU, gate) of two clamped fp32 rows, everything after the inputs in fp64; gate = IoU x z-interval IoU, NaN
    where the z intervals are one point (0 / 0), as the reference's tensor arithmetic gives it"""
    pa, pb = _corners64(a), _corners64(b)
    poly = _clip(pa, pb)
    ia = _shoelace(poly) if len(poly) >= 3 else 0.0
    ua = _shoelace(pa) + _shoelace(pb) - ia
    iou = ia / ua if ia > 0 and ua > 0 else 0.0
    za0, za1 = float(a[2]), float(a[2]) + float(a[5])
    zb0, zb1 = float(b[2]), float(b[2]) + float(b[5])
    overlap, common = min(za1, zb1) - max(za0, zb0), max(za1, zb1) - min(za0, zb0)
    return iou, iou * (overlap / common if common != 0 else math.nan)


def _rand_boxes(rng, n, lo=0.5, hi=4.0):
    b = np.zeros((n, 7), np.float64)
    b[:, 0:2] = rng.uniform(-5, 5, (n, 2))
    b[:, 2] = rng.uniform(0, 1, n)
    b[:, 3:5] = rng.uniform(lo, hi, (n, 2))
    b[:, 5] = rng.uniform(1.0, 3.0, n)
    b[:, 6] = rng.uniform(-math.pi, math.pi, n)
    return b


def _shifted(rng, a, frac=0.6, dyaw=0.3):
    """a partner for every row of a: moved by up to `frac` of its size in its own frame, turned by up to dyaw, resized"""
    n = a.shape[0]
    b = a.copy()
    u, v = rng.uniform(-frac, frac, n) * a[:, 3], rng.uniform(-frac, frac, n) * a[:, 4]
    c, s = np.cos(a[:, 6]), np.sin(a[:, 6])
    b[:, 0] += c * u + s * v
    b[:, 1] += -s * u + c * v
    b[:, 3:5] *= rng.uniform(0.8, 1.25, (n, 2))
    b[:, 6] += rng.uniform(-dyaw, dyaw, n)
    return b


def _f32(x):
    return np.ascontiguousarray(x, np.float32)


def families():
    """-> dict name -> dict(a, b float32 [n, 7] (unclamped), thr, clamp (min_yx, min_z), both (whether suppressed and
    unsuppressed pairs must both occur), finite)"""
    fam = {}

    def add(name, a, b, thr, clamp=(0.0, 0.0), both=True, finite=True):
        fam[name] = dict(a=_f32(a), b=_f32(b), thr=thr, clamp=clamp, both=both, finite=finite)

    n = 300
    rng = np.random.RandomState(101)
    a = _rand_boxes(rng, n)
    add("identical", a, a, 0.5, both=False)

    # fields differing by a few ulps (< 1e-6: the `same` override of check_same_boxes) and by 1.1e-6 .. 3e-6 (no override)
    rng = np.random.RandomState(102)
    a = _f32(_rand_boxes(rng, n, 1.0, 3.5))
    a[:, 0:2] = rng.uniform(1.0, 3.9, (n, 2))
    a[:, 6] = rng.uniform(0.6, 1.5, n) * rng.choice([-1, 1], n)
    b = a.copy()
    for k in (0, 1, 3, 4, 6):
        ulps = rng.randint(-2, 3, n).astype(np.int32)
        b[:, k] = (np.ascontiguousarray(a[:, k]).view(np.int32) + ulps).view(np.float32)
    assert np.all(np.abs(b[:, [0, 1, 3, 4, 6]] - a[:, [0, 1, 3, 4, 6]]) < 1e-6)
    add("same_below_1e-6", a, b, 0.9, both=False)
    b = a.copy()
    for k in (0, 1, 3, 4, 6):
        b[:, k] = a[:, k] + (rng.uniform(1.1e-6, 3e-6, n) * rng.choice([-1, 1], n)).astype(np.float32)
    assert np.all(np.abs(b[:, [0, 1, 3, 4, 6]].astype(np.float64) - a[:, [0, 1, 3, 4, 6]]) > 1e-6)
    add("same_above_1e-6", a, b, 0.9, both=False)

    # one box inside the other: IoU = area ratio
    rng = np.random.RandomState(103)
    a = _rand_boxes(rng, n, 2.0, 4.0)
    b = a.copy()
    b[:, 3:5] *= np.sqrt(rng.uniform(0.03, 0.9, n))[:, None]
    u, v = rng.uniform(-0.4, 0.4, n) * (a[:, 3] - b[:, 3]), rng.uniform(-0.4, 0.4, n) * (a[:, 4] - b[:, 4])
    b[:, 0] += np.cos(a[:, 6]) * u + np.sin(a[:, 6]) * v
    b[:, 1] += -np.sin(a[:, 6]) * u + np.cos(a[:, 6]) * v
    swap = rng.rand(n) < 0.5
    a2, b2 = np.where(swap[:, None], b, a), np.where(swap[:, None], a, b)
    add("contained", a2, b2, 0.3)

    # perpendicular thin walls crossing: no corner of one inside the other, IoU ~ t / 2L
    rng = np.random.RandomState(104)
    a = _rand_boxes(rng, n)
    a[:, 3] = rng.uniform(3.0, 30.0, n)
    a[:, 4] = rng.uniform(0.1, 0.3, n)
    b = a.copy()
    b[:, 3] = rng.uniform(3.0, 30.0, n)
    b[:, 4] = rng.uniform(0.1, 0.3, n)
    b[:, 6] = a[:, 6] + math.pi / 2 + rng.uniform(-0.05, 0.05, n)
    u = rng.uniform(-0.3, 0.3, n) * a[:, 3]
    b[:, 0] += np.cos(a[:, 6]) * u
    b[:, 1] += -np.sin(a[:, 6]) * u
    add("crossing_walls", a, b, 0.01)

    # shared edge, shared corner: the intersection is a segment or a point (up to the rounding of the corners)
    rng = np.random.RandomState(105)
    a = _rand_boxes(rng, n)
    b = a.copy()
    b[:, 3:5] = rng.uniform(0.5, 4.0, (n, 2))
    u = (a[:, 3] + b[:, 3]) / 2
    v = np.where(rng.rand(n) < 0.5, (a[:, 4] + b[:, 4]) / 2, rng.uniform(-0.5, 0.5, n))   # corner / edge
    b[:, 0] = a[:, 0] + np.cos(a[:, 6]) * u + np.sin(a[:, 6]) * v
    b[:, 1] = a[:, 1] - np.sin(a[:, 6]) * u + np.cos(a[:, 6]) * v
    add("shared_edge_corner", a, b, 0.01, both=False)

    # near-parallel thin walls
    def thin(rng, n):
        a = _rand_boxes(rng, n)
        a[:, 3] = rng.uniform(2.0, 6.0, n)
        a[:, 4] = rng.uniform(0.08, 0.3, n)
        b = a.copy()
        b[:, 6] = a[:, 6] + 10.0 ** rng.uniform(-4, -2, n) * rng.choice([-1, 1], n)
        u, v = rng.uniform(-0.2, 0.2, n) * a[:, 3], rng.uniform(-1.2, 1.2, n) * a[:, 4]
        b[:, 0] += np.cos(a[:, 6]) * u + np.sin(a[:, 6]) * v
        b[:, 1] += -np.sin(a[:, 6]) * u + np.cos(a[:, 6]) * v
        return a, b
    rng = np.random.RandomState(106)
    a, b = thin(rng, n)
    add("near_parallel_walls", a, b, 0.45)

    # yaw at the special angles, exactly and with jitter
    rng = np.random.RandomState(107)
    a = _rand_boxes(rng, n)
    b = _shifted(rng, a, 0.5, 0.0)
    special = np.array([0.0, math.pi / 4, -math.pi / 4, math.pi / 2, -math.pi / 2, math.pi, -math.pi])
    jit = np.where(rng.rand(n) < 0.3, 0.0, 10.0 ** rng.uniform(-6, -3, n) * rng.choice([-1, 1], n))
    a[:, 6] = special[rng.randint(7, size=n)] + jit
    jit = np.where(rng.rand(n) < 0.3, 0.0, 10.0 ** rng.uniform(-6, -3, n) * rng.choice([-1, 1], n))
    b[:, 6] = special[rng.randint(7, size=n)] + jit
    add("special_yaw", a, b, 0.5)

    # sizes of 0 and 0.01, as they are and under the clamp
    rng = np.random.RandomState(108)
    a = _rand_boxes(rng, n)
    a[:, 3:6] = rng.choice([0.0, 0.01], (n, 3))
    a[: n // 3, 3] = rng.uniform(0.5, 2.0, n // 3)               # a third are thin walls of full length
    b = a.copy()
    b[:, 0:2] += rng.uniform(-0.25, 0.25, (n, 2))
    b[:, 2] += rng.uniform(-0.2, 0.2, n)
    b[:, 6] += rng.uniform(-0.3, 0.3, n)
    b[::4] = a[::4]                                                # and a quarter are identical
    add("tiny_sizes", a, b, 0.3)
    add("tiny_sizes_clamped", a, b, 0.3, clamp=(0.3, 0.3))

    # z: touching (dyadic values: the sum z0 + dz is exact), contained, partly overlapping -- on BEV pairs of both kinds
    rng = np.random.RandomState(109)
    a = _rand_boxes(rng, n)
    b = _shifted(rng, a, 0.5, 0.2)
    a[:, 2] = rng.randint(0, 64, n) / 64.0
    a[:, 5] = rng.randint(32, 192, n) / 64.0
    kind = np.arange(n) % 3
    b[:, 5] = rng.randint(8, 64, n) / 64.0
    b[:, 2] = np.where(kind == 0, np.where(rng.rand(n) < 0.5, a[:, 2] + a[:, 5], a[:, 2] - b[:, 5]),
                       np.where(kind == 1, a[:, 2] + rng.randint(0, 8, n) / 64.0,
                                a[:, 2] + a[:, 5] - rng.randint(1, 8, n) / 64.0))
    add("z_intervals", a, b, 0.5)

    # the same shapes far from the origin
    rng = np.random.RandomState(110)
    a1, b1 = thin(rng, n // 3)
    a2 = _rand_boxes(rng, n // 3)
    b2 = _shifted(rng, a2)
    a3 = _rand_boxes(rng, n // 3, 2.0, 4.0)
    b3 = a3.copy()
    b3[:, 3:5] *= np.sqrt(rng.uniform(0.03, 0.9, n // 3))[:, None]
    a, b = np.concatenate([a1, a2, a3]), np.concatenate([b1, b2, b3])
    off = rng.uniform(195, 205, (a.shape[0], 2)) * rng.choice([-1, 1], (a.shape[0], 2))
    a[:, 0:2] += off
    b[:, 0:2] += off
    add("far_200", a, b, 0.45)

    # generic overlapping pairs at every threshold
    for k, thr in enumerate(THRS):
        rng = np.random.RandomState(120 + k)
        a = _rand_boxes(rng, n)
        frac = {0.01: 1.1, 0.9: 0.05}.get(thr, 0.6)
        b = _shifted(rng, a, frac, 0.3 if thr < 0.9 else 0.02)
        if thr == 0.9:
            b[:, 3:5] = a[:, 3:5] * rng.uniform(0.97, 1.03, (n, 2))
        add("generic_thr_%g" % thr, a, b, thr)

    # one NaN / +Inf / -Inf field, in A or in B, on pairs that suppress when finite
    rng = np.random.RandomState(130)
    base = _f32(_rand_boxes(rng, 6))
    part = _f32(_shifted(rng, base.astype(np.float64), 0.1, 0.05))
    ra, rb = [], []
    for p in range(6):
        for side in (0, 1):
            for k in range(7):
                for val in (np.nan, np.inf, -np.inf):
                    x, y = base[p].copy(), part[p].copy()
                    (x if side == 0 else y)[k] = val
                    ra.append(x)
                    rb.append(y)
    add("non_finite", np.stack(ra), np.stack(rb), 0.3, clamp=(0.0, 0.0), finite=False)
    add("non_finite_clamped", np.stack(ra), np.stack(rb), 0.3, clamp=(0.2, 0.2), finite=False)
    return fam


def pair_decision_oracle(f):
    """the contract for every pair of a family: (suppressed bool [n], gate, oracle IoU)"""
    import oracle
    gate, iou = oracle.nms_pair(clamp_sizes(f["a"], f["clamp"]), clamp_sizes(f["b"], f["clamp"]))
    return ~(gate <= 0) & (iou >= float(np.float32(f["thr"]))), gate, iou


def pair_decision_f64(f):
    """the fp64 reference for every pair of a finite family: (suppressed bool [n], IoU [n])"""
    a, b = clamp_sizes(f["a"], f["clamp"]), clamp_sizes(f["b"], f["clamp"])
    r = [pair_iou_f64(a[i], b[i]) for i in range(a.shape[0])]
    iou, gate = np.array([x[0] for x in r]), np.array([x[1] for x in r])
    return ~(gate <= 0) & (iou >= float(np.float32(f["thr"]))), iou


_MEASURED = None


def measure():
    """-> dict(delta, families: name -> dict(n, thr, doubtful (bool [n]), suppress (bool [n], the oracle's), gate_exc (the
    pairs outside the band where the oracle and the fp64 reference differ and the fp32 gate is <= 0), disagree (those
    where they differ and it is not), max_diff))"""
    global _MEASURED
    if _MEASURED is not None:
        return _MEASURED
    fam, rec, worst = families(), {}, 0.0
    for name, f in fam.items():
        sup, gate, iou = pair_decision_oracle(f)
        r = dict(n=f["a"].shape[0], thr=f["thr"], suppress=sup, gate=gate, iou=iou, both=f["both"], finite=f["finite"])
        if f["finite"]:
            r["sup64"], r["iou64"] = pair_decision_f64(f)
            r["max_diff"] = float(np.abs(iou - r["iou64"]).max())
            worst = max(worst, r["max_diff"])
        rec[name] = r
    delta = 4.0 * worst
    for name, r in rec.items():
        if not r["finite"]:
            r["doubtful"] = np.zeros(r["n"], bool)
            continue
        r["doubtful"] = np.abs(r["iou64"] - float(np.float32(r["thr"]))) <= delta
        differ = (r["suppress"] != r["sup64"]) & ~r["doubtful"]
        r["gate_exc"] = np.nonzero(differ & (r["gate"] <= 0))[0]
        r["disagree"] = np.nonzero(differ & ~(r["gate"] <= 0))[0]
    _MEASURED = dict(delta=delta, families=rec, inputs=fam)
    return _MEASURED


def report():
    m = measure()
    lines = ["delta = %.3e" % m["delta"]]
    for name, r in m["families"].items():
        lines.append("%-22s n=%4d thr=%-5g doubtful=%5.2f%% suppress=%4d max_diff=%s gate_exc=%s disagree=%s" % (
            name, r["n"], r["thr"], 100.0 * r["doubtful"].mean(), int(r["suppress"].sum()),
            "%.2e" % r["max_diff"] if r["finite"] else "-", list(r.get("gate_exc", [])), list(r.get("disagree", []))))
    return "\n".join(lines)


if __name__ == "__main__":
    print(report())
