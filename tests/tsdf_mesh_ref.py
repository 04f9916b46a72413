"""numpy fp64 restatement of the semantics of d3d_tsdf_mesh_* (include/d3d_hip.h): marching tetrahedra on the
Kuhn split of every voxel cell of a TSDF volume, on arrays shaped like TsdfRef.blocks().  Element-wise operations in the
stated order only.  The case table is built here from the rules, and the swap that orients every triangle is derived at
import in exact integer arithmetic on the unit tetrahedra, not copied from the library or the header.  Also the scenes the
mesh tests share."""
import itertools

import numpy as np

KIND_DIR = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)], np.int64)
_KIND_OF = {tuple(e): k for k, e in enumerate(KIND_DIR.tolist())}
PERMS = list(itertools.permutations(range(3)))                      # lexicographic: xyz, xzy, yxz, yzx, zxy, zyx
SIGNS = [+1, -1, -1, +1, +1, -1]


def tet_corners(t):
    """the four cube corners [4, 3] of tetrahedron t: 0, e_p1, e_p1 + e_p2, (1, 1, 1)"""
    p = PERMS[t]
    c = np.zeros((4, 3), np.int64)
    c[1, p[0]] = 1
    c[2, p[0]] = c[2, p[1]] = 1
    c[3] = 1
    return c


def _unswapped(mask):
    """the triangles of a case before any swap: a list of triangles, each three (inside corner, outside corner)"""
    ins = [j for j in range(4) if (mask >> j) & 1]
    outs = [j for j in range(4) if not (mask >> j) & 1]
    if not ins or not outs:
        return []
    if len(ins) == 1:
        return [[(ins[0], o) for o in outs]]
    if len(outs) == 1:
        return [[(i, outs[0]) for i in ins]]
    (a, b), (c, d) = ins, outs
    q = [(a, c), (a, d), (b, d), (b, c)]
    return [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]


def _derive_table():
    """TABLE[t][mask]: the oriented triangles.  A triangle is swapped when, with every crossing at the middle of its edge,
    (v1 - v0) x (v2 - v0) does not point from the inside corners to the outside ones.  Exact: twice the mid-points are
    integer vectors.  Also checks that the decision depends on (sign, mask) alone."""
    table, swapped = [], {}
    for t in range(6):
        c = tet_corners(t)
        row = []
        for mask in range(16):
            tris = _unswapped(mask)
            ins = [j for j in range(4) if (mask >> j) & 1]
            outs = [j for j in range(4) if not (mask >> j) & 1]
            done = []
            for tri in tris:
                v = [c[i] + c[o] for i, o in tri]                                   # 2 x the mid-point
                n = np.cross(v[1] - v[0], v[2] - v[0])
                # from the inside corners' centroid to the outside corners', scaled to integers
                away = len(ins) * c[outs].sum(0) - len(outs) * c[ins].sum(0)
                dot = int((n * away).sum())
                assert dot != 0
                swap = dot < 0
                assert swapped.setdefault((SIGNS[t], mask), swap) == swap
                done.append([tri[0], tri[2], tri[1]] if swap else list(tri))
            row.append(done)
        table.append(row)
    return table, swapped


TABLE, SWAPPED = _derive_table()


def table_array():
    """TABLE as d3d_tsdf_mesh_table lays it out: int8 [6][16][13]"""
    out = np.full((6, 16, 13), -1, np.int8)
    for t in range(6):
        for mask in range(16):
            out[t, mask, 0] = len(TABLE[t][mask])
            for i, tri in enumerate(TABLE[t][mask]):
                for v, (a, b) in enumerate(tri):
                    out[t, mask, 1 + 2 * (3 * i + v)] = a
                    out[t, mask, 2 + 2 * (3 * i + v)] = b
    return out


def mesh_ref(blocks, voxel, origin, min_weight=1, color=True):
    """blocks = (coords [B, 3] ascending, D, W [B, 8, 8, 8], C [B, 8, 8, 8, 3] or None, CW or None) -> (vertices fp32 [V, 3],
    triangles int32 [T, 3], vertex_color fp32 [V, 3] or None, edges int32 [V, 4])"""
    coords, D, W, C, CW = blocks
    coords = np.asarray(coords, np.int64)
    voxel, origin = np.float64(voxel), np.asarray(origin, np.float64)
    B = len(coords)
    has_color = color and C is not None
    if B == 0:
        return (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32) if has_color else None,
                np.zeros((0, 4), np.int32))
    lo = coords.min(0)
    nb = coords.max(0) - lo + 1
    n = 8 * nb + 1                                                   # one layer of absent voxels beyond the last block
    Dd = np.zeros(n, np.float32)
    seen = np.zeros(n, bool)
    block_rank = np.full(n, -1, np.int64)                            # the rank of the voxel's block in coordinate order
    Cd, CWd = np.zeros(tuple(n) + (3,), np.float32), np.zeros(n, np.float32)
    for j, c in enumerate(coords - lo):
        s = tuple(slice(8 * c[i], 8 * c[i] + 8) for i in range(3))
        Dd[s] = D[j]
        with np.errstate(invalid="ignore"):
            seen[s] = W[j].astype(np.float64) >= min_weight          # a block coordinate past 65535 is never present
        seen[s] &= np.isfinite(D[j])                                 # a tsdf that is not finite: not seen
        block_rank[s] = j
        if has_color:
            Cd[s], CWd[s] = C[j], CW[j]
    inside = Dd < 0
    m = 8 * nb                                                       # voxels that can own something
    core = tuple(slice(0, m[i]) for i in range(3))

    def shifted(a, e):
        return a[tuple(slice(e[i], e[i] + m[i]) for i in range(3))]

    # ---- vertices ----
    vid = np.full(tuple(m) + (7,), -1, np.int64)
    rows = []
    for k, e in enumerate(KIND_DIR):
        cross = seen[core] & shifted(seen, e) & (inside[core] != shifted(inside, e)) & (block_rank[core] >= 0)
        gx, gy, gz = np.nonzero(cross)
        rows.append(np.stack([gx, gy, gz, np.full(len(gx), k)], 1))
    rows = np.concatenate(rows)
    g = rows[:, :3]
    key_block = block_rank[g[:, 0], g[:, 1], g[:, 2]]
    key_voxel = ((g[:, 0] % 8) * 8 + g[:, 1] % 8) * 8 + g[:, 2] % 8
    rows = rows[np.lexsort((rows[:, 3], key_voxel, key_block))]
    V = len(rows)
    g, k = rows[:, :3], rows[:, 3]
    vid[g[:, 0], g[:, 1], g[:, 2], k] = np.arange(V)
    e = KIND_DIR[k]
    h = g + e
    at_g, at_h = (g[:, 0], g[:, 1], g[:, 2]), (h[:, 0], h[:, 1], h[:, 2])
    dg, dh = Dd[at_g].astype(np.float64), Dd[at_h].astype(np.float64)
    with np.errstate(all="ignore"):
        s = dg / (dg - dh)
    g_world = g + 8 * lo
    vertices = np.zeros((V, 3), np.float32)
    for i in range(3):
        Xi = origin[i] + g_world[:, i].astype(np.float64) * voxel
        vertices[:, i] = np.where(e[:, i] == 1, Xi + s * voxel, Xi).astype(np.float32)
    vertex_color = None
    if has_color:
        vertex_color = np.zeros((V, 3), np.float32)
        cwg, cwh = CWd[at_g], CWd[at_h]
        for c in range(3):
            cg, ch = Cd[at_g + (c,)], Cd[at_h + (c,)]
            both = (cg.astype(np.float64) + s * (ch.astype(np.float64) - cg.astype(np.float64))).astype(np.float32)
            vertex_color[:, c] = np.where((cwg > 0) & (cwh > 0), both, np.where(cwg > 0, cg, np.where(cwh > 0, ch, np.float32(0))))
    edges = np.concatenate([g_world, k[:, None]], 1).astype(np.int32)

    # ---- triangles ----
    emitted = block_rank[core] >= 0
    for c in itertools.product((0, 1), repeat=3):
        emitted = emitted & shifted(seen, c)
    tris, keys = [], []
    for t in range(6):
        c = tet_corners(t)
        mask = sum(shifted(inside, c[j]).astype(np.int64) << j for j in range(4))
        for mk in range(1, 15):
            gx, gy, gz = np.nonzero(emitted & (mask == mk))
            if len(gx) == 0:
                continue
            cell = np.stack([gx, gy, gz], 1)
            for i, tri in enumerate(TABLE[t][mk]):
                idx = []
                for a, b in tri:
                    lo_c, hi_c = c[min(a, b)], c[max(a, b)]
                    owner = cell + lo_c
                    idx.append(vid[owner[:, 0], owner[:, 1], owner[:, 2], _KIND_OF[tuple((hi_c - lo_c).tolist())]])
                tris.append(np.stack(idx, 1))
                kv = ((gx % 8) * 8 + gy % 8) * 8 + gz % 8
                keys.append(np.stack([block_rank[gx, gy, gz], kv, np.full(len(gx), t), np.full(len(gx), i)], 1))
    if tris:
        tris, keys = np.concatenate(tris), np.concatenate(keys)
        tris = tris[np.lexsort((keys[:, 3], keys[:, 2], keys[:, 1], keys[:, 0]))]
        assert (tris >= 0).all()                                     # every vertex of an emitted cell exists
    else:
        tris = np.zeros((0, 3), np.int64)
    return vertices, tris.astype(np.int32), vertex_color, edges


# ---- what the tests measure ----
def directed_edges(triangles):
    """every directed edge (a, b) of the triangles, int64 [3 T, 2]"""
    t = np.asarray(triangles, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def edge_census(triangles):
    """-> (the largest number of times a directed edge occurs, the number of directed edges whose reverse is missing)"""
    d = directed_edges(triangles)
    if len(d) == 0:
        return 0, 0
    uniq, counts = np.unique(d, axis=0, return_counts=True)
    have = set(map(tuple, uniq.tolist()))
    return int(counts.max()), sum((b, a) not in have for a, b in have)


def euler_characteristic(triangles):
    """V - E + T over the vertices the triangles refer to"""
    t = np.asarray(triangles, np.int64)
    und = np.unique(np.sort(directed_edges(t), 1), axis=0)
    return len(np.unique(t)) - len(und) + len(t)


# ---- scenes ----
SPHERE = dict(r=4.2, c=(8.3, 8.6, 8.45), trunc=4.0)                  # in voxels


def sphere_blocks(voxel=1.0, origin=(0.0, 0.0, 0.0), base=(0, 0, 0), seed=0):
    """The eight blocks base + (0..1)^3 of D = clip((|x - c| - r) / trunc, -1, 1), the centre c given in voxels from the
    first block's corner; W = 1; a seeded colour with CW = 0 on a fifth of the voxels -> blocks (coords ascending)"""
    rs = np.random.RandomState(seed)
    coords = np.array([(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.int64)
    l = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1)
    D = np.zeros((8, 8, 8, 8), np.float32)
    for j, b in enumerate(coords):
        p = (8 * b + l).astype(np.float64)
        dist = np.sqrt(((p - np.array(SPHERE["c"])) ** 2).sum(-1))
        D[j] = np.clip((dist - SPHERE["r"]) / SPHERE["trunc"], -1.0, 1.0).astype(np.float32)
    W = np.ones((8, 8, 8, 8), np.float32)
    C = rs.rand(8, 8, 8, 8, 3).astype(np.float32)
    CW = (rs.rand(8, 8, 8, 8) > 0.2).astype(np.float32) * rs.randint(1, 4, (8, 8, 8, 8)).astype(np.float32)
    C[CW == 0] = 0
    return (coords + np.array(base, np.int64)).astype(np.int32), D, W, C, CW


def sphere_distance(vertices, voxel=1.0, origin=(0.0, 0.0, 0.0), base=(0, 0, 0)):
    """| |x - c| - r | in voxels for world positions [N, 3]"""
    p = (np.asarray(vertices, np.float64) - np.asarray(origin, np.float64)) / voxel - 8.0 * np.array(base, np.float64)
    return np.abs(np.sqrt(((p - np.array(SPHERE["c"])) ** 2).sum(-1)) - SPHERE["r"])
