"""Every launch form of the TSDF volume (csrc/tsdf.hip) and of its mesh (csrc/tsdf_mesh.hip) on the designed cases of
tests/tsdf_forms.py, against the restatements tests/tsdf_ref.py and tests/tsdf_mesh_ref.py.
tests/test_tsdf_forms_cpu.py asserts on the restatements alone that every case meets the design condition named below.

Comparisons: bit for bit, as in tests/test_tsdf_gpu.py and tests/test_tsdf_mesh_gpu.py: block coordinates, tsdf, weight,
colour and colour weight, the number of rows, positions, colours, voxels, the set of rows without a normal; V, T,
vertices, vertex colours, triangles and edges.  The normals keep the bound of tests/test_tsdf_gpu.py: 2^-23 per
component, each case printing how many components differ at all.  No other tolerance.  Two invariants that do not go
through a restatement are asserted on the device's own output (tests/tsdf_forms.py): every vertex lies on its edge,
exactly; every triangle's normal has a positive dot product with the step from the inside corners of its tetrahedron to
the outside ones (per tetrahedron, where it holds by construction; over the cell's eight corners it holds on smooth
volumes only and is asserted on signs and parity; tests/test_tsdf_forms_cpu.py has the counts).

  form                                      reached by
  k_tsdf_rows, second staging round         test_mesh_and_surface[random8, closed, nonfinite]: up to 748 rows in a block;
  (c0 = 512; local < 0 and local >= 512)    [checker]: 1536 rows, the third round ends on the boundary
  k_mesh_vertices, rounds 2 .. 4            [random8]: up to 1769 vertices in a block; [random1]: 1453 without any
                                            neighbour; [checker]: exactly 2048, the fourth round ends on the boundary;
                                            all four (has_g, has_h) colour cases occur past local index 512 in random8
  k_mesh_triangles / cell_triangles,        [random8, closed, nonfinite]: all 256 corner configurations among emitted
  the device's decoding of kTetWords        cells, so every (tetrahedron, mask) pair, path, pair, owner, dir_kind and the
                                            popcount index; [closed]: the device's triangles close (edge census (1, 0))
  k_tsdf_integrate, second round of         test_frames[512, 513, 513 colour]: F = 512 is one full round, F = 513 a second
  frames (f0 = 512; skip[] reused)          round of one frame; test_frames_split: 512 + 1 against its own restatement
  probe_next's turn in block_find,          test_parity: 200 keys share one position of a table of 1024 slots, so at
  block_touch and k_tsdf_insert             least 72 insertions (k_tsdf_insert) and 72 look-ups (block_find) turn in any
                                            order; the frame then needs block (14, 14, 12), a lattice point left out:
                                            its key finds all 128 slots of that position full and block_touch turns
  the write clamps of k_tsdf_rows,          test_guards: outputs 8 rows longer, prefilled; the true counts, and counts cut
  k_mesh_vertices, k_mesh_triangles         by 5 rows / 5 vertices / 7 triangles inside a later round of the last block
  sign and weight edges                     [signs]: -0.0, +0.0, +-2^-149, +-2^-126, +-1; [weights]: W in {0, 0.5, 1, 1.5,
                                            2, NaN, +inf, -1} at min_weight 0, 0.5, 1, 2
  kTouchRun edges of k_tsdf_touch           test_pixels[2048, 2049, 2049 step 2]: the last pixel alone needs its blocks
  a tsdf that is not finite                 [nonfinite], test_nonfinite_equals_unseen, test_integrate_keeps_nonfinite
  load_apron<true> / <false>, each of the   test_forward_neighbours[corner, corner_without_1 .. 7]: one voxel whose seven
  seven forward neighbours absent in turn   forward edges each end in another block; the twins leave one block out

Not reached: more than 212 blocks or 513 frames of 48 pixels (the old modules have the larger scenes); fp32 colour images
and uint16 depth in the second round of frames (test_tsdf_gpu.py has both in the first; the round changes nothing about
how a pixel is read); a volume that runs full while the walk turns (which keys fitted depends on scheduling, so there
is no exact result to compare; test_tsdf_gpu.py has the full volume); V or T past 2^31 - 1 (a vertex list of 24 GiB,
more than a test may take; the check is host code on two 64-bit sums); a stream other than the current one (the wrappers
pass torch's current stream only, and every launch of both files takes the one stream argument).

Fixes these tests asked for: one.  A voxel whose stored tsdf is NaN or +-inf (reachable through TsdfVolume.from_blocks
only) counted as seen and outside, and every crossing edge at it gave a NaN position.  Such a voxel is now not seen
(load_apron in tsdf_volume.inc, which both files use; both restatements say the same).

Mutants (each built apart, this module run once against it on an MI355X, not kept; all arithmetic or loop-bound
changes that cannot leave a buffer or lengthen a walk).  Every one of the nine fails at least one test:
  k_tsdf_rows' c0 loop stops after a round   8 fail: test_mesh_and_surface[random8, random1, checker, closed,
                                            nonfinite], test_guards, test_nonfinite_equals_unseen,
                                            test_integrate_keeps_nonfinite (weights has at most 458 rows in a block)
  k_mesh_vertices' c0 loop likewise          9 fail: test_mesh_and_surface[random8, random1, checker, closed, weights,
                                            nonfinite], test_parity (540 vertices in a block), test_guards,
                                            test_nonfinite_equals_unseen
  bits[owner] & ((1 << kind) |              9 fail: test_mesh_and_surface[all seven cases], test_parity, test_guards
  ((1 << kind) - 1))                        (every test that compares triangles)
  k_tsdf_integrate's f0 loop stops after    test_frames[513-False, 513-True] fail; [512-False] and test_frames_split
  the first 512 frames                      pass, as they must: neither has a second round
  skip[] not recomputed in the second       test_frames[513-False, 513-True] fail: frame 512 takes camera 0's decision
  round                                     and a block that camera 2 sees is skipped
  D <= 0 in voxel_edges and k_mesh_count    5 fail: test_mesh_and_surface[signs], test_pixels[2048-1, 2049-1, 2049-2]
                                            and test_integrate_keeps_nonfinite (dyadic depths put voxels at D = 0)
  block_find gives up after cap / 8 probes  test_parity fails (a mesh that misses neighbours), nothing else: no other
                                            table fills a position
  block_touch gives up after cap / 8        test_parity fails (integrate reports a full volume: block (14, 14, 12) cannot
  probes (not asked for by the issue)       be inserted without the turn), nothing else
  the fix of non-finite tsdf taken out      test_mesh_and_surface[nonfinite], test_nonfinite_equals_unseen and
                                            test_integrate_keeps_nonfinite fail

Cost: the module's 18 tests take 4.8 s on an MI355X, restatements included; the slowest is
test_mesh_and_surface[random8] at 0.8 s, which also builds the restatements the later tests share.  The eight cases of
test_forward_neighbours came later and are of random8's size, one pass each."""
import ctypes

import numpy as np
import pytest
import torch

from tests import tsdf_forms as F
from tests.tsdf_mesh_ref import edge_census, euler_characteristic

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAD = 8
SENT_I = -7


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _volume(dev, name, seed, **kw):
    """TsdfVolume.from_blocks of a case, its blocks handed over in a seeded permutation"""
    from detection_3d_amd.tsdf import TsdfVolume
    c = F.case(name)
    order = np.random.RandomState(seed).permutation(len(c["blocks"][0]))
    put = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a[order])).to(dev)
    kw.setdefault("max_blocks", c.get("max_blocks", 64))
    return TsdfVolume.from_blocks(*[put(a) for a in c["blocks"]], voxel=c["voxel"], origin=c["origin"], **kw)


def _frames(dev, depth, intr, extr, color=None, first=0, last=None):
    from detection_3d_amd.unproject import DepthFrames
    s = slice(first, last)
    return DepthFrames(torch.from_numpy(depth[s]).to(dev), intr[s], extr[s],
                       color=None if color is None else torch.from_numpy(color[s]).to(dev))


def _same_blocks(vol, ref, what):
    coords, tsdf, weight, color, cweight = vol.blocks()
    r_coords, r_tsdf, r_weight, r_color, r_cweight = ref.blocks() if hasattr(ref, "blocks") else ref
    assert coords.dtype == torch.int32 and tsdf.dtype == torch.float32
    assert vol.n_blocks == len(r_coords), what
    assert np.array_equal(coords.cpu().numpy(), r_coords), what
    assert np.array_equal(_bits(weight.cpu().numpy()), _bits(r_weight)), what
    assert np.array_equal(_bits(tsdf.cpu().numpy()), _bits(r_tsdf)), what
    if vol.color:
        assert np.array_equal(_bits(cweight.cpu().numpy()), _bits(r_cweight)), what
        assert np.array_equal(_bits(color.cpu().numpy()), _bits(r_color)), what
    else:
        assert color is None and cweight is None


def _same_surface(vol, want, what, min_weight=1):
    """vol.surface_points at 3, 6 and 9 columns against want(columns) = TsdfRef.surface_points(columns, min_weight)
    -> (rows [N, 9], voxels) as numpy"""
    for c in (3, 6, 9):
        rows, voxels = vol.surface_points(c, min_weight, return_voxels=True)
        assert rows.dtype == torch.float32 and voxels.dtype == torch.int32
        rows, voxels = rows.cpu().numpy(), voxels.cpu().numpy()
        r_rows, r_voxels, r_has = want(c)
        assert rows.shape == r_rows.shape, (what, c)
        assert np.array_equal(voxels, r_voxels), (what, c)
        k = min(c, 6)
        assert np.array_equal(_bits(rows[:, :k]), _bits(r_rows[:, :k])), (what, c)
        assert np.isfinite(rows).all(), (what, c)
        if c == 9:
            zero = (rows[:, 6:9] == 0).all(1)
            assert np.array_equal(zero, ~r_has), what
            err = np.abs(rows[:, 6:9].astype(np.float64) - r_rows[:, 6:9].astype(np.float64))
            print(f"{what}: {vol.n_blocks} blocks, {rows.shape[0]} rows, {int(zero.sum())} without a normal; "
                  f"{int((err > 0).sum())} of {err.size} normal components differ, largest "
                  f"{err.max() if err.size else 0.0:.3e} (bound {2.0 ** -23:.3e})")
            assert (err <= 2.0 ** -23).all(), what
    return rows, voxels


def _same_mesh(vol, want, what, **mesh_kw):
    """vol.mesh(return_edges=True, **mesh_kw) and plain vol.mesh(**mesh_kw) against want = mesh_ref(...)
    -> (vertices, triangles, colours or None, edges) as numpy"""
    r_vertices, r_triangles, r_color, r_edges = want
    mesh, edges = vol.mesh(return_edges=True, **mesh_kw)
    assert mesh.vertices.dtype == torch.float32 and mesh.triangles.dtype == torch.int32 and edges.dtype == torch.int32
    vertices, triangles, edges = mesh.vertices.cpu().numpy(), mesh.triangles.cpu().numpy(), edges.cpu().numpy()
    print(f"{what}: {vol.n_blocks} blocks, {len(vertices)} vertices, {len(triangles)} triangles")
    assert vertices.shape == r_vertices.shape and triangles.shape == r_triangles.shape, what
    assert np.array_equal(edges, r_edges), what
    assert np.array_equal(_bits(vertices), _bits(r_vertices)), what
    assert np.array_equal(triangles, r_triangles), what
    color = None
    if r_color is None:
        assert mesh.vertex_color is None, what
    else:
        assert mesh.vertex_color.dtype == torch.float32
        color = mesh.vertex_color.cpu().numpy()
        assert np.array_equal(_bits(color), _bits(r_color)), what
    plain = vol.mesh(**mesh_kw)
    assert torch.equal(plain.vertices.view(torch.int32), mesh.vertices.view(torch.int32))
    assert torch.equal(plain.triangles, mesh.triangles)
    assert plain.vertex_color is None or torch.equal(plain.vertex_color.view(torch.int32), mesh.vertex_color.view(torch.int32))
    return vertices, triangles, color, edges


def _check_case(dev, name, seed):
    """mesh and surface of a case at each of its min_weights against the restatements, the kinds 0..2 identity and the two
    invariants on the device's own output -> everything the device returned, as numpy"""
    c = F.case(name)
    vol = _volume(dev, name, seed)
    assert vol.n_blocks == len(c["blocks"][0]) and vol.color == (c["blocks"][3] is not None)
    _same_blocks(vol, c["blocks"][:3] + tuple(np.zeros(0) if a is None else a for a in c["blocks"][3:]), name)
    outs = []
    for mw in c["min_weights"]:
        what = (name, "min_weight", mw)
        vertices, triangles, color, edges = _same_mesh(vol, F.case_mesh(name, mw), what, min_weight=mw)
        rows, voxels = _same_surface(vol, lambda k: F.case_surface(name, k, mw), what, mw)
        axis = edges[:, 3] < 3                                          # kinds 0..2 are the surface rows
        assert int(axis.sum()) == len(rows) and np.array_equal(edges[axis][:, :3], voxels), what
        assert np.array_equal(_bits(vertices[axis]), _bits(rows[:, :3])), what
        if color is not None:
            assert np.array_equal(_bits(color[axis]), _bits(rows[:, 3:6])), what
        F.vertices_on_their_edges(vertices, edges, c["voxel"], c["origin"])
        F.triangles_face_outwards(vertices, triangles, edges, c["blocks"], c["voxel"], c["origin"], "tet")
        if name in ("signs", "parity"):
            F.triangles_face_outwards(vertices, triangles, edges, c["blocks"], c["voxel"], c["origin"], "cell")
        outs += [vertices, triangles, edges, rows, voxels] + ([] if color is None else [color])
    return vol, outs


@pytest.mark.parametrize("name", ["random8", "random1", "checker", "closed", "weights", "signs", "nonfinite"])
def test_mesh_and_surface(dev, name):
    _, first = _check_case(dev, name, 11)
    if name == "closed":
        triangles = first[1]
        assert edge_census(triangles) == (1, 0) and euler_characteristic(triangles) % 2 == 0
    _, again = _check_case(dev, name, 12)                               # other block ids, the same bits
    assert len(first) == len(again)
    for a, b in zip(first, again):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", F.CORNER_CASES)
def test_forward_neighbours(dev, name):
    """eight blocks with a sign change exactly across a block face, a block edge and the shared corner, and the seven
    twins with one forward neighbour of the first block left out: the one apron routine with and without diagonals"""
    _check_case(dev, name, 17)


def test_parity(dev):
    """a table whose keys all share one position inside a group: insertion, look-up and the touch pass take the turn"""
    c = F.case("parity")
    vol, _ = _check_case(dev, "parity", 13)
    assert vol._slots == 1024 and vol.max_blocks == F.PARITY_MAX_BLOCKS
    ref = F.carried_on("parity")
    vol.integrate(_frames(dev, *F.parity_frame()))
    assert vol.n_blocks == len(ref.coords) > len(c["blocks"][0]) and not vol.clipped
    _same_blocks(vol, ref, "parity, then a frame")
    _same_surface(vol, lambda k: F.surface_of("parity carried on", ref, k), "parity, then a frame")


@pytest.mark.parametrize("F_,color", [(512, False), (513, False), (513, True)])
def test_frames(dev, F_, color):
    """512 frames fill one round of k_tsdf_integrate, the 513th opens a second"""
    from detection_3d_amd.tsdf import TsdfVolume
    ref = F.frames_ref(F_, color)
    vol = TsdfVolume(max_blocks=1024, color=color, **F.FRAMES_VOLUME)
    vol.integrate(_frames(dev, *F.frames513(F_, color)))
    what = ("frames", F_, color)
    _same_blocks(vol, ref, what)
    assert vol.clipped == ref.clipped
    _same_surface(vol, lambda k: F.surface_of(what, ref, k), what)


def test_frames_split(dev):
    """F = 513 as 512 + 1: each side equals its own restatement (one call and two may differ in the last bit)"""
    from detection_3d_amd.tsdf import TsdfVolume
    calls = ((0, 512), (512, 513))
    ref = F.frames_ref(513, False, calls)
    vol = TsdfVolume(max_blocks=1024, color=False, **F.FRAMES_VOLUME)
    for a, b in calls:
        vol.integrate(_frames(dev, *F.frames513(513), first=a, last=b))
    _same_blocks(vol, ref, "512 + 1")
    _same_surface(vol, lambda k: F.surface_of("512 + 1", ref, k), "512 + 1")
    one = F.frames_ref(513)
    assert np.array_equal(one.blocks()[0], ref.blocks()[0]) and np.array_equal(one.blocks()[2], ref.blocks()[2])


@pytest.mark.parametrize("width,step", [(2048, 1), (2049, 1), (2049, 2)])
def test_pixels(dev, width, step):
    """one workgroup of the touch pass holds 2048 pixels: a full one, and a second of one pixel"""
    from detection_3d_amd.tsdf import TsdfVolume
    ref = F.pixels_ref(width, step)
    vol = TsdfVolume(max_blocks=1024, color=False, **F.PIXELS_VOLUME)
    vol.integrate(_frames(dev, *F.pixels(width)), step=step)
    what = ("pixels", width, step)
    _same_blocks(vol, ref, what)
    _same_surface(vol, lambda k: F.surface_of(what, ref, k), what)


def test_guards(dev):
    """the C entries on random8 with outputs 8 rows too long: nothing past N, V, T is written, nor past smaller counts"""
    from detection_3d_amd._lib import check, lib, ptr, stream_of
    vol = _volume(dev, "random8", 14)
    n, order, L = vol.n_blocks, vol._sorted(), lib()
    r_vertices, r_triangles, r_color, r_edges = F.case_mesh("random8")
    V, T = len(r_vertices), len(r_triangles)
    full = lambda rows, cols, value, dtype: torch.full((rows + PAD, cols), value, dtype=dtype, device=dev)
    nan_rows = lambda t, a: bool(torch.isnan(t[a:]).all())
    with torch.cuda.device(dev):
        s = stream_of(dev)
        desc = vol._desc(order=order)
        # the surface rows
        nbytes = L.d3d_tsdf_surface_scratch_bytes(n)
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        info = (ctypes.c_int * 1)(0)
        check(L.d3d_tsdf_surface_count(desc, 1.0, ptr(buf), nbytes, info, s))
        for columns in (3, 6, 9):
            r_rows, r_voxels, _ = F.case_surface("random8", columns)
            N = len(r_rows)
            assert info[0] == N
            for cut in (0, 5):
                out, voxels = full(N, columns, NAN, torch.float32), full(N, 3, SENT_I, torch.int32)
                given = (ctypes.c_int * 1)(N - cut)
                check(L.d3d_tsdf_surface_rows(desc, 1.0, columns, given, ptr(buf), nbytes, ptr(out), ptr(voxels), s))
                torch.cuda.synchronize()
                k, m = min(columns, 6), N - cut
                assert np.array_equal(_bits(out[:m, :k].cpu().numpy()), _bits(r_rows[:m, :k])), (columns, cut)
                assert np.array_equal(voxels[:m].cpu().numpy(), r_voxels[:m]), (columns, cut)
                assert nan_rows(out, m) and bool((voxels[m:] == SENT_I).all()), (columns, cut)
        # the mesh
        nbytes = L.d3d_tsdf_mesh_scratch_bytes(n)
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        info = (ctypes.c_int * 2)(0, 0)
        check(L.d3d_tsdf_mesh_count(desc, 1.0, ptr(buf), nbytes, info, s))
        assert (info[0], info[1]) == (V, T)
        for cut_v, cut_t in ((0, 0), (5, 7)):
            vertices, colors = full(V, 3, NAN, torch.float32), full(V, 3, NAN, torch.float32)
            edges, triangles = full(V, 4, SENT_I, torch.int32), full(T, 3, SENT_I, torch.int32)
            given = (ctypes.c_int * 2)(V - cut_v, T - cut_t)
            check(L.d3d_tsdf_mesh_vertices(desc, given, ptr(buf), nbytes, ptr(vertices), ptr(colors), ptr(edges), s))
            check(L.d3d_tsdf_mesh_triangles(desc, given, ptr(buf), nbytes, ptr(triangles), s))
            torch.cuda.synchronize()
            v, t = V - cut_v, T - cut_t
            assert np.array_equal(_bits(vertices[:v].cpu().numpy()), _bits(r_vertices[:v])), cut_v
            assert np.array_equal(_bits(colors[:v].cpu().numpy()), _bits(r_color[:v])), cut_v
            assert np.array_equal(edges[:v].cpu().numpy(), r_edges[:v]), cut_v
            assert np.array_equal(triangles[:t].cpu().numpy(), r_triangles[:t]), cut_t
            assert nan_rows(vertices, v) and nan_rows(colors, v) and bool((edges[v:] == SENT_I).all()), cut_v
            assert bool((triangles[t:] == SENT_I).all()), cut_t


def test_nonfinite_equals_unseen(dev):
    """a voxel whose tsdf is NaN or +-inf gives what the same voxel with W = 0 gives, and every output is finite"""
    bad, twin = _volume(dev, "nonfinite", 15), _volume(dev, "nonfinite_twin", 16)
    a, ea = bad.mesh(return_edges=True)
    b, eb = twin.mesh(return_edges=True)
    outs = [(a.vertices, b.vertices), (a.triangles, b.triangles), (a.vertex_color, b.vertex_color), (ea, eb)]
    for columns in (3, 6, 9):
        outs += list(zip(bad.surface_points(columns, return_voxels=True), twin.surface_points(columns, return_voxels=True)))
    for x, y in outs:
        assert x.shape == y.shape and x.shape[0] > 5000 and torch.equal(x.view(torch.int32), y.view(torch.int32))
        assert bool(torch.isfinite(x).all())
    assert a.vertices.shape[0] == len(F.case_mesh("nonfinite")[0]) < len(F.case_mesh("random8")[0])


def test_integrate_keeps_nonfinite(dev):
    """(w NaN + S) / wn: fusion does not repair such a voxel; everything else is the restatement's, bit for bit"""
    ref = F.carried_on("nonfinite")
    vol = _volume(dev, "nonfinite", 17, max_blocks=256)
    vol.integrate(_frames(dev, *F.nonfinite_frame()))
    coords, tsdf, weight, color, cweight = [t.cpu().numpy() for t in vol.blocks()]
    r_coords, r_tsdf, r_weight, r_color, r_cweight = ref.blocks()
    assert np.array_equal(coords, r_coords) and len(coords) > 8
    for got, want in ((weight, r_weight), (color, r_color), (cweight, r_cweight)):
        assert np.array_equal(_bits(got), _bits(want))
    finite = np.isfinite(r_tsdf)
    assert (~finite).sum() == 60 and np.array_equal(np.isfinite(tsdf), finite)
    assert np.array_equal(_bits(tsdf[finite]), _bits(r_tsdf[finite]))
    assert np.array_equal(tsdf[~finite], r_tsdf[~finite], equal_nan=True)     # NaN stays NaN, +-inf keeps its sign
    seen_again = weight[~finite] > 1
    assert seen_again.sum() >= 3
    _same_surface(vol, lambda k: F.surface_of("nonfinite carried on", ref, k), "nonfinite, then a frame")
