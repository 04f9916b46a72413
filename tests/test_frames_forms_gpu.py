"""Every launch form of the mesh renderer (csrc/render.hip) and of the frame unprojection (csrc/unproject.hip) on the
designed cases of tests/frames_forms.py, against the restatements tests/render_ref.py and tests/unproject_ref.py, used as
they are.  tests/test_frames_forms_cpu.py asserts on the restatements alone that every case meets the design condition
named below.

Comparisons: bit for bit, as in tests/test_render_gpu.py and tests/test_unproject_gpu.py.  Render: tri, depth bits,
colour bits, at every pixel.  Unproject: N, pixel_of_point, position bits, colour bits, the set of rows without a normal;
the normal components keep test_unproject_gpu.py's derived bound of 2^-23, each case printing how many differ at all (on
the run recorded below: none, in any case).  No pixel and no row is excused and there is no other tolerance.  The list
length E of every frame, which no image shows, equals the sum of the rectangle areas of frames_forms.tile_rects (fp64,
render.hip's order of operations and its 1e9 px rule).

  form                                      reached by
  k_rd_tiles, rounds 2 and 3                test_r1_rounds[257, 512, 513, 768]: one tile whose list is the mesh, T = 257
  (base += kBatch, m = min(kBatch, n -     is a second round of one entry, 512 two full rounds, 513 a third of one; [255,
  base), sh[][] overwritten)                256]: one round, short and full.  Three interleaved depth layers and the windows
                                            min_depth 0, 3, 6 make 256 other triangles win each time, 768 in all, spread
                                            over the index range (the order inside a list is arbitrary, so no test can
                                            say which round holds a winner); test_r7_guards: a tile of 507 entries
  the depth range in k_rd_tiles             test_r1_rounds: min_depth 3 and 6 (a nearer hit below the range hides nothing);
                                            max_depth 3, 2.125 and (3, 4.125): the last two end inside a layer, whose
                                            farther triangles would show without the upper bound
  uint16 quantisation                       test_r2_uint16_edges: z / depth_scale = 0.5, 1.5, 2.5, 3.5 (ties to even, 0.5
                                            gives 0 with tri >= 0), 65535 (kept), 65535.5 (0); the same walls as fp32
  colour                                    test_r3_colour: fp32 NaN, +inf, -0.0, a denormal, values above 255; uint8 0 and
                                            255 at all corners; colours without return_triangles, triangles without colours
  tile_rect: none, box, whole frame         test_r4_tile_rect_paths, test_r5_thin_frames, test_r6_entry_counts: vertices
                                            on pixel centres 15, 16, 31 | 32, the last and the first pixel; off the image
                                            by more than a pixel on each side (none) and by half a pixel (box); the 1e9 px
                                            escape, crossing z = 0 (whole); behind, NaN vertex, bad indices (none);
                                            zero area (box, no hit); 37 x 53, 1 x 300 and 300 x 1: partial last tiles
  cameras that are not usable               test_r4_tile_rect_paths: fx = -16 (the mirror image), +inf (every column shows
                                            the principal one), 0, NaN, cx = NaN, a NaN translation (whole-frame lists, no
                                            hit): include/d3d_hip.h defines these by its arithmetic as it stands
  k_rd_bin<false>, the entry count          test_r6_entry_counts: E per frame of all cases above and of exact_scene at
                                            both SHAPES of test_render_gpu.py (481 and 1834 in all)
  k_rd_bin<true>, slot < n_entries;         test_r7_guards: lists 8 entries longer and prefilled; every tile's list is the
  k_rd_tiles, begin + n > n_entries         restatement's set; with E - 5 nothing from E - 5 on is written, three tiles
                                            equal the full render and the tile whose list is cut is zeros with tri == -1
  k_up_count, k_up_rows<3 | 6 | 9>,         test_u1_full_steps_and_run_edges: 2047, 2048, 2049, 4096, 4097 dense pixels:
  full steps and run edges                  local = 255 and full ballots in all four waves, a last run of one pixel
  a step with total == 0, wave_cnt[it & 1]  test_u2_empty_steps_and_runs, test_u5: run 0 dense, empty, dense, empty, lane
  an empty run                              63 of wave 3, dense, empty, lane 0 of wave 0; run 1 empty; run 2 its first and
                                            last pixel
  step                                      test_u3_lattice: 2, 3, 16, 100 (one pixel per frame); raw neighbours
  neighbour() at frame seams                test_u4_frame_seams: 9 frames of 5 rows, the pixel at p -/+ W of every seam
                                            row valid and within edge = 1; also U1's 2 x 32 x 64
  fp32 colour, no colour                    test_u5_fp32_colour_and_no_colour: NaN, -0.0, +-inf, denormals copied
  the n_rows clamps of k_up_rows            test_u6_guards: out and pixel_of_point 8 rows longer; N and N - 5, a cut
                                            inside the last step of the last run, at 3, 6 and 9 columns

Not reached: more than 2048 tiles or runs in a call (the second tile of scan_exclusive_i32, which the plan, downsample
and front modules reach on the same code); E or a pixel count past 2^31 (host checks, covered by
tests/test_scan_descriptors_cpu.py); a stream other than the current one; the Python chunking, which
tests/test_render_gpu.py::test_chunking covers.

Fixes these tests asked for: none.  Kernel and restatement agree on every case, the seven cameras of R4 included.

Mutants (each built apart, this module run once against it on an MI355X, not kept; arithmetic or loop-bound changes
only, none can leave a buffer or lengthen a loop):
  k_rd_tiles stops after its first round    5 fail: test_r1_rounds[257, 512, 513, 768], test_r7_guards
  m = kBatch, the extra entries masked to   none fails, as it must: equivalent (a masked entry is a NaN that no
  "no hit"                                  comparison accepts)
  z >= O.zmin dropped                       6 fail: test_r1_rounds[all six]
  z <= O.zmax dropped                       3 fail: test_r1_rounds[512, 513, 768] (the windows that end inside a layer;
                                            max_depth = 3 alone would not have caught it: it ends between two layers)
  rint -> floor(x + 0.5), uint16 path       2 fail: test_r2_uint16_edges[0.125, 0.625] (0.5 -> 1, 2.5 -> 3)
  q >= 1.0 -> q >= 0.0                      none fails: equivalent.  q is rint's result, an integer; the only one in
                                            [0, 1) is 0, and (uint16_t)0 is the 0 the other branch writes
  tile_rect always the whole frame          2 fail: test_r6_entry_counts and test_r7_guards' E; every image stays right
  tile_rect without the one-pixel growth    2 fail: the same two, on E (r4's seams; r7: 768 for 972).  No image changes:
                                            the growth covers rounding below 1e-6 px, which an exact case cannot reach
  the 1e9 px test dropped                   1 fails: test_r6_entry_counts (r4's escape triangle takes a box); no image
                                            changes, since the box of an fp64 projection is still conservative there
  k_up_rows uses wave_cnt[0] in every step  none fails, and it is not equivalent: the second set matters only after a
                                            step with total == 0, whose `continue` skips the barrier, and only if a wave
                                            then loads its next depth from memory before another has read four LDS words.
                                            U2 and U5 hold that sequence (empty, then dense; empty, then one lane) three
                                            times per call; the window did not open.  A deterministic case cannot open it
  k_up_rows does not skip total == 0        none fails: equivalent (zero rows are staged and copied)
  neighbour(): the vv bound replaced by     7 fail: test_u1[2 x 32 x 64, both depth types], test_u3_lattice[2, 3, 16],
  a bound on p alone                        test_u4_frame_seams, test_u6_guards
  step applied to u only                    4 fail: test_u3_lattice[2, 3, 16, 100]

Cost: the module's 39 tests take 3.0 s on an MI355X, restatements included; the slowest is test_r1_rounds[255] at
0.2 s (and as much of set-up: the first call into the library)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import frames_forms as F

pytestmark = pytest.mark.gpu
INF = math.inf
NAN = float("nan")
PAD = 8
SENT_I = -7


def _np(t):
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


# ---- render ----
def _mesh(dev, c, color=True):
    from detection_3d_amd.render import TriangleMesh
    col = c.get("color") if color else None
    return TriangleMesh(torch.from_numpy(c["vertices"]).to(dev), torch.from_numpy(c["triangles"]).to(dev),
                        None if col is None else torch.from_numpy(col).to(dev))


def _same_render(dev, c, key, what, uint16_depth=False, **kw):
    """render_depth of a case against render_ref of it: the triangle, the depth bits and the colour bits of every pixel
    -> (depth, tri, color) of the device as numpy"""
    from detection_3d_amd.render import render_depth
    ref_kw = dict(kw, depth_dtype=np.uint16) if uint16_depth else kw
    r_depth, r_tri, r_color, _ = F.render_case_ref(c, key, **ref_kw)
    frames, tri = render_depth(_mesh(dev, c), c["intr"], c["extr"], c["H"], c["W"], return_triangles=True,
                               depth_dtype=torch.uint16 if uint16_depth else torch.float32, **kw)
    depth, tri = _np(frames.depth), _np(tri)
    color = None if frames.color is None else _np(frames.color)
    assert depth.dtype == r_depth.dtype and depth.shape == r_depth.shape == tri.shape and tri.dtype == np.int32, what
    wrong = [int((tri != r_tri).sum()), int((_bits(depth) != _bits(r_depth)).sum())]
    if r_color is None:
        assert color is None, what
    else:
        assert color.dtype == r_color.dtype and color.shape == r_color.shape, what
        wrong.append(int((_bits(color) != _bits(r_color)).sum()))
    print(f"{what}: {int((r_tri >= 0).sum())} of {r_tri.size} pixels hit; differ: {wrong} (triangles, depths, colour "
          f"components)")
    assert np.array_equal(tri, r_tri), what
    assert np.array_equal(_bits(depth), _bits(r_depth)), what
    assert r_color is None or np.array_equal(_bits(color), _bits(r_color)), what
    return depth, tri, color


@pytest.mark.parametrize("T", F.R1_SIZES)
def test_r1_rounds(dev, T):
    """a list of T triangles in one tile, one to three rounds of k_rd_tiles, through every depth window"""
    c = F.r1(T)
    for lo, hi in F.R1_WINDOWS:
        _same_render(dev, c, ("r1", T), ("r1", T, lo, hi), min_depth=lo, max_depth=hi)


@pytest.mark.parametrize("d", F.R2_DEPTHS)
def test_r2_uint16_edges(dev, d):
    c = F.r2(d)
    depth, tri, _ = _same_render(dev, c, ("r2", d), ("r2", d, "uint16"), uint16_depth=True, depth_scale=F.R2_SCALE)
    assert (depth == F.R2_QUANTA[F.R2_DEPTHS.index(d)]).all() and (tri >= 0).all()
    depth, _, _ = _same_render(dev, c, ("r2", d), ("r2", d, "fp32"))
    assert (depth == np.float32(d)).all()


@pytest.mark.parametrize("uint8_color", [False, True])
def test_r3_colour(dev, uint8_color):
    from detection_3d_amd.render import render_depth
    c = F.r3(uint8_color)
    depth, tri, color = _same_render(dev, c, ("r3", uint8_color), ("r3", "uint8" if uint8_color else "fp32"))
    # with colours and without return_triangles; without colours and with it
    frames = render_depth(_mesh(dev, c), c["intr"], c["extr"], c["H"], c["W"])
    assert np.array_equal(_bits(_np(frames.depth)), _bits(depth)) and np.array_equal(_bits(_np(frames.color)), _bits(color))
    frames, tri2 = render_depth(_mesh(dev, c, color=False), c["intr"], c["extr"], c["H"], c["W"], return_triangles=True)
    assert frames.color is None and np.array_equal(_np(tri2), tri) and np.array_equal(_bits(_np(frames.depth)), _bits(depth))


@pytest.mark.parametrize("uint16_depth", [False, True])
def test_r4_tile_rect_paths(dev, uint16_depth):
    """every branch of tile_rect, seams and the partial last tiles, through seven cameras of which five are not usable"""
    _, tri, _ = _same_render(dev, F.r4(), "r4", ("r4", uint16_depth), uint16_depth=uint16_depth)
    assert (tri[:3] >= 0).all() and (tri[3:] == -1).all()


@pytest.mark.parametrize("shape", F.R5_SHAPES)
def test_r5_thin_frames(dev, shape):
    _same_render(dev, F.r5(shape), ("r5", shape), ("r5", shape))


def test_r6_entry_counts(dev):
    """E of every frame of every case, and of the exact scenes of tests/test_render_gpu.py, is the sum of the rectangle
    areas of the tile_rect restatement: no rectangle is larger than it has to be, none smaller"""
    from detection_3d_amd._lib import lib
    from detection_3d_amd.render import frame_scratch_bytes
    cases = F.render_cases() + [(f"exact_scene{s}", F.exact_case(s)) for s in F.EXACT_SHAPES]
    for name, c in cases:
        need = frame_scratch_bytes(_mesh(dev, c, color=False), c["intr"], c["extr"], c["H"], c["W"])
        fixed = lib().d3d_render_scratch_bytes(1, c["H"], c["W"])
        E = [(n - fixed) // 4 for n in need]
        assert all((n - fixed) % 4 == 0 for n in need)
        print(f"{name}: E per frame {E}")
        assert E == F.entries(c).tolist(), name


def _frames_desc(depth, intr, extr, H, W):
    from detection_3d_amd._lib import DepthFramesDesc, ptr
    return DepthFramesDesc(ptr(depth), 0, None, 0, ptr(intr), ptr(extr), 1, H, W, 0.001)


def test_r7_guards(dev):
    """the C entries on the R1 mesh over four tiles, `lists` 8 entries too long: nothing past E is written, nor past E - 5,
    and a tile whose list is cut is rendered empty"""
    from detection_3d_amd._lib import check, lib, ptr, stream_of
    c = F.r7()
    H, W = c["H"], c["W"]
    branch, rect = F.case_rects(c)
    counts = F.case_counts(c)[0].ravel()
    ends = np.cumsum(counts)
    r_depth, r_tri, _, _ = F.render_case_ref(c, "r7")
    mesh, L = _mesh(dev, c), lib()
    intr, extr = (torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in ("intr", "extr"))
    with torch.cuda.device(dev):
        s = stream_of(dev)
        nbytes = L.d3d_render_scratch_bytes(1, H, W)
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        info = (ctypes.c_int64 * 1)(0)
        for cut in (0, 5):
            depth = torch.full((1, H, W), NAN, dtype=torch.float32, device=dev)
            tri = torch.full((1, H, W), SENT_I, dtype=torch.int32, device=dev)
            frames = _frames_desc(depth, intr, extr, H, W)
            check(L.d3d_render_bin(mesh.desc, frames, ptr(buf), nbytes, info, s))
            E = int(info[0])
            assert E == ends[-1]
            lists = torch.full((E + PAD,), SENT_I, dtype=torch.int32, device=dev)
            given = (ctypes.c_int64 * 1)(E - cut)
            check(L.d3d_render_fill(mesh.desc, frames, given, ptr(buf), nbytes, ptr(lists), s))
            check(L.d3d_render_tiles(mesh.desc, frames, 0.0, INF, given, ptr(buf), nbytes, ptr(lists), ptr(tri), s))
            torch.cuda.synchronize()
            got, depth, tri = lists.cpu().numpy(), depth.cpu().numpy(), tri.cpu().numpy()
            assert (got[E - cut:] == SENT_I).all(), cut
            for t, (n, end) in enumerate(zip(counts, ends)):
                y, x = divmod(t, 2)
                members = np.flatnonzero((branch[0] != F.NONE) & (rect[0, :, 0] <= x) & (x <= rect[0, :, 1])
                                         & (rect[0, :, 2] <= y) & (y <= rect[0, :, 3]))
                assert len(members) == n
                window = (0, slice(16 * y, 16 * y + 16), slice(16 * x, 16 * x + 16))
                if end <= E - cut:
                    assert np.array_equal(np.sort(got[end - n:end]), members), (cut, t)      # the list, in some order
                    assert np.array_equal(tri[window], r_tri[window]), (cut, t)
                    assert np.array_equal(_bits(depth[window]), _bits(r_depth[window])), (cut, t)
                else:
                    written = got[end - n:E - cut]
                    assert np.isin(written, members).all() and len(np.unique(written)) == len(written), (cut, t)
                    assert (tri[window] == -1).all() and not _bits(depth[window]).any(), (cut, t)
            assert cut == 0 or ends[-2] < E - cut < ends[-1]


# ---- unproject ----
def _frames(dev, c, **kw):
    from detection_3d_amd.unproject import DepthFrames
    return DepthFrames(torch.from_numpy(c["depth"]).to(dev), c["intr"], c["extr"],
                       color=None if c["color"] is None else torch.from_numpy(c["color"]).to(dev), **kw)


def _same_normals(rows, r_rows, r_has, what):
    zero = (rows[:, 6:9] == 0).all(1)
    assert np.array_equal(zero, ~r_has), what
    err = np.abs(rows[:, 6:9].astype(np.float64) - r_rows[:, 6:9].astype(np.float64))
    print(f"{what}: {rows.shape[0]} rows, {int(zero.sum())} without a normal; {int((err > 0).sum())} of {err.size} normal "
          f"components differ, largest {err.max() if err.size else 0.0:.3e} (bound {2.0 ** -23:.3e})")
    assert (err <= 2.0 ** -23).all(), what


def _same_rows(dev, c, key, what, columns=(3, 6, 9), **kw):
    """unproject of a case against unproject_ref of it: N, pixel_of_point, position and colour bits, the rows without a
    normal, the normals within 2^-23"""
    from detection_3d_amd.unproject import unproject
    r_rows, r_pix, r_has = F.unproject_case_ref(c, key, **kw)
    fr = _frames(dev, c)
    for ncols in columns:
        rows, pix = unproject(fr, columns=ncols, return_pixels=True, **kw)
        assert rows.dtype == torch.float32 and pix.dtype == torch.int32
        rows, pix = rows.cpu().numpy(), pix.cpu().numpy()
        assert rows.shape == (r_rows.shape[0], ncols), (what, ncols)
        assert np.array_equal(pix, r_pix), (what, ncols)
        k = min(ncols, 6)
        assert np.array_equal(_bits(rows[:, :k]), _bits(r_rows[:, :k])), (what, ncols)
        if ncols == 9:
            _same_normals(rows, r_rows, r_has, what)
    return rows, pix


@pytest.mark.parametrize("float_depth", [False, True])
@pytest.mark.parametrize("shape", F.U1_SHAPES)
def test_u1_full_steps_and_run_edges(dev, shape, float_depth):
    _same_rows(dev, F.unproject_case("u1", shape, float_depth), ("u1", shape, float_depth), ("u1", shape, float_depth))


@pytest.mark.parametrize("float_depth", [False, True])
def test_u2_empty_steps_and_runs(dev, float_depth):
    c = F.unproject_case("u2", F.U2_SHAPE, float_depth, mask=F.u2_mask())
    rows, _ = _same_rows(dev, c, ("u2", float_depth), ("u2", float_depth), columns=(3, 9))
    assert rows.shape[0] == 772


@pytest.mark.parametrize("step", F.U3_STEPS)
def test_u3_lattice(dev, step):
    shape = F.U1_SHAPES[3]
    c = F.unproject_case("u1", shape, False)
    _, pix = _same_rows(dev, c, ("u1", shape, False), ("u3", step), step=step)
    assert step != 100 or pix.tolist() == [0, shape[1] * shape[2]]


def test_u4_frame_seams(dev):
    c = F.unproject_case("u4", F.U4_SHAPE, cams=F.u4_cameras())
    _same_rows(dev, c, "u4", "u4", columns=(9,), edge=1.0)


def test_u5_fp32_colour_and_no_colour(dev):
    mask = F.u2_mask()
    c = F.unproject_case("u5", F.U2_SHAPE, mask=mask, color="fp32")
    rows, pix = _same_rows(dev, c, "u5", "u5 fp32 colour", columns=(6, 9))
    assert np.array_equal(_bits(rows[:, 3:6]), _bits(c["color"].reshape(-1, 3)[pix]))
    none = F.unproject_case("u5", F.U2_SHAPE, mask=mask, color=None)
    rows, _ = _same_rows(dev, none, "u5 none", "u5 no colour", columns=(6, 9))
    assert not _bits(rows[:, 3:6]).any()


def test_u6_guards(dev):
    """the C entries on 2 x 32 x 64 dense pixels with outputs 8 rows too long: nothing past N is written, nor past N - 5"""
    from detection_3d_amd._lib import check, lib, ptr, stream_of
    shape = F.U1_SHAPES[3]
    c = F.unproject_case("u1", shape, False)
    r_rows, r_pix, r_has = F.unproject_case_ref(c, ("u1", shape, False))
    fr, L = _frames(dev, c), lib()
    with torch.cuda.device(dev):
        s = stream_of(dev)
        nbytes = L.d3d_unproject_scratch_bytes(*shape, 1)
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        info = (ctypes.c_int * 1)(0)
        check(L.d3d_unproject_count(fr.desc, 1, 0.0, INF, ptr(buf), nbytes, info, s))
        N = int(info[0])
        assert N == len(r_pix) == 2 * F.RUN
        for ncols in (3, 6, 9):
            for cut in (0, 5):
                out = torch.full((N + PAD, ncols), NAN, dtype=torch.float32, device=dev)
                pix = torch.full((N + PAD,), SENT_I, dtype=torch.int32, device=dev)
                given = (ctypes.c_int * 1)(N - cut)
                check(L.d3d_unproject_rows(fr.desc, 1, 0.0, INF, 256.0, 0.05, ncols, given, ptr(buf), nbytes, ptr(out),
                                           ptr(pix), s))
                torch.cuda.synchronize()
                out, pix, m, k = out.cpu().numpy(), pix.cpu().numpy(), N - cut, min(ncols, 6)
                assert np.array_equal(pix[:m], r_pix[:m]) and (pix[m:] == SENT_I).all(), (ncols, cut)
                assert np.array_equal(_bits(out[:m, :k]), _bits(r_rows[:m, :k])), (ncols, cut)
                assert np.isnan(out[m:]).all(), (ncols, cut)
                if ncols == 9:
                    _same_normals(out[:m], r_rows[:m], r_has[:m], ("u6", cut))
