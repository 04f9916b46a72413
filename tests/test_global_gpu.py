"""d3d_global_align on the GPU, every table and output equal to the numpy restatement of tests/global_ref.py (register.
lattice_align: the entry point as it stands), then register.global_align through manhattan_frame and icp, and
merge_scans(init_poses='global')."""
import numpy as np
import pytest
import torch

from tests import global_ref as g

pytestmark = pytest.mark.gpu

LAT, BIN = (256, 256, 64), 0.1
KEYS = ("hist", "target_bits", "corr", "peak_value", "peak_shift", "scores", "choice", "score", "support")
_CACHE = {}


def _gpu(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(dev, src, tgt, o_s=None, o_t=None, views=None, **kw):
    """src, tgt: host [.., 6] (xyz, normal) -> every output of lattice_align as numpy, shaped as global_ref shapes them"""
    from detection_3d_amd.register import lattice_align
    o_s = g.origin_of(src[:, :3]) if o_s is None else np.asarray(o_s, np.float64)
    o_t = g.origin_of(tgt[:, :3]) if o_t is None else np.asarray(o_t, np.float64)
    if views is None:
        s, t = _gpu(dev, src), _gpu(dev, tgt)
        views = (s, s[:, 3:6], t, t[:, 3:6])
    kw.setdefault("bin", BIN)
    kw.setdefault("lattice", LAT)
    found = lattice_align(views[0], views[1], _gpu(dev, o_s), views[2], views[3], _gpu(dev, o_t), return_details=True, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in found.details.items()}
    out["target_bits"] = out["target_bits"].view(np.uint32)
    count = out.pop("cell_count")
    cells = out.pop("cells")
    assert (count >= 0).all() and (count <= cells.shape[1]).all()
    out["cells"] = [cells[k, :count[k]] for k in (0, 1)]
    out.update(pose=found.pose.cpu().numpy(), choice=found.choice.cpu().numpy(), score=found.score.cpu().numpy(),
               support=found.support.cpu().numpy(), status=int(found.state.cpu()[0]), found=found)
    assert found.status == out["status"]
    return out


def _ref(src, tgt, o_s=None, o_t=None, **kw):
    o_s = g.origin_of(src[:, :3]) if o_s is None else np.asarray(o_s, np.float64)
    o_t = g.origin_of(tgt[:, :3]) if o_t is None else np.asarray(o_t, np.float64)
    kw.setdefault("bin", BIN)
    kw.setdefault("lattice", LAT)
    return g.global_ref(src[:, :3], src[:, 3:6], o_s, tgt[:, :3], tgt[:, 3:6], o_t, **kw)


def _same(got, ref, what=""):
    print(f"{what}: choice {got['choice'].tolist()} / {ref['choice'].tolist()}, score {got['score'].tolist()} / "
          f"{ref['score'].tolist()}, support {got['support'].tolist()} / {ref['support'].tolist()}, status {got['status']} / "
          f"{ref['status']}, cells {[len(c) for c in got['cells']]} / {[len(c) for c in ref['cells']]}")
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k, got[k].dtype, got[k].shape)
        assert np.array_equal(got[k], ref[k]), (what, k)
    for k in (0, 1):
        assert np.array_equal(got["cells"][k], ref["cells"][k]), (what, "cells", k)
    assert got["status"] == ref["status"], what
    assert np.array_equal(got["pose"].view(np.uint64), ref["pose"].view(np.uint64)), (what, got["pose"], ref["pose"])


def _check(dev, src, tgt, what="", **kw):
    got, ref = _run(dev, src, tgt, **kw), _ref(src, tgt, **kw)
    _same(got, ref, what)
    return got, ref


def _scene():
    """a cropped pair of the building (30 k samples a scan, a quarter turn and metres apart) with rows that must not take
    part sprinkled in, and its reference: computed once and shared, nothing modifies them"""
    if "scene" not in _CACHE:
        src, tgt, truth = g.pair(1, 1, n=30000)
        rng = np.random.RandomState(3)
        for cloud in (src, tgt):
            rows = rng.permutation(len(cloud))[:80].reshape(8, 10)
            cloud[rows[0], 0] = np.nan
            cloud[rows[1], 4] = np.nan
            cloud[rows[2], 1] = np.inf
            cloud[rows[3], 2] = np.float32(3.0e38)         # finite, and far off the lattice
            cloud[rows[4], 3:6] = 0.0
            cloud[rows[5], 3:6] = np.array([0.7, 0.0, 0.0], np.float32)         # squared length 0.49
            cloud[rows[6], 3:6] = np.array([1.0, -1.0, 0.1], np.float32)        # 2.01
            cloud[rows[7], 3:6] = np.array([0.6, 0.6, 0.52], np.float32)        # a fine length and no class
        src[rng.permutation(len(src))[:7], 0] += np.float32(1000.0)             # off the lattice: dropped and counted
        _CACHE["scene"] = (src, tgt, truth, _ref(src, tgt))
    return _CACHE["scene"]


def test_scene_matches_the_restatement_in_every_table(dev):
    src, tgt, truth, ref = _scene()
    assert ref["status"] == 0 and ref["choice"][0] == 1 and ref["support"][1] >= 7 and ref["support"][3] >= 10
    assert min(len(c) for c in ref["cells"]) > 300 and (ref["peak_value"][:8] > 0).sum() > 100
    got = _run(dev, src, tgt)
    _same(got, ref, "scene")
    found = got["found"]
    assert found.quarter_turns == 1 and found.best == ref["score"][4] and found.margin == ref["margin"]
    assert found.heading_scores == ref["score"][:4].tolist()
    # the pose is the truth to a bin
    assert (g.shift_error(got["pose"], truth, src[100, :3].astype(np.float64)) <= BIN).all()


def test_column_slices_permutation_repeat_phases_and_side_stream_give_equal_bits(dev):
    from detection_3d_amd.register import GLOBAL_PHASES
    src, tgt, _, ref = _scene()
    nine = []
    for cloud in (src, tgt):
        wide = np.random.RandomState(5).rand(len(cloud), 9).astype(np.float32)
        wide[:, :3], wide[:, 6:9] = cloud[:, :3], cloud[:, 3:6]
        nine.append(_gpu(dev, wide))
    views = (nine[0], nine[0][:, 6:9], nine[1], nine[1][:, 6:9])
    assert not views[1].is_contiguous()
    _same(_run(dev, src, tgt, views=views), ref, "nine columns")
    rng = np.random.RandomState(9)
    _same(_run(dev, src[rng.permutation(len(src))], tgt[rng.permutation(len(tgt))]), ref, "permuted")
    _same(_run(dev, src, tgt), ref, "again")
    timed = _run(dev, src, tgt, phases=True)
    _same(timed, ref, "phases")
    assert set(timed["found"].phases) == set(GLOBAL_PHASES) and all(v > 0 for v in timed["found"].phases.values())
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other = _run(dev, src, tgt)
    side.synchronize()
    _same(other, ref, "side stream")


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025])
def test_row_counts_around_a_chunk(dev, n):
    src, tgt, _, _ = _scene()
    o_s, o_t = g.origin_of(src[:, :3]), g.origin_of(tgt[:, :3])
    got, _ = _check(dev, src[:n], tgt, f"{n} source rows", o_s=o_s, o_t=o_t)
    if n == 0:
        assert got["status"] == 1 and np.array_equal(got["pose"][:3, 3], o_t - o_s) and got["score"][4] == -1
    got, _ = _check(dev, src, tgt[:n], f"{n} target rows", o_s=o_s, o_t=o_t)
    if n == 0:
        assert got["status"] == 1 and got["support"].tolist()[2:] == [0, 0]
    _check(dev, src[:n], tgt[:n], f"{n} rows each", o_s=o_s, o_t=o_t)


def _rows(cells_x=(), cells_y=(), cells_z=(), z=0):
    """rows at the centres of cells of edge 1 from the origin 0: wall rows of class x and y at (cx, cy, z), floor rows"""
    out = []
    for k, cells in enumerate((cells_x, cells_y, cells_z)):
        for c in cells:
            p = np.zeros(6, np.float32)
            p[:3] = [c[0] + 0.5, c[1] + 0.5, (c[2] if len(c) > 2 else z) + 0.5]
            p[3 + k] = 1.0
            out.append(p)
    return np.stack(out) if out else np.zeros((0, 6), np.float32)


HAND = dict(bin=1.0, lattice=(64, 64, 16), o_s=np.zeros(3), o_t=np.zeros(3))


@pytest.mark.parametrize("nx,ny", [(0, 1), (1, 0), (1024, 1025), (1025, 1024), (4096, 3)])
def test_source_cell_lists_of_edge_lengths(dev, nx, ny):
    rng = np.random.RandomState(nx + ny)
    every = [(c % 64, c // 64) for c in range(4096)]
    cx = [every[c] for c in rng.permutation(4096)[:nx]]
    cy = [every[c] for c in rng.permutation(4096)[:ny]]
    src = np.concatenate([_rows(cx, cy), _rows(cx[:5], cy[:5], z=3)])          # a cell holds one bit, however many rows
    tgt = _rows(cx, cy, [(0, 0, 1)])
    got, ref = _check(dev, src, tgt, f"lists of {nx} and {ny}", **HAND)
    assert [len(c) for c in got["cells"]] == [nx, ny]
    if nx and ny:                       # (a cloud with walls of one class only has no candidate: status 1)
        assert got["status"] == 0 and got["score"][4] == nx + ny
    else:
        assert got["status"] == 1


def _ell(L):
    """walls along the lattice's edges that no turn maps onto themselves: cells at 0 and L - 1 on both axes"""
    cx = [(0, y) for y in range(0, L)] + [(L - 1, y) for y in range(0, 9)] + [(20, y) for y in range(30, 34)]
    cy = [(x, 0) for x in range(0, L)] + [(x, L - 1) for x in range(L - 5, L)] + [(31, 7), (32, 7), (33, 9)]
    return cx, cy


@pytest.mark.parametrize("q", [0, 1, 2, 3])
def test_cells_at_the_lattice_edges_under_every_turn(dev, q):
    L = 64
    cx, cy = _ell(L)
    src = _rows(cx, cy, [(1, 1, 2)])
    tx = [g.turn(q, x, y, L) for x, y in (cx if q % 2 == 0 else cy)]
    ty = [g.turn(q, x, y, L) for x, y in (cy if q % 2 == 0 else cx)]
    tgt = _rows(tx, ty, [(5, 5, 4)])
    got, ref = _check(dev, src, tgt, f"turn {q}", **HAND)
    assert got["choice"].tolist() == [q, 0, 0, 2] and got["score"][4] == len(cx) + len(cy)
    R = g.rigid(90.0 * q, (0, 0, 0))[:3, :3].round()
    assert np.array_equal(got["pose"][:3, :3], R) and np.array_equal(got["pose"][:3, 3], np.array([32.0, 32.0, 2.0]) - R @ [32.0, 32.0, 0.0])


def test_word_boundaries_dilation_at_the_edge_and_the_extreme_shifts(dev):
    L = 64
    # bits 31 and 32 of a row's two words, the lattice's corners and edges: the dilation crosses words and stops at the edge
    tx = [(31, 10), (32, 20), (0, 0), (63, 63), (63, 0), (0, 40), (31, 63)]
    ty = [(32, 11), (31, 21), (0, 63), (63, 31), (32, 0)]
    src = _rows([(0, 63), (30, 9)], [(0, 63), (33, 12)])
    got, ref = _check(dev, src, _rows(tx, ty), "words and edges", **HAND)
    img = np.zeros((L, L), bool)
    for x, y in tx:
        img[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    assert np.array_equal(got["target_bits"][0], g.bitmap_words(img))
    # the source's corner (0, L - 1) meets the target's corner (L - 1, 0) only under the shift (L - 1, -(L - 1))
    tgt = _rows([(63, 0)], [(63, 0)])
    got, ref = _check(dev, _rows([(0, 63)], [(0, 63)]), tgt, "extreme shifts", **HAND)
    assert got["peak_shift"][0, 0] == L - 1 and got["peak_shift"][1, 0] == -(L - 1)
    assert got["choice"].tolist() == [0, L - 1, -(L - 1), 0] and got["score"][4] == 2
    assert (got["peak_value"] == -1).any() and (got["scores"] == -1).any()         # fewer than K peaks: unused slots


def test_equal_values_inside_sep_and_equal_headings(dev):
    # two equal target walls a bin apart: the smoothed histogram holds n, 3 n, 3 n, n, and the first of the equal shifts is the peak
    tgt = _rows([(10, y) for y in range(8)] + [(11, y) for y in range(8)], [(x, 30) for x in range(6)])
    src = _rows([(40, y) for y in range(8)], [(x, 5) for x in range(6)])
    got, ref = _check(dev, src, tgt, "equal values", **HAND)
    C = got["corr"][0, :127]
    assert C[63 - 30] == C[63 - 29] == 3 * 8 * 8 and got["peak_shift"][0, 0] == -30
    assert not (got["peak_shift"][0][got["peak_value"][0] > 0] == -29).any()
    for sep in (0, 1, 5, 64):
        _check(dev, src, tgt, f"sep {sep}", sep=sep, **HAND)
    for peaks in (1, 2, 63):
        _check(dev, src, tgt, f"peaks {peaks}", peaks=peaks, **HAND)
    # a square room about the lattice's centre looks the same under every turn: equal best scores, the lowest index wins
    a, b = 12, 51
    room = _rows([(a, y) for y in range(a, b + 1)] + [(b, y) for y in range(a, b + 1)],
                 [(x, a) for x in range(a, b + 1)] + [(x, b) for x in range(a, b + 1)], [(20, 20, 0)])
    got, ref = _check(dev, room, room, "square room", **HAND)
    assert got["score"][:4].tolist() == [got["score"][4]] * 4 and got["score"][5] == got["score"][4]
    assert got["choice"].tolist() == [0, 0, 0, 0] and got["status"] == 0
    # no walls at all: status 1 and the origins' shift
    floor = _rows((), (), [(x, x, 1) for x in range(20)])
    got, ref = _check(dev, floor, floor, "floor only", bin=1.0, lattice=(64, 64, 16), o_s=np.array([1.0, 2.0, 0.5]),
                      o_t=np.array([-3.0, 0.25, 0.0]))
    assert got["status"] == 1 and got["pose"][:3, 3].tolist() == [-4.0, -1.75, -0.5] and got["found"].margin == float("inf")


def test_rows_off_the_lattice_are_dropped_and_counted(dev):
    src, tgt, _, _ = _scene()
    # an origin a metre inside the cloud and a lattice shorter than it: rows fall off on both sides of every axis
    o_s, o_t = g.origin_of(src[:, :3]) + 1.0, g.origin_of(tgt[:, :3]) + np.array([2.0, 0.5, 0.25])
    got, ref = _check(dev, src, tgt, "short lattice", o_s=o_s, o_t=o_t, lattice=(128, 128, 16))
    assert got["support"][1] > 1000 and got["support"][3] > 1000 and got["support"][0] > 100 and got["support"][2] > 100
    _check(dev, src, tgt, "long lattice", lattice=(512, 512, 300), peaks=16, tol=12.0)


def _ref_chain(src, tgt, **kw):
    """the chain of global_align + icp on the host: frame_ref's frames, global_ref, register_ref.icp_ref"""
    from tests import frame_ref
    from tests import register_ref as rr
    aligned, frames = [], []
    for cloud in (src, tgt):
        F = frame_ref.manhattan_frame_ref(cloud[:, 3:6])["pose"]
        frames.append(F)
        aligned.append(np.concatenate([(cloud[:, :3].astype(np.float64) @ F[:3, :3].T).astype(np.float32),
                                       (cloud[:, 3:6].astype(np.float64) @ F[:3, :3].T).astype(np.float32)], 1))
    found = g.align_ref(aligned[0], aligned[1], **kw)
    coarse = np.linalg.inv(frames[1]) @ found["pose"] @ frames[0]
    pose, steps, status, _ = rr.icp_ref(src[:, :3], tgt[:, :3], tgt[:, 3:6], coarse, 0.1, 30, 1e-6, "plane")
    return found, coarse, pose, steps, status


def test_global_align_then_icp_lands_where_the_reference_chain_does(dev):
    """One cropped pair (x <= 20 / x >= 5), the source a quarter turn, 0.05 degrees and metres away: global_align's pose
    starts icp, and the result is within twice the reference chain's errors against the true pose.  merge_scans with
    init_poses='global' runs the same two calls and must give the same pose."""
    from detection_3d_amd.register import global_align, icp, merge_scans
    from tests import register_ref as rr
    src, tgt, truth = g.pair(2, 1, n=60000)
    kw = dict(bin=0.05, lattice=(1024, 1024, 128))
    found_ref, coarse_ref, pose_ref, steps_ref, status_ref = _ref_chain(src, tgt, **kw)
    centre = src[:, :3].astype(np.float64).mean(0)
    ref_rot, ref_pos = rr.pose_errors(pose_ref, truth, centre)
    s, t = _gpu(dev, src), _gpu(dev, tgt)
    found = global_align(s, t, source_normals=s[:, 3:6], target_normals=t[:, 3:6], **kw)
    reg = icp(s, t, target_normals=t[:, 3:6], init=found.pose, max_dist=0.1, iterations=30, tol=1e-6)
    torch.cuda.synchronize()
    rot0, pos0 = rr.pose_errors(found.pose.cpu().numpy(), truth, centre)
    ref_rot0, ref_pos0 = rr.pose_errors(coarse_ref, truth, centre)
    rot, pos = rr.pose_errors(reg.pose.cpu().numpy(), truth, centre)
    print(f"coarse: {found!r}, rotation {rot0:.3g} rad (reference {ref_rot0:.3g}), centre {pos0:.3g} m (reference {ref_pos0:.3g}); "
          f"after icp: {reg.steps} steps (reference {steps_ref}), rotation {rot:.3g} rad (reference {ref_rot:.3g}), centre "
          f"{pos:.3g} m (reference {ref_pos:.3g})")
    assert status_ref == 1 and found_ref["status"] == 0 and found_ref["choice"][0] == 1
    assert found.status == 0 and found.choice.tolist() == found_ref["choice"].tolist()
    assert found.source_frame is not None and found.pose.dtype == torch.float64 and found.pose.is_cuda
    assert reg.converged
    assert rot <= 2.0 * ref_rot and pos <= 2.0 * ref_pos
    # nine-column clouds carry their normals in columns 6:9
    nine = [torch.cat([c[:, :3], torch.zeros_like(c[:, :3]), c[:, 3:6]], 1) for c in (s, t)]
    again = global_align(nine[0], nine[1], **kw)
    assert torch.equal(again.pose, found.pose) and torch.equal(again.choice, found.choice)
    merged, poses = merge_scans([nine[1], nine[0]], init_poses="global", global_kw=kw, voxel=0.02, max_dist=0.1,
                                iterations=30, tol=1e-6)
    m_rot, m_pos = rr.pose_errors(poses[1].cpu().numpy(), truth, centre)
    print(f"merge_scans: rotation {m_rot:.3g} rad, centre {m_pos:.3g} m")
    assert merged.shape[1] == 9 and np.array_equal(poses[0].cpu().numpy(), np.eye(4))
    assert m_rot <= 2.0 * ref_rot and m_pos <= 2.0 * ref_pos
    # (its model is the target through voxel_downsample, other rows in another order: the same pose, not the same bits)
    d_rot, d_pos = rr.pose_errors(poses[1].cpu().numpy(), reg.pose.cpu().numpy(), centre)
    assert d_rot <= 2.0 * ref_rot and d_pos <= 2.0 * ref_pos


def test_cpu_tensors_are_refused():
    from detection_3d_amd._lib import D3DError
    from detection_3d_amd.register import global_align
    with pytest.raises(D3DError):
        global_align(torch.zeros((8, 9)), torch.zeros((8, 9)))
