"""detection_3d_amd.normals.estimate_normals (normals.hip) against the fp64 restatement of its semantics in
tests/normals_ref.py, and its plumbing through engine.collate and serving.BuildingPipeline.

The angle bound is derived, not tuned: an eigenvector moves by |dC| / (l1 - l0); fp32 sums of at most 50 terms about the
query give |dC| <~ 50 * 2^-24 * l2 ~ 3e-6 l2; with 3x for the solver the angle stays below 1e-5 / gap,
gap = (l1 - l0) / l2.  Points where fp32 and fp64 may pick different neighbours (`edge`) or whose gap is below 1e-2 are
left out, and they may be at most 1 % of a scene."""
import numpy as np
import pytest
import torch

from tests.normals_ref import VIEWPOINT, dense_patch, make_scene, normals_ref

pytestmark = pytest.mark.gpu

_REF = {}


def _scene(n, seed):
    key = ("scene", n, seed)
    if key not in _REF:
        _REF[key] = make_scene(n, seed)
    return _REF[key]


def _ref(name, xyz, radius=0.1, max_nn=50, orient=None, tie_scale="radius"):
    key = (name, radius, max_nn, orient, tie_scale)
    if key not in _REF:
        _REF[key] = normals_ref(xyz, radius, max_nn, orient, tie_scale)
    return _REF[key]


def _run(dev, xyz, **kw):
    from detection_3d_amd.normals import estimate_normals
    n, c = estimate_normals(torch.from_numpy(np.ascontiguousarray(xyz)).to(dev), return_counts=True, **kw)
    return n.cpu().numpy(), c.cpu().numpy()


def _angles(a, b):
    """angle between the lines of a and b (up to sign), accurate for tiny angles"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.arcsin(np.minimum(1.0, np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) *
                                                                             np.linalg.norm(b, axis=1))))


def _check(got_n, got_c, ref, rows=None, what=""):
    """checks 1-3 of the issue on the rows `rows` (default: all) of a run"""
    ref_n, ref_c, gap, edge = ref
    if rows is not None:
        ref_n, ref_c, gap, edge = ref_n[rows], ref_c[rows], gap[rows], edge[rows]
    total = ref_c.shape[0]
    # 1. counts, exactly, away from the edge points
    bad = np.flatnonzero((got_c != ref_c) & ~edge)
    print(f"{what}: {total} points, median count {np.median(ref_c)}, edge {int(edge.sum())}, count mismatches {bad.size}")
    assert bad.size == 0, (what, bad[:10], got_c[bad[:10]], ref_c[bad[:10]])
    # 2. angles
    has = ref_c >= 3
    sel = has & ~edge & (gap >= 1e-2)
    left_out = int((has & ~sel).sum())
    assert left_out <= 0.01 * total, (what, left_out, total)
    ang = _angles(got_n[sel], ref_n[sel])
    worst = float((ang * gap[sel]).max()) if sel.any() else 0.0
    print(f"{what}: {int(sel.sum())} angles compared, {left_out} left out, max angle * gap {worst:.3e} (bound 1e-5)")
    over = np.flatnonzero(ang > 1e-5 / gap[sel])
    assert over.size == 0, (what, over[:10], ang[over[:10]], gap[sel][over[:10]])
    # 3. unit length; (0, 0, 1) exactly below three neighbours
    length = np.linalg.norm(got_n.astype(np.float64), axis=1)
    assert np.abs(length - 1.0).max() <= 1e-6, (what, np.abs(length - 1.0).max())
    few = got_c < 3
    assert np.array_equal(got_n[few], np.tile(np.float32([0, 0, 1]), (int(few.sum()), 1))), what


@pytest.mark.parametrize("n,seed", [(4000, 0), (4000, 1), (8000, 2)])
def test_counts_angles_and_lengths_on_the_box_scenes(dev, n, seed):
    xyz = _scene(n, seed)
    got_n, got_c = _run(dev, xyz)
    _check(got_n, got_c, _ref(("box", n, seed), xyz), what=f"scene({n}, {seed})")
    assert (got_c < 3).any() and (got_c == 50).any()          # the isolated points and capped queries are there


def test_sign_canonical_and_towards_a_viewpoint(dev):
    xyz = _scene(4000, 0)
    ref_n, ref_c, gap, edge = _ref(("box", 4000, 0), xyz)
    got_n, got_c = _run(dev, xyz)
    k = np.argmax(np.abs(got_n), axis=1)                     # first maximum: ties go to the lowest axis
    assert (np.take_along_axis(got_n, k[:, None], 1)[:, 0] > 0).all()
    vn, vc = _run(dev, xyz, orient=VIEWPOINT)
    assert np.array_equal(vc, got_c)
    has = got_c >= 3
    assert np.array_equal(np.abs(vn), np.abs(got_n))          # the same line, whatever the sign
    to_v = np.float32(VIEWPOINT).astype(np.float64)[None, :] - xyz.astype(np.float64)
    v64 = vn.astype(np.float64)
    dots = (v64[:, 0] * to_v[:, 0] + v64[:, 1] * to_v[:, 1]) + v64[:, 2] * to_v[:, 2]
    assert (dots[has] >= 0).all(), dots[has].min()
    assert np.array_equal(vn[~has], np.tile(np.float32([0, 0, 1]), (int((~has).sum()), 1)))
    ref_v = _ref(("box", 4000, 0), xyz, orient=VIEWPOINT)[0]
    clear = has & ~edge & (np.abs((ref_v * to_v).sum(1)) / np.linalg.norm(to_v, axis=1) > 1e-3)
    assert clear.sum() > 0.9 * has.sum()
    assert ((v64[clear] * ref_v[clear]).sum(1) > 0).all()


@pytest.mark.parametrize("kw", [dict(max_nn=8), dict(max_nn=1000), dict(radius=0.05)], ids=lambda k: str(k))
def test_other_parameters(dev, kw):
    xyz = _scene(4000, 0)
    got_n, got_c = _run(dev, xyz, **kw)
    ref = _ref(("box", 4000, 0), xyz, **kw)
    _check(got_n, got_c, ref, what=f"scene(4000, 0) {kw}")
    if kw.get("max_nn") == 8:
        assert (got_c == 8).mean() > 0.9
    if kw.get("max_nn") == 1000:
        assert got_c.max() < 1000


def test_dense_cell_beyond_the_staging_budget(dev):
    """3000 points in a 5 cm cube: every query there has thousands of candidates (read from global memory, the cut taken
    among them), beside a scene that takes the staged path.  The tie flag is the tighter one of normals_ref
    (tie_scale='cut'): at this density the absolute 1e-5 r^2 flags 28 % of the dense points (843 of 3000 measured), far
    past the 1 % that may be left out, whatever computes the normals; against the cut distance itself a handful are
    flagged and every other point is held to the bound."""
    xyz = np.concatenate([dense_patch(3000, 5), _scene(4000, 0)])
    got_n, got_c = _run(dev, xyz)
    assert (got_c[:3000] == 50).all()
    _check(got_n, got_c, _ref("dense", xyz, tie_scale="cut"), what="dense cell + scene(4000, 0)")


@pytest.mark.parametrize("k", [7, 49])
def test_normals_and_cleaning_keep_the_same_neighbours(dev, k):
    """The three cell-list queries share one notion of "kept": the normals' count at max_nn = k + 1 is the k nearest
    neighbours that knn_mean_distance found plus the point itself, and both are the radius count capped at k + 1, on
    the staged path (the scene) and the unstaged one (the dense cell)."""
    from detection_3d_amd.clean import knn_mean_distance, radius_neighbors
    xyz = np.concatenate([_scene(4000, 0), dense_patch(3000, 5)])
    t = torch.from_numpy(xyz).to(dev)
    counts = _run(dev, xyz, max_nn=k + 1)[1]
    found = knn_mean_distance(t, k=k, radius=0.1)[1].cpu().numpy()
    within = radius_neighbors(t, radius=0.1).cpu().numpy()
    assert (within < k + 1).any() and (within > k + 1).any() and (within[4000:] > 1024).all()
    assert np.array_equal(counts, found + 1)
    assert np.array_equal(counts, np.minimum(within, k + 1))


def test_two_copies_500_m_apart(dev):
    from detection_3d_amd._lib import lib
    a = _scene(4000, 0)
    b = (a + np.float32([-500.0, -30.0, 0.0])).astype(np.float32)          # at negative coordinates
    both = np.concatenate([a, b])
    got_n, got_c = _run(dev, both)
    for rows, alone in ((slice(0, 4000), a), (slice(4000, 8000), b)):
        assert np.array_equal(got_c[rows], _run(dev, alone)[1])            # the copy on its own: the same counts
    ref = _ref("far", both)
    _check(got_n[:4000], got_c[:4000], ref, rows=slice(0, 4000), what="copy at +")
    _check(got_n[4000:], got_c[4000:], ref, rows=slice(4000, 8000), what="copy at -500 m")
    # the scratch is sized by the point count alone (no lattice over the extent): linear in n
    nbytes = lib().d3d_estimate_normals_scratch_bytes(8000, 50)
    assert nbytes <= 256 * 8000 + (1 << 17), nbytes
    assert lib().d3d_estimate_normals_scratch_bytes(1 << 20, 50) <= 256 * (1 << 20) + (1 << 17)


def test_small_inputs(dev):
    from detection_3d_amd.normals import estimate_normals
    z = np.float32([0, 0, 1])
    n, c = estimate_normals(torch.zeros((0, 3), device=dev), return_counts=True)
    assert n.shape == (0, 3) and c.shape == (0,) and n.dtype == torch.float32 and c.dtype == torch.int32
    for k in (1, 2):
        pts = np.float32([[1.0, 2.0, 3.0], [1.05, 2.0, 3.0]])[:k]
        gn, gc = _run(dev, pts)
        assert gc.tolist() == [k] * k and np.array_equal(gn, np.tile(z, (k, 1)))
    gn, gc = _run(dev, np.tile(np.float32([[3.0, -2.0, 0.5]]), (100, 1)))
    assert (gc == 50).all() and np.array_equal(gn, np.tile(z, (100, 1)))
    gn, gc = _run(dev, np.tile(np.float32([[3.0, -2.0, 0.5]]), (100, 1)), orient=(0.0, 0.0, -5.0))
    assert (gc == 50).all() and np.array_equal(gn, np.tile(z, (100, 1)))


def test_stride_streams_and_reproducibility(dev):
    from detection_3d_amd.normals import estimate_normals
    xyz = torch.from_numpy(_scene(4000, 1)).to(dev)
    pcl9 = torch.cat([xyz, torch.rand((4000, 6), device=dev)], 1)
    n0, c0 = estimate_normals(xyz, return_counts=True)
    n1, c1 = estimate_normals(xyz, return_counts=True)
    assert torch.equal(n0, n1) and torch.equal(c0, c1)                       # run to run
    n2, c2 = estimate_normals(pcl9[:, :3], return_counts=True)               # read through the row stride
    assert torch.equal(n0, n2) and torch.equal(c0, c2)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        n3, c3 = estimate_normals(pcl9[:, :3], return_counts=True)
    side.synchronize()
    assert torch.equal(n0, n3) and torch.equal(c0, c3)
    assert torch.equal(estimate_normals(xyz), n0)


def test_with_normals_on_the_gpu(dev):
    from detection_3d_amd.normals import estimate_normals, with_normals
    xyz = torch.from_numpy(_scene(4000, 0)).to(dev)
    nrm = estimate_normals(xyz)
    rgb = torch.rand((4000, 3), device=dev)
    out3, out6 = with_normals(xyz), with_normals(torch.cat([xyz, rgb], 1))
    out9 = with_normals(torch.cat([xyz, rgb, torch.full((4000, 3), 7.0, device=dev)], 1))
    assert out3.shape == out6.shape == out9.shape == (4000, 9)
    assert torch.equal(out3[:, :3], xyz) and torch.equal(out3[:, 3:6], torch.zeros_like(xyz))
    assert torch.equal(out6[:, 3:6], rgb) and torch.equal(out9[:, :6], out6[:, :6])
    for out in (out3, out6, out9):
        assert torch.equal(out[:, 6:9], nrm)


@pytest.fixture(scope="module")
def tiny(dev):
    """the model and scene of tests/test_detector_gpu.py"""
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.detector import build_detection_model
    from detection_3d_amd.synthetic import make_scene as make_building
    cfg = get_cfg("4c_Fpn432")
    torch.manual_seed(1)
    model = build_detection_model(cfg).to(dev).eval()
    with torch.no_grad():
        model.rpn.head.cls_logits.weight.mul_(60)
        model.rpn.head.bbox_pred.weight.mul_(20)
        model.roi_heads.box.predictor.cls_score.weight.mul_(40)
        model.roi_heads.box.predictor.bbox_pred.weight.mul_(100)
    return cfg, model, torch.from_numpy(make_building(3, 40000)).to(dev)


def _same(a, b):
    return all(a[k].shape == b[k].shape and torch.equal(a[k], b[k]) for k in ("bbox3d", "scores", "labels"))


def test_pipeline_estimates_normals_before_it_voxelises(tiny, dev):
    from detection_3d_amd.normals import with_normals
    from detection_3d_amd.serving import BuildingPipeline
    cfg, model, cloud9 = tiny
    cloud6 = cloud9[:, :6].contiguous()
    with torch.no_grad():
        got = BuildingPipeline(model, cfg, in_flight=2, device=dev, normals="estimate").map([cloud6, cloud6])
        want = BuildingPipeline(model, cfg, in_flight=2, device=dev).map([with_normals(cloud6)])
        kw = BuildingPipeline(model, cfg, in_flight=2, device=dev, normals={"radius": 0.2, "max_nn": 30}).map([cloud6])
        want_kw = BuildingPipeline(model, cfg, in_flight=2, device=dev).map([with_normals(cloud6, 0.2, 30)])
        plain = BuildingPipeline(model, cfg, in_flight=2, device=dev).map([cloud9])
        plain_none = BuildingPipeline(model, cfg, in_flight=2, device=dev, normals=None).map([cloud9])
    torch.cuda.synchronize()
    assert want[0]["bbox3d"].shape[0] > 0
    assert _same(got[0], want[0]) and _same(got[1], want[0])
    assert _same(kw[0], want_kw[0])
    assert _same(plain[0], plain_none[0])


def test_collate_estimates_normals(tiny, dev):
    from detection_3d_amd import engine
    from detection_3d_amd.normals import with_normals
    cfg, _, cloud9 = tiny
    cloud6 = cloud9[:, :6].contiguous()
    tg = {"bbox3d": torch.zeros((0, 7)), "labels": torch.zeros((0,), dtype=torch.int64)}
    got, _ = engine.collate([(cloud6, tg), (cloud6[:20000], tg)], cfg, normals="estimate")
    want, _ = engine.collate([(with_normals(cloud6), tg), (with_normals(cloud6[:20000]), tg)], cfg)
    assert got[2] == want[2] == 2 and got[1].shape[1] == 9
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    plain, _ = engine.collate([(cloud9, tg)], cfg)
    plain_none, _ = engine.collate([(cloud9, tg)], cfg, normals=None)
    assert torch.equal(plain[0], plain_none[0]) and torch.equal(plain[1], plain_none[1])
