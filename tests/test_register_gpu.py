"""detection_3d_amd.register (register.hip) against the restatement of its semantics in tests/register_ref.py.

Bounds.  nearest is defined in fp32 operation by operation, so index and the bits of dist2 must EQUAL the reference's,
with no point excused.  One ICP step sums 29 fp64 series whose terms the reference computes with the same operations;
only the order of the additions differs, and a sum of c terms in any order is within c 2^-53 sum|terms| of the exact
one (Higham 4.4), the reference's own numpy sum likewise: 4 c 2^-53 sum|terms| leaves a margin of 2 over the two.  The
solve turns a relative perturbation d of the system into one of cond(A) d of the solution; the pose after the step is
compared within 1e3 cond(A) 2^-53 of max(1, |entry|), cond(A) from the reference's system.  A trajectory is checked
step by step from the bits of the previous row, so that no difference builds up.  Recovery and merging are compared
with the errors the reference itself makes on the same inputs, times 2: the scenes' 3 mm noise sets the floor, not the
arithmetic."""
import numpy as np
import pytest
import torch

from tests import clean_ref
from tests import register_ref as rr
from tests.normals_ref import SHIFT, dense_patch, make_scene

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
_REF = {}


def _cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _scene(n, seed):
    return _cached(("scene", n, seed), lambda: make_scene(n, seed))


def _cloud0():
    return _cached(("cloud", 0), lambda: clean_ref.make_cloud(0))


def _gpu(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- nearest ----
def _check_nearest(dev, query, cloud, radius, what, gpu_query=None, gpu_cloud=None):
    """index and the bits of dist2 equal the reference's; -> (index, dist2) of the reference"""
    from detection_3d_amd.register import nearest
    ref_i, ref_d = rr.nearest_ref(query, cloud, radius)
    q = _gpu(dev, query) if gpu_query is None else gpu_query
    c = _gpu(dev, cloud) if gpu_cloud is None else gpu_cloud
    index, dist2 = nearest(q, c, radius, return_dist2=True)
    assert index.dtype == torch.int32 and dist2.dtype == torch.float32
    assert index.shape == dist2.shape == (query.shape[0],)
    only = nearest(q, c, radius)
    index, dist2, only = index.cpu().numpy(), dist2.cpu().numpy(), only.cpu().numpy()
    bad = np.flatnonzero((index != ref_i) | (_bits(dist2) != _bits(ref_d)))
    print(f"{what} r {radius}: {query.shape[0]} queries, {cloud.shape[0]} points, found {int((ref_i >= 0).sum())}, "
          f"mismatches {bad.size}")
    assert bad.size == 0, (what, bad[:10], index[bad[:10]], ref_i[bad[:10]], dist2[bad[:10]], ref_d[bad[:10]])
    assert np.array_equal(only, ref_i)
    return ref_i, ref_d


@pytest.mark.parametrize("radius", [0.05, 0.1])
def test_nearest_between_two_scans_of_the_scene(dev, radius):
    ref_i, _ = _check_nearest(dev, _scene(6000, 1), _scene(6000, 0), radius, "scene 1 -> scene 0")
    assert (ref_i >= 0).sum() > 5000 and (ref_i < 0).sum() >= 10          # the 16 isolated points find nothing


def test_nearest_of_queries_left_of_the_lattice_and_beyond_reach(dev):
    cloud = _scene(6000, 0)
    query = _scene(6000, 1) + np.float32([-0.3, 0.0, 0.0])
    left = query[:, 0] < cloud[:, 0].min()
    ref_i, _ = _check_nearest(dev, query, cloud, 0.1, "shifted by -0.3 in x")
    near = left & (query[:, 0] > cloud[:, 0].min() - 0.1)
    print(f"left of the minimum {int(left.sum())}, of those within a cell {int(near.sum())}, found {int((ref_i[left] >= 0).sum())}")
    assert left.sum() > 500 and (ref_i[left] >= 0).sum() > 0 and (ref_i[left] < 0).sum() > 100


def test_nearest_with_a_point_far_away_duplicates_and_a_dense_cell(dev):
    far = np.concatenate([_cloud0(), np.float32([[1013.7, -4.2, 1.1]])])          # one point 1 km away
    query = np.concatenate([_scene(3000, 1), np.float32([[1013.7, -4.19, 1.1], [513.0, -4.2, 1.1]])])
    ref_i, _ = _check_nearest(dev, query, far, 0.1, "one point 1 km away")
    assert ref_i[-2] == far.shape[0] - 1 and ref_i[-1] == -1
    a = _cloud0()
    twice = np.concatenate([a, a[np.random.RandomState(3).permutation(a.shape[0])]])   # every point twice
    ref_i, ref_d = _check_nearest(dev, a[::3], twice, 0.1, "every point twice")
    assert (ref_d == 0).all() and np.array_equal(ref_i, np.arange(a.shape[0], dtype=np.int32)[::3])   # the lower row
    dense = dense_patch(2000, 5)                                                   # > 1024 candidates in the 27 cells
    ref_i, _ = _check_nearest(dev, dense_patch(600, 6), dense, 0.1, "dense patch")
    assert (ref_i >= 0).all()


def test_nearest_with_rows_that_are_not_finite(dev):
    cloud = _scene(6000, 0).copy()
    cloud[100, 0] = np.nan
    cloud[200, 1] = np.inf
    cloud[300] = np.nan
    query = _scene(3000, 1).copy()
    query[:3] = _scene(6000, 0)[[100, 200, 300]]                                   # where the unusable rows were
    query[10, 2] = np.nan
    query[11, 0] = np.inf
    query[12, 1] = -np.inf
    query[13] = np.nan
    ref_i, ref_d = _check_nearest(dev, query, cloud, 0.1, "NaN and inf rows")
    assert (ref_i[10:14] == -1).all() and np.isinf(ref_d[10:14]).all()
    assert not np.isin(ref_i, [100, 200, 300]).any()
    low = _scene(600, 0).copy()
    low[7, 2] = -np.inf                                                            # the minimum itself is not finite
    _check_nearest(dev, _scene(300, 1), low, 0.1, "-inf in the cloud")


@pytest.mark.parametrize("m,n", [(1, 6000), (6000, 1), (0, 6000), (6000, 0), (0, 0), (1, 1), (129, 6000), (2049, 6000)])
def test_nearest_at_the_size_edges(dev, m, n):
    cloud = _scene(6000, 0)[:n]
    query = _scene(6000, 1)[:m]
    if n == 1:
        query = query.copy()
        query[5:8] = cloud[0] + np.float32([[0.0, 0.0, 0.0], [0.05, 0.0, 0.0], [0.2, 0.0, 0.0]])[:max(0, min(3, m - 5))]
    ref_i, _ = _check_nearest(dev, query, cloud, 0.1, f"M {m} N {n}")
    if n == 0:
        assert (ref_i == -1).all()
    if n == 1 and m > 8:
        assert ref_i[5] == 0 and ref_i[6] == 0 and ref_i[7] == -1


def test_nearest_reads_column_slices_in_place(dev):
    rs = np.random.RandomState(4)
    cloud, query = _scene(6000, 0), _scene(2049, 1)
    c9 = np.concatenate([rs.rand(6000, 3).astype(np.float32), cloud, rs.rand(6000, 3).astype(np.float32)], 1)
    q9 = np.concatenate([query, rs.rand(2049, 6).astype(np.float32)], 1)
    gc, gq = _gpu(dev, c9), _gpu(dev, q9)
    _check_nearest(dev, query, cloud, 0.1, "slices of nine columns", gpu_query=gq[:, :3], gpu_cloud=gc[:, 3:6])
    _check_nearest(dev, query, cloud, 0.1, "nine columns as they are", gpu_query=gq, gpu_cloud=gc[:, 3:])


def test_nearest_under_a_permutation_of_the_cloud(dev):
    from detection_3d_amd.register import nearest
    a = _cloud0()
    cloud = np.concatenate([a, a[:500]])                                           # some minima are not unique
    query = _gpu(dev, _scene(6000, 1))
    perm = np.random.RandomState(7).permutation(cloud.shape[0])
    i0, d0 = (t.cpu().numpy() for t in nearest(query, _gpu(dev, cloud), 0.1, return_dist2=True))
    i1, d1 = (t.cpu().numpy() for t in nearest(query, _gpu(dev, cloud[perm]), 0.1, return_dist2=True))
    assert np.array_equal(_bits(d0), _bits(d1))
    assert np.array_equal(i0 >= 0, i1 >= 0)
    hit = i0 >= 0
    same_point = (cloud[perm][i1[hit]] == cloud[i0[hit]]).all(1)                   # a tie: another row, the same place
    assert same_point.all()
    unique = hit.copy()
    unique[hit] = (i0[hit] >= 500) & (i0[hit] < a.shape[0])                        # rows without a duplicate
    assert unique.sum() > 4000 and np.array_equal(perm[i1[unique]], i0[unique])
    assert (perm[i1[hit]] != i0[hit]).sum() > 0                                    # and the ties did move


# ---- ICP ----
AXIS, DIRECTION = (0.3, -0.5, 0.8), np.array([1.0, -2.0, 0.5]) / np.linalg.norm([1.0, -2.0, 0.5])


def _pair(dev, n, degrees, cm):
    """target = scene 0, source = scene 1 moved about the cloud's centre -> dict(source, target, normals (the GPU's own
    estimate, fp32 on the host), truth (the pose that undoes the motion), centre)"""
    def make():
        from detection_3d_amd.normals import estimate_normals
        tgt = _scene(n, 0)
        centre = tgt.astype(np.float64).mean(0)
        motion = rr.motion_about(centre, AXIS, np.deg2rad(degrees), 0.01 * cm * DIRECTION)
        nrm = estimate_normals(_gpu(dev, tgt), 0.1, 50).cpu().numpy()
        return dict(source=rr.move(motion, _scene(n, 1)), target=tgt, normals=nrm, truth=np.linalg.inv(motion), centre=centre)
    return _cached(("pair", n, degrees, cm), make)


def _icp(dev, p, **kw):
    from detection_3d_amd.register import icp
    return icp(_gpu(dev, p["source"]), _gpu(dev, p["target"]), _gpu(dev, p["normals"]), **kw)


def _check_step(ref, row, pose_after, what, last_system=None, last_index=None):
    """one executed step against step_ref's result from the same pose: count exact, sums and pose within the bounds"""
    c = ref["c"]
    assert row[16] == c, (what, row[16], c)
    sum_bound = 4.0 * max(c, 1) * U * ref["magnitude"]
    assert abs(row[17] - ref["e"]) <= sum_bound[27], (what, row[17], ref["e"], sum_bound[27])
    if last_index is not None:
        assert np.array_equal(last_index, ref["index"]), what
    if last_system is not None:
        over = np.abs(last_system - ref["system"]) / np.where(sum_bound > 0, sum_bound, 1.0)
        print(f"{what}: c {c}, sums at most {over.max():.3g} of their bound")
        assert (np.abs(last_system - ref["system"]) <= sum_bound).all(), (what, last_system, ref["system"], sum_bound)
    cond = np.linalg.cond(rr.system_matrix(ref["system"])[0]) if ref["status"] != 2 else 1.0
    pose_bound = 1e3 * cond * U
    err = np.abs(pose_after.reshape(4, 4) - ref["pose"]) / np.maximum(1.0, np.abs(ref["pose"]))
    print(f"{what}: cond {cond:.3g}, pose within {err.max():.3g} (bound {pose_bound:.3g}), |w| {row[18]:.3g}, |v| {row[19]:.3g}")
    assert err.max() <= pose_bound, (what, err.max(), pose_bound)
    assert abs(row[18] - ref["wn"]) <= pose_bound and abs(row[19] - ref["vn"]) <= pose_bound, what
    return ref["status"]


@pytest.mark.parametrize("method", ["plane", "point"])
@pytest.mark.parametrize("start", ["identity", "given"])
def test_one_step_exact_pairs_and_tight_sums(dev, method, start):
    p = _pair(dev, 3000, 5.0, 5.0)
    init = np.eye(4) if start == "identity" else \
        rr.motion_about(p["centre"], (-0.2, 0.7, 0.4), np.deg2rad(1.0), (0.004, -0.006, 0.005)) @ p["truth"]
    reg = _icp(dev, p, init=torch.from_numpy(init), iterations=1, method=method, return_details=True)
    ref = rr.step_ref(init, p["source"], p["target"], p["normals"], 0.1, method)
    assert reg.pose.dtype == torch.float64 and reg.pose.shape == (4, 4) and reg.pose.is_cuda
    assert reg.history.shape == (1, 20) and reg.state.dtype == torch.int32
    assert ref["c"] > 1500
    row = reg.history[0].cpu().numpy()
    status = _check_step(ref, row, reg.pose.cpu().numpy(), f"{method} from {start}", reg.last_system.cpu().numpy(),
                         reg.last_index.cpu().numpy())
    assert np.array_equal(row[:16], reg.pose.cpu().numpy().ravel())
    assert reg.state.cpu().tolist() == [1, status] and reg.steps == 1 and reg.status == status
    assert reg.inliers == ref["c"] and abs(reg.rmse - np.sqrt(ref["e"] / ref["c"])) <= 1e-12


@pytest.mark.parametrize("method,iterations", [("plane", 30), ("point", 20)])
def test_every_step_of_a_trajectory(dev, method, iterations):
    p = _pair(dev, 6000, 3.0, 3.0)
    reg = _icp(dev, p, iterations=iterations, method=method)
    history = reg.history.cpu().numpy()
    steps, status = reg.state.cpu().tolist()
    assert 1 <= steps <= iterations
    pose = np.eye(4)
    for i in range(steps):
        ref = rr.step_ref(pose, p["source"], p["target"], p["normals"], 0.1, method)
        ref_status = _check_step(ref, history[i], history[i, :16], f"{method} step {i}")
        assert ref_status == (status if i == steps - 1 else 0) or abs(max(ref["wn"], ref["vn"]) - 1e-6) < 1e-9, (i, ref_status)
        pose = history[i, :16].reshape(4, 4)               # the GPU's own bits feed the next comparison
    assert np.array_equal(history[steps - 1, :16], reg.pose.cpu().numpy().ravel())
    assert np.isnan(history[steps:]).all()
    if method == "point":
        assert steps == iterations and status == 0          # point to point does not reach 1e-6 here
    else:
        assert status == 1 and steps < iterations


@pytest.mark.parametrize("n,degrees,cm", [(6000, 3.0, 3.0), (12000, 8.0, 8.0)])
def test_recovery_of_a_known_motion(dev, n, degrees, cm):
    """The restatement converges at tol 1e-6 in 8 and 11 steps and ends 4.4e-4 / 5.4e-4 rad and 4.2e-4 / 1.5e-4 m from
    the true motion (measured on the CPU with normals_ref's normals); the scene's 3 mm noise sets that floor."""
    from detection_3d_amd.register import icp
    p = _pair(dev, n, degrees, cm)
    reg = icp(_gpu(dev, p["source"]), _gpu(dev, p["target"]), max_dist=0.1, iterations=30, tol=1e-6, method="plane")
    ref_pose, ref_steps, ref_status, _ = rr.icp_ref(p["source"], p["target"], p["normals"], None, 0.1, 30, 1e-6, "plane")
    rot, pos = rr.pose_errors(reg.pose.cpu().numpy(), p["truth"], p["centre"])
    ref_rot, ref_pos = rr.pose_errors(ref_pose, p["truth"], p["centre"])
    print(f"n {n}, {degrees} deg / {cm} cm: {reg.steps} steps (reference {ref_steps}), status {reg.status}, rotation {rot:.3g} rad "
          f"(reference {ref_rot:.3g}), centre {pos:.3g} m (reference {ref_pos:.3g}), rmse {reg.rmse:.3g}, pairs {reg.inliers}")
    assert ref_status == 1
    assert reg.status == 1 and reg.converged and reg.steps <= ref_steps + 2
    assert rot <= 2.0 * ref_rot and pos <= 2.0 * ref_pos
    assert np.deg2rad(degrees) > 20 * ref_rot                                      # and that is a recovery


def test_degenerate_systems_leave_the_pose_alone(dev):
    """dense_patch is one plane: with its exact normal at every point the rotation about the normal and the shifts in
    the plane are free, a pivot vanishes.  (The normals estimate_normals finds there from 50 neighbours within 5 mm of
    1 mm noise are far from parallel and would give a system of full rank.)"""
    from detection_3d_amd.register import icp
    tgt, src = dense_patch(2000, 5), dense_patch(1500, 6)
    normal = np.float32([0.3, 0.2, -1.0]) / np.float32(np.sqrt(0.3 * 0.3 + 0.2 * 0.2 + 1.0))
    init = rr.motion_about(tgt.astype(np.float64).mean(0), (0.0, 0.0, 1.0), 0.01, (0.001, 0.0, 0.002))
    reg = icp(_gpu(dev, src), _gpu(dev, tgt), _gpu(dev, np.tile(normal, (2000, 1))), init=torch.from_numpy(init),
              max_dist=0.05, iterations=10, return_details=True)
    ref = rr.step_ref(init, src, tgt, np.tile(normal, (2000, 1)), 0.05, "plane")
    history = reg.history.cpu().numpy()
    print(f"one plane: state {reg.state.cpu().tolist()}, pairs {reg.inliers} (reference {ref['c']}, status {ref['status']})")
    assert ref["status"] == 2 and ref["c"] > 1000
    assert reg.state.cpu().tolist() == [1, 2] and not reg.converged
    assert np.array_equal(reg.pose.cpu().numpy(), init)                            # bit for bit
    assert np.isfinite(history[0]).all() and np.array_equal(history[0, :16], init.ravel())
    assert history[0, 16] == ref["c"] and history[0, 18] == 0 and history[0, 19] == 0
    assert np.isnan(history[1:]).all() and np.isfinite(reg.last_system.cpu().numpy()).all() and np.isfinite(reg.rmse)
    # fewer than 6 pairs
    p = _pair(dev, 6000, 3.0, 3.0)
    for method in ("plane", "point"):
        ref = rr.step_ref(np.eye(4), _scene(6000, 1), p["target"], p["normals"], 0.001, method)
        reg = icp(_gpu(dev, _scene(6000, 1)), _gpu(dev, p["target"]), _gpu(dev, p["normals"]), max_dist=0.001, method=method)
        print(f"{method}, max_dist 1 mm: pairs {ref['c']}, state {reg.state.cpu().tolist()}")
        assert ref["c"] < 6 and ref["status"] == 2
        assert reg.state.cpu().tolist() == [1, 2] and reg.inliers == ref["c"]
        assert np.array_equal(reg.pose.cpu().numpy(), np.eye(4)) and np.isfinite(reg.history[0].cpu().numpy()).all()
    # nothing to pair with at all
    for src, tgt in ((p["source"][:0], p["target"]), (p["source"], p["target"][:0])):
        reg = icp(_gpu(dev, src), _gpu(dev, tgt), method="point", iterations=3)
        assert reg.state.cpu().tolist() == [1, 2] and reg.inliers == 0 and np.isnan(reg.rmse)
        assert np.array_equal(reg.pose.cpu().numpy(), np.eye(4))


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(torch.uint8) == b.contiguous().view(torch.uint8)).all())


def test_two_calls_give_the_same_bits_and_an_early_stop_leaves_the_rest_alone(dev):
    from detection_3d_amd.register import ICP_PHASES, nearest
    p = _pair(dev, 6000, 3.0, 3.0)
    for method in ("plane", "point"):
        a = _icp(dev, p, iterations=12, method=method, return_details=True)
        b = _icp(dev, p, iterations=12, method=method, return_details=True)
        c = _icp(dev, p, iterations=12, method=method, return_details=True, phases=True)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            d = _icp(dev, p, iterations=12, method=method, return_details=True)
        side.synchronize()
        for other in (b, c, d):
            assert _same(a.history, other.history) and _same(a.state, other.state) and _same(a.pose, other.pose)
            assert _same(a.last_index, other.last_index) and _same(a.last_system, other.last_system)
        assert tuple(c.phases) == ICP_PHASES and all(v >= 0.0 for v in c.phases.values()) and c.phases["nearest"] > 0.0
        print(method, a.state.cpu().tolist(), {k: round(v, 3) for k, v in c.phases.items()})
    # the early stop: the plane run converged before its 12 steps
    reg = _icp(dev, p, iterations=12, method="plane")
    history = reg.history.cpu().numpy()
    assert reg.status == 1 and reg.steps < 12
    assert np.isfinite(history[:reg.steps]).all() and np.isnan(history[reg.steps:]).all()
    q, c = _gpu(dev, _scene(6000, 1)), _gpu(dev, _scene(6000, 0))
    i0, d0 = nearest(q, c, 0.1, return_dist2=True)
    i1, d1, ms = nearest(q, c, 0.1, return_dist2=True, phases=True)
    with torch.cuda.stream(side):
        i2, d2 = nearest(q, c, 0.1, return_dist2=True)
    side.synchronize()
    assert _same(i0, i1) and _same(d0, d1) and _same(i0, i2) and _same(d0, d2)
    assert set(ms) == {"cells", "sort", "table", "search", "tail"} and ms["search"] > 0.0


def test_merge_scans_places_three_crops_without_a_doubled_sheet(dev):
    """Three overlapping crops of make_cloud(0), the second and third moved by 2 degrees / 2 cm and -1.5 degrees / 3 cm.
    The reference runs the same chain with icp_ref for the registrations (the down-sampling, the normals and the
    neighbour counts are the package's own, which have their own tests).  On the CPU alone that chain ends 2.3e-3 /
    1.2e-3 rad and 7.5e-4 / 7.2e-4 m from the true motions after 18 and 14 steps, and the mean number of points within
    5 cm in the merged cloud is 1.035 of the unmoved cloud's, against 1.73 for the crops merged as they come."""
    from detection_3d_amd.clean import radius_neighbors
    from detection_3d_amd.downsample import voxel_downsample
    from detection_3d_amd.normals import estimate_normals
    from detection_3d_amd.register import apply_pose, merge_scans
    cloud = _cloud0()
    crops = [cloud[cloud[:, 0] <= SHIFT[0] + 0.8], cloud[cloud[:, 0] >= SHIFT[0] + 0.4], cloud[cloud[:, 1] >= SHIFT[1] + 0.2]]
    centre = cloud[:6000].astype(np.float64).mean(0)
    motions = [np.eye(4), rr.motion_about(centre, AXIS, np.deg2rad(2.0), 0.02 * DIRECTION),
               rr.motion_about(centre, (-0.6, 0.2, 0.5), np.deg2rad(-1.5), 0.03 * np.array([0.5, 1.0, -1.0]) / 1.5)]
    scans = [rr.move(m, c) for m, c in zip(motions, crops)]
    merged, poses = merge_scans([_gpu(dev, s) for s in scans], voxel=0.02, max_dist=0.1, iterations=40)
    assert merged.dtype == torch.float32 and merged.shape[1] == 3 and len(poses) == 3
    assert np.array_equal(poses[0].cpu().numpy(), np.eye(4))

    def mean_count(t):
        return float(radius_neighbors(t, 0.05).double().mean())

    union, ref_errors = _gpu(dev, scans[0]), [None]
    for i in (1, 2):
        model = voxel_downsample(union, 0.02)
        normals = estimate_normals(model, 0.1, 50)
        pose, steps, status, _ = rr.icp_ref(scans[i], model.cpu().numpy(), normals.cpu().numpy(), None, 0.1, 40, 1e-6, "plane")
        assert status == 1
        ref_errors.append(rr.pose_errors(pose, np.linalg.inv(motions[i]), centre))
        union = torch.cat([union, apply_pose(_gpu(dev, scans[i]), torch.from_numpy(pose))])
    plain = mean_count(voxel_downsample(_gpu(dev, np.concatenate(crops)), 0.02))
    ref_ratio = mean_count(voxel_downsample(union, 0.02)) / plain
    doubled = mean_count(voxel_downsample(_gpu(dev, np.concatenate(scans)), 0.02)) / plain
    ratio = mean_count(merged) / plain
    for i in (1, 2):
        rot, pos = rr.pose_errors(poses[i].cpu().numpy(), np.linalg.inv(motions[i]), centre)
        print(f"scan {i}: rotation {rot:.3g} rad (reference {ref_errors[i][0]:.3g}), centre {pos:.3g} m (reference {ref_errors[i][1]:.3g})")
        assert rot <= 2.0 * ref_errors[i][0] and pos <= 2.0 * ref_errors[i][1]
    print(f"mean count within 5 cm over the unmoved cloud's: merged {ratio:.4f}, reference {ref_ratio:.4f}, unregistered {doubled:.4f}")
    assert doubled > 1.5                                   # the statistic does see a doubled sheet
    assert abs(ratio - 1.0) <= 2.0 * abs(ref_ratio - 1.0)  # the poses' margin of 2: the excess grows with the misplacement
