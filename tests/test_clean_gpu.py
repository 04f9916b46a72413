"""detection_3d_amd.clean (clean.hip) against the fp64 restatement of its semantics in tests/clean_ref.py, and its place in
prepare.Preparation and serving.BuildingPipeline.

Bounds.  Counts, `found`, labels and sizes are integers and must be equal wherever fp32 and fp64 cannot pick different
sets: away from the reference's edge flags (a candidate within 1e-5 r^2 of r^2; a tie at the k-nearest cut).  A mean
distance is within 1e-6 relative: an fp32 d2 of an exact offset is off by at most 1.8e-7 d2 (normals_ref), its root by
half of that, and the fp64 sum of at most k + 1 roots adds nothing that shows: a margin of about 5 (10 for the root).
mu and sigma are fp64 sums of the same means: 1e-6 relative too.  The points excused from a keep comparison are at most
1 % of a cloud, and the share is asserted."""
import numpy as np
import pytest
import torch

from tests import clean_ref
from tests.normals_ref import dense_patch

pytestmark = pytest.mark.gpu

_REF = {}


def _cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _cloud(name):
    """the clouds of the tests by name -> fp32 [N, 3]"""
    def make():
        if name[0] == "scene":
            return clean_ref.make_cloud(name[1])
        if name[0] == "chains":
            return clean_ref.make_chains(0.1)
        if name[0] == "dense":
            return dense_patch(2000, 5)
        if name[0] == "twice":                                           # every point duplicated once
            a = clean_ref.make_cloud(0)
            return np.concatenate([a, a[np.random.RandomState(3).permutation(a.shape[0])]])
        if name[0] == "far":                                             # one point 1 km away
            return np.concatenate([clean_ref.make_cloud(0), np.float32([[1013.7, -4.2, 1.1]])])
        raise KeyError(name)
    return _cached(("cloud",) + name, make)


def _neighbors(name, radius):
    return _cached(("nb", name, radius), lambda: clean_ref.neighbors_ref(_cloud(name), radius))


def _knn(name, k, radius):
    return _cached(("knn", name, k, radius), lambda: clean_ref.knn_ref(_cloud(name), k, radius))


def _components(name, radius):
    return _cached(("cc", name, radius), lambda: clean_ref.components_ref(_cloud(name), radius))


def _gpu(dev, xyz):
    return torch.from_numpy(np.ascontiguousarray(xyz)).to(dev)


# ---- counts ----
def _check_counts(dev, name, radius, what):
    from detection_3d_amd.clean import radius_outliers
    xyz = _cloud(name)
    ref_c, lo, hi, edge = _neighbors(name, radius)
    n = xyz.shape[0]
    for min_neighbors in (2, 8, 30):
        keep, count = radius_outliers(_gpu(dev, xyz), radius, min_neighbors, return_counts=True)
        assert keep.dtype == torch.bool and count.dtype == torch.int32 and keep.shape == count.shape == (n,)
        keep, count = keep.cpu().numpy(), count.cpu().numpy()
        bad = np.flatnonzero((count != ref_c) & ~edge)
        excused = (lo < min_neighbors) & (min_neighbors <= hi)
        print(f"{what} r {radius} min_neighbors {min_neighbors}: {n} points, max count {ref_c.max()}, edge {int(edge.sum())}, "
              f"count mismatches {bad.size}, excused {int(excused.sum())}, kept {int(keep.sum())}")
        assert bad.size == 0, (what, bad[:10], count[bad[:10]], ref_c[bad[:10]])
        assert ((lo <= count) & (count <= hi)).all()                     # an edge point: between the two counts
        assert excused.sum() <= 0.01 * n, (what, int(excused.sum()), n)
        assert np.array_equal(keep[~excused], (ref_c >= min_neighbors)[~excused]), what
    return ref_c


@pytest.mark.parametrize("seed,radius", [(0, 0.05), (0, 0.1), (1, 0.1)])
def test_counts_and_radius_outliers_on_the_scenes(dev, seed, radius):
    ref_c = _check_counts(dev, ("scene", seed), radius, f"scene {seed}")
    assert ref_c.max() > 1024 and (ref_c == 1).sum() >= 10              # the unstaged form and the isolated points are there


# ---- statistical ----
def _check_statistical(dev, name, k, radius, std_ratio, what):
    from detection_3d_amd.clean import knn_mean_distance, statistical_outliers
    xyz = _cloud(name)
    ref_mean, ref_found, edge = _knn(name, k, radius)
    n = xyz.shape[0]
    keep, mean, stats = statistical_outliers(_gpu(dev, xyz), k, std_ratio, radius, return_stats=True)
    _, found, _, _ = knn_mean_distance(_gpu(dev, xyz), k, std_ratio, radius)
    assert keep.dtype == torch.bool and mean.dtype == torch.float64 and stats.dtype == torch.float64
    assert stats.shape == (2,) and stats.is_cuda and found.dtype == torch.int32
    keep, mean, found, (mu, sigma) = keep.cpu().numpy(), mean.cpu().numpy(), found.cpu().numpy(), stats.cpu().numpy()
    ok = ~edge
    bad = np.flatnonzero((found != ref_found) & ok)
    assert bad.size == 0, (what, bad[:10], found[bad[:10]], ref_found[bad[:10]])
    sparse = ref_found < k
    assert np.array_equal(np.isinf(mean[ok]), sparse[ok]) and (mean[ok & sparse] > 0).all()
    fin = ok & ~sparse
    rel = np.abs(mean[fin] - ref_mean[fin]) / ref_mean[fin]
    ref_mu, ref_sigma = clean_ref.stats_ref(ref_mean)
    thr = ref_mu + std_ratio * ref_sigma
    near = np.isfinite(ref_mean) & (np.abs(ref_mean - thr) <= 1e-6 * thr)
    excused = edge | near
    print(f"{what} k {k} r {radius}: {n} points, sparse {int(sparse.sum())}, edge {int(edge.sum())}, near the threshold "
          f"{int(near.sum())}, max relative error of a mean {rel.max():.3e} (bound 1e-6), mu {mu:.9e} (ref {ref_mu:.9e}), "
          f"sigma {sigma:.9e} (ref {ref_sigma:.9e}), kept {int(keep.sum())}")
    assert rel.max() <= 1e-6, (what, rel.max())
    assert abs(mu - ref_mu) <= 1e-6 * ref_mu and abs(sigma - ref_sigma) <= 1e-6 * ref_sigma, (what, mu, ref_mu, sigma, ref_sigma)
    assert excused.sum() <= 0.01 * n, (what, int(excused.sum()), n)
    want = ~sparse & (ref_mean <= thr)
    assert np.array_equal(keep[~excused], want[~excused]), what
    # the sparse points are dropped and enter neither mu nor sigma: the finite means of this run alone give them back
    assert not keep[ok & sparse].any() and sparse.any()
    own_mu, own_sigma = clean_ref.stats_ref(mean)
    assert abs(mu - own_mu) <= 1e-12 * own_mu and abs(sigma - own_sigma) <= 1e-9 * own_sigma
    assert want.sum() < (~sparse).sum()                                  # the filter has something to drop


@pytest.mark.parametrize("k,radius,std_ratio", [(20, 0.1, 1.0), (8, 0.05, 0.5)])
def test_statistical_outliers_on_a_scene(dev, k, radius, std_ratio):
    _check_statistical(dev, ("scene", 0), k, radius, std_ratio, "scene 0")


# ---- components ----
def _check_components(dev, name, radius, what):
    from detection_3d_amd.clean import connected_components
    (l0, s0), (l1, s1) = _components(name, radius)
    assert np.array_equal(l0, l1) and np.array_equal(s0, s1), f"{what}: the reference's two labellings differ"
    label, size = connected_components(_gpu(dev, _cloud(name)), radius)
    assert label.dtype == torch.int32 and size.dtype == torch.int32
    label, size = label.cpu().numpy(), size.cpu().numpy()
    print(f"{what} r {radius}: {l0.shape[0]} points, {np.unique(l0).size} components, largest {s0.max()}, "
          f"label mismatches {int((label != l0).sum())}, size mismatches {int((size != s0).sum())}")
    assert np.array_equal(label, l0) and np.array_equal(size, s0), what
    return l0, s0


@pytest.mark.parametrize("radius", [0.05, 0.1])
def test_components_of_a_scene(dev, radius):
    l0, _ = _check_components(dev, ("scene", 0), radius, "scene 0")
    assert 16 <= np.unique(l0).size <= 22


def test_components_of_the_chains(dev):
    l0, s0 = _check_components(dev, ("chains",), 0.1, "chains")           # two unions, each 3000 deep
    assert np.unique(l0).size == 2 and (s0 == 3000).all()
    l0, s0 = _check_components(dev, ("chains",), 0.05, "chains")
    assert np.array_equal(l0, np.arange(6000)) and (s0 == 1).all()


def test_components_with_duplicates_and_a_point_far_away(dev):
    l0, s0 = _check_components(dev, ("twice",), 0.1, "every point twice")
    assert s0.min() == 2
    l0, s0 = _check_components(dev, ("far",), 0.1, "one point 1 km away")
    assert l0[-1] == l0.shape[0] - 1 and s0[-1] == 1


# ---- both forms of the walk, bit stability, strides ----
def test_the_unstaged_form_alone(dev):
    """2000 points in a 5 cm cube: every neighbourhood is past the staging budget"""
    ref_c = _check_counts(dev, ("dense",), 0.1, "dense patch")
    assert ref_c.min() > 1024
    _check_components(dev, ("dense",), 0.1, "dense patch")
    from detection_3d_amd.clean import knn_mean_distance
    ref_mean, ref_found, edge = _knn(("dense",), 20, 0.1)
    mean, found, stats, _ = knn_mean_distance(_gpu(dev, _cloud(("dense",))), 20, 2.0, 0.1)
    mean, found = mean.cpu().numpy(), found.cpu().numpy()
    assert edge.sum() <= 30 and np.array_equal(found[~edge], ref_found[~edge]) and (ref_found == 20).all()
    rel = np.abs(mean - ref_mean)[~edge] / ref_mean[~edge]
    print(f"dense patch: edge {int(edge.sum())}, max relative error of a mean {rel.max():.3e} (bound 1e-6)")
    assert rel.max() <= 1e-6
    ref_mu, ref_sigma = clean_ref.stats_ref(ref_mean)
    mu, sigma = stats.cpu().numpy()
    assert abs(mu - ref_mu) <= 1e-6 * ref_mu and abs(sigma - ref_sigma) <= 1e-6 * ref_sigma


def _all_outputs(xyz):
    from detection_3d_amd.clean import connected_components, knn_mean_distance, radius_outliers
    return radius_outliers(xyz, 0.1, 8, return_counts=True) + knn_mean_distance(xyz, 20, 2.0, 0.1) + \
        connected_components(xyz, 0.1)


def _same_bits(a, b):
    def bits(t):
        return t.view(torch.int64) if t.dtype == torch.float64 else t
    return all(x.dtype == y.dtype and torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_two_runs_and_a_strided_view_give_the_same_bits(dev):
    xyz = _gpu(dev, _cloud(("scene", 1)))
    first = _all_outputs(xyz)
    assert len(first) == 8 and _same_bits(first, _all_outputs(xyz))
    pcl9 = torch.cat([xyz, torch.rand((xyz.shape[0], 6), device=dev)], 1)
    assert not pcl9[:, :3].is_contiguous() and _same_bits(first, _all_outputs(pcl9[:, :3]))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        on_side = _all_outputs(pcl9[:, :3])
    side.synchronize()
    assert _same_bits(first, on_side)


# ---- edge sizes ----
def test_edge_sizes(dev):
    from detection_3d_amd.clean import (clean_cloud, connected_components, knn_mean_distance, radius_outliers,
                                        statistical_outliers)
    empty = torch.zeros((0, 3), device=dev)
    keep, count = radius_outliers(empty, return_counts=True)
    assert keep.shape == count.shape == (0,) and keep.dtype == torch.bool
    keep, mean, stats = statistical_outliers(empty, return_stats=True)
    assert keep.shape == mean.shape == (0,) and stats.tolist() == [0.0, 0.0]
    label, size = connected_components(empty)
    assert label.shape == size.shape == (0,) and label.dtype == torch.int32
    out, source = clean_cloud(torch.zeros((0, 9), device=dev), min_neighbors=2, statistical=(3, 1.0), min_component=2,
                              return_source=True)
    assert out.shape == (0, 9) and source.shape == (0,) and source.dtype == torch.int32
    one = torch.tensor([[1.0, 2.0, 3.0]], device=dev)
    keep, count = radius_outliers(one, 0.1, 1, return_counts=True)
    assert keep.tolist() == [True] and count.tolist() == [1]
    mean, found, stats, keep = knn_mean_distance(one, 1, 2.0, 0.1)
    assert found.tolist() == [0] and torch.isinf(mean).all() and keep.tolist() == [False] and stats.tolist() == [0.0, 0.0]
    label, size = connected_components(one)
    assert label.tolist() == [0] and size.tolist() == [1]
    # two points at distance exactly r: 0.25 is a float, its square too, and so is the offset
    two = torch.tensor([[1.0, 2.0, 3.0], [1.25, 2.0, 3.0]], device=dev)
    keep, count = radius_outliers(two, 0.25, 2, return_counts=True)
    assert keep.tolist() == [True, True] and count.tolist() == [2, 2]
    label, size = connected_components(two, 0.25)
    assert label.tolist() == [0, 0] and size.tolist() == [2, 2]
    mean, found, stats, keep = knn_mean_distance(two, 1, 2.0, 0.25)
    assert found.tolist() == [1, 1] and mean.tolist() == [0.25, 0.25] and stats.tolist() == [0.25, 0.0]
    assert keep.tolist() == [True, True]
    assert radius_outliers(two, 0.2499, 2).tolist() == [False, False]
    assert connected_components(two, 0.2499)[0].tolist() == [0, 1]


# ---- clean_cloud ----
def test_clean_cloud_is_the_three_steps_by_hand(dev):
    from detection_3d_amd.clean import clean_cloud, connected_components, radius_outliers, statistical_outliers
    xyz = _gpu(dev, _cloud(("scene", 0)))
    n = xyz.shape[0]
    pcl = torch.cat([xyz, torch.arange(n * 6, dtype=torch.float32, device=dev).reshape(n, 6)], 1)
    k1 = radius_outliers(pcl[:, :3], 0.1, 8)
    a = pcl[k1]
    k2 = statistical_outliers(a[:, :3], 20, 1.0, 0.1)
    b = a[k2]
    _, size = connected_components(b[:, :3], 0.1)
    k3 = size >= 0.05 * b.shape[0]
    want = b[k3]
    rows = torch.arange(n, device=dev)[k1][k2][k3]
    out, source = clean_cloud(pcl, 0.1, min_neighbors=8, statistical=(20, 1.0), min_component=0.05, return_source=True)
    print(f"clean_cloud: {n} -> {int(k1.sum())} -> {int(k2.sum())} -> {int(k3.sum())} rows")
    assert 0 < want.shape[0] < b.shape[0] < a.shape[0] < n               # every step drops something
    assert out.shape == want.shape and torch.equal(out, want) and torch.equal(out, pcl[rows])    # order, all nine columns
    assert torch.equal(clean_cloud(pcl, 0.1, min_neighbors=8, statistical=(20, 1.0), min_component=0.05), want)
    assert source.dtype == torch.int32 and source.shape == (n,)
    kept = source >= 0
    assert int(kept.sum()) == out.shape[0] and torch.equal(torch.nonzero(kept)[:, 0], rows)
    assert torch.equal(out[source[kept].long()], pcl[kept])
    assert torch.equal(source[kept], torch.arange(out.shape[0], dtype=torch.int32, device=dev))
    # a number of points in place of a share, and a step alone
    assert torch.equal(clean_cloud(b, 0.1, min_component=int(np.ceil(0.05 * b.shape[0]))), want)
    assert torch.equal(clean_cloud(pcl, 0.1, min_neighbors=8), a)


# ---- the point of it all ----
BUILDING_CLEAN = {"radius": 0.2, "min_neighbors": 10, "min_component": 0.05}


def _building():
    """a synthetic building of 20 000 points on 4 x 3 x 2.7 m (about 20 neighbours within 0.2 m), 40 points in a 0.3 m
    blob 300 m away and 200 stray points; -> (dirty fp32 [20240, 9], number of building rows)"""
    def make():
        from detection_3d_amd.synthetic import make_scene
        house = make_scene(3, 20000, extent=(4.0, 3.0, 2.7))
        rs = np.random.RandomState(11)
        extra = np.zeros((240, 9), np.float32)
        extra[:40, :3] = rs.rand(40, 3) * 0.3 + np.array([-300.0, 1.0, 0.5])
        extra[40:, :3] = rs.rand(200, 3) * np.array([60.0, 60.0, 9.0]) + np.array([-80.0, -80.0, -3.0])
        extra[:, 8] = 1.0
        return np.concatenate([house, extra]).astype(np.float32), house.shape[0]
    return _cached(("building",), make)


def _building_ref_keep():
    """the reference's keep mask of the dirty building under BUILDING_CLEAN, and the rows it cannot decide"""
    def make():
        dirty, _ = _building()
        r, m = BUILDING_CLEAN["radius"], BUILDING_CLEAN["min_neighbors"]
        count, lo, hi, _ = clean_ref.neighbors_ref(dirty, r)
        k1 = count >= m
        undecided = (lo < m) & (m <= hi)
        (l0, s0), (l1, s1) = clean_ref.components_ref(dirty[k1], r)
        assert np.array_equal(l0, l1) and np.array_equal(s0, s1)
        keep = k1.copy()
        keep[k1] = s0 >= BUILDING_CLEAN["min_component"] * k1.sum()
        return keep, undecided
    return _cached(("building keep",), make)


def test_a_cleaned_building_is_voxelised_as_if_it_had_been_alone(dev):
    from detection_3d_amd.clean import clean_cloud
    from detection_3d_amd.voxelize import voxelize
    dirty, nb = _building()
    keep, undecided = _building_ref_keep()
    pcl = _gpu(dev, dirty)
    out, source = clean_cloud(pcl, return_source=True, **BUILDING_CLEAN)
    got = (source >= 0).cpu().numpy()
    differ = int((got != keep).sum())
    print(f"building: {nb} rows + 240, reference keeps {int(keep.sum())}, drops {int((~keep[:nb]).sum())} at the rim, "
          f"undecided {int(undecided.sum())}, kept differently {differ}")
    assert not keep[nb:].any() and not got[nb:].any()                    # the blob and the strays are gone
    assert keep[:nb].sum() > 0.9 * nb                                    # ... and the building is not
    assert differ <= undecided.sum() and differ == int((got != keep)[undecided].sum())
    # with clean: the voxels of the building's kept rows alone
    coords, feats = voxelize(out)
    alone = pcl[:nb][torch.from_numpy(got[:nb]).to(dev)]
    want_coords, want_feats = voxelize(alone)
    assert coords.shape[0] == out.shape[0] == int(got.sum())             # nothing falls out of the lattice
    assert torch.equal(coords, want_coords) and torch.equal(feats, want_feats)
    assert int(coords.max()) < 4.0 * 50 + 1
    # without: the origin is 300 m away and the building leaves the 4096 x 4096 x 512 lattice of 2 cm voxels
    dirty_coords, _ = voxelize(pcl)
    dropped = dirty.shape[0] - dirty_coords.shape[0]
    print(f"without clean: {dropped} of {dirty.shape[0]} rows leave the lattice")
    assert dropped >= nb


# ---- the chain ----
def test_preparation_is_the_three_steps_by_hand(dev):
    from detection_3d_amd.clean import clean_cloud
    from detection_3d_amd.downsample import voxel_downsample
    from detection_3d_amd.normals import with_normals
    from detection_3d_amd.prepare import Preparation
    dirty, nb = _building()
    pcl = _gpu(dev, dirty)
    chain = Preparation(downsample=0.03, clean=BUILDING_CLEAN, normals={"radius": 0.2})
    got, none = chain.cloud(pcl)
    down, inverse = voxel_downsample(pcl, 0.03, return_inverse=True)
    cleaned, source = clean_cloud(down, return_source=True, **BUILDING_CLEAN)
    want = with_normals(cleaned, radius=0.2)
    assert none is None and 0 < cleaned.shape[0] < down.shape[0] < pcl.shape[0]
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))
    got_kept, kept = chain.cloud(pcl, keep=True)
    assert torch.equal(got_kept.view(torch.int32), want.view(torch.int32)) and torch.equal(kept.cloud, cleaned)
    assert kept.source.dtype == torch.int32 and torch.equal(kept.source, source[inverse.long()])
    assert (kept.source[nb:] == -1).all() and (kept.source[:nb] >= 0).float().mean() > 0.9


def test_pipeline_point_owner_is_minus_one_for_cleaned_rows(dev):
    from detection_3d_amd.clean import clean_cloud
    from detection_3d_amd.config import get_cfg
    from detection_3d_amd.detector import build_detection_model
    from detection_3d_amd.serving import BuildingPipeline
    cfg = get_cfg("4c_Fpn432")
    torch.manual_seed(1)
    model = build_detection_model(cfg).to(dev).eval()
    with torch.no_grad():                                                # the weights of tests/test_detector_gpu.py
        model.rpn.head.cls_logits.weight.mul_(60)
        model.rpn.head.bbox_pred.weight.mul_(20)
        model.roi_heads.box.predictor.cls_score.weight.mul_(40)
        model.roi_heads.box.predictor.bbox_pred.weight.mul_(100)
    dirty, nb = _building()
    pcl = _gpu(dev, dirty)
    cleaned, source = clean_cloud(pcl, return_source=True, **BUILDING_CLEAN)
    with torch.no_grad():
        got = BuildingPipeline(model, cfg, in_flight=2, device=dev, point_owner=True, clean=BUILDING_CLEAN).map([pcl])[0]
        want = BuildingPipeline(model, cfg, in_flight=2, device=dev, point_owner=True).map([cleaned])[0]
    torch.cuda.synchronize()
    for k in ("bbox3d", "scores", "labels", "point_count"):
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    owner = got["point_owner"]
    assert owner.dtype == torch.int32 and owner.shape == (pcl.shape[0],)
    dropped = source < 0
    assert (owner[dropped] == -1).all() and dropped[nb:].all() and int(dropped.sum()) > 240
    assert torch.equal(owner[~dropped], want["point_owner"][source[~dropped].long()])
    print(f"pipeline: {got['bbox3d'].shape[0]} detections, {int((owner >= 0).sum())} owned rows, {int(dropped.sum())} cleaned away")
