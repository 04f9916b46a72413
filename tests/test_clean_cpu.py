"""detection_3d_amd.clean without a GPU: the keyword checks, the composition of the source maps and the place of the step
in prepare.Preparation with fakes in the kernels' places, and tests/clean_ref.py against a brute-force O(N^2) check."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from detection_3d_amd import clean, prepare
from detection_3d_amd._lib import D3DError
from detection_3d_amd.clean import apply_clean, clean_cloud, clean_kwargs, compose_sources, parse_clean
from detection_3d_amd.prepare import Kept, Preparation
from tests import clean_ref

CFG = SimpleNamespace(SPARSE3D=SimpleNamespace(VOXEL_SCALE=50), INPUT=SimpleNamespace(CLASSES=["wall"]))


def test_clean_kwargs_accepts():
    assert clean_kwargs(None) is None
    assert clean_kwargs({}) == {"radius": 0.1}
    given = {"radius": 0.05, "min_neighbors": 4, "statistical": [20, 2], "min_component": 0.01}
    got = clean_kwargs(given)
    assert got == {"radius": 0.05, "min_neighbors": 4, "statistical": (20, 2.0), "min_component": 0.01}
    assert isinstance(got["statistical"][1], float) and given["statistical"] == [20, 2]        # a checked copy
    assert clean_kwargs({"min_component": 500}) == {"radius": 0.1, "min_component": 500}
    assert clean_kwargs({"min_neighbors": None, "statistical": None}) == {"radius": 0.1}


@pytest.mark.parametrize("bad", [
    "radius", 0.1, [("radius", 0.1)], {"size": 1}, {"radius": 0.0}, {"radius": -1.0}, {"radius": float("inf")},
    {"radius": "wide"}, {"min_neighbors": 0}, {"min_neighbors": 2.5}, {"min_neighbors": True}, {"statistical": 20},
    {"statistical": (20,)}, {"statistical": (0, 2.0)}, {"statistical": (20, -1.0)}, {"statistical": (20, float("nan"))},
    {"statistical": (2.5, 2.0)}, {"min_component": 0}, {"min_component": 1.0}, {"min_component": 0.0},
    {"min_component": 1.5}, {"min_component": "many"}, {"min_component": True},
], ids=repr)
def test_clean_kwargs_rejects(bad):
    with pytest.raises(ValueError):
        clean_kwargs(bad)
    with pytest.raises(ValueError):
        Preparation(clean=bad)


def test_parse_clean():
    assert parse_clean(None) is None and parse_clean("") is None and parse_clean("  ") is None
    assert parse_clean("neighbors=8") == {"radius": 0.1, "min_neighbors": 8}
    assert parse_clean(" radius=0.05, neighbors=4 ,statistical=20:2.5,component=0.01") == {
        "radius": 0.05, "min_neighbors": 4, "statistical": (20, 2.5), "min_component": 0.01}
    assert parse_clean("component=500") == {"radius": 0.1, "min_component": 500}
    for bad in ("neighbors", "neighbors=", "size=3", "neighbors=few", "statistical=20", "statistical=20:x",
                "component=2.0", "radius=0", "neighbors=4,neighbors=5", "neighbors=4;component=3", "neighbors=2.5"):
        with pytest.raises(ValueError):
            parse_clean(bad)


def test_bad_values_raise_before_anything_touches_a_device():
    from detection_3d_amd import engine
    from detection_3d_amd.serving import BuildingPipeline
    for bad in ({"size": 1}, {"min_neighbors": 0}, "estimate"):
        with pytest.raises(ValueError):
            engine.collate([((), {})], None, clean=bad)
        with pytest.raises(ValueError):
            engine.train(None, None, [], None, 1, clean=bad)
        with pytest.raises(ValueError):
            engine.inference(None, None, [], None, clean=bad)
        with pytest.raises(ValueError):
            BuildingPipeline(None, None, device="cpu", clean=bad)
    pcl = torch.zeros((4, 3))
    for kw in ({"radius": 0.0, "min_neighbors": 2}, {"min_neighbors": 0}, {"statistical": (0, 1.0)}, {"min_component": 2.0}):
        with pytest.raises(ValueError):
            clean_cloud(pcl, **kw)


def test_argument_errors_follow_estimate_normals():
    for fn in (clean.radius_outliers, clean.statistical_outliers, clean.connected_components):
        with pytest.raises(D3DError):
            fn(torch.zeros((4, 3)))                                      # a CPU tensor
        with pytest.raises(ValueError):
            fn(torch.zeros((4, 2)))
        with pytest.raises(ValueError):
            fn(torch.zeros((4,)))
        with pytest.raises(ValueError):
            fn(np.zeros((4, 3), np.float32))
    with pytest.raises(D3DError):
        clean_cloud(torch.zeros((4, 3)), min_neighbors=2)


def test_every_option_none_returns_the_input_object():
    pcl = torch.zeros((5, 9))
    assert clean_cloud(pcl) is pcl
    out, source = clean_cloud(pcl, return_source=True)
    assert out is pcl and source is None
    assert apply_clean(pcl, None) is pcl and apply_clean(pcl, None, return_source=True) == (pcl, None)
    assert apply_clean(pcl, clean_kwargs({"radius": 0.2})) is pcl
    assert Preparation(clean={"radius": 0.2}).cloud(pcl)[0] is pcl


def test_compose_sources():
    first = torch.tensor([2, -1, 0, 1, -1], dtype=torch.int32)
    second = torch.tensor([-1, 0, 1], dtype=torch.int32)
    assert compose_sources(None, second) is second and compose_sources(first, None) is first
    got = compose_sources(first, second)
    assert got.dtype == torch.int32 and got.tolist() == [1, -1, -1, 0, -1]
    assert compose_sources(None, None) is None


def _fake_steps(monkeypatch, calls):
    """the three filters replaced by rules on column 0, which holds each row's own number"""
    def radius_outliers(xyz, radius, min_neighbors):
        calls.append(("radius", xyz[:, 0].tolist(), radius, min_neighbors))
        return xyz[:, 0] % 2 == 0                                        # even rows stay

    def statistical_outliers(xyz, k, std_ratio, radius):
        calls.append(("statistical", xyz[:, 0].tolist(), k, std_ratio, radius))
        return xyz[:, 0] != 4                                            # row 4 goes

    def connected_components(xyz, radius):
        calls.append(("components", xyz[:, 0].tolist(), radius))
        size = torch.where(xyz[:, 0] >= 8, 1, 3).to(torch.int32)         # rows 8 and up: components of one point
        return torch.zeros_like(size), size

    monkeypatch.setattr(clean, "radius_outliers", radius_outliers)
    monkeypatch.setattr(clean, "statistical_outliers", statistical_outliers)
    monkeypatch.setattr(clean, "connected_components", connected_components)


def test_steps_run_in_order_on_the_survivors_and_the_source_maps_compose(monkeypatch):
    calls = []
    _fake_steps(monkeypatch, calls)
    pcl = torch.arange(12, dtype=torch.float32)[:, None].repeat(1, 9)
    pcl[:, 1:] += torch.arange(1, 9, dtype=torch.float32) * 100
    out, source = clean_cloud(pcl, radius=0.2, min_neighbors=3, statistical=(5, 1.5), min_component=2, return_source=True)
    assert calls == [("radius", [float(i) for i in range(12)], 0.2, 3),
                     ("statistical", [0.0, 2.0, 4.0, 6.0, 8.0, 10.0], 5, 1.5, 0.2),
                     ("components", [0.0, 2.0, 6.0, 8.0, 10.0], 0.2)]
    assert out[:, 0].tolist() == [0.0, 2.0, 6.0] and torch.equal(out, pcl[[0, 2, 6]])        # order and every column
    assert source.dtype == torch.int32 and source.tolist() == [0, -1, 1, -1, -1, -1, 2, -1, -1, -1, -1, -1]
    assert torch.equal(clean_cloud(pcl, radius=0.2, min_neighbors=3, statistical=(5, 1.5), min_component=2), out)
    # a share of the rows given to the step: 11 rows, 0.25 -> 2.75 points, so the components of 3 stay
    del calls[:]
    out = clean_cloud(pcl, min_component=0.25, statistical=(5, 1.5))
    assert [c[0] for c in calls] == ["statistical", "components"] and out[:, 0].tolist() == [0, 1, 2, 3, 5, 6, 7]
    out = clean_cloud(pcl[:10], min_component=0.25)                      # 10 rows -> 2.5 points again
    assert out[:, 0].tolist() == [0, 1, 2, 3, 4, 5, 6, 7]
    out = clean_cloud(pcl[:10], min_component=0.35)                      # 3.5 points: nothing is large enough
    assert out.shape == (0, 9)


def _recording_chain(monkeypatch, calls, **kw):
    def fake_downsample(pcl, dkw, return_source=False):
        if dkw is None:
            return (pcl, None) if return_source else pcl
        calls.append(("downsample", pcl.shape[0], return_source))
        source = torch.tensor([0, 0, 1, 2, 3, -1], dtype=torch.int32)
        return (pcl[:4], source) if return_source else pcl[:4]

    def fake_clean(pcl, ckw, return_source=False):
        if ckw is None:
            return (pcl, None) if return_source else pcl
        calls.append(("clean", pcl.shape[0], ckw, return_source))
        source = torch.arange(pcl.shape[0], dtype=torch.int32) - 1       # the first row goes
        return (pcl[1:], source) if return_source else pcl[1:]

    def fake_estimator(xyz, radius, max_nn, orient):
        calls.append(("normals", xyz.shape[0]))
        return torch.ones((xyz.shape[0], 3))

    def fake_voxelize(pcl, cfg):
        calls.append(("voxelize", tuple(pcl.shape)))
        return "coords", "feats"

    def fake_shift(pcl, tg, scale):
        calls.append(("shift_targets", tuple(pcl.shape), scale))
        return dict(tg, shifted=True)

    monkeypatch.setattr(prepare, "apply_downsample", fake_downsample)
    monkeypatch.setattr(prepare, "apply_clean", fake_clean)
    monkeypatch.setattr(prepare, "shift_targets", fake_shift)
    chain = Preparation(voxelize_fn=fake_voxelize, **kw)
    if chain.normals is not None:
        chain.normals["estimator"] = fake_estimator
    return chain


def test_preparation_cleans_after_the_downsampling_and_before_the_normals(monkeypatch):
    calls = []
    ckw = {"radius": 0.1, "min_neighbors": 8}
    chain = _recording_chain(monkeypatch, calls, downsample=0.05, clean={"min_neighbors": 8}, normals="estimate")
    assert chain.clean == ckw
    raw = torch.zeros((6, 3))
    cloud, kept = chain.cloud(raw)
    assert calls == [("downsample", 6, False), ("clean", 4, ckw, False), ("normals", 3)] and kept is None
    assert cloud.shape == (3, 9)
    del calls[:]
    cloud, kept = chain.cloud(raw, keep=True)
    assert calls == [("downsample", 6, True), ("clean", 4, ckw, True), ("normals", 3)]
    # raw rows 0, 1 went into down-sampled row 0, which was cleaned away; raw row 5 had been dropped before
    assert kept.source.dtype == torch.int32 and kept.source.tolist() == [-1, -1, 0, 1, 2, -1]
    assert kept.cloud.shape == (3, 3) and kept.pixels is None and cloud.shape == (3, 9)
    del calls[:]
    _, _, tg = chain.scene(raw, {"bbox3d": "b"}, CFG)
    assert [c[0] for c in calls] == ["downsample", "clean", "normals", "voxelize", "shift_targets"]
    assert tg == {"bbox3d": "b", "shifted": True} and calls[-1] == ("shift_targets", (3, 9), 50)


def test_clean_alone_keeps_its_own_source_and_moves_the_frame(monkeypatch):
    calls = []
    chain = _recording_chain(monkeypatch, calls, clean={"min_component": 100})
    raw = torch.zeros((6, 3))
    cloud, kept = chain.cloud(raw, keep=True)
    assert [c[0] for c in calls] == ["clean"] and cloud.shape == (5, 3)
    assert kept == Kept(cloud, kept.source, None) and kept.source.tolist() == [-1, 0, 1, 2, 3, 4]
    del calls[:]
    _, _, tg = chain.scene(raw, {"bbox3d": "b"}, CFG)
    assert [c[0] for c in calls] == ["clean", "voxelize", "shift_targets"] and tg["shifted"]


def test_targets_in_file_frame_with_clean_alone():
    assert Preparation(clean={"min_neighbors": 8}).targets_in_file_frame
    assert Preparation(clean={"min_neighbors": 8}, normals="estimate").targets_in_file_frame
    assert not Preparation(normals="estimate").targets_in_file_frame and not Preparation().targets_in_file_frame
    rank = Preparation(clean={"min_neighbors": 8}).for_rank(3, ["wall"])
    assert rank.clean == {"radius": 0.1, "min_neighbors": 8}


def test_train_ddp_clean_option():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_ddp_clean_under_test", os.path.join(root, "scripts", "train_ddp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_args([]).clean is None
    got = mod.parse_args(["--clean", "neighbors=8,component=0.01"]).clean
    assert got == {"radius": 0.1, "min_neighbors": 8, "min_component": 0.01}
    with pytest.raises(ValueError):
        mod.parse_args(["--clean", "neighbours=8"])


# ---- the reference against brute force ----
def _brute(xyz, radius):
    p = xyz.astype(np.float64)
    r = float(np.float32(radius))
    q = p[:, None, :] - p[None, :, :]
    return (q * q).sum(2), r * r


def _cloud300():
    rs = np.random.RandomState(7)
    a = rs.rand(200, 3) * np.array([1.0, 0.8, 0.1])
    b = rs.rand(80, 3) * 0.15 + np.array([3.0, 0.0, 0.0])                # a detached clump
    c = rs.rand(20, 3) * 6.0 + np.array([0.0, 5.0, 0.0])                 # strays
    return np.concatenate([a, b, c]).astype(np.float32)


@pytest.mark.parametrize("radius", [0.1, 0.2])
def test_reference_counts_and_means_against_brute_force(radius):
    xyz = _cloud300()
    d2, r2 = _brute(xyz, radius)
    count, lo, hi, edge = clean_ref.neighbors_ref(xyz, radius)
    assert np.array_equal(count, (d2 <= r2).sum(1))
    assert (lo <= count).all() and (count <= hi).all() and np.array_equal(edge, lo != hi)
    assert count.min() == 1 and count.max() > 12
    k = 6
    mean, found, _ = clean_ref.knn_ref(xyz, k, radius)
    n = xyz.shape[0]
    want_mean, want_found = np.full(n, np.inf), np.zeros(n, np.int32)
    for i in range(n):
        order = sorted((d2[i, j], j) for j in range(n) if d2[i, j] <= r2)[:k + 1]
        want_found[i] = len(order) - 1
        if want_found[i] >= k:
            want_mean[i] = sum(np.sqrt(d) for d, _ in order) / k
    assert np.array_equal(found, want_found) and (found < k).any() and (found == k).any()
    assert np.array_equal(np.isfinite(mean), np.isfinite(want_mean))
    fin = np.isfinite(mean)
    assert np.abs(mean[fin] - want_mean[fin]).max() <= 1e-14
    mu, sigma = clean_ref.stats_ref(mean)
    assert abs(mu - want_mean[fin].mean()) <= 1e-15 and abs(sigma - want_mean[fin].std(ddof=1)) <= 1e-15
    assert clean_ref.stats_ref(np.array([np.inf, np.inf])) == (0.0, 0.0) and clean_ref.stats_ref(np.array([2.0])) == (2.0, 0.0)


@pytest.mark.parametrize("radius", [0.1, 0.2])
def test_reference_components_against_brute_force(radius):
    xyz = _cloud300()
    d2, r2 = _brute(xyz, radius)
    n = xyz.shape[0]
    label = np.arange(n)
    changed = True
    while changed:                                                       # labels flow along the edges until they settle
        new = np.where(d2 <= r2, label[None, :], n).min(1)
        changed = not np.array_equal(new, label)
        label = new
    size = np.bincount(label, minlength=n)[label]
    (l0, s0), (l1, s1) = clean_ref.components_ref(xyz, radius)
    assert np.array_equal(l0, l1) and np.array_equal(s0, s1)
    assert np.array_equal(l0, label) and np.array_equal(s0, size)
    assert 3 <= np.unique(label).size < n and size.max() >= 80


def test_reference_clouds_are_what_the_gpu_tests_count_on():
    chains = clean_ref.make_chains(0.1)
    (l0, s0), (l1, s1) = clean_ref.components_ref(chains, 0.1)
    assert np.array_equal(l0, l1) and np.unique(l0).size == 2 and (s0 == 3000).all()
    (l0, s0), (l1, s1) = clean_ref.components_ref(chains, 0.05)
    assert np.array_equal(l0, l1) and np.array_equal(l0, np.arange(6000)) and (s0 == 1).all()
