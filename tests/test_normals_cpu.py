"""The normals reference (tests/normals_ref.py) on cases with known answers, and the host side of
detection_3d_amd.normals: column handling, argument checks, the command-line flag."""
import os
import sys

import numpy as np
import pytest
import torch

from tests.normals_ref import canonical_sign, make_scene, normals_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plane(normal, n=400, seed=0):
    """noise-free points, exact in fp32 (multiples of 2^-12 below 4), on a plane with that normal: an axis plane at 1.0,
    or z = 0.5 x - 0.25 y for the tilted normal (-0.5, 0.25, 1)"""
    rs = np.random.RandomState(seed)
    uv = rs.randint(0, 600, (n, 2)) / 1024.0
    k = [i for i in range(3) if normal[i] != 0]
    if len(k) == 1:
        pts = np.ones((n, 3))
        pts[:, [i for i in range(3) if i != k[0]]] = 1.0 + uv
    else:
        pts = np.stack([uv[:, 0], uv[:, 1], 0.5 * uv[:, 0] - 0.25 * uv[:, 1]], 1)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
    return pts.astype(np.float32), np.asarray(normal, np.float64) / np.linalg.norm(normal)


@pytest.mark.parametrize("normal", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (-0.5, 0.25, 1)])
def test_reference_finds_the_normal_of_a_plane(normal):
    pts, nrm = _plane(normal)
    got, counts, gap, _ = normals_ref(pts, radius=0.1, max_nn=50)
    use = counts >= 3
    use &= np.isfinite(gap) & (gap > 1e-2)            # three collinear grid points have no normal
    assert use.sum() > 300
    assert np.abs(got[use] - canonical_sign(nrm)[None, :]).max() <= 1e-12


def test_reference_sign_and_degenerate_cases():
    got, counts, gap, _ = normals_ref(np.float32([[0, 0, 0], [0.05, 0, 0]]))
    assert counts.tolist() == [2, 2] and np.array_equal(got, [[0, 0, 1], [0, 0, 1]]) and np.isinf(gap).all()
    got, counts, _, _ = normals_ref(np.zeros((10, 3), np.float32), max_nn=4)
    assert counts.tolist() == [4] * 10 and np.array_equal(got, np.tile([0.0, 0, 1], (10, 1)))
    pts, nrm = _plane((0, 0, -1))
    got, counts, gap, _ = normals_ref(pts)
    use = (counts >= 3) & (gap > 1e-2)
    assert (got[use, 2] > 0).all()                                      # largest component positive
    got = normals_ref(pts, orient=(1.0, 2.0, -5.0))[0]
    assert (got[use, 2] < 0).all()                                      # facing a viewpoint below the plane
    assert np.array_equal(canonical_sign(np.array([[-0.6, 0.6, 0.5], [0.6, -0.6, 0.5]])),
                          [[0.6, -0.6, -0.5], [0.6, -0.6, 0.5]])       # ties: the lowest axis decides


def test_reference_cuts_by_distance_then_index():
    """a query at the origin, four points at distance 0.05 exactly (tied), one nearer, one farther: max_nn = 4 keeps the
    query, the nearer one and the two tied points of lowest index"""
    pts = np.float32([[0, 0, 0], [0, 0.05, 0], [0.05, 0, 0], [0.09, 0, 0], [-0.05, 0, 0], [0, 0, 0.03], [0, -0.05, 0]])
    got, counts, _, edge = normals_ref(pts, radius=0.1, max_nn=4)
    assert counts[0] == 4 and edge[0]                                   # tied at the cut: flagged
    # kept: 0 (d2 = 0), 5 (0.03), then 1 and 2 of the ties {1, 2, 4, 6} -> points (0,0,0), (0,0,.03), (0,.05,0), (.05,0,0)
    kept = pts[[0, 5, 1, 2]].astype(np.float64)
    c = kept - kept.mean(0)
    w, v = np.linalg.eigh(c.T @ c / 4)
    assert np.abs(got[0] - canonical_sign(v[:, 0])).max() <= 1e-12
    other = pts[[0, 5, 4, 6]].astype(np.float64)                        # the cut by index the other way round
    c = other - other.mean(0)
    assert np.abs(got[0] - canonical_sign(np.linalg.eigh(c.T @ c / 4)[1][:, 0])).max() > 1e-3
    assert normals_ref(pts, radius=0.1, max_nn=50)[1][0] == 7


def test_scene_generator():
    a, b = make_scene(4000, 0), make_scene(4000, 0)
    assert a.dtype == np.float32 and a.shape == (4000, 3) and np.array_equal(a, b)
    assert not np.array_equal(a, make_scene(4000, 1))
    assert make_scene(8000, 2).shape == (8000, 3)


def test_with_normals_columns():
    from detection_3d_amd.normals import with_normals
    calls = []

    def fake(xyz, radius, max_nn, orient):
        calls.append((tuple(xyz.shape), xyz.stride(0), radius, max_nn, orient))
        return torch.arange(xyz.shape[0] * 3, dtype=torch.float32).reshape(-1, 3)

    base = torch.rand((5, 9))
    want_n = torch.arange(15, dtype=torch.float32).reshape(5, 3)
    out3 = with_normals(base[:, :3].contiguous(), estimator=fake)
    out6 = with_normals(base[:, :6].contiguous(), 0.2, 30, (1, 2, 3), estimator=fake)
    out9 = with_normals(base, estimator=fake)
    for out in (out3, out6, out9):
        assert out.shape == (5, 9) and torch.equal(out[:, :3], base[:, :3]) and torch.equal(out[:, 6:9], want_n)
    assert torch.equal(out3[:, 3:6], torch.zeros(5, 3))
    assert torch.equal(out6[:, 3:6], base[:, 3:6]) and torch.equal(out9[:, 3:6], base[:, 3:6])
    assert out9.data_ptr() != base.data_ptr() and not torch.equal(base[:, 6:9], want_n)      # a copy
    # the estimator sees the xyz columns of the cloud in place (row stride 3, 6, 9), never a copy of the whole cloud
    assert calls == [((5, 3), 3, 0.1, 50, None), ((5, 3), 6, 0.2, 30, (1, 2, 3)), ((5, 3), 9, 0.1, 50, None)]
    for width in (2, 5, 7, 10):
        with pytest.raises(ValueError):
            with_normals(torch.zeros((4, width)), estimator=fake)
    with pytest.raises(ValueError):
        with_normals(torch.zeros(9), estimator=fake)


def test_argument_validation():
    from detection_3d_amd._lib import D3DError
    from detection_3d_amd.normals import estimate_normals, normals_kwargs, with_normals
    x = torch.zeros((4, 3))
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            estimate_normals(x, radius=bad)
    for bad in (2, 0, -5):
        with pytest.raises(ValueError):
            estimate_normals(x, max_nn=bad)
    with pytest.raises(ValueError):
        estimate_normals(x, orient=(1.0, 2.0))
    with pytest.raises(ValueError):
        estimate_normals(torch.zeros((4, 2)))
    with pytest.raises(ValueError):
        estimate_normals(torch.zeros(12))
    with pytest.raises(D3DError):                      # valid arguments, CPU tensor: no fallback
        estimate_normals(x)
    with pytest.raises(D3DError):
        with_normals(torch.zeros((4, 6)))
    assert normals_kwargs(None) is None and normals_kwargs("estimate") == {}
    assert normals_kwargs({"radius": 0.2, "max_nn": 30}) == {"radius": 0.2, "max_nn": 30}
    for bad in ("yes", {"radius": -1.0}, {"max_nn": 2}, {"k": 3}, 5):
        with pytest.raises(ValueError):
            normals_kwargs(bad)


def test_loops_take_the_keyword():
    import inspect

    from detection_3d_amd import engine
    from detection_3d_amd.serving import BuildingPipeline
    for fn in (engine.inference, engine.train, engine.collate, BuildingPipeline.__init__):
        assert inspect.signature(fn).parameters["normals"].default is None, fn
    with pytest.raises(ValueError):
        engine.collate([], None, normals="maybe")


def test_estimate_normals_flag(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "scripts"))
    sys.modules.pop("train_ddp", None)
    import train_ddp
    assert train_ddp.parse_args([]).normals is None
    assert train_ddp.parse_args(["--estimate-normals"]).normals == "estimate"
    assert train_ddp.parse_args(["--estimate-normals=0.05,30"]).normals == {"radius": 0.05, "max_nn": 30}
    assert train_ddp.parse_args(["--estimate-normals", "0.2"]).normals == {"radius": 0.2}
    assert train_ddp.parse_args(["--estimate-normals", "--steps", "3"]).normals == "estimate"
    for bad in ("0.1,50,2", "-1", "0.1,2"):
        with pytest.raises(ValueError):
            train_ddp.parse_args([f"--estimate-normals={bad}"])
