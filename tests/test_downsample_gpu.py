"""detection_3d_amd.downsample (downsample.hip) against the numpy restatement of its semantics in tests/downsample_ref.py,
and its plumbing through engine.collate and serving.BuildingPipeline.

Bounds, derived: voxels, counts, inverse and order are integers and must be exact.  The device's fp64 sum of `count`
fp32 values is off by at most count * 2^-53 relative to the sum of magnitudes, which can move the one rounding to fp32
only at a tie: every mean is within 1 fp32 ulp of the exactly rounded reference (math.fsum).  A unit normal rounded to
fp32 has a length within 2 ulp of one (each component is off by half an ulp of a value below one)."""
import numpy as np
import pytest
import torch

from tests.downsample_ref import sample_rows_ref, voxel_downsample_ref
from tests.normals_ref import make_scene

pytestmark = pytest.mark.gpu

_REF = {}


def _cloud(ncols, seed=0, n=20000):
    """make_scene's positions, random colours and random unit normals -> fp32 [n, ncols]"""
    key = ("cloud", ncols, seed, n)
    if key not in _REF:
        rs = np.random.RandomState(100 + seed)
        xyz = make_scene(n, seed)
        nrm = rs.randn(n, 3)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        _REF[key] = np.ascontiguousarray(np.concatenate([xyz, rs.rand(n, 3), nrm], 1)[:, :ncols].astype(np.float32))
    return _REF[key]


def _ref(name, pcl, voxel, normal_col="auto"):
    key = ("ref", name, voxel, normal_col)
    if key not in _REF:
        _REF[key] = voxel_downsample_ref(pcl, voxel, normal_col)
    return _REF[key]


def _run(dev, pcl, voxel, **kw):
    from detection_3d_amd.downsample import voxel_downsample
    out, inv, cnt = voxel_downsample(torch.from_numpy(np.ascontiguousarray(pcl)).to(dev), voxel, return_inverse=True,
                                     return_counts=True, **kw)
    assert out.dtype == torch.float32 and inv.dtype == torch.int32 and cnt.dtype == torch.int32
    return out.cpu().numpy(), inv.cpu().numpy(), cnt.cpu().numpy()


def _check_structure(got, ref, what):
    (out, inv, cnt), (r_out, r_inv, r_cnt) = got, ref
    print(f"{what}: {r_inv.shape[0]} points -> {r_out.shape[0]} voxels, largest {int(r_cnt.max()) if r_cnt.size else 0}")
    assert out.shape == r_out.shape, (what, out.shape, r_out.shape)
    assert np.array_equal(cnt, r_cnt), what
    assert np.array_equal(inv, r_inv), what


def _check_means(out, r_out, what, normal_col=None):
    err = np.abs(out.astype(np.float64) - r_out.astype(np.float64))
    ulp = np.spacing(np.abs(r_out)).astype(np.float64)
    worst = float((err / ulp).max()) if out.size else 0.0
    print(f"{what}: largest mean error {worst:.2f} ulp (bound 1), {int((err > 0).sum())} of {out.size} values differ")
    assert (err <= ulp).all(), (what, worst)
    if normal_col is not None:
        length = np.linalg.norm(out[:, normal_col:normal_col + 3].astype(np.float64), axis=1)
        has = length > 0
        dev_ulp = np.abs(length[has] - 1.0).max() / 2.0 ** -24
        print(f"{what}: normal lengths within {dev_ulp:.2f} ulp of one (bound 2)")
        assert dev_ulp <= 2.0, (what, dev_ulp)


def _lattice():
    """about 6000 rows of multiples of 1/16: positions in [-8, 8) (half of them in [-1, 1)^3, so that voxels of 0.25 hold
    several), 1000 duplicates of earlier rows; every fp64 sum is exact in any order"""
    rs = np.random.RandomState(7)
    wide = rs.randint(-128, 128, size=(3000, 3))
    near = rs.randint(-16, 16, size=(2000, 3))
    xyz = np.concatenate([wide, near]) / 16.0
    rest = rs.randint(-16, 17, size=(5000, 6)) / 16.0
    pcl = np.concatenate([xyz, rest], 1)
    pcl = np.concatenate([pcl, pcl[rs.randint(0, 5000, size=1000)]])
    return np.ascontiguousarray(pcl[rs.permutation(6000)].astype(np.float32))


def test_lattice_bit_for_bit(dev):
    pcl = _lattice()
    lo = pcl[:, :3].min(0).astype(np.float64) - 0.125
    assert pcl[:, :3].min() < 0 and (np.modf((pcl[:, :3].astype(np.float64) - lo) / 0.25)[0] == 0).any()   # on cell faces
    ref = voxel_downsample_ref(pcl, 0.25)
    got = _run(dev, pcl, 0.25)
    _check_structure(got, ref, "lattice")
    assert ref[2].max() > 4 and ref[0].shape[0] < 5000
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))
    # without normal columns the three are plain means
    ref_n = voxel_downsample_ref(pcl, 0.25, None)
    got_n = _run(dev, pcl, 0.25, normal_col=None)
    assert np.array_equal(got_n[0].view(np.uint32), ref_n[0].view(np.uint32))
    got_3 = _run(dev, pcl, 0.25, normal_col=3)
    assert np.array_equal(got_3[0].view(np.uint32), voxel_downsample_ref(pcl, 0.25, 3)[0].view(np.uint32))


@pytest.mark.parametrize("voxel", [0.02, 0.05])
@pytest.mark.parametrize("ncols", [3, 6, 9])
def test_random_scenes(dev, ncols, voxel):
    pcl = _cloud(ncols)
    ref = _ref(("cloud", ncols), pcl, voxel)
    got = _run(dev, pcl, voxel)
    what = f"scene C={ncols} voxel={voxel}"
    _check_structure(got, ref, what)
    assert 0 < ref[0].shape[0] < pcl.shape[0]
    _check_means(got[0], ref[0], what, 6 if ncols == 9 else None)


def test_small_and_alone(dev):
    from detection_3d_amd.downsample import voxel_downsample
    for c in (3, 9, 16):
        out, inv, cnt = voxel_downsample(torch.zeros((0, c), device=dev), 0.02, return_inverse=True, return_counts=True)
        assert out.shape == (0, c) and inv.shape == (0,) and cnt.shape == (0,)
    one = np.float32([[1.5, -2.25, 0.75, 0.1, 0.2, 0.3, 0.6, 0.0, 0.9]])
    out, inv, cnt = _run(dev, one, 0.02)
    assert np.array_equal(out.view(np.uint32), one.view(np.uint32)) and inv.tolist() == [0] and cnt.tolist() == [1]
    for n in (1025, 4097):
        rs = np.random.RandomState(n)
        pcl = rs.rand(n, 9).astype(np.float32)
        pcl[:, :3] = (rs.permutation(n)[:, None] * 0.5 + rs.rand(n, 3) * 0.25).astype(np.float32)   # 0.5 m apart
        out, inv, cnt = _run(dev, pcl, 0.05)
        assert out.shape == (n, 9) and (cnt == 1).all() and np.array_equal(inv, np.arange(n))
        assert np.array_equal(out.view(np.uint32), pcl.view(np.uint32))


def test_one_voxel_and_the_chunk_split(dev):
    same = np.tile(np.float32([[3.0, -2.0, 0.5, 0.25, 0.5, 0.75]]), (3000, 1))
    out, inv, cnt = _run(dev, same, 0.02)
    assert out.shape == (1, 6) and cnt.tolist() == [3000] and (inv == 0).all()
    assert np.array_equal(out, same[:1])
    # 5000 points inside one voxel (a long segment: ten chunks of 512 rows), 5000 scattered, interleaved
    rs = np.random.RandomState(3)
    # (with the minimum at the origin the cells are [-0.01 + 0.02 k, ...): 10.0 and 1.0 are centres of cells)
    dense = np.concatenate([np.float32([10.0, 10.0, 1.0]) + (rs.rand(5000, 3) - 0.5) * 0.015, rs.rand(5000, 3)], 1)
    wide = np.concatenate([rs.rand(5000, 3) * 8.0, rs.rand(5000, 3)], 1)
    wide[0, :3] = 0.0
    pcl = np.empty((10000, 6), np.float32)
    pcl[0::2], pcl[1::2] = dense, wide
    ref = voxel_downsample_ref(pcl, 0.02)
    got = _run(dev, pcl, 0.02)
    _check_structure(got, ref, "dense voxel + scattered")
    assert ref[2].max() == 5000
    _check_means(got[0], ref[0], "dense voxel + scattered")
    # a segment of 65 .. 512 rows (one chunk) and one just above a chunk
    for rows in (65, 512, 513):
        part = np.concatenate([dense[:rows], wide[:100]]).astype(np.float32)
        ref = voxel_downsample_ref(part, 0.02)
        got = _run(dev, part, 0.02)
        _check_structure(got, ref, f"segment of {rows}")
        assert ref[2].max() == rows
        _check_means(got[0], ref[0], f"segment of {rows}")


def test_far_clusters_and_dropped_rows(dev):
    from detection_3d_amd._lib import lib
    a = _cloud(6, n=4000)
    b = a.copy()
    b[:, :3] += np.float32([-500.0, -30.0, 0.0])
    both = np.concatenate([a, b])
    ref = voxel_downsample_ref(both, 0.02)
    got = _run(dev, both, 0.02)
    _check_structure(got, ref, "two clusters 500 m apart")
    _check_means(got[0], ref[0], "two clusters 500 m apart")
    # the scratch is linear in n and does not know the extent
    assert lib().d3d_voxel_downsample_scratch_bytes(1 << 20, 16) <= 64 * (1 << 20) + (1 << 16)
    bad = a.copy()
    bad[0, 0] = np.nan
    bad[17, 1] = np.inf
    bad[18, 2] = -np.inf           # would poison the minimum
    bad[3999, 0] = np.nan
    bad[5, 4] = np.nan             # not a position: the row is kept
    ref = voxel_downsample_ref(bad, 0.02)
    got = _run(dev, bad, 0.02)
    assert (ref[1][[0, 17, 18, 3999]] == -1).all() and (ref[1] == -1).sum() == 4 and ref[1][5] >= 0
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    fin = np.isfinite(ref[0])
    assert np.array_equal(np.isfinite(got[0]), fin)
    _check_means(np.where(fin, got[0], 0), np.where(fin, ref[0], 0), "dropped rows")
    all_bad = np.full((10, 3), np.nan, np.float32)
    out, inv, cnt = _run(dev, all_bad, 0.02)
    assert out.shape == (0, 3) and (inv == -1).all() and cnt.shape == (0,)


def test_too_wide_a_cloud_is_an_error(dev):
    from detection_3d_amd._lib import D3DError
    from detection_3d_amd.downsample import voxel_downsample
    pcl = torch.tensor([[0.0, 0.0, 0.0], [1.0e6, 0.0, 0.0]], device=dev)
    with pytest.raises(D3DError, match=r"2\^21") as e:
        voxel_downsample(pcl, 0.02)
    assert "1000000" in str(e.value)
    out = voxel_downsample(pcl, 1.0)                  # the same cloud in voxels of 1 m is fine
    assert out.shape == (2, 3)


def test_reproducible(dev):
    from detection_3d_amd.downsample import voxel_downsample
    pcl = torch.from_numpy(_cloud(9)).to(dev)
    a = voxel_downsample(pcl, 0.05, return_inverse=True, return_counts=True)
    b = voxel_downsample(pcl, 0.05, return_inverse=True, return_counts=True)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    wide = torch.cat([pcl, pcl[:, :3]], 1)[:, :9]     # a non-contiguous view is made contiguous
    assert not wide.is_contiguous()
    assert torch.equal(voxel_downsample(wide, 0.05), a[0])


@pytest.mark.parametrize("n", [1, 1000, 70001])
def test_cap(dev, n):
    from detection_3d_amd.downsample import cap_points, sample_rows
    lists = {}
    for k in sorted({1, n - 1, n // 3}):
        for seed in (0, 1, 2 ** 40 + 5):
            rows = sample_rows(n, k, seed, dev)
            assert rows.dtype == torch.int32 and rows.shape == (min(k, n),)
            got = rows.cpu().numpy()
            assert np.array_equal(got, sample_rows_ref(n, k, seed)), (n, k, seed)
            assert (np.diff(got) > 0).all()
            assert torch.equal(rows, sample_rows(n, k, seed, dev))
            lists[(k, seed)] = got
        if 0 < k < n and n >= 1000 and k > 1:
            assert not np.array_equal(lists[(k, 0)], lists[(k, 1)])
    cloud = torch.arange(n * 4, dtype=torch.float32, device=dev).reshape(n, 4)
    k = max(n // 3, 1)
    out, rows = cap_points(cloud, k, seed=1, return_rows=True)
    if k >= n:
        assert out is cloud and rows is None
    else:
        assert torch.equal(out, cloud[torch.from_numpy(lists[(k, 1)]).to(dev).long()])
        assert torch.equal(cap_points(cloud, k, seed=1), out)


@pytest.fixture(scope="module")
def tiny(dev):
    """the model and scene of tests/test_normals_gpu.py"""
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


def test_pipeline_with_every_point_alone_changes_nothing(tiny, dev):
    from detection_3d_amd.downsample import voxel_downsample
    from detection_3d_amd.serving import BuildingPipeline
    cfg, model, cloud = tiny
    voxel = 2e-5
    assert voxel_downsample(cloud, voxel).shape[0] == cloud.shape[0]
    with torch.no_grad():
        got = BuildingPipeline(model, cfg, in_flight=2, device=dev, downsample=voxel).map([cloud, cloud])
        want = BuildingPipeline(model, cfg, in_flight=2, device=dev, downsample=None).map([cloud])
    torch.cuda.synchronize()
    assert want[0]["bbox3d"].shape[0] > 0
    assert _same(got[0], want[0]) and _same(got[1], want[0])


def test_pipeline_point_owner_follows_the_voxels(tiny, dev):
    from detection_3d_amd.downsample import apply_downsample, downsample_kwargs, voxel_downsample
    from detection_3d_amd.serving import BuildingPipeline
    cfg, model, cloud = tiny
    raw = cloud.clone()
    raw[5, 0] = float("nan")
    raw[77, 2] = float("inf")
    small, voxel_of_point = voxel_downsample(raw, 0.05, return_inverse=True)
    assert small.shape[0] < raw.shape[0] and int((voxel_of_point < 0).sum()) == 2
    with torch.no_grad():
        got = BuildingPipeline(model, cfg, in_flight=2, device=dev, downsample=0.05, point_owner=True).map([raw])[0]
        want = BuildingPipeline(model, cfg, in_flight=2, device=dev, point_owner=True).map([small])[0]
    torch.cuda.synchronize()
    assert want["bbox3d"].shape[0] > 0 and _same(got, want)
    assert got["point_owner"].shape == (raw.shape[0],) and got["point_owner"].dtype == torch.int32
    gone = voxel_of_point < 0
    assert torch.equal(got["point_owner"][~gone], want["point_owner"][voxel_of_point[~gone].long()])
    assert (got["point_owner"][gone] == -1).all()
    assert torch.equal(got["point_count"], want["point_count"])
    # ... and through the cap's row list
    dkw = {"voxel": 0.05, "max_points": small.shape[0] // 2, "seed": 4}
    capped, source = apply_downsample(raw, downsample_kwargs(dkw), return_source=True)
    assert capped.shape[0] == small.shape[0] // 2 and source.shape == (raw.shape[0],)
    kept = source >= 0
    assert torch.equal(capped[source[kept].long()], small[voxel_of_point[kept].long()])
    assert int(torch.unique(source[kept]).numel()) == capped.shape[0] and bool((~kept)[gone].all())
    with torch.no_grad():
        got = BuildingPipeline(model, cfg, in_flight=2, device=dev, downsample=dkw, point_owner=True).map([raw])[0]
        want = BuildingPipeline(model, cfg, in_flight=2, device=dev, point_owner=True).map([capped])[0]
    torch.cuda.synchronize()
    assert _same(got, want)
    assert torch.equal(got["point_owner"][kept], want["point_owner"][source[kept].long()])
    assert (got["point_owner"][~kept] == -1).all()


def test_collate_downsamples(tiny, dev):
    from detection_3d_amd import engine
    from detection_3d_amd.downsample import prepare_cloud
    from detection_3d_amd.voxelize import voxelize
    cfg, _, cloud9 = tiny
    cloud6 = cloud9[:, :6].contiguous()
    tg = {"bbox3d": torch.zeros((0, 7)), "labels": torch.zeros((0,), dtype=torch.int64)}
    dkw = {"voxel": 0.05, "max_points": 5000, "seed": 2}
    got, _ = engine.collate([(cloud6, tg), (cloud6[:20000], tg)], cfg, normals="estimate", downsample=dkw)
    s3d = cfg.SPARSE3D
    parts = [voxelize(prepare_cloud(c, 0.05, 5000, 2, normals="estimate"), s3d.VOXEL_SCALE, s3d.VOXEL_FULL_SCALE)
             for c in (cloud6, cloud6[:20000])]
    assert got[2] == 2 and got[1].shape[1] == 9 and got[1].shape[0] <= 10000
    assert torch.equal(got[0][:, :3], torch.cat([p[0] for p in parts])) and torch.equal(got[1], torch.cat([p[1] for p in parts]))
    assert torch.equal(got[0][:, 3], torch.cat([torch.full((p[0].shape[0],), b, dtype=torch.int64, device=dev)
                                                for b, p in enumerate(parts)]))
    plain, _ = engine.collate([(cloud9, tg)], cfg)
    plain_none, _ = engine.collate([(cloud9, tg)], cfg, downsample=None)
    assert torch.equal(plain[0], plain_none[0]) and torch.equal(plain[1], plain_none[1])
