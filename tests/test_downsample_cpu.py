"""detection_3d_amd.downsample without a GPU: the `downsample=` keyword, the command-line flag, the cap of a cloud that is
small enough, and the spread of the cap's key mix (through its numpy restatement, tests/downsample_ref.py)."""
import numpy as np
import pytest
import torch

from detection_3d_amd.downsample import apply_downsample, cap_points, downsample_kwargs, parse_downsample
from tests.downsample_ref import row_keys, sample_rows_ref


def test_downsample_keyword():
    assert downsample_kwargs(None) is None
    assert downsample_kwargs(0.02) == {"voxel": 0.02, "seed": 0}
    assert downsample_kwargs({"voxel": 0.05, "max_points": 1000, "seed": 3}) == {"voxel": 0.05, "max_points": 1000,
                                                                                 "seed": 3}
    assert downsample_kwargs({"max_points": 10}) == {"max_points": 10, "seed": 0}
    assert downsample_kwargs({"voxel": None, "max_points": None}) == {"voxel": None, "max_points": None, "seed": 0}
    for bad in ({"voxels": 0.02}, {"voxel": 0.02, "radius": 1}):
        with pytest.raises(ValueError, match="unknown keywords"):
            downsample_kwargs(bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "0.02", True, {"voxel": 0}, {"max_points": 0}, [0.02]):
        with pytest.raises(ValueError):
            downsample_kwargs(bad)


def test_loops_check_the_keyword_before_they_touch_data():
    from detection_3d_amd import engine
    from detection_3d_amd.serving import BuildingPipeline
    with pytest.raises(ValueError, match="unknown keywords"):
        engine.collate([], None, downsample={"size": 1})
    with pytest.raises(ValueError, match="unknown keywords"):
        engine.inference(None, None, [], None, downsample={"size": 1})
    with pytest.raises(ValueError, match="unknown keywords"):
        engine.train(None, None, [], None, 1, downsample={"size": 1})
    with pytest.raises(ValueError, match="unknown keywords"):
        BuildingPipeline(None, None, device="cpu", downsample={"size": 1})


def test_parse_downsample():
    assert parse_downsample(None) is None and parse_downsample("") is None and parse_downsample("  ") is None
    assert parse_downsample("0.02") == {"voxel": 0.02, "seed": 0}
    assert parse_downsample("0.05,500000") == {"voxel": 0.05, "max_points": 500000, "seed": 0}
    for bad in ("0.02,1,2", "x", "0.02,many", "-1", "0.02,0"):
        with pytest.raises(ValueError):
            parse_downsample(bad)


def test_train_ddp_flag():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "train_ddp.py")
    spec = importlib.util.spec_from_file_location("train_ddp_for_test", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_args([]).downsample is None
    assert mod.parse_args(["--downsample", "0.02,500000"]).downsample == {"voxel": 0.02, "max_points": 500000, "seed": 0}


def test_cap_returns_a_small_cloud_as_it_is():
    pcl = torch.zeros((10, 6))
    assert cap_points(pcl, 10) is pcl and cap_points(pcl, 11) is pcl
    out, rows = cap_points(pcl, 500_000, return_rows=True)
    assert out is pcl and rows is None
    assert apply_downsample(pcl, None) is pcl
    assert apply_downsample(pcl, downsample_kwargs({"max_points": 10})) is pcl
    with pytest.raises(ValueError):
        cap_points(pcl, -1)


def test_reference_selection_is_the_k_smallest_keys():
    for n, k, seed in ((1000, 1, 0), (1000, 999, 1), (1000, 333, 2 ** 40 + 7)):
        key = row_keys(n, seed)
        assert key.max() < 2 ** 32 and np.unique(key).size == n           # the mix is a bijection: no ties
        rows = sample_rows_ref(n, k, seed)
        assert rows.shape == (k,) and (np.diff(rows) > 0).all()
        chosen = np.zeros(n, bool)
        chosen[rows] = True
        assert key[chosen].max() < key[~chosen].min()
    assert np.array_equal(sample_rows_ref(5, 9, 0), np.arange(5))
    assert not np.array_equal(row_keys(64, 0), row_keys(64, 1))
    assert not np.array_equal(row_keys(64, 0), row_keys(64, 1 << 32))     # the high half of the seed counts


@pytest.mark.parametrize("seed", range(8))
def test_key_mix_spreads_the_kept_rows(seed):
    """n = 65 536, k = 16 384: every block of 1024 consecutive rows and every residue class i mod 64 (1024 rows each)
    keeps 256 +- 84 rows; 84 = 6 sqrt(1024 * 1/4 * 3/4), six standard deviations of the binomial count, and sampling
    without replacement only tightens it."""
    n, k = 65536, 16384
    keep = np.zeros(n, bool)
    keep[sample_rows_ref(n, k, seed)] = True
    blocks = keep.reshape(64, 1024).sum(1)
    classes = keep.reshape(1024, 64).sum(0)
    print(f"seed {seed}: blocks {blocks.min()}..{blocks.max()}, residue classes {classes.min()}..{classes.max()}")
    assert np.abs(blocks - 256).max() <= 84, blocks
    assert np.abs(classes - 256).max() <= 84, classes
