"""register.global_align without a GPU: the numpy restatement of its definition (tests/global_ref.py) against a brute-force
form on a tiny lattice, its recovery of known poses on cropped scans of a building, the half-turn ambiguity of a symmetric
shell as it shows in the margin, and the argument checks of global_align and merge_scans(init_poses=...)."""
import math

import numpy as np
import pytest

from tests import global_ref as g

LATTICE = (1024, 1024, 128)          # 51 m at 0.05 m: the 25 x 19 m building from its own minimum, under every turn
# Seeds 1 .. 12.  Seed 0 of this generator draws interior walls that leave the shell nearly point-symmetric: the half turn
# scores 1330 against 1325 for the true pose at x <= 20 / x >= 5, the stated limit of the method; seed 12 stands in for it.
SEEDS = tuple(range(1, 13))


def _tiny(seed):
    """a few walls on a 32 x 32 lattice of 0.5 m cells, as two [.., 6] clouds"""
    rng = np.random.RandomState(seed)

    def cloud(n_walls, shift):
        rows = []
        for _ in range(n_walls):
            axis = int(rng.randint(2))
            off = rng.uniform(1.0, 12.0)
            a, b = np.sort(rng.uniform(0.0, 12.0, 2))
            t = np.arange(a, b + 0.25, 0.25)
            p = np.zeros((len(t), 6))
            p[:, axis], p[:, 1 - axis], p[:, 2] = off, t, rng.uniform(0.0, 2.0, len(t))
            p[:, 3 + axis] = 1.0
            rows.append(p)
        rows.append(np.array([[0.0, 0.0, 0.0, 0, 0, 1.0], [12.0, 12.0, 2.0, 0, 0, 1.0]]))
        out = np.concatenate(rows)
        out[:, :3] += shift
        return out.astype(np.float32)

    return cloud(5, (3.0, -2.0, 0.5)), cloud(6, (-7.0, 4.0, 0.0))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_matches_brute_force_on_a_tiny_lattice(seed):
    src, tgt = _tiny(seed)
    lat, bin_, K = (32, 32, 32), 0.5, 64
    ref = g.align_ref(src, tgt, bin=bin_, lattice=lat, tol=5.0, peaks=K, sep=2)
    brute = g.brute_scores(src[:, :3], src[:, 3:], g.origin_of(src[:, :3]), tgt[:, :3], tgt[:, 3:], g.origin_of(tgt[:, :3]),
                           bin_, lat, 5.0)
    seen = 0
    for q in range(4):
        for i in range(K):
            for j in range(K):
                if ref["peak_value"][2 * q, i] > 0 and ref["peak_value"][2 * q + 1, j] > 0:
                    sx, sy = int(ref["peak_shift"][2 * q, i]), int(ref["peak_shift"][2 * q + 1, j])
                    assert ref["scores"][q, i, j] == brute[q, sx + 31, sy + 31], (q, i, j)
                    seen += 1
                else:
                    assert ref["scores"][q, i, j] == -1
    assert seen >= 16 and ref["status"] == 0
    # the pick is the best the peak tables offer, and its score is what brute force finds at that turn and shift
    q, sx, sy, _ = ref["choice"]
    assert ref["score"][4] == brute[q, sx + 31, sy + 31] == ref["scores"].max()
    assert ref["score"][5] <= ref["score"][4] and [ref["score"][k] == ref["scores"][k].max() for k in range(4)] == [True] * 4


def test_peaks_are_what_the_definition_says():
    L = 7
    C = np.array([0, 5, 5, 1, 0, 7, 7, 7, 0, 0, 3, 0, 0], np.int64)           # entry s + L - 1
    value, shift = g.peaks_of(C, L, 4, 2)
    # 5 at entry 1 (the equal 5 behind it is not larger; that one has an equal value before it and is none), the first of
    # the three 7, and 3
    assert value.tolist() == [7, 5, 3, -1] and shift.tolist() == [5 - 6, 1 - 6, 10 - 6, 0]
    value, shift = g.peaks_of(C, L, 2, 0)                                     # sep 0: every positive entry, cut at K
    assert value.tolist() == [7, 7] and shift.tolist() == [5 - 6, 6 - 6]


def _recover(seed, q, **crop):
    src, tgt, truth = g.pair(seed, q, **crop)
    ref = g.align_ref(src, tgt, lattice=LATTICE)
    err = g.shift_error(ref["pose"], truth, src[:, :3].astype(np.float64).mean(0))
    print(f"seed {seed} q {q}: choice {ref['choice'].tolist()} score {ref['score'].tolist()} margin {ref['margin']:.3f} "
          f"error {err.round(4).tolist()} support {ref['support'].tolist()}")
    return ref, err


@pytest.mark.parametrize("seed", SEEDS)
def test_recovers_heading_and_shift_of_cropped_scans(seed):
    """target x <= 20, source x >= 5, 0.05 degrees of residual yaw, shifts up to 20 m: heading exact, shift within a bin"""
    for q in range(4):
        ref, err = _recover(seed, q)
        assert ref["status"] == 0 and ref["choice"][0] == q
        assert (err <= 0.05).all(), err
        assert ref["support"][1] == 0 and ref["support"][3] == 0


def test_small_overlap_of_a_symmetric_shell_shows_in_the_margin():
    """x <= 18 / x >= 7: the half turn of the shell fits nearly as well as the truth, and sometimes better (the stated
    limit); either way the margin says so.  "Near 1" is taken as at least 0.85 (recovered cases with the wider overlap
    reach down to 0.65); the restatement gives 0.972, 0.930, 0.891 and 0.911 here, three of the four on the half turn."""
    margins, wrong = [], 0
    for seed in (1, 2, 5, 8):
        ref, err = _recover(seed, 0, target_max_x=18.0, source_min_x=7.0)
        margins.append(ref["margin"])
        wrong += int(ref["choice"][0] != 0)
        assert ref["choice"][0] in (0, 2)
    assert min(margins) >= 0.85, margins
    assert wrong >= 1                   # the limit is real: it is why Alignment.margin exists


def test_no_walls_is_status_1_with_the_origins_shift():
    rng = np.random.RandomState(0)
    floor = np.zeros((500, 6), np.float32)
    floor[:, :2], floor[:, 5] = rng.uniform(0, 5, (500, 2)), 1.0
    moved = floor.copy()
    moved[:, :3] += np.array([3.0, -1.0, 0.5], np.float32)
    ref = g.align_ref(floor, moved, lattice=(256, 256, 64))
    assert ref["status"] == 1 and ref["choice"].tolist() == [0, 0, 0, 0] and ref["score"][4] == -1
    assert np.array_equal(ref["pose"][:3, 3], g.origin_of(moved[:, :3]) - g.origin_of(floor[:, :3]))
    empty = g.align_ref(floor[:0], moved, lattice=(256, 256, 64))
    assert empty["status"] == 1 and empty["support"].tolist() == [0, 0, 500, 0]


def test_argument_errors_come_before_any_gpu_work():
    import torch
    from detection_3d_amd.register import global_align, lattice_align, merge_scans
    a, b = torch.zeros((8, 9)), torch.zeros((8, 9))            # CPU tensors: a check that passed would raise D3DError
    for kw in ({"bin": 0.0}, {"bin": float("nan")}, {"bin": "x"}, {"lattice": (2048, 2048)}, {"lattice": (2048, 1024, 256)},
               {"lattice": (2000, 2000, 256)}, {"lattice": (8192, 8192, 256)}, {"lattice": (2048, 2048, 0)},
               {"lattice": (2048, 2048, 5000)}, {"lattice": 7}, {"tol": 0.0}, {"tol": 21.0}, {"peaks": 0}, {"peaks": 65},
               {"peaks": 2.5}, {"sep": -1}, {"sep": 65}, {"sep": True}, {"frame": {"max_tilt": 90.0}}, {"frame": {"nope": 1}},
               {"frame": 3}, {"normal_radius": 0.0}, {"max_nn": 2}):
        with pytest.raises(ValueError):
            global_align(a, b, **kw)
    with pytest.raises(ValueError):
        global_align(a, torch.zeros((8, 2)))
    with pytest.raises(ValueError):
        global_align(torch.zeros(8), b)
    with pytest.raises(ValueError):
        lattice_align(a, a[:, 6:9], torch.zeros(3, dtype=torch.float64), b, b[:, 6:9], torch.zeros(3, dtype=torch.float64),
                      peaks=100)
    for kw in ({"init_poses": "icp"}, {"init_poses": "global", "global_kw": {"bin": -1.0}},
               {"init_poses": "global", "global_kw": {"what": 1}}, {"global_kw": {"bin": 0.1}},
               {"init_poses": "global", "global_kw": {"lattice": (100, 100, 10)}}):
        with pytest.raises(ValueError):
            merge_scans([a, b], **kw)


def test_pose_is_exact_in_its_rotation_and_written_order():
    o_s, o_t = np.array([1.25, -3.5, 0.125]), np.array([-7.0, 2.0, 1.0])
    for q in range(4):
        P = g.pose_of(q, 5, -9, 3, o_s, o_t, 0.05, 64)
        R = P[:3, :3]
        assert set(np.abs(R).reshape(-1).tolist()) == {0.0, 1.0} and not np.signbit(R[R == 0]).any()
        assert np.allclose(R, g.rigid(90.0 * q, (0, 0, 0))[:3, :3], atol=1e-15)
        # the source's lattice centre goes to the target's, plus the shift
        centre = np.append(o_s[:2] + 0.05 * 32, o_s[2])
        want = np.array([o_t[0] + 0.05 * (5 + 32), o_t[1] + 0.05 * (-9 + 32), o_t[2] + 0.05 * 3])
        assert np.allclose(R @ centre + P[:3, 3], want, atol=1e-12)
    assert math.isinf(g.align_ref(np.zeros((0, 6), np.float32), np.zeros((0, 6), np.float32), lattice=(32, 32, 8))["margin"])
