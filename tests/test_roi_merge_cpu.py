"""The fp32 emulation of tests/roi_merge_ref.py against the fp64 reference of tests/roi_forms.py, on the cases that
test_roi_merge_gpu.py runs, and the list lengths those cases were built for.

Bound: the weights of the exact geometry class are fp32 numbers and so are their sums, so the emulation rounds only the
product w v (once), the additions down a bin's lists (one per merged cell) and the division: per element
|emulation - reference| <= gamma_n sum |w v| / NS with n = merged cells of the bin over its steps + 2."""
import numpy as np
import pytest

from tests import roi_forms as Rf
from tests import roi_merge_ref as M


def _reference(case):
    return Rf.roi_ref(case["rois"], case["scale"], case["map"], case["crop"], case["bins"], case["sr"], slopes=False)


@pytest.mark.parametrize("bf16", [False, True])
def test_emulation_matches_the_fp64_reference(bf16):
    cs, emu = M.cached(bf16)
    for name, case in cs.items():
        out, lengths = emu[name]
        R = _reference(case)
        K, NB = case["K"], Rf.nb_of(case["bins"])
        want = Rf.list_lengths(R.taps, K, NB, R.steps)
        assert np.array_equal(lengths, want), f"{name}: the emulation's lists differ from the reference's tap lists"
        per_bin = np.concatenate([lengths[a:a + NB * s].reshape(NB, s).sum(1) for a, s in
                                  zip(np.concatenate([[0], np.cumsum(NB * R.steps)[:-1]]), R.steps)]).reshape(K, 1, NB)
        bound = (Rf.gamma(1) * (per_bin + 2)).reshape((K, 1) + case["bins"]) * R.mag
        err = np.abs(out.astype(np.float64) - R.out)
        assert (err <= bound).all(), f"{name}: emulation off by {(err / np.maximum(bound, 1e-300)).max():.3f} bounds"
        assert np.abs(R.out).max() > 0


def test_exact_geometry():
    """every case is in the exact class: yaw 0, samples on the 1/8-pixel lattice, NS a power of two, fp32 weights"""
    cs, _ = M.cached(False)
    for name, case in cs.items():
        for n in range(case["K"]):
            geo = Rf.geometry(case["rois"][n], case["scale"], case["bins"], case["sr"])
            assert geo["theta"] == 0.0, name
            ns = int(np.prod(geo["g"]))
            assert ns & (ns - 1) == 0, name
            for v in Rf.sample_positions(geo, case["bins"]):
                assert np.array_equal(v * 8, np.round(v * 8)), name


def test_list_lengths_reached():
    cs, emu = M.cached(False)
    lengths = emu["lengths"][1]
    assert lengths.tolist() == M.expected_lengths()
    B = M.B
    assert {0, 1, B - 1, B, B + 1, 64} <= set(lengths.tolist())
    groups = lengths.reshape(-1, Rf.ROI_G)
    # groups in which a bin's cells begin inside a batch of B cells that holds cells of an earlier bin
    straddle = [g for g in groups if any(a % B and c for a, c in zip(np.concatenate([[0], np.cumsum(g)[:-1]]), g))]
    assert len(straddle) >= 4 and groups.sum(1).max() == 4 * 64
    one = emu["one cell"][1]
    assert one.tolist() == [1, 8, 1]
    assert cs["NS = 32"]["sr"] == 0 and emu["NS = 32"][1].size == 4 * 4 * 4       # four steps per bin
    assert emu["NS = 32"][1].max() >= 2
    # ragged last groups: 1 and 2 bins; 6 x 8 x 3 and 2 x 2 x 3: groups that straddle (ph, pw) cells
    assert Rf.nb_of(cs["one cell"]["bins"]) % Rf.ROI_G == 1 and Rf.nb_of(cs["PZ = 5"]["bins"]) % Rf.ROI_G == 2
    every = np.concatenate([v[1] for v in emu.values()])
    assert (every >= 16).sum() > 0 and ((every >= 2) & (every <= 7)).sum() > 0
