"""What test_nms_forms_gpu.py relies on, checked without a GPU: the lattice scenes' Python-greedy keep lists equal the CPU
oracle's (so the exact graph, the oracle and -- on the GPU -- the kernels are three independent statements of one
result), the margin rule, and the hard-pair families: the doubtful share, the agreement of the oracle with the fp64
reference outside the doubtful band, and that the recorded delta still holds."""
import numpy as np
import pytest

import oracle
from tests import nms_forms as F


def _oracle_keep(scene):
    return oracle.rotate_nms_3d(scene["boxes"], scene["scores"], scene["thr"]).tolist()


def test_pair_cases_of_the_issue_table():
    for st, want in ((("path", 2), [0]), (("ztouch",), [0, 1]), (("zhalf",), [0])):
        sc = F.lattice_scene([st])
        assert sc["keep"] == want == _oracle_keep(sc)
    far = F.lattice_scene([("path", 3)], [0, 2, 1])           # positions 0 and 1 are shifted by 1: IoU 1/3
    assert far["adj"][0] == [2] and far["keep"][:2] == [0, 1] and far["keep"] == _oracle_keep(far)


@pytest.mark.parametrize("n", [n for n in F.SIZES if n <= 1100])
def test_size_scenes_greedy_equals_oracle(n):
    sc = F.size_scene(n)
    assert sc["boxes"].shape == (n, 7) and sc["keep"] == _oracle_keep(sc)
    if n >= 63:
        assert 0 < len(sc["keep"]) < n


@pytest.mark.parametrize("name", [s for s in F.STRUCTURES if s != "clique_every_chunk"])
def test_structure_scenes_greedy_equals_oracle(name):
    sc = F.structure_scene(name)
    assert sc["keep"] == _oracle_keep(sc)


def test_long_path_in_random_order_and_dyadic_cliques():
    sc = F.lattice_scene([("path", 1025)], np.random.RandomState(3).permutation(1025))
    assert sc["keep"] == _oracle_keep(sc) and 342 <= len(sc["keep"]) <= 513
    sizes = []
    for thr in (0.5, 0.75, 0.9):
        cl = F.lattice_scene([("clique", 300)], np.random.RandomState(4).permutation(300), thr)
        assert cl["keep"] == _oracle_keep(cl)
        sizes.append(len(cl["keep"]))
    assert sizes[0] == 1 and sizes[0] <= sizes[1] <= sizes[2] and sizes[2] > 1


def test_margin_rule_rejects_an_iou_on_the_threshold():
    with pytest.raises(AssertionError):
        F.lattice_scene([("path", 2)], thr=0.6)                # 3/5 against float32(0.6): closer than 1e-6
    with pytest.raises(AssertionError):
        F.lattice_scene([("cliquez", 2)], thr=1.0)


def test_identical_lattice_boxes_at_threshold_one_suppress():
    two = F.identical_at_one()
    gate, iou = oracle.nms_pair(two[0::2], two[1::2])
    assert np.all(gate > 0) and np.all(iou == 1.0)
    for p in range(0, two.shape[0], 2):
        assert F.pair_iou_f64(two[p], two[p + 1])[0] == 1.0


def test_doubtful_share_and_agreement_of_the_two_references():
    m = F.measure()
    print(F.report())
    assert 0 < m["delta"] <= F.DELTA_RECORDED                  # the band of the docstring still covers a fresh measurement
    assert F.DELTA_RECORDED < 0.25 * min(F.THRS)               # ... and is far below every threshold
    exc = 0
    for name, r in m["families"].items():
        assert 200 <= r["n"] <= 4096, name
        if not r["finite"]:
            continue
        doubt = np.abs(r["iou64"] - float(np.float32(r["thr"]))) <= F.DELTA_RECORDED
        assert doubt.mean() <= F.DOUBTFUL_CAP, (name, doubt.mean())
        differ = (r["suppress"] != r["sup64"]) & ~doubt
        assert not np.any(differ & ~(r["gate"] <= 0)), (name, np.nonzero(differ)[0])
        exc += int(np.sum(differ))
        if r["both"]:
            assert r["suppress"][~doubt].any() and (~r["suppress"][~doubt]).any(), name
    assert exc == F.GATE_EXCEPTIONS_RECORDED
    assert set(F.FAMILY_RECORD) == set(m["families"])
    for name, (n, thr, doubtful, suppress) in F.FAMILY_RECORD.items():
        r = m["families"][name]
        assert (r["n"], r["thr"], int(r["doubtful"].sum()), int(r["suppress"].sum())) == (n, thr, doubtful, suppress), name


def test_non_finite_pairs_follow_the_reference_semantics():
    """iou_z = NaN leaves the decision to the BEV polygon (the pair suppresses as its finite form does): a NaN in z0 or dz,
    and z0 = +-Inf (-inf / inf); dz = +-Inf gives iou_z = 0 or negative and never suppresses; a NaN or Inf BEV field never
    suppresses (no polygon)"""
    m = F.measure()
    for name in ("non_finite", "non_finite_clamped"):
        f, r = m["inputs"][name], m["families"][name]
        bad = ~np.isfinite(f["a"]) | ~np.isfinite(f["b"])
        assert np.all(bad.sum(1) == 1)
        field = bad.argmax(1)
        nan = np.isnan(f["a"]).any(1) | np.isnan(f["b"]).any(1)
        assert np.all(r["suppress"][(field == 2) | (nan & (field == 5))]), name
        pos_inf = (f["a"] == np.inf).any(1) | (f["b"] == np.inf).any(1)
        assert not np.any(r["suppress"][pos_inf & (field == 5)]), name      # (-Inf: skipped too, unless the clamp replaces it)
        assert np.array_equal(r["suppress"][~nan & ~pos_inf & (field == 5)].all(), name == "non_finite_clamped")
        assert not np.any(r["suppress"][np.isin(field, (0, 1, 6))]), name
        if name == "non_finite":
            assert not np.any(r["suppress"][np.isin(field, (3, 4))])


def test_expect_form_restates_the_dispatch():
    assert F.expect_form(1024, F.MODE_LDS)["ncbmax"] == 16 and F.expect_form(1025, F.MODE_LDS)["ncbmax"] == 32
    assert F.expect_form(2048, F.MODE_DEFAULT)["ncbmax"] == 32 and F.expect_form(2049, F.MODE_LDS)["ncbmax"] == 64
    assert F.expect_form(4096, F.MODE_LDS)["lds_bytes"] == 66560 and F.expect_form(4032, F.MODE_LDS)["lds_bytes"] == 65536
    assert F.expect_form(4096, F.MODE_REGS, 3, 17) == dict(family=1, ncbmax=0, ncb=64, segments=3, n_max=4096, max_keep=17,
                                                         lds_bytes=0)
