"""The model of the plan builder (tests/plan_forms.py) against brute force, the plan checks against deliberately broken
plans, and the conditions the scenes of tests/test_plan_forms_gpu.py must meet for the seeds they use.  No GPU."""
import numpy as np
import pytest

from tests import plan_forms as P


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("K", [2, 8, 11, 12, 27, 28, 32])
def test_expected_rows_is_the_sort_on_explicit_keys(K):
    rng = np.random.RandomState(K)
    pool = rng.randint(1, 1 << min(K, 31), 60, dtype=np.int64)
    if K == 32:
        pool[:5] |= 1 << 31
    masks = pool[rng.randint(0, pool.size, 700)].astype(np.uint32)
    ids = list(range(masks.size))
    pc = [bin(int(m)).count("1") for m in masks]
    assert P.expected_rows(masks, K, P.IDENTITY).tolist() == ids
    radix = sorted(ids, key=lambda i: (-int(masks[i]), i))
    assert P.expected_rows(masks, K, P.RADIX).tolist() == radix == P.expected_rows(masks, K, P.BOUND).tolist()
    lo = [int(m) if K <= 11 else ((int(m) * 0x9E3779B1) % 2 ** 32) >> 21 for m in masks]
    assert all(0 <= v < 2 ** 11 for v in lo) and all(0 <= K - c < 32 for c in pc)     # the key fits 16 bits
    small = sorted(ids, key=lambda i: (K - pc[i], lo[i], i))
    assert P.expected_rows(masks, K, P.SMALL).tolist() == small
    assert P.popcount(masks).tolist() == pc
    nbr = np.where((masks[:, None] >> np.arange(K, dtype=np.uint32)[None]) & 1, 5, -1)
    assert np.array_equal(P.masks_of(nbr), masks)


def test_radix_layout_is_the_fewest_passes_of_8_to_10_bit_digits():
    for bits in range(1, 33):
        passes = next(p for p in range(1, 5) if 10 * p >= bits)
        db = next(d for d in (8, 9, 10) if d * passes >= bits)
        assert P.radix_layout(bits) == (passes, db), bits
    assert P.radix_layout(27) == (3, 9) and P.radix_layout(8) == (1, 8) and P.radix_layout(32) == (4, 8)


def test_expect_plan_form_at_every_threshold():
    f3, K = (3, 3, 3), 27
    base = dict.fromkeys(P.PLAN_FIELDS, 0)

    def want(**kw):
        return dict(base, **kw)
    # single-workgroup / radix sort at 8192 rows, with the masks of the probes (kind 0) or of the finalisation
    for n, fam, pa, db in ((8191, 2, 0, 0), (8192, 2, 0, 0), (8193, 3, 3, 9)):
        nb = (n + 31) // 32
        assert P.expect_plan_form(0, n, K, f3) == want(family=fam, masks=1, probe=1, K=K, n_rows=n, n_bound=n, n_blk=nb,
                                                       passes=pa, digit_bits=db)
        assert P.expect_plan_form(2, n, K, f3) == want(family=fam, K=K, n_rows=n, n_bound=n, n_blk=nb, passes=pa,
                                                       digit_bits=db)
        assert P.expect_plan_form(0, n, 1, (1, 1, 1), probe_mode=2) == want(family=1, K=1, n_rows=n, n_bound=n, n_blk=nb)
    assert P.expect_plan_form(1, 8193, 32, (1, 1, 32), grid_entries=9000) == want(
        family=3, K=32, n_rows=8193, n_bound=8193, n_blk=257, passes=4, digit_bits=8, grid=2)
    assert P.expect_plan_form(1, 8193, 8, (2, 2, 2), grid_entries=9000)["passes"] == 1
    # blocks of 32
    assert [P.expect_plan_form(0, n, K, f3)["n_blk"] for n in (31, 32, 33)] == [1, 1, 2]
    # the automatic half-probe form at 262144 sites (bound); the switch; filters that cannot take it
    for n, probe in ((262143, 1), (262144, 2), (262145, 2)):
        assert P.expect_plan_form(0, n, K, f3)["probe"] == probe
        assert P.expect_plan_form(0, n, K, f3, probe_mode=1)["probe"] == 1
        assert P.expect_plan_form(0, n, K, f3, probe_mode=2)["probe"] == 2
        assert P.expect_plan_form(0, n, 8, (2, 2, 2), probe_mode=2)["probe"] == 1
        assert P.expect_plan_form(0, n - 100, K, f3, prefetch_points=n)["probe"] == probe
    assert P.expect_plan_form(0, 100, K, f3, probe_mode=2)["probe"] == 2
    assert P.expect_plan_form(0, 100, 3, (1, 1, 3), probe_mode=2)["probe"] == 2
    assert P.expect_plan_form(0, 100, 9, (3, 3, 1), probe_mode=2)["probe"] == 2
    # the prefetched plan: radix by the point bound whatever the row count
    assert P.expect_plan_form(0, 17, K, f3, prefetch_points=33) == want(family=4, masks=1, probe=1, K=K, n_rows=17, n_bound=33,
                                                                        n_blk=1, passes=3, digit_bits=9)
    # grid builds at 4096 candidate entries
    for e, grid in ((0, 3), (1, 1), (4095, 1), (4096, 1), (4097, 2)):
        assert P.expect_plan_form(1, 33 if e else 0, 8, (2, 2, 2), grid_entries=e)["grid"] == grid
    assert P.expect_plan_form(1, 0, 8, (2, 2, 2), grid_entries=0)["family"] == 0
    assert P.max_out((2, 2, 2), (2, 2, 2), (32, 32, 16)) == 1 and P.max_out((3, 3, 3), (2, 2, 2), (32, 32, 16)) == 8
    assert P.max_out((1, 1, 32), (1, 1, 1), (128, 128, 1)) == 1


# ------------------------------------------------------------------------------------------------ the checks
def _mutable(plan):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in plan.items()}


def _classes(plan, masks):
    """positions of every mask class of the plan, in plan order"""
    n = plan["n_rows"]
    pm = masks[plan["rows"][:n]]
    return {int(m): np.flatnonzero(pm == m) for m in np.unique(pm)}, pm


@pytest.mark.parametrize("family", [P.SMALL, P.RADIX])
def test_every_mutation_of_a_correct_plan_is_rejected(family):
    n = 700                                                    # 21 full blocks and a tail of 28 rows + 4 padding slots
    nbr, masks, _ = P.subm_reference("structured", n, (3, 3, 3))
    K = 27
    good = P.synth_plan(nbr, family)
    P.check_plan_valid(good, nbr)
    P.check_plan_order(good, masks, family)
    cls, pm = _classes(good, masks)
    big = max(cls.values(), key=len)
    assert len(big) >= 64

    def rejected(plan, check=P.check_plan_valid):
        with pytest.raises(AssertionError):
            check(plan, nbr) if check is P.check_plan_valid else check(plan, masks, family)

    # one blkmask bit dropped / one extra
    p = _mutable(good)
    b = int(np.flatnonzero(p["blkmask"])[3])
    p["blkmask"][b] &= p["blkmask"][b] - np.uint32(1)
    rejected(p)
    p = _mutable(good)
    b = int(np.flatnonzero(p["blkmask"] != (1 << K) - 1)[0])
    free = next(k for k in range(K) if not (int(p["blkmask"][b]) >> k) & 1)
    p["blkmask"][b] |= np.uint32(1 << free)
    rejected(p)
    # two rows of one class swapped (table and block masks consistent with the swap)
    p = _mutable(good)
    a, c = int(big[1]), int(big[40])
    p["rows"][[a, c]] = p["rows"][[c, a]]
    p["nbrT"][:, [a, c]] = p["nbrT"][:, [c, a]]
    rejected(p)
    rejected(p, P.check_plan_order)
    # one nbrT entry changed
    p = _mutable(good)
    k, pos = (int(v[5]) for v in np.nonzero(p["nbrT"] >= 0))
    p["nbrT"][k, pos] = (p["nbrT"][k, pos] + 1) % n
    rejected(p)
    p = _mutable(good)
    k, pos = (int(v[5]) for v in np.nonzero(p["nbrT"][:, :n] < 0))
    p["nbrT"][k, pos] = 0
    rejected(p)
    # a padding slot holding row 0 (the unpadded tail)
    p = _mutable(good)
    assert p["rows"][n] == -1
    p["rows"][n] = 0
    rejected(p)
    p = _mutable(good)
    p["nbrT"][13, n] = 0
    rejected(p)
    # a row listed twice (in place of a row of the same class, table consistent)
    p = _mutable(good)
    p["rows"][c] = p["rows"][a]
    p["nbrT"][:, c] = p["nbrT"][:, a]
    rejected(p)
    # two whole mask classes exchanged: still a valid plan, but not the defined order
    order = good["rows"][:n].copy()
    runs = np.flatnonzero(np.diff(pm.astype(np.int64)) != 0) + 1
    segs = np.split(np.arange(n), runs)
    i = next(j for j in range(len(segs) - 1) if len(segs[j]) > 1 and pm[segs[j][0]] != pm[segs[j + 1][0]])
    segs[i], segs[i + 1] = segs[i + 1], segs[i]
    order = order[np.concatenate(segs)]
    p = _mutable(good)
    p["rows"][:n] = order
    p["nbrT"][:, :n] = nbr[order].T
    full = np.zeros(p["n_blk"] * 32, np.uint32)
    full[:n] = masks[order]
    p["blkmask"] = np.bitwise_or.reduce(full.reshape(-1, 32), axis=1)
    P.check_plan_valid(p, nbr)
    rejected(p, P.check_plan_order)


# ------------------------------------------------------------------------------------------------ the scenes
def _distinct_popcounts(masks):
    return np.unique(P.popcount(masks)).size


@pytest.mark.parametrize("scene,n", [("blob", n) for n in P.SUBM_COUNTS if n >= 8192] + [("two", 8193)])
def test_blob_scenes_have_many_masks_and_colliding_hashed_keys(scene, n):
    _, masks, _ = P.subm_reference(scene, n, (3, 3, 3))
    distinct = np.unique(masks)
    keys = P.small_key(distinct, 27)
    _, per_key = np.unique(keys, return_counts=True)
    shared = int((per_key >= 2).sum())
    print(scene, n, "masks", distinct.size, "keys shared by two or more masks", shared)
    assert distinct.size >= 1000 and shared >= 100


@pytest.mark.parametrize("n", [n for n in P.SUBM_COUNTS if n >= 127])
def test_structured_scenes_have_a_class_across_a_block_boundary(n):
    """(a class of 64 rows needs a scene of more than 64 sites: the smaller structured scenes are exempt)"""
    nbr, masks, _ = P.subm_reference("structured", n, (3, 3, 3))
    family = P.expect_plan_form(0, n, 27, (3, 3, 3))["family"]
    rows = P.expected_rows(masks, 27, family)
    pm = masks[rows]
    best = 0
    for m in np.unique(masks):
        pos = np.flatnonzero(pm == m)
        if pos.size >= 64 and pos[0] // 32 != pos[-1] // 32:
            best = max(best, pos.size)
    assert best >= 64
    assert np.unique(masks).size <= 200                   # few masks


def test_scenes_of_33_rows_or_more_have_two_popcounts():
    for scene, counts in (("blob", P.SUBM_COUNTS), ("structured", P.SUBM_COUNTS), ("border", P.EXTRA_COUNTS),
                          ("two", P.EXTRA_COUNTS)):
        for n in counts:
            for filt in P.SUBM_FILTERS:
                nbr, masks, total = P.subm_reference(scene, n, filt)
                assert nbr.shape == (n, int(np.prod(filt))) and total == int((nbr >= 0).sum())
                if n >= 33:
                    assert _distinct_popcounts(masks) >= 2, (scene, n, filt)
    for name in P.GEOMETRIES:
        for n_out in P.STRIDED_OUT_COUNTS:
            lo, nbr, dec, _ = P.strided_reference(name, ("out", n_out))
            assert lo.shape[0] == n_out == nbr.shape[0] <= dec.shape[0]
            if n_out >= 33:
                assert _distinct_popcounts(P.masks_of(nbr)) >= 2, (name, n_out)
        for n_in in P.DECONV_IN_COUNTS:
            _, nbr, dec, _ = P.strided_reference(name, ("in", n_in))
            assert dec.shape[0] == n_in
            dm = P.masks_of(dec)
            if name == "f3s2":
                assert _distinct_popcounts(dm) >= 2
            else:       # one output per input site by construction: every row has one offset, the classes are the offsets
                assert (P.popcount(dm) == 1).all() and np.unique(dm).size >= 4


def test_border_and_two_example_scenes_are_what_they_claim():
    for n in P.EXTRA_COUNTS:
        c, size = P.subm_scene("border", n)
        hi = np.asarray(size) - 1
        assert (((c[:, :3] == 0) | (c[:, :3] == hi)).any(1)).all()
        assert (((c[:, :3] == 0) | (c[:, :3] == hi)).all(1)).sum() == 8
        for d in range(3):
            assert (c[:, d] == 0).any() and (c[:, d] == hi[d]).any()
        c, size = P.subm_scene("two", n)
        a, b = c[c[:, 3] == 0], c[c[:, 3] == 1]
        assert a.shape[0] + b.shape[0] == n and b.shape[0] >= n // 2
        assert {tuple(r) for r in b[:, :3].tolist()} <= {tuple(r) for r in a[:, :3].tolist()}
        nbr, _, _ = P.subm_reference("two", n, (3, 3, 3))
        src, k = np.nonzero(nbr >= 0)
        assert (c[nbr[src, k], 3] == c[src, 3]).all()                   # no rule crosses the examples


@pytest.mark.parametrize("points", P.PREFETCH_POINTS)
def test_prefetch_scenes_have_duplicates(points):
    import oracle
    coords = P.duplicated_points(points, points)
    assert coords.shape == (points, 4)
    _, loc = oracle.input_sites(coords)
    if points >= 33:                                      # (one point is one site)
        assert loc.shape[0] <= 0.75 * points
    assert loc.shape[0] == (points + 1) // 2


def test_strided_scenes_reach_both_grid_builds():
    for name, (filt, stride, _, out_size) in P.GEOMETRIES.items():
        grids = set()
        for n_out in P.STRIDED_OUT_COUNTS:
            n_in = P.strided_coords(name, ("out", n_out)).shape[0]
            grids.add(P.expect_plan_form(1, n_out, int(np.prod(filt)), filt,
                                         grid_entries=n_in * P.max_out(filt, stride, out_size))["grid"])
        assert grids == {P.GRID_SMALL, P.GRID_TILED}, name
