"""tests/ploc_ref.py alone, without a GPU: the restatement's invariants, and that every fixture of tests/test_ploc_trees.py holds what it
is there for -- its area ratio far enough from every adoption threshold that float rounding on the device cannot flip an adoption."""
import numpy as np
import pytest

import ploc_ref as pr

RADII = sorted({pr.tuned(r, 8, 1, pr.PLOC_R_MAX) for r in pr.RADII})          # (1, 8, 31, 32)
THRESHOLDS = sorted({0.01 * pr.tuned(p, 90, 0, 1000) for p in pr.ADOPT_PCTS})   # (0, 0.9, 0.95, 10)


def test_tuned_is_pt_tuned():
    assert [pr.tuned(v, 8, 1, 32) for v in (-1, 0, 1, 8, 32, 33)] == [8, 1, 1, 8, 32, 32]
    assert [pr.tuned(v, 90, 0, 1000) for v in (-1, 0, 95, 1000, 2000)] == [90, 0, 95, 1000, 1000]


def test_fixture_sizes_are_the_ones_the_kernels_branch_on(pt, orc):
    n = {name: len(pr.arrays(pt, name)[1]) // 3 for name in pr.FIXTURES}
    assert n["soup2049"] == pr.PLOC_MIN_TRIS and n["soup2305"] == 9 * pr.TB + 1 and n["tiles"] == 9 * pr.TB
    assert n["stadium"] == 3394                              # above the limit, and small enough for a brute-force oracle in a second
    v = pr.arrays(pt, "tiles")[0].reshape(-1, 3, 3)
    ext = (v.max(1) - v.min(1)).astype(np.float32)
    assert len(np.unique(ext[:, :2], axis=0)) == 1 and (ext[:, 2] == 0).all()      # every leaf box the same size, bit for bit ...
    llo, lhi, _, _ = pr.lbvh_boxes(orc.Scene(*pr.arrays(pt, "tiles")).bvh_nodes())
    assert len(np.unique((lhi - llo).astype(np.float32), axis=0)) == 1           # ... with the leaf pad too


@pytest.mark.parametrize("name", pr.FIXTURES)
def test_restatement_merges_n_minus_one_clusters_and_repeats_itself(pt, orc, name):
    v, i, f = pr.arrays(pt, name)
    llo, lhi, nlo, nhi = pr.lbvh_boxes(orc.Scene(v, i, f).bvh_nodes())
    n = len(llo)
    assert n == len(i) // 3 and (llo <= lhi).all() and (nlo <= nhi).all()
    for radius in RADII:
        a, b = pr.ploc(llo, lhi, radius), pr.ploc(llo, lhi, radius)
        assert sum(a["rounds"]) == n - 1 and min(a["rounds"]) >= 1, (name, radius)
        assert a["area"] == b["area"] and a["rounds"] == b["rounds"] and (a["children"] == b["children"]).all()
        kids = a["children"]
        assert kids.shape == (n - 1, 2) and sorted(kids.ravel().tolist()) == list(range(2 * n - 2))   # every cluster but the root merged once
        assert (kids < n + np.arange(n - 1)[:, None]).all()                                            # ... into a later node
        assert a["area"] > 0


@pytest.mark.parametrize("name", pr.FIXTURES)
def test_fixture_ratios_stay_clear_of_every_adoption_threshold(pt, orc, name):
    for radius in RADII:
        ref = pr.fixture_reference(pt, orc, name, radius)
        print(f"{name}: n = {ref['n']}, radius {radius}: area_ploc / area_lbvh = {ref['ratio']:.4f}, {len(ref['rounds'])} rounds, "
              f"info values {pr.info_value(ref['area_lbvh'], ref['root'])} / {pr.info_value(ref['area_ploc'], ref['root'])}")
        for thr in THRESHOLDS:
            assert abs(ref["ratio"] - thr) >= 1e-3, (name, radius, ref["ratio"], thr)
        assert pr.adopted(ref["area_ploc"], ref["area_lbvh"], 1000) and not pr.adopted(ref["area_ploc"], ref["area_lbvh"], 0)


def test_fixtures_hold_what_they_are_there_for(pt, orc):
    """The stadium is adopted by the default rule at every radius, the uniform soups by none but the forced one, and the 95 % rule
    separates the two soups at radius 8."""
    for radius in RADII:
        assert pr.fixture_reference(pt, orc, "stadium", radius)["ratio"] < 0.9
        for name in ("soup2049", "soup2305", "tiles"):
            assert pr.fixture_reference(pt, orc, name, radius)["ratio"] > 0.9, (name, radius)
    assert pr.fixture_reference(pt, orc, "soup2049", 8)["ratio"] < 0.95 < pr.fixture_reference(pt, orc, "soup2305", 8)["ratio"]


def test_parity_term_pairs_up_a_grid_of_equal_tiles(pt, orc):
    """Every union area of neighbouring equal tiles ties.  "Lowest index wins" would make every cluster point left -- one merge per round;
    the parity of the pair's lower index pairs them up.  Round one is not the witness (the two halves of a quad share one box, so they
    choose each other under any rule); the rounds after it, over 1152 equal quads, are."""
    v, i, f = pr.arrays(pt, "tiles")
    llo, lhi, _, _ = pr.lbvh_boxes(orc.Scene(v, i, f).bvh_nodes())
    for radius in RADII:
        ref = pr.fixture_reference(pt, orc, "tiles", radius)
        m = ref["n"]
        assert ref["rounds"][0] >= m // 4, (radius, ref["rounds"][:4])
        assert len(ref["rounds"]) < 64
        if radius > 1:
            plain = pr.ploc(llo, lhi, radius, tie="none")
            assert ref["rounds"][1] >= 2 * plain["rounds"][1], (radius, ref["rounds"][:4], plain["rounds"][:4])


@pytest.mark.parametrize("name,radius,wrong", [("tiles", 8, dict(tie="odd")), ("tiles", 32, dict(tie="odd")), ("tiles", 8, dict(tie="none")),
                                               ("tiles", 8, dict(block=pr.TB)), ("tiles", 32, dict(block=pr.TB)),
                                               ("stadium", 1, dict(block=pr.TB)), ("stadium", 8, dict(block=pr.TB)), ("stadium", 32, dict(block=pr.TB)),
                                               ("soup2049", 8, dict(block=pr.TB)), ("soup2305", 1, dict(block=pr.TB)),
                                               ("soup2305", 8, dict(block=pr.TB)), ("soup2305", 32, dict(block=pr.TB))])
def test_area_sum_tells_a_wrong_neighbour_search_from_the_right_one(pt, orc, name, radius, wrong):
    """What the device comparison of tests/test_ploc_trees.py rests on: a k_ploc_nn whose parity tie goes the other way, or that sees no
    neighbour across a block edge, still makes a valid tree -- hit parity cannot see it -- but moves the area sum by far more than the
    one float32 ulp (2^-23 relative at most) that comparison allows."""
    v, i, f = pr.arrays(pt, name)
    llo, lhi, _, _ = pr.lbvh_boxes(orc.Scene(v, i, f).bvh_nodes())
    right = pr.fixture_reference(pt, orc, name, radius)["area_ploc"]
    bad = pr.ploc(llo, lhi, radius, **wrong)
    assert sum(bad["rounds"]) == len(llo) - 1                              # a valid tree all the same
    assert abs(bad["area"] / right - 1.0) > 2.0 ** -16, (name, radius, wrong, bad["area"] / right)


def test_refit_restatement_reproduces_the_oracles_boxes(pt, orc):
    """refit_lbvh over a tree's own triangles gives the tree back bit for bit: leaf pad, unions and child words as the builder's"""
    for name in ("soup2305", "stadium"):
        v, i, f = pr.arrays(pt, name)
        osc = orc.Scene(v, i, f)
        nodes, (_, prim) = osc.bvh_nodes(), osc.bvh_keys()
        out, a = pr.refit_lbvh(nodes, prim, v, i)
        assert out.tobytes() == nodes.tobytes() and a == pr.lbvh_area(nodes)


def test_one_ulp_helper():
    x = np.float32(14.959274)
    assert pr.within_one_ulp(x, x) and pr.within_one_ulp(np.nextafter(x, np.float32(99)), x)
    assert not pr.within_one_ulp(np.nextafter(np.nextafter(x, np.float32(99)), np.float32(99)), x)
