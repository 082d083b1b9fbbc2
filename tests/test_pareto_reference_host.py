"""CPU: the numpy restatements of tests/pareto_reference.py against what the reference's DataProcess computed on the
point sets of tests/golden/pareto_reference.npz (make_pareto_golden.py): the selection contract reproduces
filter_pareto_front's array exactly, points and order; gd / igd / spread within their stated bounds."""
import os

import numpy as np
import pytest

from tests import pareto_reference as R


@pytest.fixture(scope="module")
def sets():
    return R.golden_sets()


def test_golden_covers_the_stated_shapes(sets):
    assert len(sets) >= 300
    assert {s["C"] for s in sets} == {1, 2, 3, 17, 64, 65, 130} and {s["D"] for s in sets} == {1, 2, 3, 4}
    assert {s["range"] for s in sets} == {2, 4, 9, 40}
    assert any(len(s["front"]) == 1 for s in sets) and max(len(s["front"]) for s in sets) >= 12
    assert any(np.isnan(s["spread"]) for s in sets) and any(np.isfinite(s["spread"]) for s in sets)
    assert os.path.getsize(R.GOLDEN) < 100 * 1024


def test_select_reproduces_filter_pareto_front(sets):
    for s in sets:
        for pts, want in ((s["points"], s["front"]), (np.concatenate([s["points"], s["other"]]), s["true_front"])):
            index, count, mask = R.select(pts[:, None, :])
            n = int(count[0])
            what = (s["C"], s["D"], s["range"], s["seed"])
            assert n == len(want) and np.all(index[0, n:] == -1), what
            assert np.array_equal(pts[index[0, :n]], want), what
            assert np.array_equal(R.front_points(pts[:, None, :], index)[0, :n], want), what
            assert mask.sum() == n and np.all(mask[index[0, :n], 0] == 1), what
            # of equal points the lowest index survives
            for c in index[0, :n]:
                assert not np.any(np.all(pts[:c] == pts[c], axis=1)), what


def test_select_cap_valid_and_nan():
    rs = np.random.RandomState(3)
    obj = rs.randint(0, 6, (40, 7, 3)).astype(np.float64)
    obj[rs.rand(40, 7) < 0.2, 1] = np.nan
    valid = (rs.rand(40, 7) < 0.7).astype(np.uint8)
    valid[:, 3] = 0
    full = R.select(obj, valid)
    keep = (valid != 0) & ~np.isnan(obj).any(axis=2)
    assert full[1][3] == 0 and np.all(full[0][3] == -1) and np.all(full[2][:, 3] == 0)
    assert np.all(full[2][~keep] == 0)
    for i in range(7):
        # the same front from the candidates alone, renumbered
        ids = np.flatnonzero(keep[:, i])
        if ids.size:
            sub = R.select(obj[ids, i][:, None, :])
            assert np.array_equal(ids[sub[0][0, :sub[1][0]]], full[0][i, :full[1][i]])
    capped = R.select(obj, valid, 2)
    assert np.array_equal(capped[1], full[1]) and np.array_equal(capped[2], full[2])
    assert np.array_equal(capped[0], full[0][:, :2]) and np.any(full[1] > 2)


def test_metrics_within_their_bounds_of_the_reference(sets):
    for s in sets:
        what = (s["C"], s["D"], s["range"], s["seed"])
        for name, got in (("gd", R.gd(s["true_front"], s["front"])), ("igd", R.igd(s["true_front"], s["front"])),
                          ("spread", R.spread(s["front"], s["true_front"]))):
            value, bound = got
            want = s[name]
            print(name, what, value, want, bound)
            if np.isnan(want):
                assert np.isnan(value), (name, what)
            else:
                assert abs(value - want) <= bound, (name, what, value, want, bound)
