"""CPU: tests/search_reference.py, the numpy statement of fjsp_schedule_search: its draw stream against the library's
(fjsp_search_draws), and the search itself on Mk01 and on four 10 x 5 instances -- histories, traces that replay to the
returned plans, feasible plans, the tabu run's best, shards -- and the new symbols' declaration and host refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import decode_reference as D
from tests import critical_reference as R
from tests import helpers as H
from tests import schedule_fixture as F
from tests import search_reference as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, Q = 10, 16
MODES = [(nb, ac) for nb in (S.UNIFORM, S.CRITICAL, S.MIXED) for ac in (S.STRICT, S.SIDEWAYS, S.TABU)]


@pytest.fixture(scope="module")
def shops(built):
    """{name: (variant, [instance per env], plans int32[N][cap][3])}: Mk01 from its recorded schedule and from random plans
    (4 envs), four 10 x 5 instances under 4 envs from random plans."""
    variant, eps = F.load()["mk01"]
    mk01 = eps[0]["inst"]
    rs = np.random.RandomState(5)
    cap = len(eps[0]["table"])
    plans = np.stack([D.plan_from_table(eps[0]["table"], cap)] + [D.random_plan(mk01, rs, cap) for _ in range(3)])
    s = H.gen_10x5(4, 4200)
    arrs = [s.arrays(i) for i in range(4)]
    cap10 = max(D.plan_length(D.random_plan(a, rs)) for a in arrs)
    return {"mk01": (variant, [mk01] * 4, plans), "10x5": (0, arrs, np.stack([D.random_plan(a, rs, cap10) for a in arrs]))}


@pytest.fixture(scope="module")
def runs(shops):
    """Every mode on both shops, once: {(name, neighbourhood, accept): result}."""
    return {(name, nb, ac): S.search(insts, variant, plans, ROUNDS, Q, 0, nb, ac, 3, 11)
            for name, (variant, insts, plans) in shops.items() for nb, ac in MODES}


def test_stream_equals_the_library(built):
    """The Python stream is the library's, also at an env id at or above 2^32 and where the draw index wraps."""
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    for seed, env, first in [(0, 0, 0), (1, 1, 0), (2 ** 64 - 1, 7, 12345), (0x1234567890ABCDEF, 2 ** 32, 0), (99, 2 ** 32 + 5, 2 ** 32 - 3),
                             (5, 2 ** 40 + 3, 2 ** 32 - 1), (-1 & S.MASK, 3, 2 ** 31)]:
        got = sch.search_draws(seed, env, first, 6)
        assert got.dtype == np.uint64 and np.array_equal(got, S.draws(seed, env, first, 6)), (seed, env, first)
    assert np.array_equal(sch.search_draws(99, 2 ** 32 + 5, 0, 4), sch.search_draws(99, 5, 0, 4))       # the id is taken modulo 2^32
    assert not np.array_equal(sch.search_draws(99, 5, 0, 4), sch.search_draws(99, 6, 0, 4))
    assert not np.array_equal(sch.search_draws(99, 5, 0, 4), sch.search_draws(98, 5, 0, 4))
    assert len(sch.search_draws(1, 1, 0, 0)) == 0
    assert _capi.lib().fjsp_search_draws(1, 1, 0, 2, None) == _capi.FJSP_E_ARG
    assert S.pick(2 ** 64 - 1, 7) == 6 and S.pick(0, 7) == 0 and S.pick(2 ** 63, 1) == 0


def test_symbols_are_declared_and_refuse_without_a_device(built):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    lib = _capi.lib()
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    assert _capi.SIGNATURES["fjsp_schedule_search"] == (C.c_int, [vp, vp, i32, i32, i32, i32, i32, i32, u64, i64, vp, vp, vp, vp, vp, vp, vp])
    assert lib.fjsp_schedule_search(None, None, 1, 1, 0, 0, 0, 0, 0, 0, None, None, None, None, None, None, None) == _capi.FJSP_E_ARG
    assert lib.fjsp_schedule_search_lds(None) == 0
    header = open(os.path.join(REPO, "include", "fjsp_amd.h")).read()
    assert "#define FJSP_SEARCH_STREAM 0x%016XULL" % S.STREAM in header


@pytest.mark.parametrize("name", ["mk01", "10x5"])
def test_reference_runs_are_searches(shops, runs, name):
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    variant, insts, plans = shops[name]
    N, cap = plans.shape[0], plans.shape[1]
    improved = 0
    for nb, ac in MODES:
        res = runs[(name, nb, ac)]
        assert np.all(res["status"] == 0)
        h = res["history"]
        assert h.shape == (ROUNDS + 1, N)
        if ac != S.TABU:
            assert np.all(np.diff(h, axis=0) <= 0), (nb, ac)                      # a descent never rises
            if ac == S.STRICT:
                assert np.array_equal((np.diff(h, axis=0) < 0).sum(0), res["accepted"])
            assert np.array_equal(res["objective"][:, 0], h[-1])
        else:
            assert np.array_equal(res["objective"][:, 0], h.min(0)), (nb, ac)     # the best plan seen
            assert np.all(res["accepted"] == (res["trace"][..., 0] != 0).sum(0))
        improved += int((h[-1] < h[0]).sum())
        for e in range(N):
            # the trace replays to the returned plan (tabu: to its best prefix), every plan on the way decodes to the history
            pl, best, best_plan = plans[e], h[0, e], plans[e]
            for t in range(ROUNDS):
                if nb != S.UNIFORM:
                    pl = D.plan_from_table(R.begin_order(D.decode_one(insts[e], variant, pl, None, cap)["table"]), cap)
                pl = R.materialise_moved(pl, res["trace"][t, e], cap)
                one = D.decode_one(insts[e], variant, pl, None, cap)
                assert one["status"] == 0 and one["objective"][0] == h[t + 1, e], (nb, ac, e, t)
                if one["objective"][0] < best:
                    best, best_plan = one["objective"][0], pl
            assert np.array_equal(res["plan"][e], best_plan if ac == S.TABU else pl), (nb, ac, e)
            final = D.decode_one(insts[e], variant, res["plan"][e], None, cap)
            assert np.array_equal(final["objective"], res["objective"][e])
            assert sch.validate(insts[e], final["table"][:final["length"]], variant) == [], (nb, ac, e)
    assert improved > 0


def test_a_shard_equals_its_envs_of_the_whole_batch(shops):
    for name in ("mk01", "10x5"):
        variant, insts, plans = shops[name]
        whole = S.search(insts, variant, plans, 6, 8, 0, S.MIXED, S.TABU, 2, 21)
        part = S.search(insts[1:3], variant, plans[1:3], 6, 8, 0, S.MIXED, S.TABU, 2, 21, first_env=1)
        other = S.search(insts[1:3], variant, plans[1:3], 6, 8, 0, S.MIXED, S.TABU, 2, 21, first_env=0)
        for key in S.KEYS:
            sl = (slice(None), slice(1, 3)) if key in ("history", "trace") else (slice(1, 3),)
            assert np.array_equal(part[key], whole[key][sl]), (name, key)
        assert not np.array_equal(other["trace"], part["trace"]), name


def test_rounds_zero_and_a_plan_that_does_not_decode(shops):
    variant, insts, plans = shops["mk01"]
    res = S.search(insts, variant, plans, 0, 8, 0, S.CRITICAL, S.TABU, 2, 1)
    assert np.array_equal(res["plan"], plans) and res["history"].shape == (1, 4) and np.all(res["accepted"] == 0)
    bad = plans.copy()
    bad[2, -1] = -1                                                               # operations missing
    res = S.search(insts, variant, bad, 4, 8, 0, S.UNIFORM, S.SIDEWAYS, 0, 1)
    good = S.search(insts, variant, plans, 4, 8, 0, S.UNIFORM, S.SIDEWAYS, 0, 1)
    assert res["status"].tolist() == [0, 0, 2, 0] and np.array_equal(res["plan"][2], bad[2])
    assert np.all(res["history"][:, 2] == -1) and res["objective"][2].tolist() == [-1, -1] and res["accepted"][2] == 0
    for key in S.KEYS:
        keep = [0, 1, 3]
        a, b = (res[key][:, keep], good[key][:, keep]) if key in ("history", "trace") else (res[key][keep], good[key][keep])
        assert np.array_equal(a, b), key
