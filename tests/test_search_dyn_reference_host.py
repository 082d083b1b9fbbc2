"""CPU: tests/search_dyn_reference.py, the numpy statement of fjsp_schedule_search_dyn, on the recorded MO_DFJSP shops
gen8802 (8 rows) and gen8801 (76 rows): rounds = 0, traces that replay through schedule.apply_moves and the decode's
reference to the histories and the returned plans, descents that never rise, the tabu run's best, shards, aspiration --
and the new symbols' declaration, export and host refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import decode_dyn_reference as DD
from tests import search_dyn_cases as SC
from tests import search_dyn_reference as SD

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, Q, N = 6, 12, 3
MODES = [(col, ac) for col in (SD.MAKESPAN, SD.TARDINESS, SD.ENERGY) for ac in (SD.STRICT, SD.SIDEWAYS, SD.TABU)]


@pytest.fixture(scope="module")
def shops():
    """{name: ([instance per env], plans int32[N][cap][3])}: random plans of the two smallest recorded shops."""
    eps = SC.episodes()
    out = {}
    for name, seed in (("gen8802", 4), ("gen8801", 5)):
        a, cap = SC.shop(eps, name)
        out[name] = ([a] * N, SC.random_plans(a, N, seed, cap))
    assert out["gen8802"][1].shape == (N, 8, 3) and out["gen8801"][1].shape == (N, 76, 3)
    return out


@pytest.fixture(scope="module")
def runs(shops):
    """Every objective and accept mode on both shops, once: {(name, objective, accept): result}."""
    return {(name, col, ac): SD.search(insts, plans, ROUNDS, Q, col, ac, 2, 11) for name, (insts, plans) in shops.items() for col, ac in MODES}


def test_rounds_zero_returns_the_input_and_its_three_objectives(shops):
    for name, (insts, plans) in shops.items():
        for col, ac in MODES:
            res = SD.search(insts, plans, 0, Q, col, ac, 2, 11)
            first = DD.decode(insts, plans)
            assert np.array_equal(res["plan"], plans) and res["plan"].dtype == np.int32
            assert res["objective"].dtype == np.int64 and np.array_equal(res["objective"], first["objective"][:, 0])
            assert res["history"].shape == (1, N) and np.array_equal(res["history"][0], first["objective"][:, 0, col])
            assert res["trace"].shape == (0, N, 3) and np.all(res["accepted"] == 0) and np.all(res["status"] == 0)


@pytest.mark.parametrize("name", ["gen8802", "gen8801"])
def test_the_trace_replays(shops, runs, name):
    """Each round's move applied with schedule.apply_moves, the plan decoded with DD.decode: the history row by row, the
    returned plan (tabu: the best of the replay, the earliest among equals) and its objective."""
    import torch
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    insts, plans = shops[name]
    improved = 0
    for col, ac in MODES:
        res = runs[(name, col, ac)]
        assert np.all(res["status"] == 0) and res["history"].shape == (ROUNDS + 1, N)
        pl = torch.from_numpy(plans)
        now = DD.decode(insts, plans)["objective"][:, 0]
        assert np.array_equal(res["history"][0], now[:, col])
        best, best_plan = now.copy(), plans.copy()
        for t in range(ROUNDS):
            pl = sch.apply_moves(pl, torch.from_numpy(res["trace"][t][:, None]))[:, 0]
            one = DD.decode(insts, pl.numpy())
            assert np.all(one["status"] == 0)
            now = one["objective"][:, 0]
            assert np.array_equal(res["history"][t + 1], now[:, col]), (col, ac, t)
            better = now[:, col] < best[:, col]
            best[better], best_plan[better] = now[better], pl.numpy()[better]
        assert np.array_equal(res["plan"], best_plan if ac == SD.TABU else pl.numpy()), (col, ac)
        assert np.array_equal(res["objective"], best if ac == SD.TABU else now), (col, ac)
        assert np.array_equal(res["accepted"], (res["trace"][..., 0] != 0).sum(0))
        improved += int((res["history"][-1] < res["history"][0]).sum())
    assert improved > 0


def test_descents_never_rise_and_tabu_returns_its_best(runs):
    for (name, col, ac), res in runs.items():
        h = res["history"]
        if ac == SD.TABU:
            assert np.array_equal(res["objective"][:, col], h.min(0)), (name, col)
        else:
            assert np.all(np.diff(h, axis=0) <= 0), (name, col, ac)
            assert np.array_equal(res["objective"][:, col], h[-1])
            if ac == SD.STRICT:
                assert np.array_equal((np.diff(h, axis=0) < 0).sum(0), res["accepted"])


def test_a_shard_equals_its_envs_of_the_whole_batch(shops):
    insts, plans = shops["gen8801"]
    for col in (SD.MAKESPAN, SD.ENERGY):
        whole = SD.search(insts, plans, 5, 8, col, SD.TABU, 2, 21)
        part = SD.search(insts[1:], plans[1:], 5, 8, col, SD.TABU, 2, 21, first_env=1)
        other = SD.search(insts[1:], plans[1:], 5, 8, col, SD.TABU, 2, 21, first_env=0)
        for key in SD.KEYS:
            sl = (slice(None), slice(1, None)) if key in ("history", "trace") else (slice(1, None),)
            assert np.array_equal(part[key], whole[key][sl]), (col, key)
        assert not np.array_equal(other["trace"], part["trace"])


def test_aspiration_takes_a_tabu_candidate():
    """With a tenure beyond the rounds every moved row stays tabu, so a later move of one is taken by aspiration alone."""
    a, cap = SC.shop(SC.episodes(), "gen8801")
    k = SC.ASPIRATION
    res = SD.search([a] * 4, SC.random_plans(a, 4, 5, cap), k["rounds"], k["n_cand"], SD.MAKESPAN, SD.TABU, k["tenure"], k["seed"])
    assert sum(len(x) for x in res["aspired"]) > 0


def test_a_plan_that_does_not_decode(shops):
    insts, plans = shops["gen8802"]
    bad = plans.copy()
    bad[1, -1] = -1                                                               # operations missing
    res = SD.search(insts, bad, 4, 8, SD.ENERGY, SD.SIDEWAYS, 0, 1)
    good = SD.search(insts, plans, 4, 8, SD.ENERGY, SD.SIDEWAYS, 0, 1)
    assert res["status"].tolist() == [0, 2, 0] and np.array_equal(res["plan"][1], bad[1])
    assert np.all(res["history"][:, 1] == -1) and res["objective"][1].tolist() == [-1, -1, -1] and res["accepted"][1] == 0
    assert np.all(res["trace"][:, 1] == 0)
    for key in SD.KEYS:
        keep = [0, 2]
        x, y = (res[key][:, keep], good[key][:, keep]) if key in ("history", "trace") else (res[key][keep], good[key][keep])
        assert np.array_equal(x, y), key


def test_symbols_are_declared_exported_and_refuse_without_a_device(built):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    lib = _capi.lib()
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    assert _capi.SIGNATURES["fjsp_schedule_search_dyn"] == (C.c_int, [vp, vp, i32, i32, i32, i32, i32, u64, i64, vp, vp, vp, vp, vp, vp, vp])
    assert _capi.SIGNATURES["fjsp_schedule_search_dyn_lds"] == (C.c_int, [vp])
    header = open(os.path.join(REPO, "include", "fjsp_amd.h")).read()
    for name in ("fjsp_schedule_search_dyn", "fjsp_schedule_search_dyn_lds"):
        assert "int %s(" % name in header and hasattr(lib, name)
    assert lib.fjsp_schedule_search_dyn(None, None, 1, 1, 0, 0, 0, 0, 0, None, None, None, None, None, None, None) == _capi.FJSP_E_ARG
    assert "fjsp_schedule_search_dyn: null" in lib.fjsp_last_error().decode()
    assert lib.fjsp_schedule_search_dyn_lds(None) == 0
    assert sch.SEARCH_DYN_OBJECTIVES == ("makespan", "tardiness", "energy") and sch.SEARCH_OBJECTIVES == ("makespan", "tardiness")
