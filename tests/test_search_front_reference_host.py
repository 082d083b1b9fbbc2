"""CPU: tests/search_front_reference.py, the statement of fjsp_schedule_search_front, on the recorded MO_DFJSP shops gen8802
(8 rows) and gen8801 (76 rows) and on Mk01: the archive against the brute-force front of everything the search decoded,
replayed from the trace; unit weights against the single-objective references; drops at four slots and none at sixteen;
saturating weights; status 5 -- and the new symbols' declaration, export and host refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import decode_reference as D
from tests import schedule_fixture as F
from tests import search_dyn_reference as SD
from tests import search_front_cases as FC
from tests import search_front_reference as SF
from tests import search_reference as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCEPTS = (SF.STRICT, SF.SIDEWAYS, SF.TABU)
ROUNDS, Q, N = 6, 12, 3


@pytest.fixture(scope="module")
def eps():
    return FC.episodes()


@pytest.fixture(scope="module")
def small(eps):
    """gen8802: ([instance] * N, plans int32[N][8][3])."""
    a, cap = FC.shop(eps, "gen8802")
    return [a] * N, FC.random_plans(a, N, 4, cap)


@pytest.fixture(scope="module")
def mk01():
    """(variant, [instance] * N, plans): Mk01 from its recorded schedule and two random plans."""
    variant, eps = F.load()["mk01"]
    a = eps[0]["inst"]
    rs = np.random.RandomState(6)
    cap = len(eps[0]["table"])
    return variant, [a] * N, np.stack([D.plan_from_table(eps[0]["table"], cap)] + [D.random_plan(a, rs, cap) for _ in range(N - 1)])


def _replayed_vectors(inst, variant, plan, res, e, rounds, n_cand, seed, g):
    """Every vector env e's search decoded: the input plan's and, round by round on the plan that schedule.apply_moves makes
    of the trace, every status-0 candidate's."""
    import torch
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    cap = len(plan)
    first = SF.decode_one(inst, variant, plan, None, cap)
    vectors = [first["objective"]]
    pl = torch.from_numpy(np.ascontiguousarray(plan))[None]
    stream = S.env_stream(seed, g)
    for t in range(rounds):
        rows = pl[0].numpy()[:D.plan_length(pl[0].numpy())].astype(np.int64)
        vectors += [r["objective"] for _, _, r in SF.round_candidates(inst, variant, rows, t, n_cand, stream, cap) if r["status"] == 0]
        pl = sch.apply_moves(pl, torch.from_numpy(res["trace"][t, e][None, None]))[:, 0]
    return vectors


def _check_archive(insts, variant, plans, res, rounds, n_cand, seed):
    for e in range(len(insts)):
        members = FC.archive_set(res, e)
        assert len(set(members)) == len(members)                                   # distinct
        assert not any(SF.dominates(x, y) for x in members for y in members)       # mutually non-dominated
        assert res["front_dropped"][e] == 0
        assert set(members) == FC.brute_front(_replayed_vectors(insts[e], variant, plans[e], res, e, rounds, n_cand, seed, e)), e


@pytest.mark.parametrize("ac", ACCEPTS)
def test_the_archive_is_the_front_of_everything_decoded(eps, small, mk01, ac):
    a, plans = FC.gen8801(eps)
    k = FC.MATRIX
    res = SF.search([a] * 4, FC.VARIANT, plans, FC.weight_sets()["per_env"], k["rounds"], k["n_cand"], 64, ac, k["tenure"], k["seed"])
    assert np.all(res["status"] == 0) and min(res["entrants"]) > 0
    _check_archive([a] * 4, FC.VARIANT, plans, res, k["rounds"], k["n_cand"], k["seed"])
    insts, pl = small
    res = SF.search(insts, FC.VARIANT, pl, FC.weight_sets(N)["mixed"], ROUNDS, Q, 64, ac, 2, 11)
    _check_archive(insts, FC.VARIANT, pl, res, ROUNDS, Q, 11)
    variant, insts, pl = mk01
    res = SF.search(insts, variant, pl, np.array([[1, 1], [3, 1], [1, 0]]), ROUNDS, Q, 64, ac, 2, 11)
    assert res["front_obj"].shape == (N, 64, 2) and np.all(res["status"] == 0)
    _check_archive(insts, variant, pl, res, ROUNDS, Q, 11)


@pytest.mark.parametrize("ac", ACCEPTS)
def test_a_unit_weight_is_the_single_objective_search(eps, small, mk01, ac):
    a, plans = FC.gen8801(eps)
    cases = [([a] * 4, plans, 5, 16)] + [small + (ROUNDS, Q)]
    for insts, pl, rounds, n_cand in cases:
        for c in range(3):
            w = np.array([FC.UNITS[c]] * len(insts))
            got = SF.search(insts, FC.VARIANT, pl, w, rounds, n_cand, 8, ac, 2, 11)
            want = SD.search(insts, pl, rounds, n_cand, c, ac, 2, 11)
            for key in S.KEYS:
                assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (c, key)
    variant, insts, pl = mk01
    for c in range(2):
        got = SF.search(insts, variant, pl, np.array([FC.UNITS[c][:2]] * N), ROUNDS, Q, 8, ac, 2, 11)
        want = S.search(insts, variant, pl, ROUNDS, Q, c, S.UNIFORM, ac, 2, 11)
        for key in S.KEYS:
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (c, key)


def test_four_slots_drop_entrants_and_sixteen_do_not(eps):
    a, plans = FC.gen8801(eps)
    k = FC.DROPS
    w = FC.weight_sets()["mixed"]
    wide = SF.search([a] * 4, FC.VARIANT, plans, w, k["rounds"], k["n_cand"], 16, SF.TABU, k["tenure"], k["seed"])
    tight = SF.search([a] * 4, FC.VARIANT, plans, w, k["rounds"], k["n_cand"], 4, SF.TABU, k["tenure"], k["seed"])
    assert np.all(wide["front_dropped"] == 0) and max(wide["peak"]) > 4 and max(wide["peak"]) <= 16
    assert np.all(tight["front_dropped"] > 0) and sum(tight["left_for_dropped"]) > 0 and np.all(tight["front_count"] <= 4)
    for key in S.KEYS:                                                            # the archive decides nothing in the search
        assert np.array_equal(wide[key], tight[key]), key
    for e in range(4):                                                            # what survives is still mutually non-dominated
        members = FC.archive_set(tight, e)
        assert not any(SF.dominates(x, y) for x in members for y in members) and len(set(members)) == len(members)


def test_slots_are_stable_and_sources_name_their_round(eps):
    """A member found in round t by candidate q sits in one slot from then on: the archive of the search cut short by a
    round agrees, slot by slot, with the full search's wherever the member is still there."""
    a, plans = FC.gen8801(eps)
    k = FC.DROPS
    w = FC.weight_sets()["mixed"]
    last = k["rounds"] - 1
    full = SF.search([a] * 4, FC.VARIANT, plans, w, k["rounds"], k["n_cand"], 16, SF.TABU, k["tenure"], k["seed"])
    part = SF.search([a] * 4, FC.VARIANT, plans, w, last, k["n_cand"], 16, SF.TABU, k["tenure"], k["seed"])
    old = (full["front_src"][..., 0] < last) & (full["front_src"][..., 1] >= 0)
    assert old.any(1).sum() >= 3                                                  # (the seed: three envs keep a member of an earlier round)
    for key in ("front_src", "front_obj", "front_plan"):
        assert np.array_equal(full[key][old], part[key][old]), key
    held = full["front_src"][..., 1] >= 0
    assert np.all(full["front_src"][held][:, 0] < k["rounds"]) and np.all(full["front_src"][held][:, 1] < k["n_cand"])


def test_saturating_weights_take_the_lowest_unmasked_candidate(eps, small):
    insts, plans = small
    w = np.array([FC.SATURATING] * N, np.int64)
    assert SF.key_of(FC.SATURATING, (1, 0, 0)) == 2 ** 62 and SF.key_of(FC.SATURATING, (2, 1, 1)) == SF.KEY_MAX
    for ac in ACCEPTS:
        res = SF.search(insts, FC.VARIANT, plans, w, ROUNDS, Q, 16, ac, 1, 3)
        assert np.all(res["history"] == SF.KEY_MAX) and np.all(res["status"] == 0)
        if ac == SF.STRICT:
            assert np.all(res["accepted"] == 0)
            continue
        # sideways and tabu: every round takes the lowest q that decodes (tabu: and is no no-op and not tabu -- no aspiration,
        # nothing is below the best key); replay the rounds and name that q
        for e in range(N):
            rows = plans[e][:D.plan_length(plans[e])].astype(np.int64)
            ids, until = np.arange(len(rows)), np.zeros(len(rows), np.int64)
            stream = S.env_stream(3, e)
            for t in range(ROUNDS):
                first = None
                for q, move, r in SF.round_candidates(insts[e], FC.VARIANT, rows, t, Q, stream, len(plans[e])):
                    if r["status"] != 0:
                        continue
                    order, moved = S._order(rows, move)
                    noop = (move[0] == S.MOVE_MACHINE and move[2] == rows[move[1], 2]) or (move[0] != S.MOVE_MACHINE and order == list(range(len(rows))))
                    if ac == SF.TABU and (noop or any(until[ids[x]] > t for x in moved)):
                        continue
                    first = (move, order, moved)
                    break
                assert tuple(res["trace"][t, e]) == (first[0] if first else (0, 0, 0)), (ac, e, t)
                if first:
                    move, order, moved = first
                    until[ids[moved]] = t + 1 + 1
                    rows, ids = rows[order], ids[order]
                    if move[0] == S.MOVE_MACHINE:
                        rows[move[1], 2] = move[2]


def test_bad_weights_give_status_5_and_outrank_the_plan(small):
    insts, plans = small
    bad = plans.copy()
    bad[1, -1] = -1                                                               # operations missing: status 2
    w = np.array([[1, -1, 1], [0, 0, 0], [2, 0, 1]])
    res = SF.search(insts, FC.VARIANT, bad, w, 4, 8, 4, SF.SIDEWAYS, 0, 1)
    assert res["status"].tolist() == [5, 5, 0]
    good = SF.search(insts, FC.VARIANT, plans, np.array([[2, 0, 1]] * N), 4, 8, 4, SF.SIDEWAYS, 0, 1)
    for e in (0, 1):
        assert np.array_equal(res["plan"][e], bad[e]) and np.all(res["history"][:, e] == -1) and np.all(res["objective"][e] == -1)
        assert res["accepted"][e] == 0 and np.all(res["trace"][:, e] == 0)
        assert res["front_count"][e] == 0 and res["front_dropped"][e] == 0 and FC.archive_set(res, e) == []
    for key in SF.KEYS:
        x, y = (res[key][:, 2], good[key][:, 2]) if key in ("history", "trace") else (res[key][2], good[key][2])
        assert np.array_equal(x, y), key
    res = SF.search(insts, FC.VARIANT, bad, np.array([[1, 1, 1]] * N), 4, 8, 4, SF.SIDEWAYS, 0, 1)
    assert res["status"].tolist() == [0, 2, 0] and res["front_count"].tolist()[1] == 0 and FC.archive_set(res, 1) == []


def test_rounds_zero_is_the_input_plan_alone(small):
    insts, plans = small
    res = SF.search(insts, FC.VARIANT, plans, np.array([FC.MIXED] * N), 0, 8, 4, SF.TABU, 0, 1)
    assert np.array_equal(res["plan"], plans) and res["front_count"].tolist() == [1] * N and np.all(res["front_src"][:, 0] == (-1, 0))
    assert np.array_equal(res["front_plan"][:, 0], plans) and np.array_equal(res["front_obj"][:, 0], res["objective"])


def test_symbols_are_declared_exported_and_refuse_without_a_device(built):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    lib = _capi.lib()
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    assert _capi.SIGNATURES["fjsp_schedule_search_front"] == (C.c_int, [vp, vp, i32, i32, vp, i32, i32, u64, i64, i32] + [vp] * 12)
    assert _capi.SIGNATURES["fjsp_schedule_search_front_lds"] == (C.c_int, [vp, i32])
    header = open(os.path.join(REPO, "include", "fjsp_amd.h")).read()
    for name in ("fjsp_schedule_search_front", "fjsp_schedule_search_front_lds"):
        assert "int %s(" % name in header and hasattr(lib, name)
    assert lib.fjsp_schedule_search_front(None, None, 1, 1, None, 0, 0, 0, 0, 4, *([None] * 12)) == _capi.FJSP_E_ARG
    assert "fjsp_schedule_search_front: null" in lib.fjsp_last_error().decode()
    assert lib.fjsp_schedule_search_front_lds(None, 4) == 0
