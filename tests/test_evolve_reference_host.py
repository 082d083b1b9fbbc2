"""CPU: tests/evolve_reference.py, the statement of fjsp_schedule_evolve, on gen8801 under MO_DFJSP, on the recorded
three-order SO_DFJSP shop and on a shop of 140 jobs: every child decodes and holds its parents' operations, the history
never increases, the fixed points (one individual, 64 copies), what a mutation changes, the job set across two draws, a tie
in a tournament, saturating weights, bad weights -- and the new symbols' declaration, export and host refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import evolve_cases as EC
from tests import evolve_reference as E
from tests import search_front_reference as SF
from tests import search_reference as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gen8801():
    return EC.gen8801()


def test_the_stream_is_its_own_and_the_header_states_it():
    header = open(os.path.join(REPO, "include", "fjsp_amd.h")).read()
    assert "#define FJSP_EVOLVE_STREAM 0x%016XULL" % E.STREAM in header
    others = [int(line.split()[2][:-3], 16) for line in header.splitlines() if line.startswith("#define FJSP_") and "_STREAM 0x" in line]
    assert len(others) == len(set(others)) == 5 and E.STREAM != S.STREAM
    assert E.draw(5, 7) == S.draw(5, 7) and E.env_stream(1, 2) != S.env_stream(1, 2)


@pytest.mark.parametrize("mut_rate", EC.MUT_RATES)
def test_every_child_decodes_and_holds_its_parents_operations(gen8801, mut_rate):
    a, pops = gen8801
    res = E.evolve([a] * 2, EC.VARIANT, pops[:2, :12], EC.weight_sets(2)["per_env"], 4, mut_rate, 11)
    assert np.all(res["status"] == 0) and EC.check_children(res, pops) == 2 * 4 * 12
    mutated = res["trace"][..., 2] >= 0
    assert not mutated[:, :, 0].any()                                             # never the elite
    assert mutated.any() == (mut_rate > 0) and mutated[:, :, 1:].all() == (mut_rate == E.MUT_ONE)


def test_the_three_order_shop_and_the_140_job_shop():
    a, cap = EC.multi_order()
    pops = EC.population(a, 1, 4, cap, 3)
    res = E.evolve([a], EC.SO_DFJSP, pops, EC.plain_weights(1), 2, E.MUT_ONE, 5)
    assert np.all(res["status"] == 0) and res["population_objective"].shape == (1, 4, 2) and EC.check_children(res, pops) == 8
    assert len(E.job_numbers(a)) == a.R + 1 and E.job_numbers(a)[-1] == 134
    b = EC.many_jobs()
    assert E.job_numbers(b).tolist() == [0, 70, 140]
    pops = EC.population(b, 2, 6, 140, 4)
    res = E.evolve([b] * 2, 0, pops, EC.plain_weights(2), 3, 6554, 9)
    assert np.all(res["status"] == 0) and EC.check_children(res, pops) == 2 * 3 * 6
    # jobs beyond 127 take their bits from the third word: some child takes such a job from each parent
    s = E.env_stream(9, 0)
    sides = {E.in_set(E.child_stream(s, 1, 6, q), j) for q in range(1, 6) for j in range(128, 140)}
    assert sides == {True, False}


def test_one_individual_and_64_copies_are_fixed_points(gen8801):
    a, pops = gen8801
    w = EC.weight_sets()["mixed"]
    for generations in (0, 1, 5):
        res = E.evolve([a] * 4, EC.VARIANT, pops[:, :1], w, generations, 0, 3)
        assert np.array_equal(res["population"], pops[:, :1]) and np.array_equal(res["plan"], pops[:, 0])
        assert np.all(res["history"] == res["history"][0]) and np.all(res["trace"] == (0, 0, -1))
    copies = np.repeat(pops[:1, 5:6], 64, 1)
    res = E.evolve([a], EC.VARIANT, copies, w[:1], 3, 0, 3)
    assert np.array_equal(res["population"], copies) and np.all(res["history"] == res["history"][0])
    assert np.all(res["population_objective"] == res["objective"][:, None])


def test_a_mutation_changes_at_most_one_machine(gen8801):
    a, pops = gen8801
    res = E.evolve([a] * 2, EC.VARIANT, pops[:2, :10], EC.weight_sets(2)["mixed"], 3, E.MUT_ONE, 21)
    changed = same = 0
    for e in range(2):
        for t, made in enumerate(res["children"][e]):
            for q, (plain, child, status) in enumerate(made):
                diff = np.flatnonzero((plain != child).any(1))
                assert np.array_equal(plain[:, :2], child[:, :2]) and len(diff) <= 1
                if q == 0:
                    assert len(diff) == 0 and res["trace"][t, e, q, 2] == -1
                    continue
                u = res["trace"][t, e, q, 2]
                assert 0 <= u < 76 and all(d == u for d in diff)
                changed += len(diff)
                same += 1 - len(diff)
    assert changed > 0 and same > 0                                               # (the row's own machine may be drawn)


def test_jobs_63_and_64_take_their_bits_from_two_draws():
    b = EC.many_jobs()
    seed = EC.BIT_63_64["seed"]
    c = E.child_stream(E.env_stream(seed, 0), 1, 6, 1)
    assert E.in_set(c, 63) == bool(E.draw(c, 8) >> 63) and E.in_set(c, 64) == bool(E.draw(c, 9) & 1)
    assert E.in_set(c, 63) != E.in_set(c, 64)
    pops = EC.population(b, 1, 6, 140, 4)
    res = E.evolve([b], 0, pops, EC.plain_weights(1), 1, 0, seed)
    pa = res["trace"][0, 0, 1, 0]
    plain = res["children"][0][0][1][0]
    A = pops[0, pa, :140]
    # job 63 is job 63 of kind 0, job 64 is job 64 of kind 0: the one in the set stands where parent A has it
    for j in (63, 64):
        at_a, at_child = np.flatnonzero((A[:, 0] == 0) & (A[:, 1] == j)), np.flatnonzero((plain[:, 0] == 0) & (plain[:, 1] == j))
        if E.in_set(c, j):
            assert len(at_a) == 1 and np.array_equal(at_a, at_child)


def test_a_tie_in_a_tournament_goes_to_the_lower_index(gen8801):
    a, pops = gen8801
    k = EC.TIE
    res = E.evolve_one(a, EC.VARIANT, pops[0][:k["pop"]], EC.UNITS[0], k["generations"], 0, k["seed"], 0)
    found = 0
    for t, q, n in res["ties"]:
        c = E.child_stream(E.env_stream(k["seed"], 0), t, k["pop"], q)
        x, y = (S.pick(E.draw(c, 2 * n + i), k["pop"]) for i in range(2))
        assert x != y and res["trace"][t - 1, q, n] == min(x, y)
        found += y < x                                                            # the second pick wins by its index alone
    assert found > 0


def test_saturating_weights_make_individual_0_the_elite(gen8801):
    a, pops = gen8801
    w = np.array([EC.SATURATING] * 2, np.int64)
    res = E.evolve([a] * 2, EC.VARIANT, pops[:2, :8], w, 3, 6554, 4)
    assert np.all(res["history"] == SF.KEY_MAX) and np.all(res["status"] == 0)
    assert np.all(res["trace"][:, :, 0, :2] == 0)                                 # every key is equal: the least (key, index) is index 0
    assert np.array_equal(res["plan"], pops[:2, 0]) and np.array_equal(res["population"][:, 0], pops[:2, 0])


def test_bad_weights_and_a_plan_that_does_not_decode_stop_their_env_alone(gen8801):
    a, pops = gen8801
    pops = pops[:3, :6].copy()
    bad = pops.copy()
    bad[1, 2, 3, 2] = 99                                                          # machine out of range: status 3
    bad[1, 4, -1] = -1                                                            # operations missing: status 2, at a higher q
    w = np.array([[1, -1, 1], [60, 5, 1], [60, 5, 1]])
    res = E.evolve([a] * 3, EC.VARIANT, bad, w, 2, 6554, 1)
    assert res["status"].tolist() == [5, 3, 0]
    good = E.evolve([a] * 3, EC.VARIANT, pops, np.array([[60, 5, 1]] * 3), 2, 6554, 1)
    for e in (0, 1):
        assert np.array_equal(res["population"][e], bad[e]) and np.array_equal(res["plan"][e], bad[e, 0])
        assert np.all(res["history"][:, e] == -1) and np.all(res["objective"][e] == -1) and np.all(res["population_objective"][e] == -1)
        assert np.all(res["trace"][:, e] == 0)
    for key in E.KEYS:
        x, y = (res[key][:, 2], good[key][:, 2]) if key in ("history", "trace") else (res[key][2], good[key][2])
        assert np.array_equal(x, y), key
    assert E.evolve([a] * 3, EC.VARIANT, bad, np.array([[0, 0, 0]] * 3), 1, 0, 1)["status"].tolist() == [5, 5, 5]


def test_no_generations_describe_the_input(gen8801):
    a, pops = gen8801
    res = E.evolve([a] * 4, EC.VARIANT, pops[:, :5], EC.weight_sets()["unit2"], 0, 6554, 1)
    assert np.array_equal(res["population"], pops[:, :5]) and res["history"].shape == (1, 4) and res["trace"].shape == (0, 4, 5, 3)
    from tests import decode_dyn_reference as DD
    want = DD.decode([a] * 4, pops[:, :5], None, 5)["objective"]
    assert np.array_equal(res["population_objective"], want)
    best = want[..., 2].argmin(1)
    assert np.array_equal(res["plan"], pops[np.arange(4), best]) and np.array_equal(res["history"][0], want[..., 2].min(1))


def test_symbols_are_declared_exported_and_refuse_without_a_device(built):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    lib = _capi.lib()
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    assert _capi.SIGNATURES["fjsp_schedule_evolve"] == (C.c_int, [vp, vp, i32, i32, vp, i32, u64, i64] + [vp] * 9)
    assert _capi.SIGNATURES["fjsp_schedule_evolve_lds"] == (C.c_int, [vp])
    header = open(os.path.join(REPO, "include", "fjsp_amd.h")).read()
    for name in ("fjsp_schedule_evolve", "fjsp_schedule_evolve_lds"):
        assert "int %s(" % name in header and hasattr(lib, name)
    assert lib.fjsp_schedule_evolve(None, None, 1, 1, None, 0, 0, 0, *([None] * 9)) == _capi.FJSP_E_ARG
    assert "fjsp_schedule_evolve: null" in lib.fjsp_last_error().decode()
    assert lib.fjsp_schedule_evolve_lds(None) == 0
