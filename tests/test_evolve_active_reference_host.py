"""CPU: tests/evolve_active_reference.py, the numpy statement of fjsp_schedule_evolve_active.  With the semi-active decoder
its loop is tests/evolve_reference.py's in every key; with the active decoder every individual's vector and count are
decode_active_reference's of its plan, the children keep their parents' operations, the start population scores no worse
than semi-actively, the recorded histories of the two decoders come out (and differ), and the hand-made plans get their
hand-made begins."""
import numpy as np
import pytest

from tests import decode_active_reference as DA
from tests import evolve_active_cases as AC
from tests import evolve_active_reference as EA
from tests import evolve_cases as EC
from tests import evolve_reference as E
from tests import search_front_reference as SF


@pytest.fixture(scope="module")
def gen8801():
    return EC.gen8801()


@pytest.fixture(scope="module")
def semi_matrix(gen8801):
    """{(pop, generations, mut_rate): evolve_reference.evolve_one of env 0 of gen8801 as SO_DFJSP}, computed once."""
    a, pops = gen8801
    return {(P, T, mr): E.evolve_one(a, AC.SO_DFJSP, pops[0, :P], AC.RECORDED_WEIGHTS, T, mr, AC.SEED, 0)
            for P in AC.POPS for T in AC.GENERATIONS for mr in AC.MUT_RATES}


def _same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and np.array_equal(x, y)


@pytest.mark.parametrize("generations", AC.GENERATIONS)
@pytest.mark.parametrize("pop", AC.POPS)
def test_with_the_semi_active_decoder_the_loop_is_evolve_reference(gen8801, semi_matrix, pop, generations):
    a, pops = gen8801
    for mr in AC.MUT_RATES:
        want = semi_matrix[(pop, generations, mr)]
        got = EA.evolve_one(a, AC.SO_DFJSP, pops[0, :pop], AC.RECORDED_WEIGHTS, generations, mr, AC.SEED, 0, decode=SF.decode_one)
        for key in E.KEYS + ("ties",):
            assert _same(got[key], want[key]), (mr, key)
        assert len(got["children"]) == len(want["children"]) == generations
        for made, ref in zip(got["children"], want["children"]):
            assert all(_same(x[0], y[0]) and _same(x[1], y[1]) and x[2] == y[2] for x, y in zip(made, ref))
        assert not got["inserted"].any()                                          # (the semi-active decode counts nothing)
    # the batch form on four envs, per-env weights and global ids, MO_DFJSP included (three objectives)
    if pop == 33 and generations == 2:
        w = EC.weight_sets()["per_env"]
        want = E.evolve([a] * 4, EC.VARIANT, pops[:, :pop], w, generations, 6554, AC.SEED, first_env=3)
        got = EA.evolve([a] * 4, EC.VARIANT, pops[:, :pop], w, generations, 6554, AC.SEED, first_env=3, decode=SF.decode_one)
        assert all(_same(got[key], want[key]) for key in E.KEYS)


@pytest.mark.parametrize("variant", AC.VARIANTS)
def test_every_individual_is_scored_by_the_active_decoder(gen8801, variant):
    a, pops = gen8801
    w = AC.unit_weights(4)
    for P, T, mr in ((1, 0, 0), (2, 1, 65536), (33, 2, 6554), (8, 7, 65536)):
        res = EA.evolve([a] * 4, variant, pops[:, :P], w, T, mr, AC.SEED)
        assert np.all(res["status"] == 0) and res["inserted"].shape == (4, P) and res["inserted"].dtype == np.int32
        for e in range(4):
            for q in range(P):
                one = DA.decode_one(a, variant, res["population"][e, q], None, pops.shape[2])
                assert one["status"] == 0 and _same(one["objective"], res["population_objective"][e, q]) and one["inserted"] == res["inserted"][e, q]
            keys = [SF.key_of(w[e], res["population_objective"][e, q]) for q in range(P)]
            best = min(range(P), key=lambda q: (keys[q], q))
            assert _same(res["plan"][e], res["population"][e, best]) and _same(res["objective"][e], res["population_objective"][e, best])
            assert res["history"][T, e] == keys[best]
        assert EC.check_children(res, pops[:, :P]) == 4 * P * T


def test_the_start_population_scores_no_worse_than_semi_actively(gen8801):
    """Every row ends no later under the active decoder and the weights are non-negative: history[0] under a unit weight
    is at most the semi-active history[0]."""
    a, pops = gen8801
    for unit in ((1, 0), (0, 1)):
        for P in AC.POPS:
            act = EA.evolve_one(a, AC.SO_DFJSP, pops[0, :P], unit, 0, 0, AC.SEED, 0)
            semi = E.evolve_one(a, AC.SO_DFJSP, pops[0, :P], unit, 0, 0, AC.SEED, 0)
            assert act["status"] == semi["status"] == 0 and act["history"][0] <= semi["history"][0]
            assert np.all(act["population_objective"] <= semi["population_objective"])
            assert _same(act["population"], semi["population"])                   # (chromosomes are not rewritten)


@pytest.mark.parametrize("variant", AC.VARIANTS)
@pytest.mark.parametrize("case", range(len(AC.RECORDED)))
def test_recorded_histories_of_the_two_decoders(gen8801, variant, case):
    a, pops = gen8801
    c = AC.RECORDED[case]
    args = (a, variant, pops[0, :c["pop"]], AC.RECORDED_WEIGHTS, c["generations"], c["mut_rate"], AC.SEED, 0)
    act, semi = EA.evolve_one(*args), E.evolve_one(*args)
    assert act["history"].tolist() == c["active"] and semi["history"].tolist() == c["semi"]
    assert (not _same(act["trace"], semi["trace"])) == c["trace_differs"]
    if c["inserted"] is not None:
        assert act["inserted"][:8].tolist() == c["inserted"]


@pytest.mark.parametrize("generations", [0, 2])
@pytest.mark.parametrize("P", [1, 2])
def test_hand_made_plans_as_populations(P, generations):
    """Copies of one plan: every child is that plan (both parents hold the same rows in the same order; mut_rate 0), so the
    begins and the count of every individual of every generation are the hand-made answers."""
    cases, insts, pops = AC.hand_populations(P)
    res = EA.evolve(insts, 0, pops, AC.unit_weights(len(cases)), generations, 0, 5)
    assert np.all(res["status"] == 0) and _same(res["population"], pops)
    for i, c in enumerate(cases):
        one = DA.decode_one(c.inst, 0, res["plan"][i], None, pops.shape[2])
        assert one["table"][:len(c.plan), 4].tolist() == c.begins and one["inserted"] == c.inserted, c.name
        assert res["inserted"][i].tolist() == [c.inserted] * P and np.all(res["population_objective"][i] == one["objective"]), c.name
        assert np.all(res["history"][:, i] == SF.key_of(AC.unit_weights(len(cases))[i], one["objective"])), c.name
    assert {c.name for c in cases if c.inserted} >= {"a gap in front of the first interval, opened by a later order",
                                                     "three gaps skipped, placed in the fourth"}


def test_statuses_are_the_semi_active_ones(gen8801):
    a, pops = gen8801
    bad = pops[0, :4].copy()
    bad[2, -1] = -1
    bad[3, 0, 2] = 99
    res = EA.evolve_one(a, AC.SO_DFJSP, bad, (1, 0), 2, 0, 1, 0)
    assert res["status"] == 2 and _same(res["population"], bad) and np.all(res["history"] == -1) and not res["inserted"].any()
    assert EA.evolve_one(a, AC.SO_DFJSP, pops[0, :4], (0, 0), 2, 0, 1, 0)["status"] == SF.BAD_WEIGHTS
