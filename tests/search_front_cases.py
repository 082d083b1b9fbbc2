"""What tests/test_search_front_reference_host.py and tests/test_gpu_search_front.py share: shops, start plans, weight
vectors, and the seeds chosen on the CPU (each test that uses one asserts what it was chosen for)."""
import numpy as np

from tests import decode_dyn_reference as DD
from tests import search_dyn_cases as SC
from tests import search_front_reference as SF

episodes, shop, random_plans = SC.episodes, SC.shop, SC.random_plans

# gen8801, 4 envs, the random plans of seed 5 (search_dyn_cases' start): 10 rounds x 32 neighbours
MATRIX = dict(rounds=10, n_cand=32, tenure=3, seed=17)
# the same start under tabu with MIXED on every env: with 16 slots nothing is dropped in any env (the archives peak at 5, 5,
# 7, 7); with 4 slots entrants are dropped in every env, and in envs 2 and 3 a member leaves for an entrant that is itself
# dropped
DROPS = dict(rounds=10, n_cand=32, tenure=3, seed=0)

UNITS = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
MIXED = (60, 5, 1)                                # (a makespan unit against 60 of energy: the columns are of the order of 10^3, 10^3 and 6 x 10^4)
PER_ENV = ((60, 5, 1), (1, 1, 0), (0, 3, 1), (100, 0, 1))
SATURATING = (2 ** 62, 2 ** 62, 2 ** 62)          # every product is beyond 2^63 - 2: every key is 2^63 - 2


def weight_sets(n_env=4):
    """{name: int64[n_env][3]}: the three unit vectors, MIXED on every env, PER_ENV."""
    out = {"unit%d" % c: np.array([u] * n_env, np.int64) for c, u in enumerate(UNITS)}
    out["mixed"] = np.array([MIXED] * n_env, np.int64)
    out["per_env"] = np.array([PER_ENV[i % 4] for i in range(n_env)], np.int64)
    return out


def gen8801(eps=None):
    """(instance, plans int32[4][76][3])."""
    a, cap = shop(episodes() if eps is None else eps, "gen8801")
    return a, random_plans(a, 4, 5, cap)


def brute_front(vectors):
    """The non-dominated, distinct vectors of a list, as a set of tuples."""
    vs = set(tuple(int(x) for x in v) for v in vectors)
    return {v for v in vs if not any(SF.dominates(o, v) for o in vs)}


def archive_set(res, e):
    """Env e's archive of a result (reference or kernel, numpy arrays) as a set of tuples; asserts the free slots' form."""
    held = res["front_src"][e][:, 1] >= 0
    assert int(held.sum()) == int(res["front_count"][e])
    assert np.all(res["front_obj"][e][~held] == -1) and np.all(res["front_src"][e][~held] == -1) and np.all(res["front_plan"][e][~held] == -1)
    return [tuple(int(x) for x in v) for v in res["front_obj"][e][held]]


VARIANT = DD.VARIANT
