"""What tests/test_evolve_reference_host.py and tests/test_gpu_evolve.py share: shops, start populations, weight vectors, and
the seeds chosen on the CPU (each test that uses one asserts what it was chosen for)."""
import numpy as np

from tests import decode_limit_cases as LC
from tests import decode_reference as D
from tests import schedule_fixture as F
from tests import search_front_cases as FC

VARIANT = FC.VARIANT                              # MO_DFJSP
SO_DFJSP = 5
UNITS, MIXED, PER_ENV, SATURATING = FC.UNITS, FC.MIXED, FC.PER_ENV, FC.SATURATING
episodes, shop, weight_sets = FC.episodes, FC.shop, FC.weight_sets

POPS = (1, 2, 33, 64)
GENERATIONS = (0, 1, 2, 7)
MUT_RATES = (0, 6554, 65536)
SEED = 17                                         # of the matrix

# gen8801, env 0 (global id 0), the first 8 individuals of gen8801()'s population, unit weight, mut_rate 0, 3 generations:
# a tournament whose two picks are different individuals of equal keys (copies of the elite) and the second pick has the
# lower index and wins
TIE = dict(pop=8, generations=3, seed=8)
# the stream of child 1 of generation 1 of env 0 under this seed: jobs 63 and 64 -- the last bit of draw 8, the first of
# draw 9 -- fall on different sides of the job set
BIT_63_64 = dict(seed=3)


def population(inst, n_env, pop, cap, seed):
    """int32[n_env][pop][cap][3]: random feasible plans of `inst`."""
    rs = np.random.RandomState(seed)
    return np.stack([np.stack([D.random_plan(inst, rs, cap) for _ in range(pop)]) for _ in range(n_env)])


def gen8801(eps=None):
    """(instance, population int32[4][64][76][3]): the matrix takes its first P individuals."""
    a, cap = shop(episodes() if eps is None else eps, "gen8801")
    return a, population(a, 4, 64, cap, 5)


def multi_order():
    """(instance, rows): the recorded SO_DFJSP shop of three orders, 134 jobs, 1 157 rows."""
    variant, eps = F.load()["so_dfjsp"]
    ep = next(ep for ep in eps if ep["inst"].S > 1)
    assert variant == SO_DFJSP and ep["inst"].S == 3
    return ep["inst"], len(ep["table"])


def many_jobs():
    """Two kinds of 70 one-stage jobs on two machines, every machine eligible: 140 jobs, the job set takes three draws."""
    rs = np.random.RandomState(140)
    return LC.instance("2x70", [1, 1], rs.randint(1, 21, (2, 2)), [[70, 70]], delivery=[400])


def plain_weights(n_env):
    """Unit weights of a handle with two objectives, the makespan and the tardiness in turns."""
    return np.array([UNITS[e % 2][:2] for e in range(n_env)], np.int64)


def operations(rows):
    """The multiset of a plan's operations: its (kind, job) pairs, sorted."""
    rows = np.asarray(rows).reshape(-1, 3)
    return sorted((int(r), int(n)) for r, n, _ in rows[:D.plan_length(rows)])


def check_children(res, pops):
    """Every child of every generation of a reference result decodes and holds its parents' operations; the history never
    increases.  Returns the number of children seen."""
    seen = 0
    for e, gens in enumerate(res["children"]):
        want = operations(pops[e][0])
        for made in gens:
            for plain, child, status in made:
                assert status == 0 and operations(child) == want == operations(plain)
                seen += 1
    assert np.all(np.diff(res["history"], axis=0) <= 0)
    return seen
