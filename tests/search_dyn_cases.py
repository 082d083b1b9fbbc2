"""What tests/test_search_dyn_reference_host.py and tests/test_gpu_search_dyn.py share: the recorded MO_DFJSP shops, their
start plans, and the seeds chosen on the CPU (each test that uses one asserts what it was chosen for)."""
import numpy as np

from tests import decode_dyn_reference as DD
from tests import decode_reference as D
from tests import schedule_fixture as F

MATRIX = dict(rounds=10, n_cand=32, tenure=3, seed=17)       # gen8801, 4 envs: under objective 2 the winner differs from makespan's
ASPIRATION = dict(rounds=8, n_cand=32, tenure=100, seed=2)   # gen8801, 4 envs, tabu on the makespan: a tabu candidate is taken


def episodes():
    variant, eps = F.load()["mo_dfjsp"]
    assert variant == DD.VARIANT
    return eps


def shop(eps, name):
    """(instance, rows of its recorded table)."""
    ep = next(ep for ep in eps if ep["inst"].name == name)
    return ep["inst"], len(ep["table"])


def random_plans(inst, n, seed, cap):
    rs = np.random.RandomState(seed)
    return np.stack([D.random_plan(inst, rs, cap) for _ in range(n)])
