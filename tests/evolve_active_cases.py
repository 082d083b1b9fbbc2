"""What tests/test_evolve_active_reference_host.py and tests/test_gpu_evolve_active.py share: the shops of
tests/evolve_cases.py on handles the active decoder takes (gen8801 created as SO_DFJSP or SO_FJSSP, not as MO_DFJSP), the
histories recorded for the two decoders, and the batches with more envs than are resident.  Each figure chosen or recorded
for a property is asserted by the test that uses it."""
import numpy as np

from tests import decode_active_cases as AC
from tests import decode_limit_cases as DL
from tests import evolve_cases as EC

SO_FJSSP, SO_DFJSP = 0, EC.SO_DFJSP
VARIANTS = (SO_DFJSP, SO_FJSSP)
POPS, GENERATIONS, MUT_RATES, SEED = EC.POPS, EC.GENERATIONS, EC.MUT_RATES, EC.SEED

# gen8801 as SO_DFJSP or SO_FJSSP, env 0 (global id 0) of evolve_cases.gen8801()'s population, weights (1, 0), seed 17: the
# history of the least makespan under the active and under the semi-active decoder, whether the traces of the two runs
# differ, and the rows the first individuals of the active run's last generation inserted.  A kernel that still decoded
# semi-actively would give the second history.
RECORDED = (
    dict(pop=8, generations=3, mut_rate=6554, active=[624, 624, 624, 612], semi=[945, 945, 880, 871], trace_differs=True,
         inserted=[44, 38, 38, 40, 34, 44, 39, 44]),
    dict(pop=64, generations=7, mut_rate=65536, active=[566] * 5 + [553] * 3, semi=[814] + [758] * 4 + [737] * 3, trace_differs=True,
         inserted=None),
    dict(pop=2, generations=2, mut_rate=0, active=[624, 624, 624], semi=[969, 969, 969], trace_differs=False, inserted=[44, 36]),
)
RECORDED_WEIGHTS = (1, 0)


def unit_weights(n_env):
    """int64[n_env][2]: the makespan and the tardiness in turns."""
    return EC.plain_weights(n_env)


def hand_populations(P):
    """(cases, instances, populations int32[n][P][cap][3]): decode_active_cases.cases() as populations of P copies of each
    hand-made plan, env i on case i's instance, padded to the capacity of a batch that holds them all."""
    cases = AC.cases()
    cap = max(len(c.plan) for c in cases)
    pops = np.stack([np.stack([DL.padded(c.plan, cap)] * P) for c in cases]).astype(np.int32)
    return cases, [c.inst for c in cases], pops


def more_than_resident(pops, resident, P, extra=5):
    """(populations int32[N][P][cap][3], weights int64[N][2]) of N = resident + extra envs: env e takes the first P
    individuals of base population e % len(pops); env 1 holds an individual whose last row is missing (status 2) and env 2
    has all-zero weights (status 5), so workgroups 1 and 2 of a grid of `resident` meet a status on their first tenant and
    still owe their second, envs resident + 1 and resident + 2."""
    N = resident + extra
    out = np.ascontiguousarray(np.stack([pops[e % len(pops), :P] for e in range(N)]), np.int32)
    L = int(np.sum(out[1, P - 1, :, 0] >= 0))
    out[1, P - 1, L - 1] = -1
    w = unit_weights(N).copy()
    w[2] = 0
    return out, w


def compared(resident, extra=5):
    """The envs of more_than_resident that the tests decide by the numpy reference: the first tenants around the statuses,
    the last first tenant and every second tenant."""
    return [0, 1, 2, 4, resident - 1] + list(range(resident, resident + extra))
