"""Instances, actions and oracle drivers of the asynchronous order-arrival service's tests (fjsp_env_step_async).

Shared by tests/test_async_cases_host.py (CPU: the C oracle with a recording LP hook proves what the GPU tests lean on)
and tests/test_gpu_async_arrivals.py (the service against the blocking fjsp_env_step and the oracle, bit for bit).
Every instance comes from tests/lp_cases.make_instance: two orders, seeded processing times and eligibility.

Two families:

    lock-step   the second order arrives at t = 100 000, long after the first is dispatched: every env reaches its arrival
                in the step that dispatches the last operation of the first order, whatever rules it plays (the shop runs
                empty and the clock jumps, SO_FJSSP.py:228-231), so all envs of an instance park in ONE call, with ONE LP.
                lock3: Jr [2, 1], M 2, one job per kind: 3 + 3 operations;  lock4: Jr [1, 1, 1, 1]: 4 + 4.
    staggered   the second order arrives while jobs of the first are in the shop: envs that play different rules park in
                different calls with different (Q, n_now).  One instance per chunk count of the kernels:
                stag1  K  12, M  3          one chunk
                stag2  K  70, M  9          two chunks, the MP > 8 record layout
                stag4  K 132, M 12, 3 machines per operation   four chunks (a host LP stays at tens of milliseconds)
"""
import numpy as np

from tests import lp_cases as LC

SO_FJSSP, MO_DFJSP, SO_DFJSP = 0, 4, 5
ACTION_SPACE = {SO_FJSSP: (6, 5), SO_DFJSP: (6, 5), MO_DFJSP: (12, 10)}
# the rule pair whose two rules both end in random.choice (SO_FJSSP.py:296,320; MO_DFJSP_breakdown.py:381,428)
RANDOM_PAIR = {SO_FJSSP: (5, 4), SO_DFJSP: (5, 4), MO_DFJSP: (11, 9)}
ENV_SEED_STRIDE = 1000003        # batch.ENV_SEED_STRIDE (importing it would pull torch into the CPU test)

LOCKSTEP = ("lock3", "lock4")
STAGGERED = {1: "stag1", 2: "stag2", 4: "stag4"}      # by chunk count
# (chunks, variant, N) of the staggered GPU cases
STAGGERED_SETS = [(1, SO_FJSSP, 40), (1, SO_DFJSP, 40), (1, MO_DFJSP, 40), (2, SO_FJSSP, 24), (2, MO_DFJSP, 24), (4, MO_DFJSP, 12)]
EXTRA_STEPS = 5                  # applied steps per env beyond two full episodes
RNG_SEED = 5                     # rng_seed of every batch of these tests
# arrival time of the second order of the staggered instances: inside the first order's makespan under every rule
# (tests/test_async_cases_host.py holds the conditions these were chosen for)
STAG_ARRIVE = {"stag1": 15, "stag2": 40, "stag4": 60}


def arr(name):
    if name == "lock3":
        return LC.make_instance(name, 71, [2, 1], 2, count=1, arrive1=100000)
    if name == "lock4":
        return LC.make_instance(name, 72, [1, 1, 1, 1], 2, count=1, arrive1=100000)
    if name == "stag1":
        return LC.make_instance(name, 73, [3] * 4, 3, count=1, arrive1=STAG_ARRIVE[name])
    if name == "stag2":
        return LC.make_instance(name, 74, [5] * 14, 9, count=1, arrive1=STAG_ARRIVE[name])
    if name == "stag4":
        return LC.make_instance(name, 75, [6] * 22, 12, per_op=3, count=1, arrive1=STAG_ARRIVE[name])
    raise KeyError(name)


def instance_set(names, variant):
    """Product InstanceSet of the named instances with the host solver's reset-time x; MO_DFJSP: machine data with the
    dense breakdown windows of test_randomised_differential_vs_oracle."""
    s = LC.instance_set([arr(n) for n in names])
    if variant == MO_DFJSP:
        for i in range(len(names)):
            s.generate_machine_data(i, 900 + i, max_windows=4, window_gap=(1, 60), window_len=(1, 30))
    return s


def ops_first(a):
    """Operations of the first order = the (1-based) step in which a lock-step env reaches its arrival."""
    return int((np.asarray(a.count).reshape(a.S, a.R)[0] * np.asarray(a.Jr)).sum())


def ops_total(a):
    return int((np.asarray(a.count).reshape(a.S, a.R) * np.asarray(a.Jr)[None, :]).sum())


def env_seed(e, rng_seed=RNG_SEED):
    return (rng_seed + e * ENV_SEED_STRIDE) & (2 ** 64 - 1)


def actions(variant, T, N, seed):
    """uint8[T, N, 2]: a random rule pair per env per step over the variant's whole action space."""
    rs = np.random.RandomState(seed)
    n0, n1 = ACTION_SPACE[variant]
    return np.stack([rs.randint(0, n0, (T, N)), rs.randint(0, n1, (T, N))], 2).astype(np.uint8)


def staggered_actions(chunks, variant, N):
    """The actions of the staggered GPU case: two episodes + EXTRA_STEPS applied steps per env."""
    T = 2 * ops_total(arr(STAGGERED[chunks])) + EXTRA_STEPS
    return actions(variant, T, N, 4000 + 10 * chunks + variant)


def mo_rows(variant, N, seed=77):
    """step()'s extra arguments per env: MO_DFJSP reward policies 0 .. 3 with normalisers; None for the SO variants."""
    if variant != MO_DFJSP:
        return None
    rs = np.random.RandomState(seed)
    return [(float(rs.randint(0, 4)), float(rs.randint(20, 90)), float(rs.choice([0.0, 17.0, 250.0])), float(rs.randint(500, 5000)))
            for _ in range(N)]


_LP_MEMO = {}


def _lp(a, Q, now):
    """The product's host LP, remembered per (instance, Q, n_now): the envs of a case pose the same reset-time LP."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    key = (a.name if hasattr(a, "name") else id(a), np.asarray(a.p).tobytes(), Q.tobytes(), now.tobytes())
    if key not in _LP_MEMO:
        _LP_MEMO[key] = fi.fluid_lp(a.Jr, a.p, Q, now)[0]
    return _LP_MEMO[key]


def arrivals(a, acts, rng_seed, variant, mo=None):
    """One episode of instance arrays `a` (InstanceSet.arrays) on the C oracle with a recording LP hook.  Returns (T,
    [(step, Q, n_now)]): the episode's steps and, for every LP the oracle asked for AFTER reset, the 0-based step that
    asked and the LP's inputs."""
    from oracle import pyoracle
    calls, now_step = [], [-1]

    def hook(Q, n_now):
        if now_step[0] >= 0:
            calls.append((now_step[0], Q.copy(), n_now.copy()))
        return _lp(a, Q, n_now)
    env = pyoracle.OracleEnv(a, hook, variant, rng_seed, ddt=getattr(a, "ddt", None) if variant == MO_DFJSP else None)
    env.reset()
    t = 0
    while not env.done:
        now_step[0] = t
        if variant == MO_DFJSP:
            m = mo if mo is not None else (1, 0, 0, 0)
            env.step_dyn(acts[t], int(m[0]), *[v if v > 0 else None for v in m[1:4]])
        else:
            env.step(acts[t])
        t += 1
    return t, calls
