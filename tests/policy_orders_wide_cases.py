"""Instances and expected builds of the tests of the segmented policy kernels (fjsp_env_play_policy_orders,
fjsp_env_rollout_policy_orders; csrc/fjsp_kernels_policy.inc) on order batches of two and four chunks of 64 operation types.

Shared by tests/test_policy_orders_wide_cases_host.py (CPU: the C oracle plays every case through its arrivals and into its
last chunk; the slice / workgroup / LP-route arithmetic restated) and tests/test_gpu_policy_orders_wide.py (the kernels
against the per-step paths and the oracle).

A case is one batch of three instances built with tests.wave_limit_cases.make (M = 3, processing times 1..5): the edge
instance, a one-order filler with K = 5 (an environment that never parks) and a two-order filler with K = 64 (the upper
chunks of a 2- or 4-chunk record stay empty); the fillers share the batch's padded sizes.  Environment e plays instance
e % 3.  The edge instances: `kinds` kinds of `stages` operations, one order per entry of `arrive`, `jobs` jobs per kind
and order.  The expected build of a 20-input actor (EnvBatch.policy_orders_build) and the LP service a create under
FJSP_LP_IMPL=global / device picks (EnvBatch.lp_on_device: 0 host, 1 tableau in LDS, 2 tableau in global memory):

    name     kinds x stages  arrive        jobs  K    jobs  steps  KC  slice   envs/wg  global  device
    k65      13 x 5          0, 40, 80     1      65    39   195   2   3904 B  8        2       0
    k65flat  65 x 1          0, 15, 30     1      65   195   195   2   5440 B  8        1       1
    k128     32 x 4          0, 40, 80     1     128    96   384   2   4416 B  8        2       0
    k129     43 x 3          0, 60         1     129    86   258   4   7488 B  8        2       0
    k256     64 x 4          0, 100        1     256   128   512   4   7488 B  8        0       0
    k129x2   43 x 3          0, 80, 160    2     129   258   774   4   9024 B  4        2       0

The K = 64 filler is 16 kinds of 4 operations with its second order at 30; k65flat's is 64 kinds of one operation (a 67-row
tableau, second order at 15), so that the whole batch stays inside the LDS rule.
"""
import numpy as np

from tests import wave_limit_cases as WC

M = 3
STATE_SIZE = 20                  # SO_FJSSP / SO_DFJSP
RNG_SEED = 31                    # rng_seed of every batch of these tests
ENV_SEED_STRIDE = WC.ENV_SEED_STRIDE
SEED = 4242                      # instance seeds: SEED + 10 x the case's position + the instance's
VARIANTS = (0, 5)                # SO_FJSSP, SO_DFJSP
ACTION_SPACE = (6, 5)
HOST, LDS, GLOBAL = 0, 1, 2      # EnvBatch.lp_on_device

# name: edge shape, then the expected build
SPECS = {
    "k65": dict(kinds=13, stages=5, arrive=(0, 40, 80), jobs=1, K=65, n_jobs=39, steps=195, kc=2, slice=3904, envs_per_wg=8,
                lp_global=GLOBAL, lp_device=HOST, N=12),
    "k65flat": dict(kinds=65, stages=1, arrive=(0, 15, 30), jobs=1, K=65, n_jobs=195, steps=195, kc=2, slice=5440, envs_per_wg=8,
                    lp_global=LDS, lp_device=LDS, N=12),
    "k128": dict(kinds=32, stages=4, arrive=(0, 40, 80), jobs=1, K=128, n_jobs=96, steps=384, kc=2, slice=4416, envs_per_wg=8,
                 lp_global=GLOBAL, lp_device=HOST, N=12),
    "k129": dict(kinds=43, stages=3, arrive=(0, 60), jobs=1, K=129, n_jobs=86, steps=258, kc=4, slice=7488, envs_per_wg=8,
                 lp_global=GLOBAL, lp_device=HOST, N=12),
    "k256": dict(kinds=64, stages=4, arrive=(0, 100), jobs=1, K=256, n_jobs=128, steps=512, kc=4, slice=7488, envs_per_wg=8,
                 lp_global=HOST, lp_device=HOST, N=12),
    "k129x2": dict(kinds=43, stages=3, arrive=(0, 80, 160), jobs=2, K=129, n_jobs=258, steps=774, kc=4, slice=9024, envs_per_wg=4,
                   lp_global=GLOBAL, lp_device=HOST, N=6),
}
NAMES = tuple(SPECS)
N_SMALL = 3                      # fewer envs than a workgroup: one env per instance
LP_ROUTES = {"host": "lp_host", "device": "lp_device", "global": "lp_global"}      # FJSP_LP_IMPL -> the SPECS entry


def lp_expected(name, route):
    """EnvBatch.lp_on_device of case `name` created under FJSP_LP_IMPL=route."""
    return HOST if route == "host" else SPECS[name][LP_ROUTES[route]]


_ARRS = {}


def instances(name):
    """[edge, one-order filler, two-order K = 64 filler]: the arguments of InstanceSet.set_raw (WC.make)."""
    if name not in _ARRS:
        sp = SPECS[name]
        seed = SEED + 10 * NAMES.index(name)
        S = len(sp["arrive"])
        fill = [1] * 64 if sp["stages"] == 1 else [4] * 16
        _ARRS[name] = [
            WC.make(name + "/edge", seed, [sp["stages"]] * sp["kinds"], M, np.full((S, sp["kinds"]), sp["jobs"]), arrive=sp["arrive"]),
            WC.make(name + "/one", seed + 1, [3, 2], M, [2, 2]),
            WC.make(name + "/k64", seed + 2, fill, M, np.ones((2, len(fill))), arrive=(0, 15 if sp["stages"] == 1 else 30))]
    return _ARRS[name]


def instance_set(name):
    """The product InstanceSet of the case's three instances, with the host solver's reset-time fluid solution."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    arrs = instances(name)
    s = fi.InstanceSet(len(arrs))
    for i, a in enumerate(arrs):
        s.set_raw(i, a.Jr, a.p, a.elig_n, a.elig_list, a.count, a.arrive, a.delivery, a.ddt)
    return s.solve_fluid()


def set_arrays(name, s=None):
    """InstanceSet.arrays of the case's instances (with x), named like the case's."""
    s = instance_set(name) if s is None else s
    out = []
    for i, a in enumerate(instances(name)):
        b = s.arrays(i)
        b.name = a.name
        out.append(b)
    return out


def env_seed(e):
    return (RNG_SEED + e * ENV_SEED_STRIDE) & (2 ** 64 - 1)


def actions(name, variant, N):
    """uint8[steps, N, 2]: a seeded random rule pair per env and step over the whole action space."""
    rs = np.random.RandomState(50000 + 10 * NAMES.index(name) + variant)
    T = SPECS[name]["steps"]
    return np.stack([rs.randint(0, ACTION_SPACE[0], (T, N)), rs.randint(0, ACTION_SPACE[1], (T, N))], 2).astype(np.uint8)


# ---- the build arithmetic, restated (csrc/fjsp_kernels.hip lds_bytes_per_wave and policy_geometry, csrc/fjsp_policy.h
# actor_lds_floats, csrc/fjsp_env.hip plan_batch / plan_layout / choose_lp_service)

def chunks(K):
    return 1 if K <= 64 else (2 if K <= 128 else 4)


def slice_bytes(n_jobs, K):
    """The LDS slice of one environment in the policy kernels: 16 observation doubles, 8 of tail header, three rows of
    KP + 2 doubles, one 8-byte word per job (job tables padded to 64), then padded to 64 modulo 256."""
    KP, JP = 64 * chunks(K), -(-n_jobs // 64) * 64
    raw = (24 + 3 * (KP + 2)) * 8 + JP * 8
    return raw + (64 + 256 - raw % 256) % 256


def actor_bytes(S):
    """The actor's LDS weight image (S -> 128 -> 128 -> 32 padded actions, three bias rows), rounded up to 256 bytes."""
    floats = S * 128 + 128 * 128 + 128 * 32 + 128 + 128 + 32
    return (floats * 4 + 255) & ~255


def envs_per_workgroup(n_jobs, K, S=STATE_SIZE):
    """The most environments of 16, 8, 4, 2, 1 whose slices and actor scratch (768 B each) fit the CU's 160 KB beside the
    actor; 0 if not even one does."""
    for W in (16, 8, 4, 2, 1):
        if actor_bytes(S) + W * (slice_bytes(n_jobs, K) + (32 + 128 + 32) * 4) <= 160 * 1024:
            return W
    return 0


def expected_build(arrs, S=STATE_SIZE):
    """(kc, envs per workgroup, slice bytes, segments) of a batch of these instances: the largest of each size decides."""
    K = max(a.K for a in arrs)
    n_jobs = max(int(a.count.sum()) for a in arrs)
    return chunks(K), envs_per_workgroup(n_jobs, K, S), slice_bytes(n_jobs, K), max(a.S for a in arrs)


def expected_lp(arrs, route):
    """EnvBatch.lp_on_device of a batch of these instances created under FJSP_LP_IMPL=route: the LDS simplex where every
    tableau fits its rule (device, global), else the global one where every tableau is within its limits (global only),
    else the host."""
    from tests import lp_cases as LC, lp_global_cases as LG
    if route == "host":
        return HOST
    if LC.fits_device(arrs):
        return LDS
    return GLOBAL if route == "global" and all(LG.within_global(a) for a in arrs) else HOST
