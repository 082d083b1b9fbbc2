"""GPU: the device simplex (csrc/fjsp_lp_device.hip) on every compiled width and at its service edges.

The device file restates the host simplex (csrc/fjsp_lp.cpp) pivot for pivot, so the reference is the host solver and the
bar is BIT equality of x (`H.bits`): through the test hook `lp_device_solve` on the fixture instances and on the
generated cases of tests/lp_cases.py -- 2, 3, 4, 6, 7 and 8 chunks of 64 columns, up to 86 rows, leaving rows in both
halves, ties decided by signatures, by magnitudes and by the sequential scan; tests/test_lp_reference.py counts on the CPU
which branches those LPs take -- and through the order-arrival service itself: trajectories played with the LPs on the
device equal those played with the host service, at 4, 6 and 8 chunks, with more LPs in one launch than the launch has
workgroups, and with narrow and wide tableaus taking turns in one workgroup's LDS.  The create-time rule (device from
16 384 environments on, largest tableau within 156 KB of LDS and 512 columns) is pinned at its boundaries.

Failures are only ever the graceful ones (an input the host solver refuses too); nothing here provokes a device fault.
"""
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import lp_cases as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def test_device_lp_equals_the_host_lp(torch_gpu):
    """csrc/fjsp_lp_device.hip restates the host simplex (csrc/fjsp_lp.cpp) pivot for pivot: on every instance of the
    mo_dfjsp / multiorder suites whose tableau fits the LDS, for the reset-time LP and for random live states (jobs spread
    over the stages, so precedence rows come and go with n_now == 0), the device's x equals the host's BIT FOR BIT."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, VARIANT_MO_DFJSP
    rs = np.random.RandomState(17)
    checked = 0
    for suite, variant in (("mo_dfjsp", VARIANT_MO_DFJSP), ("multiorder", 0)):
        insts, _, _ = H.load_suite(suite)
        for i, a in enumerate(insts):
            s = H.instance_set_from([a])
            with H.env_var("FJSP_LP_IMPL", "device"):      # (small batches default to the host service)
                b = EnvBatch(s, 4, variant=variant, rng_seed=1)
            if not b.lp_on_device:
                continue                                   # (tableau beyond the LDS: this batch keeps the host service)
            koff = np.concatenate([[0], np.cumsum(a.Jr)])
            K, M = a.p.shape
            for trial in range(6):
                Q = np.zeros(K, np.int32); now = np.zeros(K, np.int32)
                for r in range(len(a.Jr)):
                    n = int(rs.randint(1, 25))
                    if trial == 0:
                        stages = np.zeros(n, np.int64)                             # every job at stage 0: the reset-time LP
                    else:
                        stages = rs.randint(0, a.Jr[r], n)                          # jobs spread over the stages (one stays at the last)
                        stages[0] = a.Jr[r] - 1 if trial % 2 else stages[0]
                    for j in range(a.Jr[r]):
                        Q[koff[r] + j] = max(1, int((stages <= j).sum()))           # tasks of (r, j) still unprocessed (class_FJSSP.py:234-235)
                        now[koff[r] + j] = int((stages == j).sum())                 # jobs waiting at (r, j)                 (:236-237)
                want, _ = fi.fluid_lp(a.Jr, a.p, Q, now)
                got = b.lp_device_solve(trial % 4, Q, now)[:K * M].reshape(K, M)
                assert np.array_equal(H.bits(got), H.bits(want)), "%s instance %d (%s) trial %d" % (suite, i, a.name, trial)
                checked += 1
    assert checked >= 12


def test_device_lp_service_leaves_every_trajectory_unchanged(torch_gpu):
    """The dynamic environment with its order-arrival LPs on the device (FJSP_LP_IMPL=device) against the same batch with
    FJSP_LP_IMPL=host:
    rewards step by step, final makespan / tardiness / energy and the number of LPs are identical."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, VARIANT_MO_DFJSP, global_actions
    insts, _, _ = H.load_suite("mo_dfjsp")

    def tableau_bytes(a):        # rows x columns of the largest tableau of the instance (csrc/fjsp_lp_limits.h lp_device_lds_bytes)
        K, M = a.p.shape
        nr = K + M + (K - len(a.Jr))
        return nr * (int((a.p > 0).sum()) + 1 + nr + 1) * 8
    insts = [a for a in insts if tableau_bytes(a) < 130 * 1024]      # (the industrial folders and the generated ones; not data/HMPSAC)
    assert len(insts) >= 4
    s = H.instance_set_from(insts)
    N, T = 96, 1600
    acts = torch.from_numpy(global_actions(29, 0, N, T, 12, 10)).cuda()
    mo = torch.zeros(N, 4, dtype=torch.float64, device="cuda"); mo[:, 0] = 1.0

    def play(impl):
        with H.env_var("FJSP_LP_IMPL", impl):
            b = EnvBatch(s, N, variant=VARIANT_MO_DFJSP, rng_seed=5)
        b.reset()
        rew = torch.zeros(T, N, dtype=torch.float64, device="cuda")
        for t in range(T):
            live = b.done == 0
            _, r, d = b.step(acts[t], mo=mo)
            rew[t] = torch.where(live, r, torch.zeros_like(r))
            if t % 50 == 49 and bool((b.done != 0).all()):
                break
        return b, rew, b.read()

    dev, rew_d, fin_d = play("device")
    host, rew_h, fin_h = play("host")
    assert dev.lp_on_device == 1 and host.lp_on_device == 0
    assert dev.lp_device_pivots > 0 and host.lp_device_pivots == 0
    assert bool((fin_d["done"] != 0).all())
    assert torch.equal(rew_d, rew_h)
    for k in ("delay_time_sum", "makespan", "completion_time", "step_count", "energy_consumption", "done", "status"):
        assert torch.equal(fin_d[k], fin_h[k]), k
    assert dev.lp_solves == host.lp_solves > 0


# ------------------------------------------------------------------------------------------------ the generated cases
def _device_batch(arrs, n_envs, variant=0):
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    with H.env_var("FJSP_LP_IMPL", "device"):
        b = EnvBatch(LC.instance_set(arrs), n_envs, variant=variant, rng_seed=1)
    assert b.lp_on_device == 1
    return b


def test_device_lp_equals_the_host_lp_on_every_generated_case(torch_gpu):
    """Every case and state of tests/lp_cases.py through lp_device_solve: x bit for bit.  (Which pivot loop, row half and
    ratio-test branch each LP takes: tests/test_lp_reference.py::test_generated_cases_keep_their_coverage.)"""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    checked = 0
    for c in LC.cases():
        a = c.arr
        b = _device_batch([a], 4)
        for t, (name, Q, now) in enumerate(c.states):
            want, _ = fi.fluid_lp(a.Jr, a.p, Q, now)
            got = b.lp_device_solve(t % 4, Q, now)[:a.K * a.M].reshape(a.K, a.M)
            assert np.array_equal(H.bits(got), H.bits(want)), "case %s state %s" % (c.name, name)
            checked += 1
    assert checked >= 60


def test_device_lp_in_a_batch_of_instances_of_different_widths(torch_gpu):
    """One batch of six instances from 1 to 8 chunks wide (the batch's machine stride is the widest instance's, its LDS the
    largest tableau's): the hook picks the instance by env % n_inst, and every LP is the host's bit for bit -- a narrow
    tableau after a wide one on the same handle and the reverse."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    cases = {c.name: c for c in LC.cases()}
    group = [cases[n] for n in ("c2", "c8", "d111", "c6", "rows4b", "c3")]
    arrs = [c.arr for c in group]
    assert LC.fits_device(arrs)
    b = _device_batch(arrs, 3 * len(arrs))
    for rnd in range(3):
        for i, c in enumerate(group):
            a = c.arr
            name, Q, now = c.states[(rnd + i) % len(c.states)]
            want, _ = fi.fluid_lp(a.Jr, a.p, Q, now)
            got = b.lp_device_solve(i + rnd * len(arrs), Q, now)[:a.K * a.M].reshape(a.K, a.M)
            assert np.array_equal(H.bits(got), H.bits(want)), "case %s state %s round %d" % (c.name, name, rnd)


# ---------------------------------------------------------------------------------------------------- the service path
def _play_both(torch, make_batch, N, T, acts, mo):
    """The same batch played with the LPs on the device and on the host; the equalities of
    test_device_lp_service_leaves_every_trajectory_unchanged.  Returns (device batch, largest rise of lp_solves in one step)."""
    def play(impl):
        with H.env_var("FJSP_LP_IMPL", impl):
            b = make_batch()
        b.reset()
        rew = torch.zeros(T, N, dtype=torch.float64, device="cuda")
        rise, solved = 0, 0
        for t in range(T):
            live = b.done == 0
            _, r, d = b.step(acts[t], mo=mo)
            rew[t] = torch.where(live, r, torch.zeros_like(r))
            now = b.lp_solves
            rise, solved = max(rise, now - solved), now
            if bool((b.done != 0).all()):
                break
        return b, rew, b.read(), rise

    dev, rew_d, fin_d, rise_d = play("device")
    host, rew_h, fin_h, rise_h = play("host")
    assert dev.lp_on_device == 1 and host.lp_on_device == 0
    assert dev.lp_device_pivots > 0 and host.lp_device_pivots == 0
    assert bool((fin_d["done"] != 0).all())
    assert torch.equal(rew_d, rew_h)
    for k in ("delay_time_sum", "makespan", "completion_time", "step_count", "energy_consumption", "done", "status"):
        if k in fin_h or k in fin_d:
            assert torch.equal(fin_d[k], fin_h[k]), k
    assert dev.lp_solves == host.lp_solves > 0
    assert rise_d == rise_h
    return dev, rise_d


@pytest.mark.parametrize("name", ["c4", "c6", "c8"])
def test_device_lp_service_on_wide_tableaus(torch_gpu, name):
    """MO_DFJSP batches of the 4-, 6- and 8-chunk instances, random rule pairs: the order-arrival LPs on the device leave
    rewards, totals and the number of LPs as the host service gives them."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, VARIANT_MO_DFJSP, global_actions
    a = next(c.arr for c in LC.cases() if c.name == name)
    assert ((a.p > 0).sum(0) > 0).all()                          # (MO_DFJSP: every machine has an eligible operation)
    N, T = 48, 4 * a.K + 8                                       # two orders of two jobs per kind: 4 K operations
    acts = torch.from_numpy(global_actions(31, 0, N, T, 12, 10)).cuda()
    mo = torch.zeros(N, 4, dtype=torch.float64, device="cuda"); mo[:, 0] = 1.0

    def make_batch():
        s = LC.instance_set([a]).generate_machine_data(0, 7)
        return EnvBatch(s, N, variant=VARIANT_MO_DFJSP, rng_seed=5)

    _play_both(torch, make_batch, N, T, acts, mo)


def _late_order(name, seed, M, **kw):
    """Jr and job counts of case c6 (44 operations in the first order) with the second order arriving long after the first
    is dispatched: every environment of the batch then reaches its order arrival in the same vector step -- the one that
    dispatches its 44th operation (the clock jumps to the arrival, SO_FJSSP.py:231) -- whatever rules it plays."""
    return LC.make_instance(name, seed, [2] * 7 + [1] * 8, M, arrive1=100000, **kw)


def test_more_device_lps_in_one_launch_than_workgroups(torch_gpu):
    """lp_device_kernel launches at most 256 workgroups, which stride over the parked environments and re-use their LDS:
    640 environments of one small instance play the same non-random rule pair, park in the same step, and the 640 LPs of
    that one launch leave every trajectory as the host service does."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    a = _late_order("late2", 41, 3)                              # 44 rows x 112 columns: 2 chunks
    N, T = 640, 4 * a.K + 8
    acts = torch.zeros(T, N, 2, dtype=torch.uint8, device="cuda")
    acts[..., 0], acts[..., 1] = 2, 1                            # largest fluid gap, shortest processing time: no random.choice
    dev, rise = _play_both(torch, lambda: EnvBatch(LC.instance_set([a]), N, variant=0, rng_seed=5), N, T, acts, None)
    assert rise > 256 and rise == N


def test_narrow_and_wide_tableaus_share_a_workgroups_lds(torch_gpu):
    """A 2-chunk and a 6-chunk instance interleaved by env % n_inst, random rule pairs, 600 environments that all park in the
    same step: each of the 256 workgroups solves two or three LPs of that launch one after the other in the same LDS, narrow
    after wide and wide after narrow (`dims` and `s_fail` are shared across them)."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, global_actions
    narrow, wide = _late_order("late2", 41, 3), _late_order("late6", 42, 15)     # 44 x 112 and 44 x 376
    assert LC.fits_device([narrow, wide])
    assert [(int((x.p > 0).sum()) + 2 * x.K - x.R + x.M + 2 + 63) // 64 for x in (narrow, wide)] == [2, 6]
    N, T = 600, 4 * wide.K + 8
    acts = torch.from_numpy(global_actions(37, 0, N, T, 6, 5)).cuda()
    dev, rise = _play_both(torch, lambda: EnvBatch(LC.instance_set([narrow, wide]), N, variant=0, rng_seed=5), N, T, acts, None)
    assert rise == N


# -------------------------------------------------------------------------------------------------- the create-time rule
class _without_env_var(object):
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.old = os.environ.pop(self.name, None)

    def __exit__(self, *exc):
        if self.old is not None:
            os.environ[self.name] = self.old


def test_create_rule_at_its_boundaries(torch_gpu):
    """choose_lp_service (csrc/fjsp_env.hip): FJSP_LP_IMPL=device puts the LPs on the device exactly when the restated
    lp_device_lds_bytes of the largest tableau is within 156 KB (159 744 B) and the tableau within 512 columns; without the
    variable the device serves batches from 16 384 environments on; FJSP_LP_IMPL=host never does.
    (No tableau of 512 columns fits 156 KB -- tests/test_lp_reference.py sweeps it -- so at 512 and 513 columns it is the
    LDS term that refuses; the prediction is the restated rule's either way.)"""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    Jr, M = [2] + [1] * 18, 21                                   # case c8's shape: 42 rows in the worst case
    K, R = 20, 19
    fit = max(nx for nx in range(K, K * M + 1) if LC.lds_bytes(K, M, nx, R, M) <= LC.LDS_LIMIT)
    assert LC.LDS_LIMIT - 344 < LC.lds_bytes(K, M, fit, R, M) <= LC.LDS_LIMIT < LC.lds_bytes(K, M, fit + 1, R, M)
    shapes = [LC.make_instance("under", 51, Jr, M, nx=fit), LC.make_instance("over", 52, Jr, M, nx=fit + 1),
              LC.make_instance("col512", 53, [1] * 22, 22, nx=466), LC.make_instance("col513", 54, [1] * 22, 22, nx=467)]
    assert [int((a.p > 0).sum()) + 2 * a.K - a.R + a.M + 2 for a in shapes[2:]] == [512, 513]
    seen = []
    for a in shapes:
        with H.env_var("FJSP_LP_IMPL", "device"):
            b = EnvBatch(LC.instance_set([a]), 4, variant=0, rng_seed=1)
        assert b.lp_on_device == int(LC.fits_device([a])), a.name
        seen.append(b.lp_on_device)
        if a.name == "under":                                    # the largest allocation the rule lets through holds its LP
            _, Q, now = LC.make_states(a, 151)[0]
            want, _ = fi.fluid_lp(a.Jr, a.p, Q, now)
            got = b.lp_device_solve(0, Q, now)[:a.K * a.M].reshape(a.K, a.M)
            assert np.array_equal(H.bits(got), H.bits(want))
        del b
    assert seen == [1, 0, 0, 0]
    small = next(c.arr for c in LC.cases() if c.name == "c2")
    s = LC.instance_set([small])
    with _without_env_var("FJSP_LP_IMPL"):
        assert EnvBatch(s, 16383, variant=0, rng_seed=1).lp_on_device == 0
        assert EnvBatch(s, 16384, variant=0, rng_seed=1).lp_on_device == 1
    with H.env_var("FJSP_LP_IMPL", "host"):
        assert EnvBatch(s, 4, variant=0, rng_seed=1).lp_on_device == 0
        assert EnvBatch(s, 16384, variant=0, rng_seed=1).lp_on_device == 0


# ------------------------------------------------------------------------------------------------------ graceful failures
def test_hook_refuses_bad_inputs_and_stays_usable(torch_gpu):
    """Q[k] = 0 is FJSP_E_LP, as the host solver refuses it; a Q[k] or n_now[k] outside 0 ... 65 535 is FJSP_E_ARG (the
    device stages 16-bit counts: 65 536 must not arrive as 0, nor 65 537 as 1).  After either the same handle solves a
    valid LP bit for bit: the error word was cleared."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd._capi import FjspError
    c = next(c for c in LC.cases() if c.name == "c4")
    a = c.arr
    b = _device_batch([a], 4)
    _, Q, now = c.states[1]

    def solves_exactly():
        want, _ = fi.fluid_lp(a.Jr, a.p, Q, now)
        got = b.lp_device_solve(1, Q, now)[:a.K * a.M].reshape(a.K, a.M)
        assert np.array_equal(H.bits(got), H.bits(want))

    solves_exactly()
    Q0 = Q.copy(); Q0[3] = 0
    with pytest.raises(FjspError) as ei:
        fi.fluid_lp(a.Jr, a.p, Q0, now)
    assert ei.value.code == -4                                   # FJSP_E_LP
    with pytest.raises(FjspError) as ei:
        b.lp_device_solve(0, Q0, now)
    assert ei.value.code == -4
    solves_exactly()
    for which, value in (("Q", 65536), ("Q", 65537), ("Q", -1), ("now", 65536), ("now", -1)):
        Qb, nb = Q.copy(), now.copy()
        (Qb if which == "Q" else nb)[5] = value
        with pytest.raises(FjspError) as ei:
            b.lp_device_solve(0, Qb, nb)
        assert ei.value.code == -1, (which, value)               # FJSP_E_ARG
    solves_exactly()
    Qt = Q.copy(); Qt[5] = 65535                                 # the largest count the device stages
    want, _ = fi.fluid_lp(a.Jr, a.p, Qt, now)
    got = b.lp_device_solve(2, Qt, now)[:a.K * a.M].reshape(a.K, a.M)
    assert np.array_equal(H.bits(got), H.bits(want))
