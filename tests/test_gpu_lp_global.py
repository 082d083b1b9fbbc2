"""GPU: the device simplex with its tableau in global memory (csrc/fjsp_lp_global.hip, FJSP_LP_IMPL=global).

It restates the host simplex (csrc/fjsp_lp.cpp) pivot for pivot, so the reference is the host solver and the bar is BIT
equality of x (`H.bits`): through the hook `lp_device_solve` on the generated cases of tests/lp_global_cases.py (three and
four row groups, 9 and 21 chunks of 64 columns, both together, the row and the column limit on either side), on the
reference's own instances beyond the LDS, on a batch in which narrow and wide tableaus take turns in one scratch slot;
through the order-arrival service (trajectories equal the host service's; more LPs in one launch than scratch slots);
and through the device generator's third LP list on the MPPPO training distribution, where no LP goes to the host any more.
tests/test_lp_global_reference.py counts on the CPU which branches the generated cases take.

Every handle is created under FJSP_LP_IMPL=global.  Failures are only ever the graceful ones (an input the host solver
refuses too); nothing here provokes a device fault.
"""
import numpy as np
import pytest

from tests import helpers as H
from tests import lp_cases as LC
from tests import lp_global_cases as GC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _global_batch(s, n_envs, variant=0, rng_seed=1):
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    with H.env_var("FJSP_LP_IMPL", "global"):
        return EnvBatch(s, n_envs, variant=variant, rng_seed=rng_seed)


def _check_states(b, a, states, what, env0=0):
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    n = 0
    for t, (name, Q, now) in enumerate(states):
        want, _ = fi.fluid_lp(a.Jr, a.p, Q, now)
        got = b.lp_device_solve(env0 + (t % 4) * b.n_inst, Q, now)[:a.K * a.M].reshape(a.K, a.M)
        assert np.array_equal(H.bits(got), H.bits(want)), "%s state %s" % (what, name)
        n += 1
    return n


# ------------------------------------------------------------------------------------------------ 1. the generated cases
def test_global_lp_equals_the_host_lp_on_every_generated_case(torch_gpu):
    """Every case and state of tests/lp_global_cases.py through lp_device_solve on a 4-environment batch: x bit for bit."""
    checked = 0
    for c in GC.cases():
        b = _global_batch(LC.instance_set([c.arr]), 4)
        assert b.lp_on_device == 2, c.name
        checked += _check_states(b, c.arr, c.states, "case " + c.name)
    assert checked == 20


def test_global_lp_at_its_row_and_column_limits(torch_gpu):
    """256 rows and 1536 columns are admitted and solved bit for bit; 257 rows and 1537 columns keep the host service."""
    seen = {}
    for c, admitted in GC.limit_cases():
        b = _global_batch(LC.instance_set([c.arr]), 4)
        seen[c.name] = b.lp_on_device
        if admitted:
            assert b.lp_on_device == 2, c.name
            _check_states(b, c.arr, c.states, "case " + c.name)
        del b
    assert seen == {"l_rows256": 2, "l_rows257": 0, "l_cols1536": 2, "l_cols1537": 0}


# ------------------------------------------------------------------------------------------------ 2. the fixture instances
def _fixture(suite, name):
    return next(a for a in H.load_suite(suite)[0] if a.name.endswith(name))


@pytest.mark.parametrize("suite,name", [("mo_dfjsp", "HMPSAC/DDT0.5_M10_S1"), ("mo_dfjsp", "HMPSAC/DDT1.0_M15_S3"),
                                        ("multiorder", "HMPSAC/DDT0.5_M20_S3"), ("large", "MPPPO/DDT1.0_M15_R10"),
                                        ("large", "MPPPO/DDT0.5_M20_R5"), ("so_dfjsp", "Mk01"), ("large", "Mk04")])
def test_global_lp_equals_the_host_lp_on_the_reference_instances(torch_gpu, suite, name):
    """The reference's own instances beyond the LDS: the reset-time LP and five random live states (jobs spread over the
    stages, so precedence rows come and go with n_now == 0), built as in test_gpu_lp_device.py.  MO_DFJSP and multi-order
    instances play their own variant; a single-order instance gets generated machine data and plays MO_DFJSP, the one
    variant that gives such a batch an order-arrival service and with it the hook."""
    from deep_reinforcement_learning_for_fjsp_amd.batch import VARIANT_MO_DFJSP
    a = _fixture(suite, name)
    assert not LC.fits_device([a]) and GC.within_global(a)
    if suite == "mo_dfjsp":
        s, variant = H.instance_set_from([a]), VARIANT_MO_DFJSP
    elif a.S > 1:
        s, variant = H.instance_set_from([a]), 0
    else:
        s, variant = H.instance_set_from([a]).generate_machine_data(0, 7), VARIANT_MO_DFJSP
    b = _global_batch(s, 4, variant=variant)
    assert b.lp_on_device == 2
    rs = np.random.RandomState(17)
    koff = np.concatenate([[0], np.cumsum(a.Jr)])
    states = []
    for trial in range(6):
        Q = np.zeros(a.K, np.int32); now = np.zeros(a.K, np.int32)
        for r in range(len(a.Jr)):
            n = int(rs.randint(1, 25))
            if trial == 0:
                stages = np.zeros(n, np.int64)                             # every job at stage 0: the reset-time LP
            else:
                stages = rs.randint(0, a.Jr[r], n)                          # jobs spread over the stages (one stays at the last)
                stages[0] = a.Jr[r] - 1 if trial % 2 else stages[0]
            for j in range(a.Jr[r]):
                Q[koff[r] + j] = max(1, int((stages <= j).sum()))
                now[koff[r] + j] = int((stages == j).sum())
        states.append(("trial%d" % trial, Q, now))
    assert _check_states(b, a, states, "%s/%s" % (suite, name)) == 6


# --------------------------------------------------------------------------------------- 3. tableaus of different sizes
def test_narrow_and_wide_tableaus_take_turns_in_one_scratch_slot(torch_gpu):
    """One batch of c2 (25 x 87), g_cols9 (56 x 538) and g_rows4 (200 x 402): the hook solves in slot 0 of the pool, a narrow
    tableau after a wide one and the reverse, a two-group after a four-group one; every LP is the host's bit for bit."""
    by_name = {c.name: c for c in LC.cases() + GC.cases()}
    group = [by_name[n] for n in ("c2", "g_cols9", "g_rows4")]
    arrs = [c.arr for c in group]
    b = _global_batch(LC.instance_set(arrs), 3 * len(arrs))
    assert b.lp_on_device == 2
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    for rnd in range(3):
        for i in (0, 1, 2) if rnd % 2 == 0 else (2, 1, 0):
            c = group[i]
            a = c.arr
            name, Q, now = c.states[(rnd + i) % len(c.states)]
            want, _ = fi.fluid_lp(a.Jr, a.p, Q, now)
            got = b.lp_device_solve(i + rnd * len(arrs), Q, now)[:a.K * a.M].reshape(a.K, a.M)
            assert np.array_equal(H.bits(got), H.bits(want)), "case %s state %s round %d" % (c.name, name, rnd)


# ---------------------------------------------------------------------------------------------------- 4. the service path
def _play(torch, make_batch, impl, N, T, acts, mo):
    with H.env_var("FJSP_LP_IMPL", impl):
        b = make_batch()
    b.reset()
    rew = torch.zeros(T, N, dtype=torch.float64, device="cuda")
    rise, solved = 0, 0
    for t in range(T):
        live = b.done == 0
        _, r, d = b.step(acts[t], mo=mo)
        rew[t] = torch.where(live, r, torch.zeros_like(r))
        if t % 16 == 15 or t + 1 == T:
            now = b.lp_solves
            rise, solved = max(rise, now - solved), now
            if bool((b.done != 0).all()):
                break
    return b, rew, b.read(), rise


def _play_both(torch, make_batch, N, T, acts, mo):
    glo, rew_g, fin_g, rise_g = _play(torch, make_batch, "global", N, T, acts, mo)
    host, rew_h, fin_h, rise_h = _play(torch, make_batch, "host", N, T, acts, mo)
    assert glo.lp_on_device == 2 and host.lp_on_device == 0
    assert glo.lp_device_pivots > 0 and host.lp_device_pivots == 0
    assert bool((fin_g["done"] != 0).all())
    assert torch.equal(rew_g, rew_h)
    for k in ("delay_time_sum", "makespan", "completion_time", "energy_consumption", "step_count", "done", "status"):
        if k in fin_h or k in fin_g:
            assert torch.equal(fin_g[k], fin_h[k]), k
    assert glo.lp_solves == host.lp_solves > 0
    return glo, rise_g


def test_global_lp_service_leaves_every_trajectory_unchanged(torch_gpu):
    """MO_DFJSP on the two data/HMPSAC fixtures of the mo_dfjsp suite (91 x 328 and 113 x 538), 16 environments, random
    rule pairs, played to done with FJSP_LP_IMPL=global and =host: rewards step by step, the totals and the number of LPs
    are identical."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, VARIANT_MO_DFJSP, global_actions
    insts = [a for a in H.load_suite("mo_dfjsp")[0] if a.name.startswith("HMPSAC/")]
    assert len(insts) == 2 and not any(LC.fits_device([a]) for a in insts)
    s = H.instance_set_from(insts)
    N = 16
    T = max(int((a.count.sum(0) * a.Jr).sum()) for a in insts) + 16
    acts = torch.from_numpy(global_actions(29, 0, N, T, 12, 10)).cuda()
    mo = torch.zeros(N, 4, dtype=torch.float64, device="cuda"); mo[:, 0] = 1.0
    _play_both(torch, lambda: EnvBatch(s, N, variant=VARIANT_MO_DFJSP, rng_seed=5), N, T, acts, mo)


def test_more_global_lps_in_one_launch_than_scratch_slots(torch_gpu):
    """300 environments of a 56 x 538 instance whose second order arrives long after the first is dispatched play the same
    non-random rule pair and park in the same step: 300 LPs in one launch of at most 256 workgroups, each with its slot."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    a = LC.make_instance("late9", 33, [2] * 12, 20, arrive1=100000)          # g_cols9's shape
    assert GC.shape(a) == (56, 538)
    N, T = 300, 4 * a.K + 8
    acts = torch.zeros(T, N, 2, dtype=torch.uint8, device="cuda")
    acts[..., 0], acts[..., 1] = 2, 1                            # largest fluid gap, shortest processing time: no random.choice
    s = LC.instance_set([a])

    def play(impl):
        with H.env_var("FJSP_LP_IMPL", impl):
            b = EnvBatch(s, N, variant=0, rng_seed=5)
        b.reset()
        rew = torch.zeros(T, N, dtype=torch.float64, device="cuda")
        rise, solved = 0, 0
        for t in range(T):
            live = b.done == 0
            _, r, d = b.step(acts[t])
            rew[t] = torch.where(live, r, torch.zeros_like(r))
            now = b.lp_solves
            rise, solved = max(rise, now - solved), now
            if bool((b.done != 0).all()):
                break
        return b, rew, b.read(), rise

    glo, rew_g, fin_g, rise_g = play("global")
    host, rew_h, fin_h, rise_h = play("host")
    assert glo.lp_on_device == 2 and host.lp_on_device == 0
    assert rise_g == rise_h == N > 256
    assert torch.equal(rew_g, rew_h) and bool((fin_g["done"] != 0).all())
    for k in fin_h:
        assert torch.equal(fin_g[k], fin_h[k]), k
    assert glo.lp_solves == host.lp_solves > 0 and glo.lp_device_pivots > 0


# ------------------------------------------------------------------------------------------------- 5. the generated route
def test_generated_mpppo_batch_solves_no_lp_on_the_host(torch_gpu):
    """The MPPPO training distribution (K <= 60, M <= 20, K - R <= 48: at most 128 rows x 1330 columns) generated on the
    device under FJSP_LP_IMPL=global: the LPs beyond the LDS go to the global-memory simplex, none to the host threads, and
    every x is the host solver's bit for bit -- after the create and after a regenerate onto other seeds."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    q = fi.reference_training_ranges("mpppo")
    with H.env_var("FJSP_LP_IMPL", "global"):
        G = EnvBatch.generated(q, 64, 1000)
    for seed in (1000, 5000):
        if seed != 1000:
            G.regenerate(seed)
        st = G.generated_stats()
        assert st["instances"] == 64 and st["lp_host"] == 0 and st["lp_global"] > 0, st
        assert st["lp_device"] + st["lp_global"] == 64 and st["global_pivots"] > 0 and st["ms"]["lp_global"] > 0.0, st
        s = fi.InstanceSet(64).generate_range(seed, q).solve_fluid()
        n_glob = 0
        for i in range(64):
            a, want = G.instance_arrays(i), s.arrays(i)
            assert np.array_equal(a.p, want.p), (seed, i)
            assert np.array_equal(H.bits(a.x), H.bits(want.x)), (seed, i)
            nx = int((np.asarray(want.p) > 0).sum())                # (the LDS rule in a batch padded to M_max machines)
            fits = LC.lds_bytes(want.K, want.M, nx, want.R, q.M_max) <= LC.LDS_LIMIT and nx + 2 * want.K + want.M - want.R + 2 <= LC.MAX_COLUMNS
            n_glob += 0 if fits else 1
        assert n_glob == st["lp_global"], (seed, st)


# ---------------------------------------------------------------------------------------------------- 6. graceful failures
def test_hook_refuses_bad_inputs_and_stays_usable(torch_gpu):
    """Q[k] = 0 is FJSP_E_LP, as the host solver refuses it; a count of 65 536 is FJSP_E_ARG; after either the same handle
    solves a valid LP bit for bit."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd._capi import FjspError
    c = next(c for c in GC.cases() if c.name == "g_both")
    a = c.arr
    b = _global_batch(LC.instance_set([a]), 4)
    assert b.lp_on_device == 2
    _, Q, now = c.states[1]

    def solves_exactly():
        want, _ = fi.fluid_lp(a.Jr, a.p, Q, now)
        got = b.lp_device_solve(1, Q, now)[:a.K * a.M].reshape(a.K, a.M)
        assert np.array_equal(H.bits(got), H.bits(want))

    solves_exactly()
    Q0 = Q.copy(); Q0[3] = 0
    with pytest.raises(FjspError) as ei:
        b.lp_device_solve(0, Q0, now)
    assert ei.value.code == -4                                   # FJSP_E_LP
    solves_exactly()
    for which in ("Q", "now"):
        Qb, nb = Q.copy(), now.copy()
        (Qb if which == "Q" else nb)[5] = 65536
        with pytest.raises(FjspError) as ei:
            b.lp_device_solve(0, Qb, nb)
        assert ei.value.code == -1, which                        # FJSP_E_ARG
    solves_exactly()
