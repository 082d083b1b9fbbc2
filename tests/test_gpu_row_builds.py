"""GPU: the builds of the row kernels (csrc/fjsp_group.hip, one 16-lane row per environment) that large batches run,
against the C oracle at their edges.

The launcher picks a build per launch, and EnvBatch.row_build reports which, from the function the launchers decide
with: the per-step kernel is the small-batch "early" build up to a crossover and the register-lean build beyond it;
the machine capacity MPC is 5 or 8 after the batch's largest machine count; the fused kernel is always lean, with the
instance's static tables resident in LDS while the waves a CU gets fit, and read from memory beyond.  The randomised
differential test runs at 62 environments (early build, resident fused kernel); the large-batch tests run 10x5
SO_FJSSP only.  Here every case runs for SO_FJSSP, SO_DFJSP and MO_FJSSP_discretes on two instance sets:

  * "mp5" (largest M = 5: MPC 5, M = 1..5) and "mp8" (largest M = 8: MPC 8, rows of M = 1..8), one job per kind,
    operation-type counts K of exactly 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63 and 64 plus random fill,
    eligibility from one machine to all M, processing times in [2000, 65535] in a quarter of them (clocks beyond
    2^16); mp8 also holds instances where every type runs on all 7 or 8 machines with its fluid solution spread over
    all of them, so that Machine.gap_ave ranks 7 or 8 candidates at a clock > 0 (three passes of the lean walk);
  * env e plays instance 2 + e % n_inst: the first wave mixes K = 1 and K = 64, the second holds only K <= 16, and
    n_inst is no multiple of 4, so every wave composition recurs shifted;
  * actions are batch.global_actions over the variant's whole action space (random-choice rules included), so a
    batch of n environments plays the first n of the 5121 environments the oracle replays.

Cases (sizes; the build each asserts): lean per step against the oracle (5121; early 0): choices, rewards, done and
states at every step, then the totals; early against lean on the same environments (5120; early 1), bit for bit at
every step; the fused kernel at the residency boundary (4096 / 4097 at MPC 5, 3072 / 3073 at MPC 8, and 5121;
resident 1 / 0 / 0), with and without a final state, against the per-step results; steps without a state (5121);
autoreset and masked reset (5121); recording through the lean per-step and the non-resident fused kernel (5121)
against schedule.from_trace of every oracle replay; a batch with as many instances as environments (5121, mp8,
SO_FJSSP: g_open without the modulo); FJSP_GROUP_KENV=0 (the fourth-slot round trip of the lean build), bit-equal to
the default batch.
"""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

FIRST = 2                        # the instances sit at an offset inside the set
N_LEAN = 5121                    # per-step launches: the lean build (asserted through row_build)
N_EARLY = 5120                   # ... and the early build
RESIDENT_EDGE = {"mp5": 4096, "mp8": 3072}      # fused kernel: the largest batch with resident tables (asserted)
RNG = 4242
ACTION_SEED = 77
N_ACTIONS = {0: (6, 5), 5: (6, 5), 2: (18, 1)}
DET = {0: (2, 0), 5: (2, 0), 2: (0, 0)}         # deterministic rule pairs (the random.choice stream goes on across resets)
KW = {0: {}, 5: {}, 2: dict(mo=True)}
TOTALS = ("delay_time_sum", "makespan", "step_time", "step_count", "completion_time")

# (kinds R, stages J) in instance order: K = R x J.  Instances 0-3 (the first wave) mix K = 1 and K = 64, instances 4-7
# (the second wave) have K <= 16; every count of the module docstring appears.
SHAPES = [(1, 1), (8, 8), (1, 1), (1, 64),
          (2, 1), (1, 2), (15, 1), (4, 4),
          (8, 2), (1, 16), (1, 17), (1, 31), (4, 8), (2, 16), (3, 11), (11, 3), (1, 47), (12, 4), (3, 16), (7, 7),
          (9, 7), (7, 9), (4, 16), (5, 3), (3, 5), (2, 8), (6, 8), (13, 1), (3, 21), (2, 32)]
N_RANDOM = {"mp5": 12, "mp8": 11}              # (n_inst: 42 and 45)
# mp8 only (set_raw): every operation type eligible on all M machines, (R, J, M); their fluid solution x is spread over
# every machine (set_x), so every idle machine is a fluid machine and one job (R = 1) finds all M idle at every step
FULL_ELIG = [(1, 24, 8), (1, 30, 7), (2, 10, 8), (3, 8, 8)]


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _feasible(s, i, variant):
    # SO_DFJSP divides by the operation count of every machine (class_FJSP.py:159): none may have zero
    return variant != 5 or bool((s.arrays(i).p > 0).any(axis=0).all())


def _generate(s, i, seed, R, J, M, long, variant, rs):
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    pmin, pmax = (2000, 65535) if long else (1, int(rs.randint(2, 60)))
    prm = fi.GenParams(R_min=R, R_max=R, J_min=J, J_max=J, M=M, p_min=pmin, p_max=pmax, N_min=1, N_max=1, S=1,
                       DDT=float(rs.choice([0.5, 1.0, 1.5])), t_si_min=20.0, t_si_max=80.0)
    s.generate(i, seed, prm)
    while not _feasible(s, i, variant):
        seed += 7919
        s.generate(i, seed, prm)


def _all_eligible(s, i, R, J, M, long, rs):
    K = R * J
    p = rs.randint(2000, 65536, (K, M)) if long else rs.randint(1, 40, (K, M))
    elig = np.tile(np.arange(M, dtype=np.int32), (K, 1))
    s.set_raw(i, np.full(R, J), p, np.full(K, M), elig, np.ones(R), [0], [int(p.mean() * K / 2)], ddt=1.0)


def build_instances(mp, variant, n_inst=None, seed_base=0):
    """The instance set `mp` ("mp5" / "mp8") for `variant`: SHAPES in order, then random fill (and in mp8 the
    all-eligible instances), M = 1..MP by the instance index.  n_inst: that many instances, the same plan repeated with
    other seeds.  Returns (InstanceSet, n_inst); the instances sit at FIRST."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    MP = 5 if mp == "mp5" else 8
    rs = np.random.RandomState(9000 + 10 * MP + variant + seed_base)
    plan = [(R, J, None) for R, J in SHAPES]
    for _ in range(N_RANDOM[mp]):
        R = int(rs.randint(1, 16))
        plan.append((R, int(rs.randint(1, 64 // R + 1)), None))
    if mp == "mp8":
        plan[12:12] = FULL_ELIG
    if n_inst is not None:
        plan = [plan[i % len(plan)] for i in range(n_inst)]
    n = len(plan)
    s = fi.InstanceSet(FIRST + n)
    for i, (R, J, M) in enumerate(plan):
        long = i % 4 == 3                      # a quarter: p in [2000, 65535]
        if M is not None:
            _all_eligible(s, FIRST + i, R, J, M, long, rs)
        else:
            # (the K = 1 instances of the first wave get M = MP and M = 1)
            M = MP if i in (0, 1) else (1 if i == 2 else 1 + (i * 3) % MP)
            _generate(s, FIRST + i, 70000 + 1000 * MP + 100 * variant + seed_base + 7 * i, R, J, M, long, variant, rs)
    s.solve_fluid(FIRST, n)
    for i, (R, J, M) in enumerate(plan):
        if M is not None:
            s.set_x(FIRST + i, np.full((R * J, M), 1.0 / M))
    assert max(s.dims(FIRST + i)["M"] for i in range(n)) == MP
    return s, n


def global_actions(variant, n, T):
    from deep_reinforcement_learning_for_fjsp_amd.batch import global_actions as ga
    n0, n1 = N_ACTIONS[variant]
    return ga(ACTION_SEED + variant, 0, n, T, n0, n1)


def mo_rows(variant, n):
    """MO_FJSSP_discretes: step()'s weight rows of the first n global envs (the three kinds of the randomised test)."""
    if variant != 2:
        return None
    rs = np.random.RandomState(31)
    kinds, w0 = rs.randint(0, 3, N_LEAN), np.round(rs.rand(N_LEAN), 2)
    cn, tn = rs.randint(20, 90, N_LEAN), rs.randint(30, 400, N_LEAN)
    rows = [(1.0, 0.0, -1.0, -1.0) if k == 0 else (0.0, 1.0, -1.0, -1.0) if k == 1 else
            (float(w0[e]), float(1.0 - w0[e]), float(cn[e]), float(tn[e])) for e, k in enumerate(kinds)]
    return rows[:n]


def replay(s, n_inst, variant, actions_h, mo):
    """Every environment of a batch (rng_seed RNG, first_env 0) replayed on the C oracle: H.play_oracle dicts."""
    from deep_reinforcement_learning_for_fjsp_amd.batch import ENV_SEED_STRIDE
    out = []
    for e in range(actions_h.shape[1]):
        a = s.arrays(FIRST + e % n_inst)
        seed = (RNG + e * ENV_SEED_STRIDE) & (2 ** 64 - 1)
        out.append(H.play_oracle(a, a.x, actions_h[:, e], seed, variant=variant, mo=None if mo is None else mo[e]))
    return out


def steps(torch, b, acts, mo, stateless_until=0):
    """reset(), then every step of acts (device u8[T, N, 2]) through the per-step launch, traced; steps t <
    stateless_until return no state.  Numpy: state [T, N, S], reward, done [T, N], trace [T, N, 2], state0, fin (read())."""
    T, N = acts.shape[0], b.N
    st = torch.zeros(T, N, b.state_size, dtype=torch.float64, device=b.device)
    rw = torch.zeros(T, N, dtype=torch.float64, device=b.device)
    dn = torch.zeros(T, N, dtype=torch.uint8, device=b.device)
    tr = torch.zeros(T, N, 2, dtype=torch.int16, device=b.device)
    st0 = b.reset().cpu().numpy()
    for t in range(T):
        b.step(acts[t], mo=mo, state=t >= stateless_until, state_out=st[t], reward_out=rw[t], done_out=dn[t], trace_out=tr[t])
    return dict(state=st.cpu().numpy(), reward=rw.cpu().numpy(), done=dn.cpu().numpy(), trace=tr.cpu().numpy(), state0=st0,
                fin={k: v.cpu().numpy() for k, v in b.read().items()})


def check_against_oracle(run, want, variant, tag, states_from=0):
    """A per-step run against the oracle replays of its environments: choices, rewards and done flags bit for bit at every
    step (-1 / -1 and done after the episode), states from step `states_from` on (H.assert_state_close), the totals."""
    fin = run["fin"]
    assert (fin["done"] == 1).all() and (fin["status"] & ~4 == 0).all(), tag
    for e, w in enumerate(want):
        Te, te = w["T"], "%s env %d (K=%d)" % (tag, e, w["T"])
        tr = run["trace"][:, e]
        assert np.array_equal(tr[:Te, 0], w["k"]) and np.array_equal(tr[:Te, 1], w["m"]), te + " choices"
        assert (tr[Te:] == -1).all(), te + " choices after the episode"
        assert np.array_equal(H.bits(run["reward"][:Te, e]), H.bits(w["reward"])), te + " rewards"
        assert np.array_equal(run["done"][:Te, e], w["done"]) and (run["done"][Te:, e] == 1).all(), te + " done"
        if states_from == 0:
            H.assert_state_close(run["state0"][e], w["state0"], te + " reset", **KW[variant])
        H.assert_state_close(run["state"][states_from:Te, e], w["states"][states_from:], te, **KW[variant])
        assert fin["step_count"][e] == Te and fin["step_time"][e] == w["step_time"][-1], te
        assert fin["makespan"][e] == w["makespan"] and fin["delay_time_sum"][e] == w["delay_time_sum"], te
        assert fin["completion_time"][e] == w["completion_time"], te


def assert_runs_equal(a, b, n, tag, state=True):
    """Two per-step runs, the first n environments of each, bit for bit at every step, and their totals."""
    for key in ("reward", "done", "trace") + (("state",) if state else ()):
        x, y = a[key][:, :n], b[key][:, :n]
        if x.dtype == np.float64:
            x, y = H.bits(x), H.bits(y)
        if not np.array_equal(x, y):
            t, e = np.argwhere(x != y)[0][:2]
            raise AssertionError("%s: %s differs at step %d env %d" % (tag, key, t, e))
    for key in TOTALS + ("done", "status"):
        assert np.array_equal(a["fin"][key][:n], b["fin"][key][:n]), (tag, key)


class Case(object):
    pass


@pytest.fixture(scope="module", params=[(v, mp) for v in (0, 5, 2) for mp in ("mp5", "mp8")], ids=lambda p: "v%d-%s" % p)
def case(request, torch_gpu):
    """One (variant, instance set): instances, actions, weight rows, the oracle replays of all N_LEAN environments and
    their per-step run in the lean build, which every case compares with."""
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    torch = torch_gpu
    c = Case()
    c.variant, c.mp = request.param
    c.MPC = 5 if c.mp == "mp5" else 8
    c.s, c.n_inst = build_instances(c.mp, c.variant)
    c.T = max(c.s.dims(FIRST + i)["K"] for i in range(c.n_inst))
    assert c.T == 64
    c.actions_h = global_actions(c.variant, N_LEAN, c.T)
    c.acts = torch.from_numpy(c.actions_h).cuda()
    rows = mo_rows(c.variant, N_LEAN)
    c.mo = lambda n: None if rows is None else torch.tensor(rows[:n], dtype=torch.float64).cuda()
    c.batch = lambda n: EnvBatch(c.s, n, first=FIRST, n_inst=c.n_inst, variant=c.variant, rng_seed=RNG)
    c.tag = "variant %d %s" % (c.variant, c.mp)
    c.want = replay(c.s, c.n_inst, c.variant, c.actions_h, rows)
    b = c.batch(N_LEAN)
    assert b.kernel_family == 1
    assert b.row_build() == dict(early=0, mpc=c.MPC, resident=0), c.tag
    c.lean = steps(torch, b, c.acts, c.mo(N_LEAN))
    return c


def test_lean_steps_match_the_oracle(case):
    check_against_oracle(case.lean, case.want, case.variant, case.tag + " lean")


def test_early_build_equals_the_lean_build(torch_gpu, case):
    b = case.batch(N_EARLY)
    assert b.row_build() == dict(early=1, mpc=case.MPC, resident=0), case.tag
    early = steps(torch_gpu, b, case.acts[:, :N_EARLY].contiguous(), case.mo(N_EARLY))
    assert np.array_equal(H.bits(early["state0"]), H.bits(case.lean["state0"][:N_EARLY])), case.tag
    assert_runs_equal(early, case.lean, N_EARLY, case.tag + " early vs lean")


def test_fused_kernel_at_the_residency_boundary(case):
    lean, edge = case.lean, RESIDENT_EDGE[case.mp]
    for N, resident in ((edge, 1), (edge + 1, 0), (N_LEAN, 0)):
        tag = "%s fused N=%d" % (case.tag, N)
        acts, mo, Ks = case.acts[:, :N].contiguous(), case.mo(N), lean["fin"]["step_count"][:N]
        for state in (True, False):
            b = case.batch(N)
            assert b.row_build(fused=True) == dict(early=0, mpc=case.MPC, resident=resident), tag
            b.reset()
            tr, rw, st_last = b.rollout(acts, mo=mo, state=state)
            fin = {k: v.cpu().numpy() for k, v in b.read().items()}
            assert np.array_equal(tr.cpu().numpy(), lean["trace"][:, :N]), tag + " traces"
            assert np.array_equal(H.bits(rw.cpu().numpy()), H.bits(lean["reward"][:, :N])), tag + " rewards"
            for key in TOTALS + ("done",):
                assert np.array_equal(fin[key], lean["fin"][key][:N]), (tag, state, key)
            if state:
                assert np.array_equal(H.bits(st_last.cpu().numpy()), H.bits(lean["state"][Ks - 1, np.arange(N)])), tag + " state_last"
            else:
                assert st_last is None


def test_steps_without_a_state(torch_gpu, case):
    """Steps 0..5 return no state; the steps after them rebuild v(t-1) first and must match the oracle."""
    b = case.batch(N_LEAN)
    k = 6
    run = steps(torch_gpu, b, case.acts, case.mo(N_LEAN), stateless_until=k)
    assert_runs_equal(run, case.lean, N_LEAN, case.tag + " stateless steps", state=False)
    check_against_oracle(run, case.want, case.variant, case.tag + " after stateless steps", states_from=k)


def test_autoreset_and_masked_reset(torch_gpu, case):
    torch = torch_gpu
    N, mo = N_LEAN, case.mo(N_LEAN)
    b = case.batch(N)
    b.reset()
    for t in range(case.T):
        b.step(case.acts[t], mo=mo, state=False)
    assert bool((b.done == 1).all())
    # one autoreset step = reset() + step() of a fresh batch, with a deterministic rule pair
    det = torch.tensor(DET[case.variant], dtype=torch.uint8).repeat(N, 1).cuda()
    fresh = case.batch(N)
    st0 = fresh.reset().clone()
    st_f, r_f, d_f = [x.clone() for x in fresh.step(det, mo=mo)]
    st_a, r_a, d_a = b.step(det, autoreset=True, mo=mo)
    assert torch.equal(st_a, st_f) and torch.equal(r_a, r_f) and torch.equal(d_a, d_f), case.tag
    fa, ff = b.read(), fresh.read()
    for key in TOTALS:
        assert torch.equal(fa[key], ff[key]), (case.tag, key)
    assert int((fa["status"] != 0).sum()) == 0, case.tag               # the sticky status bits were cleared
    # reset(mask) one step into the episode: the masked envs restart (and replay their first step), the others keep going
    mask = torch.from_numpy(((np.arange(N) % 3 == 0) | (np.arange(N) == N - 1)).astype(np.uint8)).cuda()
    on, off = mask.bool(), ~mask.bool()
    st_m = fresh.reset(mask).clone()
    assert torch.equal(st_m[on], st0[on]) and torch.equal(st_m[off], st_f[off]), case.tag
    st_2, r_2, _ = fresh.step(det, mo=mo)
    assert torch.equal(st_2[on], st_f[on]) and torch.equal(r_2[on], r_f[on]), case.tag


def test_recording_lean_and_non_resident(torch_gpu, case):
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    lean, N = case.lean, N_LEAN
    b = case.batch(N)
    b.record_schedule()
    rec = steps(torch_gpu, b, case.acts, case.mo(N))                      # gstep_rec_kernel<V, MPC, false>
    assert_runs_equal(rec, lean, N, case.tag + " recorded steps")
    b2 = case.batch(N)
    assert b2.row_build(fused=True) == dict(early=0, mpc=case.MPC, resident=0), case.tag
    b2.record_schedule()
    b2.reset()
    tr, rw, st_last = b2.rollout(case.acts, mo=case.mo(N))                # grollout_rec_kernel<V, MPC, false>, not resident
    Ks = lean["fin"]["step_count"]
    assert np.array_equal(tr.cpu().numpy(), lean["trace"]), case.tag + " recorded rollout traces"
    assert np.array_equal(H.bits(rw.cpu().numpy()), H.bits(lean["reward"])), case.tag + " recorded rollout rewards"
    assert np.array_equal(H.bits(st_last.cpu().numpy()), H.bits(lean["state"][Ks - 1, np.arange(N)])), case.tag
    for path, x in (("steps", b), ("rollout", b2)):
        table, length = [t.cpu().numpy() for t in x.schedule()]
        for e, w in enumerate(case.want):
            a = case.s.arrays(FIRST + e % case.n_inst)
            rows = sch.from_trace(a, w["k"], w["m"], w["job_n"], w["step_time"])
            assert length[e] == w["T"] and np.array_equal(table[e, :w["T"]], rows), (case.tag, path, e)
            assert (table[e, w["T"]:] == -1).all(), (case.tag, path, e)


def test_kenv_off_equals_the_default_batch(torch_gpu, case):
    """FJSP_GROUP_KENV=0 (read at create): the lean g_open fetches 48 operation words, and one more round trip where a
    wave has more (kmax = 64 in both sets)."""
    with H.env_var("FJSP_GROUP_KENV", "0"):
        b = case.batch(N_LEAN)
    run = steps(torch_gpu, b, case.acts, case.mo(N_LEAN))
    assert_runs_equal(run, case.lean, N_LEAN, case.tag + " FJSP_GROUP_KENV=0")


def test_as_many_instances_as_environments(torch_gpu):
    """mp8 SO_FJSSP, 5121 environments on 5121 instances: g_open's branch without the modulo."""
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    torch = torch_gpu
    s, n = build_instances("mp8", 0, n_inst=N_LEAN, seed_base=500)
    acts_h = global_actions(0, N_LEAN, 64)
    b = EnvBatch(s, N_LEAN, first=FIRST, n_inst=n, variant=0, rng_seed=RNG)
    assert b.row_build() == dict(early=0, mpc=8, resident=0)
    run = steps(torch, b, torch.from_numpy(acts_h).cuda(), None)
    check_against_oracle(run, replay(s, n, 0, acts_h, None), 0, "n_inst == N")
