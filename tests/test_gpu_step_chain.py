"""GPU: the small-batch ("early") build of the per-step row kernel (csrc/fjsp_group.hip, gstep_kernel<V, MPC, true>) where
its memory requests were taken off the step's dependent chain:

  * g_open requests every word of the instance and of the environment record straight-line -- a lane without an operation
    type, job or machine reads the LAST entry its row reads anyway and drops the value -- so the first and the last
    instance of a set and the first and the last environment of a batch must stay inside their allocations and mask
    to exactly the values of the predicated loads;
  * the reset observation of a row restarted by autoreset stays in a register of its own until the end of the step;
  * the chosen operation's column (processing times, {arrival, rate}) is requested before Machine.gap_ave's operands are
    laid out and walked, and consumed only where the key is formed.

Instances come from build_instances of tests/test_gpu_row_builds.py ("mp5" / "mp8": K of exactly 1, 2, 15, 16, 17, 31, 32,
33, 47, 48, 49, 63, 64, M = 1..8, the all-eligible instances that make gap_ave rank 7-8 candidates), built with two
instances more than its plan so that the set ENDS with a K = 1 and then a K = 64 instance; a batch plays a window
[first, first + n_inst) of the set.  Actions are batch.global_actions over the variant's whole action space.  Every case
asserts the early build through EnvBatch.row_build, compares every step's (k, m), reward, done and state with the C oracle
(the helpers and tolerances of test_gpu_row_builds.py), checks the chosen (k, m) against the instance's processing times,
and compares bit for bit with the same batch created under FJSP_GROUP_EARLY=0 (the lean build).

Not covered: autoreset mode 2 (a finished row idles silently).  The public per-step entry points pass 0 or 1 to the
kernel; mode 2 is used by fjsp_env_rollout's step-by-step fallback, which row-kernel batches never take.
"""
import numpy as np
import pytest

from tests import helpers as H
from tests import test_gpu_row_builds as RB

pytestmark = pytest.mark.gpu

FIRST, RNG = RB.FIRST, RB.RNG
T_EP = 64                                        # the longest episode (K = 64)


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def plan_len(mp):
    return len(RB.SHAPES) + RB.N_RANDOM[mp] + (len(RB.FULL_ELIG) if mp == "mp8" else 0)


class Sets(object):
    pass


@pytest.fixture(scope="module", params=[(v, mp) for v in (0, 5, 2) for mp in ("mp5", "mp8")], ids=lambda p: "v%d-%s" % p)
def sets(request, torch_gpu):
    """One (variant, instance set): the plan of build_instances and its first two instances once more, so index L is a K = 1
    and index L + 1 (the last instance of the set) a K = 64 instance."""
    c = Sets()
    c.torch = torch_gpu
    c.variant, c.mp = request.param
    c.MPC = 5 if c.mp == "mp5" else 8
    c.L = plan_len(c.mp)
    c.s, n = RB.build_instances(c.mp, c.variant, n_inst=c.L + 2)
    assert n == c.L + 2
    c.K = [c.s.dims(FIRST + i)["K"] for i in range(n)]
    assert c.K[c.L] == 1 and c.K[c.L + 1] == 64 and c.K[2:6] == [1, 64, 2, 2]
    c.tag = "variant %d %s" % (c.variant, c.mp)
    return c


def make_batch(c, N, first, n_inst, early):
    """The batch of N environments on instances [first, first + n_inst) of the set (indices without FIRST), in the early or
    the lean build (asserted)."""
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    with H.env_var("FJSP_GROUP_EARLY", None if early else "0"):
        b = EnvBatch(c.s, N, first=FIRST + first, n_inst=n_inst, variant=c.variant, rng_seed=RNG)
    assert b.kernel_family == 1
    assert b.row_build() == dict(early=1 if early else 0, mpc=c.MPC, resident=0), c.tag
    return b


def mo_tensor(c, N):
    rows = RB.mo_rows(c.variant, N)
    return rows, (None if rows is None else c.torch.tensor(rows, dtype=c.torch.float64).cuda())


def oracle_envs(c, N, first, n_inst, rows):
    """One oracle environment per env of the batch (env e plays instance first + e % n_inst; seeds as EnvBatch)."""
    from deep_reinforcement_learning_for_fjsp_amd.batch import ENV_SEED_STRIDE
    from oracle import pyoracle
    out = []
    for e in range(N):
        a = c.s.arrays(FIRST + first + e % n_inst)
        seed = (RNG + e * ENV_SEED_STRIDE) & (2 ** 64 - 1)
        out.append((a, pyoracle.OracleEnv(a, a.x, c.variant, seed, ddt=getattr(a, "ddt", None) if c.variant == 2 else None)))
    return out


def oracle_step(c, env, action, mo):
    if mo is None:
        return env.step(action)
    return env.step_mo(int(action[0]), (mo[0], mo[1]), mo[2] if mo[2] > 0 else None, mo[3] if mo[3] > 0 else None)


def replay(c, N, first, n_inst, actions_h, rows):
    """H.play_oracle dicts of one episode per env (test_gpu_row_builds.replay for a window of the set)."""
    from deep_reinforcement_learning_for_fjsp_amd.batch import ENV_SEED_STRIDE
    out = []
    for e in range(N):
        a = c.s.arrays(FIRST + first + e % n_inst)
        seed = (RNG + e * ENV_SEED_STRIDE) & (2 ** 64 - 1)
        out.append(H.play_oracle(a, a.x, actions_h[:, e], seed, variant=c.variant, mo=None if rows is None else rows[e]))
    return out


def check_km_against_p(c, trace, first, n_inst, tag):
    """Every chosen (k, m) is an operation type of the env's instance and a machine that can process it."""
    for e in range(trace.shape[1]):
        p = c.s.arrays(FIRST + first + e % n_inst).p
        k, m = trace[:, e, 0].astype(np.int64), trace[:, e, 1].astype(np.int64)
        on = k >= 0
        assert (m[on] >= 0).all() and (k[on] < p.shape[0]).all() and (m[on] < p.shape[1]).all(), "%s env %d" % (tag, e)
        assert (p[k[on], m[on]] > 0).all(), "%s env %d: a column of the wrong operation or machine" % (tag, e)
        assert (m[~on] == -1).all(), "%s env %d" % (tag, e)


def one_episode(c, N, first, n_inst, actions_h, tag):
    """Early build against the oracle and against the lean build, one episode from reset()."""
    torch = c.torch
    rows, mo = mo_tensor(c, N)
    acts = torch.from_numpy(np.ascontiguousarray(actions_h)).cuda()
    early = RB.steps(torch, make_batch(c, N, first, n_inst, True), acts, mo)
    lean = RB.steps(torch, make_batch(c, N, first, n_inst, False), acts, mo)
    assert np.array_equal(H.bits(early["state0"]), H.bits(lean["state0"])), tag
    RB.assert_runs_equal(early, lean, N, tag + " early vs lean")
    check_km_against_p(c, early["trace"], first, n_inst, tag)
    RB.check_against_oracle(early, replay(c, N, first, n_inst, actions_h, rows), c.variant, tag)


# ---------------------------------------------------------------- partial last wave, instance mapping, ends of the allocations
@pytest.mark.parametrize("last_k", [1, 64])
@pytest.mark.parametrize("N,n_inst", [(7, 7), (62, 31)], ids=["7envs-n_inst==N", "62envs-n_inst<N"])
def test_partial_last_wave_at_the_ends_of_both_allocations(sets, N, n_inst, last_k):
    """7 and 62 environments (3 and 2 live rows in the last wave); the last env of the batch plays the last instance of
    the window, which is the K = 1 (the window's largest K decides the clamp of every row) or the K = 64 instance at the end
    of the set; n_inst == N takes g_open's path without the modulo, n_inst < N (62 on 31) the modulo."""
    c = sets
    end = c.L if last_k == 1 else c.L + 1
    first = end - n_inst + 1
    assert (N - 1) % n_inst == n_inst - 1 and c.K[first + (N - 1) % n_inst] == last_k
    acts = RB.global_actions(c.variant, N, T_EP)
    one_episode(c, N, first, n_inst, acts, "%s N=%d last K=%d" % (c.tag, N, last_k))


def test_only_k1_instances(sets):
    """A batch whose largest instance has one operation type: every lane of g_open reads entry 0 of its row."""
    c = sets
    acts = RB.global_actions(c.variant, 7, T_EP)
    one_episode(c, 7, c.L, 1, acts, c.tag + " K=1 only")


# ---------------------------------------------------------------- autoreset
def play_autoreset(c, b, acts, mo, with_state):
    """reset(), then every step of acts with autoreset; with_state[t]: the step returns a state.  Numpy arrays."""
    torch = c.torch
    T, N = acts.shape[0], b.N
    st = torch.zeros(T, N, b.state_size, dtype=torch.float64, device=b.device)
    rw = torch.zeros(T, N, dtype=torch.float64, device=b.device)
    dn = torch.zeros(T, N, dtype=torch.uint8, device=b.device)
    tr = torch.zeros(T, N, 2, dtype=torch.int16, device=b.device)
    b.reset()
    for t in range(T):
        b.step(acts[t], autoreset=True, mo=mo, state=bool(with_state[t]), state_out=st[t], reward_out=rw[t], done_out=dn[t],
               trace_out=tr[t])
    fin = {k: v.cpu().numpy() for k, v in b.read().items()}
    return dict(state=st.cpu().numpy(), reward=rw.cpu().numpy(), done=dn.cpu().numpy(), trace=tr.cpu().numpy(), fin=fin)


def test_autoreset_three_episodes_per_env(sets):
    """Instances 2..8 of the set on 7 environments: the first wave holds K = 1, 64, 2, 2, the second K = 15, 16, 16 and a
    dead row.  192 autoreset steps = at least three episodes of every env: the K = 1 row restarts in every launch, the
    K = 2 rows in every second one (several rows of a wave restart in the same launch), the second wave has launches
    without a restart.  Every step against the oracle (reset and step again on the same oracle env: random.choice's
    stream goes on), the v(t) - v(t-1) entries of the step after each restart included; the same with state-less steps
    interleaved before and after restarts; both bit for bit against the lean build."""
    c, torch = sets, sets.torch
    N, first, n_inst, T = 7, 2, 7, 3 * T_EP
    assert c.K[first:first + 7][:4] == [1, 64, 2, 2]
    actions_h = RB.global_actions(c.variant, N, T)
    acts = torch.from_numpy(actions_h).cuda()
    rows, mo = mo_tensor(c, N)
    always = np.ones(T, bool)
    pattern = np.array([True, False, False, True, True, False, True, False, False, False, True] * (T // 11 + 1))[:T]
    runs = {}
    for name, ws in (("states", always), ("mixed", pattern)):
        early = play_autoreset(c, make_batch(c, N, first, n_inst, True), acts, mo, ws)
        lean = play_autoreset(c, make_batch(c, N, first, n_inst, False), acts, mo, ws)
        tag = "%s autoreset (%s)" % (c.tag, name)
        for key in ("reward", "done", "trace"):
            assert np.array_equal(early[key], lean[key]) if early[key].dtype != np.float64 else \
                np.array_equal(H.bits(early[key]), H.bits(lean[key])), (tag, key)
        assert np.array_equal(H.bits(early["state"][ws]), H.bits(lean["state"][ws])), tag + " states"
        for key in RB.TOTALS + ("done", "status"):
            assert np.array_equal(early["fin"][key], lean["fin"][key]), (tag, key)
        assert (early["fin"]["status"] == 0).all(), tag
        runs[name] = early
    check_km_against_p(c, runs["states"]["trace"], first, n_inst, c.tag + " autoreset")
    assert np.array_equal(runs["mixed"]["trace"], runs["states"]["trace"])
    assert np.array_equal(H.bits(runs["mixed"]["reward"]), H.bits(runs["states"]["reward"]))
    # the oracle, episode after episode
    kw = RB.KW[c.variant]
    for e, (a, env) in enumerate(oracle_envs(c, N, first, n_inst, rows)):
        env.reset()
        episodes, restarted = 0, False
        for t in range(T):
            te = "%s autoreset env %d (K=%d) step %d" % (c.tag, e, a.K, t)
            if env.done:
                env.reset(); restarted = True; episodes += 1
            s, r, d = oracle_step(c, env, actions_h[t, e], None if rows is None else rows[e])
            for name in ("states", "mixed"):
                run = runs[name]
                assert run["trace"][t, e, 0] == env.trace.k_sel and run["trace"][t, e, 1] == env.trace.m_sel, te
                assert H.bits(run["reward"][t, e]) == H.bits(r) and run["done"][t, e] == int(d), te
                if name == "states" or pattern[t]:
                    what = te + " " + name + (": v(t) - v(t-1) of the step after a restart" if restarted else "")
                    H.assert_state_close(run["state"][t, e], s, what, **kw)
            restarted = False
        assert episodes >= 2, "three episodes per env"           # (two restarts = the third episode has begun)


def test_autoreset_0_on_finished_rows(sets):
    """Three steps into the episode the K = 1 and K = 2 rows of the first wave are done and the K = 64 row is not: a step
    without autoreset flags the finished rows FJSP_ST_STEP_AFTER_DONE and leaves them alone (no choice, reward 0, totals
    unchanged) while the other rows step on; bit for bit against the lean build."""
    c, torch = sets, sets.torch
    N, first, n_inst = 7, 2, 7
    actions_h = RB.global_actions(c.variant, N, 5)
    acts = torch.from_numpy(actions_h).cuda()
    _, mo = mo_tensor(c, N)
    out = {}
    for early in (True, False):
        b = make_batch(c, N, first, n_inst, early)
        b.reset()
        for t in range(3):
            b.step(acts[t], mo=mo)
        before = {k: v.cpu().numpy() for k, v in b.read().items()}
        tr = torch.zeros(N, 2, dtype=torch.int16, device=b.device)
        st, rw, dn = [x.clone() for x in b.step(acts[3], mo=mo, trace_out=tr)]
        after = {k: v.cpu().numpy() for k, v in b.read().items()}
        out[early] = (before, after, tr.cpu().numpy(), st.cpu().numpy(), rw.cpu().numpy(), dn.cpu().numpy())
    before, after, tr, st, rw, dn = out[True]
    fin = before["done"] == 1
    assert fin.tolist() == [True, False, True, True, False, False, False], c.tag
    assert (after["status"][fin] == 4).all() and (after["status"][~fin] == 0).all(), c.tag
    assert (tr[fin] == -1).all() and (tr[~fin] >= 0).all() and (rw[fin] == 0.0).all() and (dn[fin] == 1).all(), c.tag
    for key in RB.TOTALS:
        assert np.array_equal(after[key][fin], before[key][fin]), (c.tag, key)
    assert (after["step_count"][~fin] == 4).all(), c.tag
    for x, y in zip(out[True][1:], out[False][1:]):
        if isinstance(x, dict):
            for key in x:
                assert np.array_equal(x[key], y[key]), (c.tag, key)
        else:
            assert np.array_equal(H.bits(x) if x.dtype == np.float64 else x, H.bits(y) if y.dtype == np.float64 else y), c.tag


# ---------------------------------------------------------------- Machine.gap_ave waves
def set_gap_rule(variant, a, envs, on):
    """actions u8[T, N, 2] with the machine rule of `envs` forced to gap_ave (on) or away from it."""
    a = a.copy()
    for e in envs:
        if variant == 2:                 # flat action: machine rule = a % 3, gap_ave = 1
            f = a[:, e, 0].astype(np.int64)
            a[:, e, 0] = (f - f % 3 + 1) if on else np.where(f % 3 == 1, f + 1, f)
        else:                            # machine rule 3 (SO_FJSSP.py:313-317)
            a[:, e, 1] = 3 if on else np.where(a[:, e, 1] == 3, 2, a[:, e, 1])
    return a


@pytest.mark.parametrize("layout", ["A", "B"])
def test_gap_ave_waves(sets, layout):
    """Instances 0..15 on 16 environments (four waves).  Layout A: one row of the first wave (K = 64) plays the gap_ave
    machine rule and its neighbours do not, all four rows of the second wave do, none of the third does.  Layout B: all
    four rows of the first wave do -- one of them on the M = 1 instance, whose candidate list has one member (no walk) --
    one row of the second, none of the third.  The fourth wave: in mp8 the all-eligible instances with the rule at every
    step (7-8 candidates at t > 0), in mp5 whatever global_actions draws."""
    c = sets
    N, first, n_inst = 16, 0, 16
    acts = RB.global_actions(c.variant, N, T_EP)
    one, four = ([1], [4, 5, 6, 7]) if layout == "A" else ([5], [0, 1, 2, 3])
    wave_one = [e for e in range(4 * (one[0] // 4), 4 * (one[0] // 4) + 4) if e not in one]
    acts = set_gap_rule(c.variant, acts, one + four, True)
    acts = set_gap_rule(c.variant, acts, wave_one + [8, 9, 10, 11], False)
    assert c.s.dims(FIRST + 2)["M"] == 1
    if c.mp == "mp8":
        assert [c.s.dims(FIRST + i)["M"] for i in (12, 13, 14, 15)] == [M for _, _, M in RB.FULL_ELIG]
        acts = set_gap_rule(c.variant, acts, [12, 13, 14, 15], True)
    one_episode(c, N, first, n_inst, acts, "%s gap_ave layout %s" % (c.tag, layout))
