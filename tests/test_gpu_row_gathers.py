"""The row kernels (csrc/fjsp_group.hip) on the smallest shapes at which what a row keeps per LANE and what it keeps per ROW
can come apart: the padding job lane (15 jobs), one slot in use and three padded (K = 15), the fourth slot on (K = 49..64),
a K = 17 row next to a K = 64 row in one wave (the slot count is wave-wide, the padding per row), M = 8 and M = 2, and a
batch of 5 (a wave with one live row).  The early build's prologue hands every lane of a row the row's eight scalar words
(EnvScalars 0..7) by loads from the row's one address and keeps obs_prev per lane; rows restarted by autoreset, rows of a
partly filled wave and state-less steps (g_obs_refresh, the second copy of the observation) all pass through it.

Generated single-job instances, at most 16 environments a batch, random rule pairs over all 6 x 5 (18 flat actions for
MO_FJSSP_discretes), autoreset on, played until every environment is at least in its third episode.  Every step against the C
oracle (oracle/pyoracle, reset and stepped again on the same oracle env: random.choice's stream goes on): (k, m), reward and
done bit for bit, the state exactly but for the three std entries (H.assert_state_close: H.POW_RTOL) -- on the early build,
on the lean build (FJSP_GROUP_EARLY=0 at create) and, for the first episode, through rollout (the fused kernel); each shape
once more with state-less steps interleaved.

The CPU test pins, on the oracle alone, the fact that lets a row kernel read "this operation type is unassigned" from its own
state: with one job per kind, "the job's stage <= the type's stage" is "the type has not been dispatched" at every step."""
import numpy as np
import pytest

from tests import helpers as H

FIRST = 2                       # the instances sit at an offset inside the set
RNG = 911
N_ACT = {0: (6, 5), 2: (18, 1)}
KW = {0: {}, 2: dict(mo=True)}
PATTERN = [True, False, False, True, True, False, True, False, False, False, True]      # which steps hand a state back ("mixed")

# name -> [(kinds R, stages J or (J_min, J_max), machines M)] per instance, environments N (env e plays instance e % n_inst)
SHAPES = {
    "jobs15": ([(15, (2, 4), 5), (15, 1, 3), (15, 4, 4), (14, (1, 4), 5)], 8),       # lane 15 is the one padding job lane
    "k15": ([(3, 5, 3), (3, 5, 5), (5, 3, 4), (15, 1, 2)], 8),                      # K = 15: slot 0 in use, three padded
    "k49_64": ([(7, 7, 5), (10, (5, 6), 5), (8, 8, 4), (12, (4, 5), 5), (15, 4, 6), (9, 7, 3)], 12),     # slot 3 on
    "k17_k64": ([(1, 17, 3), (8, 8, 5)], 2),                                        # nslots is the wave's, the padding the row's
    "m8": ([(10, (3, 5), 8), (6, 4, 8), (1, 9, 8), (12, 5, 8)], 8),
    "m2": ([(10, (3, 5), 2), (4, 4, 2), (15, 2, 2), (2, 1, 2)], 8),
    "batch5": ([(10, (3, 5), 5), (5, 5, 5), (1, 1, 1), (12, 4, 4), (9, (3, 5), 5)], 5),   # the second wave has one live row
}


def build_set(name, variant):
    """The instances of a shape, generated and solved; returns (set, n_inst, N)."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    plan, N = SHAPES[name]
    rs = np.random.RandomState(sorted(SHAPES).index(name) + 100 * variant)
    s = fi.InstanceSet(FIRST + len(plan))
    for i, (R, J, M) in enumerate(plan):
        jlo, jhi = (J, J) if isinstance(J, int) else J
        pmin, pmax = (2000, 65535) if i % 4 == 3 else (1, int(rs.randint(2, 40)))      # (every fourth: clocks beyond 2^16)
        prm = fi.GenParams(R_min=R, R_max=R, J_min=jlo, J_max=jhi, M=M, p_min=pmin, p_max=pmax, N_min=1, N_max=1, S=1,
                           DDT=float(rs.choice([0.5, 1.0, 1.5])), t_si_min=20.0, t_si_max=80.0)
        s.generate(FIRST + i, 7000 + 97 * sorted(SHAPES).index(name) + i + 1000 * variant, prm)
    s.solve_fluid(FIRST, len(plan))
    return s, len(plan), N


def episode_len(s, n_inst):
    return max(int(s.dims(FIRST + i)["K"]) for i in range(n_inst))


def actions_for(variant, N, T):
    from deep_reinforcement_learning_for_fjsp_amd.batch import global_actions
    n0, n1 = N_ACT[variant]
    return global_actions(60 + variant, 0, N, T, n0, n1)


def mo_rows(variant, N):
    if variant != 2:
        return None
    rs = np.random.RandomState(31)
    kinds, w0 = rs.randint(0, 3, N), np.round(rs.rand(N), 2)
    return [(1.0, 0.0, -1.0, -1.0) if k == 0 else (0.0, 1.0, -1.0, -1.0) if k == 1 else
            (float(w0[e]), float(1.0 - w0[e]), float(rs.randint(20, 90)), float(rs.randint(30, 400))) for e, k in enumerate(kinds)]


def oracle_envs(s, n_inst, N, variant):
    from deep_reinforcement_learning_for_fjsp_amd.batch import ENV_SEED_STRIDE
    from oracle import pyoracle
    out = []
    for e in range(N):
        a = s.arrays(FIRST + e % n_inst)
        seed = (RNG + e * ENV_SEED_STRIDE) & (2 ** 64 - 1)
        out.append((a, pyoracle.OracleEnv(a, a.x, variant, seed, ddt=getattr(a, "ddt", None) if variant == 2 else None)))
    return out


def oracle_step(env, action, mo):
    if mo is None:
        return env.step(action)
    return env.step_mo(int(action[0]), (mo[0], mo[1]), mo[2] if mo[2] > 0 else None, mo[3] if mo[3] > 0 else None)


def oracle_autoreset(s, n_inst, N, variant, actions_h, rows):
    """Every env on the oracle, episode after episode: per env the list over t of (k, m, reward, done, state) and the number of
    restarts.  Computed once per (shape, variant) and shared by the build variants."""
    out = []
    for e, (a, env) in enumerate(oracle_envs(s, n_inst, N, variant)):
        env.reset()
        rec, restarts = [], 0
        for t in range(actions_h.shape[0]):
            if env.done:
                env.reset(); restarts += 1
            st, r, d = oracle_step(env, actions_h[t, e], None if rows is None else rows[e])
            rec.append((env.trace.k_sel, env.trace.m_sel, r, int(d), np.array(st, np.float64)))
        out.append((rec, restarts))
    return out


# ------------------------------------------------------------------ CPU: the identity, on the oracle alone
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_unassigned_is_job_stage_le_type_stage_on_the_oracle(built, name):
    """One job per kind, one order: operation type k = first(kind) + stage.  Over two episodes of every env of the shape, with
    random rule pairs: before and after every dispatch, for EVERY operation type, "the stage of the type's job <= the type's
    stage" equals "the type has not been dispatched"; a reset puts both back together."""
    s, n_inst, N = build_set(name, 0)
    T = 2 * episode_len(s, n_inst)
    actions_h = actions_for(0, N, T)
    for e, (a, env) in enumerate(oracle_envs(s, n_inst, N, 0)):
        Jr = np.asarray(a.Jr, np.int64)
        first = np.concatenate([[0], np.cumsum(Jr)[:-1]])
        kind_of = np.repeat(np.arange(len(Jr)), Jr)
        stage_of = np.arange(int(Jr.sum())) - first[kind_of]
        env.reset()
        job_stage = np.zeros(len(Jr), np.int64)
        dispatched = np.zeros(int(Jr.sum()), bool)
        for t in range(T):
            if env.done:
                env.reset()
                job_stage[:] = 0; dispatched[:] = False
            assert np.array_equal(job_stage[kind_of] <= stage_of, ~dispatched), "%s env %d step %d" % (name, e, t)
            env.step(actions_h[t, e])
            k, r = env.trace.k_sel, env.trace.job_kind
            assert kind_of[k] == r and stage_of[k] == job_stage[r] and not dispatched[k], "%s env %d step %d: stage order" % (name, e, t)
            dispatched[k] = True
            job_stage[r] += 1
            assert np.array_equal(job_stage[kind_of] <= stage_of, ~dispatched), "%s env %d step %d" % (name, e, t)
            assert bool(env.done) == bool(dispatched.all())


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


class Case(object):
    pass


_CASES = {}


def case_for(name, variant):
    """Instances, actions and the oracle's record of a (shape, variant): built once, read-only afterwards."""
    if (name, variant) not in _CASES:
        c = Case()
        c.name, c.variant = name, variant
        c.s, c.n_inst, c.N = build_set(name, variant)
        c.T_ep = episode_len(c.s, c.n_inst)
        c.T = 2 * c.T_ep + 2                       # the longest env finishes two episodes and restarts once more
        c.actions_h = actions_for(variant, c.N, c.T)
        c.rows = mo_rows(variant, c.N)
        c.want = oracle_autoreset(c.s, c.n_inst, c.N, variant, c.actions_h, c.rows)
        assert all(restarts >= 2 for _, restarts in c.want), name
        _CASES[(name, variant)] = c
    return _CASES[(name, variant)]


def make_batch(c, early):
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    with H.env_var("FJSP_GROUP_EARLY", None if early else "0"):
        b = EnvBatch(c.s, c.N, first=FIRST, n_inst=c.n_inst, variant=c.variant, rng_seed=RNG)
    assert b.kernel_family == 1 and b.row_build()["early"] == (1 if early else 0), c.name
    return b


def play_autoreset(torch, c, b, with_state):
    acts = torch.from_numpy(np.ascontiguousarray(c.actions_h)).cuda()
    mo = None if c.rows is None else torch.tensor(c.rows, dtype=torch.float64).cuda()
    T, N = c.T, c.N
    st = torch.zeros(T, N, b.state_size, dtype=torch.float64, device=b.device)
    rw = torch.zeros(T, N, dtype=torch.float64, device=b.device)
    dn = torch.zeros(T, N, dtype=torch.uint8, device=b.device)
    tr = torch.zeros(T, N, 2, dtype=torch.int16, device=b.device)
    b.reset()
    for t in range(T):
        b.step(acts[t], autoreset=True, mo=mo, state=bool(with_state[t]), state_out=st[t], reward_out=rw[t], done_out=dn[t],
               trace_out=tr[t])
    assert int((b.read()["status"] != 0).sum()) == 0, c.name
    return st.cpu().numpy(), rw.cpu().numpy(), dn.cpu().numpy(), tr.cpu().numpy()


def check_steps(c, run, with_state, tag):
    st, rw, dn, tr = run
    for e, (rec, _) in enumerate(c.want):
        for t, (k, m, r, d, s) in enumerate(rec):
            te = "%s %s env %d step %d" % (c.name, tag, e, t)
            assert tr[t, e, 0] == k and tr[t, e, 1] == m, te + " (k, m)"
            assert H.bits(rw[t, e]) == H.bits(r), te + " reward"
            assert dn[t, e] == d, te + " done"
            if with_state[t]:
                H.assert_state_close(st[t, e], s, te, **KW[c.variant])


def run_case(torch, name, variant, build, mixed):
    c = case_for(name, variant)
    if build == "fused":
        # the fused kernel plays one episode from reset (no autoreset inside a launch): the oracle's first episode
        from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
        b = EnvBatch(c.s, c.N, first=FIRST, n_inst=c.n_inst, variant=c.variant, rng_seed=RNG)
        assert b.kernel_family == 1
        b.reset()
        acts = torch.from_numpy(np.ascontiguousarray(c.actions_h[:c.T_ep])).cuda()
        mo = None if c.rows is None else torch.tensor(c.rows, dtype=torch.float64).cuda()
        tr, rw, st_last = b.rollout(acts, mo=mo, state=not mixed)
        tr, rw = tr.cpu().numpy(), rw.cpu().numpy()
        assert (st_last is None) == mixed
        for e, (rec, _) in enumerate(c.want):
            Te = [d for (_, _, _, d, _) in rec].index(1) + 1
            for t in range(c.T_ep):
                te = "%s fused env %d step %d" % (c.name, e, t)
                k, m, r = (rec[t][0], rec[t][1], rec[t][2]) if t < Te else (-1, -1, 0.0)
                assert tr[t, e, 0] == k and tr[t, e, 1] == m and H.bits(rw[t, e]) == H.bits(r), te
            if st_last is not None:
                H.assert_state_close(st_last[e].cpu().numpy(), rec[Te - 1][4], "%s fused env %d last state" % (c.name, e), **KW[c.variant])
        return
    with_state = np.array((PATTERN * (c.T // len(PATTERN) + 1))[:c.T]) if mixed else np.ones(c.T, bool)
    run = play_autoreset(torch, c, make_batch(c, build == "early"), with_state)
    check_steps(c, run, with_state, build + (" mixed" if mixed else ""))


@pytest.mark.gpu
@pytest.mark.parametrize("mixed", [False, True], ids=["states", "mixed"])
@pytest.mark.parametrize("build", ["early", "lean", "fused"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_row_kernels_against_the_oracle(torch_gpu, name, build, mixed):
    """SO_FJSSP.  `mixed`: steps that return no state interleaved (PATTERN), which puts g_obs_refresh on the path; for the
    fused kernel: the rollout without a final state (no observation inside the kernel)."""
    run_case(torch_gpu, name, 0, build, mixed)


@pytest.mark.gpu
@pytest.mark.parametrize("build", ["early", "lean", "fused"])
def test_mo_discretes_15_jobs(torch_gpu, build):
    """MO_FJSSP_discretes (flat actions, weighted rewards, 25-entry state) on the 15-job shape."""
    run_case(torch_gpu, "jobs15", 2, build, False)
