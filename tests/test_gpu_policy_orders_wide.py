"""GPU: the segmented policy kernels (fjsp_env_play_policy_orders, fjsp_env_rollout_policy_orders) on order batches of two
and four chunks of 64 operation types, in the workgroup build whose size follows from LDS (8, 4 and 1 environments), on the
three arrival-LP services (host, LDS `device`, `global`).  tests/test_gpu_policy_orders.py runs KC = 1 only, and the
rollout only in the sixteen-env build.

The batches are tests/policy_orders_wide_cases.py's (tests/test_policy_orders_wide_cases_host.py proves on the CPU that the
oracle plays each through its arrivals into its last chunk, and that the table's builds follow from the size rules).
Every comparison is bit for bit: the kernels against the per-step paths they replace (policy_search._play_loop,
MPPPO.per_step_rollout with the native actor: the same device arithmetic one launch at a time), and the played episodes --
their returned actions replayed on the C oracle -- against the oracle's totals and dispatches, which is what fails if the
environment step inside the policy build and inside the loop are wrong together.  A test that runs with kernel_only(True)
fails if play falls back to the loop; policy_orders_build says which build ran."""
import numpy as np
import pytest

from tests import helpers as H
from tests import policy_orders_wide_cases as PW

pytestmark = pytest.mark.gpu

# (case, variant, FJSP_LP_IMPL at create, envs)
PLAYS = [("k65", 0, "host", 12), ("k65", 0, "global", 12), ("k65", 5, "host", 12), ("k65", 0, "host", PW.N_SMALL),
         ("k65flat", 0, "device", 12), ("k128", 0, "global", 12), ("k129", 0, "host", 12), ("k129", 0, "global", 12),
         ("k256", 0, "host", 12), ("k129x2", 0, "host", 6)]
PLAY_IDS = ["%s-v%d-%s-N%d" % p for p in PLAYS]
ORACLE_TOTALS = ("makespan", "delay_time_sum", "completion_time")


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture
def kernel_only(monkeypatch):
    """The kernel path must run: the per-step loop raises if play falls back to it."""
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    loop = PS._play_loop

    def boom(*a, **k):
        raise AssertionError("play fell back to the per-step loop")

    def on(flag):
        monkeypatch.setattr(PS, "_play_loop", boom if flag else loop)
    return on


def _actor(torch, seed):
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.MPPPO import ActorNet
    torch.manual_seed(seed)
    return ActorNet(20, 128, 2, 30).cuda()


_SETS = {}


def _set(name):
    """(InstanceSet, its arrays) of a case; cached."""
    if name not in _SETS:
        s = PW.instance_set(name)
        _SETS[name] = (s, PW.set_arrays(name, s))
    return _SETS[name]


def _maker(name, variant, lp, N, made=None):
    """make() of an EnvBatch of the case on LP route `lp` (None: the library's choice); the batches made go to `made`."""
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    s, _ = _set(name)

    def make():
        with H.env_var("FJSP_LP_IMPL", lp):
            b = EnvBatch(s, N, variant=variant, rng_seed=PW.RNG_SEED)
        if lp is not None:
            assert b.lp_on_device == PW.lp_expected(name, lp), (name, lp, b.lp_on_device)
        if made is not None:
            made.append(b)
        return b
    return make


def _assert_build(b, name):
    sp = PW.SPECS[name]
    build = b.policy_orders_build(20)
    assert (build["kc"], build["envs_per_workgroup"], build["segments"]) == (sp["kc"], sp["envs_per_wg"], len(sp["arrive"])), (name, build)
    assert build["lds_bytes"] == PW.actor_bytes(20) + sp["envs_per_wg"] * (sp["slice"] + 768), (name, build)


_PLAYED = {}


def _played(torch, kernel_only, case):
    """Greedy and sampled play of a case, kernel against loop, recording on (the _rec twins); cached, with the kernel runs'
    host LP counts."""
    if case not in _PLAYED:
        name, variant, lp, N = case
        made = []
        make = _maker(name, variant, lp, N, made)
        actor = _actor(torch, 3)
        greedy = H.kernel_vs_loop(make, actor, kernel_only)
        sampled = H.kernel_vs_loop(make, actor, kernel_only, greedy=False, seed=17)
        _PLAYED[case] = dict(greedy=greedy, sampled=sampled, lp_solves=(made[0].lp_solves, made[2].lp_solves))
    return _PLAYED[case]


@pytest.mark.parametrize("case", PLAYS, ids=PLAY_IDS)
def test_play_equals_the_loop(torch_gpu, kernel_only, case):
    """The table's build and LP service, then greedy and sampled play through the segments against the per-step loop:
    actions, steps, read(), the batch's state / reward / done rows and the recorded schedule; every env plays all its
    operations through every arrival; on the host route the service solved an LP per park."""
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    name, variant, lp, N = case
    sp = PW.SPECS[name]
    s, arrs = _set(name)
    b = _maker(name, variant, lp, N)()
    _assert_build(b, name)
    assert [b.env_seed(e) for e in range(N)] == [PW.env_seed(e) for e in range(N)]
    for route in PW.LP_ROUTES:                    # (k256: beyond the global kernel's 256 rows, the host under every route)
        assert _maker(name, variant, route, N)().lp_on_device == PW.lp_expected(name, route)
    got = _played(torch_gpu, kernel_only, case)
    assert not np.array_equal(got["greedy"]["actions"], got["sampled"]["actions"])
    ops = H.ops(s, 3, N)
    assert ops[0] == sp["steps"]
    for what in ("greedy", "sampled"):
        g = got[what]
        assert np.array_equal(g["steps"], ops), what
        assert np.all(g["read"]["done"] == 1) and np.all(g["read"]["status"] == 0), what
        assert np.array_equal(g["schedule"][1], ops), what
    # the twin that does not record (kernel_vs_loop's batches record): the same greedy episode
    b.reset()
    kernel_only(True)
    res = PS.play(b, _actor(torch_gpu, 3), record_actions=True)
    kernel_only(False)
    H.same(dict(actions=H.host(res["actions"]), steps=H.host(res["steps"]), read=H.read(b)),
           {k: got["greedy"][k] for k in ("actions", "steps", "read")}, "play without recording")
    if lp == "host":
        # at least one LP per env with a later order, at most one per later order
        per = N // 3
        for n in got["lp_solves"]:
            assert per * sum(a.S > 1 for a in arrs) <= n <= per * sum(a.S - 1 for a in arrs), (name, n)


@pytest.mark.parametrize("case", PLAYS, ids=PLAY_IDS)
def test_played_episodes_equal_the_oracle(torch_gpu, kernel_only, case):
    """Every env's returned action rows, replayed on the C oracle with the env's seed: read() is the oracle's makespan,
    total tardiness, completion time, step count and last clock, and the recorded schedule is the oracle's dispatches.
    (The oracle solves its arrival LPs with the product's host solver; the device services equal it bit for bit --
    tests/test_gpu_lp_device.py, tests/test_gpu_lp_global.py -- so the episodes of those routes are pinned as well.)"""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    name, variant, lp, N = case
    _, arrs = _set(name)
    got = _played(torch_gpu, kernel_only, case)
    for what in ("greedy", "sampled"):
        g = got[what]
        table, length = g["schedule"]
        for e in range(N):
            a = arrs[e % 3]
            te = "%s %s env %d" % (PLAY_IDS[PLAYS.index(case)], what, e)
            w = H.play_oracle(a, a.x, g["actions"][:, e], PW.env_seed(e), variant=variant)
            r = g["read"]
            assert w["T"] == r["step_count"][e] == length[e], te
            for key in ORACLE_TOTALS:
                assert r[key][e] == w[key], "%s %s %d, the oracle %d" % (te, key, r[key][e], w[key])
            assert r["step_time"][e] == w["step_time"][-1], te
            rows = sch.from_trace(a, w["k"], w["m"], w["job_n"], w["step_time"])
            assert np.array_equal(table[e, :w["T"]], rows), te + " schedule"
            assert (table[e, w["T"]:] == -1).all(), te + " rows after the episode"


def test_one_env_per_workgroup(torch_gpu, kernel_only):
    """4 kinds x 2 stages x 337 jobs x 3 orders = 4044 jobs: 4096 job words, a slice of 34 624 bytes, and two envs no longer
    fit beside the actor.  Host arrival LPs: play's default keeps the loop there, fused="segments" plays the segments, and
    the first 40 steps -- through an arrival -- are the loop's bit for bit (8088 steps an episode)."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    from deep_reinforcement_learning_for_fjsp_amd._capi import GenOrders, GenParams, GenRanges
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    prm = GenParams(R_min=4, R_max=4, J_min=2, J_max=2, M=0, p_min=5, p_max=30, N_min=337, N_max=337, S=0, DDT=0.0,
                    t_si_min=20.0, t_si_max=40.0)
    s = fi.InstanceSet(1).generate_range(4600, GenOrders(GenRanges(prm, 4, 4, 1.0, 1.0), 3, 3)).solve_fluid()
    assert s.dims(0)["jobs"] == 4044 and PW.envs_per_workgroup(4044, 8) == 1
    actor = _actor(torch, 7)

    def make():
        with H.env_var("FJSP_LP_IMPL", "host"):
            b = EnvBatch(s, 3, rng_seed=5)
        assert b.lp_on_device == 0
        b.record_schedule()
        b.reset()
        return b
    build = make().policy_orders_build(20)
    assert (build["envs_per_workgroup"], build["kc"], build["segments"]) == (1, 1, 3), build
    assert build["lds_bytes"] == PW.actor_bytes(20) + PW.slice_bytes(4044, 8) + 768
    outs = []
    for fused in ("segments", False):
        b = make()
        kernel_only(bool(fused))
        res = PS.play(b, actor, fused=fused, max_steps=40, record_actions=True)
        outs.append(H.play_outcome(b, res))
        if fused:
            assert b.lp_solves > 0, "no order arrived within the steps played"
    kernel_only(False)
    H.same(outs[0], outs[1], "one env per workgroup, segments vs loop")
    assert np.all(outs[0]["steps"] == 40) and np.all(outs[0]["read"]["status"] == 0)


# ---- rollout rows

def _narrow_set():
    """The 204-job KC = 1 shape of test_gpu_policy_orders.py::test_the_narrow_workgroup: eight envs per workgroup."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd._capi import GenOrders, GenParams, GenRanges
    if "narrow" not in _SETS:
        prm = GenParams(R_min=4, R_max=4, J_min=2, J_max=2, M=0, p_min=5, p_max=30, N_min=17, N_max=17, S=0, DDT=0.0,
                        t_si_min=100.0, t_si_max=200.0)
        _SETS["narrow"] = fi.InstanceSet(2).generate_range(4400, GenOrders(GenRanges(prm, 4, 4, 1.0, 1.0), 3, 3)).solve_fluid()
    return _SETS["narrow"]


def _rollout_env(name, lp, variant=0):
    """(mk_env, operations per env): mk_env(route=lp) makes the wrapper on that route and asserts its LP service and build."""
    from deep_reinforcement_learning_for_fjsp_amd.environments import BatchedSODFJSP, BatchedSOFJSSP
    cls = BatchedSODFJSP if variant == 5 else BatchedSOFJSSP
    if name == "narrow":
        s, n_inst, N, want, lp_want = _narrow_set(), 2, 6, (1, 8), {"host": 0, "device": 1}
    else:
        s, n_inst, N = _set(name)[0], 3, PW.SPECS[name]["N"]
        want, lp_want = (PW.SPECS[name]["kc"], PW.SPECS[name]["envs_per_wg"]), {r: PW.lp_expected(name, r) for r in PW.LP_ROUTES}

    def mk_env(route=lp):
        with H.env_var("FJSP_LP_IMPL", route):
            e = cls(s, n_envs=N, rng_seed=9)
        assert e.batch.lp_on_device == lp_want[route], (name, route)
        build = e.batch.policy_orders_build(20)
        assert (build["kc"], build["envs_per_workgroup"]) == want, (name, build)
        return e
    return mk_env, H.ops(s, n_inst, N)


def _learner(torch):
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO import MPPPO as M
    torch.manual_seed(11)
    return M.PPOLearner(20, 30, 128, 2, 2, device=torch.device("cuda", 0), seed=5)


@pytest.mark.parametrize("name,lp,record", [("narrow", "host", False), ("narrow", "device", True), ("k65", "global", True),
                                            ("k129", "global", True), ("k129x2", "host", False)])
def test_rollout_rows_equal_the_per_step_path(torch_gpu, name, lp, record):
    """fjsp_env_rollout_policy_orders in the build of fewer than sixteen envs against per_step_rollout, T = the longest
    episode: valid, flat actions, log-probabilities, states, next states, rewards, dones, actions of every valid row, the
    final state and read().  `record`: both sides record their schedule (the recording twin), compared too -- with
    test_rollout_parks_in_its_last_admitted_step (k65, host, not recording) both twins run at one, two and four chunks."""
    torch = torch_gpu
    mk_env, ops = _rollout_env(name, lp)
    full, _ = H.rollouts(torch, mk_env, _learner(torch), int(ops.max()), record=record)
    assert np.array_equal(full["steps"].cpu().numpy(), ops) and bool((full["done"] == 1).all())
    assert len(set(full["flat"].long().flatten().tolist())) > 15              # the policy did sample around
    if record:
        assert np.array_equal(full["schedule_length"].cpu().numpy(), ops)


def test_rollout_parks_in_its_last_admitted_step(torch_gpu):
    """k65 on the host route: T = the longest episode, then T = p + 1 with p the step of the first arrival under the sampled
    actions: an env parks in the last admitted step, and a later segment of the narrow build still completes its row."""
    torch = torch_gpu
    mk_env, ops = _rollout_env("k65", "host")
    learner = _learner(torch)
    T = int(ops.max())
    full, pairs = H.rollouts(torch, mk_env, learner, T)
    assert np.array_equal(full["steps"].cpu().numpy(), ops) and bool((full["done"] == 1).all())
    assert len(set(full["flat"].long().flatten().tolist())) > 15
    # the first arrival under those actions: replay them step by step on the host route and watch the solve counter
    probe = mk_env("host").batch
    probe.reset()
    p = None
    for t in range(T):
        n0 = probe.lp_solves
        probe.rollout(pairs[t:t + 1].contiguous(), trace=False, rewards=False)
        if probe.lp_solves > n0:
            p = t
            break
    assert p is not None and p + 1 < T
    short, _ = H.rollouts(torch, mk_env, learner, p + 1)
    assert np.array_equal(short["steps"].cpu().numpy(), np.minimum(ops, p + 1))
    assert np.array_equal(short["valid"][p].cpu().numpy() == 1, ops > p) and np.any(ops > p)
    for k in ("valid", "flat", "logp", "states", "nxt", "rewards", "dones", "actions"):
        assert torch.equal(short[k], full[k][:p + 1]), k


# ---- search entry points

def test_best_of_through_a_two_chunk_build(torch_gpu, kernel_only):
    """best_of(k = 3) on k65 with the loop made to raise: the 3 x 12 branch batch starts from the source's rows through the
    state map in segment 0 of the two-chunk narrow build.  It never loses to the greedy play, block 0 is the greedy play,
    and the branch's episodes -- played once more with their actions recorded -- replay to the reported objective."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import lookahead as LA
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    make = _maker("k65", 0, None, 12)
    N, k = 12, 3
    actor = _actor(torch, 6)
    kernel_only(True)
    twin = make()
    twin.reset()
    PS.play(twin, actor)
    greedy = H.read(twin)["makespan"].astype(np.float64)
    b = make()
    _assert_build(b, "k65")
    b.reset()
    start, rows = b.snapshot(), b.state.clone()
    res = PS.best_of(b, actor, k, "makespan", seed=3)
    obj, best = H.host(res["objective"]), H.host(res["best"])
    assert res["branch"].N == k * N
    _assert_build(res["branch"], "k65")
    assert np.all(obj <= greedy) and np.array_equal(obj[best == 0], greedy[best == 0])
    r, rb = H.read(b), H.read(res["branch"])
    assert np.all(r["done"] == 1) and np.all(rb["done"] == 1) and np.all(rb["status"] == 0)
    assert np.array_equal(r["makespan"].astype(np.float64), obj)
    assert np.array_equal(obj, rb["makespan"].reshape(k, N).min(axis=0).astype(np.float64))
    # the same branch episodes once more, actions recorded, then replayed by the plain rollout
    src = torch.as_tensor(np.tile(np.arange(N, dtype=np.int64), k), device="cuda")
    again = LA.make_branch(b, k)
    again.restore(start, src.cpu().numpy(), rows=False)
    acts = PS._play(again, actor, 5, N, 3, None, None, None, src, rows, True, True)["actions"]
    H.same(H.read(again), rb, "branch played again")
    fresh = LA.make_branch(b, k)
    fresh.restore(start, src.cpu().numpy(), rows=False)
    fresh.rollout(acts, trace=False, rewards=False)
    H.same(H.read(fresh), rb, "branch actions replayed")
    kernel_only(False)
