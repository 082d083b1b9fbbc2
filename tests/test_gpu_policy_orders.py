"""GPU: the in-launch policy kernels on batches with order arrivals (fjsp_env_play_policy_orders,
fjsp_env_rollout_policy_orders: one policy launch per segment of the episode, the arrival service between the launches)
against the per-step paths they replace -- policy_search._play_loop and MPPPO.per_step_rollout with the native actor.  Every
comparison is bit for bit (H.same / torch.equal): both sides run the same device arithmetic, so no tolerance applies.

Shapes: the generated instances of the `multiorder` suite (gen777: S = 3, 72 operations; gen778: S = 4, 143) and of the
`so_dfjsp` suite (gen6600 / 6601 / 6602: S = 3 / 2 / 1 -- one batch with an env that never parks), eight envs per instance
(24 and 16 envs: a partial workgroup of the sixteen-env build)."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

UNSUPPORTED = -5
SUITES = {"multiorder": (0, 4), "so_dfjsp": (5, 3)}          # suite -> (variant, largest order count of its gen instances)
ROUTES = {"host": 0, "device": 1}                            # FJSP_LP_IMPL -> EnvBatch.lp_on_device


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


def _actor(torch, S, A, seed, hidden=128, layers=2):
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.MPPPO import ActorNet
    torch.manual_seed(seed)
    return ActorNet(S, hidden, layers, A).cuda()


_SETS = {}


def _gen_set(suite, names=None):
    """(fixture arrays, InstanceSet) of the suite's generated instances (or of those named); cached."""
    key = (suite, names)
    if key not in _SETS:
        insts, _, _ = H.load_suite(suite)
        insts = [a for a in insts if (a.name in names if names else a.name.startswith("gen"))]
        assert insts
        _SETS[key] = (insts, H.instance_set_from(insts))
    return _SETS[key]


def _maker(suite, lp, per_inst=8, rng_seed=21, names=None):
    """make() of an EnvBatch of per_inst envs per instance, created on LP route `lp` (None: the library's choice)."""
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    insts, s = _gen_set(suite, names)

    def make():
        with H.env_var("FJSP_LP_IMPL", lp):
            b = EnvBatch(s, per_inst * len(insts), variant=SUITES[suite][0], rng_seed=rng_seed)
        if lp is not None:
            assert b.lp_on_device == ROUTES[lp]
        return b
    return make, insts, s


def _replays(make, got, what):
    """The returned actions, replayed by the plain fused rollout from reset, end where the play ended."""
    fresh = make()
    fresh.reset()
    fresh.rollout(got["actions"], trace=False, rewards=False)
    H.same(H.read(fresh), got["read"], what)


@pytest.mark.parametrize("lp", sorted(ROUTES))
@pytest.mark.parametrize("suite", sorted(SUITES))
def test_play_equals_the_loop(torch_gpu, kernel_only, suite, lp):
    """Greedy and sampled play through the segments against the per-step loop, recording on: actions, steps, read(), the
    batch's state / reward / done rows and the schedule; every env plays all its operations through every arrival."""
    make, insts, s = _maker(suite, lp)
    actor = _actor(torch_gpu, 20, 30, 3)
    N = 8 * len(insts)
    greedy = H.kernel_vs_loop(make, actor, kernel_only)
    sampled = H.kernel_vs_loop(make, actor, kernel_only, greedy=False, seed=17)
    assert not np.array_equal(greedy["actions"], sampled["actions"])
    for got, what in ((greedy, "greedy"), (sampled, "sampled")):
        assert np.array_equal(got["steps"], H.ops(s, len(insts), N)), what
        _replays(make, got, "%s %s %s replay" % (suite, lp, what))


@pytest.mark.parametrize("suite", sorted(SUITES))
def test_segments(torch_gpu, kernel_only, suite):
    """policy_orders_build reports one segment per order of the batch's largest instance; the envs of that instance finish
    (kernel_vs_loop asserts done), so every one of its S - 1 parks was served."""
    make, insts, s = _maker(suite, None)
    b = make()
    build = b.policy_orders_build(20)
    assert build["segments"] == SUITES[suite][1] == max(a.S for a in insts)
    assert build["envs_per_workgroup"] == 16 and build["kc"] == 1
    with H.env_var("FJSP_LP_IMPL", "host"):
        bh = make()
    bh.reset()
    kernel_only(True)
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    PS.play(bh, _actor(torch_gpu, 20, 30, 3))
    kernel_only(False)
    r = H.read(bh)
    assert np.all(r["done"] == 1) and np.all(r["status"] == 0)
    assert np.array_equal(r["step_count"], H.ops(s, len(insts), bh.N))
    # (the host service solved an LP per park: at least one per env with a later order, at most one per later order)
    assert 8 * sum(a.S > 1 for a in insts) <= bh.lp_solves <= 8 * sum(a.S - 1 for a in insts)


def _first_arrival(torch, make, actor):
    """(p, actions u8[p, N, 2]): the step of a host-route batch's first order arrival -- the host service's solve counter
    rises in it -- under the greedy actor (actor given) or the rule pair (0, 0) at every step, and the steps before it."""
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    with H.env_var("FJSP_LP_IMPL", "host"):
        b = make()
    assert b.lp_on_device == 0
    b.reset()
    pre = []
    for p in range(200):
        n0 = b.lp_solves
        if actor is None:
            a = torch.zeros(1, b.N, 2, dtype=torch.uint8, device="cuda")
            b.rollout(a, trace=False, rewards=False)
        else:
            a = PS.play(b, actor, fused=False, max_steps=1, record_actions=True)["actions"]
        if b.lp_solves > n0:
            return p, (torch.cat(pre) if pre else None)
        pre.append(a.clone())
    raise AssertionError("no order arrived")


def _advanced(make, pre):
    b = make()
    b.record_schedule()
    b.reset()
    if pre is not None:
        b.rollout(pre, trace=False, rewards=False)
    return b


@pytest.mark.parametrize("forced", [False, True])
def test_park_in_step_0_of_the_call(torch_gpu, kernel_only, forced):
    """A call whose very first step meets an arrival: two identical batches are advanced to the step before an env's first
    arrival, then played both ways, with the actor's own step 0 and with a forced one (`first`, the rule pair the
    discovery run applied).  Segment 0 then leaves such an env with steps_out = 1 and nothing but its action row."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    actor = _actor(torch, 20, 30, 4)
    make_any, insts, s = _maker("multiorder", None, per_inst=4, names=("gen777",))
    p, pre = _first_arrival(torch, make_any, None if forced else actor)
    assert 0 < p < 72
    kw = dict(first=torch.zeros(4, 2, dtype=torch.uint8, device="cuda")) if forced else {}
    for lp in sorted(ROUTES):
        make, _, _ = _maker("multiorder", lp, per_inst=4, names=("gen777",))
        outs = []
        for fused in (True, False):
            b = _advanced(make, pre)
            kernel_only(fused)
            res = PS.play(b, actor, fused=fused, record_actions=True, **kw)
            kernel_only(False)
            outs.append(H.play_outcome(b, res))
        H.same(outs[0], outs[1], "park in step 0, %s, forced %r" % (lp, forced))
        got = outs[0]
        assert np.all(got["read"]["done"] == 1) and np.all(got["read"]["status"] == 0)
        assert np.array_equal(got["steps"], got["read"]["step_count"] - p) and np.all(got["steps"] == 72 - p)
        if forced:
            assert np.all(got["actions"][0] == 0)
    make, _, _ = _maker("multiorder", "host", per_inst=4, names=("gen777",))
    b = _advanced(make, pre)
    n0 = b.lp_solves
    kernel_only(True)
    res = PS.play(b, actor, max_steps=1, **kw)
    kernel_only(False)
    assert b.lp_solves > n0, "no env parked in step 0 of the call"
    assert np.all(H.host(res["steps"]) == 1) and np.all(H.read(b)["step_count"] == p + 1)


@pytest.mark.parametrize("lp", sorted(ROUTES))
@pytest.mark.parametrize("suite", sorted(SUITES))
def test_rollout_rows_equal_the_per_step_path(torch_gpu, suite, lp):
    """fjsp_env_rollout_policy_orders against per_step_rollout: states, actions, rewards, next states, dones, valid, flat
    actions, log-probabilities of every valid row and the last state.  T = the longest episode, and T = p + 1 with p the
    step of the first arrival under the sampled actions: an env parks in the last admitted step, and the next segment
    still completes its row."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO import MPPPO as M
    from deep_reinforcement_learning_for_fjsp_amd.environments import BatchedSODFJSP, BatchedSOFJSSP
    insts, s = _gen_set(suite)
    cls = BatchedSODFJSP if suite == "so_dfjsp" else BatchedSOFJSSP

    def mk_env(route=lp):
        with H.env_var("FJSP_LP_IMPL", route):
            e = cls(s, n_envs=8 * len(insts), rng_seed=9)
        assert e.batch.lp_on_device == ROUTES[route]
        return e
    torch.manual_seed(11)
    learner = M.PPOLearner(20, 30, 128, 2, 2, device=torch.device("cuda", 0), seed=5)
    ops = H.ops(s, len(insts), 8 * len(insts))
    T = int(ops.max())
    full, pairs = H.rollouts(torch, mk_env, learner, T)
    assert np.array_equal(full["steps"].cpu().numpy(), ops) and bool((full["done"] == 1).all())
    assert len(set(full["flat"].long().flatten().tolist())) > 15              # the policy did sample around
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


def test_the_narrow_workgroup(torch_gpu, kernel_only):
    """A multi-order batch whose envs do not fit sixteen to a workgroup.  The suites' two large multi-order shops (111 and
    134 jobs: 128 and 192 job words, slices of 2880 and 3392 bytes) still fit sixteen beside a 20-input actor
    (16 x (slice + 768) <= 163840 - 93440), so the batch is generated: 4 kinds x 17 jobs x 3 orders = 204 jobs, 256 job
    words, a slice of 3904 bytes -- eight envs per workgroup, the 512-thread build."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd._capi import GenOrders, GenParams, GenRanges
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    prm = GenParams(R_min=4, R_max=4, J_min=2, J_max=2, M=0, p_min=5, p_max=30, N_min=17, N_max=17, S=0, DDT=0.0,
                    t_si_min=100.0, t_si_max=200.0)
    s = fi.InstanceSet(2).generate_range(4400, GenOrders(GenRanges(prm, 4, 4, 1.0, 1.0), 3, 3)).solve_fluid()
    make = lambda: EnvBatch(s, 6, rng_seed=3)
    build = make().policy_orders_build(20)
    assert build["envs_per_workgroup"] == 8 and build["kc"] == 1 and build["segments"] == 3
    got = H.kernel_vs_loop(make, _actor(torch_gpu, 20, 30, 6), kernel_only)
    assert np.array_equal(got["steps"], H.ops(s, 2, 6)) and np.all(got["steps"] == 4 * 2 * 17 * 3)


def test_play_keeps_the_loop_where_the_segments_measured_no_gain(torch_gpu, kernel_only):
    """Host arrival LPs and fewer than four envs per workgroup (4 kinds x 120 jobs x 4 orders = 1920 jobs: a slice of
    17 KB, two envs beside the actor): play's default is the per-step loop there, fused="segments" plays the segments, and
    the first steps through an arrival are the loop's bit for bit (3840 steps an episode: the test plays 40)."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    from deep_reinforcement_learning_for_fjsp_amd._capi import GenOrders, GenParams, GenRanges
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    prm = GenParams(R_min=4, R_max=4, J_min=2, J_max=2, M=0, p_min=5, p_max=30, N_min=120, N_max=120, S=0, DDT=0.0,
                    t_si_min=20.0, t_si_max=40.0)
    s = fi.InstanceSet(1).generate_range(4500, GenOrders(GenRanges(prm, 4, 4, 1.0, 1.0), 4, 4)).solve_fluid()
    actor = _actor(torch, 20, 30, 7)

    def make(lp):
        with H.env_var("FJSP_LP_IMPL", lp):
            b = EnvBatch(s, 3, rng_seed=5)
        assert b.lp_on_device == ROUTES[lp]
        b.record_schedule()
        b.reset()
        return b
    b = make("host")
    assert b.policy_orders_build(20)["envs_per_workgroup"] == 2
    kernel_only(True)
    with pytest.raises(AssertionError, match="fell back to the per-step loop"):
        PS.play(b, actor, max_steps=1)
    d = make("device")                                       # (on the device route the segments stay the default)
    PS.play(d, actor, max_steps=40)
    assert np.all(H.read(d)["step_count"] == 40)
    outs = []
    for fused in ("segments", False):
        b = make("host")
        kernel_only(bool(fused))
        res = PS.play(b, actor, fused=fused, max_steps=40, record_actions=True)
        outs.append(H.play_outcome(b, res))
        if fused:
            assert b.lp_solves > 0, "no order arrived within the steps played"
    kernel_only(False)
    H.same(outs[0], outs[1], "two envs per workgroup, segments vs loop")
    assert np.all(outs[0]["steps"] == 40) and np.all(outs[0]["read"]["status"] == 0)


def test_refusals(torch_gpu):
    """The segmented entries answer FJSP_E_UNSUPPORTED, saying why, for a batch without order arrivals, a MO_DFJSP batch and
    an actor of another shape; play still decodes each of them."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    from deep_reinforcement_learning_for_fjsp_amd._capi import ActorParams
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.Buffer import RolloutBuffer
    from deep_reinforcement_learning_for_fjsp_amd.agents.native_actor import native_actor_params
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, VARIANT_MO_DFJSP
    lib, p = _capi.lib(), _capi.ptr

    def both(b, ap, div, mo, text):
        N, S, T = b.N, b.state_size, 10
        steps = torch.zeros(N, dtype=torch.int32, device="cuda")
        assert lib.fjsp_env_play_policy_orders(b._h, C.byref(ap), div, N, None, T, p(mo), b._p_state, N, None, None, None, p(steps),
                                               b._p_state, b._p_reward, b._p_done, b._stream()) == UNSUPPORTED
        assert text in lib.fjsp_last_error(), lib.fjsp_last_error()
        memory = RolloutBuffer(T, N, S, device=0)
        eps = torch.zeros(1, dtype=torch.float32, device="cuda")
        seed = torch.tensor([7], dtype=torch.int64, device="cuda")
        flat, logp = torch.zeros(T, N, device="cuda"), torch.zeros(T, N, device="cuda")
        st0 = b.state.clone()
        assert lib.fjsp_env_rollout_policy_orders(b._h, memory._h, C.byref(ap), p(eps), p(seed), div, T, p(mo), p(st0), p(flat),
                                                  p(logp), b._p_state, b._stream()) == UNSUPPORTED
        assert text in lib.fjsp_last_error(), lib.fjsp_last_error()

    narrow = _actor(torch, 20, 30, 8)
    # a single-order batch: the one-launch entries play it
    s1 = H.gen_10x5(4, 360)
    b = EnvBatch(s1, 8, rng_seed=11)
    b.reset()
    both(b, native_actor_params(narrow), 5, None, b"no order arrivals")
    with pytest.raises(_capi.FjspError) as err:
        b.policy_orders_build(20)
    assert err.value.code == UNSUPPORTED and "no order arrivals" in str(err.value)
    res = PS.play(b, narrow)
    assert np.all(H.read(b)["done"] == 1) and np.array_equal(H.host(res["steps"]), H.ops(s1, 4, 8))
    # a 200 x 5 actor on a batch with order arrivals
    make, insts, s = _maker("multiorder", None, per_inst=2)
    b = make()
    b.reset()
    wide = _actor(torch, 20, 30, 8, hidden=200, layers=5)
    assert native_actor_params(wide) is None
    lin = [m for m in wide.modules() if isinstance(m, torch.nn.Linear)]
    ap = ActorParams(p(lin[0].weight), p(lin[0].bias), p(lin[1].weight), p(lin[1].bias), p(lin[-1].weight), p(lin[-1].bias), 20, 200, 30)
    both(b, ap, 5, None, b"in-kernel actor")
    res = PS.play(b, wide)
    assert np.all(H.read(b)["done"] == 1) and np.array_equal(H.host(res["steps"]), H.ops(s, len(insts), b.N))
    # a MO_DFJSP batch, order arrivals and all
    dinsts, _, _ = H.load_suite("mo_dfjsp")
    dinsts = [a for a in dinsts if a.name.startswith("gen")]
    assert any(a.S > 1 for a in dinsts)
    ds = H.instance_set_from(dinsts)
    N = 2 * len(dinsts)
    mo = torch.zeros(N, 4, dtype=torch.float64, device="cuda"); mo[:, 0] = 1.0
    d = EnvBatch(ds, N, variant=VARIANT_MO_DFJSP, rng_seed=12)
    d.reset()
    both(d, native_actor_params(_actor(torch, 30, 30, 9)), 10, mo, b"MO_DFJSP")
    with pytest.raises(_capi.FjspError) as err:
        d.policy_orders_build(30)
    assert err.value.code == UNSUPPORTED and "MO_DFJSP" in str(err.value)
    PS.play(d, _actor(torch, 30, 120, 10, hidden=200, layers=5), mo=mo)
    assert np.all(H.read(d)["done"] == 1)


def test_best_of_through_the_segments(torch_gpu, kernel_only):
    """best_of on a multi-order batch with the loop made to raise: the k x N branch batch of lookahead.make_branch starts
    from the source's rows through the state map in segment 0.  It never loses to the greedy play, block 0 is the greedy
    play, and the branch's episodes -- played once more with their actions recorded -- replay to the reported objective."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import lookahead as LA
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    make, insts, s = _maker("multiorder", None, per_inst=4)
    N, k = 4 * len(insts), 4
    actor = _actor(torch, 20, 30, 6)
    kernel_only(True)
    twin = make()
    twin.reset()
    PS.play(twin, actor)
    greedy = H.read(twin)["makespan"].astype(np.float64)
    b = make()
    b.reset()
    start, rows = b.snapshot(), b.state.clone()
    res = PS.best_of(b, actor, k, "makespan", seed=3)
    obj, best = H.host(res["objective"]), H.host(res["best"])
    assert res["branch"].N == k * N
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


def test_ppo_round_through_the_segments(torch_gpu, monkeypatch):
    """One PPO(fused_rollout=True) round on a generated 64-env SO_DFJSP handle with 1..3 orders per instance, the per-step
    rollout bodies made to raise: the rollout ran through fjsp_env_rollout_policy_orders."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd._capi import GenOrders, GenParams, GenRanges
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO import MPPPO as M
    from deep_reinforcement_learning_for_fjsp_amd.environments import BatchedSODFJSP
    prm = GenParams(R_min=3, R_max=3, J_min=2, J_max=3, M=0, p_min=5, p_max=30, N_min=2, N_max=3, S=0, DDT=0.0,
                    t_si_min=100.0, t_si_max=200.0)
    env = BatchedSODFJSP(GenOrders(GenRanges(prm, 3, 6, 0.5, 1.5), 1, 3), n_envs=64, seed_base=900, rng_seed=3)
    assert env.batch.policy_orders_build(20)["segments"] == 3

    def boom(*a, **k):
        raise AssertionError("the rollout fell back to the per-step loop")
    monkeypatch.setattr(M, "_rollout_steps", boom)
    monkeypatch.setattr(M.RolloutCollector, "_capture", boom)
    torch.manual_seed(0)
    agent = M.PPO(env, hidden_size=128, hidden_layer=2, seed=1, max_steps=81, fused_rollout=True)      # 81 = 3 x 3 x 3 x 3 operations at most
    before = [q.detach().clone() for q in agent.learner.actor_new.parameters()]
    tard, mk, (c_loss, a_loss) = agent.run_one_policy_network()
    assert np.isfinite(tard) and np.isfinite(mk) and np.isfinite(c_loss) and np.isfinite(a_loss)
    r = env.read()
    assert bool((r["done"] == 1).all()) and int(((r["status"] & ~4) != 0).sum()) == 0
    valid = agent.memory.valid[:len(agent.memory)]
    assert torch.equal(valid.sum(0).long(), r["step_count"].long())
    tot = (agent.memory.rewards[:len(agent.memory)].double() * valid.double()).sum(0)
    assert torch.equal(-tot.long(), r["delay_time_sum"])
    assert any(not torch.equal(x, y) for x, y in zip(before, agent.learner.actor_new.parameters()))
