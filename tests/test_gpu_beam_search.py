"""GPU: policy_search.beam_search against what it must reduce to (greedy play and policy_lookahead at width 1) and, at
larger widths, against a host-driven loop over the calls that existed before it (actor forward, torch.log, snapshot /
restore / rollout, play for the expansion) with the numpy selection of tests/beam_reference.py."""
import numpy as np
import pytest

from tests import beam_reference as R
from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _actor(torch, S, A, seed):
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.MPPPO import ActorNet
    torch.manual_seed(seed)
    return ActorNet(S, 128, 2, A).cuda()


def _reference_search(torch, src, actor, W, score, objective, flat_candidates, pair_div, A, mo=None):
    """The beam search of `src` (left untouched) driven from the host: dict(cost, best, actions, objective).  objective:
    the read() entry to minimise ("makespan", "delay_time_sum") or None."""
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    from deep_reinforcement_learning_for_fjsp_amd.agents.native_actor import native_actor_forward
    from deep_reinforcement_learning_for_fjsp_amd.lookahead import make_branch
    N, P, cols = src.N, len(flat_candidates), np.arange(src.N)
    flat_candidates = np.asarray(flat_candidates)
    pair = (lambda a: np.stack([a // pair_div, a % pair_div], -1)) if pair_div else (lambda a: np.stack([a, np.zeros_like(a)], -1))
    beams = make_branch(src, W)
    beams.restore(src.snapshot(), np.tile(cols, W), rows=True)
    mo_beams = None if mo is None else mo.repeat(W, 1)
    if score == "rollout":
        expand = make_branch(src, W * P)
        emap = (np.arange(W)[:, None, None] * N + np.zeros((1, P, 1), np.int64) + cols[None, None, :]).reshape(-1)
        first = torch.as_tensor(np.broadcast_to(pair(flat_candidates)[None, :, None, :], (W, P, N, 2)).reshape(-1, 2).astype(np.uint8)).cuda()
        mo_expand = None if mo is None else mo.repeat(W * P, 1)
    cum = np.full((W, N), np.inf)
    cum[0] = 0.0
    back = []
    while True:
        done = H.read(beams)["done"].reshape(W, N) != 0
        if done.all():
            break
        snap = beams.snapshot()
        c = np.full((W, N, A), np.inf)
        if score == "logp":
            with torch.no_grad():
                probs = native_actor_forward(actor, beams.state)
            full = (torch.from_numpy(cum).cuda()[:, :, None] - torch.log(probs.double()).reshape(W, N, A)).cpu().numpy()
            c[:, :, flat_candidates] = full[:, :, flat_candidates]
        else:
            expand.restore(snap, emap, rows=False)
            PS.play(expand, actor, mo=mo_expand, first=first, state_in=beams.state, state_src=torch.as_tensor(emap).cuda())
            re = H.read(expand)
            assert np.all(re["done"] == 1) and np.all(re["status"] == 0)
            c[:, :, flat_candidates] = re[objective].astype(np.float64).reshape(W, P, N).transpose(0, 2, 1)
        c[~(cum < np.inf)] = np.inf
        c[:, :, 0] = np.where(done, cum, c[:, :, 0])
        parent, action, cum = R.beam_select(c, done, W)
        none = parent < 0
        assert not np.any(none[0] & ~done[0])
        parent, action = np.where(none, parent[:1], parent), np.where(none, action[:1], action)
        beams.restore(snap, (parent.astype(np.int64) * N + cols).reshape(-1), rows=True)
        act = torch.as_tensor(pair(np.maximum(action, 0).reshape(-1)).astype(np.uint8)).cuda()
        beams.rollout(act[None].contiguous(), trace=False, rewards=False, mo=mo_beams, state=True)
        back.append((parent, action))
    r = H.read(beams)
    best, obj = np.zeros(N, np.int64), None
    if objective is not None:
        final = np.where(cum < np.inf, r[objective].astype(np.float64).reshape(W, N), np.inf)
        best = np.argmin(final, axis=0)
        obj = final[best, cols]
    actions, rank = np.zeros((len(back), N, 2), np.uint8), best.copy()
    for t in range(len(back) - 1, -1, -1):
        parent, action = back[t]
        a = action[rank, cols]
        actions[t, a >= 0] = pair(a[a >= 0])
        rank = parent[rank, cols]
    return dict(cost=cum, best=best, actions=actions, objective=obj)


def _flat(pairs, pair_div):
    return [a * pair_div + b for a, b in pairs]


def _same_as_reference(res, ref):
    assert np.array_equal(H.bits(H.host(res["cost"])), H.bits(ref["cost"]))
    assert np.array_equal(H.host(res["best"]), ref["best"])
    assert res["actions"].dtype == np.uint8 and np.array_equal(res["actions"], ref["actions"])
    if ref["objective"] is None:
        assert res["objective"] is None
    else:
        assert np.array_equal(H.bits(H.host(res["objective"])), H.bits(ref["objective"]))


def _replays(torch, fresh, res, objective, mo=None):
    fresh.rollout(torch.from_numpy(res["actions"]).cuda(), trace=False, rewards=False, mo=mo)
    r = H.read(fresh)
    assert np.all(r["done"] == 1)
    assert np.array_equal(r[objective].astype(np.float64), H.host(res["objective"]))


def test_logp_width_1_is_greedy_play(torch_gpu):
    """Every action of the variant as candidate: actions, steps, read(), the final rows and the schedule of greedy play on
    an identical batch, bit for bit."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    s, N = H.gen_10x5(32, 400), 128
    actor = _actor(torch, 20, 30, 21)
    outs = []
    for beam in (False, True):
        b = EnvBatch(s, N, rng_seed=13)
        b.record_schedule()
        b.reset()
        if beam:
            res = PS.beam_search(b, actor, 1)
            assert res["objective"] is None and np.all(H.host(res["best"]) == 0) and res["expand"] is None
            res = dict(actions=res["actions"], steps=res["steps"].astype(np.int32))
        else:
            res = PS.play(b, actor, record_actions=True)
            res = dict(actions=H.host(res["actions"]), steps=H.host(res["steps"]))
        outs.append(dict(res=res, read=H.read(b), state=H.bits(H.host(b.state)), done=H.host(b.done), reward=H.bits(H.host(b.reward)),
                         schedule=[H.host(x) for x in b.schedule()]))
    H.same(outs[0], outs[1], "greedy play vs beam of width 1")
    assert np.all(outs[1]["read"]["done"] == 1) and np.array_equal(outs[1]["res"]["steps"], H.ops(s, 32, N))


@pytest.mark.parametrize("width", [4, 7])
def test_logp_equals_the_reference_loop(torch_gpu, width):
    """width x 30 = 120 and 210 candidates: neither is a multiple of 64."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    s, N = H.gen_10x5(16, 410), 64
    actor = _actor(torch, 20, 30, 22)
    make = lambda: EnvBatch(s, N, rng_seed=14)
    src = make()
    src.reset()
    ref = _reference_search(torch, src, actor, width, "logp", "makespan", _flat(H.DET_SO, 5), 5, 30)
    timings = {}
    res = PS.beam_search(src, actor, width, objective="makespan", candidates=H.DET_SO, timings=timings)
    _same_as_reference(res, ref)
    assert res["beams"].N == width * N and res["cost"].shape == (width, N)
    assert set(timings) == {"forward", "select", "snapshot", "restore", "rollout", "step"} and timings["rollout"] == 0.0
    assert np.array_equal(res["steps"], H.ops(s, 16, N))
    cost = H.host(res["cost"])
    assert np.all(np.diff(cost, axis=0) >= 0) and np.all(np.isfinite(cost))           # ranks in ascending cost
    assert np.array_equal(H.read(src)["makespan"].astype(np.float64), H.host(res["objective"]))
    fresh = make()
    fresh.reset()
    _replays(torch, fresh, res, "makespan")
    # the most likely sequence (objective=None: rank 0) through reused beams
    src2 = make()
    src2.reset()
    ref0 = _reference_search(torch, src2, actor, width, "logp", None, _flat(H.DET_SO, 5), 5, 30)
    res0 = PS.beam_search(src2, actor, width, candidates=H.DET_SO, beams=res["beams"])
    _same_as_reference(res0, ref0)
    assert res0["beams"] is res["beams"] and np.all(H.host(res0["best"]) == 0)


def test_rollout_width_1_is_policy_lookahead(torch_gpu):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    s, N = H.gen_10x5(16, 420), 32
    actor = _actor(torch, 20, 30, 23)
    a = EnvBatch(s, N, rng_seed=15)
    a.reset()
    look = PS.policy_lookahead(a, actor, "makespan", candidates=H.DET_SO)
    b = EnvBatch(s, N, rng_seed=15)
    b.reset()
    res = PS.beam_search(b, actor, 1, objective="makespan", score="rollout", candidates=H.DET_SO)
    assert res["expand"].N == 20 * N
    assert np.array_equal(res["steps"], look["steps"])
    live = np.arange(look["actions"].shape[0])[:, None] < look["steps"][None, :]
    assert res["actions"].shape == look["actions"].shape
    assert np.array_equal(res["actions"][live], look["actions"][live])
    assert np.array_equal(H.bits(H.host(res["objective"])), H.bits(H.host(look["objective"])))
    H.same(H.read(a), H.read(b), "policy_lookahead vs rollout beam of width 1")


def test_rollout_width_2_equals_the_reference_loop(torch_gpu):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    s, N = H.gen_10x5(16, 430), 32
    actor = _actor(torch, 20, 30, 24)
    make = lambda: EnvBatch(s, N, rng_seed=16)
    src = make()
    src.reset()
    ref = _reference_search(torch, src, actor, 2, "rollout", "makespan", _flat(H.DET_SO, 5), 5, 30)
    timings = {}
    res = PS.beam_search(src, actor, 2, objective="makespan", score="rollout", candidates=H.DET_SO, timings=timings)
    _same_as_reference(res, ref)
    assert timings["rollout"] > 0.0 and timings["forward"] == 0.0
    fresh = make()
    fresh.reset()
    _replays(torch, fresh, res, "makespan")
    # deterministic candidates: a kept beam ends with the objective its last rollout promised
    assert np.array_equal(H.host(res["objective"]), H.host(res["cost"]).min(axis=0))


def test_logp_mo_discretes_equals_the_reference_loop(torch_gpu):
    """A flat-action variant with `mo` rows, on the committed suite."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, VARIANT_MO_FJSSP_DISCRETES
    insts, _, _ = H.load_suite("mo_discretes")
    insts = [a for a in insts if a.S == 1 and a.K <= 64]
    assert len(insts) >= 2
    s = H.instance_set_from(insts)
    N = 4 * len(insts)
    mo = torch.tensor([[0.5, 0.5, 800.0, 300.0]], dtype=torch.float64, device="cuda").repeat(N, 1)
    actor = _actor(torch, 25, 18, 25)
    src = EnvBatch(s, N, variant=VARIANT_MO_FJSSP_DISCRETES, rng_seed=17)
    src.reset()
    ref = _reference_search(torch, src, actor, 3, "logp", "delay_time_sum", list(range(18)), 0, 18, mo=mo)
    res = PS.beam_search(src, actor, 3, objective="tardiness", mo=mo)
    _same_as_reference(res, ref)
    r = H.read(src)
    assert np.all(r["done"] == 1) and np.array_equal(r["delay_time_sum"].astype(np.float64), H.host(res["objective"]))


def test_mid_episode_recording_source(torch_gpu):
    """A recording source stepped four times by fixed actions: the winner's schedule (the four steps included) is a valid
    schedule of its instance with the objective the search returns, and the source ends as the winning beam."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    NI, N, W = 16, 64, 4
    s = H.gen_10x5(NI, 440)
    actor = _actor(torch, 20, 30, 26)
    b = EnvBatch(s, N, rng_seed=18)
    b.record_schedule()
    b.reset()
    acts = torch.tensor(H.DET_SO, dtype=torch.uint8, device="cuda")[torch.arange(N, device="cuda") % 20]
    for t in range(4):
        b.step(acts)
    res = PS.beam_search(b, actor, W, objective="makespan", candidates=H.DET_SO)
    beams = res["beams"]
    assert beams._lib.fjsp_env_schedule_capacity(beams._h) > 0
    assert np.array_equal(res["steps"], H.ops(s, NI, N) - 4) and res["actions"].shape[0] == res["steps"].max()
    r, rb, best = H.read(b), H.read(beams), H.host(res["best"])
    win = best * N + np.arange(N)
    for key in r:
        assert np.array_equal(r[key], rb[key][win]), key
    assert np.all(r["done"] == 1) and np.array_equal(r["makespan"].astype(np.float64), H.host(res["objective"]))
    assert np.array_equal(H.bits(H.host(b.state)), H.bits(H.host(beams.state))[win])
    table, length = [H.host(x) for x in b.schedule()]
    for e in range(0, N, 5):
        a = s.arrays(e % NI)
        rows = sch.rows(table, length, e)
        assert sch.validate(a, rows, 0) == [], e
        assert sch.objectives(a, rows, 0)["makespan"] == r["makespan"][e], e
    # branch batches of another size are refused before anything is touched
    with pytest.raises(ValueError, match="beam_search"):
        PS.beam_search(b, actor, W + 1, objective="makespan", candidates=H.DET_SO, beams=beams)
    with pytest.raises(ValueError, match="beam_search"):
        PS.beam_search(b, actor, W, objective="makespan", score="rollout", candidates=H.DET_SO, beams=beams, expand=beams)
    H.same(H.read(b), r, "the source after the refused calls")


def test_width_4_leaves_the_greedy_path(torch_gpu):
    """Width 1 and width 4 are not silently the same search: for one of eight fixed seeds the most likely sequence a beam
    of 4 keeps differs from the greedy one."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    s, N = H.gen_10x5(16, 450), 32
    found = None
    for seed in range(31, 39):
        actor = _actor(torch, 20, 30, seed)
        g = EnvBatch(s, N, rng_seed=19)
        g.reset()
        greedy = H.host(PS.play(g, actor, record_actions=True)["actions"])
        b = EnvBatch(s, N, rng_seed=19)
        b.reset()
        res = PS.beam_search(b, actor, 4)
        assert res["actions"].shape == greedy.shape
        if not np.array_equal(res["actions"], greedy):
            found = seed
            break
    assert found is not None
