"""GPU: the two searches that end in pareto.select -- lookahead.rule_front over fixed rule pairs and
policy_search.pareto_front over several actors' sampled episodes -- against the existing ways of playing the same
episodes one at a time (EnvBatch.rollout, policy_search.best_of / play) and tests/pareto_reference.py.  Small fixtures:
8 envs over 2 generated 10x5 instances (SO_FJSSP), 4 envs over 2 MO_FJSSP_discretes instances with per-env mo rows."""
import numpy as np
import pytest

from tests import helpers as H
from tests import pareto_reference as R
from tests.golden import make_lookahead_golden as G

pytestmark = pytest.mark.gpu

N = 8
ALL_SO = [(a, m) for a in range(6) for m in range(5)]          # all 30 pairs; task rule 5 and machine rule 4 are random.choice
OBJ = ("makespan", "tardiness")


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def so_instances(torch_gpu):
    return H.gen_10x5(2, 370)


def _so_source(torch, s, seed=31, record=True, presteps=2):
    """A recording SO_FJSSP batch, reset and stepped `presteps` times with deterministic pairs: mid-episode."""
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    b = EnvBatch(s, N, rng_seed=seed)
    if record:
        b.record_schedule()
    b.reset()
    pre = torch.tensor(H.DET_SO, dtype=torch.uint8, device="cuda")[(torch.arange(N, device="cuda") * 3) % 20]
    for _ in range(presteps):
        b.step(pre)
    return b


def _mo_source(torch):
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, VARIANT_MO_FJSSP_DISCRETES
    insts, _, _ = H.load_suite("mo_discretes")
    insts = [a for a in insts if a.S == 1 and a.K <= 64 and int((a.count.reshape(a.S, a.R) * a.Jr[None, :]).sum()) <= 64][:2]
    assert len(insts) == 2
    s = H.instance_set_from(insts)
    make = lambda: EnvBatch(s, 4, variant=VARIANT_MO_FJSSP_DISCRETES, rng_seed=33)
    return s, make, G.mo_rows(torch, 4)


def _everything(b):
    """What "the source is left exactly as it was" covers: rows, read() and the schedule, floats by bits."""
    out = dict(read=H.read(b), state=H.bits(H.host(b.state)), done=H.host(b.done), reward=H.bits(H.host(b.reward)))
    if b._lib.fjsp_env_schedule_capacity(b._h) > 0:
        out["schedule"] = [H.host(x) for x in b.schedule()]
    return out


def _vectors(b, objectives=OBJ):
    r = b.read()
    key = dict(makespan="makespan", tardiness="delay_time_sum")
    return np.stack([r[key[o]].double().cpu().numpy() for o in objectives], axis=1)          # [n, D]


def _check_selection(res, cap):
    obj = res["objectives"].cpu().numpy()
    want = R.select(obj, None, cap)
    index = res["index"].cpu().numpy()
    assert index.dtype == want[0].dtype and index.shape == want[0].shape
    assert np.array_equal(index, want[0])
    assert np.array_equal(res["count"].cpu().numpy(), want[1])
    assert np.array_equal(res["mask"].cpu().numpy(), want[2])
    assert np.array_equal(H.bits(res["front"].cpu().numpy()), H.bits(R.front_points(obj, want[0])))
    return obj, want


def test_rule_front_so(torch_gpu, so_instances):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.lookahead import make_branch, rule_front
    s = so_instances
    b = _so_source(torch, s)
    before = _everything(b)
    res = rule_front(b, ALL_SO)
    H.same(_everything(b), before, "source after rule_front")
    assert res["objectives"].shape == (30, N, 2) and res["objectives"].dtype == torch.float64 and res["branch"].N == 30 * N
    obj, want = _check_selection(res, 30)
    assert np.all(want[1] >= 1)
    T = int(H.ops(s, 2, N).max())
    for p, pair in enumerate(ALL_SO):
        if pair[0] == 5 or pair[1] == 4:
            continue
        alone = _so_source(torch, s, record=False)
        alone.rollout(torch.tensor(pair, dtype=torch.uint8, device="cuda").expand(T, N, 2).contiguous(), trace=False, rewards=False)
        assert np.all(H.read(alone)["done"] == 1)
        assert np.array_equal(H.bits(obj[p]), H.bits(_vectors(alone))), pair
    # a reused branch, a cap below the fronts, a callable objective and one objective only
    again = rule_front(b, ALL_SO, objectives=("tardiness", lambda r: r["makespan"].double(), "makespan"), branch=res["branch"], cap=1)
    assert again["branch"] is res["branch"] and again["index"].shape == (N, 1) and again["front"].shape == (N, 1, 3)
    got = again["objectives"].cpu().numpy()
    assert np.array_equal(got[:, :, 0], obj[:, :, 1]) and np.array_equal(got[:, :, 1], obj[:, :, 0]) and np.array_equal(got[:, :, 2], obj[:, :, 0])
    _check_selection(again, 1)
    one = rule_front(b, H.DET_SO, objectives=("makespan",), branch=make_branch(b, 20))
    _, w = _check_selection(one, 20)
    assert np.all(w[1] == 1)
    assert np.array_equal(one["front"][:, 0, 0].cpu().numpy(), one["objectives"][:, :, 0].min(dim=0).values.cpu().numpy())
    H.same(_everything(b), before, "source after three calls")
    with pytest.raises(ValueError, match="energy"):
        rule_front(b, H.DET_SO, objectives=("makespan", "energy"))
    with pytest.raises(ValueError):
        rule_front(b, [(6, 0)])


def test_rule_front_mo(torch_gpu):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.lookahead import rule_front
    s, make, mo = _mo_source(torch)
    b = make()
    b.reset()
    before = _everything(b)
    res = rule_front(b, list(range(18)), mo=mo)
    H.same(_everything(b), before, "source after rule_front")
    obj, _ = _check_selection(res, 18)
    T = int(H.ops(s, 2, 4).max())
    for p in (0, 4, 8, 14):                                         # flat actions below 15 use no random.choice rule
        alone = make()
        alone.reset()
        alone.rollout(torch.tensor([p, 0], dtype=torch.uint8, device="cuda").expand(T, 4, 2).contiguous(), trace=False, rewards=False, mo=mo)
        assert np.all(H.read(alone)["done"] == 1)
        assert np.array_equal(H.bits(obj[p]), H.bits(_vectors(alone))), p


def _actors(torch, S, A, hidden=128, layers=2):
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.MPPPO import ActorNet
    out = []
    for seed in (41, 42):
        torch.manual_seed(seed)
        out.append(ActorNet(S, hidden, layers, A).cuda())
    return out


def _check_pareto_front(torch, make_source, actors, k, seed, mo=None, schedule_of=None):
    """pareto_front's contract against best_of, play and the reference; returns its result with keep_branches."""
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    P = len(actors)
    b = make_source()
    before = _everything(b)
    res = PS.pareto_front(b, actors, k, seed=seed, mos=mo)
    H.same(_everything(b), before, "source after pareto_front")
    n = b.N
    assert res["objectives"].shape == (P * k, n, 2) and res["branch"].N == k * n
    obj, want = _check_selection(res, P * k)
    index = want[0]
    assert np.array_equal(res["policy"].cpu().numpy(), np.where(index >= 0, index // k, -1))
    assert np.array_equal(res["block"].cpu().numpy(), np.where(index >= 0, index % k, -1))
    assert res["policy"].dtype == torch.int32 and res["block"].dtype == torch.int32
    for p, actor in enumerate(actors):
        twin = make_source()
        bo = PS.best_of(twin, actor, k, "makespan", seed=seed, mo=mo)
        assert np.array_equal(H.bits(obj[p * k:(p + 1) * k].reshape(k * n, 2)), H.bits(_vectors(bo["branch"]))), p
        greedy = make_source()
        PS.play(greedy, actor, mo=mo)
        assert np.array_equal(H.bits(obj[p * k]), H.bits(_vectors(greedy))), p
    kept = PS.pareto_front(b, actors, k, seed=seed, mos=None if mo is None else [mo] * P, keep_branches=True, cap=2,
                           branch=[res["branch"]] + [None] * (P - 1))
    H.same(_everything(b), before, "source after keep_branches")
    assert "branch" not in kept and len(kept["branches"]) == P and kept["branches"][0] is res["branch"]
    assert len({id(x) for x in kept["branches"]}) == P and kept["index"].shape == (n, 2)
    assert np.array_equal(kept["objectives"].cpu().numpy(), obj)
    _check_selection(kept, 2)
    for p in range(P):
        assert np.array_equal(H.bits(_vectors(kept["branches"][p]).reshape(k, n, 2)), H.bits(obj[p * k:(p + 1) * k])), p
    return kept


def test_pareto_front_so_with_schedules(torch_gpu, so_instances):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    s, k = so_instances, 3
    kept = _check_pareto_front(torch, lambda: _so_source(torch, s, seed=35), _actors(torch, 20, 30), k, 5)
    front, policy, block = [kept[x].cpu().numpy() for x in ("front", "policy", "block")]
    for i in range(N):                       # the schedule of every env's first front member
        br = kept["branches"][policy[i, 0]]
        assert br._lib.fjsp_env_schedule_capacity(br._h) > 0
        table, length = [H.host(x) for x in br.schedule()]
        rows = sch.rows(table, length, block[i, 0] * N + i)
        a = s.arrays(i % 2)
        assert sch.validate(a, rows, 0) == [], i
        o = sch.objectives(a, rows, 0)
        assert o["makespan"] == front[i, 0, 0] and o["delay_time_sum"] == front[i, 0, 1], i


def test_pareto_front_mo_and_an_actor_of_another_shape(torch_gpu, so_instances):
    """MO_FJSSP_discretes with per-env mo rows (one for all actors, and one per actor), and 200 x 5 actors, which the
    play kernel refuses: the per-step loop gives the same contract."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    s, make, mo = _mo_source(torch)

    def source():
        b = make()
        b.reset()
        return b
    _check_pareto_front(torch, source, _actors(torch, 25, 18), 3, 9, mo=mo)
    wide = _actors(torch, 20, 30, hidden=200, layers=5)
    _check_pareto_front(torch, lambda: _so_source(torch, so_instances, seed=36, record=False), wide, 3, 6)
    b = _so_source(torch, so_instances, seed=36)
    with pytest.raises(ValueError):
        PS.pareto_front(b, wide, 3, mos=[None])
    with pytest.raises(ValueError):
        PS.pareto_front(b, wide, 600)
    with pytest.raises(ValueError):
        PS.pareto_front(b, wide, 3, objectives=("makespan", "flowtime"))
