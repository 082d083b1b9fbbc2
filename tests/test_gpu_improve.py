"""GPU: policy_search.improve, the hill climber on fjsp_schedule_decode, on Mk01 and one instance with order arrivals:
8 envs' rule schedules, 20 rounds x 64 neighbours."""
import numpy as np
import pytest

from tests import helpers as H
from tests import schedule_fixture as F

pytestmark = pytest.mark.gpu

N, ROUNDS, NEIGHBOURS = 8, 20, 64


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module", params=["mk01", "multiorder"])
def start(request, torch_gpu):
    """(batch, instance, variant, plan int32[N, cap, 3]): the schedules of N episodes of random rule pairs."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, global_actions
    torch = torch_gpu
    variant, eps = F.load()[request.param]
    a = eps[0]["inst"]
    b = EnvBatch(H.instance_set_from([a]), N, variant=variant, rng_seed=5)
    T = b.record_schedule()
    acts = torch.from_numpy(global_actions(23, 0, N, T, 6, 5)).cuda()
    b.reset()
    for t in range(T):
        b.step(acts[t])
    assert bool((b.done != 0).all())
    table, length = b.schedule()
    assert bool((length == T).all())
    return b, a, variant, sch.plan_of(table).contiguous()


def _run(start, **kw):
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as ps
    b, a, variant, plan = start
    return ps.improve(b, plan, kw.pop("rounds", ROUNDS), NEIGHBOURS, **kw)


@pytest.mark.parametrize("objective", ["makespan", "tardiness"])
def test_history_objective_and_feasibility(torch_gpu, start, objective):
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    b, a, variant, plan = start
    res = _run(start, objective=objective, seed=1)
    hist = res["history"].cpu().numpy()
    assert hist.shape == (ROUNDS + 1, N) and np.all(np.diff(hist, axis=0) <= 0)
    col = ("makespan", "tardiness").index(objective)
    obj = res["objective"].cpu().numpy()
    assert np.array_equal(obj[:, col], hist[-1])
    first = b.decode(plan)
    assert np.array_equal(first["objective"][:, 0, col].cpu().numpy(), hist[0])
    table, length = res["table"].cpu().numpy(), res["length"].cpu().numpy()
    assert np.array_equal(sch.plan_of(table), res["plan"].cpu().numpy())
    for i in range(N):
        rows = table[i, :length[i]].astype(np.int64)
        assert length[i] == plan.shape[1] and np.all(table[i, length[i]:] == -1)
        assert sch.validate(a, rows, variant) == [], i
        want = sch.objectives(a, rows, variant)
        assert obj[i].tolist() == [want["makespan"], want["delay_time_sum"]], i
    acc = res["accepted"].cpu().numpy()
    assert np.all(acc >= (np.diff(hist, axis=0) < 0).sum(0)) and np.all(acc <= ROUNDS)


def test_same_seed_same_result_other_seed_other_plan(torch_gpu, start):
    torch = torch_gpu
    x, y, z = _run(start, seed=3), _run(start, seed=3), _run(start, seed=4)
    for key in ("plan", "objective", "history", "accepted", "table", "length"):
        assert torch.equal(x[key], y[key]), key
    assert not torch.equal(x["plan"], z["plan"])


def test_no_rounds_returns_the_input(torch_gpu, start):
    torch = torch_gpu
    b, a, variant, plan = start
    res = _run(start, rounds=0)
    assert torch.equal(res["plan"], plan) and res["history"].shape == (1, N) and int(res["accepted"].sum()) == 0
    assert torch.equal(res["objective"], b.decode(plan)["objective"][:, 0])


def test_strict_acceptance_never_takes_an_equal_move(torch_gpu, start):
    res = _run(start, seed=2, sideways=False)
    hist = res["history"].cpu().numpy()
    assert np.array_equal(res["accepted"].cpu().numpy(), (np.diff(hist, axis=0) < 0).sum(0))
    loose = _run(start, seed=2, sideways=True)
    assert np.all(loose["accepted"].cpu().numpy() >= (np.diff(loose["history"].cpu().numpy(), axis=0) < 0).sum(0))


def test_arguments_are_checked(torch_gpu, start):
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as ps
    b, a, variant, plan = start
    with pytest.raises(ValueError):
        ps.improve(b, plan, 1, objective="energy")
    with pytest.raises(ValueError):
        ps.improve(b, plan, -1)
    broken = plan.clone()
    broken[0, 0, 2] = 99
    with pytest.raises(ValueError):
        ps.improve(b, broken, 1)
