"""GPU: policy_search.improve's neighbourhoods -- "uniform" is the default, "critical" and "mixed" draw from the moves of
the critical path (schedule.critical) -- on Mk01 and a batch of 10 x 5 instances: 8 envs' rule schedules, 12 rounds x 32
neighbours."""
import numpy as np
import pytest

from tests import helpers as H
from tests import schedule_fixture as F

pytestmark = pytest.mark.gpu

N, ROUNDS, NEIGHBOURS = 8, 12, 32
KEYS = ("plan", "objective", "history", "accepted", "table", "length")


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module", params=["mk01", "10x5"])
def start(request, torch_gpu):
    """(batch, instances per env, variant, plan int32[N, cap, 3]): the schedules of N episodes of random rule pairs."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, global_actions
    torch = torch_gpu
    if request.param == "mk01":
        variant, eps = F.load()["mk01"]
        s, n_inst = H.instance_set_from([eps[0]["inst"]]), 1
    else:
        variant, n_inst = 0, 4
        s = fi.InstanceSet(n_inst).generate_range(4200, fi.bench_10x5_params()).solve_fluid()
    b = EnvBatch(s, N, variant=variant, rng_seed=5)
    T = b.record_schedule()
    acts = torch.from_numpy(global_actions(23, 0, N, T, 6, 5)).cuda()
    b.reset()
    for t in range(T):
        b.step(acts[t])
    assert bool((b.done != 0).all())
    table, length = b.schedule()
    return b, [s.arrays(i % n_inst) for i in range(N)], variant, sch.plan_of(table).contiguous()


def _run(start, **kw):
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as ps
    b, insts, variant, plan = start
    return ps.improve(b, plan, kw.pop("rounds", ROUNDS), NEIGHBOURS, **kw)


def test_the_default_is_uniform(torch_gpu, start):
    x, y = _run(start, seed=3), _run(start, seed=3, neighbourhood="uniform")
    for key in KEYS:
        assert torch_gpu.equal(x[key], y[key]), key


@pytest.mark.parametrize("neighbourhood", ["critical", "mixed"])
def test_seed_history_objective_and_feasibility(torch_gpu, start, neighbourhood):
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    b, insts, variant, plan = start
    res, again = _run(start, seed=1, neighbourhood=neighbourhood), _run(start, seed=1, neighbourhood=neighbourhood)
    for key in KEYS:
        assert torch.equal(res[key], again[key]), key
    hist = res["history"].cpu().numpy()
    assert hist.shape == (ROUNDS + 1, N) and np.all(np.diff(hist, axis=0) <= 0)
    assert np.array_equal(b.decode(plan)["objective"][:, 0, 0].cpu().numpy(), hist[0])
    back = b.decode(res["plan"], want_table=True)
    assert bool((back["status"] == 0).all())
    assert torch.equal(back["objective"][:, 0], res["objective"]) and torch.equal(back["table"][:, 0], res["table"])
    obj = res["objective"].cpu().numpy()
    assert np.array_equal(obj[:, 0], hist[-1])
    table, length = res["table"].cpu().numpy(), res["length"].cpu().numpy()
    assert np.array_equal(sch.plan_of(table), res["plan"].cpu().numpy())
    for i in range(N):
        rows = table[i, :length[i]].astype(np.int64)
        assert np.all(table[i, length[i]:] == -1)
        assert sch.validate(insts[i], rows, variant) == [], i
        want = sch.objectives(insts[i], rows, variant)
        assert obj[i].tolist() == [want["makespan"], want["delay_time_sum"]], i
    acc = res["accepted"].cpu().numpy()
    assert np.all(acc >= (np.diff(hist, axis=0) < 0).sum(0)) and np.all(acc <= ROUNDS)


@pytest.mark.parametrize("neighbourhood", ["critical", "mixed"])
def test_no_rounds_returns_the_input(torch_gpu, start, neighbourhood):
    torch = torch_gpu
    b, insts, variant, plan = start
    res = _run(start, rounds=0, neighbourhood=neighbourhood)
    assert torch.equal(res["plan"], plan) and res["history"].shape == (1, N) and int(res["accepted"].sum()) == 0
    assert torch.equal(res["objective"], b.decode(plan)["objective"][:, 0])


def test_arguments_are_checked(torch_gpu, start):
    for neighbourhood in ("critical", "mixed"):
        with pytest.raises(ValueError):
            _run(start, rounds=1, neighbourhood=neighbourhood, objective="tardiness")
    with pytest.raises(ValueError):
        _run(start, rounds=1, neighbourhood="n5")
