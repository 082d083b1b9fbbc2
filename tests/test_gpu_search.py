"""GPU: fjsp_schedule_search (schedule.search, policy_search.local_search) against tests/search_reference.py bit for bit --
plan, objective, history, accepted, status and trace -- in every neighbourhood and accept mode, at its edges, replayed
through the decode and critical kernels, twice, in shards, and where it refuses."""
import numpy as np
import pytest

from tests import decode_limit_cases as LC
from tests import decode_reference as D
from tests import helpers as H
from tests import schedule_fixture as F
from tests import search_reference as S

pytestmark = pytest.mark.gpu

MODES = [(nb, ac) for nb in (S.UNIFORM, S.CRITICAL, S.MIXED) for ac in (S.STRICT, S.SIDEWAYS, S.TABU)]
LDS_CU = 160 * 1024
ASPIRATION_SEED = 1              # a seed with which the reference takes a tabu candidate (the test asserts that it does)


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _batch(s, N, variant=0, **kw):
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    return EnvBatch(s, N, variant=variant, **kw)


@pytest.fixture(scope="module")
def shops(torch_gpu):
    """{name: (batch, variant, [instance per env], plans int32[8][cap][3])}: Mk01, one instance under 8 envs, from its recorded
    schedule and random plans; four 10 x 5 instances under 8 envs (env e on instance e % 4) from random plans."""
    variant, eps = F.load()["mk01"]
    mk01 = eps[0]["inst"]
    rs = np.random.RandomState(6)
    b = _batch(H.instance_set_from([mk01]), 8, variant)
    cap = b.decode_capacity()
    plans = np.stack([D.plan_from_table(eps[0]["table"], cap)] + [D.random_plan(mk01, rs, cap) for _ in range(7)])
    s = H.gen_10x5(4, 4200)
    arrs = [s.arrays(i % 4) for i in range(8)]
    b10 = _batch(s, 8)
    cap10 = b10.decode_capacity()
    return {"mk01": (b, variant, [mk01] * 8, plans), "10x5": (b10, 0, arrs, np.stack([D.random_plan(a, rs, cap10) for a in arrs]))}


def _search(torch, b, plans, rounds, Q, col, nb, ac, tenure, seed):
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    got = sch.search(b, torch.from_numpy(np.ascontiguousarray(plans)), rounds, Q, col, nb, ac, tenure, seed, trace=True)
    return {k: v.cpu().numpy() for k, v in got.items()}


def _compare(torch, b, insts, variant, plans, rounds, Q, col, nb, ac, tenure, seed, what):
    got = _search(torch, b, plans, rounds, Q, col, nb, ac, tenure, seed)
    want = S.search(insts, variant, plans, rounds, Q, col, nb, ac, tenure, seed, first_env=b.first_env)
    for key in S.KEYS:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (what, key)
    return want


@pytest.mark.parametrize("nb, ac", MODES)
@pytest.mark.parametrize("name", ["mk01", "10x5"])
def test_kernel_equals_the_reference(torch_gpu, shops, name, nb, ac):
    b, variant, insts, plans = shops[name]
    want = _compare(torch_gpu, b, insts, variant, plans, 12, 32, 0, nb, ac, 3, 17, (name, nb, ac))
    assert np.all(want["status"] == 0) and want["accepted"].sum() > 0


def test_tardiness_objective(torch_gpu, shops):
    b, variant, insts, plans = shops["10x5"]
    for ac in (S.SIDEWAYS, S.TABU):
        want = _compare(torch_gpu, b, insts, variant, plans, 6, 16, 1, S.UNIFORM, ac, 2, 5, ("tardiness", ac))
        assert np.array_equal(want["history"][0], D.decode(insts, variant, plans)["objective"][:, 0, 1])


@pytest.mark.parametrize("Q", [1, 5, 64])
def test_candidate_counts(torch_gpu, shops, Q):
    b, variant, insts, plans = shops["mk01"]
    for nb, ac in ((S.UNIFORM, S.SIDEWAYS), (S.MIXED, S.TABU)):
        _compare(torch_gpu, b, insts, variant, plans, 6, Q, 0, nb, ac, 2, 3, (Q, nb, ac))


@pytest.mark.parametrize("tenure", [0, 50])
def test_tenure_zero_and_beyond_the_rounds(torch_gpu, shops, tenure):
    b, variant, insts, plans = shops["mk01"]
    for nb in (S.UNIFORM, S.CRITICAL):
        _compare(torch_gpu, b, insts, variant, plans, 6, 16, 0, nb, S.TABU, tenure, 9, (tenure, nb))


def test_aspiration_takes_a_tabu_candidate(torch_gpu, shops):
    """With a tenure beyond the rounds every moved row stays tabu, so a later move of one is taken by aspiration alone."""
    b, variant, insts, plans = shops["mk01"]
    want = _compare(torch_gpu, b, insts, variant, plans, 6, 32, 0, S.UNIFORM, S.TABU, 100, ASPIRATION_SEED, "aspiration")
    assert sum(len(x) for x in want["aspired"]) > 0





def _one_operation():
    return LC.instance("one-operation", [1], [[3]], [1])


def _one_job_fixed_machines():
    return LC.instance("one-job", [3], [[2, 0], [0, 3], [4, 0]], [1])


def _late_order():
    return LC.instance("late-order", [2, 1], [[3, 4, 0], [0, 2, 5], [6, 0, 1]], [[1, 1], [1, 2]], arrive=(0, 25), delivery=(20, 40))


def test_one_operation_clamps_the_swap_span(torch_gpu):
    a = _one_operation()
    b = _batch(H.instance_set_from([a]), 2)
    plans = np.stack([D.random_plan(a, np.random.RandomState(1), b.decode_capacity())] * 2)
    for nb, ac in MODES:
        want = _compare(torch_gpu, b, [a, a], 0, plans, 6, 8, 0, nb, ac, 1, 2, ("L = 1", nb, ac))
        assert np.all(want["trace"][..., 0] != S.MOVE_SWAP) and np.array_equal(want["plan"], plans)


def test_empty_critical_lists_accept_nothing(torch_gpu):
    a = _one_job_fixed_machines()
    b = _batch(H.instance_set_from([a]), 3)
    plans = np.stack([D.random_plan(a, np.random.RandomState(1), b.decode_capacity())] * 3)
    for ac in (S.STRICT, S.SIDEWAYS, S.TABU):
        want = _compare(torch_gpu, b, [a] * 3, 0, plans, 6, 16, 0, S.CRITICAL, ac, 1, 2, ("empty list", ac))
        assert np.all(want["accepted"] == 0) and np.all(want["trace"] == 0)
        _compare(torch_gpu, b, [a] * 3, 0, plans, 6, 16, 0, S.MIXED, ac, 1, 2, ("empty list, mixed", ac))


def test_so_dfjsp_orders_with_a_late_arrival(torch_gpu):
    a = _late_order()
    b = _batch(H.instance_set_from([a]), 4, 5)
    rs = np.random.RandomState(3)
    plans = np.stack([D.random_plan(a, rs, b.decode_capacity()) for _ in range(4)])
    first = D.decode([a] * 4, 5, plans)
    assert np.all(first["status"] == 0) and np.all(first["table"][:, 0, :, 5].max(1) > 25)      # the late order is waited for
    for nb, ac in MODES:
        _compare(torch_gpu, b, [a] * 4, 5, plans, 6, 16, 0, nb, ac, 2, 4, ("late order", nb, ac))
    _compare(torch_gpu, b, [a] * 4, 5, plans, 6, 16, 1, S.UNIFORM, S.TABU, 2, 4, "late order, tardiness")


def _wide_window(rs):
    """A shop whose critical path runs over machine 0 (five jobs of 100 there, after one unit on machine 1) while machines 1
    and 2 work through 300 operations of one unit: in begin order some two hundred rows stand between two operations that
    follow each other on machine 0, so the pair moves of those arcs rotate windows of several waves."""
    a = LC.instance("wide-window", [2, 1, 1], [[0, 1, 0], [100, 0, 0], [0, 1, 0], [0, 0, 1]], [5, 150, 150])
    plans = []
    for _ in range(2):
        rest = [(1, n, 1) for n in range(150)] + [(2, n, 2) for n in range(150)]
        rest = [rest[i] for i in rs.permutation(len(rest))]
        for n in range(1, 5):
            rest.insert(int(rs.randint(0, 120)), (0, n, 1))
        plans.append(np.array([(0, 0, 1)] + rest + [(0, n, 0) for n in range(5)], np.int32))
    return a, np.stack(plans)


def test_pair_moves_that_rotate_more_rows_than_a_wave(torch_gpu):
    a, plans = _wide_window(np.random.RandomState(4))
    b = _batch(H.instance_set_from([a]), 2)
    assert b.decode_capacity() == plans.shape[1]
    down = up = 0
    for ac, seed in ((S.SIDEWAYS, 0), (S.TABU, 0), (S.TABU, 1)):
        want = _compare(torch_gpu, b, [a, a], 0, plans, 6, 8, 0, S.CRITICAL, ac, 2, seed, ("wide window", ac, seed))
        pairs = want["trace"].reshape(-1, 3)
        pairs = pairs[pairs[:, 0] == S.MOVE_PAIR]
        dv, dw = pairs[:, 2] & 0xFFFF, pairs[:, 2] >> 16
        down, up = max(down, int(dw.max())), max(up, int((dv - dw - 1).max()))
    assert down > 64 and up > 128                  # rows moved one place down (u + 1 .. w) and up (w + 1 .. v - 1) by one move


def test_rounds_zero_returns_the_input(torch_gpu, shops):
    b, variant, insts, plans = shops["mk01"]
    for nb, ac in MODES:
        want = _compare(torch_gpu, b, insts, variant, plans, 0, 8, 0, nb, ac, 1, 2, ("rounds 0", nb, ac))
        assert np.array_equal(want["plan"], plans) and want["history"].shape == (1, 8) and want["trace"].shape == (0, 8, 3)


def test_a_plan_that_does_not_decode_stops_its_env_alone(torch_gpu, shops):
    b, variant, insts, plans = shops["mk01"]
    bad = plans.copy()
    bad[5, -1] = -1                                                               # operations missing: status 2
    bad[6, 3, 2] = 99                                                             # machine out of range: status 3
    for nb, ac in ((S.UNIFORM, S.SIDEWAYS), (S.CRITICAL, S.TABU)):
        want = _compare(torch_gpu, b, insts, variant, bad, 6, 16, 0, nb, ac, 2, 8, ("bad plan", nb, ac))
        good = S.search(insts, variant, plans, 6, 16, 0, nb, ac, 2, 8)
        assert want["status"].tolist() == [0, 0, 0, 0, 0, 2, 3, 0]
        assert np.array_equal(want["plan"][5:7], bad[5:7]) and np.all(want["history"][:, 5:7] == -1) and np.all(want["objective"][5:7] == -1)
        keep = [0, 1, 2, 3, 4, 7]
        for key in S.KEYS:
            x, y = (want[key][:, keep], good[key][:, keep]) if key in ("history", "trace") else (want[key][keep], good[key][keep])
            assert np.array_equal(x, y), key
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as ps
    with pytest.raises(ValueError):
        ps.local_search(b, torch_gpu.from_numpy(bad), 2)


@pytest.mark.parametrize("name", ["mk01", "10x5"])
def test_replay_through_the_decode_and_critical_kernels(torch_gpu, shops, name):
    """local_search's trace, replayed round by round with schedule.decode / begin_order / apply_moves, gives its history and
    its plan (tabu: the best plan of the replay, the earliest among equals)."""
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as ps
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    b, variant, insts, plans = shops[name]
    start = torch.from_numpy(plans).cuda()
    for nbh in sch.SEARCH_NEIGHBOURHOODS:
        for accept in sch.SEARCH_ACCEPT:
            res = ps.local_search(b, start, 12, 32, "makespan", 23, accept, 3, nbh, trace=True)
            assert set(res) == {"plan", "objective", "history", "accepted", "table", "length", "status", "trace"}
            assert res["accepted"].dtype == torch.int64 and bool((res["status"] == 0).all())
            pl = start
            first = sch.decode(b, pl)["objective"][:, 0, 0]
            assert torch.equal(first, res["history"][0])
            best, best_plan = first.clone(), start.clone()
            for t in range(12):
                if nbh != "uniform":
                    pl = sch.begin_order(sch.decode(b, pl, want_table=True)["table"][:, 0])[0].contiguous()
                pl = sch.apply_moves(pl, res["trace"][t][:, None])[:, 0].contiguous()
                now = sch.decode(b, pl)
                assert bool((now["status"] == 0).all()) and torch.equal(now["objective"][:, 0, 0], res["history"][t + 1]), (nbh, accept, t)
                better = now["objective"][:, 0, 0] < best
                best = torch.where(better, now["objective"][:, 0, 0], best)
                best_plan = torch.where(better[:, None, None], pl, best_plan)
            assert torch.equal(res["plan"], best_plan if accept == "tabu" else pl), (nbh, accept)
            last = sch.decode(b, res["plan"], want_table=True)
            assert torch.equal(last["objective"][:, 0], res["objective"]) and torch.equal(last["table"][:, 0], res["table"])
            assert torch.equal(last["length"][:, 0], res["length"])
            assert torch.equal(res["accepted"], (res["trace"][..., 0] != 0).sum(0))


def test_the_same_call_twice_and_shards(torch_gpu, shops):
    torch = torch_gpu
    b, variant, insts, plans = shops["mk01"]
    for nb, ac in ((S.UNIFORM, S.SIDEWAYS), (S.MIXED, S.TABU)):
        one = _search(torch, b, plans, 12, 32, 0, nb, ac, 3, 31)
        two = _search(torch, b, plans, 12, 32, 0, nb, ac, 3, 31)
        shard = _batch(H.instance_set_from(insts[:1]), 4, variant, first_env=3)
        part = _search(torch, shard, plans[3:7], 12, 32, 0, nb, ac, 3, 31)
        for key in S.KEYS:
            assert np.array_equal(one[key], two[key]), key
            sl = (slice(None), slice(3, 7)) if key in ("history", "trace") else (slice(3, 7),)
            assert np.array_equal(part[key], one[key][sl]), key
        assert not np.array_equal(_search(torch, b, plans, 12, 32, 0, nb, ac, 3, 32)["trace"], one["trace"])


def _search_bytes(jobs, M, ops):
    """fjsp_schedule_search_lds, restated: 64 decoder states, 15 words and a flag byte per plan row, the move list, 4 words."""
    return 64 * LC.state_bytes(jobs, M) + 4 * (15 * ops + (ops + 3) // 4 + 3 * 128 + 4)


def _two_kinds(jobs, M=2):
    rs = np.random.RandomState(jobs)
    return LC.instance("search-%d" % jobs, [1, 1], rs.randint(1, 21, (2, M)), [jobs - jobs // 3, jobs // 3])


def test_the_lds_limit(torch_gpu, shops):
    """One instance just under the limit runs and equals the reference; one job more is refused, with the bytes in the message."""
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    under = max(j for j in range(16, 1000) if _search_bytes(j, 2, j) <= LDS_CU)
    assert _search_bytes(under + 1, 2, under + 1) > LDS_CU
    assert shops["mk01"][0].search_lds() == _search_bytes(10, 6, 55)
    a = _two_kinds(under)
    b = _batch(H.instance_set_from([a]), 2)
    assert b.search_lds() == _search_bytes(under, 2, under) and b.decode_capacity() == under
    rs = np.random.RandomState(2)
    plans = np.stack([D.random_plan(a, rs, under) for _ in range(2)])
    _compare(torch, b, [a, a], 0, plans, 2, 4, 0, S.MIXED, S.TABU, 1, 6, "under the limit")
    over = _two_kinds(under + 1)
    big = _batch(H.instance_set_from([over]), 1)
    assert big.search_lds() == 0 and big.decode_group() > 0
    with pytest.raises(_capi.FjspError) as err:
        sch.search(big, torch.full((1, under + 1, 3), -1, dtype=torch.int32), 1, 4)
    assert err.value.code == _capi.FJSP_E_UNSUPPORTED and str(_search_bytes(under + 1, 2, under + 1)) in str(err.value)


def test_refusals(torch_gpu, shops):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as ps
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    b, variant, insts, plans = shops["mk01"]
    plan = torch.from_numpy(plans).cuda()
    for args in [(1, 65), (1, 0), (-1, 8), (1, 8, 1, 1), (1, 8, 1, 2), (1, 8, 2, 0), (1, 8, 0, 3), (1, 8, 0, 0, 3), (1, 8, 0, 0, 2, -1),
                 (2 ** 31 - 1, 64)]:
        with pytest.raises(_capi.FjspError) as err:
            sch.search(b, plan, *args)
        assert err.value.code == _capi.FJSP_E_ARG, args
    with pytest.raises(ValueError):
        sch.search(b, plan[:, :-1], 1, 8)
    for kw in (dict(neighbours=65), dict(neighbours=0), dict(objective="energy"), dict(neighbourhood="critical", objective="tardiness"),
               dict(accept="anneal"), dict(tenure=-1), dict(neighbourhood="path")):
        with pytest.raises(ValueError):
            ps.local_search(b, plan, 1, **kw)
    with pytest.raises(ValueError):
        ps.local_search(b, plan, -1)
    mo_variant, eps = F.load()["mo_dfjsp"]
    dyn = _batch(H.instance_set_from([eps[0]["inst"]]), 1, mo_variant)
    assert dyn.search_lds() == 0
    with pytest.raises(_capi.FjspError) as err:
        sch.search(dyn, torch.full((1, dyn.decode_capacity(), 3), -1, dtype=torch.int32), 1, 8)
    assert err.value.code == _capi.FJSP_E_UNSUPPORTED
