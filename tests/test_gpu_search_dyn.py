"""GPU: fjsp_schedule_search_dyn (schedule.search_dyn, policy_search.local_search on a MO_DFJSP batch) against
tests/search_dyn_reference.py bit for bit -- plan, objective, history, accepted, status and trace -- in every accept mode
and objective, on the recorded shops and the hand-made window cases, at its edges, replayed through the decode kernel,
twice, in shards, at the LDS limit, and where it refuses."""
import numpy as np
import pytest

from tests import decode_dyn_reference as DD
from tests import decode_reference as D
from tests import helpers as H
from tests import schedule_fixture as F
from tests import search_dyn_cases as SC
from tests import search_dyn_reference as SD

pytestmark = pytest.mark.gpu

LDS_CU = 160 * 1024
ACCEPTS = (SD.STRICT, SD.SIDEWAYS, SD.TABU)
COLS = (SD.MAKESPAN, SD.TARDINESS, SD.ENERGY)


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def eps():
    return SC.episodes()


def _batch(s, N, **kw):
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    return EnvBatch(s, N, variant=DD.VARIANT, **kw)


def _solved(arrs):
    """An InstanceSet of hand-made MO_DFJSP shops (tests/decode_dyn_reference.py shop), fluid LPs solved here."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    s = fi.InstanceSet(len(arrs))
    for i, a in enumerate(arrs):
        s.set_raw(i, a.Jr, a.p, a.elig_n, a.elig_list, a.count, a.arrive, a.delivery, a.ddt)
        s.set_dynamic(i, a.power, a.idle_power, a.bk_n, a.bk)
    return s.solve_fluid()


@pytest.fixture(scope="module")
def gen8801(torch_gpu, eps):
    """(batch of 4 envs, instance, plans int32[4][76][3]): 76 rows, 6 machines, 19 windows, 3 orders; random plans."""
    a, cap = SC.shop(eps, "gen8801")
    b = _batch(H.instance_set_from([a]), 4)
    assert b.decode_capacity() == cap == 76
    return b, a, SC.random_plans(a, 4, 5, cap)


@pytest.fixture(scope="module")
def matrix(gen8801):
    """The reference on gen8801 in every accept mode and objective, once: {(accept, objective): result}."""
    b, a, plans = gen8801
    k = SC.MATRIX
    return {(ac, col): SD.search([a] * 4, plans, k["rounds"], k["n_cand"], col, ac, k["tenure"], k["seed"]) for ac in ACCEPTS for col in COLS}


def _search(torch, b, plans, rounds, Q, col, ac, tenure, seed):
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    got = sch.search_dyn(b, torch.from_numpy(np.ascontiguousarray(plans)), rounds, Q, col, ac, tenure, seed, trace=True)
    return {k: v.cpu().numpy() for k, v in got.items()}


def _equal(got, want, what):
    for key in SD.KEYS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (what, key)


def _compare(torch, b, insts, plans, rounds, Q, col, ac, tenure, seed, what):
    want = SD.search(insts, plans, rounds, Q, col, ac, tenure, seed, first_env=b.first_env)
    _equal(_search(torch, b, plans, rounds, Q, col, ac, tenure, seed), want, what)
    return want


@pytest.mark.parametrize("col", COLS)
@pytest.mark.parametrize("ac", ACCEPTS)
def test_kernel_equals_the_reference_on_gen8801(torch_gpu, gen8801, matrix, ac, col):
    b, a, plans = gen8801
    k = SC.MATRIX
    want = matrix[(ac, col)]
    _equal(_search(torch_gpu, b, plans, k["rounds"], k["n_cand"], col, ac, k["tenure"], k["seed"]), want, (ac, col))
    assert np.all(want["status"] == 0) and want["accepted"].sum() > 0 and want["objective"].shape == (4, 3)


def test_energy_is_the_key_under_objective_2(matrix):
    """The same start and the same draws: the first round's winner by energy is not the winner by makespan in some env."""
    for ac in ACCEPTS:
        assert np.any(matrix[(ac, SD.ENERGY)]["trace"][0] != matrix[(ac, SD.MAKESPAN)]["trace"][0]), ac


def test_the_smallest_shop(torch_gpu, eps):
    """gen8802: 8 rows, 3 machines, 5 windows."""
    a, cap = SC.shop(eps, "gen8802")
    assert cap == 8 and a.M == 3 and int(np.sum(a.bk_n)) == 5
    b = _batch(H.instance_set_from([a]), 3)
    plans = SC.random_plans(a, 3, 4, cap)
    for ac in ACCEPTS:
        for col in COLS:
            _compare(torch_gpu, b, [a] * 3, plans, 8, 16, col, ac, 2, 3, ("gen8802", ac, col))


def test_hand_made_shops_and_a_one_operation_plan(torch_gpu):
    """DD.hand_cases: one- and two-machine shops, one per window branch, env i on case i.  Seven of them are one operation on
    one machine: L = 1 clamps the swap span, no swap is ever taken and the plan stays."""
    cases = DD.hand_cases()
    insts = [c[1] for c in cases]
    b = _batch(_solved(insts), len(cases))
    cap = b.decode_capacity()
    assert cap == 3
    plans = np.full((len(cases), cap, 3), -1, np.int32)
    for i, c in enumerate(cases):
        plans[i, :len(c[2])] = c[2]
    single = [i for i, c in enumerate(cases) if len(c[2]) == 1]
    assert len(single) == 7
    for ac in ACCEPTS:
        for col in COLS:
            want = _compare(torch_gpu, b, insts, plans, 4, 8, col, ac, 1, 2, ("hand-made", ac, col))
            assert np.array_equal(want["history"][0], [c[4][col] for c in cases])
            assert np.all(want["trace"][:, single, 0] != SD.S.MOVE_SWAP) and np.array_equal(want["plan"][single], plans[single])


def test_the_nine_recorded_shops_in_one_batch(torch_gpu, eps):
    """Env i on episode i's instance: plans of 8 to 1 157 rows under cap = 1 157 (padding rows), nine instances under one
    launch (inst = env % n_inst), plans that many waves' worth of rows copy in and out of LDS."""
    insts = [ep["inst"] for ep in eps]
    b = _batch(H.instance_set_from(insts), len(eps))
    cap = b.decode_capacity()
    assert cap == 1157 and len(eps) == 9 and b.search_dyn_lds() > 0
    plans = np.stack([D.plan_from_table(ep["table"], cap) for ep in eps])
    want = _compare(torch_gpu, b, insts, plans, 2, 8, SD.MAKESPAN, SD.SIDEWAYS, 0, 4, "nine shops")
    assert np.all(want["status"] == 0)
    _compare(torch_gpu, b, insts, plans, 2, 8, SD.ENERGY, SD.TABU, 1, 4, "nine shops, tabu on energy")


@pytest.mark.parametrize("Q", [1, 5, 64])
def test_candidate_counts(torch_gpu, gen8801, Q):
    b, a, plans = gen8801
    for col, ac in ((SD.MAKESPAN, SD.SIDEWAYS), (SD.ENERGY, SD.TABU)):
        _compare(torch_gpu, b, [a] * 4, plans, 4, Q, col, ac, 2, 3, (Q, col, ac))


@pytest.mark.parametrize("tenure", [0, 50])
def test_tenure_zero_and_beyond_the_rounds(torch_gpu, gen8801, tenure):
    b, a, plans = gen8801
    _compare(torch_gpu, b, [a] * 4, plans, 6, 16, SD.TARDINESS, SD.TABU, tenure, 9, tenure)


def test_aspiration_takes_a_tabu_candidate(torch_gpu, gen8801):
    b, a, plans = gen8801
    k = SC.ASPIRATION
    want = _compare(torch_gpu, b, [a] * 4, plans, k["rounds"], k["n_cand"], SD.MAKESPAN, SD.TABU, k["tenure"], k["seed"], "aspiration")
    assert sum(len(x) for x in want["aspired"]) > 0


def test_a_plan_that_does_not_decode_stops_its_env_alone(torch_gpu, gen8801):
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as ps
    b, a, plans = gen8801
    bad = plans.copy()
    bad[2, 3, 2] = 99                                                             # machine out of range: status 3
    for col, ac in ((SD.MAKESPAN, SD.SIDEWAYS), (SD.ENERGY, SD.TABU)):
        want = _compare(torch_gpu, b, [a] * 4, bad, 5, 16, col, ac, 2, 8, ("bad plan", col, ac))
        good = SD.search([a] * 4, plans, 5, 16, col, ac, 2, 8)
        assert want["status"].tolist() == [0, 0, 3, 0]
        assert np.array_equal(want["plan"][2], bad[2]) and np.all(want["history"][:, 2] == -1) and np.all(want["objective"][2] == -1)
        assert np.all(want["trace"][:, 2] == 0) and want["accepted"][2] == 0
        keep = [0, 1, 3]
        for key in SD.KEYS:
            x, y = (want[key][:, keep], good[key][:, keep]) if key in ("history", "trace") else (want[key][keep], good[key][keep])
            assert np.array_equal(x, y), key
    with pytest.raises(ValueError):
        ps.local_search(b, torch_gpu.from_numpy(bad), 2)


def test_rounds_zero_returns_the_input(torch_gpu, gen8801):
    b, a, plans = gen8801
    for ac in ACCEPTS:
        want = _compare(torch_gpu, b, [a] * 4, plans, 0, 8, SD.ENERGY, ac, 1, 2, ("rounds 0", ac))
        assert np.array_equal(want["plan"], plans) and want["history"].shape == (1, 4) and want["trace"].shape == (0, 4, 3)
        assert np.array_equal(want["objective"], DD.decode([a] * 4, plans)["objective"][:, 0])


def test_the_same_call_twice_and_shards(torch_gpu, gen8801):
    b, a, plans = gen8801
    for col, ac in ((SD.MAKESPAN, SD.SIDEWAYS), (SD.ENERGY, SD.TABU)):
        one = _search(torch_gpu, b, plans, 10, 32, col, ac, 3, 31)
        two = _search(torch_gpu, b, plans, 10, 32, col, ac, 3, 31)
        parts = [_search(torch_gpu, _batch(H.instance_set_from([a]), 2, first_env=k), plans[k:k + 2], 10, 32, col, ac, 3, 31) for k in (0, 2)]
        for key in SD.KEYS:
            assert np.array_equal(one[key], two[key]), key
            assert np.array_equal(np.concatenate([p[key] for p in parts], 1 if key in ("history", "trace") else 0), one[key]), key
        assert not np.array_equal(_search(torch_gpu, b, plans, 10, 32, col, ac, 3, 32)["trace"], one["trace"])


def test_replay_through_the_decode_kernel(torch_gpu, gen8801):
    """The trace applied round by round with schedule.apply_moves and decoded by decode_dyn on the device gives the history
    and the plan (tabu: the best plan of the replay, the earliest among equals)."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    b, a, plans = gen8801
    start = torch.from_numpy(plans).cuda()
    for col in COLS:
        for ac in ACCEPTS:
            res = sch.search_dyn(b, start, 10, 32, col, ac, 3, 23, trace=True)
            pl = start
            first = sch.decode_dyn(b, pl)["objective"][:, 0]
            assert torch.equal(first[:, col], res["history"][0])
            best, best_plan = first.clone(), start.clone()
            for t in range(10):
                pl = sch.apply_moves(pl, res["trace"][t][:, None])[:, 0].contiguous()
                now = sch.decode_dyn(b, pl)
                assert bool((now["status"] == 0).all()) and torch.equal(now["objective"][:, 0, col], res["history"][t + 1]), (col, ac, t)
                better = now["objective"][:, 0, col] < best[:, col]
                best = torch.where(better[:, None], now["objective"][:, 0], best)
                best_plan = torch.where(better[:, None, None], pl, best_plan)
            assert torch.equal(res["plan"], best_plan if ac == SD.TABU else pl), (col, ac)
            assert torch.equal(res["objective"], best if ac == SD.TABU else now["objective"][:, 0]), (col, ac)


def _search_dyn_bytes(jobs, M, ops):
    """fjsp_schedule_search_dyn_lds, restated: 64 states of 5 bytes per job (rounded up to 16 jobs) + 8 per machine, 24 bytes per plan row."""
    return 64 * (5 * ((jobs + 15) // 16 * 16) + 8 * M) + 24 * ops


def _two_kinds(jobs, M=2):
    """Two kinds of one stage on M machines, every machine eligible, two windows on machine 0."""
    rs = np.random.RandomState(jobs)
    p = rs.randint(1, 21, (2, M))
    return DD.shop(p, rs.randint(1, 51, (2, M)), rs.randint(1, 10, M), [[(7, 12), (40, 44)]] + [[] for _ in range(M - 1)], Jr=[1, 1],
                   count=[[jobs - jobs // 3, jobs // 3]], delivery=(int(p.max()) * 3,))


def test_the_lds_limit(torch_gpu, gen8801):
    """One instance just under the limit runs and equals the reference; one job more is refused, with the bytes in the message."""
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    under = max(j for j in range(16, 1000) if _search_dyn_bytes(j, 2, j) <= LDS_CU)
    assert _search_dyn_bytes(under + 1, 2, under + 1) > LDS_CU
    assert gen8801[0].search_dyn_lds() == _search_dyn_bytes(24, 6, 76) and gen8801[0].search_lds() == 0
    a = _two_kinds(under)
    b = _batch(_solved([a]), 2)
    assert b.search_dyn_lds() == _search_dyn_bytes(under, 2, under) and b.decode_capacity() == under
    rs = np.random.RandomState(2)
    plans = np.stack([D.random_plan(a, rs, under) for _ in range(2)])
    _compare(torch, b, [a, a], plans, 2, 4, SD.ENERGY, SD.TABU, 1, 6, "under the limit")
    big = _batch(_solved([_two_kinds(under + 1)]), 1)
    assert big.search_dyn_lds() == 0 and big.decode_dyn_group() > 0
    with pytest.raises(_capi.FjspError) as err:
        sch.search_dyn(big, torch.full((1, under + 1, 3), -1, dtype=torch.int32), 1, 4)
    assert err.value.code == _capi.FJSP_E_UNSUPPORTED and str(_search_dyn_bytes(under + 1, 2, under + 1)) in str(err.value)


def test_refusals(torch_gpu, gen8801):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as ps
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    torch = torch_gpu
    b, a, plans = gen8801
    plan = torch.from_numpy(plans).cuda()
    # another variant: refused, with a pointer at the entry that searches it
    mk01 = F.load()["mk01"][1][0]["inst"]
    so = EnvBatch(H.instance_set_from([mk01]), 1)
    assert so.search_dyn_lds() == 0 and so.search_lds() > 0
    with pytest.raises(_capi.FjspError) as err:
        sch.search_dyn(so, torch.full((1, so.decode_capacity(), 3), -1, dtype=torch.int32), 1, 8)
    assert err.value.code == _capi.FJSP_E_UNSUPPORTED and "fjsp_schedule_search " in str(err.value) + " "
    # the arguments: (rounds, n_cand, objective, accept, tenure)
    for args in [(1, 0), (1, 65), (-1, 8), (1, 8, 0, 0, -1), (1, 8, 3), (1, 8, -1), (1, 8, 0, 3), (2 ** 31 - 1, 64)]:
        with pytest.raises(_capi.FjspError) as err:
            sch.search_dyn(b, plan, *args)
        assert err.value.code == _capi.FJSP_E_ARG, args
    out = sch.search_dyn(b, plan, 1, 8, trace=True)
    ptr, st = _capi.ptr, b._stream()
    full = [b._h, ptr(plan), 1, 8, 0, 1, 0, 0, 0, ptr(out["plan"]), ptr(out["objective"]), ptr(out["history"]), ptr(out["accepted"]),
            ptr(out["status"]), ptr(out["trace"]), st]
    for null in (0, 1, 9, 10, 11, 12, 13):
        assert b._lib.fjsp_schedule_search_dyn(*[None if i == null else v for i, v in enumerate(full)]) == _capi.FJSP_E_ARG, null
    assert b._lib.fjsp_schedule_search_dyn(*[None if i == 14 else v for i, v in enumerate(full)]) == 0          # d_trace may be null
    with pytest.raises(ValueError):
        sch.search_dyn(b, plan[:, :-1], 1, 8)
    for kw in (dict(neighbourhood="critical"), dict(neighbourhood="mixed"), dict(objective="power"), dict(neighbours=65), dict(accept="anneal"),
               dict(tenure=-1)):
        with pytest.raises(ValueError):
            ps.local_search(b, plan, 1, **kw)
    with pytest.raises(ValueError):
        ps.local_search(b, plan[:, :-1], 1)


def test_local_search_on_a_mo_dfjsp_batch(torch_gpu, gen8801):
    """Three objective columns, table and length of the returned plan, the history's end against the objective, and a
    BatchedMODFJSP wrapper taken like its batch."""
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as ps
    from deep_reinforcement_learning_for_fjsp_amd.environments import BatchedMODFJSP
    torch = torch_gpu
    b, a, plans = gen8801
    plan = torch.from_numpy(plans).cuda()
    first = DD.decode([a] * 4, plans)["objective"][:, 0]
    for col, objective in enumerate(("makespan", "tardiness", "energy")):
        for accept in ("sideways", "tabu"):
            res = ps.local_search(b, plan, 20, 64, objective=objective, seed=col, accept=accept, tenure=4, trace=True)
            assert set(res) == {"plan", "objective", "history", "accepted", "table", "length", "status", "trace"}
            assert tuple(res["objective"].shape) == (4, 3) and res["accepted"].dtype == torch.int64 and bool((res["status"] == 0).all())
            want = DD.decode([a] * 4, res["plan"].cpu().numpy())
            assert np.all(want["status"] == 0)
            assert np.array_equal(res["objective"].cpu().numpy(), want["objective"][:, 0]), objective
            assert np.array_equal(res["table"].cpu().numpy(), want["table"][:, 0]) and np.array_equal(res["length"].cpu().numpy(), want["length"][:, 0])
            hist = res["history"].cpu().numpy()
            assert hist.shape == (21, 4) and np.array_equal(hist[0], first[:, col])
            if accept == "sideways":
                assert np.all(np.diff(hist, axis=0) <= 0) and np.array_equal(hist[-1], want["objective"][:, 0, col])
            else:
                assert np.array_equal(hist.min(0), want["objective"][:, 0, col])
            assert np.any(want["objective"][:, 0, col] < hist[0]), objective      # (20 x 64 neighbours of a random plan do find a better one)
    env = BatchedMODFJSP(H.instance_set_from([a]), n_envs=4)
    res = ps.local_search(b, plan, 5, 16, objective="energy", seed=3)
    wrapped = ps.local_search(env, plan, 5, 16, objective="energy", seed=3)
    for key in res:
        assert torch.equal(res[key], wrapped[key]), key
