"""GPU: fjsp_schedule_search_front (schedule.search_front, policy_search.front_search) against
tests/search_front_reference.py bit for bit in every output -- plan, objective, history, accepted, status, trace and the
archive's vectors, sources, plans, count and drops -- in every accept mode under unit, mixed and per-env weights, with
archives of 1, 4, 16 and 64 slots, against the single-objective entries, on both families, at its edges, twice, in shards,
at the LDS limit, and where it refuses."""
import numpy as np
import pytest

from tests import decode_dyn_reference as DD
from tests import decode_limit_cases as LC
from tests import decode_reference as D
from tests import helpers as H
from tests import pareto_reference as PR
from tests import schedule_fixture as F
from tests import search_front_cases as FC
from tests import search_front_reference as SF
from tests import search_reference as S
from tests import test_gpu_search_dyn as TD

pytestmark = pytest.mark.gpu

LDS_CU = 160 * 1024
ACCEPTS = (SF.STRICT, SF.SIDEWAYS, SF.TABU)
WEIGHTS = ("unit0", "unit1", "unit2", "mixed", "per_env")


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def eps():
    return FC.episodes()


def _batch(s, N, variant=FC.VARIANT, **kw):
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    return EnvBatch(s, N, variant=variant, **kw)


@pytest.fixture(scope="module")
def gen8801(torch_gpu, eps):
    """(batch of 4 envs, instance, plans int32[4][76][3])."""
    a, plans = FC.gen8801(eps)
    b = _batch(H.instance_set_from([a]), 4)
    assert b.decode_capacity() == plans.shape[1] == 76
    return b, a, plans


@pytest.fixture(scope="module")
def plain(torch_gpu):
    """{name: (batch, variant, [instance per env], plans int32[8][cap][3])}: Mk01, one instance under 8 envs, and four 10 x 5
    instances under 8 envs (env e on instance e % 4), as tests/test_gpu_search.py builds them."""
    variant, eps = F.load()["mk01"]
    mk01 = eps[0]["inst"]
    rs = np.random.RandomState(6)
    b = _batch(H.instance_set_from([mk01]), 8, variant)
    cap = b.decode_capacity()
    plans = np.stack([D.plan_from_table(eps[0]["table"], cap)] + [D.random_plan(mk01, rs, cap) for _ in range(7)])
    s = H.gen_10x5(4, 4200)
    arrs = [s.arrays(i % 4) for i in range(8)]
    b10 = _batch(s, 8, 0)
    cap10 = b10.decode_capacity()
    return {"mk01": (b, variant, [mk01] * 8, plans), "10x5": (b10, 0, arrs, np.stack([D.random_plan(a, rs, cap10) for a in arrs]))}


def _front(torch, b, plans, w, rounds, Q, cap_front, ac, tenure, seed, want_plans=True):
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    got = sch.search_front(b, torch.from_numpy(np.ascontiguousarray(plans)), torch.from_numpy(np.ascontiguousarray(w, np.int64)), rounds, Q,
                           cap_front, ac, tenure, seed, trace=True, want_plans=want_plans)
    return {k: v.cpu().numpy() for k, v in got.items() if v is not None}


def _equal(got, want, what, keys=SF.KEYS):
    for key in keys:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (what, key)


def _compare(torch, b, insts, variant, plans, w, rounds, Q, cap_front, ac, tenure, seed, what):
    want = SF.search(insts, variant, plans, w, rounds, Q, cap_front, ac, tenure, seed, first_env=b.first_env)
    _equal(_front(torch, b, plans, w, rounds, Q, cap_front, ac, tenure, seed), want, what)
    return want


@pytest.fixture(scope="module")
def matrix(gen8801):
    """The reference on gen8801 with 16 slots in every accept mode under every weight set, once: {(accept, name): result}."""
    b, a, plans = gen8801
    k, ws = FC.MATRIX, FC.weight_sets()
    return {(ac, name): SF.search([a] * 4, FC.VARIANT, plans, ws[name], k["rounds"], k["n_cand"], 16, ac, k["tenure"], k["seed"])
            for ac in ACCEPTS for name in WEIGHTS}


@pytest.mark.parametrize("name", WEIGHTS)
@pytest.mark.parametrize("ac", ACCEPTS)
def test_kernel_equals_the_reference_on_gen8801(torch_gpu, gen8801, matrix, ac, name):
    b, a, plans = gen8801
    k = FC.MATRIX
    want = matrix[(ac, name)]
    _equal(_front(torch_gpu, b, plans, FC.weight_sets()[name], k["rounds"], k["n_cand"], 16, ac, k["tenure"], k["seed"]), want, (ac, name))
    assert np.all(want["status"] == 0) and want["accepted"].sum() > 0 and min(want["entrants"]) > 0 and want["front_obj"].shape == (4, 16, 3)


def test_the_weights_steer_the_search(matrix):
    """The same start and draws: under the mixed key some round takes another move than under each unit vector."""
    for ac in ACCEPTS:
        assert all(np.any(matrix[(ac, "mixed")]["trace"] != matrix[(ac, "unit%d" % c)]["trace"]) for c in range(3)), ac
        assert np.any(matrix[(ac, "per_env")]["trace"] != matrix[(ac, "mixed")]["trace"])


@pytest.mark.parametrize("cap_front", [1, 4, 64])
def test_archives_of_one_four_and_sixty_four_slots(torch_gpu, gen8801, cap_front):
    """Four slots: entrants are dropped in every env and a member leaves for an entrant that is itself dropped."""
    b, a, plans = gen8801
    k = FC.DROPS
    want = _compare(torch_gpu, b, [a] * 4, FC.VARIANT, plans, FC.weight_sets()["mixed"], k["rounds"], k["n_cand"], cap_front, SF.TABU,
                    k["tenure"], k["seed"], cap_front)
    if cap_front == 4:
        assert np.all(want["front_dropped"] > 0) and sum(want["left_for_dropped"]) > 0
    if cap_front == 1:
        assert np.all(want["front_dropped"] > 0) and np.all(want["front_count"] <= 1)
    if cap_front == 64:
        assert np.all(want["front_dropped"] == 0)
    _compare(torch_gpu, b, [a] * 4, FC.VARIANT, plans, FC.weight_sets()["per_env"], 6, 16, cap_front, SF.SIDEWAYS, 0, 5, (cap_front, "sideways"))


def test_unit_weights_equal_the_single_objective_entries(torch_gpu, gen8801, plain):
    """A cross-check that needs no reference: fjsp_schedule_search_dyn / fjsp_schedule_search (uniform) on the same batch."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    b, a, plans = gen8801
    k = FC.MATRIX
    for ac in ACCEPTS:
        for c in range(3):
            got = _front(torch, b, plans, FC.weight_sets()["unit%d" % c], k["rounds"], k["n_cand"], 8, ac, k["tenure"], k["seed"])
            one = sch.search_dyn(b, torch.from_numpy(plans), k["rounds"], k["n_cand"], c, ac, k["tenure"], k["seed"], trace=True)
            _equal(got, {key: v.cpu().numpy() for key, v in one.items()}, (ac, c), S.KEYS)
    pb, variant, insts, pl = plain["mk01"]
    for ac in ACCEPTS:
        for c in range(2):
            got = _front(torch, pb, pl, np.array([FC.UNITS[c][:2]] * 8), 8, 32, 8, ac, 3, 17)
            one = sch.search(pb, torch.from_numpy(pl), 8, 32, c, S.UNIFORM, ac, 3, 17, trace=True)
            _equal(got, {key: v.cpu().numpy() for key, v in one.items()}, ("mk01", ac, c), S.KEYS)


def test_the_smallest_shop(torch_gpu, eps):
    """gen8802: 8 rows, 3 machines, 5 windows."""
    a, cap = FC.shop(eps, "gen8802")
    b = _batch(H.instance_set_from([a]), 3)
    plans = FC.random_plans(a, 3, 4, cap)
    for ac in ACCEPTS:
        for name in ("mixed", "per_env"):
            _compare(torch_gpu, b, [a] * 3, FC.VARIANT, plans, FC.weight_sets(3)[name], 8, 16, 8, ac, 2, 3, ("gen8802", ac, name))


def test_hand_made_shops_and_a_one_operation_plan(torch_gpu):
    """DD.hand_cases: one- and two-machine shops, one per window branch, env i on case i; seven of them are one operation on one
    machine (L = 1 clamps the swap span): their archive is what the reassignments to the only machine leave of it."""
    cases = DD.hand_cases()
    insts = [c[1] for c in cases]
    b = _batch(TD._solved(insts), len(cases))
    cap = b.decode_capacity()
    plans = np.full((len(cases), cap, 3), -1, np.int32)
    for i, c in enumerate(cases):
        plans[i, :len(c[2])] = c[2]
    single = [i for i, c in enumerate(cases) if len(c[2]) == 1]
    assert cap == 3 and len(single) == 7
    w = np.array([FC.PER_ENV[i % 4] for i in range(len(cases))])
    for ac in ACCEPTS:
        want = _compare(torch_gpu, b, insts, FC.VARIANT, plans, w, 4, 8, 4, ac, 1, 2, ("hand-made", ac))
        assert np.array_equal(want["history"][0], [SF.key_of(w[i], c[4]) for i, c in enumerate(cases)])
        assert np.all(want["front_count"][single] == 1) and np.all(want["front_src"][single, 0] == (-1, 0))


def test_the_nine_recorded_shops_in_one_batch(torch_gpu, eps):
    """Env i on episode i's instance: plans of 8 to 1 157 rows under cap = 1 157, nine instances under one launch, member
    plans that many waves' worth of rows write."""
    insts = [ep["inst"] for ep in eps]
    b = _batch(H.instance_set_from(insts), len(eps))
    cap = b.decode_capacity()
    assert cap == 1157 and len(eps) == 9 and b.search_front_lds(8) > 0
    plans = np.stack([D.plan_from_table(ep["table"], cap) for ep in eps])
    w = np.array([FC.PER_ENV[i % 4] for i in range(9)])
    want = _compare(torch_gpu, b, insts, FC.VARIANT, plans, w, 2, 8, 8, SF.TABU, 1, 4, "nine shops")
    assert np.all(want["status"] == 0) and sum(want["entrants"]) > 0


@pytest.mark.parametrize("Q", [1, 2, 63, 64])
def test_candidate_counts(torch_gpu, gen8801, Q):
    b, a, plans = gen8801
    for name, ac in (("per_env", SF.SIDEWAYS), ("mixed", SF.TABU)):
        _compare(torch_gpu, b, [a] * 4, FC.VARIANT, plans, FC.weight_sets()[name], 4, Q, 16, ac, 2, 3, (Q, name, ac))


@pytest.mark.parametrize("tenure", [0, 50])
def test_tenure_zero_and_beyond_the_rounds(torch_gpu, gen8801, tenure):
    b, a, plans = gen8801
    _compare(torch_gpu, b, [a] * 4, FC.VARIANT, plans, FC.weight_sets()["mixed"], 6, 16, 16, SF.TABU, tenure, 9, tenure)


def test_saturating_weights(torch_gpu, gen8801):
    b, a, plans = gen8801
    w = np.array([FC.SATURATING, FC.SATURATING, (2 ** 62, 0, 0), (2 ** 63 - 1, 2 ** 63 - 1, 2 ** 63 - 1)], np.int64)
    for ac in ACCEPTS:
        want = _compare(torch_gpu, b, [a] * 4, FC.VARIANT, plans, w, 5, 16, 16, ac, 1, 3, ("saturating", ac))
        assert np.all(want["history"] == SF.KEY_MAX) and np.all(want["status"] == 0)


def test_a_bad_plan_and_bad_weights_stop_their_envs_alone(torch_gpu, gen8801):
    b, a, plans = gen8801
    bad = plans.copy()
    bad[2, 3, 2] = 99                                                             # machine out of range: status 3
    bad[3, 5, 0] = -7                                                             # no such kind, under bad weights: status 5 outranks 1
    w = np.array([FC.MIXED, (0, -1, 4), FC.MIXED, (0, 0, 0)], np.int64)
    for ac in (SF.SIDEWAYS, SF.TABU):
        want = _compare(torch_gpu, b, [a] * 4, FC.VARIANT, bad, w, 5, 16, 8, ac, 2, 8, ("bad", ac))
        assert want["status"].tolist() == [0, 5, 3, 5]
        good = SF.search([a] * 4, FC.VARIANT, plans, np.array([FC.MIXED] * 4), 5, 16, 8, ac, 2, 8)
        for key in SF.KEYS:
            x, y = (want[key][:, 0], good[key][:, 0]) if key in ("history", "trace") else (want[key][0], good[key][0])
            assert np.array_equal(x, y), key
        assert np.array_equal(want["plan"][1:], bad[1:]) and np.all(want["front_count"][1:] == 0) and np.all(want["front_plan"][1:] == -1)


def test_rounds_zero_returns_the_input(torch_gpu, gen8801):
    b, a, plans = gen8801
    for ac in ACCEPTS:
        want = _compare(torch_gpu, b, [a] * 4, FC.VARIANT, plans, FC.weight_sets()["per_env"], 0, 8, 4, ac, 1, 2, ("rounds 0", ac))
        assert np.array_equal(want["plan"], plans) and want["front_count"].tolist() == [1] * 4 and np.array_equal(want["front_plan"][:, 0], plans)
        assert np.array_equal(want["front_obj"][:, 0], DD.decode([a] * 4, plans)["objective"][:, 0]) and want["trace"].shape == (0, 4, 3)


def test_the_same_call_twice_and_shards(torch_gpu, gen8801):
    b, a, plans = gen8801
    w = FC.weight_sets()["per_env"]
    for ac in (SF.SIDEWAYS, SF.TABU):
        one = _front(torch_gpu, b, plans, w, 10, 32, 16, ac, 3, 31)
        two = _front(torch_gpu, b, plans, w, 10, 32, 16, ac, 3, 31)
        parts = [_front(torch_gpu, _batch(H.instance_set_from([a]), 2, first_env=k), plans[k:k + 2], w[k:k + 2], 10, 32, 16, ac, 3, 31) for k in (0, 2)]
        for key in SF.KEYS:
            assert np.array_equal(one[key], two[key]), key
            assert np.array_equal(np.concatenate([p[key] for p in parts], 1 if key in ("history", "trace") else 0), one[key]), key
        assert not np.array_equal(_front(torch_gpu, b, plans, w, 10, 32, 16, ac, 3, 32)["trace"], one["trace"])
        bare = _front(torch_gpu, b, plans, w, 10, 32, 16, ac, 3, 31, want_plans=False)          # d_front_plan may be null
        assert "front_plan" not in bare
        _equal(bare, one, "no plans", [key for key in SF.KEYS if key != "front_plan"])


def test_members_decode_to_their_vectors_and_are_their_round_s_moves(torch_gpu, gen8801):
    """Every member plan decodes through decode_dyn to its front_obj row (a free slot's plan of -1 does not decode: -1); a
    member with source (t, q) is schedule.apply_moves of candidate q's move on the replayed start plan of round t."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    b, a, plans = gen8801
    k = FC.MATRIX
    w = FC.weight_sets()["per_env"]
    res = sch.search_front(b, torch.from_numpy(plans), torch.from_numpy(w), k["rounds"], k["n_cand"], 16, SF.TABU, k["tenure"], k["seed"], trace=True)
    dec = sch.decode_dyn(b, res["front_plan"], n_cand=16)
    assert torch.equal(dec["objective"], res["front_obj"])
    held = res["front_src"][..., 1] >= 0
    assert torch.equal((dec["status"] == 0), held) and torch.equal(held.sum(1).to(torch.int32), res["front_count"])
    src, fplan = res["front_src"].cpu().numpy(), res["front_plan"].cpu()
    pl = torch.from_numpy(plans).cuda()
    seen = 0
    for t in range(k["rounds"]):
        now = pl.cpu().numpy()
        for e in range(4):
            rows = now[e][:D.plan_length(now[e])].astype(np.int64)
            moves = [m for _, m, _ in SF.round_candidates(a, FC.VARIANT, rows, t, k["n_cand"], S.env_stream(k["seed"], e), 76)]
            for s in np.flatnonzero(src[e, :, 0] == t):
                want = sch.apply_moves(pl[e:e + 1], torch.tensor([[moves[src[e, s, 1]]]], dtype=torch.int32).cuda())[0, 0]
                assert torch.equal(want.cpu(), fplan[e, s]), (t, e, s)
                seen += 1
        pl = sch.apply_moves(pl, res["trace"][t][:, None])[:, 0].contiguous()
    assert seen > 0 and seen == int(((src[..., 0] >= 0)).sum())


@pytest.mark.parametrize("ac", ACCEPTS)
@pytest.mark.parametrize("name", ["mk01", "10x5"])
def test_the_plain_family(torch_gpu, plain, name, ac):
    b, variant, insts, plans = plain[name]
    w = np.array([(1, 1), (3, 1), (1, 0), (0, 1), (1, 20), (7, 2), (2 ** 62, 2 ** 62), (1, 3)], np.int64)
    want = _compare(torch_gpu, b, insts, variant, plans, w, 8, 32, 16, ac, 3, 17, (name, ac))
    assert np.all(want["status"] == 0) and want["front_obj"].shape == (8, 16, 2) and want["accepted"].sum() > 0


def test_so_dfjsp_orders_with_a_late_arrival(torch_gpu):
    a = LC.instance("late-order", [2, 1], [[3, 4, 0], [0, 2, 5], [6, 0, 1]], [[1, 1], [1, 2]], arrive=(0, 25), delivery=(20, 40))
    b = _batch(H.instance_set_from([a]), 4, 5)
    rs = np.random.RandomState(3)
    plans = np.stack([D.random_plan(a, rs, b.decode_capacity()) for _ in range(4)])
    w = np.array([(1, 1), (1, 0), (0, 1), (2, 5)], np.int64)
    for ac in ACCEPTS:
        _compare(torch_gpu, b, [a] * 4, 5, plans, w, 6, 16, 8, ac, 2, 4, ("late order", ac))


def _front_bytes(jobs, M, ops, cap_front, NO):
    """fjsp_schedule_search_front_lds, restated: 64 states of 5 bytes per job (rounded up to 16 jobs) + 4 per machine (8 on
    MO_DFJSP), 24 bytes per plan row, 8 NO + 8 per slot, 64 x (8 NO + 4)."""
    return 64 * (5 * ((jobs + 15) // 16 * 16) + (8 if NO == 3 else 4) * M) + 24 * ops + cap_front * (8 * NO + 8) + 64 * (8 * NO + 4)


def test_the_lds_limit(torch_gpu, gen8801, plain):
    """One instance just under the limit runs and equals the reference; one job more is refused, with the bytes in the message."""
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    under = max(j for j in range(16, 1000) if _front_bytes(j, 2, j, 64, 3) <= LDS_CU)
    assert _front_bytes(under + 1, 2, under + 1, 64, 3) > LDS_CU
    for cf in (1, 16, 64):
        assert gen8801[0].search_front_lds(cf) == _front_bytes(24, 6, 76, cf, 3)
    assert gen8801[0].search_front_lds(0) == 0 and gen8801[0].search_front_lds(65) == 0
    mb = plain["mk01"][0]
    a01 = plain["mk01"][2][0]
    jobs01 = int(np.asarray(a01.count).sum())
    assert mb.search_front_lds(16) == _front_bytes(jobs01, a01.M, mb.decode_capacity(), 16, 2)
    a = TD._two_kinds(under)
    b = _batch(TD._solved([a]), 2)
    assert b.search_front_lds(64) == _front_bytes(under, 2, under, 64, 3) and b.decode_capacity() == under
    rs = np.random.RandomState(2)
    plans = np.stack([D.random_plan(a, rs, under) for _ in range(2)])
    _compare(torch, b, [a, a], FC.VARIANT, plans, np.array([FC.MIXED, (1, 1, 0)]), 2, 4, 64, SF.TABU, 1, 6, "under the limit")
    big = _batch(TD._solved([TD._two_kinds(under + 1)]), 1)
    assert big.search_front_lds(64) == 0
    with pytest.raises(_capi.FjspError) as err:
        sch.search_front(big, torch.full((1, under + 1, 3), -1, dtype=torch.int32), torch.ones(1, 3, dtype=torch.int64), 1, 4, 64)
    assert err.value.code == _capi.FJSP_E_UNSUPPORTED and str(_front_bytes(under + 1, 2, under + 1, 64, 3)) in str(err.value)


def test_refusals(torch_gpu, gen8801):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    b, a, plans = gen8801
    plan = torch.from_numpy(plans).cuda()
    w = torch.ones(4, 3, dtype=torch.int64).cuda()
    # (rounds, n_cand, cap_front, accept, tenure)
    for args in [(1, 0), (1, 65), (-1, 8), (1, 8, 0), (1, 8, 65), (1, 8, 4, 3), (1, 8, 4, -1), (1, 8, 4, 0, -1), (2 ** 31 - 1, 64)]:
        with pytest.raises(_capi.FjspError) as err:
            sch.search_front(b, plan, w, *args)
        assert err.value.code == _capi.FJSP_E_ARG, args
    out = sch.search_front(b, plan, w, 1, 8, 4, trace=True)
    ptr, st = _capi.ptr, b._stream()
    full = [b._h, ptr(plan), 1, 8, ptr(w), 1, 0, 0, 0, 4, ptr(out["plan"]), ptr(out["objective"]), ptr(out["history"]), ptr(out["accepted"]),
            ptr(out["status"]), ptr(out["trace"]), ptr(out["front_obj"]), ptr(out["front_src"]), ptr(out["front_plan"]), ptr(out["front_count"]),
            ptr(out["front_dropped"]), st]
    for null in (0, 1, 4, 10, 11, 12, 13, 14, 16, 17, 19, 20):
        assert b._lib.fjsp_schedule_search_front(*[None if i == null else v for i, v in enumerate(full)]) == _capi.FJSP_E_ARG, null
    for null in (15, 18):                                                         # d_trace and d_front_plan may be null
        assert b._lib.fjsp_schedule_search_front(*[None if i == null else v for i, v in enumerate(full)]) == 0, null
    for bad in (plan[:, :-1], ):
        with pytest.raises(ValueError):
            sch.search_front(b, bad, w, 1, 8)
    with pytest.raises(ValueError):
        sch.search_front(b, plan, w[:, :2], 1, 8)


def test_front_search_sorts_and_merges(torch_gpu, eps):
    """8 envs over 2 instances (gen8801, gen8802; env e on instance e % 2), per-env weights: the sorted fronts against the
    reference's archives, the merged fronts against tests/pareto_reference.py on those archives, and the ValueErrors."""
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as ps
    torch = torch_gpu
    shops = [FC.shop(eps, "gen8801")[0], FC.shop(eps, "gen8802")[0]]
    b = _batch(H.instance_set_from(shops), 8)
    cap = b.decode_capacity()
    insts = [shops[e % 2] for e in range(8)]
    rs = np.random.RandomState(9)
    plans = np.stack([D.random_plan(insts[e], rs, cap) for e in range(8)])
    w = np.array([FC.PER_ENV[(e // 2) % 4] for e in range(8)], np.int64)
    plan = torch.from_numpy(plans).cuda()
    res = ps.front_search(b, plan, 8, w, neighbours=32, cap_front=16, accept="tabu", tenure=3, seed=5, merge=True)
    assert set(res) == {"plan", "objective", "history", "accepted", "table", "length", "status", "front", "front_plan", "front_src", "count",
                        "dropped", "merged_front", "merged_count"}
    want = SF.search(insts, FC.VARIANT, plans, w, 8, 32, 16, SF.TABU, 3, 5)
    for key, ref in (("plan", "plan"), ("objective", "objective"), ("history", "history"), ("count", "front_count"), ("dropped", "front_dropped")):
        assert np.array_equal(res[key].cpu().numpy(), want[ref]), key
    front, fplan, fsrc = (res[key].cpu().numpy() for key in ("front", "front_plan", "front_src"))
    for e in range(8):
        held = np.flatnonzero(want["front_src"][e][:, 1] >= 0)
        order = sorted(held, key=lambda s: tuple(want["front_obj"][e, s]))
        n = len(order)
        assert np.array_equal(front[e, :n], want["front_obj"][e, order]) and np.all(front[e, n:] == -1)
        assert np.array_equal(fplan[e, :n], want["front_plan"][e, order]) and np.all(fplan[e, n:] == -1)
        assert np.array_equal(fsrc[e, :n], want["front_src"][e, order]) and np.all(fsrc[e, n:] == -1)
    # candidate k * 16 + s of instance i is slot s of env 2 k + i
    obj = want["front_obj"].reshape(4, 2, 16, 3).transpose(0, 2, 1, 3).reshape(64, 2, 3).astype(np.float64)
    valid = (want["front_src"][..., 1] >= 0).reshape(4, 2, 16).transpose(0, 2, 1).reshape(64, 2)
    index, count, _ = PR.select(obj, valid)
    assert np.array_equal(res["merged_count"].cpu().numpy(), count) and np.all(count >= 1)
    assert np.array_equal(res["merged_front"].cpu().numpy(), PR.front_points(obj, index), equal_nan=True)
    # the weights: None is ones, a vector is every env's
    ones = ps.front_search(b, plan, 3, None, neighbours=8, cap_front=4, seed=1)
    vec = ps.front_search(b, plan, 3, [1, 1, 1], neighbours=8, cap_front=4, seed=1)
    assert "merged_front" not in ones and all(torch.equal(ones[key], vec[key]) for key in ones)
    for kw in (dict(weights=[1, 1]), dict(weights=[1, -1, 1]), dict(weights=[0, 0, 0]), dict(weights=[0.5, 1, 1]), dict(weights=np.ones((7, 3), np.int64)),
               dict(cap_front=65), dict(cap_front=0), dict(neighbours=65), dict(accept="anneal"), dict(tenure=-1)):
        with pytest.raises(ValueError):
            ps.front_search(b, plan, 1, **kw)
    bad = plan.clone()
    bad[1, 0, 2] = 99
    with pytest.raises(ValueError):
        ps.front_search(b, bad, 1)
    many = _batch(H.instance_set_from(shops[1:]), 17)                             # 17 envs of one instance x 64 slots > 1024
    with pytest.raises(ValueError):
        ps.front_search(many, torch.full((17, 8, 3), -1, dtype=torch.int32), 1, merge=True)
    huge = torch.zeros(2, 4, 3, dtype=torch.int64).cuda()
    huge[1, 2, 0] = 2 ** 53
    held = torch.ones(2, 4, dtype=torch.bool).cuda()
    with pytest.raises(ValueError):
        ps.merge_fronts(huge, held, 1)
    huge[1, 2, 0] = 2 ** 53 - 1
    assert ps.merge_fronts(huge, held, 1)[1].tolist() == [1]
