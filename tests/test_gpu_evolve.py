"""GPU: fjsp_schedule_evolve (schedule.evolve, policy_search.genetic_search, seed_population) against
tests/evolve_reference.py bit for bit in every output -- population, its vectors, best plan, objective, history, status and
trace -- over population sizes, generation counts and mutation rates under unit, mixed and per-env weights, on both
families, on the 140-job and the three-order shops, with shared instances, in shards, against the decode entries on the
device, where an env is copied through, and where the entry refuses."""
import numpy as np
import pytest

from tests import decode_dyn_reference as DD
from tests import evolve_cases as EC
from tests import evolve_reference as E
from tests import helpers as H
from tests import schedule_fixture as F
from tests import search_front_reference as SF
from tests import test_gpu_search_dyn as TD

pytestmark = pytest.mark.gpu

LDS_CU = 160 * 1024


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _batch(s, N, variant=EC.VARIANT, **kw):
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    return EnvBatch(s, N, variant=variant, **kw)


@pytest.fixture(scope="module")
def gen8801(torch_gpu):
    """(batch of 4 envs, instance, population int32[4][64][76][3])."""
    a, pops = EC.gen8801()
    b = _batch(H.instance_set_from([a]), 4)
    assert b.decode_capacity() == pops.shape[2] == 76
    return b, a, pops


@pytest.fixture(scope="module")
def mk01(torch_gpu):
    """(batch of 4 envs on a handle of two objectives, variant, instance, population int32[4][64][55][3])."""
    variant, eps = F.load()["mk01"]
    a = eps[0]["inst"]
    b = _batch(H.instance_set_from([a]), 4, variant)
    return b, variant, a, EC.population(a, 4, 64, b.decode_capacity(), 6)


def _evolve(torch, b, pops, w, generations, mut_rate, seed, trace=True):
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    got = sch.evolve(b, torch.from_numpy(np.ascontiguousarray(pops)), generations, torch.from_numpy(np.ascontiguousarray(w, np.int64)),
                     mut_rate, seed, trace=trace)
    return {k: v.cpu().numpy() for k, v in got.items() if v is not None}


def _equal(got, want, what, keys=E.KEYS):
    for key in keys:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (what, key)


def _compare(torch, b, insts, variant, pops, w, generations, mut_rate, seed, what):
    want = E.evolve(insts, variant, pops, w, generations, mut_rate, seed, first_env=b.first_env)
    _equal(_evolve(torch, b, pops, w, generations, mut_rate, seed), want, what)
    return want


@pytest.mark.parametrize("mut_rate", EC.MUT_RATES)
@pytest.mark.parametrize("generations", EC.GENERATIONS)
@pytest.mark.parametrize("pop", EC.POPS)
def test_kernel_equals_the_reference_on_gen8801(torch_gpu, gen8801, pop, generations, mut_rate):
    b, a, pops = gen8801
    ws = EC.weight_sets()
    for name in ("unit%d" % ((pop + generations) % 3), "mixed", "per_env"):
        want = _compare(torch_gpu, b, [a] * 4, EC.VARIANT, pops[:, :pop], ws[name], generations, mut_rate, EC.SEED, (pop, generations, mut_rate, name))
        assert np.all(want["status"] == 0) and want["population_objective"].shape == (4, pop, 3)
        if pop > 1 and generations > 0:
            mutated = want["trace"][..., 2] >= 0                                 # never the elite; none at rate 0, every other child at 65536
            assert not mutated[..., 0].any() and (mut_rate > 0 or not mutated.any()) and (mut_rate < E.MUT_ONE or mutated[..., 1:].all())


@pytest.mark.parametrize("generations", EC.GENERATIONS)
@pytest.mark.parametrize("pop", EC.POPS)
def test_kernel_equals_the_reference_on_a_handle_of_two_objectives(torch_gpu, mk01, pop, generations):
    b, variant, a, pops = mk01
    for mut_rate in EC.MUT_RATES:
        want = _compare(torch_gpu, b, [a] * 4, variant, pops[:, :pop], EC.plain_weights(4), generations, mut_rate, EC.SEED, ("mk01", pop, generations, mut_rate))
        assert np.all(want["status"] == 0) and want["population_objective"].shape == (4, pop, 2)


def test_every_unit_weight(torch_gpu, gen8801):
    b, a, pops = gen8801
    ws = EC.weight_sets()
    ends = [_compare(torch_gpu, b, [a] * 4, EC.VARIANT, pops[:, :16], ws["unit%d" % c], 4, 6554, 3, ("unit", c))["objective"][:, c] for c in range(3)]
    first = DD.decode([a] * 4, pops[:, :16], None, 16)["objective"]
    assert all(np.all(ends[c] <= first[..., c].min(1)) for c in range(3))


def test_the_140_job_shop_takes_three_draws_for_its_job_set(torch_gpu):
    a = EC.many_jobs()
    b = _batch(H.instance_set_from([a]), 2, 0)
    assert b.decode_capacity() == 140 and b.evolve_lds() == 64 * (5 * 144 + 4 * 2 + 4 * 5) + 1024
    pops = EC.population(a, 2, 12, 140, 4)
    for mut_rate in (0, 6554):
        want = _compare(torch_gpu, b, [a] * 2, 0, pops, EC.plain_weights(2), 3, mut_rate, EC.BIT_63_64["seed"], ("2x70", mut_rate))
        assert np.all(want["status"] == 0)
    c = E.child_stream(E.env_stream(EC.BIT_63_64["seed"], 0), 1, 12, 1)
    assert E.in_set(c, 63) != E.in_set(c, 64)


def test_the_three_order_so_dfjsp_shop_and_the_smallest_mo_dfjsp_shop(torch_gpu):
    a, cap = EC.multi_order()
    b = _batch(H.instance_set_from([a]), 2, EC.SO_DFJSP)
    assert b.decode_capacity() == cap == 1157
    want = _compare(torch_gpu, b, [a] * 2, EC.SO_DFJSP, EC.population(a, 2, 4, cap, 3), EC.plain_weights(2), 2, E.MUT_ONE, 5, "three orders")
    assert np.all(want["status"] == 0)
    a, cap = EC.shop(EC.episodes(), "gen8802")                                    # 8 rows, 3 machines, 5 breakdown windows
    b = _batch(H.instance_set_from([a]), 3)
    for mut_rate in EC.MUT_RATES:
        _compare(torch_gpu, b, [a] * 3, EC.VARIANT, EC.population(a, 3, 9, cap, 2), EC.weight_sets(3)["per_env"], 5, mut_rate, 7, ("gen8802", mut_rate))


def test_envs_that_share_instances_and_shards(torch_gpu, gen8801):
    """Env e on instance e % 2 of (gen8801, gen8800 padded to its capacity); envs 2..3 with first_env = 2 equal those envs of
    the whole batch."""
    eps = EC.episodes()
    a, c = EC.shop(eps, "gen8801")[0], EC.shop(eps, "gen8800")[0]
    insts = [a, c, a, c]
    b = _batch(H.instance_set_from([a, c]), 4)
    cap = b.decode_capacity()
    assert cap == 76 and b.n_inst == 2
    pops = np.stack([EC.population(insts[e], 1, 10, cap, 20 + e)[0] for e in range(4)])
    w = EC.weight_sets()["per_env"]
    whole = _compare(torch_gpu, b, insts, EC.VARIANT, pops, w, 3, 6554, 13, "shared instances")
    assert np.all(whole["status"] == 0)
    part = _evolve(torch_gpu, _batch(H.instance_set_from([a, c]), 2, first_env=2), pops[2:], w[2:], 3, 6554, 13)
    for key in E.KEYS:
        x = whole[key][:, 2:] if key in ("history", "trace") else whole[key][2:]
        assert np.array_equal(part[key], x), key
    again = _evolve(torch_gpu, b, pops, w, 3, 6554, 13)
    other = _evolve(torch_gpu, b, pops, w, 3, 6554, 14)
    assert all(np.array_equal(again[key], whole[key]) for key in E.KEYS) and not np.array_equal(other["trace"], whole["trace"])


@pytest.mark.parametrize("generations", [4, 5])
def test_consistency_with_the_decode_entries(torch_gpu, gen8801, mk01, generations):
    """Without the reference: decode / decode_dyn of the last generation gives its vectors with status 0; the best plan and
    objective are its least (key, index); the history ends at that key; rows past a plan's end are -1; both parities of
    `generations` leave the last generation in the population returned."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    for b, pops, w, decode in ((gen8801[0], gen8801[2][:, :33], EC.weight_sets()["per_env"], sch.decode_dyn),
                               (mk01[0], mk01[3][:, :33], EC.plain_weights(4), sch.decode)):
        res = sch.evolve(b, torch.from_numpy(pops), generations, torch.from_numpy(w), 6554, 5)
        dec = decode(b, res["population"], n_cand=33)
        assert bool((dec["status"] == 0).all()) and torch.equal(dec["objective"], res["population_objective"])
        obj = res["population_objective"].cpu().numpy()
        keys = np.array([[SF.key_of(w[e], obj[e, q]) for q in range(33)] for e in range(4)], object)
        best = np.array([min(range(33), key=lambda q: (keys[e][q], q)) for e in range(4)])
        pop_out = res["population"].cpu().numpy()
        assert np.array_equal(res["plan"].cpu().numpy(), pop_out[np.arange(4), best]) and np.array_equal(res["objective"].cpu().numpy(), obj[np.arange(4), best])
        hist = res["history"].cpu().numpy()
        assert hist[-1].tolist() == [keys[e][best[e]] for e in range(4)] and np.all(np.diff(hist, axis=0) <= 0)
        L = dec["length"].cpu().numpy()
        assert np.all(L == L[0, 0]) and np.all(pop_out[:, :, L[0, 0]:] == -1) and np.all(pop_out[:, :, :L[0, 0]] >= 0)
        # the generation before, evolved one step further from where it stood, is not asked of the entry; the same call with
        # one generation fewer differs in its last generation, so the buffer returned is the last one written
        less = sch.evolve(b, torch.from_numpy(pops), generations - 1, torch.from_numpy(w), 6554, 5)
        assert not torch.equal(less["population"], res["population"]) and torch.equal(less["history"], res["history"][:-1])


@pytest.mark.parametrize("code", [1, 2, 3])
def test_an_individual_that_does_not_decode_stops_its_env_alone(torch_gpu, gen8801, code):
    b, a, pops = gen8801
    pops = pops[:, :6]
    bad = pops.copy()
    if code == 1:
        bad[2, 3, 5, 0] = 99                                                      # no such kind
    elif code == 2:
        bad[2, 3, -1] = -1                                                        # operations missing
    else:
        bad[2, 3, 5, 2] = 99                                                      # machine out of range
    bad[2, 5, 0, 2] = 99                                                          # (status 3 at a higher q does not decide)
    w = EC.weight_sets()["per_env"]
    for generations in (0, 3):
        want = _compare(torch_gpu, b, [a] * 4, EC.VARIANT, bad, w, generations, 6554, 8, ("bad individual", code, generations))
        good = E.evolve([a] * 4, EC.VARIANT, pops, w, generations, 6554, 8)
        assert want["status"].tolist() == [0, 0, code, 0]
        assert np.array_equal(want["population"][2], bad[2]) and np.array_equal(want["plan"][2], bad[2, 0])
        assert np.all(want["history"][:, 2] == -1) and np.all(want["objective"][2] == -1) and np.all(want["population_objective"][2] == -1)
        assert np.all(want["trace"][:, 2] == 0)
        keep = [0, 1, 3]
        for key in E.KEYS:
            x, y = (want[key][:, keep], good[key][:, keep]) if key in ("history", "trace") else (want[key][keep], good[key][keep])
            assert np.array_equal(x, y), key


def test_bad_weights_give_status_5_and_stop_their_env_alone(torch_gpu, gen8801):
    b, a, pops = gen8801
    pops = pops[:, :6].copy()
    pops[1, 2, 0, 2] = 99                                                         # (status 5 outranks the individual's status 3)
    w = np.array([EC.PER_ENV[0], [1, -1, 1], [0, 0, 0], EC.PER_ENV[3]], np.int64)
    want = _compare(torch_gpu, b, [a] * 4, EC.VARIANT, pops, w, 3, 6554, 8, "bad weights")
    good = E.evolve([a] * 4, EC.VARIANT, gen8801[2][:, :6], EC.weight_sets()["per_env"], 3, 6554, 8)
    assert want["status"].tolist() == [0, 5, 5, 0]
    for e in (1, 2):
        assert np.array_equal(want["population"][e], pops[e]) and np.all(want["history"][:, e] == -1) and np.all(want["trace"][:, e] == 0)
    for key in E.KEYS:
        x, y = (want[key][:, [0, 3]], good[key][:, [0, 3]]) if key in ("history", "trace") else (want[key][[0, 3]], good[key][[0, 3]])
        assert np.array_equal(x, y), key


def test_saturating_weights_and_a_tie(torch_gpu, gen8801):
    b, a, pops = gen8801
    want = _compare(torch_gpu, b, [a] * 4, EC.VARIANT, pops[:, :8], np.array([EC.SATURATING] * 4, np.int64), 3, 6554, 4, "saturating")
    assert np.all(want["history"] == SF.KEY_MAX) and np.all(want["trace"][:, :, 0, :2] == 0)
    k = EC.TIE
    want = _compare(torch_gpu, b, [a] * 4, EC.VARIANT, pops[:, :k["pop"]], EC.weight_sets()["unit0"], k["generations"], 0, k["seed"], "tie")
    assert len(want["ties"][0]) > 0


def _evolve_bytes(jobs, M, dyn):
    """fjsp_schedule_evolve_lds, restated: 64 states of 5 bytes per job (rounded up to 16 jobs) + 4 per machine (8 on
    MO_DFJSP) and 64 job sets of a bit per job in words of 4 bytes, and two rows of 64 keys."""
    j16 = (jobs + 15) // 16 * 16
    return 64 * (5 * j16 + (8 if dyn else 4) * M + 4 * ((j16 + 31) // 32)) + 1024


def test_refusals_and_the_lds_limit(torch_gpu, gen8801):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as ps
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    b, a, pops = gen8801
    assert b.evolve_lds() == _evolve_bytes(24, 6, True)
    pop = torch.from_numpy(pops[:, :8]).cuda()
    w = torch.from_numpy(EC.weight_sets()["mixed"]).cuda()
    out = sch.evolve(b, pop, 1, w, trace=True)
    canary = {k: v.clone() for k, v in out.items()}
    work = torch.empty_like(pop)
    ptr, st = _capi.ptr, b._stream()
    full = [b._h, ptr(pop), 8, 1, ptr(w), 6554, 0, 0, ptr(out["population"]), ptr(work), ptr(out["population_objective"]), ptr(out["plan"]),
            ptr(out["objective"]), ptr(out["history"]), ptr(out["status"]), ptr(out["trace"]), st]
    for null in (0, 1, 4, 8, 9, 10, 11, 12, 13, 14):
        assert b._lib.fjsp_schedule_evolve(*[None if i == null else v for i, v in enumerate(full)]) == _capi.FJSP_E_ARG, null
    # (pop, generations, mut_rate)
    for bad in [(0, 1, 0), (65, 1, 0), (8, -1, 0), (8, 1, -1), (8, 1, 65537), (64, 2 ** 26, 0)]:
        args = list(full)
        args[2], args[3], args[5] = bad
        assert b._lib.fjsp_schedule_evolve(*args) == _capi.FJSP_E_ARG, bad
    # a handle beyond the limit: refused with the bytes, before any device work
    under = max(j for j in range(16, 1000) if _evolve_bytes(j, 2, True) <= LDS_CU)
    big = _batch(TD._solved([TD._two_kinds(under + 16)]), 1)
    assert big.evolve_lds() == 0 and _batch(TD._solved([TD._two_kinds(under)]), 1).evolve_lds() == _evolve_bytes(under, 2, True)
    with pytest.raises(_capi.FjspError) as err:
        sch.evolve(big, torch.full((1, 2, under + 16, 3), -1, dtype=torch.int32), 1)
    assert err.value.code == _capi.FJSP_E_UNSUPPORTED and str(_evolve_bytes(under + 16, 2, True)) in str(err.value)
    torch.cuda.synchronize()
    for k, v in out.items():                                                      # no refused call wrote anything
        assert torch.equal(v, canary[k]), k
    assert b._lib.fjsp_schedule_evolve(*[None if i == 15 else v for i, v in enumerate(full)]) == 0              # d_trace may be null
    with pytest.raises(ValueError):
        sch.evolve(b, pop[:, :, :-1], 1)
    with pytest.raises(ValueError):
        sch.evolve(b, pop, 1, w[:, :2])
    for kw in (dict(objective="power"), dict(mutation=1.5), dict(generations=-1), dict(weights=[1, -1, 0]), dict(weights=[0, 0, 0])):
        with pytest.raises(ValueError):
            ps.genetic_search(b, pop, **{"generations": 1, **kw})
    with pytest.raises(ValueError):
        ps.seed_population(b, pop[:, 0], 65)


def test_seed_population_and_genetic_search(torch_gpu, gen8801):
    from deep_reinforcement_learning_for_fjsp_amd import pareto
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as ps
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    b, a, pops = gen8801
    plan = torch.from_numpy(pops[:, 0]).cuda()
    pop = ps.seed_population(b, plan, 32, shake=5, seed=3)
    assert tuple(pop.shape) == (4, 32, 76, 3) and pop.dtype == torch.int32 and torch.equal(pop[:, 0], plan)
    assert torch.equal(pop, ps.seed_population(b, plan, 32, shake=5, seed=3)) and not torch.equal(pop, ps.seed_population(b, plan, 32, shake=5, seed=4))
    assert bool((sch.decode_dyn(b, pop, n_cand=32)["status"] == 0).all())
    assert len({pop[0, q].cpu().numpy().tobytes() for q in range(32)}) > 16       # the shaken individuals differ
    three = ps.seed_population(b, torch.from_numpy(pops[:, :3]), 8, shake=2, seed=1)
    assert torch.equal(three[:, :3].cpu(), torch.from_numpy(pops[:, :3])) and bool((sch.decode_dyn(b, three, n_cand=8)["status"] == 0).all())
    for q in range(3, 8):                                                         # individual q is plan q mod 3, shaken: the same operations
        assert EC.operations(three[0, q].cpu().numpy()) == EC.operations(pops[0, q % 3])
    assert torch.equal(ps.seed_population(b, plan, 4, shake=0), plan[:, None].expand(4, 4, 76, 3))

    res = ps.genetic_search(b, pop, 6, objective="energy", mutation=0.1, seed=2, merge=True)
    assert set(res) == {"plan", "objective", "history", "population", "population_objective", "status", "merged_front", "merged_count"}
    want = E.evolve([a] * 4, EC.VARIANT, pop.cpu().numpy(), np.array([EC.UNITS[2]] * 4), 6, 6554, 2)
    for key, ref in (("plan", "plan"), ("objective", "objective"), ("history", "history"), ("population", "population"),
                     ("population_objective", "population_objective"), ("status", "status")):
        assert np.array_equal(res[key].cpu().numpy(), want[ref]), key
    # (one instance: candidate k * 32 + s is individual s of env k)
    vec = res["population_objective"].to(torch.float64).reshape(4 * 32, 1, 3).contiguous()
    index, count, _ = pareto.select(vec, torch.ones(4 * 32, 1, dtype=torch.bool, device=vec.device))
    assert torch.equal(res["merged_count"], count) and torch.equal(res["merged_front"].nan_to_num(-1.0), pareto.front_points(vec, index).nan_to_num(-1.0))
    assert int(count[0]) >= 1
    weighted = ps.genetic_search(b, pop, 2, weights=[60, 5, 1], seed=2)
    assert np.array_equal(weighted["history"].cpu().numpy(), E.evolve([a] * 4, EC.VARIANT, pop.cpu().numpy(), np.array([EC.MIXED] * 4), 2, 6554, 2)["history"])
