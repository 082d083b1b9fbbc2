"""GPU: fjsp_schedule_evolve_active (schedule.evolve_active, policy_search.genetic_search(decoder="active")) against
tests/evolve_active_reference.py bit for bit in every output -- population, its vectors, best plan, objective, history,
status, trace and inserted rows -- over population sizes, generation counts and mutation rates on two handles of two
objectives, on the hand-made plans of the active decoder, the 140-job and the three-order shops, with shared instances, in
shards, with more envs than are resident at once (a workgroup evolves a second env on the LDS and the workspace slots of
its first, also behind an env that stopped with a status), against decode_active on the device, and where the entry
refuses."""
import numpy as np
import pytest

from tests import decode_limit_cases as DL
from tests import evolve_active_cases as AC
from tests import evolve_active_reference as EA
from tests import evolve_cases as EC
from tests import evolve_reference as E
from tests import helpers as H
from tests import schedule_fixture as F

pytestmark = pytest.mark.gpu

LDS_CU = 160 * 1024


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _batch(s, N, variant, **kw):
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    return EnvBatch(s, N, variant=variant, **kw)


@pytest.fixture(scope="module")
def gen8801(torch_gpu):
    """(batch of 4 envs created as SO_DFJSP, instance, population int32[4][64][76][3])."""
    a, pops = EC.gen8801()
    b = _batch(H.instance_set_from([a]), 4, AC.SO_DFJSP)
    assert b.decode_capacity() == pops.shape[2] == 76
    return b, a, pops


@pytest.fixture(scope="module")
def mk01(torch_gpu):
    """(batch of 4 envs, variant, instance, population int32[4][64][55][3]), as tests/test_gpu_evolve.py builds it."""
    variant, eps = F.load()["mk01"]
    a = eps[0]["inst"]
    b = _batch(H.instance_set_from([a]), 4, variant)
    return b, variant, a, EC.population(a, 4, 64, b.decode_capacity(), 6)


def _evolve(torch, b, pops, w, generations, mut_rate, seed, trace=True):
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    got = sch.evolve_active(b, torch.from_numpy(np.ascontiguousarray(pops)), generations, torch.from_numpy(np.ascontiguousarray(w, np.int64)),
                            mut_rate, seed, trace=trace)
    return {k: v.cpu().numpy() for k, v in got.items() if v is not None}


def _equal(got, want, what, keys=EA.KEYS):
    for key in keys:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (what, key)


def _compare(torch, b, insts, variant, pops, w, generations, mut_rate, seed, what):
    want = EA.evolve(insts, variant, pops, w, generations, mut_rate, seed, first_env=b.first_env)
    _equal(_evolve(torch, b, pops, w, generations, mut_rate, seed), want, what)
    return want


def _envs(res, envs):
    """The envs `envs` of a result, key by key (history and trace carry the env on their second axis)."""
    return {k: (res[k][:, envs] if k in ("history", "trace") else res[k][envs]) for k in EA.KEYS}


@pytest.mark.parametrize("mut_rate", AC.MUT_RATES)
@pytest.mark.parametrize("generations", AC.GENERATIONS)
@pytest.mark.parametrize("pop", AC.POPS)
def test_kernel_equals_the_reference_on_gen8801(torch_gpu, gen8801, pop, generations, mut_rate):
    b, a, pops = gen8801
    want = _compare(torch_gpu, b, [a] * 4, AC.SO_DFJSP, pops[:, :pop], AC.unit_weights(4), generations, mut_rate, AC.SEED, (pop, generations, mut_rate))
    assert np.all(want["status"] == 0) and want["population_objective"].shape == (4, pop, 2) and want["inserted"].sum() > 0
    if pop > 1 and generations > 0:
        mutated = want["trace"][..., 2] >= 0
        assert not mutated[..., 0].any() and (mut_rate > 0 or not mutated.any()) and (mut_rate < E.MUT_ONE or mutated[..., 1:].all())


@pytest.mark.parametrize("mut_rate", AC.MUT_RATES)
@pytest.mark.parametrize("generations", AC.GENERATIONS)
@pytest.mark.parametrize("pop", AC.POPS)
def test_kernel_equals_the_reference_on_mk01(torch_gpu, mk01, pop, generations, mut_rate):
    b, variant, a, pops = mk01
    want = _compare(torch_gpu, b, [a] * 4, variant, pops[:, :pop], AC.unit_weights(4), generations, mut_rate, AC.SEED, ("mk01", pop, generations, mut_rate))
    assert np.all(want["status"] == 0) and want["population_objective"].shape == (4, pop, 2)


@pytest.mark.parametrize("case", range(len(AC.RECORDED)))
def test_recorded_histories_are_the_active_ones(torch_gpu, gen8801, case):
    """What a kernel that still decoded semi-actively would fail without the reference: env 0's recorded history."""
    b, a, pops = gen8801
    c = AC.RECORDED[case]
    got = _evolve(torch_gpu, b, pops[:, :c["pop"]], np.array([AC.RECORDED_WEIGHTS] * 4), c["generations"], c["mut_rate"], AC.SEED)
    assert got["history"][:, 0].tolist() == c["active"] != c["semi"]
    if c["inserted"] is not None:
        assert got["inserted"][0, :8].tolist() == c["inserted"]


@pytest.mark.parametrize("generations", [0, 2])
@pytest.mark.parametrize("P", [1, 2])
def test_hand_made_plans(torch_gpu, P, generations):
    """decode_active_cases' plans as populations of copies, env i on case i's instance: the reference, and the hand-made
    begins and counts themselves (decode_active's table of the winner)."""
    torch = torch_gpu
    cases, insts, pops = AC.hand_populations(P)
    b = _batch(H.instance_set_from(insts), len(cases), 0)
    assert b.decode_capacity() == pops.shape[2]
    want = _compare(torch, b, insts, 0, pops, AC.unit_weights(len(cases)), generations, 0, 5, ("hand-made", P, generations))
    got = b.evolve_active(torch.from_numpy(pops), generations, torch.from_numpy(AC.unit_weights(len(cases))), 0, 5)
    table = b.decode_active(got["plan"], want_table=True)["table"].cpu().numpy()
    for i, c in enumerate(cases):
        assert want["status"][i] == 0 and table[i, 0, :len(c.plan), 4].tolist() == c.begins, c.name
        assert got["inserted"][i].tolist() == [c.inserted] * P, c.name


def test_the_140_job_shop_takes_three_draws_for_its_job_set(torch_gpu):
    a = EC.many_jobs()
    b = _batch(H.instance_set_from([a]), 2, 0)
    assert b.decode_capacity() == 140
    pops = EC.population(a, 2, 12, 140, 4)
    for mut_rate in (0, 6554):
        want = _compare(torch_gpu, b, [a] * 2, 0, pops, AC.unit_weights(2), 3, mut_rate, EC.BIT_63_64["seed"], ("2x70", mut_rate))
        assert np.all(want["status"] == 0)
    c = E.child_stream(E.env_stream(EC.BIT_63_64["seed"], 0), 1, 12, 1)
    assert E.in_set(c, 63) != E.in_set(c, 64)


@pytest.fixture(scope="module")
def three_orders(torch_gpu):
    """(instance, cap, InstanceSet, base populations int32[2][2][1157][3]) of the recorded three-order SO_DFJSP shop."""
    a, cap = EC.multi_order()
    return a, cap, H.instance_set_from([a]), EC.population(a, 2, 2, cap, 3)


def test_the_three_order_shop(torch_gpu, three_orders):
    a, cap, s, pops = three_orders
    b = _batch(s, 2, AC.SO_DFJSP)
    assert b.decode_capacity() == cap == 1157
    want = _compare(torch_gpu, b, [a] * 2, AC.SO_DFJSP, pops, AC.unit_weights(2), 1, E.MUT_ONE, 5, "three orders")
    assert np.all(want["status"] == 0) and np.all(want["inserted"] > 0)


def test_envs_that_share_instances_and_shards(torch_gpu):
    """Env e on instance e % 2 of (gen8801, gen8800 padded to its capacity); envs 2..3 with first_env = 2 equal those envs of
    the whole batch."""
    eps = EC.episodes()
    a, c = EC.shop(eps, "gen8801")[0], EC.shop(eps, "gen8800")[0]
    insts = [a, c, a, c]
    s = H.instance_set_from([a, c])
    b = _batch(s, 4, AC.SO_DFJSP)
    cap = b.decode_capacity()
    assert cap == 76 and b.n_inst == 2
    pops = np.stack([EC.population(insts[e], 1, 10, cap, 20 + e)[0] for e in range(4)])
    w = AC.unit_weights(4)
    whole = _compare(torch_gpu, b, insts, AC.SO_DFJSP, pops, w, 3, 6554, 13, "shared instances")
    assert np.all(whole["status"] == 0)
    part = _evolve(torch_gpu, _batch(s, 2, AC.SO_DFJSP, first_env=2), pops[2:], w[2:], 3, 6554, 13)
    _equal(part, _envs(whole, [2, 3]), "shard")
    again = _evolve(torch_gpu, b, pops, w, 3, 6554, 13)
    other = _evolve(torch_gpu, b, pops, w, 3, 6554, 14)
    _equal(again, whole, "again")
    assert not np.array_equal(other["trace"], whole["trace"])


def _more_than_resident(torch, a, s, variant, base, resident, P, generations, envs, what):
    """N = resident + 5 envs in one call: the reference on `envs`, every env against a call on the shard of 64 envs that
    holds it (every env of a shard is its workgroup's first tenant), the statuses where they belong."""
    pops, w = AC.more_than_resident(base, resident, P)
    N = len(pops)
    b = _batch(s, N, variant)
    assert b.evolve_active_resident() == resident == b.decode_active_resident() // 64 and N == resident + 5
    got = _evolve(torch, b, pops, w, generations, 6554, AC.SEED)
    assert got["status"][:3].tolist() == [0, 2, 5] and not got["status"][3:].any()
    assert np.all(got["inserted"][1:3] == 0) and got["inserted"][resident + 1].sum() > 0 and got["inserted"][resident + 2].sum() > 0
    for e in envs:
        one = EA.evolve([a], variant, pops[e:e + 1], w[e:e + 1], generations, 6554, AC.SEED, first_env=e)
        _equal(_envs(got, [e]), one, (what, e))
    for k in range(0, N, 64):
        n = min(64, N - k)
        part = _evolve(torch, _batch(s, n, variant, first_env=k), pops[k:k + n], w[k:k + n], generations, 6554, AC.SEED)
        _equal(part, _envs(got, list(range(k, k + n))), (what, "shard at", k))


def test_more_envs_than_are_resident_on_gen8801(torch_gpu, gen8801):
    _, a, pops = gen8801
    envs = AC.compared(2048)
    assert envs == [0, 1, 2, 4, 2047, 2048, 2049, 2050, 2051, 2052]
    _more_than_resident(torch_gpu, a, H.instance_set_from([a]), AC.SO_DFJSP, pops, 2048, 4, 2, envs, "gen8801 beyond resident")


def test_more_envs_than_are_resident_on_the_three_order_shop(torch_gpu, three_orders):
    """The reference on six envs: the first tenants around the statuses, the last first tenant, and the second tenants of
    the two workgroups whose first stopped with a status.  Resident: 128 MiB / (8 bytes x 1157 rows x 64 lanes) = 226 envs."""
    a, cap, s, pops = three_orders
    assert (128 << 20) // (8 * cap * 64) == 226
    _more_than_resident(torch_gpu, a, s, AC.SO_DFJSP, pops, 226, 2, 1, [0, 1, 2, 225, 227, 228], "three orders beyond resident")


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
    w = AC.unit_weights(4)
    for generations in (0, 3):
        want = _compare(torch_gpu, b, [a] * 4, AC.SO_DFJSP, bad, w, generations, 6554, 8, ("bad individual", code, generations))
        good = EA.evolve([a] * 4, AC.SO_DFJSP, pops, w, generations, 6554, 8)
        assert want["status"].tolist() == [0, 0, code, 0]
        assert np.array_equal(want["population"][2], bad[2]) and np.array_equal(want["plan"][2], bad[2, 0])
        assert np.all(want["history"][:, 2] == -1) and np.all(want["objective"][2] == -1) and np.all(want["population_objective"][2] == -1)
        assert np.all(want["trace"][:, 2] == 0) and np.all(want["inserted"][2] == 0)
        _equal(_envs(want, [0, 1, 3]), _envs(good, [0, 1, 3]), "the other envs")


def test_bad_weights_give_status_5_and_stop_their_env_alone(torch_gpu, gen8801):
    b, a, pops = gen8801
    pops = pops[:, :6].copy()
    pops[1, 2, 0, 2] = 99                                                         # (status 5 outranks the individual's status 3)
    w = np.array([[1, 0], [1, -1], [0, 0], [0, 1]], np.int64)
    want = _compare(torch_gpu, b, [a] * 4, AC.SO_DFJSP, pops, w, 3, 6554, 8, "bad weights")
    good = EA.evolve([a] * 4, AC.SO_DFJSP, gen8801[2][:, :6], np.array([[1, 0], [1, 1], [1, 1], [0, 1]], np.int64), 3, 6554, 8)
    assert want["status"].tolist() == [0, 5, 5, 0]
    for e in (1, 2):
        assert np.array_equal(want["population"][e], pops[e]) and np.all(want["history"][:, e] == -1) and np.all(want["trace"][:, e] == 0)
        assert np.all(want["inserted"][e] == 0)
    _equal(_envs(want, [0, 3]), _envs(good, [0, 3]), "the other envs")


@pytest.mark.parametrize("generations", [4, 5])
def test_consistency_with_decode_active(torch_gpu, gen8801, mk01, generations):
    """Without the reference: decode_active of the last generation gives its vectors and counts with status 0, decode_active
    of the best plan gives the objective; the semi-active decode of the same rows gives no less."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    for b, pops in ((gen8801[0], gen8801[2][:, :33]), (mk01[0], mk01[3][:, :33])):
        w = torch.from_numpy(AC.unit_weights(4))
        res = sch.evolve_active(b, torch.from_numpy(pops), generations, w, 6554, 5)
        dec = sch.decode_active(b, res["population"], n_cand=33)
        assert bool((dec["status"] == 0).all()) and torch.equal(dec["objective"], res["population_objective"])
        assert torch.equal(dec["inserted"], res["inserted"]) and res["inserted"].dtype == torch.int32
        best = sch.decode_active(b, res["plan"])
        assert torch.equal(best["objective"][:, 0], res["objective"])
        assert bool((sch.decode(b, res["population"], n_cand=33)["objective"] >= res["population_objective"]).all())
        key = (res["objective"] * w.to(res["objective"].device)).sum(1)
        assert torch.equal(res["history"][-1], key) and bool((res["history"][1:] <= res["history"][:-1]).all())
        L = dec["length"].cpu().numpy()
        pop_out = res["population"].cpu().numpy()
        assert np.all(L == L[0, 0]) and np.all(pop_out[:, :, L[0, 0]:] == -1) and np.all(pop_out[:, :, :L[0, 0]] >= 0)
        less = sch.evolve_active(b, torch.from_numpy(pops), generations - 1, w, 6554, 5)
        assert not torch.equal(less["population"], res["population"]) and torch.equal(less["history"], res["history"][:-1])


def _evolve_bytes(jobs, M):
    """fjsp_schedule_evolve_lds of a handle of two objectives, restated (tests/test_gpu_evolve.py)."""
    j16 = (jobs + 15) // 16 * 16
    return 64 * (5 * j16 + 4 * M + 4 * ((j16 + 31) // 32)) + 1024


def _two_kinds(jobs):
    rs = np.random.RandomState(jobs)
    return DL.instance("2 kinds", [1, 1], rs.randint(1, 21, (2, 2)), [[jobs - jobs // 3, jobs // 3]], delivery=[60])


def test_refusals_and_the_lds_limit(torch_gpu, gen8801):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    b, a, pops = gen8801
    assert b.evolve_lds() == _evolve_bytes(24, 6) and b.evolve_active_resident() == 2048
    pop = torch.from_numpy(pops[:, :8]).cuda()
    w = torch.from_numpy(AC.unit_weights(4)).cuda()
    out = sch.evolve_active(b, pop, 1, w, trace=True)
    canary = {k: v.clone() for k, v in out.items()}
    work = torch.empty_like(pop)
    ptr, st = _capi.ptr, b._stream()
    full = [b._h, ptr(pop), 8, 1, ptr(w), 6554, 0, 0, ptr(out["population"]), ptr(work), ptr(out["population_objective"]), ptr(out["plan"]),
            ptr(out["objective"]), ptr(out["history"]), ptr(out["status"]), ptr(out["trace"]), ptr(out["inserted"]), st]
    for null in (0, 1, 4, 8, 9, 10, 11, 12, 13, 14):
        assert b._lib.fjsp_schedule_evolve_active(*[None if i == null else v for i, v in enumerate(full)]) == _capi.FJSP_E_ARG, null
    for bad in [(0, 1, 0), (65, 1, 0), (8, -1, 0), (8, 1, -1), (8, 1, 65537), (64, 2 ** 26, 0)]:      # (pop, generations, mut_rate)
        args = list(full)
        args[2], args[3], args[5] = bad
        assert b._lib.fjsp_schedule_evolve_active(*args) == _capi.FJSP_E_ARG, bad
    # MO_DFJSP: refused with decode_active's reason, and nothing is resident
    dyn = _batch(H.instance_set_from([a]), 4, EC.VARIANT)
    assert dyn.evolve_active_resident() == 0 and dyn.evolve_lds() > 0
    for call in (lambda: sch.evolve_active(dyn, pop, 1), lambda: sch.decode_active(dyn, pop[:, 0])):
        with pytest.raises(_capi.FjspError) as err:
            call()
        assert err.value.code == _capi.FJSP_E_UNSUPPORTED and "an insertion under breakdown shifts is not defined" in str(err.value)
    # a handle beyond evolve's limit: refused as evolve refuses it, with the bytes, before any device work
    under = max(j for j in range(16, 1000) if _evolve_bytes(j, 2) <= LDS_CU)
    big = _batch(H.instance_set_from([_two_kinds(under + 16)]), 1, 0)
    fits = _batch(H.instance_set_from([_two_kinds(under)]), 1, 0)
    assert big.evolve_lds() == 0 and fits.evolve_lds() == _evolve_bytes(under, 2) and fits.evolve_active_resident() == fits.decode_active_resident() // 64 > 0
    empty = torch.full((1, 2, under + 16, 3), -1, dtype=torch.int32)
    messages = []
    for entry in (sch.evolve_active, sch.evolve):
        with pytest.raises(_capi.FjspError) as err:
            entry(big, empty, 1)
        assert err.value.code == _capi.FJSP_E_UNSUPPORTED and str(_evolve_bytes(under + 16, 2)) in str(err.value)
        messages.append(str(err.value).replace("fjsp_schedule_evolve_active", "fjsp_schedule_evolve"))
    assert messages[0] == messages[1]
    torch.cuda.synchronize()
    for k, v in out.items():                                                      # no refused call wrote anything
        assert torch.equal(v, canary[k]), k
    for null in (15, 16):                                                         # d_trace and d_pop_inserted may be null
        assert b._lib.fjsp_schedule_evolve_active(*[None if i == null else v for i, v in enumerate(full)]) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        sch.evolve_active(b, pop[:, :, :-1], 1)
    with pytest.raises(ValueError):
        sch.evolve_active(b, pop, 1, w[:, :1])


def test_genetic_search_under_either_decoder(torch_gpu, gen8801):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as ps
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    b, a, pops = gen8801
    pop = torch.from_numpy(pops[:, :32]).cuda()
    res = ps.genetic_search(b, pop, 6, objective="makespan", mutation=0.1, seed=2, decoder="active")
    assert set(res) == {"plan", "objective", "history", "population", "population_objective", "status", "inserted", "active_plan", "table"}
    want = EA.evolve([a] * 4, AC.SO_DFJSP, pops[:, :32], np.array([[1, 0]] * 4), 6, 6554, 2)
    for key in ("plan", "objective", "history", "population", "population_objective", "status", "inserted"):
        assert np.array_equal(res[key].cpu().numpy(), want[key]), key
    # the begin-ordered plan of the winner decodes semi-actively to the table and to the active objective
    dec = sch.decode(b, res["active_plan"], want_table=True)
    assert bool((dec["status"] == 0).all()) and torch.equal(dec["objective"][:, 0], res["objective"]) and torch.equal(dec["table"][:, 0], res["table"])
    assert bool((sch.decode(b, res["plan"])["objective"][:, 0, 0] >= res["objective"][:, 0]).all())
    # the default is the path as it was: schedule.evolve on the same inputs, key by key
    w = torch.tensor([[0, 1]] * 4)
    plain = ps.genetic_search(b, pop, 3, objective="tardiness", seed=4)
    same = sch.evolve(b, pop, 3, w, 6554, 4)
    assert set(plain) == {"plan", "objective", "history", "population", "population_objective", "status"}
    assert all(torch.equal(plain[k], same[k]) for k in plain)
    named = ps.genetic_search(b, pop, 3, objective="tardiness", seed=4, decoder="semi_active")
    assert all(torch.equal(plain[k], named[k]) for k in plain)
    assert not torch.equal(ps.genetic_search(b, pop, 3, objective="tardiness", seed=4, decoder="active")["history"], plain["history"])
    with pytest.raises(ValueError):
        ps.genetic_search(b, pop, 1, decoder="lamarckian")
    dyn = _batch(H.instance_set_from([a]), 4, EC.VARIANT)
    assert ps.genetic_search(dyn, pop, 1)["status"].tolist() == [0] * 4
    with pytest.raises(_capi.FjspError):
        ps.genetic_search(dyn, pop, 1, decoder="active")
