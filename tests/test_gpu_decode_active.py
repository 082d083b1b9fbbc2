"""GPU: fjsp_schedule_decode_active (schedule.decode_active, policy_search.left_shift) against
tests/decode_active_reference.py bit for bit -- objectives, status, tables, lengths and inserted rows -- on hand-made plans
with known answers, the reference's own schedules and random plans, every workgroup size the launcher chooses and the
candidate counts around them, more candidates than are resident at once (workspace slots used again), every status code
beside valid candidates, closure through the semi-active decode, and the refusals.

One store path: every candidate's intervals live in the handle's workspace, whatever the plan's size; Mk01 (55 rows) and the
so_dfjsp fixture's 1157-row plan are both among the golden plans below."""
import numpy as np
import pytest

from tests import decode_active_cases as AC
from tests import decode_active_reference as A
from tests import decode_reference as D
from tests import helpers as H
from tests import schedule_fixture as F

pytestmark = pytest.mark.gpu

SUITES = ("mk01", "synth10x5", "multijob", "so_sfjsp", "mo_discretes", "multiorder", "so_dfjsp")
SEMI_KEYS = ("objective", "status", "table", "length")


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def suites():
    return F.load()


def _instances(specs, seed=1):
    """A solved InstanceSet of hand-made shops: specs = [(Jr, jobs per kind, M)], p uniform in 1..20 on a random non-empty
    eligible set, one order at 0."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    rs = np.random.RandomState(seed)
    s = fi.InstanceSet(len(specs))
    for i, (Jr, jobs, M) in enumerate(specs):
        K = int(np.sum(Jr))
        p = rs.randint(1, 21, (K, M)) * (rs.rand(K, M) < 0.6)
        for k in range(K):
            if not p[k].any():
                p[k, rs.randint(M)] = rs.randint(1, 21)
        elig_list = np.zeros((K, M), np.int32)
        for k in range(K):
            e = np.flatnonzero(p[k])
            elig_list[k, :len(e)] = e
        s.set_raw(i, Jr, p, (p > 0).sum(1), elig_list, [jobs], [0], [int(p.max()) * 3])
    return s.solve_fluid()


def _batch(s, N, variant=0):
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    return EnvBatch(s, N, variant=variant)


def _random_moves(rs, plans, n_cand, machines=6):
    """int32[N][n_cand][3]: kinds 0, 1, 2 and 4 at rows inside the plan; machines 0 .. machines - 1 (some ineligible, some
    out of range); pair moves of rows at most 8 apart (some reach past the plan: status 4)."""
    N = len(plans)
    L = np.array([D.plan_length(pl) for pl in plans])
    mv = np.zeros((N, n_cand, 3), np.int32)
    mv[..., 0] = rs.choice([0, 1, 2, 4], (N, n_cand))
    mv[..., 1] = (rs.rand(N, n_cand) * np.maximum(L, 1)[:, None]).astype(np.int32)
    mv[..., 2] = rs.randint(0, machines, (N, n_cand))
    dv = rs.randint(1, 9, (N, n_cand))
    dw = (rs.rand(N, n_cand) * dv).astype(np.int64)
    mv[..., 2] = np.where(mv[..., 0] == 4, dv | (dw << 16), mv[..., 2])
    return mv


def _compare(torch, b, insts, variant, plan, moves, n_cand, what):
    args = (torch.from_numpy(np.ascontiguousarray(plan)), None if moves is None else torch.from_numpy(moves), n_cand)
    got = b.decode_active(*args, want_table=True)
    want = A.decode(insts, variant, plan, moves, n_cand)
    for key in A.KEYS:
        assert got[key].dtype == {"objective": torch.int64}.get(key, torch.int32)
        assert np.array_equal(got[key].cpu().numpy(), want[key]), (what, key)
    lean = b.decode_active(*args)
    assert lean["table"] is None
    for key in ("objective", "status", "length", "inserted"):
        assert np.array_equal(lean[key].cpu().numpy(), want[key]), (what, key, "without a table")
    return want


def test_hand_made_cases(torch_gpu):
    """The six plans with known answers, env i on case i's instance in one batch (padding rows), and each alone."""
    cases = AC.cases()
    insts = [c.inst for c in cases]
    b = _batch(H.instance_set_from(insts), len(cases))
    cap = b.decode_capacity()
    plan = np.stack([AC.DL.padded(c.plan, cap) for c in cases])
    want = _compare(torch_gpu, b, insts, 0, plan, None, 1, "hand-made")
    for i, c in enumerate(cases):
        assert want["status"][i, 0] == 0 and want["table"][i, 0, :len(c.plan), 4].tolist() == c.begins and want["inserted"][i, 0] == c.inserted, c.name
        one = _batch(H.instance_set_from([c.inst]), 1)
        _compare(torch_gpu, one, [c.inst], 0, c.plan[None], None, 1, c.name)


@pytest.mark.parametrize("suite", SUITES)
def test_golden_plans(torch_gpu, suites, suite):
    """Every episode of the suite in one batch, env i on episode i's instance (plans of different lengths: padding rows):
    the recorded plans bare, then as shared parents of three candidates with a move each, then random plans per candidate."""
    variant, eps = suites[suite]
    insts = [ep["inst"] for ep in eps]
    b = _batch(H.instance_set_from(insts), len(eps), variant)
    cap = b.decode_capacity()
    assert cap == max(len(ep["table"]) for ep in eps)
    plan = np.stack([D.plan_from_table(ep["table"], cap) for ep in eps])
    want = _compare(torch_gpu, b, insts, variant, plan, None, 1, suite)
    assert np.all(want["status"] == 0)
    rs = np.random.RandomState(len(eps))
    moved = _compare(torch_gpu, b, insts, variant, plan, _random_moves(rs, plan, 3), 3, suite + " moved")
    assert (moved["status"] == 0).any()
    per = np.stack([[D.random_plan(a, rs, cap) for _ in range(2)] for a in insts])
    rand = _compare(torch_gpu, b, insts, variant, per, None, 2, suite + " random")
    assert np.all(rand["status"] == 0) and rand["inserted"].sum() > 0


def test_random_plans_on_the_smallest_shapes_and_a_mixed_batch(torch_gpu, suites):
    """One job x one operation x one machine; M = 1; Mk01; and one batch that mixes them (padding rows, machines of the
    larger instances out of range on the smaller)."""
    s = _instances([([1], [1], 1), ([2, 3], [2, 1], 1), ([2, 1, 3], [1, 2, 1], 3)])
    mk01 = suites["mk01"][1][0]["inst"]
    rs = np.random.RandomState(2)
    for ids in ([0], [1], [3], [0, 1, 2, 3]):
        arrs = [mk01 if i == 3 else s.arrays(i) for i in ids]
        N = 2 * len(ids)
        b = _batch(H.instance_set_from(arrs), N)
        insts = [arrs[i % len(ids)] for i in range(N)]
        cap = b.decode_capacity()
        plan = np.stack([D.random_plan(a, rs, cap) for a in insts])
        want = _compare(torch_gpu, b, insts, 0, plan, None, 1, ids)
        assert np.all(want["status"] == 0)
        per = np.stack([[D.random_plan(a, rs, cap) for _ in range(5)] for a in insts])
        _compare(torch_gpu, b, insts, 0, per, _random_moves(rs, per[:, 0], 5), 5, (ids, "per candidate"))


SHOPS = [(([2] * 5, [2] * 5, 5), 256), (([2] * 4, [16] * 4, 5), 128), (([2] * 6, [50] * 6, 8), 64), (([2] * 12, [50] * 12, 20), 32)]


@pytest.mark.parametrize("spec, group", SHOPS, ids=[str(g) for _, g in SHOPS])
def test_every_workgroup_size(torch_gpu, spec, group):
    """10 jobs (256 candidates per workgroup), 64 jobs (128), 300 jobs (64, beyond 64 KB of LDS) and the largest shop of the
    reference's training distribution, 12 kinds x 50 jobs on 20 machines (32, the upper half of the wave idle): G - 1, G and
    G + 1 candidates of one env, own plans drawn from three so that the reference decodes few."""
    s = _instances([spec], seed=group)
    a = s.arrays(0)
    b = _batch(s, 1)
    assert b.decode_active_group() == group == b.decode_group()
    assert b.decode_active_resident() % group == 0 and 0 < b.decode_active_resident() <= 512 * group
    rs = np.random.RandomState(group)
    cap = b.decode_capacity()
    base = np.stack([D.random_plan(a, rs, cap) for _ in range(3)])
    ref = [A.decode_one(a, 0, pl) for pl in base]
    assert all(r["status"] == 0 for r in ref) and sum(r["inserted"] for r in ref) > 0
    for count in (group - 1, group, group + 1):
        pick = rs.randint(0, 3, count)
        got = b.decode_active(torch_gpu.from_numpy(base[pick][None]), None, count, want_table=True)
        for key in A.KEYS:
            want = np.stack([np.asarray(ref[i][key]) for i in pick])[None]
            assert np.array_equal(got[key].cpu().numpy(), want), (group, count, key)


def test_more_candidates_than_are_resident_use_the_slots_again(torch_gpu, suites):
    """One call on Mk01 with more candidates than the bounded grid holds at once: every workgroup decodes a second group on
    the entries its first group left behind.  Eight distinct (plan, move) pairs -- plans that insert a lot, a begin-ordered
    plan that inserts nothing, and one failure of each status -- are tiled over envs and candidates so that a slot's
    successive tenants differ; the reference decodes the eight once."""
    torch = torch_gpu
    variant, eps = suites["mk01"]
    a = eps[0]["inst"]
    probe = _batch(H.instance_set_from([a]), 1, variant)
    resident, cap, Q = probe.decode_active_resident(), probe.decode_capacity(), 64
    assert resident == probe.decode_active_group() * min(512, (128 << 20) // (8 * cap * probe.decode_active_group()))
    N = resident // Q + 3
    assert N * Q > resident                                                # the call really exceeds the resident bound
    rs = np.random.RandomState(5)
    plans = [D.random_plan(a, rs, cap) for _ in range(8)]
    plans[1] = A.begin_ordered_plan(A.decode_one(a, variant, plans[1])["table"], cap)
    moves = np.zeros((8, 3), np.int32)
    moves[2] = (2, 7, 0)
    moves[3] = (4, 3, 6 | (2 << 16))
    plans[4][5, 0] = 99                                                    # status 1
    plans[5][cap - 1] = -1                                                 # status 2
    moves[6] = (1, 0, 7)                                                   # status 3
    moves[7] = (3, 0, 0)                                                   # status 4
    ref = [A.decode_one(a, variant, plans[d], moves[d]) for d in range(8)]
    assert [r["status"] for r in ref[4:]] == [1, 2, 3, 4] and ref[1]["inserted"] == 0 and ref[1]["status"] == 0
    assert ref[0]["inserted"] > 0 and ref[3]["status"] == 0
    g = torch.arange(N * Q, device="cuda")
    idx = ((g * 5 + g // Q + g // resident) % 8).reshape(N, Q)                       # (what follows a tenant in its slot is another pair)
    b = _batch(H.instance_set_from([a]), N, variant)
    got = b.decode_active(torch.from_numpy(np.stack(plans)).cuda()[idx], torch.from_numpy(moves).cuda()[idx], Q, want_table=True)
    for key in A.KEYS:
        want = torch.from_numpy(np.stack([np.asarray(r[key]) for r in ref])).cuda()[idx]
        assert torch.equal(got[key], want.to(got[key].dtype)), key
    first, again = idx.flatten()[:resident], idx.flatten()[resident:]
    assert bool((first[:len(again)] != again).any())


@pytest.fixture(scope="module")
def wave(torch_gpu, suites):
    """128 valid candidates of one Mk01 env (two waves of one workgroup), own plans, with their reference results."""
    variant, eps = suites["mk01"]
    a = eps[0]["inst"]
    b = _batch(H.instance_set_from([a]), 1, variant)
    rs = np.random.RandomState(11)
    cap = b.decode_capacity()
    base = [D.random_plan(a, rs, cap) for _ in range(4)]
    ref = [A.decode_one(a, variant, pl) for pl in base]
    pick = np.arange(128) % 4
    plan = np.stack([base[i] for i in pick])[None]
    want = {key: np.stack([np.asarray(ref[i][key]) for i in pick])[None] for key in A.KEYS}
    assert np.all(want["status"] == 0) and want["inserted"].sum() > 0
    return b, a, variant, plan, want


def test_a_failure_of_each_status_beside_valid_candidates(torch_gpu, wave):
    """Lanes 0, 31, 63 and 64 of one group fail with status 1, 2, 3 and 4: their code, -1 objectives, length 0, nothing
    inserted and a table of -1; every other candidate keeps its result."""
    torch = torch_gpu
    b, a, variant, plan, base = wave
    plan, moves = plan.copy(), np.zeros((1, 128, 3), np.int32)
    want = {k: v.copy() for k, v in base.items()}
    L = D.plan_length(plan[0, 0])
    plan[0, 0, 3, 0] = 99
    plan[0, 31, L - 1] = plan[0, 31, 0]
    moves[0, 63] = (1, 2, 7)
    moves[0, 64] = (4, 0, 0)
    for lane, code in ((0, 1), (31, 2), (63, 3), (64, 4)):
        one = A.decode_one(a, variant, plan[0, lane], moves[0, lane])
        assert one["status"] == code and one["length"] == 0 and one["inserted"] == 0 and np.all(one["table"] == -1)
        for key in A.KEYS:
            want[key][0, lane] = one[key]
    got = b.decode_active(torch.from_numpy(plan), torch.from_numpy(moves), 128, want_table=True)
    for key in A.KEYS:
        assert np.array_equal(got[key].cpu().numpy(), want[key]), key


def test_closure_idempotence_and_the_semi_active_decode_around_a_call(torch_gpu, suites):
    """On the device: decode(begin_order(active table)) is the active table in begin order, decode_active of that plan
    inserts nothing, and decode of the input plans returns the same before and after a decode_active call on the handle."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    variant, eps = suites["multiorder"]
    insts = [ep["inst"] for ep in eps]
    b = _batch(H.instance_set_from(insts), len(eps), variant)
    cap = b.decode_capacity()
    rs = np.random.RandomState(4)
    plan = torch.from_numpy(np.stack([[D.random_plan(a, rs, cap) for _ in range(3)] for a in insts])).cuda()
    before = b.decode(plan, None, 3, want_table=True)
    want = D.decode(insts, variant, plan.cpu().numpy(), None, 3)
    act = b.decode_active(plan, None, 3, want_table=True)
    after = b.decode(plan, None, 3, want_table=True)
    for key in SEMI_KEYS:
        assert np.array_equal(before[key].cpu().numpy(), want[key]) and torch.equal(before[key], after[key]), key
    assert bool((act["status"] == 0).all()) and bool((act["inserted"] > 0).any())
    assert bool((act["objective"] <= before["objective"]).all()) and bool((act["objective"][..., 0] < before["objective"][..., 0]).any())
    ordered, table = sch.begin_order(act["table"])
    back = b.decode(ordered.contiguous(), None, 3, want_table=True)
    assert torch.equal(back["table"], table) and torch.equal(back["objective"], act["objective"]) and torch.equal(back["length"], act["length"])
    again = b.decode_active(ordered.contiguous(), None, 3, want_table=True)
    assert torch.equal(again["table"], table) and bool((again["inserted"] == 0).all()) and torch.equal(again["objective"], act["objective"])


def test_left_shift(torch_gpu, suites):
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as ps
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    variant, eps = suites["mk01"]
    a = eps[0]["inst"]
    N, K = 3, 4
    b = _batch(H.instance_set_from([a]), N, variant)
    cap = b.decode_capacity()
    rs = np.random.RandomState(8)
    pop = np.stack([[D.random_plan(a, rs, cap) for _ in range(K)] for _ in range(N)])
    want = A.decode([a] * N, variant, pop, None, K)
    semi = D.decode([a] * N, variant, pop, None, K)
    for plan, pick in ((pop, lambda x: x), (pop[:, 1], lambda x: x[:, 1])):
        res = ps.left_shift(b, torch.from_numpy(np.ascontiguousarray(plan)))
        assert tuple(res["plan"].shape) == plan.shape and res["plan"].dtype == torch.int32
        assert np.array_equal(res["objective"].cpu().numpy(), pick(want["objective"]))
        assert np.array_equal(res["inserted"].cpu().numpy(), pick(want["inserted"]))
        assert np.array_equal(res["before"].cpu().numpy(), pick(semi["objective"]))
        flat = pick(want["table"]).reshape(-1, cap, 6)
        ordered = np.stack([t[np.argsort(t[:, 4], kind="stable")] for t in flat]).reshape(pick(want["table"]).shape)
        assert np.array_equal(res["table"].cpu().numpy(), ordered)
        assert np.array_equal(res["plan"].cpu().numpy(), ordered[..., [0, 2, 3]])
        back = sch.decode(b, res["plan"], None, K if plan.ndim == 4 else 1, want_table=True)
        assert torch.equal(back["table"].reshape(res["table"].shape), res["table"])
        assert torch.equal(back["objective"].reshape(res["objective"].shape), res["objective"])
    bad = pop.copy()
    bad[1, 2, 0, 0] = 99
    with pytest.raises(ValueError):
        ps.left_shift(b, torch.from_numpy(bad))
    with pytest.raises(ValueError):
        ps.left_shift(b, torch.from_numpy(pop[0, 0]))


def test_refusals(torch_gpu, suites):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as ps
    torch = torch_gpu
    variant, eps = suites["mk01"]
    b = _batch(H.instance_set_from([eps[0]["inst"]]), 2, variant)
    cap = b.decode_capacity()
    lib, ptr, st = b._lib, _capi.ptr, b._stream()
    plan = torch.full((2, 3, cap, 3), -1, dtype=torch.int32, device="cuda")
    obj = torch.zeros(2, 3, 2, dtype=torch.int64, device="cuda")
    status = torch.zeros(2, 3, dtype=torch.int32, device="cuda")
    ins = torch.zeros(2, 3, dtype=torch.int32, device="cuda")
    call = lambda h, pl, qp, nc, o, stt, i=None: lib.fjsp_schedule_decode_active(h, pl, qp, None, nc, o, stt, None, None, i, st)
    assert call(None, ptr(plan), 1, 3, ptr(obj), ptr(status)) == _capi.FJSP_E_ARG
    assert call(b._h, None, 1, 3, ptr(obj), ptr(status)) == _capi.FJSP_E_ARG
    assert call(b._h, ptr(plan), 1, 3, None, ptr(status)) == _capi.FJSP_E_ARG
    assert call(b._h, ptr(plan), 1, 3, ptr(obj), None) == _capi.FJSP_E_ARG
    assert call(b._h, ptr(plan), 1, 0, ptr(obj), ptr(status)) == _capi.FJSP_E_ARG
    assert call(b._h, ptr(plan), 2, 3, ptr(obj), ptr(status)) == _capi.FJSP_E_ARG
    assert call(b._h, ptr(plan), 0, 3, ptr(obj), ptr(status)) == _capi.FJSP_E_ARG
    assert call(b._h, ptr(plan), 3, 3, ptr(obj), ptr(status)) == 0 and call(b._h, ptr(plan), 1, 3, ptr(obj), ptr(status), ptr(ins)) == 0
    assert bool((status == 2).all()) and bool((ins == 0).all()) and bool((obj == -1).all())          # empty plans
    with pytest.raises(ValueError):
        b.decode_active(plan[:, 0, :-1])
    with pytest.raises(ValueError):
        b.decode_active(plan, n_cand=2)
    with pytest.raises(ValueError):
        b.decode_active(plan[:, 0], moves=torch.zeros(2, 2, 3, dtype=torch.int32), n_cand=3)
    with pytest.raises(ValueError):
        b.decode_active(plan[:, 0], n_cand=0)
    # MO_DFJSP: an insertion under breakdown shifts is not defined
    dvariant, deps = suites["mo_dfjsp"]
    dyn = _batch(H.instance_set_from([deps[0]["inst"]]), 1, dvariant)
    assert dyn.decode_active_group() == 0 and dyn.decode_active_resident() == 0
    empty = torch.full((1, dyn.decode_capacity(), 3), -1, dtype=torch.int32)
    with pytest.raises(_capi.FjspError) as err:
        dyn.decode_active(empty)
    assert err.value.code == _capi.FJSP_E_UNSUPPORTED and "fjsp_schedule_decode_active:" in str(err.value)
    with pytest.raises(_capi.FjspError) as err:
        ps.left_shift(dyn, empty)
    assert err.value.code == _capi.FJSP_E_UNSUPPORTED
    # 1040 jobs: 5 bytes a job is more than 5120 bytes a candidate, as for decode
    big = _batch(_instances([([1], [1040], 1)]), 1)
    assert big.decode_active_group() == 0
    with pytest.raises(_capi.FjspError) as err:
        big.decode_active(torch.full((1, 1040, 3), -1, dtype=torch.int32))
    assert err.value.code == _capi.FJSP_E_UNSUPPORTED
