"""GPU: fjsp_schedule_decode (schedule.decode) against tests/decode_reference.py bit for bit -- objectives, status, tables
and lengths -- on the reference's own schedules, random plans, every workgroup size the launcher chooses and the candidate
counts around them, every move, every status code, the refusals, and the round trip of a live recording."""
import numpy as np
import pytest

from tests import decode_reference as D
from tests import helpers as H
from tests import schedule_fixture as F

pytestmark = pytest.mark.gpu

SINGLE = ("mk01", "synth10x5", "multijob", "so_sfjsp", "mo_discretes")
ORDERS = ("multiorder", "so_dfjsp")
KEYS = ("objective", "status", "table", "length")


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


def _random_moves(rs, plans, n_cand):
    """int32[N][n_cand][3]: kinds 0, 1, 2 at rows inside the plan, machines 0 .. 5 (some ineligible, some out of range)."""
    N = len(plans)
    L = np.array([D.plan_length(pl) for pl in plans])
    mv = np.zeros((N, n_cand, 3), np.int32)
    mv[..., 0] = rs.randint(0, 3, (N, n_cand))
    mv[..., 1] = (rs.rand(N, n_cand) * np.maximum(L, 1)[:, None]).astype(np.int32)
    mv[..., 2] = rs.randint(0, 6, (N, n_cand))
    return mv


def _compare(torch, b, insts, variant, plan, moves, n_cand, what):
    got = b.decode(torch.from_numpy(np.ascontiguousarray(plan)), None if moves is None else torch.from_numpy(moves), n_cand, want_table=True)
    want = D.decode(insts, variant, plan, moves, n_cand)
    for key in KEYS:
        assert np.array_equal(got[key].cpu().numpy(), want[key]), (what, key)
    lean = b.decode(torch.from_numpy(np.ascontiguousarray(plan)), None if moves is None else torch.from_numpy(moves), n_cand)
    assert lean["table"] is None
    for key in ("objective", "status", "length"):
        assert np.array_equal(lean[key].cpu().numpy(), want[key]), (what, key, "without a table")
    return want


@pytest.mark.parametrize("suite", SINGLE + ORDERS)
def test_golden_plans(torch_gpu, suites, suite):
    """Every episode of the suite in one batch, env i on episode i's instance (plans of different lengths: padding rows).
    The single-order suites also give back the reference's table itself."""
    variant, eps = suites[suite]
    insts = [ep["inst"] for ep in eps]
    b = _batch(H.instance_set_from(insts), len(eps), variant)
    cap = b.decode_capacity()
    assert cap == max(len(ep["table"]) for ep in eps)
    plan = np.stack([D.plan_from_table(ep["table"], cap) for ep in eps])
    want = _compare(torch_gpu, b, insts, variant, plan, None, 1, suite)
    assert np.all(want["status"] == 0)
    if suite in SINGLE:
        for i, ep in enumerate(eps):
            assert np.array_equal(want["table"][i, 0, :len(ep["table"])], ep["table"]), (suite, i)
    # ... and as the candidates of shared parents, each with a move
    rs = np.random.RandomState(len(eps))
    _compare(torch_gpu, b, insts, variant, plan, _random_moves(rs, plan, 3), 3, suite + " moved")


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


@pytest.fixture(scope="module")
def synth(torch_gpu):
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    s = fi.InstanceSet(1).generate_range(4000, fi.bench_10x5_params()).solve_fluid()
    return s, s.arrays(0)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257, 513])
def test_candidate_counts_around_waves_and_workgroups(torch_gpu, synth, count):
    """10 x 5 instances decode 256 candidates per workgroup: one wave +- 1, one workgroup +- 1, two workgroups + 1, as the
    candidates of one env (shared and own plans) and as envs of one candidate."""
    s, a = synth
    rs = np.random.RandomState(count)
    b = _batch(s, 1)
    assert b.decode_group() == 256
    cap = b.decode_capacity()
    per = np.stack([D.random_plan(a, rs, cap) for _ in range(count)])[None]
    moves = _random_moves(rs, np.repeat(per[:, 0], count, 0), 1).reshape(1, count, 3)
    _compare(torch_gpu, b, [a], 0, per[:, 0], moves, count, (count, "shared"))
    _compare(torch_gpu, b, [a], 0, per, moves, count, (count, "own"))
    if count > 1:
        _compare(torch_gpu, _batch(s, count), [a] * count, 0, per[0], None, 1, (count, "envs"))


@pytest.mark.parametrize("spec, group", [(([2] * 4, [16] * 4, 5), 128), (([2] * 6, [50] * 6, 8), 64), (([2] * 12, [50] * 12, 20), 32)])
def test_every_workgroup_size(torch_gpu, spec, group):
    """The launcher's other workgroups: 64 jobs (128 candidates), 300 jobs (64, beyond 64 KB of LDS) and the largest shop of
    the reference's training distribution, 12 kinds x 50 jobs on 20 machines (32, the upper half of the wave idle)."""
    s = _instances([spec], seed=group)
    a = s.arrays(0)
    b = _batch(s, 1)
    assert b.decode_group() == group
    rs = np.random.RandomState(group)
    cap = b.decode_capacity()
    parent = D.random_plan(a, rs, cap)[None]
    for count in ((group - 1, group + 1, 2 * group + 1) if group > 32 else (group + 1,)):
        moves = _random_moves(rs, np.repeat(parent, count, 0), 1).reshape(1, count, 3)
        moves[..., 2] = rs.randint(0, spec[2] + 1, (1, count))
        _compare(torch_gpu, b, [a], 0, parent, moves, count, (group, count))


def test_moves_equal_the_decode_of_the_materialised_plan(torch_gpu, suites):
    """Each kind at u = 0, L - 2, L - 1, a swap inside one job, a reassignment to the machine the row has."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    a = suites["mk01"][1][0]["inst"]
    b = _batch(H.instance_set_from([a]), 2)
    cap = b.decode_capacity()
    rs = np.random.RandomState(7)
    p, koff = np.asarray(a.p), np.concatenate(([0], np.cumsum(a.Jr)))
    mixed = D.random_plan(a, rs, cap)
    # job after job: every neighbouring pair inside a job is a swap that changes nothing
    by_job = np.array(sorted(mixed.tolist(), key=lambda row: (row[0], row[1])), np.int32)
    plan = np.stack([mixed, by_job])
    L = D.plan_length(mixed)
    assert L == cap and D.plan_length(by_job) == L
    stage_of = lambda pl, u: int(np.sum((pl[:u, 0] == pl[u, 0]) & (pl[:u, 1] == pl[u, 1])))
    moves = []
    for pl in plan:
        mv = [(0, 0, 0)]
        for u in (0, L - 2, L - 1):
            elig = np.flatnonzero(p[koff[pl[u, 0]] + stage_of(pl, u)] > 0)
            mv += [(1, u, int(elig[-1])), (1, u, int(pl[u, 2])), (2, u, 0)]
        moves.append(mv)
    moves = np.array(moves, np.int32)
    Q = moves.shape[1]
    assert by_job[0, 0] == by_job[1, 0] and by_job[0, 1] == by_job[1, 1]              # (2, 0, 0) on by_job: one job
    want = _compare(torch, b, [a, a], 0, plan, moves, Q, "moves")
    valid = ~((moves[..., 0] == 2) & (moves[..., 1] == L - 1))
    assert np.all(want["status"][valid] == 0) and np.all(want["status"][~valid] == 4) and (~valid).sum() == 2
    made = sch.apply_moves(torch.from_numpy(plan).cuda(), torch.from_numpy(moves).cuda())
    assert np.array_equal(made.cpu().numpy(), np.stack([[D.materialise(plan[i], moves[i, q]) for q in range(Q)] for i in range(2)]))
    again = b.decode(made, None, Q, want_table=True)
    for key in KEYS:
        assert np.array_equal(again[key].cpu().numpy()[valid], want[key][valid]), key
    same = np.flatnonzero((moves[1, :, 0] == 2) & (moves[1, :, 1] == 0))[0]
    assert np.array_equal(want["table"][1, same], want["table"][1, 0])


STATUS_CASES = [
    ("no kind", 1, lambda pl, L: pl.__setitem__((3, 0), 99), None),
    ("no job", 1, lambda pl, L: pl.__setitem__((L - 1, 1), 1), None),
    ("negative kind", 1, lambda pl, L: pl.__setitem__((0, 0), -1), None),
    ("too many rows", 2, lambda pl, L: pl.__setitem__((L - 1, slice(None)), pl[0].copy()), None),
    ("operations missing", 2, lambda pl, L: pl.__setitem__((L - 1, slice(None)), -1), None),
    ("empty plan", 2, lambda pl, L: pl.__setitem__((slice(None), slice(None)), -1), None),
    ("machine out of range", 3, lambda pl, L: pl.__setitem__((2, 2), 5), None),
    ("machine negative", 3, lambda pl, L: pl.__setitem__((2, 2), -1), None),
    ("machine by move", 3, None, lambda L: (1, 0, 7)),
    ("unknown kind", 4, None, lambda L: (3, 0, 0)),
    ("negative move kind", 4, None, lambda L: (-1, 0, 0)),
    ("u negative", 4, None, lambda L: (1, -1, 0)),
    ("u past the plan", 4, None, lambda L: (1, L, 0)),
    ("u far past the plan", 4, None, lambda L: (2, 1 << 30, 0)),
    ("u on the padding", 4, lambda pl, L: pl.__setitem__((L - 1, slice(None)), -1), lambda L: (1, L - 1, 0)),
    ("swap into the padding", 4, lambda pl, L: pl.__setitem__((L - 1, slice(None)), -1), lambda L: (2, L - 2, 0)),
    ("swap of the last row", 4, None, lambda L: (2, L - 1, 0)),
    ("bad move on a bad plan", 4, lambda pl, L: pl.__setitem__((0, 0), 99), lambda L: (2, -5, 0)),
]


@pytest.fixture(scope="module")
def wave(torch_gpu, synth):
    """128 valid candidates of one 10 x 5 env (two waves), own plans and moves, with their reference results."""
    s, a = synth
    b = _batch(s, 1)
    rs = np.random.RandomState(11)
    cap = b.decode_capacity()
    plan = np.stack([D.random_plan(a, rs, cap) for _ in range(128)])[None]
    moves = np.zeros((1, 128, 3), np.int32)
    want = D.decode([a], 0, plan, moves, 128)
    assert np.all(want["status"] == 0)
    return b, a, plan, moves, want


@pytest.mark.parametrize("name, code, spoil, move", STATUS_CASES, ids=[c[0] for c in STATUS_CASES])
def test_status_codes_in_lane_0_63_and_mid_wave(torch_gpu, wave, name, code, spoil, move):
    """The failed candidates get their code, -1 objectives, length 0 and a table of -1; the valid candidates between and
    beside them (the second wave included) keep their results."""
    torch = torch_gpu
    b, a, plan, moves, base = wave
    plan, moves = plan.copy(), moves.copy()
    want = {k: v.copy() for k, v in base.items()}
    for lane in (0, 31, 63):
        L = D.plan_length(plan[0, lane])
        if spoil is not None:
            spoil(plan[0, lane], L)
        if move is not None:
            moves[0, lane] = move(L)
        one = D.decode_one(a, 0, plan[0, lane], moves[0, lane])
        assert one["status"] == code and one["length"] == 0 and np.all(one["table"] == -1) and one["objective"].tolist() == [-1, -1]
        for key in KEYS:
            want[key][0, lane] = one[key]
    got = b.decode(torch.from_numpy(plan), torch.from_numpy(moves), 128, want_table=True)
    for key in KEYS:
        assert np.array_equal(got[key].cpu().numpy(), want[key]), (name, key)


def test_refusals(torch_gpu, suites, synth):
    import ctypes as C
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    torch = torch_gpu
    s, a = synth
    b = _batch(s, 2)
    cap = b.decode_capacity()
    lib, ptr, st = b._lib, _capi.ptr, b._stream()
    plan = torch.full((2, 3, cap, 3), -1, dtype=torch.int32, device="cuda")
    obj = torch.zeros(2, 3, 2, dtype=torch.int64, device="cuda")
    status = torch.zeros(2, 3, dtype=torch.int32, device="cuda")
    call = lambda h, pl, qp, nc, o, stt: lib.fjsp_schedule_decode(h, pl, qp, None, nc, o, stt, None, None, st)
    assert call(None, ptr(plan), 1, 3, ptr(obj), ptr(status)) == _capi.FJSP_E_ARG
    assert call(b._h, None, 1, 3, ptr(obj), ptr(status)) == _capi.FJSP_E_ARG
    assert call(b._h, ptr(plan), 1, 3, None, ptr(status)) == _capi.FJSP_E_ARG
    assert call(b._h, ptr(plan), 1, 3, ptr(obj), None) == _capi.FJSP_E_ARG
    assert call(b._h, ptr(plan), 1, 0, ptr(obj), ptr(status)) == _capi.FJSP_E_ARG
    assert call(b._h, ptr(plan), 2, 3, ptr(obj), ptr(status)) == _capi.FJSP_E_ARG
    assert call(b._h, ptr(plan), 0, 3, ptr(obj), ptr(status)) == _capi.FJSP_E_ARG
    assert call(b._h, ptr(plan), 3, 3, ptr(obj), ptr(status)) == 0 and call(b._h, ptr(plan), 1, 3, ptr(obj), ptr(status)) == 0
    assert lib.fjsp_schedule_decode_capacity(b._h) == cap == int((np.asarray(a.count) * np.asarray(a.Jr)[None, :]).sum())
    with pytest.raises(ValueError):
        b.decode(plan[:, 0, :-1])
    with pytest.raises(ValueError):
        b.decode(plan, n_cand=2)
    with pytest.raises(ValueError):
        b.decode(plan[:, 0], moves=torch.zeros(2, 2, 3, dtype=torch.int32), n_cand=3)
    with pytest.raises(ValueError):
        b.decode(plan[:, 0], n_cand=0)
    # MO_DFJSP: breakdown shifts and energy are not decoded
    variant, eps = suites["mo_dfjsp"]
    dyn = _batch(H.instance_set_from([eps[0]["inst"]]), 1, variant)
    assert dyn.decode_group() == 0 and dyn.decode_capacity() > 0
    with pytest.raises(_capi.FjspError) as err:
        dyn.decode(torch.full((1, dyn.decode_capacity(), 3), -1, dtype=torch.int32))
    assert err.value.code == _capi.FJSP_E_UNSUPPORTED
    # 1040 jobs: 5 bytes a job is more than 5120 bytes a candidate
    big = _batch(_instances([([1], [1040], 1)]), 1)
    assert big.decode_group() == 0 and big.decode_capacity() == 1040
    with pytest.raises(_capi.FjspError) as err:
        big.decode(torch.full((1, 1040, 3), -1, dtype=torch.int32))
    assert err.value.code == _capi.FJSP_E_UNSUPPORTED


def test_live_recording_round_trip(torch_gpu):
    """64 single-order envs play random rule pairs with recording on; decoding the recorded sequence and machines returns
    the recorded table: the environments' schedules are semi-active."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, global_actions
    torch = torch_gpu
    NI, N = 8, 64
    s = fi.InstanceSet(NI).generate_range(4100, fi.bench_10x5_params()).solve_fluid()
    b = EnvBatch(s, N, rng_seed=3)
    T = b.record_schedule()
    assert T == b.decode_capacity()
    acts = torch.from_numpy(global_actions(17, 0, N, T, 6, 5)).cuda()
    b.reset()
    for t in range(T):
        b.step(acts[t])
    table, length = b.schedule()
    assert bool((b.done != 0).all())
    got = b.decode(sch.plan_of(table), want_table=True)
    assert bool((got["status"] == 0).all())
    assert torch.equal(got["table"][:, 0], table) and torch.equal(got["length"][:, 0], length)
    fin = b.read()
    assert torch.equal(got["objective"][:, 0, 0], fin["makespan"].to(torch.int64))
    assert torch.equal(got["objective"][:, 0, 1], fin["delay_time_sum"].to(torch.int64))
    assert b.schedule()[0].equal(table)                                   # decoding touched no env
    # a Batched* wrapper of the same instances is taken like its batch
    from deep_reinforcement_learning_for_fjsp_amd.environments import BatchedSOFJSSP
    env = BatchedSOFJSSP(s, n_envs=N, rng_seed=3)
    assert torch.equal(sch.decode(env, sch.plan_of(table))["objective"], got["objective"])
