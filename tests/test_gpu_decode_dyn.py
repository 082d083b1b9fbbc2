"""GPU: fjsp_schedule_decode_dyn (schedule.decode_dyn) against tests/decode_dyn_reference.py bit for bit -- objectives with
the energy, status, tables and lengths, with and without a table -- on the reference's own MO_DFJSP schedules, random
plans, every move, the hand-made window cases, every status code, every workgroup size and the state limit, the refusals,
the round trip of live recordings, and policy_search.improve on a MO_DFJSP batch."""
import numpy as np
import pytest

from tests import critical_reference as R
from tests import decode_dyn_reference as DD
from tests import decode_reference as D
from tests import helpers as H
from tests import schedule_fixture as F

pytestmark = pytest.mark.gpu

KEYS = DD.KEYS
VARIANT = DD.VARIANT


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def eps():
    variant, eps = F.load()["mo_dfjsp"]
    assert variant == VARIANT
    return eps


def _solved(arrs):
    """An InstanceSet of hand-made MO_DFJSP shops (tests/decode_dyn_reference.py shop), fluid LPs solved here."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    s = fi.InstanceSet(len(arrs))
    for i, a in enumerate(arrs):
        s.set_raw(i, a.Jr, a.p, a.elig_n, a.elig_list, a.count, a.arrive, a.delivery, a.ddt)
        s.set_dynamic(i, a.power, a.idle_power, a.bk_n, a.bk)
    return s.solve_fluid()


def _random_shop(rs, Jr, jobs, M, windows=3):
    """Jr[R] stages, jobs[R] jobs per kind, one order at 0: p in 1..20 on a random eligible set that leaves no operation
    and no machine empty, power 1..50, idle power 1..9, up to `windows` disjoint windows per machine in time order."""
    K = int(np.sum(Jr))
    p = rs.randint(1, 21, (K, M)) * (rs.rand(K, M) < 0.6)
    for k in range(K):
        if not p[k].any():
            p[k, rs.randint(M)] = rs.randint(1, 21)
    for m in range(M):
        if not p[:, m].any():
            p[rs.randint(K), m] = rs.randint(1, 21)
    win = []
    for m in range(M):
        t, w = 0, []
        for _ in range(rs.randint(0, windows + 1)):
            t += int(rs.randint(1, 40))
            w.append((t, t + int(rs.randint(1, 15))))
            t = w[-1][1]
        win.append(w)
    return DD.shop(p, rs.randint(1, 51, (K, M)) * (p > 0), rs.randint(1, 10, M), win, Jr=Jr, count=[list(jobs)], delivery=(int(p.max()) * 3,))


def _batch(s, N):
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    return EnvBatch(s, N, variant=VARIANT)


def _random_moves(rs, plans, n_cand, M):
    """int32[N][n_cand][3]: kinds 0, 1, 2, 4 at rows inside the plan, machines 0 .. M (eligible, ineligible, out of range)."""
    N = len(plans)
    L = np.array([D.plan_length(pl) for pl in plans])
    mv = np.zeros((N, n_cand, 3), np.int32)
    mv[..., 0] = rs.choice([0, 1, 2, 4], (N, n_cand))
    mv[..., 1] = (rs.rand(N, n_cand) * np.maximum(L, 1)[:, None]).astype(np.int32)
    mv[..., 2] = rs.randint(0, M + 1, (N, n_cand))
    pair = mv[..., 0] == 4
    dv = rs.randint(1, 6, (N, n_cand))
    dw = (rs.rand(N, n_cand) * dv).astype(np.int32)
    mv[..., 2] = np.where(pair, dv | (dw << 16), mv[..., 2])                  # (some reach past the plan: status 4)
    return mv


def _compare(torch, b, insts, plan, moves, n_cand, what):
    pl = torch.from_numpy(np.ascontiguousarray(plan))
    mv = None if moves is None else torch.from_numpy(np.ascontiguousarray(moves))
    got = b.decode_dyn(pl, mv, n_cand, want_table=True)
    want = DD.decode(insts, plan, moves, n_cand)
    assert tuple(got["objective"].shape) == (len(insts), n_cand, 3)
    for key in KEYS:
        assert np.array_equal(got[key].cpu().numpy(), want[key]), (what, key)
    lean = b.decode_dyn(pl, mv, n_cand)
    assert lean["table"] is None
    for key in ("objective", "status", "length"):
        assert np.array_equal(lean[key].cpu().numpy(), want[key]), (what, key, "without a table")
    return want


def test_the_reference_schedules_in_one_batch(torch_gpu, eps):
    """The 9 reference-recorded MO_DFJSP schedules, env i on episode i's instance: plans of 8 to 1 157 rows (padding rows),
    1 to 5 orders, up to 63 windows.  The kernel returns the reference's tables."""
    insts = [ep["inst"] for ep in eps]
    b = _batch(H.instance_set_from(insts), len(eps))
    cap = b.decode_capacity()
    assert cap == 1157 and min(len(ep["table"]) for ep in eps) == 8
    assert b.decode_dyn_group() > 0 and b.decode_group() == 0
    plan = np.stack([D.plan_from_table(ep["table"], cap) for ep in eps])
    want = _compare(torch_gpu, b, insts, plan, None, 1, "reference schedules")
    assert np.all(want["status"] == 0)
    for i, ep in enumerate(eps):
        assert np.array_equal(want["table"][i, 0, :len(ep["table"])], ep["table"]), i


def test_the_smallest_shop(torch_gpu, eps):
    """gen8802 alone: 8 rows, 3 machines, 5 windows; random plans, N = 2, as parents with moves and per candidate."""
    a = eps[7]["inst"]
    assert a.name == "gen8802" and len(eps[7]["table"]) == 8 and a.M == 3 and int(np.sum(a.bk_n)) == 5
    b = _batch(H.instance_set_from([a]), 2)
    assert b.decode_capacity() == 8 and b.decode_dyn_group() == 256
    rs = np.random.RandomState(2)
    plan = np.stack([D.random_plan(a, rs, 8) for _ in range(2)])
    want = _compare(torch_gpu, b, [a, a], plan, None, 1, "gen8802")
    assert np.all(want["status"] == 0)
    per = np.stack([[D.random_plan(a, rs, 8) for _ in range(5)] for _ in range(2)])
    _compare(torch_gpu, b, [a, a], per, _random_moves(rs, per[:, 0], 5, a.M), 5, "gen8802 per candidate")


@pytest.mark.parametrize("n_cand", [3, 65])
def test_moves(torch_gpu, eps, n_cand):
    """Every move kind on the 76-row gen8801 shop (6 machines, 19 windows, 3 orders), on a shared parent and on per-candidate
    plans; among them a MOVE_MACHINE onto a machine with windows and one onto an ineligible machine."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    a = eps[6]["inst"]
    assert a.name == "gen8801"
    b = _batch(H.instance_set_from([a]), 2)
    cap = b.decode_capacity()
    rs = np.random.RandomState(n_cand)
    parent = np.stack([D.random_plan(a, rs, cap) for _ in range(2)])
    moves = _random_moves(rs, parent, n_cand, a.M)
    # row 0 is a first stage: onto an eligible machine with windows, and onto an ineligible one (or, if it has none, machine M)
    p0 = np.asarray(a.p)[np.concatenate(([0], np.cumsum(a.Jr)))[parent[0, 0, 0]]]
    with_windows = [m for m in np.flatnonzero(p0 > 0) if a.bk_n[m] > 0]
    assert with_windows
    bad = np.flatnonzero(p0 == 0)
    moves[0, 0] = (sch.MOVE_MACHINE, 0, with_windows[0])
    moves[0, 1] = (sch.MOVE_MACHINE, 0, bad[0] if len(bad) else a.M)
    moves[0, 2] = sch.pair_move(3, 9, 5)
    want = _compare(torch, b, [a, a], parent, moves, n_cand, "shared parent")
    assert want["status"][0, 0] == 0 and want["status"][0, 1] == 3 and want["status"][0, 2] == 0
    assert {0, 1, 2, 4} <= set(moves[..., 0].flatten().tolist())
    per = np.stack([[D.random_plan(a, rs, cap) for _ in range(n_cand)] for _ in range(2)])
    _compare(torch, b, [a, a], per, moves, n_cand, "per candidate")
    # a move equals the decode of its materialised plan
    made = sch.apply_moves(torch.from_numpy(parent).cuda(), torch.from_numpy(moves).cuda())
    assert np.array_equal(made.cpu().numpy(), np.stack([[R.materialise_moved(parent[i], moves[i, q]) for q in range(n_cand)] for i in range(2)]))
    again = b.decode_dyn(made, None, n_cand, want_table=True)
    valid = want["status"] != 4
    for key in KEYS:
        assert np.array_equal(again[key].cpu().numpy()[valid], want[key][valid]), key


def test_hand_made_cases_in_lane_0_63_and_mid_wave(torch_gpu):
    """The written answers of tests/decode_dyn_reference.py hand_cases, every case in lane 0, lane 63 and mid-wave: 72 envs
    on the cases' shops in rotation (env i on case (i + rot) % cases)."""
    cases = DD.hand_cases()
    C = len(cases)
    N = 72
    seen = set()
    for rot in range(C):
        order = [cases[(c + rot) % C] for c in range(C)]
        b = _batch(_solved([c[1] for c in order]), N)
        assert b.decode_dyn_group() == 256
        cap = b.decode_capacity()
        assert cap == 3
        plan = np.full((N, cap, 3), -1, np.int32)
        for i in range(N):
            rows = order[i % C][2]
            plan[i, :len(rows)] = rows
        insts = [order[i % C][1] for i in range(N)]
        want = _compare(torch_gpu, b, insts, plan, None, 1, rot)
        for i in range(N):
            name, _, rows, table, objective = order[i % C]
            assert want["status"][i, 0] == 0 and want["table"][i, 0, :len(rows)].tolist() == [list(r) for r in table], (name, i)
            assert tuple(want["objective"][i, 0].tolist()) == objective, (name, i)
            seen.add((name, "mid" if 0 < i < 63 else i))
    for name in [c[0] for c in cases]:
        assert {(name, 0), (name, 63), (name, "mid")} <= seen


STATUS_CASES = [
    ("no kind", 1, lambda pl, L: pl.__setitem__((3, 0), 99), None),
    ("no job", 1, lambda pl, L: pl.__setitem__((L - 1, 1), 60000), None),
    ("negative kind", 1, lambda pl, L: pl.__setitem__((0, 0), -1), None),
    ("too many rows", 2, lambda pl, L: pl.__setitem__((L - 1, slice(None)), pl[0].copy()), None),
    ("operations missing", 2, lambda pl, L: pl.__setitem__((L - 1, slice(None)), -1), None),
    ("empty plan", 2, lambda pl, L: pl.__setitem__((slice(None), slice(None)), -1), None),
    ("machine out of range", 3, lambda pl, L: pl.__setitem__((2, 2), 6), None),
    ("machine negative", 3, lambda pl, L: pl.__setitem__((2, 2), -1), None),
    ("machine by move", 3, None, lambda L: (1, 0, 7)),
    ("unknown kind", 4, None, lambda L: (3, 0, 0)),
    ("u negative", 4, None, lambda L: (1, -1, 0)),
    ("u past the plan", 4, None, lambda L: (1, L, 0)),
    ("swap of the last row", 4, None, lambda L: (2, L - 1, 0)),
    ("pair past the plan", 4, None, lambda L: (4, L - 2, 2 | (1 << 16))),
    ("pair with dw >= dv", 4, None, lambda L: (4, 0, 2 | (2 << 16))),
    ("bad move on a bad plan", 4, lambda pl, L: pl.__setitem__((0, 0), 99), lambda L: (2, -5, 0)),
]


@pytest.fixture(scope="module")
def wave(torch_gpu, eps):
    """128 valid candidates of one gen8801 env (two waves), own plans, with their reference results."""
    a = eps[6]["inst"]
    b = _batch(H.instance_set_from([a]), 1)
    rs = np.random.RandomState(11)
    cap = b.decode_capacity()
    plan = np.stack([D.random_plan(a, rs, cap) for _ in range(128)])[None]
    moves = np.zeros((1, 128, 3), np.int32)
    want = DD.decode([a], plan, moves, 128)
    assert np.all(want["status"] == 0)
    return b, a, plan, moves, want


@pytest.mark.parametrize("name, code, spoil, move", STATUS_CASES, ids=[c[0] for c in STATUS_CASES])
def test_status_codes_in_lane_0_31_and_63(torch_gpu, wave, name, code, spoil, move):
    """The failed candidates get their code, three -1 objectives, length 0 and a table of -1; the valid candidates between
    and beside them (the second wave included) keep their results."""
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
        one = DD.decode_one(a, plan[0, lane], moves[0, lane])
        assert one["status"] == code and one["length"] == 0 and np.all(one["table"] == -1) and one["objective"].tolist() == [-1, -1, -1]
        for key in KEYS:
            want[key][0, lane] = one[key]
    got = b.decode_dyn(torch.from_numpy(plan), torch.from_numpy(moves), 128, want_table=True)
    for key in KEYS:
        assert np.array_equal(got[key].cpu().numpy(), want[key]), (name, key)


# (stages per kind, jobs per kind, machines) -> candidates per workgroup; bytes per candidate = 5 x jobs rounded up to 16 + 8 M
GROUPS = [(([2, 1], [3, 4], 3), 256),             # 16 jobs:   104 bytes
          (([2] * 4, [16] * 4, 5), 128),          # 64 jobs:   360
          (([1] * 6, [50] * 6, 8), 64),           # 304 jobs: 1584 (beyond 64 KB of LDS for 64 candidates: one workgroup to a CU)
          (([1] * 12, [50] * 12, 20), 32),        # 608 jobs: 3200
          (([1], [1008], 10), 32)]                # 1008 jobs: 5040 + 80 = 5120, the limit


@pytest.mark.parametrize("spec, group", GROUPS, ids=["256", "128", "64", "32", "limit"])
def test_every_workgroup_size_and_the_state_limit(torch_gpu, spec, group):
    rs = np.random.RandomState(group + spec[2])
    a = _random_shop(rs, *spec)
    b = _batch(_solved([a]), 1)
    jobs16 = (sum(spec[1]) + 15) // 16 * 16
    assert 5 * jobs16 + 8 * spec[2] <= 5120 and b.decode_dyn_group() == group
    cap = b.decode_capacity()
    parent = D.random_plan(a, rs, cap)[None]
    for count in ((group - 1, group + 1) if group > 64 else (group + 1,)):
        moves = _random_moves(rs, np.repeat(parent, count, 0), 1, a.M).reshape(1, count, 3)
        _compare(torch_gpu, b, [a], parent, moves, count, (group, count))


def test_refusals(torch_gpu, eps):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    torch = torch_gpu
    # a job over the limit: 1009 jobs round up to 1024: 5120 + 80 bytes
    rs = np.random.RandomState(5)
    big = _batch(_solved([_random_shop(rs, [1], [1009], 10)]), 1)
    assert big.decode_dyn_group() == 0 and big.decode_capacity() == 1009
    with pytest.raises(_capi.FjspError) as err:
        big.decode_dyn(torch.full((1, 1009, 3), -1, dtype=torch.int32))
    assert err.value.code == _capi.FJSP_E_UNSUPPORTED and "5200" in str(err.value)
    # another variant: refused, with a pointer at the entry that decodes it
    mk01 = F.load()["mk01"][1][0]["inst"]
    so = EnvBatch(H.instance_set_from([mk01]), 1)
    assert so.decode_dyn_group() == 0 and so.decode_group() > 0
    with pytest.raises(_capi.FjspError) as err:
        so.decode_dyn(torch.full((1, so.decode_capacity(), 3), -1, dtype=torch.int32))
    assert err.value.code == _capi.FJSP_E_UNSUPPORTED and "fjsp_schedule_decode " in str(err.value) + " "
    # the arguments
    a = eps[7]["inst"]
    b = _batch(H.instance_set_from([a]), 2)
    cap = b.decode_capacity()
    lib, ptr, st = b._lib, _capi.ptr, b._stream()
    plan = torch.full((2, 3, cap, 3), -1, dtype=torch.int32, device="cuda")
    obj = torch.zeros(2, 3, 3, dtype=torch.int64, device="cuda")
    status = torch.zeros(2, 3, dtype=torch.int32, device="cuda")
    call = lambda h, pl, qp, nc, o, stt: lib.fjsp_schedule_decode_dyn(h, pl, qp, None, nc, o, stt, None, None, st)
    assert call(None, ptr(plan), 1, 3, ptr(obj), ptr(status)) == _capi.FJSP_E_ARG
    assert call(b._h, None, 1, 3, ptr(obj), ptr(status)) == _capi.FJSP_E_ARG
    assert call(b._h, ptr(plan), 1, 3, None, ptr(status)) == _capi.FJSP_E_ARG
    assert call(b._h, ptr(plan), 1, 3, ptr(obj), None) == _capi.FJSP_E_ARG
    assert call(b._h, ptr(plan), 1, 0, ptr(obj), ptr(status)) == _capi.FJSP_E_ARG
    assert call(b._h, ptr(plan), 2, 3, ptr(obj), ptr(status)) == _capi.FJSP_E_ARG
    assert call(b._h, ptr(plan), 3, 3, ptr(obj), ptr(status)) == 0 and call(b._h, ptr(plan), 1, 3, ptr(obj), ptr(status)) == 0
    with pytest.raises(ValueError):
        b.decode_dyn(plan[:, 0, :-1])
    with pytest.raises(ValueError):
        b.decode_dyn(plan, n_cand=2)


def test_live_recording_round_trip(torch_gpu, eps):
    """Single-order MO_DFJSP envs play the golden episodes' actions with recording on: decoding the recorded sequence and
    machines returns the recorded table, and the decoded objectives are the env's, the energy included."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    torch = torch_gpu
    played = 0
    for ep in eps:
        a = ep["inst"]
        if a.S != 1:
            continue
        b = EnvBatch(H.instance_set_from([a]), 1, rng_seed=ep["rng_seed"], variant=VARIANT)
        assert b.record_schedule() == b.decode_capacity()
        b.reset()
        b.rollout(torch.from_numpy(np.ascontiguousarray(ep["actions"][:, None, :])).cuda(),
                  mo=torch.from_numpy(np.maximum(ep["mo"], 0.0)[None, :]).cuda())
        table, length = b.schedule()
        fin = b.read()
        assert bool((fin["done"] != 0).all()) and np.array_equal(table[0, :len(ep["table"])].cpu().numpy(), ep["table"])
        got = b.decode_dyn(sch.plan_of(table), want_table=True)
        assert bool((got["status"] == 0).all())
        assert torch.equal(got["table"][:, 0], table) and torch.equal(got["length"][:, 0], length)
        assert torch.equal(got["objective"][:, 0, 0], fin["completion_time"].to(torch.int64))
        assert torch.equal(got["objective"][:, 0, 1], fin["delay_time_sum"].to(torch.int64))
        assert torch.equal(got["objective"][:, 0, 2], fin["energy_consumption"].to(torch.int64))
        assert b.schedule()[0].equal(table)                               # decoding touched no env
        played += 1
        last = a, table, got
    assert played == 3
    # a Batched* wrapper is taken like its batch
    from deep_reinforcement_learning_for_fjsp_amd.environments import BatchedMODFJSP
    a, table, got = last
    env = BatchedMODFJSP(H.instance_set_from([a]), n_envs=1)
    assert torch.equal(sch.decode_dyn(env, sch.plan_of(table))["objective"], got["objective"])


def test_improve_on_a_mo_dfjsp_batch(torch_gpu, eps):
    """policy_search.improve on gen8801 (76 rows), 20 rounds x 64 neighbours per objective: the history never rises, the
    returned plan decodes to the returned objective (three columns), energy is an objective, critical paths are refused."""
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as ps
    torch = torch_gpu
    a = eps[6]["inst"]
    N = 4
    b = _batch(H.instance_set_from([a]), N)
    cap = b.decode_capacity()
    assert cap == 76
    rs = np.random.RandomState(3)
    plan = torch.from_numpy(np.stack([D.random_plan(a, rs, cap) for _ in range(N)])).cuda()
    for col, objective in enumerate(("makespan", "tardiness", "energy")):
        res = ps.improve(b, plan, 20, 64, objective=objective, seed=col)
        hist = res["history"].cpu().numpy()
        assert hist.shape == (21, N) and np.all(np.diff(hist, axis=0) <= 0), objective
        assert tuple(res["objective"].shape) == (N, 3)
        want = DD.decode([a] * N, res["plan"].cpu().numpy())
        assert np.all(want["status"] == 0)
        assert np.array_equal(res["objective"].cpu().numpy(), want["objective"][:, 0]), objective
        assert np.array_equal(res["table"].cpu().numpy(), want["table"][:, 0])
        assert np.array_equal(hist[-1], want["objective"][:, 0, col]) and np.array_equal(hist[0], DD.decode([a] * N, plan.cpu().numpy())["objective"][:, 0, col])
        assert np.any(hist[-1] < hist[0]), objective                      # (20 x 64 neighbours of a random plan do find a better one)
    for nb in ("critical", "mixed"):
        with pytest.raises(ValueError):
            ps.improve(b, plan, 1, 8, neighbourhood=nb)
    with pytest.raises(ValueError):
        ps.improve(b, plan, 1, 8, objective="power")
