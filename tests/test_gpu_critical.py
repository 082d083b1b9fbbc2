"""GPU: fjsp_schedule_critical (schedule.critical) against tests/critical_reference.py bit for bit -- tails, flags, paths,
moves, counts, status and makespan -- on hand-made tables, the smallest shops, the golden suites, every workgroup size and
the table counts around them, every max_moves edge, every status code and range check and the refusals; and the decoder's
MOVE_PAIR against the decode of the materialised plan."""
import numpy as np
import pytest

from tests import critical_cases as K
from tests import critical_reference as R
from tests import decode_reference as D
from tests import helpers as H
from tests import schedule_fixture as F

pytestmark = pytest.mark.gpu

SUITES = ("mk01", "synth10x5", "multijob", "multiorder", "so_dfjsp", "so_sfjsp", "mo_discretes")
DKEYS = ("objective", "status", "table", "length")


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def suites():
    return F.load()


def _random_shops(specs, seed=1):
    """(Jr, p, jobs) per spec (Jr, jobs per kind, M): p uniform in 1..20 on a random non-empty eligible set."""
    rs = np.random.RandomState(seed)
    out = []
    for Jr, jobs, M in specs:
        k = int(np.sum(Jr))
        p = rs.randint(1, 21, (k, M)) * (rs.rand(k, M) < 0.6)
        for i in range(k):
            if not p[i].any():
                p[i, rs.randint(M)] = rs.randint(1, 21)
        out.append((Jr, p, jobs))
    return K.instance_set(out)


def _batch(s, N, variant=0):
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    return EnvBatch(s, N, variant=variant)


def _decoded(a, variant, plan, cap):
    one = D.decode_one(a, variant, plan, None, cap)
    assert one["status"] == 0
    return one["table"]


def _compare(torch, b, insts, tables, n_cand, max_moves, what, want=None):
    """critical on the device against the reference; tables int32[N][n_cand][cap][6].  Returns the reference's answer."""
    got = b.critical(torch.from_numpy(np.ascontiguousarray(tables)), n_cand, max_moves)
    want = R.critical(insts, tables, n_cand, max_moves) if want is None else want
    for key in R.KEYS:
        g = got[key].cpu().numpy()
        assert g.dtype == want[key].dtype and g.shape == want[key].shape, (what, key, g.dtype, g.shape, want[key].shape)
        assert np.array_equal(g, want[key]), (what, key)
    return want


def test_hand_made_tables(torch_gpu):
    """The tie, both-tight, both-predecessors, skipped-arc and idle tables: the reference's answers and the written ones."""
    names = sorted(K.HAND)
    a = K.hand_arrays()
    b = _batch(K.instance_set([(K.HAND_JR, K.HAND_P, K.HAND_JOBS)]), len(names))
    assert b.decode_capacity() == K.CAP
    tables = np.stack([K.table(K.HAND[n][0]) for n in names])[:, None]
    for max_moves in (0, 1, 2, 3, 4):
        want = _compare(torch_gpu, b, [a] * len(names), tables, 1, max_moves, ("hand", max_moves))
        for i, n in enumerate(names):
            written = K.hand_answer(n, max_moves)
            for key in R.KEYS:
                assert np.array_equal(want[key][i, 0], written[key]), (n, max_moves, key)


def test_smallest_shops(torch_gpu):
    """One job x one operation x one machine; an M = 1 shop; a one-job shop; and the three in one batch."""
    s = _random_shops([([1], [1], 1), ([2, 3], [2, 1], 1), ([4], [1], 3)])
    rs = np.random.RandomState(3)
    for ids in ([0], [1], [2], [0, 1, 2]):
        arrs = [s.arrays(i) for i in ids]
        N = 2 * len(ids)
        b = _batch(H.instance_set_from(arrs), N)
        insts = [arrs[i % len(ids)] for i in range(N)]
        cap = b.decode_capacity()
        tables = np.stack([[_decoded(a, 0, D.random_plan(a, rs, cap), cap) for _ in range(3)] for a in insts])
        want = _compare(torch_gpu, b, insts, tables, 3, 8, ids)
        assert np.all(want["status"] == 0)


@pytest.mark.parametrize("suite", SUITES)
def test_golden_suites(torch_gpu, suites, suite):
    """Every episode in one batch: its recorded plan's table as decoded and in begin order (schedule.begin_order, which
    the reference's statement confirms), plus two random plans' tables.  multiorder and so_dfjsp have paths that end
    at an order's arrival."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    variant, eps = suites[suite]
    insts = [ep["inst"] for ep in eps]
    b = _batch(H.instance_set_from(insts), len(eps), variant)
    cap = b.decode_capacity()
    assert suite != "multijob" or b.decode_group() == 64          # (its largest episode: beyond 64 KB of LDS at 128)
    rs = np.random.RandomState(len(suite))
    given = np.stack([_decoded(ep["inst"], variant, D.plan_from_table(ep["table"], cap), cap) for ep in eps])
    plan, ordered = sch.begin_order(torch.from_numpy(given).cuda())
    ordered = ordered.cpu().numpy()
    assert np.array_equal(ordered, np.stack([R.begin_order(t) for t in given]))
    assert np.array_equal(plan.cpu().numpy(), ordered[..., [0, 2, 3]])
    rand = [np.stack([_decoded(ep["inst"], variant, D.random_plan(ep["inst"], rs, cap), cap) for ep in eps]) for _ in range(2)]
    tables = np.stack([given, ordered] + rand, 1)
    want = _compare(torch, b, insts, tables, 4, 128, suite)
    assert np.all(want["status"] == 0) and np.all(want["skipped"][:, 1] == 0)
    if suite in ("multiorder", "so_dfjsp"):
        last = np.take_along_axis(want["path"], np.maximum(want["path_len"] - 1, 0)[..., None], -1)[..., 0]
        begins = np.take_along_axis(tables[..., 4], last[..., None], -1)[..., 0]
        assert (begins > 0).any(), "no path of this suite ends at an arrival"


@pytest.fixture(scope="module")
def synth(torch_gpu):
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    s = fi.InstanceSet(1).generate_range(4000, fi.bench_10x5_params()).solve_fluid()
    return s, s.arrays(0)


@pytest.mark.parametrize("count", [1, 63, 65, 257])
def test_table_counts_around_waves_and_workgroups(torch_gpu, synth, count):
    """10 x 5 instances take 256 tables per workgroup: tables of different random plans, as one env's and as envs of one."""
    s, a = synth
    rs = np.random.RandomState(count)
    b = _batch(s, 1)
    assert b.decode_group() == 256
    cap = b.decode_capacity()
    tables = np.stack([_decoded(a, 0, D.random_plan(a, rs, cap), cap) for _ in range(count)])
    _compare(torch_gpu, b, [a], tables[None], count, 16, (count, "tables of one env"))
    if count > 1:
        _compare(torch_gpu, _batch(s, count), [a] * count, tables[:, None], 1, 16, (count, "envs"))


@pytest.mark.parametrize("spec, group, count", [(([2] * 4, [16] * 4, 5), 128, 129), (([2] * 12, [50] * 12, 20), 32, 33)])
def test_other_workgroup_sizes(torch_gpu, spec, group, count):
    """The groups no golden suite takes (multijob: 64): 64 jobs (128 tables a workgroup) and the largest shop of the reference's training distribution, 12 kinds x 50 jobs on
    20 machines (32, the upper half of the wave idle): one table more than a workgroup takes, of three random plans."""
    s = _random_shops([spec], seed=group)
    a = s.arrays(0)
    b = _batch(s, 1)
    assert b.decode_group() == group
    rs = np.random.RandomState(group)
    cap = b.decode_capacity()
    some = [_decoded(a, 0, D.random_plan(a, rs, cap), cap) for _ in range(3)]
    some.append(R.begin_order(some[0]))
    pick = np.arange(count) % len(some)
    once = R.critical([a], np.stack(some)[None], len(some), 128)                # (the reference once per distinct table)
    assert np.all(once["status"] == 0) and once["skipped"][0, 3] == 0
    _compare(torch_gpu, b, [a], np.stack(some)[pick][None], count, 128, group, {key: v[:, pick] for key, v in once.items()})


def test_max_moves_edges(torch_gpu, suites):
    """max_moves 0 with a null pointer, 1, n_moves and n_moves + 1."""
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    torch = torch_gpu
    variant, eps = suites["mk01"]
    a = eps[0]["inst"]
    b = _batch(H.instance_set_from([a]), 1, variant)
    cap = b.decode_capacity()
    tables = R.begin_order(_decoded(a, variant, D.plan_from_table(eps[0]["table"], cap), cap))[None, None]
    n = int(R.critical([a], tables, 1, 0)["n_moves"][0, 0])
    assert n > 2
    for max_moves in (0, 1, n, n + 1):
        want = _compare(torch, b, [a], tables, 1, max_moves, ("max_moves", max_moves))
        assert want["n_moves"][0, 0] == n and want["moves"].shape == (1, 1, max_moves, 3)
    assert np.all(want["moves"][0, 0, :n, 0] != 0) and np.all(want["moves"][0, 0, n] == 0)
    # the raw call: null d_moves goes with max_moves = 0 only
    t = torch.from_numpy(tables).cuda()
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    tail, flags, path = i32(1, 1, cap), torch.zeros(1, 1, cap, dtype=torch.uint8, device="cuda"), i32(1, 1, cap)
    scal = [i32(1, 1) for _ in range(5)]
    ptr = _capi.ptr
    call = lambda h, tb, nc, mv, mm: b._lib.fjsp_schedule_critical(h, tb, nc, ptr(tail), ptr(flags), ptr(path), ptr(scal[0]), mv, mm,
                                                                 ptr(scal[1]), ptr(scal[2]), ptr(scal[3]), ptr(scal[4]), b._stream())
    assert call(b._h, ptr(t), 1, None, 0) == 0
    assert int(scal[1][0, 0]) == n and int(scal[3][0, 0]) == 0
    assert call(b._h, ptr(t), 1, None, 1) == _capi.FJSP_E_ARG
    assert call(b._h, ptr(t), 1, None, -1) == _capi.FJSP_E_ARG
    assert call(b._h, ptr(t), 0, None, 0) == _capi.FJSP_E_ARG
    assert call(None, ptr(t), 1, None, 0) == _capi.FJSP_E_ARG
    assert call(b._h, None, 1, None, 0) == _capi.FJSP_E_ARG
    with pytest.raises(ValueError):
        b.critical(t[:, :, :-1])
    with pytest.raises(ValueError):
        b.critical(t, n_cand=2)
    with pytest.raises(ValueError):
        b.critical(t, max_moves=-1)


def test_status_codes_and_range_checks(torch_gpu):
    """One table per range check and an empty one, each between valid tables of one wave: the failed tables get their
    code, -1 / 0 outputs and no moves, their neighbours keep their results."""
    names = sorted(K.BAD_ROWS)
    a = K.hand_arrays()
    b = _batch(K.instance_set([(K.HAND_JR, K.HAND_P, K.HAND_JOBS)]), 1)
    tables = [K.table(K.VALID)]
    for n in names:
        tables += [K.bad_table(n), K.table(K.HAND["both tight, machine later"][0])]
    tables += [K.table([]), K.table(K.VALID)]
    tables = np.stack(tables)[None]
    want = _compare(torch_gpu, b, [a], tables, tables.shape[1], 4, "status")
    codes = want["status"][0]
    assert codes[1:1 + 2 * len(names):2].tolist() == [1] * len(names) and codes[-2] == 2
    assert (codes != 0).sum() == len(names) + 1
    bad = codes != 0
    assert np.all(want["tail"][0, bad] == -1) and np.all(want["path"][0, bad] == -1) and np.all(want["makespan"][0, bad] == -1)
    for key in ("flags", "moves", "path_len", "n_moves", "skipped"):
        assert not want[key][0, bad].any(), key


def test_refusals(torch_gpu, suites):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    torch = torch_gpu
    variant, eps = suites["mo_dfjsp"]
    dyn = _batch(H.instance_set_from([eps[0]["inst"]]), 1, variant)
    with pytest.raises(_capi.FjspError) as err:
        dyn.critical(torch.full((1, dyn.decode_capacity(), 6), -1, dtype=torch.int32))
    assert err.value.code == _capi.FJSP_E_UNSUPPORTED
    big = _batch(_random_shops([([1], [1040], 1)]), 1)
    assert big.decode_group() == 0
    with pytest.raises(_capi.FjspError) as err:
        big.critical(torch.full((1, 1040, 6), -1, dtype=torch.int32))
    assert err.value.code == _capi.FJSP_E_UNSUPPORTED


# ---- MOVE_PAIR in fjsp_schedule_decode
def _compare_pairs(torch, b, insts, variant, plan, moves, n_cand, what):
    """decode with pair moves against the materialised plans' decode (shared parents plan[N][cap][3] or own
    [N][n_cand][cap][3]), and against schedule.apply_moves followed by a plain decode."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    got = b.decode(torch.from_numpy(np.ascontiguousarray(plan)), torch.from_numpy(moves), n_cand, want_table=True)
    cap = plan.shape[-2]
    parent = lambda i, q: plan[i] if plan.ndim == 3 else plan[i, q]
    ones = [[R.decode_moved(insts[i], variant, parent(i, q), moves[i, q], cap) for q in range(n_cand)] for i in range(len(insts))]
    for key in DKEYS:
        want = np.array([[one[key] for one in per] for per in ones])
        assert np.array_equal(got[key].cpu().numpy(), want), (what, key)
    made = sch.apply_moves(torch.from_numpy(np.ascontiguousarray(plan)).cuda(), torch.from_numpy(moves).cuda())
    want_made = np.stack([[R.materialise_moved(parent(i, q), moves[i, q]) for q in range(n_cand)] for i in range(len(insts))])
    for i in range(len(insts)):                          # (up to the plan's end: the reference drops rows behind a first -1 row)
        for q in range(n_cand):
            Lp = D.plan_length(parent(i, q))
            assert np.array_equal(made[i, q, :Lp + 1].cpu().numpy(), want_made[i, q, :Lp + 1]), (what, "apply_moves", i, q)
    again = b.decode(made, None, n_cand, want_table=True)
    ok = got["status"].cpu().numpy() == 0
    for key in DKEYS:
        assert np.array_equal(again[key].cpu().numpy()[ok], got[key].cpu().numpy()[ok]), (what, key, "materialised")
    return np.array([[one["status"] for one in per] for per in ones])


def _random_triples(rs, L, count):
    u = rs.randint(0, L - 1, count)
    v = np.array([rs.randint(x + 1, L) for x in u])
    w = np.array([rs.randint(x, y) for x, y in zip(u, v)])
    return np.stack([np.full(count, 4), u, (v - u) | ((w - u) << 16)], 1).astype(np.int32)


@pytest.mark.parametrize("suite", ("mk01", "synth10x5", "multiorder"))
def test_pair_moves_emitted_and_random(torch_gpu, suites, suite):
    """Every pair move critical emits on the begin-ordered recorded plans, and random valid (u, v, w), with shared and
    with per-candidate parents."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    torch = torch_gpu
    variant, eps = suites[suite]
    eps = eps[:4]
    insts = [ep["inst"] for ep in eps]
    b = _batch(H.instance_set_from(insts), len(eps), variant)
    cap = b.decode_capacity()
    rs = np.random.RandomState(5)
    tables = np.stack([R.begin_order(_decoded(ep["inst"], variant, D.plan_from_table(ep["table"], cap), cap)) for ep in eps])
    plan = np.ascontiguousarray(tables[..., [0, 2, 3]])
    Q = 24
    res = b.critical(torch.from_numpy(tables), 1, Q)
    moves = res["moves"][:, 0].cpu().numpy()
    pairs = (moves[..., 0] == 4).sum()
    assert pairs > 0 and int(res["skipped"].sum()) == 0
    status = _compare_pairs(torch, b, insts, variant, plan, moves, Q, (suite, "emitted"))
    assert np.all(status[moves[..., 0] == 4] == 0)
    rand = np.stack([_random_triples(rs, D.plan_length(pl), Q) for pl in plan])
    status = _compare_pairs(torch, b, insts, variant, plan, rand, Q, (suite, "random, shared"))
    assert (status == 0).any()
    own = np.stack([[D.random_plan(a, rs, cap) for _ in range(Q)] for a in insts])
    rand = np.stack([np.concatenate([_random_triples(rs, D.plan_length(pl), 1) for pl in per]) for per in own])
    _compare_pairs(torch, b, insts, variant, own, rand, Q, (suite, "random, own"))
    packed = sch.pair_move(3, 9, 5)
    assert packed == (sch.MOVE_PAIR, 3, 6 | (2 << 16)) and sch.MOVE_PAIR == 4
    with pytest.raises(ValueError):
        sch.pair_move(3, 3, 3)


def test_pair_move_edges_and_refusals(torch_gpu, suites):
    """dw = 0 and dw = dv - 1, u = 0 and v = L - 1, dv = 1 on two rows of one job (no same-job exception), and every
    refusal: status 4, with the plan's end found late where rows stand behind the first -1 row."""
    torch = torch_gpu
    variant, eps = suites["mk01"]
    a = eps[0]["inst"]
    cap = len(eps[0]["table"])
    rs = np.random.RandomState(9)
    mixed = D.random_plan(a, rs, cap)
    short = mixed.copy()
    short[cap - 3] = -1                        # rows behind the first -1 row: L = cap - 3
    L = cap
    by_job = np.array(sorted(mixed.tolist(), key=lambda row: (row[0], row[1])), np.int32)      # job after job
    P = lambda u, v, w: (4, u, (v - u) | ((w - u) << 16))
    valid = [P(2, 9, 2), P(2, 9, 8), P(0, 5, 3), P(7, L - 1, 10), P(0, L - 1, 0), P(0, L - 1, L - 2), P(0, 1, 0)]
    refused = [(4, 2, -1), (4, 2, 0), (4, 2, 3 | (3 << 16)), (4, 2, 3 | (4 << 16)), (4, -1, 1), (4, L - 1, 1), (4, L, 1), (4, 1 << 30, 1),
               (4, 2, 65535), (4, 0x7fffffff, 65535 | (32767 << 16)), (3, 0, 0)]
    at_end = [P(cap - 6, cap - 3, cap - 5), P(cap - 6, cap - 2, cap - 5), P(cap - 6, cap - 4, cap - 5)]
    moves = np.array([valid + refused + at_end] * 3, np.int32)
    Q, nv, nr = moves.shape[1], len(valid), len(refused)
    b = _batch(H.instance_set_from([a]), 3, variant)
    status = _compare_pairs(torch, b, [a] * 3, variant, np.stack([mixed, short, by_job]), moves, Q, "edges")
    assert np.all(status[:, nv:nv + nr] == 4)
    assert np.all(status[0, :nv] != 4) and np.all(status[0, nv + nr:] != 4) and (status[0, :nv] == 0).any()
    assert status[1, nv + nr:].tolist() == [4, 4, 2], "v on the first -1 row, behind it, and in front of it (operations missing)"
    assert np.all(status[1, 3:6] == 4), "v = cap - 1 lies behind the short plan's end"
    assert status[2, 6] != 4 and tuple(by_job[0, :2]) == tuple(by_job[1, :2]), "two rows of one job: moved like any other"
