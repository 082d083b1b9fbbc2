"""CPU: tests/decode_active_reference.py, the numpy statement of fjsp_schedule_decode_active, on the reference's own
schedules and random plans (tests/golden/schedule.npz) -- dominance over the semi-active decode row by row, closure through
it, idempotence, activity by brute force, the count of inserted rows -- on hand-made plans with known answers, on every
status code and every move kind, and the new symbols' export / declaration."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import critical_reference as R
from tests import decode_active_cases as AC
from tests import decode_active_reference as A
from tests import decode_reference as D
from tests import schedule_fixture as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUITES = ("mk01", "synth10x5", "multijob", "so_sfjsp", "mo_discretes", "multiorder", "so_dfjsp")
SYMBOLS = ("fjsp_schedule_decode_active", "fjsp_schedule_decode_active_group", "fjsp_schedule_decode_active_resident")
RANDOM_PLANS = 2                                                           # per episode, beside its recorded plan


@pytest.fixture(scope="module")
def suites():
    return F.load()


def test_symbols_are_exported_declared_and_bound(built):
    from deep_reinforcement_learning_for_fjsp_amd import _build, _capi
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    header = open(os.path.join(REPO, "include", "fjsp_amd.h")).read()
    for name in SYMBOLS:
        assert name in exported, name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _capi.SIGNATURES, name
    vp, i32 = C.c_void_p, C.c_int32
    assert _capi.SIGNATURES["fjsp_schedule_decode_active"] == (C.c_int, [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp])
    text = header[header.index("decoded ACTIVELY"):header.index("fjsp_schedule_decode_active_resident(")]
    for word in ("ORDERING", "one stream", "8 cap G groups bytes", "no clock exceeds its semi-active value", "FJSP_DECODE_ACTIVE_WORKSPACE_BYTES"):
        assert word in text, word


def test_null_and_count_refusals_need_no_device(built):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    lib = _capi.lib()
    assert lib.fjsp_schedule_decode_active(None, None, 1, None, 1, None, None, None, None, None, None) == _capi.FJSP_E_ARG
    assert "fjsp_schedule_decode_active" in lib.fjsp_last_error().decode()
    assert lib.fjsp_schedule_decode_active_group(None) == 0 and lib.fjsp_schedule_decode_active_resident(None) == 0


def _check_plan(a, variant, plan, what):
    """Every property of one plan's active decode; returns (the active result, the semi-active result)."""
    semi = D.decode_one(a, variant, plan)
    act = A.decode_one(a, variant, plan)
    assert semi["status"] == D.OK and act["status"] == A.OK and act["length"] == semi["length"], what
    L = act["length"]
    s, t = semi["table"][:L].astype(np.int64), act["table"][:L].astype(np.int64)
    # dominance, row by row: the same operations on the same machines, none ends later
    assert np.array_equal(t[:, :4], s[:, :4]) and np.all(t[:, 5] <= s[:, 5]) and np.array_equal(t[:, 5] - t[:, 4], s[:, 5] - s[:, 4]), what
    assert np.all(act["objective"] <= semi["objective"]), what
    assert np.all(act["table"][L:] == -1), what
    # inserted == 0 exactly where the two tables coincide
    assert (act["inserted"] == 0) == np.array_equal(t, s), what
    assert act["inserted"] <= int((t[:, 4] < s[:, 4]).sum()), what          # (an inserted row begins before the semi-active free[m])
    # closure: the begin-ordered plan decodes semi-actively to the same table, row for row
    ordered = A.begin_ordered_plan(act["table"])
    want = t[np.argsort(t[:, 4], kind="stable")]
    back = D.decode_one(a, variant, ordered)
    assert back["status"] == D.OK and np.array_equal(back["table"][:L], want) and np.array_equal(back["objective"], act["objective"]), what
    # idempotence: decoding it actively inserts nothing
    again = A.decode_one(a, variant, ordered)
    assert again["inserted"] == 0 and np.array_equal(again["table"][:L], want) and np.array_equal(again["objective"], act["objective"]), what
    assert A.is_active(a, act["table"]), what
    return act, semi


@pytest.mark.parametrize("suite", SUITES)
def test_dominance_closure_idempotence_activity_on_the_golden_suites(suites, suite):
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    variant, eps = suites[suite]
    rs = np.random.RandomState(len(suite))
    improved = inserted = plans = 0
    for i, ep in enumerate(eps):
        a = ep["inst"]
        for c, plan in enumerate([D.plan_from_table(ep["table"])] + [D.random_plan(a, rs) for _ in range(RANDOM_PLANS)]):
            act, semi = _check_plan(a, variant, plan, (suite, i, c))
            if c == 1:
                assert sch.validate(a, act["table"][:act["length"]], variant) == [], (suite, i)
                obj = sch.objectives(a, act["table"][:act["length"]], variant)
                assert act["objective"].tolist() == [obj["makespan"], obj["delay_time_sum"]], (suite, i)
            improved += int(act["objective"][0] < semi["objective"][0])
            inserted += act["inserted"]
            plans += 1
    assert plans == 3 * len(eps) and inserted > 0 and improved > 0, (suite, improved, inserted)


def test_a_semi_active_table_is_not_always_active(suites):
    """is_active is a test that can fail: some random plan of Mk01 leaves a gap its semi-active decode does not use."""
    variant, eps = suites["mk01"]
    a = eps[0]["inst"]
    rs = np.random.RandomState(3)
    verdicts = [A.is_active(a, D.decode_one(a, variant, D.random_plan(a, rs))["table"]) for _ in range(8)]
    assert not all(verdicts)


@pytest.mark.parametrize("case", AC.cases(), ids=lambda c: c.name)
def test_hand_made_cases(case):
    act = A.decode_one(case.inst, case.variant, case.plan)
    assert act["status"] == A.OK and act["length"] == len(case.plan)
    assert act["table"][:, 4].tolist() == case.begins and act["inserted"] == case.inserted
    _check_plan(case.inst, case.variant, case.plan, case.name)


def test_mid_interval_case_starts_at_the_interval_end():
    case = [c for c in AC.cases() if c.name.startswith("a job ready in the middle")][0]
    tab = A.decode_one(case.inst, case.variant, case.plan)["table"]
    assert tab[1, 5] == 3 and tab[0, 4] < 3 < tab[0, 5] and tab[2, 4] == tab[0, 5]   # ready at 3 inside [0, 5): begins at 5


def _tiny():
    return AC.DL.instance("tiny", [2, 1], [[3, 4], [0, 2], [5, 1]], [2, 1], delivery=[6])


TINY_PLAN = np.array([[0, 0, 0], [0, 1, 1], [1, 0, 0], [0, 0, 1], [0, 1, 1]], np.int32)


@pytest.mark.parametrize("plan, want", [
    ([[2, 0, 0]] + TINY_PLAN[1:].tolist(), A.NO_JOB),
    ([[0, 2, 0]] + TINY_PLAN[1:].tolist(), A.NO_JOB),
    (TINY_PLAN.tolist() + [[1, 0, 0]], A.STAGES),
    (TINY_PLAN[:4].tolist(), A.STAGES),
    ([], A.STAGES),
    (TINY_PLAN[:3].tolist() + [[0, 0, 0]] + TINY_PLAN[4:].tolist(), A.MACHINE),
    ([[0, 0, 2]] + TINY_PLAN[1:].tolist(), A.MACHINE),
])
def test_status_codes_are_the_semi_active_decoders(plan, want):
    full = np.full((7, 3), -1, np.int32)
    full[:len(plan)] = np.asarray(plan, np.int32).reshape(-1, 3)
    got = A.decode_one(_tiny(), 0, full)
    assert got["status"] == want == D.decode_one(_tiny(), 0, full)["status"]
    assert got["length"] == 0 and got["inserted"] == 0 and got["objective"].tolist() == [-1, -1] and np.all(got["table"] == -1)


@pytest.mark.parametrize("move", [(3, 0, 0), (-1, 0, 0), (1, -1, 0), (1, 5, 0), (2, 4, 0), (4, 0, 0), (4, 3, 2), (4, 0, -1), (4, 0, 2 | (2 << 16))])
def test_bad_moves_are_status_4_and_outrank_a_bad_row(move):
    full = np.full((7, 3), -1, np.int32)
    full[:5] = TINY_PLAN
    assert A.decode_one(_tiny(), 0, full, move)["status"] == A.BAD_MOVE
    bad = full.copy()
    bad[0] = (2, 0, 0)
    got = A.decode_one(_tiny(), 0, bad, move)
    assert got["status"] == A.BAD_MOVE and got["inserted"] == 0 and got["length"] == 0


def test_every_move_kind_equals_the_decode_of_the_materialised_plan(suites):
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    variant, eps = suites["mk01"]
    a = eps[0]["inst"]
    rs = np.random.RandomState(9)
    plan = D.random_plan(a, rs)
    L = D.plan_length(plan)
    p, koff = np.asarray(a.p), np.concatenate(([0], np.cumsum(a.Jr)))
    stage_of = lambda u: int(np.sum((plan[:u, 0] == plan[u, 0]) & (plan[:u, 1] == plan[u, 1])))
    moves = [(0, 3, 1), (2, 0, 0), (2, L - 2, 0), sch.pair_move(1, 9, 4), sch.pair_move(0, L - 1, 0), sch.pair_move(5, 6, 5)]
    moves += [(1, u, int(np.flatnonzero(p[koff[plan[u, 0]] + stage_of(u)] > 0)[-1])) for u in (0, L // 2, L - 1)]
    kinds, shifted = set(), 0
    for move in moves:
        made = R.materialise_moved(plan, move)
        x, y = A.decode_one(a, variant, plan, move), A.decode_one(a, variant, made)
        # (a pair move that carries a row's machine to another stage of its job can end in status 3: the same on both sides)
        assert x["status"] in (A.OK, A.MACHINE) and all(np.array_equal(x[k], y[k]) for k in A.KEYS), move
        if x["status"] == A.OK:
            kinds.add(move[0])
            shifted += x["inserted"]
    assert kinds == {0, 1, 2, 4} and shifted > 0
    assert A.decode_one(a, variant, plan, (1, 0, 99))["status"] == A.MACHINE
