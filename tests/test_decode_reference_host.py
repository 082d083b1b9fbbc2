"""CPU: tests/decode_reference.py, the numpy statement of fjsp_schedule_decode, pinned to the reference's own schedules
(tests/golden/schedule.npz), its status codes and moves on hand-made plans, and the new symbols' export / declaration."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import decode_reference as D
from tests import helpers as H
from tests import schedule_fixture as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE = ("mk01", "synth10x5", "multijob", "so_sfjsp", "mo_discretes")
ORDERS = ("multiorder", "so_dfjsp")
SYMBOLS = ("fjsp_schedule_decode", "fjsp_schedule_decode_capacity", "fjsp_schedule_decode_group")


@pytest.fixture(scope="module")
def suites():
    return F.load()


def _tiny():
    """Two kinds: kind 0 has two stages and two jobs, kind 1 one stage and one job; two machines, stage (0, 1) runs on
    machine 1 only.  One order arriving at 0."""
    a = H.Arrays()
    a.Jr = np.array([2, 1], np.int32)
    a.p = np.array([[3, 4], [0, 2], [5, 1]], np.int32)
    a.count = np.array([[2, 1]], np.int32)
    a.arrive = np.array([0], np.int32)
    a.delivery = np.array([6], np.int32)
    return a


# a complete plan of _tiny: (r, n, m)
TINY_PLAN = np.array([[0, 0, 0], [0, 1, 1], [1, 0, 0], [0, 0, 1], [0, 1, 1], [-1, -1, -1], [-1, -1, -1]], np.int32)[:5]


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
    assert _capi.SIGNATURES["fjsp_schedule_decode"] == (C.c_int, [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp])
    assert "fjsp_decode.hip" in _build.HIP_SOURCES
    assert "SO_FJSSP.py:176-196" in header[header.index("Explicit schedules decoded"):header.index("fjsp_schedule_decode_group(")]
    assert "class_FJSSP.py:212-218" in header[header.index("Explicit schedules decoded"):header.index("fjsp_schedule_decode_group(")]


def test_null_and_count_refusals_need_no_device(built):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    lib = _capi.lib()
    assert lib.fjsp_schedule_decode(None, None, 1, None, 1, None, None, None, None, None) == _capi.FJSP_E_ARG
    assert lib.fjsp_schedule_decode_capacity(None) == 0 and lib.fjsp_schedule_decode_group(None) == 0


@pytest.mark.parametrize("suite", SINGLE)
def test_single_order_suites_decode_to_the_reference_rows(suites, suite):
    """The environments' schedules are semi-active: decoding the recorded sequence and machines gives the recorded times."""
    variant, eps = suites[suite]
    rows = 0
    for ep in eps:
        want = ep["table"]
        got = D.decode_one(ep["inst"], variant, D.plan_from_table(want))
        assert got["status"] == D.OK and got["length"] == len(want), (suite, ep["source"])
        assert np.array_equal(got["table"], want), (suite, ep["source"])
        rows += len(want)
    assert rows > 0


def test_single_order_suites_hold_2646_rows(suites):
    assert sum(len(ep["table"]) for s in SINGLE for ep in suites[s][1]) == 2646


@pytest.mark.parametrize("suite", ORDERS)
def test_order_suites_never_later_feasible_and_never_worse(suites, suite):
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    variant, eps = suites[suite]
    earlier = 0
    for ep in eps:
        a, want = ep["inst"], ep["table"].astype(np.int64)
        got = D.decode_one(a, variant, D.plan_from_table(want))
        assert got["status"] == D.OK and got["length"] == len(want), (suite, ep["source"])
        t = got["table"].astype(np.int64)
        assert np.array_equal(t[:, :4], want[:, :4]) and np.all(t[:, 4] <= want[:, 4]), (suite, ep["source"])
        earlier += int((t[:, 4] < want[:, 4]).sum())
        assert sch.validate(a, t, variant) == [], (suite, ep["source"])
        new, old = sch.objectives(a, t, variant), sch.objectives(a, want, variant)
        assert new["makespan"] == old["makespan"] and new["delay_time_sum"] <= old["delay_time_sum"], (suite, ep["source"])
        assert got["objective"].tolist() == [new["makespan"], new["delay_time_sum"]]
    assert earlier == {"multiorder": 120, "so_dfjsp": 74}[suite]


def test_objective_equals_schedule_objectives_on_random_plans(suites):
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    rs = np.random.RandomState(5)
    for suite in ("mk01", "multiorder"):
        variant, eps = suites[suite]
        a = eps[0]["inst"]
        for _ in range(3):
            got = D.decode_one(a, variant, D.random_plan(a, rs))
            assert got["status"] == D.OK
            assert sch.validate(a, got["table"], variant) == []
            obj = sch.objectives(a, got["table"], variant)
            assert got["objective"].tolist() == [obj["makespan"], obj["delay_time_sum"]]


def test_hand_made_plan_times():
    got = D.decode_one(_tiny(), 0, TINY_PLAN)
    assert got["status"] == D.OK and got["length"] == 5
    assert got["table"].tolist() == [[0, 0, 0, 0, 0, 3], [0, 0, 1, 1, 0, 4], [1, 0, 0, 0, 3, 8], [0, 1, 0, 1, 4, 6], [0, 1, 1, 1, 6, 8]]
    # due dates of kind 0: round(round(6 * 2 / 2) * n / 2) = 0, 3; of kind 1: 0
    assert got["objective"].tolist() == [8, (6 - 0) + (8 - 3) + (8 - 0)]


@pytest.mark.parametrize("plan, want", [
    ([[2, 0, 0]] + TINY_PLAN[1:].tolist(), D.NO_JOB),                      # no kind 2
    ([[0, 2, 0]] + TINY_PLAN[1:].tolist(), D.NO_JOB),                      # kind 0 has jobs 0 and 1
    ([[-1, 0, 0]] + TINY_PLAN[1:].tolist(), D.NO_JOB),
    (TINY_PLAN.tolist() + [[1, 0, 0]], D.STAGES),                          # a second row of a one-stage job
    (TINY_PLAN[:4].tolist(), D.STAGES),                                    # the plan ends with an operation missing
    ([], D.STAGES),
    (TINY_PLAN[:3].tolist() + [[0, 0, 0]] + TINY_PLAN[4:].tolist(), D.MACHINE),   # p = 0
    ([[0, 0, 2]] + TINY_PLAN[1:].tolist(), D.MACHINE),                     # two machines
    ([[0, 0, -1]] + TINY_PLAN[1:].tolist(), D.MACHINE),
])
def test_status_codes_on_hand_made_plans(plan, want):
    full = np.full((7, 3), -1, np.int32)
    full[:len(plan)] = np.asarray(plan, np.int32).reshape(-1, 3)
    got = D.decode_one(_tiny(), 0, full)
    assert got["status"] == want and got["length"] == 0
    assert got["objective"].tolist() == [-1, -1] and np.all(got["table"] == -1) and got["table"].shape == (7, 6)


@pytest.mark.parametrize("move", [(3, 0, 0), (-1, 0, 0), (1, -1, 0), (1, 5, 0), (1, 7, 0), (2, -1, 0), (2, 4, 0), (2, 6, 0)])
def test_bad_moves_are_status_4(move):
    full = np.full((7, 3), -1, np.int32)
    full[:5] = TINY_PLAN
    assert D.decode_one(_tiny(), 0, full, move)["status"] == D.BAD_MOVE
    bad = full.copy()
    bad[0] = (2, 0, 0)                                                     # a bad move outranks a bad row
    assert D.decode_one(_tiny(), 0, bad, move)["status"] == D.BAD_MOVE
    assert np.array_equal(D.materialise(full, move), full)


def test_each_move_kind_against_a_hand_materialised_plan():
    a = _tiny()
    full = np.full((7, 3), -1, np.int32)
    full[:5] = TINY_PLAN
    cases = [
        ((0, 3, 1), TINY_PLAN),
        ((1, 0, 1), [[0, 0, 1]] + TINY_PLAN[1:].tolist()),
        ((1, 4, 1), TINY_PLAN),                                            # the machine it has
        ((2, 0, 0), [[0, 1, 1], [0, 0, 0]] + TINY_PLAN[2:].tolist()),
        ((2, 3, 0), TINY_PLAN[:3].tolist() + [[0, 1, 1], [0, 0, 1]]),
        ((2, 2, 0), TINY_PLAN[:2].tolist() + [[0, 0, 1], [1, 0, 0]] + TINY_PLAN[4:].tolist()),
    ]
    for move, rows in cases:
        want = np.full((7, 3), -1, np.int32)
        want[:5] = np.asarray(rows)
        assert np.array_equal(D.materialise(full, move), want), move
        x, y = D.decode_one(a, 0, full, move), D.decode_one(a, 0, want)
        assert x["status"] == D.OK and all(np.array_equal(x[k], y[k]) for k in x), move
    # two rows of one job: the swap changes nothing
    same = np.full((7, 3), -1, np.int32)
    same[:5] = [[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 1], [1, 0, 1]]
    assert np.array_equal(D.materialise(same, (2, 0, 0)), same) and np.array_equal(D.materialise(same, (2, 2, 0)), same)
    assert D.decode_one(a, 0, same, (2, 0, 0))["table"].tolist() == D.decode_one(a, 0, same)["table"].tolist()
    # reassigning to an ineligible machine is the row's own status
    assert D.decode_one(a, 0, full, (1, 3, 0))["status"] == D.MACHINE


def test_apply_moves_matches_the_reference():
    """schedule.apply_moves (tensor indexing, runs on the CPU as well) against materialise, shared and per-candidate plans."""
    import torch
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    full = np.full((7, 3), -1, np.int32)
    full[:5] = TINY_PLAN
    other = full.copy()
    other[:5] = [[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 1], [1, 0, 1]]
    moves = np.array([[(0, 0, 0), (1, 0, 1), (1, 4, 0), (2, 0, 0), (2, 3, 0), (2, 4, 0), (3, 1, 1), (1, 9, 0), (2, -1, 0)],
                      [(2, 0, 0), (2, 1, 0), (2, 2, 0), (2, 3, 0), (1, 2, 0), (1, -1, 0), (0, 9, 9), (2, 6, 0), (1, 5, 1)]], np.int32)
    plans = np.stack([full, other])
    want = np.stack([[D.materialise(plans[i], moves[i, q]) for q in range(moves.shape[1])] for i in range(2)])
    got = sch.apply_moves(torch.from_numpy(plans), torch.from_numpy(moves))
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
    per = np.ascontiguousarray(np.broadcast_to(plans[:, None], (2, moves.shape[1], 7, 3)))
    assert np.array_equal(sch.apply_moves(torch.from_numpy(per), torch.from_numpy(moves)).numpy(), want)
    assert np.array_equal(sch.plan_of(np.arange(24).reshape(1, 4, 6)), np.arange(24).reshape(1, 4, 6)[..., [0, 2, 3]])
