"""The dispatched-schedule table on the host: C ABI exports, and the pure-numpy schedule module (rows / validate /
objectives) against the reference-held fixtures (tests/golden/*.npz, reference episodes with their per-step
operation type, machine, job and clock)."""
import ctypes
import os

import numpy as np
import pytest

from tests import helpers as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fjsp_env_record_schedule", "fjsp_env_schedule_capacity", "fjsp_env_schedule")
# suites without breakdown windows: a task runs p[k][m] from the clock at its dispatch
PLAIN = [(s, 0) for s in ("mk01", "synth10x5", "multijob", "large", "edge", "multiorder")] + \
        [("so_dfjsp", 5), ("mo_discretes", 2), ("so_sfjsp", 1)]


def test_library_exports_and_header_declares_the_schedule_abi(built):
    from deep_reinforcement_learning_for_fjsp_amd import _build
    lib = ctypes.CDLL(_build.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    hdr = open(os.path.join(REPO, "include", "fjsp_amd.h")).read()
    for name in SYMBOLS:
        assert (name + "(") in hdr, name
    assert "FJSP_ST_SCHEDULE_OVERFLOW = 16" in hdr
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    for name in SYMBOLS:
        assert name in _capi.SIGNATURES


def _episodes(suite, variant):
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    insts, eps, _ = H.load_suite(suite)
    for ep in eps:
        a = insts[ep["inst"]]
        T = ep["T"]
        rows = sch.from_trace(a, ep["k"][:T], ep["m"][:T], ep["job_n"][:T], ep["step_time"][:T])
        yield a, ep, rows


@pytest.mark.parametrize("suite,variant", PLAIN)
def test_reference_schedules_are_feasible_and_reproduce_the_objectives(suite, variant):
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    n = 0
    for a, ep, rows in _episodes(suite, variant):
        assert sch.validate(a, rows, variant) == [], (suite, ep["inst"])
        # the job identity the trace records agrees with the kind of the chosen operation type
        assert np.array_equal(rows[:, 0], ep["job_r"][:ep["T"]])
        obj = sch.objectives(a, rows, variant)
        assert obj["makespan"] == int(ep["final"][0]) == int(np.max(ep["tend"]))
        assert obj["delay_time_sum"] == int(ep["final"][1])
        if "completion" in ep and int(ep["completion"]) > 0:      # (variants that keep completion_time)
            assert obj["completion_time"] == int(ep["completion"])
        n += 1
    assert n > 0


def test_rows_group_per_machine_in_start_order():
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    a, ep, rows = next(_episodes("synth10x5", 0))
    cap = len(rows) + 3
    table = np.full((2, cap, 6), -1, np.int32)
    table[1, :len(rows)] = rows
    length = np.array([0, len(rows)], np.int32)
    got = sch.rows(table, length, 1)
    assert len(sch.rows(table, length, 0)) == 0
    assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, rows.tolist()))
    assert np.all(np.diff(got[:, 3]) >= 0)
    for m in np.unique(got[:, 3]):
        assert np.all(np.diff(got[got[:, 3] == m, 4]) >= 0)
    assert sch.validate(a, got, 0) == []


def test_validate_rejects_broken_schedules():
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    a, ep, rows = next(_episodes("multijob", 0))
    assert sch.validate(a, rows, 0) == []
    p = np.asarray(a.p)
    koff = np.concatenate(([0], np.cumsum(a.Jr)))

    # an overlap on a machine: move a task onto the start of another task of its machine (p unchanged)
    bad = rows.copy()
    i = int(np.argmax(rows[:, 4] > 0))
    same_m = np.where((rows[:, 3] == rows[i, 3]) & (np.arange(len(rows)) != i))[0]
    j = same_m[0]
    bad[i, 4] = rows[j, 4]; bad[i, 5] = rows[j, 4] + (rows[i, 5] - rows[i, 4])
    assert any("overlaps" in v for v in sch.validate(a, bad, 0))

    # a precedence swap: stage 1 of a job starts before its stage 0 ends
    bad = rows.copy()
    s1 = np.where(rows[:, 1] == 1)[0][0]
    s0 = np.where((rows[:, 0] == rows[s1, 0]) & (rows[:, 2] == rows[s1, 2]) & (rows[:, 1] == 0))[0][0]
    bad[s1, 4], bad[s1, 5] = rows[s0, 4], rows[s0, 4] + (rows[s1, 5] - rows[s1, 4])
    assert any("before stage 0 ends" in v for v in sch.validate(a, bad, 0))

    # a wrong processing time
    bad = rows.copy()
    bad[3, 5] += 1
    assert any("takes" in v for v in sch.validate(a, bad, 0))

    # an ineligible machine
    bad = rows.copy()
    k = int(koff[rows[5, 0]] + rows[5, 1])
    zero = np.where(p[k] == 0)[0]
    if len(zero):
        bad[5, 3] = zero[0]
        assert any("cannot process" in v for v in sch.validate(a, bad, 0))

    # a missing operation, and a duplicated one
    assert any("missing" in v for v in sch.validate(a, rows[:-1], 0))
    assert any("twice" in v for v in sch.validate(a, np.concatenate([rows, rows[:1]]), 0))


def test_validate_rejects_a_start_before_the_order_arrives():
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    a, ep, rows = next(_episodes("multiorder", 0))
    assert sch.validate(a, rows, 0) == []
    orders = sch.order_of_jobs(a)
    late = [i for i, (r, j, n) in enumerate(rows[:, :3].tolist()) if j == 0 and orders[r][n] > 0]
    assert late
    bad = rows.copy()
    i = late[0]
    bad[i, 5] -= bad[i, 4]; bad[i, 4] = 0
    assert any("before its order arrives" in v for v in sch.validate(a, bad, 0))


def test_breakdown_shift_matches_the_reference_rules():
    """MO_DFJSP_breakdown.py:203-231 on hand-made windows: a window covering the dispatch time moves the start, one
    beginning inside the task stretches it, one beginning exactly at its end changes neither."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    w = [(10, 20), (30, 35), (60, 70)]
    assert sch.shifted(w, 12, 5) == (20, 25)           # covered start: begins at the window's end
    assert sch.shifted(w, 25, 10) == (25, 40)          # (30, 35) begins inside: +5
    assert sch.shifted(w, 50, 10) == (50, 60)          # (60, 70) begins at the end: task unchanged
    assert sch.shifted(w, 0, 5) == (0, 5)

    class Inst(object):
        Jr = np.array([1]); p = np.array([[5]]); count = np.array([[1]]); arrive = np.array([0]); delivery = np.array([100])
        bk_n = np.array([3]); bk = np.array(w)
    ok = np.array([[0, 0, 0, 0, 20, 25]])
    assert sch.validate(Inst(), ok, 4) == []
    assert sch.validate(Inst(), np.array([[0, 0, 0, 0, 12, 17]]), 4) != []      # inside a window, unshifted
    assert sch.validate(Inst(), np.array([[0, 0, 0, 0, 20, 26]]), 4) != []


# ---------------------------------------------------------------- tests/golden/schedule.npz (the reference's task objects)
def test_reference_schedule_fixture_is_feasible_and_matches_the_episodes():
    """Every table the reference produced (breakdown instances included) passes validate, reproduces the episode's
    makespan / tardiness, and -- without breakdowns -- equals the schedule rebuilt from the existing fixture's trace."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    from tests import schedule_fixture as F
    fx = F.load()
    assert set(fx) == {"mk01", "synth10x5", "multijob", "multiorder", "so_sfjsp", "so_dfjsp", "mo_discretes", "mo_dfjsp"}
    for suite, (variant, eps) in fx.items():
        _, src_eps, _ = H.load_suite(suite)
        for ep in eps:
            a, table = ep["inst"], ep["table"].astype(np.int64)
            src = src_eps[ep["source"]]
            T = src["T"]
            assert len(table) == T and np.array_equal(ep["actions"], src["actions"][:T])
            assert sch.validate(a, table, variant) == [], (suite, ep["source"])
            obj = sch.objectives(a, table, variant)
            assert obj["delay_time_sum"] == int(src["final"][1]), (suite, ep["source"])
            if variant != 4:
                assert obj["makespan"] == int(src["final"][0])
                rebuilt = sch.from_trace(a, src["k"][:T], src["m"][:T], src["job_n"][:T], src["step_time"][:T])
                assert np.array_equal(rebuilt, table), (suite, ep["source"])
            else:
                # makespan = max machine time_end: at least the last task end (a window opening at it delays the machine)
                assert obj["makespan"] <= int(src["final"][0])


def test_reference_schedule_fixture_exercises_the_breakdown_shifts():
    """The mo_dfjsp episodes hold tasks whose start the reference moved past a covering window, and tasks ending exactly
    where a window of their machine opens (MO_DFJSP_breakdown.py:213-228)."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    from tests import schedule_fixture as F
    variant, eps = F.load()["mo_dfjsp"]
    moved = at_end = 0
    for ep in eps:
        a, table = ep["inst"], ep["table"].astype(np.int64)
        src = H.load_suite("mo_dfjsp")[1][ep["source"]]
        clock = np.concatenate(([0], src["step_time"][:src["T"] - 1]))
        moved += int(np.sum(table[:, 4] > clock))
        w = sch.breakdowns_of(a)
        at_end += sum(1 for r in table.tolist() if any(bs == r[5] for bs, _ in w[r[3]]))
        # a task whose start did not move began at the dispatch clock
        assert np.all(table[:, 4] >= clock)
    assert moved > 0 and at_end > 0
