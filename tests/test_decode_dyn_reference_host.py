"""CPU: tests/decode_dyn_reference.py, the numpy statement of fjsp_schedule_decode_dyn, pinned to the reference's own
MO_DFJSP schedules and episodes, to schedule.validate / schedule.objectives on random plans, and to hand-made shops with
written answers, one per branch of the contract."""
import numpy as np
import pytest

from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
from tests import decode_dyn_reference as DD
from tests import decode_reference as D
from tests import helpers as H
from tests import schedule_fixture as F


@pytest.fixture(scope="module")
def schedules():
    variant, eps = F.load()["mo_dfjsp"]
    assert variant == DD.VARIANT and len(eps) == 9
    return eps


def test_the_reference_tables_decode_to_themselves(schedules):
    stretched = 0
    for i, ep in enumerate(schedules):
        a, t = ep["inst"], ep["table"]
        one = DD.decode_one(a, D.plan_from_table(t))
        assert one["status"] == 0 and one["length"] == len(t), i
        assert np.array_equal(one["table"], t), (i, np.flatnonzero((one["table"] != t).any(1))[:5])
        obj = sch.objectives(a, t, DD.VARIANT)
        assert one["objective"][0] == obj["makespan"] and one["objective"][1] == obj["delay_time_sum"], i
        k = np.concatenate(([0], np.cumsum(a.Jr)))[t[:, 0]] + t[:, 1]
        stretched += int(((t[:, 5] - t[:, 4]) != np.asarray(a.p)[k, t[:, 3]]).sum())
    assert stretched > 0                                                 # (the tables do exercise the windows)


def test_the_reference_episodes_end_with_the_decoded_objectives():
    """All 54 episodes as plans.  An episode may differ only where the decode is tighter than the event clock: more than
    one order, and the first row that begins before the reference dispatched it is a first-stage row of a later order that
    the decode starts at the order's arrival.  At most 6 such episodes."""
    insts, eps, _ = H.load_suite("mo_dfjsp")
    assert len(eps) == 54
    tighter = []
    for e, ep in enumerate(eps):
        a = insts[ep["inst"]]
        plan = np.stack([ep["job_r"], ep["job_n"], ep["m"]], 1)
        one = DD.decode_one(a, plan)
        assert one["status"] == 0, e
        want = (int(ep["completion"]), int(ep["delay"][-1]), int(ep["energy"]))
        got = tuple(int(v) for v in one["objective"])
        if got == want:
            continue
        assert a.S > 1, (e, got, want)
        clock = np.concatenate(([0], np.asarray(ep["step_time"], np.int64)[:-1]))
        early = np.flatnonzero(one["table"][:len(plan), 4] < clock)
        assert len(early), (e, got, want)
        r, j, n, m, begin, end = (int(v) for v in one["table"][early[0]])
        s = int(sch.order_of_jobs(a)[r][n])
        assert j == 0 and s >= 1 and begin == int(a.arrive[s]), (e, early[0], (r, j, n, m, begin, end), s)
        tighter.append(e)
    assert len(tighter) <= 6, tighter


def _energy_of(a, table):
    """Energy of a decoded table, recomputed machine by machine: sum(power * p) + idle_power * the gaps between a task's end
    and the next dispatch on the machine.  The dispatch time of a row is the later of its job's and its machine's release
    (the machines' ends, which a window starting at a task's end moves), rebuilt here from the rows in table order."""
    p = np.asarray(a.p, np.int64)
    power = np.asarray(a.power, np.int64).reshape(p.shape)
    koff = np.concatenate(([0], np.cumsum(np.asarray(a.Jr, np.int64))))
    windows = sch.breakdowns_of(a)
    arrive = np.asarray(a.arrive, np.int64)
    orders = sch.order_of_jobs(a)
    job_free, m_free, per_machine = {}, {}, {}
    work = 0
    for r, j, n, m, b, e in np.asarray(table, np.int64).tolist():
        t = max(job_free.get((r, n), int(arrive[orders[r][n]])), m_free.get(m, 0))
        d = int(p[koff[r] + j, m])
        assert sch.shifted(windows[m], t, d) == (b, e)
        mend = e + sum(be - bs for bs, be in windows[m] if bs == e)
        job_free[(r, n)] = m_free[m] = mend
        per_machine.setdefault(m, []).append((t, e))
        work += int(power[koff[r] + j, m]) * d
    idle = sum(int(a.idle_power[m]) * sum(t1 - e0 for (_, e0), (t1, _) in zip(rows, rows[1:])) for m, rows in per_machine.items())
    return work + idle


def test_random_plans_are_feasible_and_agree_with_the_host_objectives(schedules):
    rs = np.random.RandomState(0)
    done = 0
    for i, ep in enumerate(schedules):
        a = ep["inst"]
        if len(ep["table"]) > 700:
            continue
        for _ in range(3):
            one = DD.decode_one(a, D.random_plan(a, rs))
            assert one["status"] == 0
            assert sch.validate(a, one["table"], DD.VARIANT) == [], i
            obj = sch.objectives(a, one["table"], DD.VARIANT)
            assert (obj["makespan"], obj["delay_time_sum"]) == (int(one["objective"][0]), int(one["objective"][1])), i
            assert _energy_of(a, one["table"]) == int(one["objective"][2]), i
            done += 1
    assert done == 21


@pytest.mark.parametrize("name, a, plan, table, objective", DD.hand_cases(), ids=[c[0] for c in DD.hand_cases()])
def test_hand_made_shops(name, a, plan, table, objective):
    one = DD.decode_one(a, plan)
    assert one["status"] == 0 and one["length"] == len(plan)
    assert one["table"].tolist() == [list(row) for row in table]
    assert tuple(int(v) for v in one["objective"]) == objective
    assert sch.validate(a, one["table"], DD.VARIANT) == []


def test_moves_and_status_codes_are_the_decoders(schedules):
    """Moves are applied as tests/decode_reference.py and tests/critical_reference.py apply them; the failures are coded
    alike, with three -1 objectives."""
    from tests import critical_reference as R
    a = schedules[7]["inst"]
    plan = D.plan_from_table(schedules[7]["table"])
    L = len(plan)
    for move in ((1, 0, 0), (1, 0, 1), (1, 0, 2), (2, 0, 0), (2, L - 2, 0), sch.pair_move(1, 4, 2), (0, 0, 0)):
        want = DD.decode_one(a, R.materialise_moved(plan, move))
        got = DD.decode_one(a, plan, move)
        for key in DD.KEYS:
            assert np.array_equal(got[key], want[key]), (move, key)
    for move, code in (((3, 0, 0), 4), ((1, L, 0), 4), ((2, L - 1, 0), 4), ((4, 0, 0), 4), ((1, 0, 3), 3), ((1, 0, -1), 3)):
        got = DD.decode_one(a, plan, move)
        assert got["status"] == code and got["objective"].tolist() == [-1, -1, -1] and got["length"] == 0 and np.all(got["table"] == -1)
    spoiled = plan.copy(); spoiled[0, 0] = 9
    assert DD.decode_one(a, spoiled)["status"] == 1
    spoiled = plan.copy(); spoiled[L - 1] = spoiled[0]
    assert DD.decode_one(a, spoiled)["status"] == 2
    assert DD.decode_one(a, plan[:-1])["status"] == 2
