"""Plain numpy statement of fjsp_schedule_decode_dyn (include/fjsp_amd.h): explicit schedules of MO_DFJSP -> times shifted
by the machines' breakdown windows, (makespan, tardiness, energy) and status codes, with the moves.  Written from the entry
point's contract and deep_reinforcement_learning_for_fjsp_amd.schedule (order_of_jobs, due_dates, breakdowns_of),
independently of the kernel; the tests of the kernel compare with it bit for bit.  Python integers throughout.

Plans, moves and status codes are tests/decode_reference.py's (moved, plan_length); MOVE_PAIR is stated as
tests/critical_reference.py states it: the materialised plan decoded without a move."""
import numpy as np

from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
from tests import critical_reference as R
from tests import decode_reference as D

OK, NO_JOB, STAGES, MACHINE, BAD_MOVE = range(5)
VARIANT = sch.VARIANT_MO_DFJSP
KEYS = ("objective", "status", "table", "length")


def shift(windows, t, d):
    """(begin, end, machine_end) of a task of duration d dispatched at t on a machine with these windows, file order."""
    begin, end = t, t + d
    machine_end = end
    for bs, be in windows:
        if bs <= t < be:
            begin += be - t
            end += be - t
            machine_end = end
        elif t < bs < end:
            end += be - bs
            machine_end = end
        elif bs == end:
            machine_end += be - bs
        elif bs > end:
            break
    return begin, end, machine_end


def decode_one(inst, plan, move=None, cap=None):
    """dict(status, objective int64[3], table int32[cap][6], length) of one candidate."""
    plan = np.asarray(plan, np.int64).reshape(-1, 3)
    cap = len(plan) if cap is None else cap
    fail = lambda code: dict(status=code, objective=np.array([-1, -1, -1], np.int64), table=np.full((cap, 6), -1, np.int32), length=0)
    if move is not None and int(move[0]) == R.MOVE_PAIR:
        if not R.pair_ok(plan, move):
            return fail(BAD_MOVE)
        rows, ok = D.moved(R.materialise_pair(plan, move), None)
    else:
        rows, ok = D.moved(plan, move)
    if not ok:
        return fail(BAD_MOVE)
    Jr = np.asarray(inst.Jr, np.int64)
    p = np.asarray(inst.p, np.int64)
    power = np.asarray(inst.power, np.int64).reshape(p.shape)
    idle = np.asarray(inst.idle_power, np.int64)
    windows = sch.breakdowns_of(inst)
    koff = np.concatenate(([0], np.cumsum(Jr)))
    arrive = np.asarray(inst.arrive, np.int64)
    orders = sch.order_of_jobs(inst)
    due = sch.due_dates(inst, VARIANT)
    R_, M = len(Jr), p.shape[1]
    ready = [[int(v) for v in arrive[orders[r]]] for r in range(R_)]
    stage = [[0] * len(orders[r]) for r in range(R_)]
    free = [0] * M
    last_end = [None] * M
    table = np.full((cap, 6), -1, np.int32)
    makespan = tard = energy = 0
    for i, (r, n, m) in enumerate(rows.tolist()):
        if not (0 <= r < R_ and 0 <= n < len(orders[r])):
            return fail(NO_JOB)
        j = stage[r][n]
        if j >= Jr[r]:
            return fail(STAGES)
        k = int(koff[r]) + j
        if not (0 <= m < M) or p[k, m] <= 0:
            return fail(MACHINE)
        d = int(p[k, m])
        t = max(ready[r][n], free[m])
        begin, end, machine_end = shift(windows[m], t, d)
        energy += int(power[k, m]) * d
        if last_end[m] is not None:
            energy += (t - last_end[m]) * int(idle[m])
        last_end[m] = end
        ready[r][n] = free[m] = machine_end
        stage[r][n] = j + 1
        makespan = max(makespan, end)
        if j == Jr[r] - 1:
            tard += max(0, end - int(due[r][n]))
        table[i] = (r, j, n, m, begin, end)
    if any(stage[r][n] != Jr[r] for r in range(R_) for n in range(len(orders[r]))):
        return fail(STAGES)
    return dict(status=OK, objective=np.array([makespan, tard, energy], np.int64), table=table, length=len(rows))


def decode(insts, plan, moves=None, n_cand=1, cap=None):
    """The entry point on a batch: insts[i] is env i's instance; plan int[N][cap][3] or [N][n_cand][cap][3]; moves None or
    int[N][n_cand][3].  dict(objective int64[N][n_cand][3], status int32[N][n_cand], table int32[N][n_cand][cap][6],
    length int32[N][n_cand])."""
    plan = np.asarray(plan)
    N = len(insts)
    cap = plan.shape[-2] if cap is None else cap
    out = dict(objective=np.zeros((N, n_cand, 3), np.int64), status=np.zeros((N, n_cand), np.int32),
               table=np.zeros((N, n_cand, cap, 6), np.int32), length=np.zeros((N, n_cand), np.int32))
    for i in range(N):
        for q in range(n_cand):
            one = decode_one(insts[i], plan[i] if plan.ndim == 3 else plan[i, q], None if moves is None else moves[i][q], cap)
            for key in out:
                out[key][i, q] = one[key]
    return out


def shop(p, power, idle_power, windows, Jr=None, count=None, arrive=(0,), delivery=(0,)):
    """A hand-made MO_DFJSP instance: p[K][M] and power[K][M] (0 = ineligible), idle_power[M], windows[m] = [(bs, be), ...]
    in file order; Jr defaults to one kind of K stages, count[S][R] to one job of it."""
    a = type("Shop", (), {})()
    a.p = np.asarray(p, np.int32).reshape(len(p), -1)
    a.K, a.M = a.p.shape
    a.Jr = np.asarray([a.K] if Jr is None else Jr, np.int32)
    a.R = len(a.Jr)
    a.arrive, a.delivery = np.asarray(arrive, np.int32), np.asarray(delivery, np.int32)
    a.S = len(a.arrive)
    a.count = np.asarray([[1] * a.R] * a.S if count is None else count, np.int32).reshape(a.S, a.R)
    a.power = np.asarray(power, np.int32).reshape(a.K, a.M)
    a.idle_power = np.asarray(idle_power, np.int32)
    a.bk_n = np.asarray([len(w) for w in windows], np.int32)
    a.bk = np.asarray([v for w in windows for pair in w for v in pair], np.int32).reshape(-1, 2)
    a.elig_n = (a.p > 0).sum(1).astype(np.int32)
    a.elig_list = np.zeros((a.K, a.M), np.int32)
    for k in range(a.K):
        e = np.flatnonzero(a.p[k])
        a.elig_list[k, :len(e)] = e
    a.ddt = 1.0
    a.name = "hand-made"
    return a


def hand_cases():
    """[(name, shop, plan rows (r, n, m), want table rows, want (makespan, tardiness, energy))]: one case per branch of the
    contract, the answers written out by hand."""
    cases = []
    # one machine, one job of one stage, p = 5, power 3, due 4
    one = lambda windows, due=4: shop([[5]], [[3]], [7], [windows], delivery=(due,))
    # a dispatch inside a window: t = 0 in (0, 4): begin 4, end 9; late by 5
    cases.append(("dispatch inside a window", one([(0, 4)]), [(0, 0, 0)], [(0, 0, 0, 0, 4, 9)], (9, 5, 15)))
    # a window inside the operation: (2, 6) stretches end 5 -> 9, begin stays 0
    cases.append(("window inside an operation", one([(2, 6)]), [(0, 0, 0)], [(0, 0, 0, 0, 0, 9)], (9, 5, 15)))
    # a machine without windows; the first task of a machine pays no idle energy
    cases.append(("no windows, first task", one([]), [(0, 0, 0)], [(0, 0, 0, 0, 0, 5)], (5, 1, 15)))
    # an extension that runs into the next window: (3, 5) -> end 7, then (6, 10) lies inside -> end 11
    cases.append(("extension into the next window", one([(3, 5), (6, 10)]), [(0, 0, 0)], [(0, 0, 0, 0, 0, 11)], (11, 7, 15)))
    # file order and the stop: the later window (20, 30) stands first and stops the walk (20 > 5): (2, 6) is never seen
    cases.append(("later window listed first", one([(20, 30), (2, 6)]), [(0, 0, 0)], [(0, 0, 0, 0, 0, 5)], (5, 1, 15)))
    # ... while in time order the same windows stretch the operation
    cases.append(("the same windows in time order", one([(2, 6), (20, 30)]), [(0, 0, 0)], [(0, 0, 0, 0, 0, 9)], (9, 5, 15)))
    # a window starting exactly at the end.  Two machines, kind 0 with two stages, kind 1 with one; p: stage (0,0) 5 on m0;
    # stage (0,1) 2 on m1; stage (1,0) 3 on m0.  m0 has window (5, 8): row 0 ends at 5, the machine at 8.  The job's next
    # stage on m1 waits for 8 (8..10), the next row on m0 too (8..11), but end = 5 stands in the table.  Due 5 for all:
    # tardiness = (10 - 5) + (11 - 5) = 11, none from row 0's machine end.  Energy: 5*2 + 2*4 + 3*6 = 36 working;
    # idle on m0: (t = 8) - (last_end = 5) = 3 at idle power 10 = 30; m1's first task pays none: 66.
    two = shop([[5, 0], [0, 2], [3, 0]], [[2, 0], [0, 4], [6, 0]], [10, 100], [[(5, 8)], []], Jr=[2, 1], delivery=(5,))
    cases.append(("window starting exactly at the end", two, [(0, 0, 0), (0, 0, 1), (1, 0, 0)],
                  [(0, 0, 0, 0, 0, 5), (0, 1, 0, 1, 8, 10), (1, 0, 0, 0, 8, 11)], (11, 11, 66)))
    # ... and at a job's last stage the tardiness is that of the table's end: 5 - 4 = 1, not 8 - 4
    cases.append(("window starting exactly at the last stage's end", one([(5, 8)]), [(0, 0, 0)], [(0, 0, 0, 0, 0, 5)], (5, 1, 15)))
    # idle energy is measured to the dispatch time, not to the shifted begin: two jobs of one stage on one machine, window
    # (6, 9): row 0 0..5 (the walk stops at 6 > 5, machine end 5); job 1 arrives with order 1 at 7, t = 7 in (6, 9): begin 9,
    # end 14, gap = 7 - 5 = 2 (not 9 - 5)
    gap = shop([[5]], [[3]], [7], [[(6, 9)]], count=[[1], [1]], arrive=(0, 7), delivery=(5, 20))
    cases.append(("idle gap to the dispatch time", gap, [(0, 0, 0), (0, 1, 0)], [(0, 0, 0, 0, 0, 5), (0, 0, 1, 0, 9, 14)], (14, 0, 15 + 15 + 2 * 7)))
    return cases
