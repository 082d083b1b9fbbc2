"""Plain numpy statement of fjsp_schedule_decode_active (include/fjsp_amd.h): explicit schedules decoded with insertion
into machine gaps -> times, objectives, status codes and the count of inserted rows, with the moves.  Written from the
entry point's contract -- per machine a list of busy intervals in ascending begin order, walked FROM THE FIRST -- on top
of decode_reference (moved, plan_length), critical_reference (the pair move's materialised plan) and
deep_reinforcement_learning_for_fjsp_amd.schedule (order_of_jobs, due_dates), independently of the kernel, which walks the
lists from the back; the tests of the kernel compare with it bit for bit.

is_active is the definition the decoder is named after, checked by brute force on a finished table."""
import numpy as np

from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
from tests import critical_reference as R
from tests import decode_reference as D

OK, NO_JOB, STAGES, MACHINE, BAD_MOVE = range(5)
KEYS = ("objective", "status", "table", "length", "inserted")


def moved(plan, move):
    """(rows of the moved plan up to its end, ok) for every kind the decoder takes: 0, 1, 2 as decode_reference.moved, 4 as
    critical_reference materialises it; ok False = status 4."""
    if move is not None and int(move[0]) == R.MOVE_PAIR:
        if not R.pair_ok(plan, move):
            return np.asarray(plan, np.int64).reshape(-1, 3)[:D.plan_length(plan)].copy(), False
        made = R.materialise_pair(plan, move)
        return made[:D.plan_length(made)].astype(np.int64), True
    return D.moved(plan, move)


def decode_one(inst, variant, plan, move=None, cap=None):
    """dict(status, objective int64[2], table int32[cap][6], length, inserted) of one candidate."""
    plan = np.asarray(plan, np.int64).reshape(-1, 3)
    cap = len(plan) if cap is None else cap
    fail = lambda code: dict(status=code, objective=np.array([-1, -1], np.int64), table=np.full((cap, 6), -1, np.int32), length=0,
                             inserted=0)
    rows, ok = moved(plan, move)
    if not ok:
        return fail(BAD_MOVE)
    Jr = np.asarray(inst.Jr, np.int64)
    p = np.asarray(inst.p, np.int64)
    koff = np.concatenate(([0], np.cumsum(Jr)))
    arrive = np.asarray(inst.arrive, np.int64)
    orders = sch.order_of_jobs(inst)
    due = sch.due_dates(inst, variant)
    R_, M = len(Jr), p.shape[1]
    ready = [arrive[orders[r]].copy() for r in range(R_)]
    stage = [np.zeros(len(orders[r]), np.int64) for r in range(R_)]
    busy = [[] for _ in range(M)]                                          # per machine: (begin, end), ascending begin
    table = np.full((cap, 6), -1, np.int32)
    makespan = tard = inserted = 0
    for t, (r, n, m) in enumerate(rows.tolist()):
        if not (0 <= r < R_ and 0 <= n < len(orders[r])):
            return fail(NO_JOB)
        j = int(stage[r][n])
        if j >= Jr[r]:
            return fail(STAGES)
        if not (0 <= m < M) or p[koff[r] + j, m] <= 0:
            return fail(MACHINE)
        d, s = int(p[koff[r] + j, m]), int(ready[r][n])
        at = len(busy[m])
        for i, (b, e) in enumerate(busy[m]):
            if s + d <= b:
                at = i
                break
            s = max(s, e)
        inserted += at < len(busy[m])
        busy[m].insert(at, (s, s + d))
        ready[r][n] = s + d
        stage[r][n] = j + 1
        makespan = max(makespan, s + d)
        if j == Jr[r] - 1:
            tard += max(0, s + d - int(due[r][n]))
        table[t] = (r, j, n, m, s, s + d)
    if any(np.any(stage[r] != Jr[r]) for r in range(R_)):
        return fail(STAGES)
    return dict(status=OK, objective=np.array([makespan, tard], np.int64), table=table, length=len(rows), inserted=int(inserted))


def decode(insts, variant, plan, moves=None, n_cand=1, cap=None):
    """The entry point on a batch, as decode_reference.decode: insts[i] is env i's instance; plan int[N][cap][3] or
    [N][n_cand][cap][3]; moves None or int[N][n_cand][3].  decode_reference.decode's dict and inserted int32[N][n_cand]."""
    plan = np.asarray(plan)
    N = len(insts)
    cap = plan.shape[-2] if cap is None else cap
    out = dict(objective=np.zeros((N, n_cand, 2), np.int64), status=np.zeros((N, n_cand), np.int32),
               table=np.zeros((N, n_cand, cap, 6), np.int32), length=np.zeros((N, n_cand), np.int32),
               inserted=np.zeros((N, n_cand), np.int32))
    for i in range(N):
        for q in range(n_cand):
            one = decode_one(insts[i], variant, plan[i] if plan.ndim == 3 else plan[i, q], None if moves is None else moves[i][q], cap)
            for key in out:
                out[key][i, q] = one[key]
    return out


def begin_ordered_plan(table, cap=None):
    """int32[cap][3]: the plan of a table's rows sorted stably by begin (schedule.begin_order on one table, in numpy)."""
    rows = np.asarray(table, np.int64).reshape(-1, 6)
    rows = rows[:R.table_length(rows)]
    return D.plan_from_table(rows[np.argsort(rows[:, 4], kind="stable")], len(np.asarray(table).reshape(-1, 6)) if cap is None else cap)


def is_active(inst, table):
    """True iff no operation of the table could start earlier with every other operation where it is: at no time t' in
    [end of its job predecessor, or its order's arrival; its begin) is its machine idle throughout [t', t' + d).  If any
    such t' exists the least one is the lower bound itself or the end of another operation on the machine (an earlier start
    could slide left until it meets one of them), so those are the times tried, each against every other operation of the
    machine."""
    rows = np.asarray(table, np.int64).reshape(-1, 6)
    rows = rows[:R.table_length(rows)]
    arrive = np.asarray(inst.arrive, np.int64)
    orders = sch.order_of_jobs(inst)
    end_of = {(r, j, n): e for r, j, n, m, b, e in rows.tolist()}
    on = {}
    for i, (r, j, n, m, b, e) in enumerate(rows.tolist()):
        on.setdefault(m, []).append((b, e, i))
    for i, (r, j, n, m, b, e) in enumerate(rows.tolist()):
        low = end_of[(r, j - 1, n)] if j > 0 else int(arrive[orders[r][n]])
        others = [(ob, oe) for ob, oe, oi in on[m] if oi != i and oe > low and ob < e]   # (the rest cannot meet [low, e))
        for t in [low] + [oe for _, oe in others]:
            if low <= t < b and all(t + (e - b) <= ob or oe <= t for ob, oe in others):
                return False
    return True
