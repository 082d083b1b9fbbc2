"""Plain numpy statement of fjsp_schedule_decode (include/fjsp_amd.h): explicit schedules -> times, objectives and
status codes, with the moves.  Written from the entry point's contract and deep_reinforcement_learning_for_fjsp_amd.schedule
(order_of_jobs, due_dates), independently of the kernel; the tests of the kernel compare with it bit for bit.

A plan is int[cap][3] rows (r, n, m) in sequence order and ends at its first row of three -1.  A move is (kind, u, m_new):
0 nothing, 1 row u runs on m_new, 2 rows u and u + 1 change places unless they are rows of one job."""
import numpy as np

from deep_reinforcement_learning_for_fjsp_amd import schedule as sch

OK, NO_JOB, STAGES, MACHINE, BAD_MOVE = range(5)


def plan_length(plan):
    plan = np.asarray(plan, np.int64).reshape(-1, 3)
    end = np.flatnonzero((plan == -1).all(1))
    return int(end[0]) if len(end) else len(plan)


def moved(plan, move):
    """(rows of the moved plan up to its end, ok): ok False = status 4 (unknown kind, u or u + 1 outside the plan)."""
    plan = np.asarray(plan, np.int64).reshape(-1, 3)
    rows = plan[:plan_length(plan)].copy()
    L = len(rows)
    if move is None:
        return rows, True
    kind, u, m_new = (int(v) for v in move)
    if kind == 0:
        return rows, True
    if kind == 1:
        if not 0 <= u < L:
            return rows, False
        rows[u, 2] = m_new
        return rows, True
    if kind == 2:
        if not (0 <= u and u + 1 < L):
            return rows, False
        if not (rows[u, 0] == rows[u + 1, 0] and rows[u, 1] == rows[u + 1, 1]):
            rows[[u, u + 1]] = rows[[u + 1, u]]
        return rows, True
    return rows, False


def materialise(plan, move, cap=None):
    """The moved plan as int32[cap][3] with -1 rows past its end (what schedule.apply_moves builds); a refused move
    leaves the plan as it is."""
    rows, _ = moved(plan, move)
    cap = len(np.asarray(plan).reshape(-1, 3)) if cap is None else cap
    out = np.full((cap, 3), -1, np.int32)
    out[:len(rows)] = rows
    return out


def decode_one(inst, variant, plan, move=None, cap=None):
    """dict(status, objective int64[2], table int32[cap][6], length) of one candidate."""
    plan = np.asarray(plan, np.int64).reshape(-1, 3)
    cap = len(plan) if cap is None else cap
    fail = lambda code: dict(status=code, objective=np.array([-1, -1], np.int64), table=np.full((cap, 6), -1, np.int32), length=0)
    rows, ok = moved(plan, move)
    if not ok:
        return fail(BAD_MOVE)
    Jr = np.asarray(inst.Jr, np.int64)
    p = np.asarray(inst.p, np.int64)
    koff = np.concatenate(([0], np.cumsum(Jr)))
    arrive = np.asarray(inst.arrive, np.int64)
    orders = sch.order_of_jobs(inst)
    due = sch.due_dates(inst, variant)
    R, M = len(Jr), p.shape[1]
    ready = [arrive[orders[r]].copy() for r in range(R)]
    stage = [np.zeros(len(orders[r]), np.int64) for r in range(R)]
    free = np.zeros(M, np.int64)
    table = np.full((cap, 6), -1, np.int32)
    makespan = tard = 0
    for t, (r, n, m) in enumerate(rows.tolist()):
        if not (0 <= r < R and 0 <= n < len(orders[r])):
            return fail(NO_JOB)
        j = int(stage[r][n])
        if j >= Jr[r]:
            return fail(STAGES)
        if not (0 <= m < M) or p[koff[r] + j, m] <= 0:
            return fail(MACHINE)
        begin = max(int(ready[r][n]), int(free[m]))
        end = begin + int(p[koff[r] + j, m])
        ready[r][n] = free[m] = end
        stage[r][n] = j + 1
        makespan = max(makespan, end)
        if j == Jr[r] - 1:
            tard += max(0, end - int(due[r][n]))
        table[t] = (r, j, n, m, begin, end)
    if any(np.any(stage[r] != Jr[r]) for r in range(R)):
        return fail(STAGES)
    return dict(status=OK, objective=np.array([makespan, tard], np.int64), table=table, length=len(rows))


def decode(insts, variant, plan, moves=None, n_cand=1, cap=None):
    """The entry point on a batch: insts[i] is env i's instance; plan int[N][cap][3] or [N][n_cand][cap][3]; moves None or
    int[N][n_cand][3].  dict(objective int64[N][n_cand][2], status int32[N][n_cand], table int32[N][n_cand][cap][6],
    length int32[N][n_cand])."""
    plan = np.asarray(plan)
    N = len(insts)
    cap = plan.shape[-2] if cap is None else cap
    out = dict(objective=np.zeros((N, n_cand, 2), np.int64), status=np.zeros((N, n_cand), np.int32),
               table=np.zeros((N, n_cand, cap, 6), np.int32), length=np.zeros((N, n_cand), np.int32))
    for i in range(N):
        for q in range(n_cand):
            one = decode_one(insts[i], variant, plan[i] if plan.ndim == 3 else plan[i, q], None if moves is None else moves[i][q], cap)
            for key in out:
                out[key][i, q] = one[key]
    return out


def plan_from_table(table, cap=None):
    """int32[cap][3] plan of a table's rows (r, j, n, m, begin, end)."""
    table = np.asarray(table).reshape(-1, 6)
    cap = len(table) if cap is None else cap
    out = np.full((cap, 3), -1, np.int32)
    out[:len(table)] = table[:, [0, 2, 3]]
    return out


def random_plan(inst, rs, cap=None):
    """A random feasible plan of `inst`: a uniform interleaving of the jobs' operations, a uniform eligible machine each."""
    Jr = np.asarray(inst.Jr, np.int64)
    p = np.asarray(inst.p, np.int64)
    koff = np.concatenate(([0], np.cumsum(Jr)))
    orders = sch.order_of_jobs(inst)
    seq = [(r, n) for r in range(len(Jr)) for n in range(len(orders[r])) for _ in range(int(Jr[r]))]
    seq = [seq[i] for i in rs.permutation(len(seq))]
    stage, rows = {}, []
    for r, n in seq:
        j = stage.get((r, n), 0)
        stage[(r, n)] = j + 1
        rows.append((r, n, int(rs.choice(np.flatnonzero(p[koff[r] + j] > 0)))))
    cap = len(rows) if cap is None else cap
    out = np.full((cap, 3), -1, np.int32)
    out[:len(rows)] = rows
    return out
