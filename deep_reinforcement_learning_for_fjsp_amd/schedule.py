"""Host-side use of a recorded schedule (EnvBatch.schedule / fjsp_env_schedule).  Pure numpy.

A table row is one dispatched operation, (r, j, n, m, time_begin, time_end): kind r, stage j, job number n within
kind r (counted over all orders, class_FJSSP.py:212-216), machine m and the task's start and end as the reference's
dispatch sets them (SO_FJSSP.py:176-196, shifted by machine breakdowns in MO_DFJSP_breakdown.py:203-247).

    rows(table, length, i)                      one env's rows, grouped per machine in start order (machine.task_list)
    validate(inst, rows, variant, breakdowns)   feasibility check; returns the list of violations (empty: feasible)
    objectives(inst, rows, variant)             makespan / completion time and total tardiness (delay_time_sum)

`inst` is anything with the instance arrays of instances.InstanceArrays: Jr[R], p[K][M] (0 = ineligible),
count[S][R], arrive[S], delivery[S] (and bk_n[M], bk[W][2] for MO_DFJSP breakdown windows).
"""
import numpy as np

VARIANT_SO_SFJSP = 1
VARIANT_MO_DFJSP = 4
VARIANT_SO_DFJSP = 5

R_, J_, N_, M_, B_, E_ = range(6)


def _np(t):
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.asarray(t)


def rows(table, length, i):
    """Env i's schedule as int64 rows (r, j, n, m, begin, end): grouped per machine (ascending m), each machine's
    operations in start order -- the reference's machine.task_list (SO_FJSSP.py:196)."""
    table, length = _np(table), _np(length)
    n = int(length[i])
    t = table[i, :n].astype(np.int64)
    order = np.lexsort((np.arange(n), t[:, B_], t[:, M_]))      # machine, then start, then dispatch order
    return t[order]


def _count(inst):
    return np.asarray(inst.count, np.int64).reshape(len(np.asarray(inst.arrive)), len(np.asarray(inst.Jr)))


def _koff(inst):
    return np.concatenate(([0], np.cumsum(np.asarray(inst.Jr, np.int64))))


def order_of_jobs(inst):
    """order_of[r][n]: the order job n of kind r arrives with (jobs of kind r are numbered across orders in order)."""
    cnt = _count(inst)
    return [np.repeat(np.arange(cnt.shape[0]), cnt[:, r]) for r in range(cnt.shape[1])]


def due_dates(inst, variant):
    """due[r][n]: job (r, n)'s due date as the environment sets it (class_FJSSP.py:214-218: round(round(delivery * J_r /
    count) * n / count) with n counted over all orders; the order's delivery time for MO_DFJSP (class_MODFJSP.py:224) and
    SO_DFJSP (class_FJSP.py:229)).  Python's round: half to even, like np.rint."""
    cnt = _count(inst)
    Jr = np.asarray(inst.Jr, np.int64)
    delivery = np.asarray(inst.delivery, np.int64)
    out = []
    for r in range(cnt.shape[1]):
        d = []
        n = 0
        for s in range(cnt.shape[0]):
            c = int(cnt[s, r])
            if c == 0:
                continue
            r_due = int(np.rint(float(delivery[s] * Jr[r]) / float(c)))
            for _ in range(c):
                if variant in (VARIANT_MO_DFJSP, VARIANT_SO_DFJSP):
                    d.append(int(delivery[s]))
                else:
                    d.append(int(np.rint(float(r_due * n) / float(c))))
                n += 1
        out.append(np.array(d, np.int64))
    return out


def breakdowns_of(inst):
    """Breakdown windows per machine in file order, [(start, end), ...] (MO_DFJSP_instance_read.py:56-73), or None."""
    if not hasattr(inst, "bk_n"):
        return None
    bk = np.asarray(inst.bk, np.int64).reshape(-1, 2)
    out, q = [], 0
    for m in range(len(inst.bk_n)):
        c = int(inst.bk_n[m])
        out.append([tuple(int(v) for v in bk[q + i]) for i in range(c)])
        q += c
    return out


def shifted(windows, t, duration):
    """MO_DFJSP_breakdown.py:203-231: (time_begin, time_end) of a task of `duration` dispatched at t on a machine with
    these windows (file order)."""
    begin, end = t, t + duration
    for bs, be in windows:
        if bs <= t < be:
            begin += be - t
            end += be - t
        elif t < bs < end:
            end += be - bs
        elif bs == end:
            pass                       # only the machine's time_end moves
        elif bs > end:
            break
    return begin, end


def validate(inst, rows, variant, breakdowns=None):
    """Feasibility of one env's schedule.  Checks that every operation of every job appears exactly once, that the
    stages of a job run in order without overlapping, that the machine is eligible and end - begin == p[k][m] (with
    breakdown windows: that begin / end are what the windows make of some dispatch time), that no two operations
    overlap on a machine and that no job starts before its order arrives.  breakdowns: windows per machine
    (breakdowns_of); None takes the instance's own for MO_DFJSP.  Returns the list of violations (empty: feasible)."""
    rows = np.asarray(rows, np.int64).reshape(-1, 6)
    Jr = np.asarray(inst.Jr, np.int64)
    p = np.asarray(inst.p, np.int64)
    koff = _koff(inst)
    cnt = _count(inst)
    arrive = np.asarray(inst.arrive, np.int64)
    if breakdowns is None and variant == VARIANT_MO_DFJSP:
        breakdowns = breakdowns_of(inst)
    bad = []
    R, K, M = len(Jr), p.shape[0], p.shape[1]
    jobs = cnt.sum(0)
    seen = {}
    for i, (r, j, n, m, b, e) in enumerate(rows.tolist()):
        if not (0 <= r < R and 0 <= j < Jr[r] and 0 <= n < jobs[r] and 0 <= m < M):
            bad.append("row %d %s: no such operation / machine" % (i, (r, j, n, m, b, e)))
            continue
        if (r, j, n) in seen:
            bad.append("operation (r=%d, j=%d, n=%d) appears twice" % (r, j, n))
        seen[(r, j, n)] = (m, b, e)
        k = int(koff[r] + j)
        if p[k, m] <= 0:
            bad.append("operation (r=%d, j=%d, n=%d) on machine %d, which cannot process it" % (r, j, n, m))
            continue
        if breakdowns is None or not breakdowns[m]:
            if e - b != p[k, m]:
                bad.append("operation (r=%d, j=%d, n=%d) on machine %d takes %d, p = %d" % (r, j, n, m, e - b, p[k, m]))
        else:
            w = breakdowns[m]
            ok = shifted(w, b, int(p[k, m])) == (b, e) or any(be == b and shifted(w, bs, int(p[k, m])) == (b, e) for bs, be in w)
            if not ok:
                bad.append("operation (r=%d, j=%d, n=%d) on machine %d: (%d, %d) is no breakdown shift of p = %d"
                           % (r, j, n, m, b, e, p[k, m]))
    for r in range(R):
        for n in range(int(jobs[r])):
            for j in range(int(Jr[r])):
                if (r, j, n) not in seen:
                    bad.append("operation (r=%d, j=%d, n=%d) is missing" % (r, j, n))
    orders = order_of_jobs(inst)
    for (r, j, n), (m, b, e) in seen.items():
        if j == 0 and b < arrive[orders[r][n]]:
            bad.append("job (r=%d, n=%d) starts at %d, before its order arrives at %d" % (r, n, b, arrive[orders[r][n]]))
        nxt = seen.get((r, j + 1, n))
        if nxt is not None and nxt[1] < e:
            bad.append("job (r=%d, n=%d): stage %d starts at %d before stage %d ends at %d" % (r, n, j + 1, nxt[1], j, e))
    for m in range(M):
        on = sorted((b, e) for (m2, b, e) in seen.values() if m2 == m)
        for (b0, e0), (b1, e1) in zip(on, on[1:]):
            if b1 < e0:
                bad.append("machine %d: (%d, %d) overlaps (%d, %d)" % (m, b0, e0, b1, e1))
    return bad


def objectives(inst, rows, variant):
    """dict(makespan, completion_time, delay_time_sum) of one env's schedule: the latest task end (completion_time,
    MO_FJSSP_discretes.py:122; without breakdown windows also max(machine.time_end), SO_FJSSP.py:426), and the total
    tardiness of the jobs' last stages against their due dates (delay_time_sum at episode end, SO_FJSSP.py:200-202)."""
    rows = np.asarray(rows, np.int64).reshape(-1, 6)
    Jr = np.asarray(inst.Jr, np.int64)
    due = due_dates(inst, variant)
    end = int(rows[:, E_].max()) if len(rows) else 0
    tard = 0
    for r, j, n, m, b, e in rows.tolist():
        if j == Jr[r] - 1:
            tard += max(0, e - int(due[r][n]))
    return dict(makespan=end, completion_time=end, delay_time_sum=tard)


def from_trace(inst, k, m, job_n, step_time_after, t0=0):
    """Rows in dispatch order rebuilt from a per-step trace without breakdowns: chosen operation type k, machine m, job
    number, and the clock AFTER each step (the task starts at the clock before it: t0, then the previous step's)."""
    koff = _koff(inst)
    p = np.asarray(inst.p, np.int64)
    k = np.asarray(k, np.int64)
    r = np.searchsorted(koff, k, side="right") - 1
    j = k - koff[r]
    begin = np.concatenate(([t0], np.asarray(step_time_after, np.int64)[:-1]))
    end = begin + p[k, np.asarray(m, np.int64)]
    return np.stack([r, j, np.asarray(job_n, np.int64), np.asarray(m, np.int64), begin, end], 1)
