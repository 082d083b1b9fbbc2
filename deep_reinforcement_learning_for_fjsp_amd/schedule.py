"""Host-side use of a recorded schedule (EnvBatch.schedule / fjsp_env_schedule), pure numpy, and the way back:
explicit schedules decoded on the device (plan_of / decode / apply_moves, fjsp_schedule_decode) and their critical paths
(critical / begin_order, fjsp_schedule_critical).

A table row is one dispatched operation, (r, j, n, m, time_begin, time_end): kind r, stage j, job number n within
kind r (counted over all orders, class_FJSSP.py:212-216), machine m and the task's start and end as the reference's
dispatch sets them (SO_FJSSP.py:176-196, shifted by machine breakdowns in MO_DFJSP_breakdown.py:203-247).

    rows(table, length, i)                      one env's rows, grouped per machine in start order (machine.task_list)
    validate(inst, rows, variant, breakdowns)   feasibility check; returns the list of violations (empty: feasible)
    objectives(inst, rows, variant)             makespan / completion time and total tardiness (delay_time_sum)
    plan_of(table)                              the (r, n, m) columns of a table: the explicit schedule it records
    decode(batch, plan, moves, n_cand)          times and objectives of explicit schedules, on the device
    decode_dyn(batch, plan, moves, n_cand)      the same on MO_DFJSP: breakdown shifts, and energy as a third objective
    decode_active(batch, plan, moves, n_cand)   decode with insertion into machine gaps (active schedules), and the rows inserted
    apply_moves(plan, moves)                    the plans that decode's moves stand for, materialised
    pair_move(u, v, w)                          the MOVE_PAIR that puts rows u and v, v first, behind row w
    critical(batch, table, n_cand, max_moves)   tails, critical flags, one critical path and its moves, on the device
    begin_order(table)                          the same schedule with its rows sorted by begin: (plan, table)
    search(batch, plan, rounds, n_cand, ...)    hill climbing / tabu search, all rounds in one launch (fjsp_schedule_search)
    search_dyn(batch, plan, rounds, n_cand, ...) the same on MO_DFJSP: uniform neighbourhood, energy as a third objective
    search_front(batch, plan, weights, ...)     that search steered by a weighted sum, keeping the Pareto archive of its decodes
    search_draws(seed, env, first, n)           the draw stream of that search, on the host
    evolve(batch, pop_plans, generations, ...)  a genetic algorithm on populations of plans, all generations in one launch
    evolve_active(batch, pop_plans, ...)        evolve with every individual scored by the active decoder, and the rows inserted

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


# ---- explicit schedules on the device (fjsp_schedule_decode, csrc/fjsp_decode.hip)
MOVE_NONE, MOVE_MACHINE, MOVE_SWAP = 0, 1, 2
MOVE_PAIR = 4                                   # (3 is no kind: decode refuses it)
PAIR_DW_MAX = 32767                             # dw of a MOVE_PAIR's dv | dw << 16: the field is a non-negative int32
DECODE_OK, DECODE_NO_JOB, DECODE_STAGES, DECODE_MACHINE, DECODE_BAD_MOVE = range(5)


def plan_of(table):
    """The explicit schedule a table records: its (r, n, m) columns, rows in dispatch order, -1 rows past the end.  A
    slice of `table` (device tensor or numpy array) of shape [..., cap, 3]; the stage column is implied by the order."""
    return table[..., [R_, N_, M_]]


def _plan_length(plan):
    """Rows in front of the first row of three -1, per plan: int64[...]."""
    import torch
    end = (plan == -1).all(-1)
    cap = plan.shape[-2]
    pos = torch.arange(cap, device=plan.device).expand(end.shape)
    return torch.where(end, pos, torch.full_like(pos, cap)).amin(-1)


def apply_moves(plan, moves):
    """The plans decode(batch, plan, moves) decodes, materialised with tensor indexing.  plan: int32[N, cap, 3] (one
    parent per env) or [N, Q, cap, 3]; moves: int32[N, Q, 3] = (kind, u, m_new).  Returns int32[N, Q, cap, 3].  Kind 1
    sets row u's machine, kind 2 exchanges rows u and u + 1 unless they are rows of one job, kind 4 (pair_move) puts rows
    u and v, v first, behind row w; a move decode refuses (status 4: unknown kind, u or v outside the plan, a third field
    that is no dv | dw << 16 with 1 <= dv, 0 <= dw < dv -- a negative field, which is what dw > 32767 makes of an int32,
    included) leaves its plan as it is.  Rows may carry further columns
    behind the three (improve keeps each row's operation type there): they move with their rows."""
    import torch
    moves = torch.as_tensor(moves, device=plan.device).to(torch.int64)
    N, Q = moves.shape[0], moves.shape[1]
    out = (plan[:, None].expand(N, Q, *plan.shape[1:]) if plan.dim() == 3 else plan).clone()
    if out.dim() != 4 or tuple(out.shape[:2]) != (N, Q) or out.shape[3] < 3:
        raise ValueError("plan must be [N, cap, 3] or [N, Q, cap, 3] with moves [N, Q, 3]")
    L = _plan_length(out[..., :3])
    kind, u, m_new = moves[..., 0], moves[..., 1], moves[..., 2]
    i, q = torch.meshgrid(torch.arange(N, device=out.device), torch.arange(Q, device=out.device), indexing="ij")
    ok1 = (kind == MOVE_MACHINE) & (u >= 0) & (u < L)
    out[i[ok1], q[ok1], u[ok1], 2] = m_new[ok1].to(out.dtype)
    ok2 = (kind == MOVE_SWAP) & (u >= 0) & (u + 1 < L)
    i2, q2, u2 = i[ok2], q[ok2], u[ok2]
    a, b = out[i2, q2, u2], out[i2, q2, u2 + 1]
    other = ~((a[:, 0] == b[:, 0]) & (a[:, 1] == b[:, 1]))
    i2, q2, u2, a, b = i2[other], q2[other], u2[other], a[other], b[other]
    out[i2, q2, u2] = b
    out[i2, q2, u2 + 1] = a
    dv, dw = m_new & 0xFFFF, m_new >> 16
    ok4 = (kind == MOVE_PAIR) & (m_new >= 0) & (dv >= 1) & (dw < dv) & (u >= 0) & (u + dv < L)
    pu, pw, pv = u[..., None], (u + dw)[..., None], (u + dv)[..., None]
    t = torch.arange(out.shape[2], device=out.device).expand(N, Q, -1)
    src = torch.where(t < pw, t + 1, torch.where(t == pw, pv, torch.where(t == pw + 1, pu, t - 1)))
    src = torch.where(ok4[..., None] & (t >= pu) & (t <= pv), src, t)           # position t of the moved plan is old row src
    return torch.gather(out, 2, src[..., None].expand(-1, -1, -1, out.shape[3]))


def pair_move(u, v, w):
    """The MOVE_PAIR (4, u, dv | dw << 16) that takes rows u and v = u + dv out of the plan and puts them, v first,
    directly behind old row w = u + dw, u <= w < v (w = u: v in front of u; w = v - 1: u behind v).  Integers give a tuple,
    tensors / arrays a stacked [..., 3] of their kind.  The third field is a non-negative int32, so w <= u + PAIR_DW_MAX
    (32767) besides v <= u + 65535: ValueError unless 0 <= u <= w < v <= u + 65535 and w - u <= 32767, for integers and
    for every element of a tensor / array (checking a device tensor synchronises)."""
    if all(isinstance(x, (int, np.integer)) for x in (u, v, w)):
        u, v, w = int(u), int(v), int(w)
        if not (0 <= u <= w < v <= u + 65535 and w - u <= PAIR_DW_MAX):
            raise ValueError("pair_move needs 0 <= u <= w < v <= u + 65535 and w - u <= %d, got %r" % (PAIR_DW_MAX, (u, v, w)))
        return (MOVE_PAIR, u, (v - u) | ((w - u) << 16))
    ref = next((x for x in (u, v, w) if hasattr(x, "new_full")), None)
    if ref is not None:                                          # (a scalar among tensors takes their dtype and device)
        import torch
        u, v, w = torch.broadcast_tensors(*(x if hasattr(x, "new_full") else torch.as_tensor(x, dtype=ref.dtype, device=ref.device)
                                            for x in (u, v, w)))
        dv, dw = v.to(torch.int64) - u, w.to(torch.int64) - u
    else:
        ref = next((x for x in (u, v, w) if isinstance(x, np.ndarray)), None)
        u, v, w = np.broadcast_arrays(*(x if isinstance(x, np.ndarray) else np.asarray(x, None if ref is None else ref.dtype)
                                        for x in (u, v, w)))
        dv, dw = v.astype(np.int64) - u, w.astype(np.int64) - u
    if not bool(((u >= 0) & (dw >= 0) & (dw < dv) & (dv <= 65535) & (dw <= PAIR_DW_MAX)).all()):
        raise ValueError("pair_move needs 0 <= u <= w < v <= u + 65535 and w - u <= %d in every element" % PAIR_DW_MAX)
    third = (dv | (dw << 16)).to(u.dtype) if hasattr(dv, "new_full") else (dv | (dw << 16)).astype(u.dtype)
    if hasattr(third, "new_full"):
        return torch.stack([torch.full_like(third, MOVE_PAIR), u + 0 * third, third], -1)
    return np.stack([np.full_like(third, MOVE_PAIR), u + 0 * third, third], -1)


def decode(batch, plan, moves=None, n_cand=1, want_table=False):
    """Times and objectives of explicit schedules on the device (fjsp_schedule_decode): n_cand candidates per env of
    `batch` (an EnvBatch or a Batched* wrapper), each decoded on its env's instance; the envs' episodes are not touched.

    plan: int32[N, cap, 3] -- one parent plan per env, shared by its candidates -- or [N, n_cand, cap, 3]; rows (r, n, m)
    in sequence order, -1 rows past the end, cap = batch.decode_capacity().  moves: None or int32[N, n_cand, 3] = (kind,
    u, m_new), applied while the plan is read (MOVE_NONE, MOVE_MACHINE, MOVE_SWAP, MOVE_PAIR with m_new = dv | dw << 16,
    dw <= 32767: a negative third field is refused, status 4).
    Returns dict(objective=int64[N, n_cand, 2] (makespan, total tardiness), status=int32[N, n_cand] (DECODE_*),
    table=int32[N, n_cand, cap, 6] or None, length=int32[N, n_cand]), device tensors; a failed candidate has objective -1,
    length 0 and a table of -1.  ValueError for shapes that do not fit; FjspError where the library refuses (MO_DFJSP, which
    decode_dyn decodes; an instance whose per-candidate state exceeds the limit of include/fjsp_amd.h)."""
    return _decode(batch, plan, moves, n_cand, want_table, "fjsp_schedule_decode", 2)


def decode_dyn(batch, plan, moves=None, n_cand=1, want_table=False):
    """decode on a MO_DFJSP batch (fjsp_schedule_decode_dyn): the same arguments, checks, status codes and results, the
    times shifted by the machines' breakdown windows as MO_DFJSP_breakdown.py:203-247 shifts them, and objective=int64[N,
    n_cand, 3] = (makespan, total tardiness, energy), -1 on failure.  Every operation is dispatched at max(its job's
    release, its machine's end); the contract is in include/fjsp_amd.h.  FjspError on a batch that is not MO_DFJSP.
    Energy is an objective of the decode only: objectives() cannot compute it from a table, because a dispatch that a
    window swallows leaves its dispatch time, which the idle energy is measured to, in no row."""
    return _decode(batch, plan, moves, n_cand, want_table, "fjsp_schedule_decode_dyn", 3)


def decode_active(batch, plan, moves=None, n_cand=1, want_table=False):
    """decode with insertion into machine gaps (fjsp_schedule_decode_active), the active decoder of the FJSP literature:
    the same arguments, checks, moves, status codes and results, but a row starts in the earliest idle interval of its
    machine that is long enough and begins no earlier than its job is ready, not behind everything the machine holds.  No
    row ends later than in decode's table of the same plan.  The table's rows stand at their plan positions, so it is not in
    begin order: begin_order(table) gives the plan that decode decodes to the same schedule.
    Returns decode's dict and inserted=int32[N, n_cand], the rows placed in front of an interval already on their machine
    (0 for a failed candidate; where it is 0 the table is decode's).  The calls on one batch share a device workspace:
    issue them on one stream.  FjspError on MO_DFJSP (an insertion under breakdown shifts is not defined)."""
    return _decode(batch, plan, moves, n_cand, want_table, "fjsp_schedule_decode_active", 2)


def _decode(batch, plan, moves, n_cand, want_table, entry, n_obj):
    import torch
    from ._capi import check, ptr
    b = getattr(batch, "batch", batch)
    n_cand = int(n_cand)
    if n_cand < 1:
        raise ValueError("n_cand must be at least 1")
    cap = int(b._lib.fjsp_schedule_decode_capacity(b._h))
    if not torch.is_tensor(plan):
        plan = torch.as_tensor(np.asarray(plan))
    if plan.dim() == 3 and tuple(plan.shape) == (b.N, cap, 3):
        q_plans = 1
    elif plan.dim() == 4 and tuple(plan.shape) == (b.N, n_cand, cap, 3):
        q_plans = n_cand
    else:
        raise ValueError("plan must have shape %s or %s, got %s" % ((b.N, cap, 3), (b.N, n_cand, cap, 3), tuple(plan.shape)))
    plan = plan.to(device=b.device, dtype=torch.int32).contiguous()
    if moves is not None:
        if not torch.is_tensor(moves):
            moves = torch.as_tensor(np.asarray(moves))
        if tuple(moves.shape) != (b.N, n_cand, 3):
            raise ValueError("moves must have shape %s, got %s" % ((b.N, n_cand, 3), tuple(moves.shape)))
        moves = moves.to(device=b.device, dtype=torch.int32).contiguous()
    objective = torch.empty(b.N, n_cand, n_obj, dtype=torch.int64, device=b.device)
    status = torch.empty(b.N, n_cand, dtype=torch.int32, device=b.device)
    length = torch.empty(b.N, n_cand, dtype=torch.int32, device=b.device)
    table = torch.empty(b.N, n_cand, cap, 6, dtype=torch.int32, device=b.device) if want_table else None
    out = dict(objective=objective, status=status, table=table, length=length)
    more = ()
    if entry == "fjsp_schedule_decode_active":
        out["inserted"] = torch.empty(b.N, n_cand, dtype=torch.int32, device=b.device)
        more = (ptr(out["inserted"]),)
    check(getattr(b._lib, entry)(b._h, ptr(plan), q_plans, ptr(moves), n_cand, ptr(objective), ptr(status), ptr(table), ptr(length), *more, b._stream()))
    return out


CRITICAL_OK, CRITICAL_BAD_ROW, CRITICAL_EMPTY = range(3)
FLAG_CRITICAL, FLAG_PATH, FLAG_MACHINE_ARC = 1, 2, 4


def critical(batch, table, n_cand=1, max_moves=0):
    """Critical paths of decoded schedules on the device (fjsp_schedule_critical): n_cand tables per env of `batch`, one
    lane per table; the envs' episodes are not touched.

    table: int32[N, cap, 6] (n_cand = 1) or [N, n_cand, cap, 6], rows (r, stage, n, m, begin, end) as decode(...,
    want_table=True) and EnvBatch.schedule() write them, -1 rows past the end.  The arcs are those of the table's own
    order: a row's job (machine) predecessor is the latest row in front of it of the same job (on the same machine).
    Returns a dict of device tensors, [N, n_cand] in front of every shape:
      makespan int32 -- C, the largest end;  status int32 -- CRITICAL_OK, CRITICAL_BAD_ROW (a row fails a range check),
      CRITICAL_EMPTY; with the latter two tail, path and makespan are -1 and everything else is 0;
      tail int32[cap] -- the work that must follow a row: max over its job and its machine successor of their tail + their
      duration, 0 without a successor, -1 past the table;  flags uint8[cap] -- FLAG_CRITICAL (end + tail = C) |
      FLAG_PATH | FLAG_MACHINE_ARC (joined to its path successor by a machine arc);
      path int32[cap], path_len int32 -- row indices from the first row that ends at C backwards, each step to the tight
      predecessor (end = begin) that stands later in the table, a row that is both predecessors as a job arc;
      moves int32[max_moves, 3], n_moves, skipped int32 -- the path's neighbourhood for decode: a MOVE_PAIR per machine arc
      of the path that exchanges its two operations on their machine, then a MOVE_MACHINE per path operation and other
      eligible machine; n_moves counts them all, the first max_moves are written, MOVE_NONE behind them; skipped counts
      the machine arcs that no pair move expresses: w not in front of the first row of a's job in (u, v), or w - u >
      32767, which the move's third field cannot carry (see begin_order: neither happens in a begin-ordered table).
    ValueError for shapes that do not fit; FjspError where the library refuses, as decode."""
    import torch
    from ._capi import check, ptr
    b = getattr(batch, "batch", batch)
    n_cand, max_moves = int(n_cand), int(max_moves)
    if n_cand < 1 or max_moves < 0:
        raise ValueError("critical needs n_cand >= 1 and max_moves >= 0")
    cap = int(b._lib.fjsp_schedule_decode_capacity(b._h))
    if not torch.is_tensor(table):
        table = torch.as_tensor(np.asarray(table))
    if tuple(table.shape) not in ((b.N, n_cand, cap, 6),) + (((b.N, cap, 6),) if n_cand == 1 else ()):
        raise ValueError("table must have shape %s, got %s" % ((b.N, n_cand, cap, 6), tuple(table.shape)))
    table = table.to(device=b.device, dtype=torch.int32).contiguous()
    new = lambda *shape, dtype=torch.int32: torch.empty((b.N, n_cand) + shape, dtype=dtype, device=b.device)
    out = dict(tail=new(cap), flags=new(cap, dtype=torch.uint8), path=new(cap), path_len=new(), moves=new(max_moves, 3),
               n_moves=new(), skipped=new(), status=new(), makespan=new())
    check(b._lib.fjsp_schedule_critical(b._h, ptr(table), n_cand, ptr(out["tail"]), ptr(out["flags"]), ptr(out["path"]),
                                        ptr(out["path_len"]), ptr(out["moves"]) if max_moves else None, max_moves, ptr(out["n_moves"]),
                                        ptr(out["skipped"]), ptr(out["status"]), ptr(out["makespan"]), b._stream()))
    return out


def begin_order(table):
    """(plan, table) with the rows of every table stably sorted by begin, -1 rows left at the end; table: int32[..., cap,
    6], a device tensor or an array, as decode writes it.  Two facts make this the form to search from.  It is the same
    schedule: along every job arc and every machine arc begin increases strictly, because p > 0, so the sorted plan
    keeps every job's and every machine's sequence and decodes to the same times.  And in this order critical() skips no
    machine arc a -> b: the last row of b's job between them begins before b does, the first row of a's job between them
    begins no earlier than b, so the former stands in front of the latter and the pair move exists.  Its dw fits: the rows
    between a and b all begin within a's duration, at most p_a + 1 of them per machine, and create's clock rule keeps p
    at 508 at most on any instance of more than 32 768 operations (MOVE_PAIR), so v - u <= 32 x 509 = 16 288."""
    import torch
    if not torch.is_tensor(table):
        table = torch.as_tensor(np.asarray(table))
    end = (table == -1).all(-1)
    key = torch.where(end, torch.full_like(table[..., B_], torch.iinfo(table.dtype).max), table[..., B_])
    order = torch.sort(key, dim=-1, stable=True).indices
    table = torch.gather(table, -2, order[..., None].expand(table.shape))
    return plan_of(table), table


SEARCH_OBJECTIVES = ("makespan", "tardiness")
SEARCH_DYN_OBJECTIVES = ("makespan", "tardiness", "energy")
SEARCH_NEIGHBOURHOODS = ("uniform", "critical", "mixed")
SEARCH_ACCEPT = ("strict", "sideways", "tabu")
SEARCH_MAX_NEIGHBOURS = 64


def search_draws(seed, env, first, n):
    """Draws first .. first + n - 1 of the search stream of the env with global id `env` (fjsp_search_draws, host only):
    uint64[n].  Candidate q of round t of a search with n_cand neighbours owns draws 3 (t n_cand + q) + 0, 1, 2."""
    import ctypes as C
    from ._capi import check, lib
    n = int(n)
    if n < 0:
        raise ValueError("search_draws needs n >= 0")
    out = np.zeros(n, np.uint64)
    check(lib().fjsp_search_draws(int(seed) & (2 ** 64 - 1), int(env), int(first) & 0xFFFFFFFF, n, out.ctypes.data_as(C.POINTER(C.c_uint64))))
    return out


def search(batch, plan, rounds, n_cand, objective=0, neighbourhood=0, accept=1, tenure=0, seed=0, trace=False):
    """fjsp_schedule_search on the current stream: the whole hill climb or tabu search of every env in one launch (the
    contract is in include/fjsp_amd.h; policy_search.local_search is the checked form).  plan: int32[N, cap, 3]; the codes
    are the indices of SEARCH_OBJECTIVES, SEARCH_NEIGHBOURHOODS and SEARCH_ACCEPT.  Passes batch.first_env.  Returns dict(plan=
    int32[N, cap, 3], objective=int64[N, 2], history=int64[rounds + 1, N], accepted=int32[N], status=int32[N], trace=
    int32[rounds, N, 3] or None), device tensors.  ValueError for a plan of another shape; FjspError where the library refuses."""
    return _search(batch, plan, rounds, "fjsp_schedule_search", 2, (int(n_cand), int(objective), int(neighbourhood), int(accept), int(tenure)), seed, trace)


def search_dyn(batch, plan, rounds, n_cand, objective=0, accept=1, tenure=0, seed=0, trace=False):
    """search on a MO_DFJSP batch (fjsp_schedule_search_dyn): the uniform neighbourhood, every decode decode_dyn's, objective
    an index of SEARCH_DYN_OBJECTIVES.  The same draws, accept modes and dict, with objective=int64[N, 3] (makespan, total
    tardiness, energy).  FjspError on a batch that is not MO_DFJSP."""
    return _search(batch, plan, rounds, "fjsp_schedule_search_dyn", 3, (int(n_cand), int(objective), int(accept), int(tenure)), seed, trace)


def search_front(batch, plan, weights, rounds, n_cand, cap_front=64, accept=1, tenure=0, seed=0, trace=False, want_plans=True):
    """fjsp_schedule_search_front on the current stream: search steered by the key sum_c weights[e, c] * objective[c], and the
    Pareto archive of every vector the search decodes, in one launch (the contract is in include/fjsp_amd.h;
    policy_search.front_search is the checked form).  Either family: NO = 3 objectives on MO_DFJSP, 2 elsewhere.  plan:
    int32[N, cap, 3]; weights: int64[N, NO]; accept an index of SEARCH_ACCEPT.  Passes batch.first_env.  Returns search's
    dict (history holds the key) and front_obj=int64[N, cap_front, NO], front_src=int32[N, cap_front, 2], front_plan=
    int32[N, cap_front, cap, 3] or None (want_plans=False), front_count=int32[N], front_dropped=int32[N], device tensors.
    ValueError for a plan or weights of another shape; FjspError where the library refuses."""
    import torch
    from ._capi import check, ptr
    b = getattr(batch, "batch", batch)
    cap = int(b._lib.fjsp_schedule_decode_capacity(b._h))
    n_obj = 3 if b.variant == VARIANT_MO_DFJSP else 2
    if not torch.is_tensor(plan):
        plan = torch.as_tensor(np.asarray(plan))
    if tuple(plan.shape) != (b.N, cap, 3):
        raise ValueError("plan must have shape %s, got %s" % ((b.N, cap, 3), tuple(plan.shape)))
    if not torch.is_tensor(weights):
        weights = torch.as_tensor(np.asarray(weights, np.int64))
    if tuple(weights.shape) != (b.N, n_obj):
        raise ValueError("weights must have shape %s, got %s" % ((b.N, n_obj), tuple(weights.shape)))
    plan = plan.to(device=b.device, dtype=torch.int32).contiguous()
    weights = weights.to(device=b.device, dtype=torch.int64).contiguous()
    rows, F = max(int(rounds), 0), min(max(int(cap_front), 0), 64)
    new = lambda *shape, dtype=torch.int32: torch.empty(shape, dtype=dtype, device=b.device)
    out = dict(plan=torch.empty_like(plan), objective=new(b.N, n_obj, dtype=torch.int64), history=new(rows + 1, b.N, dtype=torch.int64),
               accepted=new(b.N), status=new(b.N), trace=new(rows, b.N, 3) if trace else None,
               front_obj=new(b.N, F, n_obj, dtype=torch.int64), front_src=new(b.N, F, 2),
               front_plan=new(b.N, F, cap, 3) if want_plans else None, front_count=new(b.N), front_dropped=new(b.N))
    check(b._lib.fjsp_schedule_search_front(b._h, ptr(plan), int(rounds), int(n_cand), ptr(weights), int(accept), int(tenure),
                                            int(seed) & (2 ** 64 - 1), int(b.first_env), int(cap_front), ptr(out["plan"]), ptr(out["objective"]),
                                            ptr(out["history"]), ptr(out["accepted"]), ptr(out["status"]), ptr(out["trace"]),
                                            ptr(out["front_obj"]), ptr(out["front_src"]), ptr(out["front_plan"]), ptr(out["front_count"]),
                                            ptr(out["front_dropped"]), b._stream()))
    return out


EVOLVE_MAX_POPULATION = 64
EVOLVE_MUT_ONE = 65536                          # mut_rate of a mutation in every child


def evolve(batch, pop_plans, generations, weights=None, mut_rate=6554, seed=0, trace=False):
    """fjsp_schedule_evolve on the current stream: `generations` generations of a genetic algorithm on a population of plans
    per env -- tournament selection by the key sum_c weights[e, c] * objective[c], precedence-preserving order crossover,
    a machine mutation in mut_rate / 65536 of the children, one elite -- in one launch (the contract is in
    include/fjsp_amd.h; policy_search.genetic_search is the checked form).  Either family: NO = 3 objectives on MO_DFJSP, 2
    elsewhere.  pop_plans: int32[N, P, cap, 3], P in 1..64; weights: None (the makespan alone) or int64[N, NO].  Passes
    batch.first_env.  Returns dict(population=int32[N, P, cap, 3] the last generation, population_objective=int64[N, P, NO],
    plan=int32[N, cap, 3] and objective=int64[N, NO] of the individual of least (key, index), history=int64[generations + 1,
    N] the least key of every generation, status=int32[N], trace=int32[generations, N, P, 3] (parent A, parent B, mutated row
    or -1) or None), device tensors.  ValueError for a population or weights of another shape; FjspError where the library
    refuses."""
    return _evolve(batch, pop_plans, generations, weights, mut_rate, seed, trace, "fjsp_schedule_evolve")


def evolve_active(batch, pop_plans, generations, weights=None, mut_rate=6554, seed=0, trace=False):
    """evolve with every individual scored by the active decoder (fjsp_schedule_evolve_active), the genetic algorithm as
    the FJSP literature scores it: the same arguments, checks, draws and results, but generation 0 and every child are
    decoded by decode_active's rule, so the keys of the tournaments, population_objective, objective and history are the
    active objectives.  The plans are not rewritten: population and plan hold the merged rows in merge order, which
    decode_active decodes to those objectives (policy_search.left_shift gives the begin-ordered plans).
    Returns evolve's dict and inserted=int32[N, P], the rows each individual of the last generation placed in front of an
    interval (zeros for an env with a status).  Shares decode_active's device workspace: issue the calls of both on one
    stream.  FjspError on MO_DFJSP (an insertion under breakdown shifts is not defined) and where evolve refuses."""
    return _evolve(batch, pop_plans, generations, weights, mut_rate, seed, trace, "fjsp_schedule_evolve_active")


def _evolve(batch, pop_plans, generations, weights, mut_rate, seed, trace, entry):
    import torch
    from ._capi import check, ptr
    b = getattr(batch, "batch", batch)
    cap = int(b._lib.fjsp_schedule_decode_capacity(b._h))
    n_obj = 3 if b.variant == VARIANT_MO_DFJSP else 2
    if not torch.is_tensor(pop_plans):
        pop_plans = torch.as_tensor(np.asarray(pop_plans))
    if pop_plans.dim() != 4 or tuple(pop_plans.shape) != (b.N, pop_plans.shape[1], cap, 3):
        raise ValueError("pop_plans must have shape %s, got %s" % ((b.N, "P", cap, 3), tuple(pop_plans.shape)))
    P = int(pop_plans.shape[1])
    if weights is None:
        weights = torch.tensor([1] + [0] * (n_obj - 1), dtype=torch.int64).expand(b.N, n_obj)
    elif not torch.is_tensor(weights):
        weights = torch.as_tensor(np.asarray(weights, np.int64))
    if tuple(weights.shape) != (b.N, n_obj):
        raise ValueError("weights must have shape %s, got %s" % ((b.N, n_obj), tuple(weights.shape)))
    pop_plans = pop_plans.to(device=b.device, dtype=torch.int32).contiguous()
    weights = weights.to(device=b.device, dtype=torch.int64).contiguous()
    rows = max(int(generations), 0)
    new = lambda *shape, dtype=torch.int32: torch.empty(shape, dtype=dtype, device=b.device)
    out = dict(population=torch.empty_like(pop_plans), population_objective=new(b.N, P, n_obj, dtype=torch.int64), plan=new(b.N, cap, 3),
               objective=new(b.N, n_obj, dtype=torch.int64), history=new(rows + 1, b.N, dtype=torch.int64), status=new(b.N),
               trace=new(rows, b.N, P, 3) if trace else None)
    work = torch.empty_like(pop_plans)
    more = ()
    if entry == "fjsp_schedule_evolve_active":
        out["inserted"] = new(b.N, P)
        more = (ptr(out["inserted"]),)
    check(getattr(b._lib, entry)(b._h, ptr(pop_plans), P, int(generations), ptr(weights), int(mut_rate), int(seed) & (2 ** 64 - 1),
                                 int(b.first_env), ptr(out["population"]), ptr(work), ptr(out["population_objective"]), ptr(out["plan"]),
                                 ptr(out["objective"]), ptr(out["history"]), ptr(out["status"]), ptr(out["trace"]), *more, b._stream()))
    return out


def _search(batch, plan, rounds, entry, n_obj, codes, seed, trace):
    import torch
    from ._capi import check, ptr
    b = getattr(batch, "batch", batch)
    cap = int(b._lib.fjsp_schedule_decode_capacity(b._h))
    if not torch.is_tensor(plan):
        plan = torch.as_tensor(np.asarray(plan))
    if tuple(plan.shape) != (b.N, cap, 3):
        raise ValueError("plan must have shape %s, got %s" % ((b.N, cap, 3), tuple(plan.shape)))
    plan = plan.to(device=b.device, dtype=torch.int32).contiguous()
    rows = max(int(rounds), 0)
    out = dict(plan=torch.empty_like(plan), objective=torch.empty(b.N, n_obj, dtype=torch.int64, device=b.device),
               history=torch.empty(rows + 1, b.N, dtype=torch.int64, device=b.device),
               accepted=torch.empty(b.N, dtype=torch.int32, device=b.device), status=torch.empty(b.N, dtype=torch.int32, device=b.device),
               trace=torch.empty(rows, b.N, 3, dtype=torch.int32, device=b.device) if trace else None)
    check(getattr(b._lib, entry)(b._h, ptr(plan), int(rounds), *codes, int(seed) & (2 ** 64 - 1), int(b.first_env), ptr(out["plan"]),
                                 ptr(out["objective"]), ptr(out["history"]), ptr(out["accepted"]), ptr(out["status"]), ptr(out["trace"]), b._stream()))
    return out
