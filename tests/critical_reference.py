"""Plain numpy statement of fjsp_schedule_critical (include/fjsp_amd.h) and of the decoder's MOVE_PAIR, written from the
contract and independently of the kernel; the tests of the kernel compare with it bit for bit.

A table is int[cap][6] rows (r, stage, n, m, begin, end) and ends at its first row of six -1.  The arcs are those of the
table's own order: the job (machine) predecessor of a row is the latest row in front of it with the same (r, n) (the same
m).  Predecessors are built forwards, tails backwards, the path follows the rule of the contract, the moves come in its
order.  MOVE_PAIR is stated as "materialise, then decode_reference.decode_one without a move"."""
import numpy as np

from tests import decode_reference as D

OK, BAD_ROW, EMPTY = range(3)
CRITICAL, PATH, MACHINE_ARC = 1, 2, 4
MOVE_MACHINE, MOVE_PAIR = 1, 4
KEYS = ("tail", "flags", "path", "path_len", "moves", "n_moves", "skipped", "status", "makespan")


def table_length(table):
    table = np.asarray(table, np.int64).reshape(-1, 6)
    end = np.flatnonzero((table == -1).all(1))
    return int(end[0]) if len(end) else len(table)


def predecessors(rows):
    """(jp, mp): per row the latest earlier row of its job / on its machine, -1 without one."""
    jp, mp = np.full(len(rows), -1), np.full(len(rows), -1)
    last_j, last_m = {}, {}
    for t, (r, _, n, m, _, _) in enumerate(rows.tolist()):
        jp[t], mp[t] = last_j.get((r, n), -1), last_m.get(m, -1)
        last_j[(r, n)] = last_m[m] = t
    return jp, mp


def critical_one(inst, table, max_moves=0, cap=None):
    """dict(KEYS) of one table: arrays of cap (tail int32, flags uint8, path int32), moves int32[max_moves][3], scalars."""
    table = np.asarray(table, np.int64).reshape(-1, 6)
    cap = len(table) if cap is None else cap
    out = dict(tail=np.full(cap, -1, np.int32), flags=np.zeros(cap, np.uint8), path=np.full(cap, -1, np.int32), path_len=0,
               moves=np.zeros((max_moves, 3), np.int32), n_moves=0, skipped=0, status=OK, makespan=-1)
    L = table_length(table)
    rows = table[:L]
    Jr, p = np.asarray(inst.Jr, np.int64), np.asarray(inst.p, np.int64)
    koff = np.concatenate(([0], np.cumsum(Jr)))
    jobs = np.asarray(inst.count, np.int64).reshape(len(np.asarray(inst.arrive)), len(Jr)).sum(0)
    M = p.shape[1]
    if L == 0:
        out["status"] = EMPTY
        return out
    for r, j, n, m, b, e in rows.tolist():
        if not (0 <= r < len(Jr) and 0 <= n < jobs[r] and 0 <= m < M and 0 <= j < Jr[r] and 0 <= b < e):
            out["status"] = BAD_ROW
            return out
    begin, end = rows[:, 4], rows[:, 5]
    C = int(end.max())
    e0 = int(np.flatnonzero(end == C)[0])
    jp, mp = predecessors(rows)
    # tails, backwards: a row hands tail + duration to both of its predecessors
    tail = np.zeros(L, np.int64)
    for t in range(L - 1, -1, -1):
        for q in (jp[t], mp[t]):
            if q >= 0:
                tail[q] = max(tail[q], tail[t] + end[t] - begin[t])
    flags = np.where(end + tail == C, CRITICAL, 0)
    # the path
    path, cur = [e0], e0
    while True:
        tight = [(q, kind) for q, kind in ((jp[cur], 0), (mp[cur], MACHINE_ARC)) if q >= 0 and end[q] == begin[cur]]
        if not tight:
            break
        q = max(x[0] for x in tight)
        arc = 0 if q == jp[cur] else MACHINE_ARC
        flags[q] |= arc
        path.append(int(q))
        cur = q
    flags[path] |= PATH
    # the moves
    moves, skipped = [], 0
    job = lambda t: (rows[t, 0], rows[t, 2])
    for v, u in zip(path, path[1:]):
        if not flags[u] & MACHINE_ARC:
            continue
        of_b = [t for t in range(u + 1, v) if job(t) == job(v)]
        of_a = [t for t in range(u + 1, v) if job(t) == job(u)]
        w = of_b[-1] if of_b else u
        if (not of_a or w < of_a[0]) and w - u <= 32767:            # (dv | dw << 16 stays a non-negative int32)
            moves.append((MOVE_PAIR, u, (v - u) | ((w - u) << 16)))
        else:
            skipped += 1
    for t in path:
        r, j, _, m = rows[t, :4]
        moves += [(MOVE_MACHINE, t, m2) for m2 in range(M) if m2 != m and p[koff[r] + j, m2] > 0]
    out["tail"][:L] = tail
    out["flags"][:L] = flags
    out["path"][:len(path)] = path
    k = min(len(moves), max_moves)
    if k:
        out["moves"][:k] = moves[:k]
    out.update(path_len=len(path), n_moves=len(moves), skipped=skipped, makespan=C)
    return out


def critical(insts, tables, n_cand=1, max_moves=0):
    """The entry point on a batch: insts[i] is env i's instance, tables int[N][n_cand][cap][6]; arrays [N][n_cand][...]."""
    tables = np.asarray(tables)
    N, cap = len(insts), tables.shape[-2]
    tables = tables.reshape(N, n_cand, cap, 6)
    ones = [[critical_one(insts[i], tables[i, q], max_moves, cap) for q in range(n_cand)] for i in range(N)]
    return {key: np.array([[one[key] for one in per] for per in ones], np.uint8 if key == "flags" else np.int32).reshape(
        (N, n_cand) + np.shape(ones[0][0][key])) for key in KEYS}


# ---- MOVE_PAIR of the decoder
def pair_ok(plan, move):
    """Whether decode takes (4, u, dv | dw << 16) on this plan: else status 4."""
    _, u, third = (int(x) for x in move)
    dv, dw = third & 0xFFFF, third >> 16
    return third >= 0 and 1 <= dv and 0 <= dw < dv and u >= 0 and u + dv < D.plan_length(plan)


def materialise_pair(plan, move, cap=None):
    """The plan a MOVE_PAIR stands for: old rows 0 .. u-1, u+1 .. w, v, u, w+1 .. v-1, v+1 ..; a refused move leaves the
    plan as it is.  int32[cap][3], -1 rows past the end."""
    plan = np.asarray(plan, np.int64).reshape(-1, 3)
    L = D.plan_length(plan)
    order = list(range(L))
    if pair_ok(plan, move):
        u, third = int(move[1]), int(move[2])
        v, w = u + (third & 0xFFFF), u + (third >> 16)
        order = list(range(u)) + list(range(u + 1, w + 1)) + [v, u] + list(range(w + 1, v)) + list(range(v + 1, L))
    out = np.full((len(plan) if cap is None else cap, 3), -1, np.int32)
    out[:L] = plan[order]
    return out


def decode_pair(inst, variant, plan, move, cap=None):
    """decode_reference.decode_one's dict for a MOVE_PAIR candidate: the materialised plan decoded without a move."""
    plan = np.asarray(plan, np.int64).reshape(-1, 3)
    cap = len(plan) if cap is None else cap
    if not pair_ok(plan, move):
        return dict(status=D.BAD_MOVE, objective=np.array([-1, -1], np.int64), table=np.full((cap, 6), -1, np.int32), length=0)
    return D.decode_one(inst, variant, materialise_pair(plan, move), None, cap)


def decode_moved(inst, variant, plan, move, cap=None):
    """Any move: kind 4 as decode_pair, the others as decode_reference.decode_one states them (4 where it knows none)."""
    return decode_pair(inst, variant, plan, move, cap) if int(move[0]) == MOVE_PAIR else D.decode_one(inst, variant, plan, move, cap)


def materialise_moved(plan, move, cap=None):
    return materialise_pair(plan, move, cap) if int(move[0]) == MOVE_PAIR else D.materialise(plan, move, cap)


def machine_sequences(table):
    """{m: [(r, stage, n) in begin order]} of a decoded table."""
    rows = np.asarray(table, np.int64).reshape(-1, 6)
    rows = rows[:table_length(rows)]
    rows = rows[np.lexsort((np.arange(len(rows)), rows[:, 4]))]
    seq = {}
    for r, j, n, m, _, _ in rows.tolist():
        seq.setdefault(m, []).append((r, j, n))
    return seq


def begin_order(table):
    """The table with its rows stably sorted by begin, -1 rows at the end."""
    table = np.asarray(table).reshape(-1, 6)
    L = table_length(table)
    out = table.copy()
    out[:L] = table[:L][np.argsort(table[:L, 4], kind="stable")]
    return out
