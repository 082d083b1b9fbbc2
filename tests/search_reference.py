"""Plain numpy statement of fjsp_schedule_search (include/fjsp_amd.h): hill climbing and tabu search on explicit schedules,
round by round, with its own statement of the draw stream.  Written from the entry point's contract on top of the two
references the decoder and the critical paths are tested with (tests/decode_reference.py, tests/critical_reference.py),
independently of the kernel; the tests of the kernel compare with it bit for bit.

    draw(seed, i), env_stream(seed, g), pick(d, n)     the stream: splitmix64, all integers
    search_one(inst, variant, plan, ..., g)            one env: dict(plan, objective, history, accepted, status, trace) and,
                                                       for the tests, aspired = the rounds that took a tabu candidate
    search(insts, variant, plans, ..., first_env)      the entry point on a batch: insts[e] is env e's instance"""
import numpy as np

from tests import critical_reference as R
from tests import decode_reference as D

MASK = (1 << 64) - 1
STREAM = 0x8CB92BA72F3D8DD7                      # FJSP_SEARCH_STREAM
LIST_MAX = 128
MOVE_NONE, MOVE_MACHINE, MOVE_SWAP, MOVE_PAIR = 0, 1, 2, 4
UNIFORM, CRITICAL, MIXED = range(3)
STRICT, SIDEWAYS, TABU = range(3)
KEYS = ("plan", "objective", "history", "accepted", "status", "trace")


def draw(seed, i):
    """Draw i (0-based, a uint32 that wraps) of the splitmix64 stream `seed`."""
    z = (seed + (((i & 0xFFFFFFFF) + 1) & 0xFFFFFFFF) * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def env_stream(seed, g):
    """The stream of the env with global id g."""
    return draw((seed & MASK) ^ STREAM, g & 0xFFFFFFFF)


def draws(seed, g, first, n):
    s = env_stream(seed, g)
    return np.array([draw(s, first + i) for i in range(n)], np.uint64)


def pick(d, n):
    return ((d >> 32) * n) >> 32


def _padded(rows, cap):
    out = np.full((cap, 3), -1, np.int32)
    out[:len(rows)] = rows
    return out


def _order(rows, move):
    """Position -> old row of the plan the move stands for (a move inside the plan), and the rows it moves."""
    kind, u, third = move
    L = len(rows)
    order = list(range(L))
    if kind == MOVE_MACHINE:
        return order, [u]
    if kind == MOVE_SWAP:
        if not (rows[u, 0] == rows[u + 1, 0] and rows[u, 1] == rows[u + 1, 1]):
            order[u], order[u + 1] = u + 1, u
        return order, [u, u + 1]
    v, w = u + (third & 0xFFFF), u + (third >> 16)
    return list(range(u)) + list(range(u + 1, w + 1)) + [v, u] + list(range(w + 1, v)) + list(range(v + 1, L)), [u, v]


def search_one(inst, variant, plan, rounds, n_cand, objective=0, neighbourhood=UNIFORM, accept=SIDEWAYS, tenure=0, seed=0, g=0):
    plan = np.asarray(plan, np.int32).reshape(-1, 3)
    cap = len(plan)
    first = D.decode_one(inst, variant, plan, None, cap)
    out = dict(plan=plan.copy(), objective=np.array([-1, -1], np.int64), history=np.full(rounds + 1, -1, np.int64), accepted=0,
               status=first["status"], trace=np.zeros((rounds, 3), np.int32), aspired=[])
    if first["status"] != 0:
        return out
    col = objective
    Jr, p = np.asarray(inst.Jr, np.int64), np.asarray(inst.p, np.int64)
    koff = np.concatenate(([0], np.cumsum(Jr)))
    L = first["length"]
    rows = plan[:L].astype(np.int64)
    ids = np.arange(L)
    until = np.zeros(L, np.int64)
    cur = first["objective"].copy()
    best, best_plan = cur.copy(), plan.copy()
    out["history"][0] = cur[col]
    s = env_stream(seed, g)
    for t in range(rounds):
        listed = np.zeros((0, 3), np.int64)
        if neighbourhood != UNIFORM:
            one = D.decode_one(inst, variant, _padded(rows, cap), None, cap)
            assert one["status"] == 0 and np.array_equal(one["objective"], cur)
            order = np.argsort(one["table"][:L, 4], kind="stable")
            table = R.begin_order(one["table"])
            assert np.array_equal(table[:L], one["table"][:L][order])
            rows, ids = rows[order], ids[order]
            assert np.array_equal(rows, table[:L][:, [0, 2, 3]])
            crit = R.critical_one(inst, table, LIST_MAX, cap)
            assert crit["status"] == 0 and crit["skipped"] == 0
            listed = crit["moves"][:min(crit["n_moves"], LIST_MAX)].astype(np.int64)
        start = _padded(rows, cap)
        stage = np.array([np.sum((rows[:i, 0] == rows[i, 0]) & (rows[:i, 1] == rows[i, 1])) for i in range(L)], np.int64)
        winner = None                                                   # (objective, q, move, both objectives, tabu)
        for q in range(n_cand):
            c = [draw(s, 3 * (t * n_cand + q) + i) for i in range(3)]
            if neighbourhood == CRITICAL or (neighbourhood == MIXED and q < n_cand // 2):
                if len(listed) == 0:
                    continue
                move = tuple(int(x) for x in listed[pick(c[2], len(listed))])
            elif q % 2 == 0:
                u = pick(c[0], L)
                elig = np.flatnonzero(p[koff[rows[u, 0]] + stage[u]] > 0)
                move = (MOVE_MACHINE, u, int(elig[pick(c[1], len(elig))]))
            else:
                move = (MOVE_SWAP, pick(c[0], max(L - 1, 1)), 0)
            res = R.decode_moved(inst, variant, start, move, cap)
            if res["status"] != 0:
                continue
            value, tabu = int(res["objective"][col]), False
            if accept == TABU:
                order, moved = _order(rows, move)
                if (move[0] == MOVE_MACHINE and move[2] == rows[move[1], 2]) or (move[0] != MOVE_MACHINE and order == list(range(L))):
                    continue                                            # changes nothing
                tabu = any(until[ids[x]] > t for x in moved)
                if tabu and not value < best[col]:
                    continue
            if winner is None or value < winner[0]:
                winner = (value, q, move, res["objective"].copy(), tabu)
        take = winner is not None and (accept == TABU or winner[0] < cur[col] or (winner[0] == cur[col] and accept == SIDEWAYS))
        if take:
            value, q, move, both, tabu = winner
            order, moved = _order(rows, move)
            if accept == TABU:
                until[ids[moved]] = min(t + 1 + tenure, 2 ** 31 - 1)
                if tabu:
                    out["aspired"].append(t)
            rows, ids = rows[order], ids[order]
            if move[0] == MOVE_MACHINE:
                rows[move[1], 2] = move[2]
            assert np.array_equal(_padded(rows, cap), R.materialise_moved(start, move, cap))
            cur = both
            out["accepted"] += 1
            out["trace"][t] = move
            if accept == TABU and cur[col] < best[col]:
                best, best_plan = cur.copy(), _padded(rows, cap)
        out["history"][t + 1] = cur[col]
    if accept != TABU:
        best = cur
        if rounds > 0:
            best_plan = _padded(rows, cap)
    out.update(plan=best_plan, objective=np.asarray(best, np.int64))
    return out


def search(insts, variant, plans, rounds, n_cand, objective=0, neighbourhood=UNIFORM, accept=SIDEWAYS, tenure=0, seed=0, first_env=0):
    """insts[e]: env e's instance; plans int[N][cap][3].  dict(plan int32[N][cap][3], objective int64[N][2], history
    int64[rounds + 1][N], accepted int32[N], status int32[N], trace int32[rounds][N][3], aspired: list per env)."""
    ones = [search_one(insts[e], variant, plans[e], rounds, n_cand, objective, neighbourhood, accept, tenure, seed, first_env + e)
            for e in range(len(insts))]
    return dict(plan=np.stack([o["plan"] for o in ones]).astype(np.int32), objective=np.stack([o["objective"] for o in ones]).astype(np.int64),
                history=np.stack([o["history"] for o in ones], 1).astype(np.int64), accepted=np.array([o["accepted"] for o in ones], np.int32),
                status=np.array([o["status"] for o in ones], np.int32),
                trace=np.stack([o["trace"] for o in ones], 1).astype(np.int32).reshape(rounds, len(insts), 3), aspired=[o["aspired"] for o in ones])
