"""Plain numpy statement of fjsp_schedule_search_dyn (include/fjsp_amd.h): hill climbing and tabu search on explicit
schedules of MO_DFJSP, round by round.  Written from the entry point's contract on top of the references it names: the
draw stream, the index map of a move and the shape of the result are tests/search_reference.py's (draw, env_stream, pick,
_order, _padded), every decode is tests/decode_dyn_reference.py's decode_one.  Independent of the kernel; the tests of the
kernel compare with it bit for bit.  Only the uniform neighbourhood exists: the plan is never reordered.

    search_one(inst, plan, ..., g)                one env: dict(plan, objective int64[3], history, accepted, status, trace)
                                                  and, for the tests, aspired = the rounds that took a tabu candidate
    search(insts, plans, ..., first_env)          the entry point on a batch: insts[e] is env e's instance"""
import numpy as np

from tests import decode_dyn_reference as DD
from tests import search_reference as S

MAKESPAN, TARDINESS, ENERGY = range(3)
STRICT, SIDEWAYS, TABU = S.STRICT, S.SIDEWAYS, S.TABU
KEYS = S.KEYS


def search_one(inst, plan, rounds, n_cand, objective=MAKESPAN, accept=SIDEWAYS, tenure=0, seed=0, g=0):
    plan = np.asarray(plan, np.int32).reshape(-1, 3)
    cap = len(plan)
    first = DD.decode_one(inst, plan, None, cap)
    out = dict(plan=plan.copy(), objective=np.array([-1, -1, -1], np.int64), history=np.full(rounds + 1, -1, np.int64), accepted=0,
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
    s = S.env_stream(seed, g)
    for t in range(rounds):
        start = S._padded(rows, cap)
        stage = np.array([np.sum((rows[:i, 0] == rows[i, 0]) & (rows[:i, 1] == rows[i, 1])) for i in range(L)], np.int64)
        winner = None                                                   # (objective, q, move, the three objectives, tabu)
        for q in range(n_cand):
            c = [S.draw(s, 3 * (t * n_cand + q) + i) for i in range(3)]
            if q % 2 == 0:
                u = S.pick(c[0], L)
                elig = np.flatnonzero(p[koff[rows[u, 0]] + stage[u]] > 0)
                move = (S.MOVE_MACHINE, u, int(elig[S.pick(c[1], len(elig))]))
            else:
                move = (S.MOVE_SWAP, S.pick(c[0], max(L - 1, 1)), 0)
            res = DD.decode_one(inst, start, move, cap)
            if res["status"] != 0:
                continue
            value, tabu = int(res["objective"][col]), False
            if accept == TABU:
                order, moved = S._order(rows, move)
                if (move[0] == S.MOVE_MACHINE and move[2] == rows[move[1], 2]) or (move[0] != S.MOVE_MACHINE and order == list(range(L))):
                    continue                                            # changes nothing
                tabu = any(until[ids[x]] > t for x in moved)
                if tabu and not value < best[col]:
                    continue
            if winner is None or value < winner[0]:
                winner = (value, q, move, res["objective"].copy(), tabu)
        take = winner is not None and (accept == TABU or winner[0] < cur[col] or (winner[0] == cur[col] and accept == SIDEWAYS))
        if take:
            value, q, move, three, tabu = winner
            order, moved = S._order(rows, move)
            if accept == TABU:
                until[ids[moved]] = min(t + 1 + tenure, 2 ** 31 - 1)
                if tabu:
                    out["aspired"].append(t)
            rows, ids = rows[order], ids[order]
            if move[0] == S.MOVE_MACHINE:
                rows[move[1], 2] = move[2]
            cur = three
            out["accepted"] += 1
            out["trace"][t] = move
            if accept == TABU and cur[col] < best[col]:
                best, best_plan = cur.copy(), S._padded(rows, cap)
        out["history"][t + 1] = cur[col]
    if accept != TABU:
        best = cur
        if rounds > 0:
            best_plan = S._padded(rows, cap)
    out.update(plan=best_plan, objective=np.asarray(best, np.int64))
    return out


def search(insts, plans, rounds, n_cand, objective=MAKESPAN, accept=SIDEWAYS, tenure=0, seed=0, first_env=0):
    """insts[e]: env e's instance; plans int[N][cap][3].  dict(plan int32[N][cap][3], objective int64[N][3], history
    int64[rounds + 1][N], accepted int32[N], status int32[N], trace int32[rounds][N][3], aspired: list per env)."""
    ones = [search_one(insts[e], plans[e], rounds, n_cand, objective, accept, tenure, seed, first_env + e) for e in range(len(insts))]
    return dict(plan=np.stack([o["plan"] for o in ones]).astype(np.int32), objective=np.stack([o["objective"] for o in ones]).astype(np.int64),
                history=np.stack([o["history"] for o in ones], 1).astype(np.int64), accepted=np.array([o["accepted"] for o in ones], np.int32),
                status=np.array([o["status"] for o in ones], np.int32),
                trace=np.stack([o["trace"] for o in ones], 1).astype(np.int32).reshape(rounds, len(insts), 3), aspired=[o["aspired"] for o in ones])
