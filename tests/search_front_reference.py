"""Plain numpy / Python-int statement of fjsp_schedule_search_front (include/fjsp_amd.h): the hill climb or tabu search of
explicit schedules steered by a weighted sum of the objectives, and the Pareto archive of everything it decodes.  Written
from the entry point's contract on top of the references it names: the draw stream, the index map of a move and the shape
of the result are tests/search_reference.py's (draw, env_stream, pick, _order, _padded); every decode is
tests/decode_dyn_reference.py's on MO_DFJSP (three objectives) and tests/decode_reference.py's elsewhere (two).
Independent of the kernel; the tests of the kernel compare with it bit for bit.  Keys are Python integers: no wrap.

    key_of(w, vec)                                 the saturating weighted sum
    round_candidates(inst, variant, rows, ...)     the candidates of one round: (q, move, result of the decode)
    search_one(inst, variant, plan, w, ..., g)     one env: dict of KEYS and, for the tests, aspired, peak (the archive's
                                                   largest size), entrants (how many vectors were entrants) and
                                                   left_for_dropped (members that only a dropped entrant dominated)
    search(insts, variant, plans, weights, ...)    the entry point on a batch: insts[e] is env e's instance"""
import numpy as np

from tests import decode_dyn_reference as DD
from tests import decode_reference as D
from tests import search_reference as S

STRICT, SIDEWAYS, TABU = S.STRICT, S.SIDEWAYS, S.TABU
KEY_MAX = 2 ** 63 - 2                            # a key saturates one below the "no candidate" sentinel
BAD_WEIGHTS = 5
KEYS = S.KEYS + ("front_obj", "front_src", "front_plan", "front_count", "front_dropped")


def n_objectives(variant):
    return 3 if variant == DD.VARIANT else 2


def decode_one(inst, variant, plan, move, cap):
    return DD.decode_one(inst, plan, move, cap) if variant == DD.VARIANT else D.decode_one(inst, variant, plan, move, cap)


def key_of(w, vec):
    """sum_c w[c] * vec[c], every product and every partial sum saturating at 2^63 - 2."""
    total = 0
    for wc, x in zip(w, vec):
        total = min(total + min(int(wc) * int(x), KEY_MAX), KEY_MAX)
    return total


def leq(a, b):
    return all(x <= y for x, y in zip(a, b))


def dominates(a, b):
    return leq(a, b) and tuple(a) != tuple(b)


def round_candidates(inst, variant, rows, t, n_cand, stream, cap):
    """[(q, move, decode result)] of round t on the plan `rows` (int[L][3]): q even (1, u, m), q odd (2, u, 0), as the
    uniform neighbourhood of fjsp_schedule_search draws them."""
    Jr, p = np.asarray(inst.Jr, np.int64), np.asarray(inst.p, np.int64)
    koff = np.concatenate(([0], np.cumsum(Jr)))
    L = len(rows)
    start = S._padded(rows, cap)
    stage = np.array([np.sum((rows[:i, 0] == rows[i, 0]) & (rows[:i, 1] == rows[i, 1])) for i in range(L)], np.int64)
    out = []
    for q in range(n_cand):
        c = [S.draw(stream, 3 * (t * n_cand + q) + i) for i in range(3)]
        if q % 2 == 0:
            u = S.pick(c[0], L)
            elig = np.flatnonzero(p[koff[rows[u, 0]] + stage[u]] > 0)
            move = (S.MOVE_MACHINE, u, int(elig[S.pick(c[1], len(elig))]))
        else:
            move = (S.MOVE_SWAP, S.pick(c[0], max(L - 1, 1)), 0)
        out.append((q, move, decode_one(inst, variant, start, move, cap)))
    return out


def archive_round(slots, cands, t):
    """One round of the archive rule on `slots` (list of None or (vector, (round, q), plan)), in place; cands: [(q, vector,
    plan)] of the round's status-0 candidates.  Returns (entrants, dropped, members that left for a dropped entrant alone)."""
    members = [m for m in slots if m is not None]
    entrants = []
    for q, v, pl in cands:
        if any(leq(m[0], v) for m in members):
            continue
        if any(dominates(v2, v) for q2, v2, _ in cands if q2 != q):
            continue
        if any(v2 == v for q2, v2, _ in cands if q2 < q):
            continue
        entrants.append((q, v, pl))
    left = [m for m in members if any(dominates(v, m[0]) for _, v, _ in entrants)]
    for s, m in enumerate(slots):
        if m is not None and any(m is x for x in left):
            slots[s] = None
    free = [s for s, m in enumerate(slots) if m is None]
    for (q, v, pl), s in zip(entrants, free):
        slots[s] = (v, (t, q), pl)
    by_dropped = sum(not any(dominates(v, m[0]) for _, v, _ in entrants[:len(free)]) for m in left)
    return len(entrants), max(len(entrants) - len(free), 0), by_dropped


def search_one(inst, variant, plan, w, rounds, n_cand, cap_front, accept=SIDEWAYS, tenure=0, seed=0, g=0):
    plan = np.asarray(plan, np.int32).reshape(-1, 3)
    cap, NO = len(plan), n_objectives(variant)
    w = [int(x) for x in w]
    assert len(w) == NO
    out = dict(plan=plan.copy(), objective=np.full(NO, -1, np.int64), history=np.full(rounds + 1, -1, np.int64), accepted=0,
               status=0, trace=np.zeros((rounds, 3), np.int32), aspired=[], peak=0, entrants=0, left_for_dropped=0,
               front_obj=np.full((cap_front, NO), -1, np.int64), front_src=np.full((cap_front, 2), -1, np.int32),
               front_plan=np.full((cap_front, cap, 3), -1, np.int32), front_count=0, front_dropped=0)
    if any(x < 0 for x in w) or all(x == 0 for x in w):
        out["status"] = BAD_WEIGHTS                                     # (outranks the plan's status)
        return out
    first = decode_one(inst, variant, plan, None, cap)
    out["status"] = first["status"]
    if first["status"] != 0:
        return out
    vec = lambda res: tuple(int(x) for x in res["objective"])
    L = first["length"]
    rows = plan[:L].astype(np.int64)
    ids = np.arange(L)
    until = np.zeros(L, np.int64)
    cur = vec(first)
    best, best_plan = cur, plan.copy()
    out["history"][0] = key_of(w, cur)
    slots = [None] * cap_front
    slots[0] = (cur, (-1, 0), S._padded(rows, cap))
    peak = 1
    s = S.env_stream(seed, g)
    for t in range(rounds):
        start = S._padded(rows, cap)
        cands = round_candidates(inst, variant, rows, t, n_cand, s, cap)
        ok = [(q, move, res) for q, move, res in cands if res["status"] == 0]
        n_ent, n_drop, n_by = archive_round(slots, [(q, vec(res), D.materialise(start, move, cap)) for q, move, res in ok], t)
        out["entrants"] += n_ent
        out["front_dropped"] += n_drop
        out["left_for_dropped"] += n_by
        peak = max(peak, sum(m is not None for m in slots))
        winner = None                                                   # (key, q, move, vector, tabu)
        for q, move, res in ok:
            value, tabu = key_of(w, vec(res)), False
            if accept == TABU:
                order, moved = S._order(rows, move)
                if (move[0] == S.MOVE_MACHINE and move[2] == rows[move[1], 2]) or (move[0] != S.MOVE_MACHINE and order == list(range(L))):
                    continue                                            # changes nothing
                tabu = any(until[ids[x]] > t for x in moved)
                if tabu and not value < key_of(w, best):
                    continue
            if winner is None or value < winner[0]:
                winner = (value, q, move, vec(res), tabu)
        now = key_of(w, cur)
        take = winner is not None and (accept == TABU or winner[0] < now or (winner[0] == now and accept == SIDEWAYS))
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
            if accept == TABU and key_of(w, cur) < key_of(w, best):
                best, best_plan = cur, S._padded(rows, cap)
        out["history"][t + 1] = key_of(w, cur)
    if accept != TABU:
        best = cur
        if rounds > 0:
            best_plan = S._padded(rows, cap)
    out.update(plan=best_plan, objective=np.asarray(best, np.int64), peak=peak, front_count=sum(m is not None for m in slots))
    for i, m in enumerate(slots):
        if m is not None:
            out["front_obj"][i], out["front_src"][i], out["front_plan"][i] = m
    return out


def search(insts, variant, plans, weights, rounds, n_cand, cap_front, accept=SIDEWAYS, tenure=0, seed=0, first_env=0):
    """insts[e]: env e's instance; plans int[N][cap][3]; weights int[N][NO].  dict(plan int32[N][cap][3], objective
    int64[N][NO], history int64[rounds + 1][N], accepted, status int32[N], trace int32[rounds][N][3], front_obj
    int64[N][cap_front][NO], front_src int32[N][cap_front][2], front_plan int32[N][cap_front][cap][3], front_count,
    front_dropped int32[N]; aspired, peak, entrants, left_for_dropped: lists per env)."""
    N = len(insts)
    ones = [search_one(insts[e], variant, plans[e], weights[e], rounds, n_cand, cap_front, accept, tenure, seed, first_env + e) for e in range(N)]
    stack = lambda key, dtype, axis=0: np.stack([np.asarray(o[key]) for o in ones], axis).astype(dtype)
    return dict(plan=stack("plan", np.int32), objective=stack("objective", np.int64), history=stack("history", np.int64, 1),
                accepted=stack("accepted", np.int32), status=stack("status", np.int32),
                trace=stack("trace", np.int32, 1).reshape(rounds, N, 3), front_obj=stack("front_obj", np.int64),
                front_src=stack("front_src", np.int32), front_plan=stack("front_plan", np.int32),
                front_count=stack("front_count", np.int32), front_dropped=stack("front_dropped", np.int32),
                aspired=[o["aspired"] for o in ones], peak=[o["peak"] for o in ones], entrants=[o["entrants"] for o in ones],
                left_for_dropped=[o["left_for_dropped"] for o in ones])
