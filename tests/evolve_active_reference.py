"""Plain numpy / Python-int statement of fjsp_schedule_evolve_active (include/fjsp_amd.h): fjsp_schedule_evolve's genetic
algorithm with the decoder as an argument.  The loop is stated once more here, on tests/evolve_reference.py's own stream
(draw, env_stream, child_stream), crossover and least, so that one text runs under either decoder:

    decode=search_front_reference.decode_one     the semi-active decode: the loop must then equal evolve_reference.evolve_one
                                                 in every key (tests/test_evolve_active_reference_host.py pins it there)
    decode=decode_active_reference.decode_one    the active decode (the default): the entry point's contract

A decoder is decode(inst, variant, plan, move, cap) -> dict(status, objective, length[, inserted]).  Independent of the
kernel; the tests of the kernel compare with it bit for bit.

    evolve_one(inst, variant, pop, w, ..., g, decode)   one env: dict of KEYS: evolve_reference.KEYS, inserted int32[P] (of
                                                 the last generation's individuals, zeros with a status), children and ties
                                                 as evolve_reference keeps them
    evolve(insts, variant, pops, weights, ...)   the entry point on a batch: insts[e] is env e's instance"""
import numpy as np

from tests import decode_active_reference as DA
from tests import evolve_reference as E
from tests import search_front_reference as SF
from tests import search_reference as S

KEYS = E.KEYS + ("inserted",)


def evolve_one(inst, variant, pop, w, generations, mut_rate, seed=0, g=0, decode=DA.decode_one):
    pop = np.asarray(pop, np.int32)
    P, cap = pop.shape[0], pop.shape[1]
    NO = SF.n_objectives(variant)
    w = [int(x) for x in w]
    assert len(w) == NO and 1 <= P <= 64 and 0 <= mut_rate <= E.MUT_ONE
    out = dict(population=pop.copy(), population_objective=np.full((P, NO), -1, np.int64), plan=pop[0].copy(),
               objective=np.full(NO, -1, np.int64), history=np.full(generations + 1, -1, np.int64), status=0,
               trace=np.zeros((generations, P, 3), np.int32), inserted=np.zeros(P, np.int32), children=[], ties=[])
    if any(x < 0 for x in w) or all(x == 0 for x in w):
        out["status"] = SF.BAD_WEIGHTS
        return out
    made = [decode(inst, variant, pop[q], None, cap) for q in range(P)]
    bad = [r["status"] for r in made if r["status"] != 0]
    if bad:
        out["status"] = bad[0]                                          # (of the lowest such q)
        return out
    Jr, p = np.asarray(inst.Jr, np.int64), np.asarray(inst.p, np.int64)
    koff = np.concatenate(([0], np.cumsum(Jr)))
    jbeg = E.job_numbers(inst)
    L = made[0]["length"]
    assert all(r["length"] == L for r in made)
    rows = [pop[q][:L].astype(np.int64) for q in range(P)]
    vec_of = lambda r: tuple(int(x) for x in r["objective"])
    keys = [SF.key_of(w, vec_of(r)) for r in made]
    out["history"][0] = min(keys)
    s = E.env_stream(seed, g)
    for t in range(1, generations + 1):
        best = E._least(keys)
        new_rows, new_keys, new_made, kept = [], [], [], []
        for q in range(P):
            c = E.child_stream(s, t, P, q)
            if q == 0:
                a = b = best
                child = rows[best].copy()
                u = -1
            else:
                picks = [S.pick(E.draw(c, i), P) for i in range(4)]
                parents = []
                for n, (x, y) in enumerate((picks[:2], picks[2:])):
                    if x != y and keys[x] == keys[y]:
                        out["ties"].append((t, q, n))
                    parents.append(min((x, y), key=lambda i: (keys[i], i)))
                a, b = parents
                child = E.crossover(rows[a], rows[b], jbeg, c)
                u = S.pick(E.draw(c, 5), L) if S.pick(E.draw(c, 4), E.MUT_ONE) < mut_rate else -1
            plain = child.copy()
            if u >= 0:                                                  # the mutated row is fixed before it is placed
                stage = int(np.sum((child[:u, 0] == child[u, 0]) & (child[:u, 1] == child[u, 1])))
                elig = np.flatnonzero(p[koff[child[u, 0]] + stage] > 0)
                child[u, 2] = int(elig[S.pick(E.draw(c, 6), len(elig))])
            res = decode(inst, variant, S._padded(child, cap), None, cap)
            kept.append((plain, child.copy(), res["status"]))
            new_made.append(res)
            new_rows.append(child if res["status"] == 0 else child[:0])
            new_keys.append(SF.key_of(w, vec_of(res)) if res["status"] == 0 else E.NONE_KEY)
            out["trace"][t - 1, q] = (a, b, u)
        rows, keys, made = new_rows, new_keys, new_made
        out["children"].append(kept)
        out["history"][t] = min(keys)
    best = E._least(keys)
    vecs = [vec_of(r) for r in made]
    out.update(population=np.stack([S._padded(r, cap) for r in rows]), population_objective=np.array(vecs, np.int64).reshape(P, NO),
               plan=S._padded(rows[best], cap), objective=np.asarray(vecs[best], np.int64),
               inserted=np.array([r.get("inserted", 0) if r["status"] == 0 else 0 for r in made], np.int32))
    return out


def evolve(insts, variant, pops, weights, generations, mut_rate, seed=0, first_env=0, decode=DA.decode_one):
    """evolve_reference.evolve's dict and inserted int32[N][P]."""
    N = len(insts)
    ones = [evolve_one(insts[e], variant, pops[e], weights[e], generations, mut_rate, seed, first_env + e, decode) for e in range(N)]
    stack = lambda key, dtype, axis=0: np.stack([np.asarray(o[key]) for o in ones], axis).astype(dtype)
    return dict(population=stack("population", np.int32), population_objective=stack("population_objective", np.int64),
                plan=stack("plan", np.int32), objective=stack("objective", np.int64), history=stack("history", np.int64, 1),
                status=stack("status", np.int32), trace=stack("trace", np.int32, 1), inserted=stack("inserted", np.int32),
                children=[o["children"] for o in ones], ties=[o["ties"] for o in ones])
