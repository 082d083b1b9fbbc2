"""Plain numpy / Python-int statement of fjsp_schedule_evolve (include/fjsp_amd.h): a genetic algorithm on populations of
explicit schedules -- binary tournaments, precedence-preserving order crossover over a random job set, a machine mutation,
one elite -- generation by generation.  Written from the entry point's contract on top of the references it names: pick is
tests/search_reference.py's, every decode is tests/decode_dyn_reference.py's on MO_DFJSP (three objectives) and
tests/decode_reference.py's elsewhere (two), the key is tests/search_front_reference.py's.  The draw arithmetic is written
out once more here, on purpose: the stream is this entry's own.  Independent of the kernel; the tests of the kernel compare
with it bit for bit.

    draw(seed, i), env_stream(seed, g), child_stream(s, t, pop, q)   the stream: splitmix64, all integers
    job_numbers(inst)                              first job number of every kind
    in_set(c, j)                                   is job j in the job set of the child whose stream is c?
    crossover(A, B, jbeg, c)                       the child's rows before the mutation
    evolve_one(inst, variant, pop, w, ..., g)      one env: dict of KEYS and, for the tests, children: per generation and
                                                   child (rows before the mutation, rows, status of the decode), and ties:
                                                   the (generation, child, tournament) whose two picks differ with equal keys
    evolve(insts, variant, pops, weights, ...)     the entry point on a batch: insts[e] is env e's instance"""
import numpy as np

from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
from tests import search_front_reference as SF
from tests import search_reference as S

MASK = (1 << 64) - 1
STREAM = 0xC2B2AE3D27D4EB4F                      # FJSP_EVOLVE_STREAM
NONE_KEY = 2 ** 63 - 1                           # the key of a child that failed
MUT_ONE = 65536
KEYS = ("population", "population_objective", "plan", "objective", "history", "status", "trace")


def draw(seed, i):
    """Draw i (0-based, a uint32 that wraps) of the splitmix64 stream `seed`."""
    z = (seed + (((i & 0xFFFFFFFF) + 1) & 0xFFFFFFFF) * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def env_stream(seed, g):
    return draw((seed & MASK) ^ STREAM, g & 0xFFFFFFFF)


def child_stream(s, t, pop, q):
    """The stream of child q of generation t (1-based)."""
    return draw(s, ((t - 1) * pop + q) & 0xFFFFFFFF)


def job_numbers(inst):
    """First job number of every kind: the jobs are numbered over the kinds in order."""
    return np.concatenate(([0], np.cumsum([len(o) for o in sch.order_of_jobs(inst)]))).astype(np.int64)


def in_set(c, j):
    return (draw(c, 8 + (j >> 6)) >> (j & 63)) & 1 == 1


def crossover(A, B, jbeg, c):
    """Position t' of the child is A[t'] if its job is in the set, else the next row of B whose job is not."""
    member = lambda row: in_set(c, int(jbeg[row[0]]) + int(row[1]))
    rest = iter([row for row in B if not member(row)])
    return np.array([row if member(row) else next(rest) for row in A], np.int64).reshape(-1, 3)


def _least(keys):
    return min(range(len(keys)), key=lambda i: (keys[i], i))


def evolve_one(inst, variant, pop, w, generations, mut_rate, seed=0, g=0):
    pop = np.asarray(pop, np.int32)
    P, cap = pop.shape[0], pop.shape[1]
    NO = SF.n_objectives(variant)
    w = [int(x) for x in w]
    assert len(w) == NO and 1 <= P <= 64 and 0 <= mut_rate <= MUT_ONE
    out = dict(population=pop.copy(), population_objective=np.full((P, NO), -1, np.int64), plan=pop[0].copy(),
               objective=np.full(NO, -1, np.int64), history=np.full(generations + 1, -1, np.int64), status=0,
               trace=np.zeros((generations, P, 3), np.int32), children=[], ties=[])
    if any(x < 0 for x in w) or all(x == 0 for x in w):
        out["status"] = SF.BAD_WEIGHTS
        return out
    first = [SF.decode_one(inst, variant, pop[q], None, cap) for q in range(P)]
    bad = [r["status"] for r in first if r["status"] != 0]
    if bad:
        out["status"] = bad[0]                                          # (of the lowest such q)
        return out
    Jr, p = np.asarray(inst.Jr, np.int64), np.asarray(inst.p, np.int64)
    koff = np.concatenate(([0], np.cumsum(Jr)))
    jbeg = job_numbers(inst)
    L = first[0]["length"]
    assert all(r["length"] == L for r in first)
    rows = [pop[q][:L].astype(np.int64) for q in range(P)]
    vecs = [tuple(int(x) for x in r["objective"]) for r in first]
    keys = [SF.key_of(w, v) for v in vecs]
    out["history"][0] = min(keys)
    s = env_stream(seed, g)
    for t in range(1, generations + 1):
        best = _least(keys)
        new_rows, new_vecs, new_keys, made = [], [], [], []
        for q in range(P):
            c = child_stream(s, t, P, q)
            if q == 0:
                a = b = best
                child = rows[best].copy()
                u = -1
            else:
                picks = [S.pick(draw(c, i), P) for i in range(4)]
                parents = []
                for n, (x, y) in enumerate((picks[:2], picks[2:])):
                    if x != y and keys[x] == keys[y]:
                        out["ties"].append((t, q, n))
                    parents.append(min((x, y), key=lambda i: (keys[i], i)))
                a, b = parents
                child = crossover(rows[a], rows[b], jbeg, c)
                u = S.pick(draw(c, 5), L) if S.pick(draw(c, 4), MUT_ONE) < mut_rate else -1
            plain = child.copy()
            if u >= 0:
                stage = int(np.sum((child[:u, 0] == child[u, 0]) & (child[:u, 1] == child[u, 1])))
                elig = np.flatnonzero(p[koff[child[u, 0]] + stage] > 0)
                child[u, 2] = int(elig[S.pick(draw(c, 6), len(elig))])
            res = SF.decode_one(inst, variant, S._padded(child, cap), None, cap)
            made.append((plain, child.copy(), res["status"]))
            vec = tuple(int(x) for x in res["objective"])
            new_rows.append(child if res["status"] == 0 else child[:0])
            new_vecs.append(vec)
            new_keys.append(SF.key_of(w, vec) if res["status"] == 0 else NONE_KEY)
            out["trace"][t - 1, q] = (a, b, u)
        rows, vecs, keys = new_rows, new_vecs, new_keys
        out["children"].append(made)
        out["history"][t] = min(keys)
    best = _least(keys)
    out.update(population=np.stack([S._padded(r, cap) for r in rows]), population_objective=np.array(vecs, np.int64).reshape(P, NO),
               plan=S._padded(rows[best], cap), objective=np.asarray(vecs[best], np.int64))
    return out


def evolve(insts, variant, pops, weights, generations, mut_rate, seed=0, first_env=0):
    """insts[e]: env e's instance; pops int[N][P][cap][3]; weights int[N][NO].  dict(population int32[N][P][cap][3],
    population_objective int64[N][P][NO], plan int32[N][cap][3], objective int64[N][NO], history int64[generations + 1][N],
    status int32[N], trace int32[generations][N][P][3]; children, ties: lists per env)."""
    N = len(insts)
    ones = [evolve_one(insts[e], variant, pops[e], weights[e], generations, mut_rate, seed, first_env + e) for e in range(N)]
    stack = lambda key, dtype, axis=0: np.stack([np.asarray(o[key]) for o in ones], axis).astype(dtype)
    return dict(population=stack("population", np.int32), population_objective=stack("population_objective", np.int64),
                plan=stack("plan", np.int32), objective=stack("objective", np.int64), history=stack("history", np.int64, 1),
                status=stack("status", np.int32), trace=stack("trace", np.int32, 1), children=[o["children"] for o in ones],
                ties=[o["ties"] for o in ones])
