"""Instances, actions and conditions of the size-limit tests of the one-wave-per-environment kernels (csrc/fjsp_kernels.hip).

Shared by tests/test_wave_limit_cases_host.py (CPU: the C oracle plays every case and proves the condition the case exists
for; the create-time limit pairs) and tests/test_gpu_wave_limits.py (the kernels against the oracle at every step).

A case is (family, shape, variant): a few instances built with InstanceSet.set_raw from a seeded generator, at offset
FIRST inside their set, played by N_ENVS = 6 environments (env e plays instance e % n_inst; 6 is no multiple of the 4
environments of a workgroup) under seeded random actions over the variant's whole action space.  Processing times are
1..5 and the eligible machines of an operation type are drawn from one to all M unless the family says otherwise.  Every
machine has an eligible operation (SO_DFJSP and MO_DFJSP divide by that count).  `edge` names the instances that carry the
limit; the others are fillers that share the batch's padded sizes.  condition(case, e, rec, acts) is the predicate on the
oracle's replay of environment e that the edge instances must satisfy.

    chunks    largest K = 64 | 65, 128 | 129, 255 | 256 (one, two, four chunks of 64 operation types), kinds of 1..16
              stages, 2 jobs per kind (the general walk, not single_job); fillers with K = 1 and K = 64, so that a 2- or
              4-chunk build also opens records whose upper chunks are empty.  SO_FJSSP, SO_SFJSP, MO_FJSSP_discretes,
              SO_DFJSP.  Condition: an operation type of the instance's last chunk is dispatched.
    kinds     R = 255 | 256 kinds of one stage and one job: index 255 in the 8-bit kind field; the batch is single_job at
              255 and not at 256 (check_instance).  SO_FJSSP, SO_DFJSP.  Condition: the highest kind is dispatched.
    stages    a kind of 254 | 255 stages (one job) beside a kind of one stage on a machine of its own (45 jobs of 100
              time units, so the long job finishes while the shop is busy): SO_FJSSP, SO_SFJSP; MO_DFJSP with 253 | 254
              stages, its limit.  "two": two orders of one job per kind, SO_FJSSP, 253 | 254 stages likewise.  Condition:
              a job of the long kind finishes at least 20 steps before the episode's end; "two": and before the second
              order's last job does.
    machines  M = 8 | 9 | 31 | 32, 6 kinds x 4 stages, 3 jobs per kind; operation type 0 runs on all M, two of every kind's
              stages run on machine M - 1 alone; a filler with M = 3.  MO_DFJSP: power, idle power and up to 4 breakdown
              windows on every machine.  SO_FJSSP, MO_DFJSP, SO_DFJSP.  Condition: machine M - 1 is chosen under a
              deterministic and under the random machine rule; MO_DFJSP: and one of its windows delays a dispatch.
    jobs      2 kinds x 1 stage with 16 | 17 (jcap), 64 | 65, 128 | 129 (JP) jobs, 65 of them in one kind from 128 on; "131":
              3 kinds with 129 jobs in one.  SO_FJSSP, SO_SFJSP.  Condition: every job number of the largest kind is dispatched.
    orders    S = 64 orders of kinds [1, 2] stages, one job per kind and order.  "gap7": arrivals 7 apart, the shop runs
              empty and the clock jumps to the next arrival; "burst": four orders at 0 and sixty at 30, operation types
              bound to one machine each.  SO_FJSSP, MO_DFJSP.  Condition: at least 20 idle jumps; at least two arrivals
              within one step (at one step_time).
    late      R = 256 kinds of one job, order delivery at the most negative value check_instance admits, SO_DFJSP (due
              date = order delivery): every tardiness is close to 2^31, their total close to 2^39.  Condition:
              delay_time_sum > 2^38.
    chunk_orders  the chunks family with order arrivals: largest K = 65 | 128 | 129 (two, two and four chunks), kinds of
              1..16 stages, three orders (at 0, 25, 50) of one job per kind; fillers with K = 1 (one order: an environment
              that never waits for an arrival) and K = 64 (two orders), so the batch runs the kernels with order arrivals
              and a 2- or 4-chunk build also opens records whose upper chunks are empty.  SO_FJSSP, SO_DFJSP.  Condition:
              S - 1 arrivals happen and an operation type of the last chunk is dispatched after the first of them.
              Appended to case_ids() with a seed base of its own: the older cases keep their instances and actions.
"""
import numpy as np

from tests import async_cases as AC

FIRST = 2                        # the instances sit at an offset inside the set
N_ENVS = 6
RNG_SEED = 911                   # rng_seed of every batch of these tests
ENV_SEED_STRIDE = AC.ENV_SEED_STRIDE
ACTION_SPACE = {0: (6, 5), 1: (20, 1), 2: (18, 1), 4: (12, 10), 5: (6, 5)}
RANDOM_MACHINE_RULE = {0: 4, 5: 4, 4: 9}       # the machine rule that ends in random.choice (SO_FJSSP.py:320, MO_DFJSP_breakdown.py:428)
DET_PAIR = {0: (2, 0), 1: (0, 0), 2: (0, 0), 4: (2, 0), 5: (2, 0)}
STATE_KW = {0: {}, 1: dict(sf=True), 2: dict(mo=True), 4: dict(dyn=True), 5: {}}
MAX_STEPS = 520

CHUNK_K = (64, 65, 128, 129, 255, 256)
CHUNK_ORDERS_K = (65, 128, 129)
CHUNK_ORDERS_ARRIVE = (0, 25, 50)
CHUNK_ORDERS_SEED = 20000        # the family's own seed base (the older families: 7000 + 131 x their sorted index)
MACHINE_M = (8, 9, 31, 32)
JOB_TOTALS = {"16": (8, 8), "17": (9, 8), "64": (32, 32), "65": (33, 32), "128": (65, 63), "129": (65, 64), "131": (129, 1, 1)}
ORDERS_S = 64
# stages of the long kind, up to the longest a batch may hold: 255 in a single-order batch, 254 in a batch with order arrivals
# (several orders, MO_DFJSP), whose jobs keep 255 in their next-stage byte while their order has not arrived (fjsp_env_create)
STAGES_SINGLE = (254, 255)
STAGES_ARRIVALS = (253, 254)


def case_ids():
    """[(family, shape, variant)] of every case, cheap: nothing is built."""
    out = [("chunks", str(K), v) for K in CHUNK_K for v in (0, 1, 2, 5)]
    out += [("kinds", str(R), v) for R in (255, 256) for v in (0, 5)]
    out += [("stages", "so", v) for v in (0, 1, 4)] + [("stages", "two", 0)]
    out += [("machines", str(M), v) for M in MACHINE_M for v in (0, 4, 5)]
    out += [("jobs", n, v) for n in JOB_TOTALS for v in (0, 1)]
    out += [("orders", pat, v) for pat in ("gap7", "burst") for v in (0, 4)]
    out += [("late", "256", 5)]
    # families added later go last (actions() seeds by position) and bring their own seed base (_build)
    out += [("chunk_orders", str(K), v) for K in CHUNK_ORDERS_K for v in (0, 5)]
    return out


def case_name(cid):
    return "%s-%s-v%d" % cid


class Arr(object):
    """One instance: the arguments of InstanceSet.set_raw."""


def make(name, seed, Jr, M, count, arrive=(0,), delivery=None, p_range=(1, 5), full_ops=(), bound=None):
    """Seeded instance.  count: jobs per kind (one order) or [S][R].  bound: {operation type: machine} for types that run
    on that machine alone; full_ops: types eligible on all M; the others draw 1..M machines.  A machine left without an
    operation gets one.  delivery None: each order is due half of its serial work per machine after it arrives."""
    rs = np.random.RandomState(seed)
    a = Arr()
    a.name, a.Jr = name, np.asarray(Jr, np.int32)
    a.R, a.M = len(Jr), M
    K = a.K = int(a.Jr.sum())
    a.arrive = np.asarray(arrive, np.int32)
    a.S = len(a.arrive)
    a.count = np.asarray(count, np.int32).reshape(a.S, a.R)
    bound = bound or {}
    el = np.zeros((K, M), bool)
    for k in range(K):
        if k in bound:
            el[k, bound[k]] = True
        elif k in full_ops:
            el[k] = True
        else:
            el[k, rs.choice(M, int(rs.randint(1, M + 1)), replace=False)] = True
    free = [k for k in range(K) if k not in bound]
    for m in np.nonzero(~el.any(axis=0))[0]:
        el[free[int(rs.randint(len(free)))], m] = True
    t = rs.randint(p_range[0], p_range[1] + 1, (K, M))
    a.p = np.where(el, t, 0).astype(np.int32)
    a.elig_n = el.sum(1).astype(np.int32)
    a.elig_list = np.zeros((K, M), np.int32)
    for k in range(K):
        ms = np.nonzero(el[k])[0]
        a.elig_list[k, :len(ms)] = ms
    if delivery is None:
        work = (a.count * a.Jr[None, :]).sum(1) * float(np.mean(p_range))
        delivery = a.arrive + np.maximum(1, work / (2.0 * M)).astype(np.int64)
    a.delivery = np.asarray(delivery, np.int32)
    a.ddt = 1.0
    return a


def ops_total(a):
    return int((a.count * a.Jr[None, :]).sum())


def _kinds(rs, K):
    """Kinds of 1..16 stages that add up to K operation types."""
    Jr = []
    while sum(Jr) < K:
        Jr.append(min(int(rs.randint(1, 17)), K - sum(Jr)))
    return Jr


def late_delivery(ops, pmax):
    """The most negative order delivery check_instance admits (csrc/fjsp_env.hip): worst-case clock + |delivery| <= 2^31 - 1
    with one job per kind and one order at 0."""
    return -(2 ** 31 - 1 - ops * pmax)


class Case(object):
    def __init__(self, cid, arrs, edge=None, finite=False, record=False, windows=0):
        self.id, self.name = cid, case_name(cid)
        self.family, self.shape, self.variant = cid
        self.arrs, self.n_inst = arrs, len(arrs)
        self.edge = list(range(len(arrs))) if edge is None else edge
        self.finite = finite          # also assert that no state entry is NaN or infinite
        self.record = record          # also compare the recorded schedule with the oracle's
        self.windows = windows        # MO_DFJSP: breakdown windows per machine (up to)
        self.T = max(ops_total(a) for a in arrs)
        assert self.T <= MAX_STEPS, (self.name, self.T)


_CASES = {}


def case(cid):
    if cid not in _CASES:
        _CASES[cid] = _build(cid)
    return _CASES[cid]


def _build(cid):
    family, shape, v = cid
    tag = case_name(cid)
    if family == "chunk_orders":
        K, M = int(shape), 6
        seed = CHUNK_ORDERS_SEED + 131 * CHUNK_ORDERS_K.index(K) + v
        rs = np.random.RandomState(seed)
        fill = _kinds(rs, 64)
        big = _kinds(rs, K)
        arrs = [make(tag + "/k1", seed + 1, [1], M, [2], full_ops=(0,)),
                make(tag + "/k64", seed + 2, fill, M, np.ones((2, len(fill))), arrive=CHUNK_ORDERS_ARRIVE[:2]),
                make(tag + "/edge", seed + 3, big, M, np.ones((3, len(big))), arrive=CHUNK_ORDERS_ARRIVE)]
        return Case(cid, arrs, edge=[2], record=K == 128)
    seed = 7000 + 131 * sorted(set(c[:2] for c in case_ids() if c[0] != "chunk_orders")).index(cid[:2]) + v
    rs = np.random.RandomState(seed)
    if family == "chunks":
        K, M = int(shape), 6
        fill = _kinds(rs, 64)
        big = _kinds(rs, K)
        arrs = [make(tag + "/k1", seed + 1, [1], M, [2], full_ops=(0,)),
                make(tag + "/k64", seed + 2, fill, M, [2] * len(fill)),
                make(tag + "/edge", seed + 3, big, M, [2] * len(big))]
        return Case(cid, arrs, edge=[2], record=K == 256)
    if family == "kinds":
        R = int(shape)
        return Case(cid, [make(tag, seed + 1, [1] * R, 4, [1] * R)])
    if family == "stages":
        arrs = []
        single = shape == "so" and v != 4
        for L in (STAGES_SINGLE if single else STAGES_ARRIVALS):
            arrs.append(_stages_instance("%s/%d" % (tag, L), seed + L, L, shape))
        return Case(cid, arrs, finite=True, windows=4 if v == 4 else 0)
    if family == "machines":
        M = int(shape)
        Jr = [4] * 6
        # stages 1 and 3 of every kind run on machine M - 1 alone, operation type 0 on all M
        bound = {4 * r + j: M - 1 for r in range(6) for j in (1, 3)}
        arrs = [make(tag + "/edge", seed + 1, Jr, M, [3] * 6, full_ops=(0,), bound=bound),
                make(tag + "/m3", seed + 2, [3, 2], 3, [2, 2], full_ops=(0,))]
        return Case(cid, arrs, edge=[0], record=M == 32, windows=4 if v == 4 else 0)
    if family == "jobs":
        counts = JOB_TOTALS[shape]
        R = len(counts)
        arrs = [make(tag + "/edge", seed + 1, [1] * R, 3, list(counts)),
                make(tag + "/j2", seed + 2, [1, 1], 3, [1, 1])]
        return Case(cid, arrs, edge=[0])
    if family == "orders":
        S = ORDERS_S
        if shape == "gap7":
            arrive = 7 * np.arange(S)
            a = make(tag, seed + 1, [1, 2], 3, np.ones((S, 2)), arrive=arrive, delivery=arrive + 4, p_range=(1, 3))
        else:
            arrive = np.array([0] * 4 + [30] * (S - 4))
            a = make(tag, seed + 1, [1, 2], 3, np.ones((S, 2)), arrive=arrive, delivery=arrive + 20, bound={0: 0, 1: 1, 2: 2})
            # machines 0 and 1 (the first stages, 5 and 4 time units) stay busy through the burst, machine 2 (the last stage,
            # 1 time unit) falls idle with nothing waiting for it: its completions bring orders in without ending the step
            a.p[0, 0], a.p[1, 1], a.p[2, 2] = 5, 4, 1
        return Case(cid, [a], finite=True, record=True)
    if family == "late":
        R = int(shape)
        a = make(tag, seed + 1, [1] * R, 4, [1] * R)
        a.p[0, a.elig_list[0, 0]] = 5                       # the largest processing time is exactly 5
        a.delivery = np.array([late_delivery(R, 5)], np.int32)
        return Case(cid, [a])
    raise KeyError(cid)


def _stages_instance(name, seed, L, shape):
    """Kind 0: L stages, each on machine 0, 1 or both; kind 1: one stage on machine 2 alone."""
    M = 3
    if shape == "so":       # 45 short jobs of 100 time units: machine 2 is busy long after the long job has finished
        a = make(name, seed, [L, 1], M, [1, 45], bound={L: 2})
        a.p[L, 2] = 100
    else:                   # two orders of one job per kind, the second arrives at 40
        a = make(name, seed, [L, 1], M, [[1, 1], [1, 1]], arrive=(0, 40), bound={L: 2})
    el = a.p[:L] > 0
    el[:, 2] = False        # the long kind keeps off machine 2
    el[~el.any(axis=1), 0] = True
    rs = np.random.RandomState(seed + 1)
    a.p[:L] = np.where(el, rs.randint(1, 6, (L, M)), 0)
    a.elig_n[:L] = el.sum(1)
    a.elig_list[:L] = 0
    for k in range(L):
        ms = np.nonzero(el[k])[0]
        a.elig_list[k, :len(ms)] = ms
    assert (a.p > 0).any(axis=0).all()
    return a


def instance_set(c):
    """The product InstanceSet of case c: its instances from FIRST on, with the host solver's reset-time fluid solution
    (and MO_DFJSP: machine data; c.windows breakdown windows per machine at most)."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    s = fi.InstanceSet(FIRST + c.n_inst)
    for i, a in enumerate(c.arrs):
        s.set_raw(FIRST + i, a.Jr, a.p, a.elig_n, a.elig_list, a.count, a.arrive, a.delivery, a.ddt)
    s.solve_fluid(FIRST, c.n_inst)
    if c.variant == 4:
        for i in range(c.n_inst):
            s.generate_machine_data(FIRST + i, 900 + i, max_windows=c.windows, window_gap=(1, 60), window_len=(1, 30))
            if c.family == "machines" and i in c.edge:
                _top_machine_windows(s, FIRST + i)
    return s


def _top_machine_windows(s, i):
    """Machine M - 1 gets four short windows inside the first 40 time units, where it is dispatched to again and again."""
    a = s.arrays(i)
    off = np.concatenate(([0], np.cumsum(a.bk_n)))
    bk = [a.bk[off[m]:off[m + 1]] for m in range(a.M - 1)] + [np.array([(3, 6), (12, 15), (22, 26), (34, 38)], np.int32)]
    a.bk_n[a.M - 1] = 4
    s.set_dynamic(i, a.power, a.idle_power, a.bk_n, np.concatenate(bk).reshape(-1, 2))


def set_arrays(c, s=None):
    """InstanceSet.arrays of every instance of the case (with x and the machine data), named like the case's."""
    s = instance_set(c) if s is None else s
    out = []
    for i, a in enumerate(c.arrs):
        b = s.arrays(FIRST + i)
        b.name = a.name
        out.append(b)
    return out


def env_seed(e):
    return (RNG_SEED + e * ENV_SEED_STRIDE) & (2 ** 64 - 1)


def actions(c):
    """uint8[T, N_ENVS, 2]: a random rule pair per env and step over the variant's whole action space."""
    rs = np.random.RandomState(30000 + case_ids().index(c.id))
    n0, n1 = ACTION_SPACE[c.variant]
    return np.stack([rs.randint(0, n0, (c.T, N_ENVS)), rs.randint(0, n1, (c.T, N_ENVS))], 2).astype(np.uint8)


def mo_rows(c):
    """step()'s extra arguments per env: MO_FJSSP_discretes weight vectors with and without normalisers, MO_DFJSP reward
    policies 0..3 with normalisers (as test_randomised_differential_vs_oracle draws them); None for the other variants."""
    rs = np.random.RandomState(77 + c.variant)
    if c.variant == 2:
        kinds, w0 = rs.randint(0, 3, N_ENVS), np.round(rs.rand(N_ENVS), 2)
        return [(1.0, 0.0, -1.0, -1.0) if k == 0 else (0.0, 1.0, -1.0, -1.0) if k == 1 else
                (float(w0[e]), float(1.0 - w0[e]), float(rs.randint(20, 90)), float(rs.randint(30, 400))) for e, k in enumerate(kinds)]
    if c.variant == 4:
        return [(float(rs.randint(0, 4)), float(rs.randint(20, 90)), float(rs.choice([0.0, 17.0, 250.0])), float(rs.randint(500, 5000)))
                for _ in range(N_ENVS)]
    return None


def replay(c, arrs, acts):
    """Every environment of the case on the C oracle: tests.helpers.play_oracle dicts, env e on instance e % n_inst."""
    from tests import helpers as H
    mo = mo_rows(c)
    return [H.play_oracle(arrs[e % c.n_inst], arrs[e % c.n_inst].x, acts[:, e], env_seed(e), variant=c.variant,
                          mo=None if mo is None else mo[e]) for e in range(N_ENVS)]


def dispatch_rows(a, rec):
    """(rows, delayed): the schedule rows (r, j, n, m, time_begin, time_end) of a replay in dispatch order, and per dispatch
    whether a breakdown window of its machine moved its start or its end.  The task starts at the clock before its step; a
    window of the machine that covers the start moves start and end behind it, one that begins inside the task stretches
    the end by its length, in the machine's window order (MO_DFJSP_breakdown.py:204-231)."""
    koff = np.concatenate(([0], np.cumsum(a.Jr)))
    k, m = np.asarray(rec["k"], np.int64), np.asarray(rec["m"], np.int64)
    r = np.searchsorted(koff, k, side="right") - 1
    clock = np.concatenate(([0], np.asarray(rec["step_time"], np.int64)[:-1]))
    begin, end = clock.copy(), clock + np.asarray(a.p, np.int64)[k, m]
    delayed = np.zeros(len(k), bool)
    if hasattr(a, "bk_n"):
        off = np.concatenate(([0], np.cumsum(a.bk_n)))
        for t in range(len(k)):
            for bs, be in np.asarray(a.bk, np.int64).reshape(-1, 2)[off[m[t]]:off[m[t] + 1]]:
                if bs <= clock[t] < be:
                    begin[t] += be - clock[t]; end[t] += be - clock[t]; delayed[t] = True
                elif clock[t] < bs < end[t]:
                    end[t] += be - bs; delayed[t] = True
                elif bs > end[t]:
                    break
    return np.stack([r, k - koff[r], np.asarray(rec["job_n"], np.int64), m, begin, end], 1), delayed


def arrival_steps(c, a, acts_e, e):
    """The 0-based steps of env e's episode in which an order arrived (one entry per arrival after reset)."""
    mo = mo_rows(c)
    return [step for step, _, _ in AC.arrivals(a, acts_e, env_seed(e), c.variant, None if mo is None else mo[e])[1]]


def idle_jumps(a, rec):
    """Steps after which every job that has arrived is finished and the clock stands at the next order's arrival."""
    per_order = (a.count * a.Jr[None, :]).sum(1)
    done_after = np.cumsum(per_order)
    n = 0
    for s in range(1, a.S):
        t = int(done_after[s - 1]) - 1          # the step that dispatched the last operation of orders 0 .. s - 1
        if t < rec["T"] - 1 and rec["step_time"][t] == a.arrive[s] and (s == 1 or rec["step_time"][t - 1] < a.arrive[s]):
            n += 1
    return n


def condition(c, e, a, rec, acts_e):
    """The condition case c exists for, on the oracle's replay `rec` of env e (instance arrays a, actions acts_e).
    Returns (holds, what was measured)."""
    T = rec["T"]
    if c.family == "chunks":
        last = (a.K - 1) // 64
        n = int((rec["k"] // 64 == last).sum())
        return n > 0 and a.K == int(c.shape), "dispatches in chunk %d: %d" % (last, n)
    if c.family == "kinds":
        hit = bool((rec["job_r"] == a.R - 1).any())
        return hit and a.R == int(c.shape), "kind %d dispatched: %s" % (a.R - 1, hit)
    if c.family == "stages":
        L = int(a.Jr[0])
        ends = np.nonzero((rec["job_r"] == 0) & (rec["k"] == L - 1))[0]
        ok = len(ends) > 0 and int(ends[0]) <= T - 1 - 20
        if c.shape == "two":
            ok = ok and int(ends[0]) < int(np.nonzero(rec["job_n"] == 1)[0].max())
        return ok, "long job finishes at step %s of %d" % (ends[:1], T)
    if c.family == "machines":
        top = rec["m"] == a.M - 1
        rnd = acts_e[:T, 1] == RANDOM_MACHINE_RULE[c.variant]
        ok = bool((top & rnd).any()) and bool((top & ~rnd).any())
        what = "machine %d: %d random, %d deterministic choices" % (a.M - 1, (top & rnd).sum(), (top & ~rnd).sum())
        if c.variant == 4:
            delayed = dispatch_rows(a, rec)[1]
            ok = ok and bool((top & delayed).any())
            what += ", %d delayed by its windows" % (top & delayed).sum()
        return ok and a.M == int(c.shape), what
    if c.family == "jobs":
        r = int(np.argmax(a.count[0]))
        seen = set(rec["job_n"][rec["job_r"] == r].tolist())
        return seen == set(range(int(a.count[0, r]))) and int(a.count.sum()) == sum(JOB_TOTALS[c.shape]), "%d job numbers" % len(seen)
    if c.family == "orders":
        if c.shape == "gap7":
            n = idle_jumps(a, rec)
            return n >= 20 and a.S == ORDERS_S, "%d idle jumps" % n
        steps = arrival_steps(c, a, acts_e, e)
        most = max(steps.count(t) for t in set(steps))
        return most >= 2 and len(steps) == a.S - 1 == ORDERS_S - 1, "up to %d arrivals in one step" % most
    if c.family == "late":
        return rec["delay_time_sum"] > 2 ** 38, "delay_time_sum %d" % rec["delay_time_sum"]
    if c.family == "chunk_orders":
        steps = sorted(arrival_steps(c, a, acts_e, e))
        last = (a.K - 1) // 64
        n = int((rec["k"][steps[0] + 1:] // 64 == last).sum()) if steps else 0
        ok = len(steps) == a.S - 1 == 2 and n > 0 and a.K == int(c.shape) and last == (1 if a.K <= 128 else 2)
        return ok, "arrivals in steps %s, %d dispatches in chunk %d after the first" % (steps, n, last)
    raise KeyError(c.family)
