"""Generated fluid-LP cases for the device simplex (csrc/fjsp_lp_device.hip) that reach what the fixture instances do not.

Shared by tests/test_lp_reference.py (CPU: the restatement of tests/lp_reference.py against the host solver and HiGHS, and
the coverage these cases must keep) and tests/test_gpu_lp_device.py (the device solver against the host solver, bit for
bit).  A case is an instance built with InstanceSet.set_raw from a seeded generator -- two orders, so that a batch of it
has the order-arrival service -- plus several (Q, n_now) states: the reset-time state, jobs spread over the stages
(precedence rows come and go with n_now == 0), and one state with every n_now[k + 1] > 0 (no precedence rows).

Shapes (rows nr = K + M + precedence rows, columns nc = nx + nr + 2; worst case = every precedence row present):

    c2     K 12 M  5 R  4 full eligibility   nr 25  nc  87   2 chunks
    c3     K 15 M  8 R  5 full               nr 33  nc 155   3 chunks
    c4     K 20 M 10 R  5 full               nr 45  nc 247   4 chunks                       lp_pivots<4>
    c6     K 22 M 15 R 15 full               nr 44  nc 376   6 chunks, t in the last one    lp_pivots<6>, RB = 2
    c7     K 16 M 24 R 12 full               nr 44  nc 430   7 chunks                       lp_pivots<8>
    c8     K 20 M 21 R 19 nx 410             nr 42  nc 454   8 chunks (158 KB of 159 744 B)  lp_pivots<8>, last chunk used
    rows4  K 30 M 16 R  6 nx 178             nr 70  nc 250   4 chunks, rows 64-69 in the second half
    rows4b K 40 M 10 R  4 3 machines per op  nr 86  nc 208   4 chunks, rows 64-85 in the second half
    rowsM  K 60 M  8 R 55 2 machines per op  nr 73  nc 195   4 chunks, machine rows 64-67 in the second half
    d111 / dM1 / dK1                         one kind x one operation x one machine; M = 1; K = 1
    wide_p K 12 M  5 R  4 full, processing times log-uniform over 1 ... 65 535 (1 and 65 535 on one machine)
    s<seed>                                  small LPs of the ratio-test search below

Job counts: a few per kind, the training distribution's hundreds per kind, and Q up to 65 535 (states "big").

Ratio-test search.  `search_ratio_classes` runs the restatement over small seeded LPs (`search_case`) and counts the
pivots per class of the device's ratio test.  Bound: seeds 0 ... 99 999, three states each (chosen by CPU time: two
minutes on 8 cores, `python -m tests.lp_cases`).  SEARCH_RESULT holds what it found -- 3 059 939 pivots, 4 860 of them
decided by magnitudes, 11 409 with near-ties of different ratios (`bad`), none that fired the `small` underflow guard and
none whose column walk ended on signs alone -- and SEARCH_SEEDS the seeds committed as cases, at least one per class found;
tests/test_lp_reference.py asserts that the committed cases still reach each of those classes.
"""
import numpy as np

LDS_LIMIT = 156 * 1024           # csrc/fjsp_env.hip choose_lp_service
MAX_COLUMNS = 512                # csrc/fjsp_lp_limits.h kLpLdsColumns (csrc/fjsp_lp_device.hip: kZT * 64)


def lds_bytes(K, M, nx, R, MP):
    """csrc/fjsp_lp_limits.h lp_device_lds_bytes, restated: the LDS of the largest tableau an instance can need."""
    nr = K + M + (K - R)
    nc = nx + 1 + nr + 1
    b = nr * nc * 8 + nc * 8 + 2 * nr * 8 + nr * 4 + K * M * 2 + K * 2 + nr * 2 + K * MP * 2 + K * 8 + 128
    return (b + 15) & ~15


def fits_device(arrs):
    """csrc/fjsp_env.hip choose_lp_service for a batch of these instances (MP = the batch's largest M)."""
    MP = max(a.M for a in arrs)
    for a in arrs:
        nx = int((a.p > 0).sum())
        if lds_bytes(a.K, a.M, nx, a.R, MP) > LDS_LIMIT or nx + 1 + (a.K + a.M + a.K - a.R) + 1 > MAX_COLUMNS:
            return False
    return True


class Arr(object):
    """One generated instance: the arguments of InstanceSet.set_raw."""


def make_instance(name, seed, Jr, M, nx=None, per_op=None, p_range=(1, 20), log_p=False, count=2, arrive1=10):
    """Seeded instance.  nx: full eligibility with K * M - nx random pairs removed; per_op: that many machines per
    operation; neither: full eligibility.  Two orders (the second arrives at arrive1) of `count` jobs per kind."""
    rs = np.random.RandomState(seed)
    a = Arr()
    a.name, a.Jr = name, np.asarray(Jr, np.int32)
    a.R, a.S, a.M = len(Jr), 2, M
    K = a.K = int(a.Jr.sum())
    el = np.ones((K, M), bool)
    if per_op is not None:
        el[:] = False
        for k in range(K):
            el[k, rs.choice(M, per_op, replace=False)] = True
    elif nx is not None:
        while el.sum() > nx:
            k, m = rs.randint(K), rs.randint(M)
            if el[k, m] and el[k].sum() > 1 and el[:, m].sum() > 1:
                el[k, m] = False
    if log_p:
        t = np.floor(np.exp(rs.uniform(np.log(p_range[0]), np.log(p_range[1] + 1), (K, M)))).astype(np.int64)
        t = np.clip(t, p_range[0], p_range[1])
        m0 = int(np.argmax(el.sum(0)))
        ks = np.nonzero(el[:, m0])[0]
        t[ks[0], m0], t[ks[-1], m0] = p_range[0], p_range[1]     # the two ends of the range meet in one machine row
    else:
        t = rs.randint(p_range[0], p_range[1] + 1, (K, M))
    a.p = np.where(el, t, 0).astype(np.int32)
    a.elig_n = el.sum(1).astype(np.int32)
    a.elig_list = np.zeros((K, M), np.int32)
    for k in range(K):
        ms = np.nonzero(el[k])[0]
        a.elig_list[k, :len(ms)] = ms
    a.count = np.full((2, a.R), count, np.int32)
    a.arrive = np.array([0, arrive1], np.int32)
    a.delivery = np.array([400, 400 + arrive1], np.int32)
    a.ddt = 1.0
    return a


def state_from_stages(a, stages_of_kind):
    """Q = tasks of (r, j) still unprocessed, n_now = jobs waiting at (r, j) (class_FJSSP.py:234-237) for jobs at the
    given stages."""
    koff = np.concatenate(([0], np.cumsum(a.Jr)))
    Q = np.zeros(a.K, np.int32); now = np.zeros(a.K, np.int32)
    for r in range(a.R):
        st = np.asarray(stages_of_kind[r])
        for j in range(int(a.Jr[r])):
            Q[koff[r] + j] = max(1, int((st <= j).sum()))
            now[koff[r] + j] = int((st == j).sum())
    return Q, now


def make_states(a, seed, jobs=(1, 25), big=False):
    """[(label, Q, n_now)]: reset-time, two spread states, one without precedence rows (and one with Q up to 65 535)."""
    rs = np.random.RandomState(seed)
    out = []
    n = [int(rs.randint(jobs[0], jobs[1] + 1)) for _ in range(a.R)]
    out.append(("reset",) + state_from_stages(a, [np.zeros(n[r], np.int64) for r in range(a.R)]))
    for t in range(2):
        st = []
        for r in range(a.R):
            s = rs.randint(0, a.Jr[r], int(rs.randint(jobs[0], jobs[1] + 1)))
            if t:
                s[0] = a.Jr[r] - 1
            st.append(s)
        out.append(("spread%d" % t,) + state_from_stages(a, st))
    st = [np.concatenate([np.arange(a.Jr[r]), rs.randint(0, a.Jr[r], int(rs.randint(jobs[0], jobs[1] + 1)))]) for r in range(a.R)]
    out.append(("noprec",) + state_from_stages(a, st))
    if big:
        st = [rs.randint(0, a.Jr[r], 65535 if r % 2 == 0 else int(rs.randint(30000, 65535))) for r in range(a.R)]
        out.append(("big",) + state_from_stages(a, st))
    return out


class Case(object):
    def __init__(self, arr, states):
        self.arr, self.states, self.name = arr, states, arr.name


def search_case(seed):
    """A small seeded LP family of the ratio-test search: shapes and number ranges drawn from the seed."""
    rs = np.random.RandomState(100000 + seed)
    R = int(rs.randint(1, 5))
    Jr = rs.randint(1, 5, R)
    M = int(rs.randint(2, 7))
    p_range, log_p = [((1, 3), False), ((1, 20), False), ((40, 400), False), ((1, 65535), True)][int(rs.randint(4))]
    per_op = int(rs.randint(1, M + 1))
    a = make_instance("s%d" % seed, 200000 + seed, Jr, M, per_op=per_op if per_op < M else None, p_range=p_range, log_p=log_p)
    jobs = [(1, 5), (1, 25), (100, 600)][int(rs.randint(3))]
    return Case(a, make_states(a, 300000 + seed, jobs)[:3])


# What `python -m tests.lp_cases` (search_ratio_classes over seeds 0 ... 99 999) reported, and the seeds kept as cases.
SEARCH_BOUND = 100000
SEARCH_RESULT = {"pivots": 3059939, "magnitude": 4860, "sign": 0, "small": 0, "bad": 11409}
SEARCH_SEEDS = {"magnitude": (6822, 16464, 39100), "bad": (19423, 39100)}


def cases():
    out = []
    add = lambda a, seed, **kw: out.append(Case(a, make_states(a, seed, **kw)))
    add(make_instance("c2", 11, [3] * 4, 5), 111, big=True)
    add(make_instance("c3", 12, [3] * 5, 8), 112, jobs=(100, 600))
    add(make_instance("c4", 13, [4] * 5, 10), 113, big=True)
    add(make_instance("c6", 14, [2] * 7 + [1] * 8, 15), 114)
    add(make_instance("c7", 15, [2] * 4 + [1] * 8, 24), 115, jobs=(100, 600))
    add(make_instance("c8", 16, [2] + [1] * 18, 21, nx=410), 116)
    add(make_instance("rows4", 17, [5] * 6, 16, nx=178), 117)
    add(make_instance("rows4b", 18, [10] * 4, 10, per_op=3), 118, jobs=(100, 600))
    add(make_instance("rowsM", 23, [2] * 5 + [1] * 50, 8, per_op=2), 123)
    add(make_instance("d111", 19, [1], 1), 119)
    add(make_instance("dM1", 20, [2, 1], 1), 120)
    add(make_instance("dK1", 21, [1], 3), 121)
    add(make_instance("wide_p", 22, [3] * 4, 5, p_range=(1, 65535), log_p=True), 122, jobs=(100, 600))
    for seed in sorted(set(s for v in SEARCH_SEEDS.values() for s in v)):
        out.append(search_case(seed))
    return out


def instance_set(arrs):
    """A product InstanceSet of these instances with the host solver's reset-time fluid solution."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    s = fi.InstanceSet(len(arrs))
    for i, a in enumerate(arrs):
        s.set_raw(i, a.Jr, a.p, a.elig_n, a.elig_list, a.count, a.arrive, a.delivery, a.ddt)
    return s.solve_fluid()


def _search_one(seed):
    from tests import lp_reference as LR
    c = search_case(seed)
    hits = dict(pivots=0, magnitude=0, sign=0, small=0, bad=0)
    for _, Q, now in c.states:
        try:
            _, _, rec = LR.fluid_lp_reference(c.arr.Jr, c.arr.p, Q, now)
        except LR.LpFailure:
            continue
        for pv in rec:
            hits["pivots"] += 1
            hits["magnitude"] += pv["decided"] == "magnitude"
            hits["sign"] += pv["decided"] == "sign"
            hits["small"] += bool(pv["small"])
            hits["bad"] += bool(pv["bad"])
    return seed, hits


def search_ratio_classes(seeds, processes=16):
    """Pivots per ratio-test class over search_case(seed), and the seeds that reach each class."""
    import multiprocessing as mp
    total, where = {}, {}
    with mp.Pool(processes) as pool:
        for seed, hits in pool.imap_unordered(_search_one, seeds, chunksize=8):
            for key, n in hits.items():
                total[key] = total.get(key, 0) + int(n)
                if n and key != "pivots":
                    where.setdefault(key, []).append((int(n), seed))
    return total, {key: sorted(v, reverse=True)[:6] for key, v in where.items()}


if __name__ == "__main__":
    import sys
    bound = int(sys.argv[1]) if len(sys.argv) > 1 else SEARCH_BOUND
    total, where = search_ratio_classes(range(bound))
    print("seeds 0 ... %d:" % (bound - 1), total)
    print("(pivots of the class, seed), most first:", where)
