"""Instances, plans and conditions of the limit tests of the schedule decoder and its critical paths (csrc/fjsp_decode.hip:
decode_kinds_kernel, schedule_decode_kernel, schedule_critical_kernel) at the sizes fjsp_env_create accepts.

Shared by tests/test_decode_limit_cases_host.py (CPU: the two numpy references decode every case and prove the condition the
case exists for; the create-time limit pairs) and tests/test_gpu_decode_limits.py (the kernels against the references, bit for
bit).  Importable without a GPU; nothing here touches a device.

A case is a batch: `arrs` instances, env i of N on instance i % n_inst, `cap` = the operations of the largest.  Per env it
holds D distinct plans (the hand-made or edge plan first), a list of combos (d, move) -- plan d decoded under `move`, None or
(kind, u, third) -- and `pick`[Q]: candidate q of every env is combo pick[q].  Q = the workgroup's candidates + 1, lane 0 and
lane MID carry combo 0.  critical() reads the undisturbed tables of the picked plans.  Every move critical writes on each
distinct table (the first max_moves of its list) is decoded again (reference(c)["emitted"]); in the long cases, where every
further candidate costs the reference a walk over the whole table, the first written move of each table.

    long-32767 | 32768 | 32769 | 65535   tables of that many rows, L = cap with no -1 row; plan 0 holds a job whose first and
              last rows are rows 0 and cap - 1; a MOVE_MACHINE and a MOVE_SWAP at rows cap - 1 and cap - 2 (the swap at cap - 1
              is refused).  Two kinds (128 stages x 255 jobs, 1 stage x the rest) or, at 65 535, one kind of 255 stages x 257
              jobs; processing times 1..clock_cap, the largest create's clock rule admits.
    far       the pair move whose w - u is 32 767 | 32 768 | 32 891 (far_plan): a machine arc a (row 0) -> b on the critical path
              with the last row of b's job in between that far from a; K = 256, M = 32, 33 146 rows.
    kinds     R = 255 (M = 31) and R = 256 (M = 32) kinds of one stage beside a K = 1, M = 1 filler: kind index 255, entry 256 of
              the kind table, machine M - 1 in plans, in MOVE_MACHINE targets and in emitted moves, machine 31 out of range on
              the M = 31 instance of a batch padded to 32.
    stages-so | stages-two   a kind of 254 and of 255 stages in a single-order batch, of 253 and 254 with two orders, each
              beside the filler.
    clock-one p = 65 535, eight kinds, one order that arrives at the latest time the clock rule admits: the hand-made plan's
              makespan is 2^31 - 1 with nothing to spare, total tardiness 8 x about 2^31 > 2^32, and in critical every end +
              tail = C lies above 2^30, on tables a decode wrote.
    clock-two the same with two orders, the second at the latest arrival: two jobs of every kind halve the rule, the makespan
              is 2^30 - 1.  shifted_clock_tables: its tables 2^30 later, an extra for critical alone (foreign tables).
    late      SO_DFJSP, R = 256 kinds of one job, p = 65 535 and the most negative delivery create admits: total tardiness
              about 2^39.
    orders-gap7 | burst, SO_FJSSP and SO_DFJSP   S = 64 orders (wave_limit_cases' instances): jobs released at their arrival
              and numbered across the orders, critical paths that end at an arrival.
    group-B-on | m | j   B = 256, 512, 1024, 2560, 5120 bytes of candidate state exactly (on), and one machine (m) or sixteen
              jobs (j) more: decode_group 256 | 128, 128 | 64, 64 | 64, 64 | 32, 32 | 0.
"""
import numpy as np

from tests import critical_reference as R
from tests import decode_reference as D
from tests import wave_limit_cases as WC

INT_MAX = 2 ** 31 - 1
MID = 37                          # the mid-wave lane that carries combo 0 beside lane 0
P_MAX = 65535
LONG_ROWS = (32767, 32768, 32769, 65535)
FAR_DW = (32767, 32768, 32891)
GROUP_BYTES = {256: (48, 4, 256), 512: (96, 8, 128), 1024: (192, 16, 64), 2560: (496, 20, 64), 5120: (1008, 20, 32)}   # B: (jobs, M, G)
GROUP_OVER = {256: 128, 512: 64, 1024: 64, 2560: 32, 5120: 0}
MOVE_NONE, MOVE_MACHINE, MOVE_SWAP, MOVE_PAIR = 0, 1, 2, 4
DKEYS = ("objective", "status", "table", "length")


# ---- instances --------------------------------------------------------------------------------------------------------------
def with_x(a):
    """The arguments of set_x: uniform over the eligible machines (no decode reads the fluid solution)."""
    el = np.asarray(a.p) > 0
    a.x = el / el.sum(1, keepdims=True).astype(np.float64)
    return a


def instance(name, Jr, p, count, arrive=(0,), delivery=None):
    """An instance with the processing times given: the arguments of InstanceSet.set_raw and set_x."""
    a = WC.Arr()
    a.name, a.Jr = name, np.asarray(Jr, np.int32)
    a.p = np.asarray(p, np.int32)
    a.R, (a.K, a.M) = len(a.Jr), a.p.shape
    assert a.K == int(a.Jr.sum())
    a.arrive = np.asarray(arrive, np.int32)
    a.S = len(a.arrive)
    a.count = np.asarray(count, np.int32).reshape(a.S, a.R)
    el = a.p > 0
    assert el.any(1).all() and el.any(0).all(), name
    a.elig_n = el.sum(1).astype(np.int32)
    a.elig_list = np.zeros((a.K, a.M), np.int32)
    for k in range(a.K):
        ms = np.flatnonzero(el[k])
        a.elig_list[k, :len(ms)] = ms
    a.delivery = np.asarray(a.arrive + 100 if delivery is None else delivery, np.int32)
    a.ddt = 1.0
    return with_x(a)


def ops_total(a):
    return WC.ops_total(a)


def jobs_kind_max(a):
    return int(a.count.sum(0).max())


def clock_rule(a):
    """check_instance's clock rule (csrc/fjsp_env.hip) on instance a: (clock_max + due_max, that x the most jobs of a kind);
    create admits the instance iff both are at most 2^31 - 1."""
    worst = int(a.arrive.max()) + ops_total(a) * int(a.p.max()) + int(np.abs(a.delivery.astype(np.int64)).max())
    return worst, worst * jobs_kind_max(a)


def clock_cap(ops, jobs_kind, rest=0):
    """The largest processing time the clock rule admits: (rest + ops x p) x max(jobs_kind, 1) <= 2^31 - 1, rest = the last
    arrival + the largest |delivery|."""
    return min(P_MAX, (INT_MAX // max(jobs_kind, 1) - rest) // ops)


def filler(name):
    return instance(name + "/k1m1", [1], [[3]], [2], delivery=[4])


def set_of(c):
    """The product InstanceSet of case c."""
    from tests import helpers as H
    return H.instance_set_from(c.arrs)


# ---- plans ------------------------------------------------------------------------------------------------------------------
def padded(rows, cap):
    out = np.full((cap, 3), -1, np.int32)
    out[:len(rows)] = rows
    return out


def ends_apart(a, rs, cap):
    """A random plan in which job (0, 0) holds row 0 and the last row."""
    rows = D.random_plan(a, rs)
    mine = np.flatnonzero((rows[:, 0] == 0) & (rows[:, 1] == 0))
    assert len(mine) >= 2
    keep = np.ones(len(rows), bool)
    keep[[mine[0], mine[-1]]] = False
    return padded(np.concatenate([rows[mine[:1]], rows[keep], rows[mine[-1:]]]), cap)


def begin_ordered(a, variant, plan, cap):
    one = D.decode_one(a, variant, plan, None, cap)
    assert one["status"] == 0
    return D.plan_from_table(R.begin_order(one["table"]), cap)


# ---- the far pair move ------------------------------------------------------------------------------------------------------
FAR_JOBS, FAR_STAGES = 131, 253
FAR_PA, FAR_PB, FAR_P0 = 420, 430, 5


def far_instance():
    """Kind 0: 253 stages x 131 jobs, p = 1 on machines 2..31, stage 0 also on machine 0 with p = 420.  Kind 1: 3 stages x 1
    job, stage 0 on machine 1 (p = 5), stages 1 and 2 on machine 0 (p = 430)."""
    p = np.zeros((256, 32), np.int32)
    p[:FAR_STAGES, 2:] = 1
    p[0, 0] = FAR_PA
    p[FAR_STAGES, 1] = FAR_P0
    p[FAR_STAGES + 1:, 0] = FAR_PB
    a = instance("far", [FAR_STAGES, 3], p, [FAR_JOBS, 1], delivery=[2000])
    assert a.p.max() <= clock_cap(ops_total(a), FAR_JOBS, 2000)
    return a


def far_plan(dw, cap):
    """a = stage 0 of job (0, 0) on machine 0 in row 0; the other 130 jobs of kind 0 job after job, job n on machine 2 +
    (n - 1) % 30 (done by 1265); stage 0 of kind 1 in row dw; stage 1 of a's job (machine 31, free at 1012); b and c = stages 1
    and 2 of kind 1 on machine 0 (b begins when a ends, at 420; c ends at 1280, last of all); the rest of a's job (ends at 1264).
    Returns (plan, v): b stands in row v, w = dw is the last row of b's job in (0, v) and stands in front of a's stage 1."""
    others = [(0, n, 2 + (n - 1) % 30) for n in range(1, FAR_JOBS) for _ in range(FAR_STAGES)]
    assert 1 <= dw <= len(others) + 1
    rows = [(0, 0, 0)] + others[:dw - 1] + [(1, 0, 1)] + others[dw - 1:] + [(0, 0, 31), (1, 0, 0), (1, 0, 0)] + [(0, 0, 31)] * (FAR_STAGES - 2)
    return padded(rows, cap), len(others) + 3


# ---- cases ------------------------------------------------------------------------------------------------------------------
class Case(object):
    def __init__(self, name, variant, arrs, group, plans, combos, max_moves=16, N=None, check_all=True):
        self.name, self.variant, self.arrs, self.group = name, variant, arrs, group
        self.n_inst, self.N = len(arrs), len(arrs) if N is None else N
        self.cap = max(ops_total(a) for a in arrs)
        self.plans, self.combos = plans, combos                # [N][D] plans int32[cap][3]; [N][C] (d, move)
        self.max_moves = max_moves
        self.check_all = check_all                             # False (long tables): only the first written move is decoded again
        self.Q = group + 1
        if group:
            assert len(plans) == len(combos) == self.N and len({len(x) for x in plans}) == len({len(x) for x in combos}) == 1
            C = len(combos[0])
            self.pick = np.arange(self.Q) % C
            self.pick[min(MID, self.Q - 1)] = 0

    def inst(self, i):
        return self.arrs[i % self.n_inst]

    def plan_array(self):
        """int32[N][Q][cap][3]: candidate q of env i decodes the plan of its combo."""
        return np.stack([np.stack([self.plans[i][self.combos[i][c][0]] for c in self.pick]) for i in range(self.N)])

    def move_array(self):
        """int32[N][Q][3]"""
        mv = lambda m: (0, 0, 0) if m is None else m
        return np.array([[mv(self.combos[i][c][1]) for c in self.pick] for i in range(self.N)], np.int64).astype(np.int32)


def state_bytes(jobs, M):
    """The decoder's state of one candidate (include/fjsp_amd.h): 5 bytes per job, jobs rounded up to 16, 4 per machine."""
    jw = (jobs + 15) // 16 * 16
    return (jw + jw // 4 + M) * 4


def group_of(nbytes):
    """decode_group: the largest of 256, 128, 64 within 64 KB, else 64 or 32 within 160 KB, else 0."""
    for G in (256, 128, 64):
        if G * nbytes <= 64 * 1024:
            return G
    return 64 if 64 * nbytes <= 160 * 1024 else (32 if 32 * nbytes <= 160 * 1024 else 0)


def batch_group(arrs):
    return group_of(state_bytes(max(int(a.count.sum()) for a in arrs), max(a.M for a in arrs)))


def _edge_moves(a, plan, cap):
    """MOVE_MACHINE at rows cap - 1 and cap - 2 (to another eligible machine where the operation has one), MOVE_SWAP at rows
    cap - 2 and cap - 1 (the latter refused: u + 1 is outside the plan)."""
    L = D.plan_length(plan)
    koff = np.concatenate(([0], np.cumsum(a.Jr)))
    out = []
    for u in (L - 1, L - 2):
        r, n, m = (int(x) for x in plan[u])
        stage = int(np.sum((plan[:u, 0] == r) & (plan[:u, 1] == n)))
        other = [int(x) for x in np.flatnonzero(a.p[koff[r] + stage] > 0) if x != m]
        out.append((MOVE_MACHINE, u, other[-1] if other else m))
    return out + [(MOVE_SWAP, L - 2, 0), (MOVE_SWAP, L - 1, 0)]


def _standard(name, variant, arrs, seed, N=None, max_moves=16, hand=None, extra_moves=None, check_all=True):
    """Per env: plan 0 = hand(i) if given, else a random plan with job (0, 0) at both ends where the instance has such a job;
    plan 1 random; plan 2 = plan 1 in begin order.  Combos: the three plans, then plans 0 and 1 under the edge moves."""
    N = len(arrs) if N is None else N
    rs = np.random.RandomState(seed)
    cap = max(ops_total(a) for a in arrs)
    plans, combos = [], []
    for i in range(N):
        a = arrs[i % len(arrs)]
        if hand is not None and hand(i) is not None:
            p0 = hand(i)
        elif int(a.Jr[0]) >= 2:
            p0 = ends_apart(a, rs, cap)
        else:
            p0 = D.random_plan(a, rs, cap)
        p1 = D.random_plan(a, rs, cap)
        plans.append([p0, p1, begin_ordered(a, variant, p1, cap)])
        cb = [(0, None), (1, None), (2, None)]
        if D.plan_length(p0) >= 2:
            mv0, mv1 = _edge_moves(a, p0, cap), _edge_moves(a, p1, cap)
            cb += [(0, mv0[0]), (0, mv0[2]), (1, mv1[1]), (1, mv1[3])]
        cb += [] if extra_moves is None else extra_moves(i, a, plans[-1])
        combos.append(cb)
    width = max(len(cb) for cb in combos)
    combos = [cb + [(0, None)] * (width - len(cb)) for cb in combos]
    return Case(name, variant, arrs, batch_group(arrs), plans, combos, max_moves, N, check_all)


def _long(rows):
    seed = 41000 + rows
    rs = np.random.RandomState(seed)
    if rows == 65535:
        Jr, count = [255], [257]
    else:
        Jr, count = [128, 1], [255, rows - 128 * 255]
    cap_p = clock_cap(rows, max(count), 100)
    a = instance("long-%d" % rows, Jr, rs.randint(1, cap_p + 1, (sum(Jr), 2)), count)
    a.p[0, 0] = cap_p
    assert ops_total(a) == rows
    # (each further candidate costs the reference a walk over the whole table: one emitted move per table is decoded again)
    return _standard("long-%d" % rows, 0, [a], seed, max_moves=4, check_all=False)


def _far():
    a = far_instance()
    cap = ops_total(a)
    hand = [far_plan(dw, cap) for dw in FAR_DW]
    plans = [pl for pl, _ in hand]
    plans.append(begin_ordered(a, 0, plans[1], cap))
    v = hand[0][1]
    wrapped = lambda dw: int(np.array([v | (dw << 16)], np.int64).astype(np.int32)[0])       # what an int32 makes of dv | dw << 16
    combos = [(0, None), (1, None), (2, None), (3, None), (0, (MOVE_PAIR, 0, v | (FAR_DW[0] << 16))),
              (1, (MOVE_PAIR, 0, wrapped(FAR_DW[1]))), (2, (MOVE_PAIR, 0, wrapped(FAR_DW[2])))]
    return Case("far", 0, [a], batch_group([a]), [plans], [combos], max_moves=4)


def _kinds():
    arrs = [with_x(WC.make("kinds/255", 42001, [1] * 255, 31, [1] * 255, full_ops=range(0, 255, 3))),
            with_x(WC.make("kinds/256", 42002, [1] * 256, 32, [1] * 256, full_ops=range(0, 256, 3))), filler("kinds")]

    def extra(i, a, plans):
        """Row 0 and the last row of plan 1 to machine 31 (the top machine at M = 32, out of range at M = 31 and M = 1), a row
        of kind R - 1 to machine M - 1."""
        L = D.plan_length(plans[1])
        top = int(np.flatnonzero(plans[1][:L, 0] == a.R - 1)[0])
        return [(1, (MOVE_MACHINE, 0, 31)), (1, (MOVE_MACHINE, L - 1, 31)), (1, (MOVE_MACHINE, top, a.M - 1))]
    return _standard("kinds", 0, arrs, 42000, max_moves=48, extra_moves=extra)


def _stages(shape):
    Ls = WC.STAGES_SINGLE if shape == "so" else WC.STAGES_ARRIVALS
    arrs = [with_x(WC._stages_instance("stages-%s/%d" % (shape, L), 43000 + L, L, shape)) for L in Ls] + [filler("stages-" + shape)]
    return _standard("stages-" + shape, 0, arrs, 43000 + len(shape), max_moves=24)


CLOCK_KINDS = 8


CLOCK_MAX = {"one": INT_MAX, "two": INT_MAX // 2}     # two orders hold two jobs of every kind (set_raw): the clock rule halves


def _clock(orders):
    """p = 65 535 everywhere, kinds 1, 3, 5, 7 on machine 0 alone, deliveries 0, so every due date is 0.
    "one": a single order that arrives at 2^31 - 1 - 8 x 65535 (create puts no rule on the arrival of a single order, and the
    decoder releases every job at it).  "two": two orders of one job per kind, at 0 and at 2^30 - 1 - 16 x 65535.
    The hand-made plan runs a job of the last order first and everything on machine 0: the makespan is CLOCK_MAX, the worst
    case of the clock rule itself; with one order that is the last int32."""
    Rk = CLOCK_KINDS
    p = np.full((Rk, 2), P_MAX, np.int32)
    p[1::2, 1] = 0
    S = 1 if orders == "one" else 2
    late = CLOCK_MAX[orders] - S * Rk * P_MAX
    a = instance("clock-" + orders, [1] * Rk, p, np.ones((S, Rk)), arrive=[0, late][2 - S:], delivery=[0] * S)
    cap = ops_total(a)
    hand = padded([(0, S - 1, 0)] + [(r, n, 0) for r in range(Rk) for n in range(S) if (r, n) != (0, S - 1)], cap)
    return _standard("clock-" + orders, 0, [a, filler("clock")], 44000 + S, hand=lambda i: hand if i == 0 else None)


def shifted_clock_tables():
    """Tables for critical alone, as an extra beside clock-one: the two-order case's three tables with every time 2^30 later (a
    foreign table: idle time in front), so that ends, tails' sums and C reach 2^31 - 1.  (arrays a, int32[3][cap][6])"""
    c = case("clock-two")
    tabs = np.stack([one["table"] for one in reference(c)["plain"][0]]).astype(np.int64)
    tabs[..., 4:][tabs[..., 4:] >= 0] += 2 ** 30
    assert tabs.max() == INT_MAX
    return c.arrs[0], tabs.astype(np.int32)


def _late():
    a = WC.make("late", 45001, [1] * 256, 4, [1] * 256, p_range=(P_MAX, P_MAX))
    a.delivery = np.array([WC.late_delivery(256, P_MAX)], np.int32)
    return _standard("late", 5, [with_x(a)], 45000, max_moves=24)


def _orders(pattern, variant):
    a = with_x(WC.case(("orders", pattern, 0)).arrs[0])
    return _standard("orders-%s-v%d" % (pattern, variant), variant, [a, filler("orders")], 46000 + variant + len(pattern), max_moves=24)


def _group(nbytes, side):
    jobs, M, G = GROUP_BYTES[nbytes]
    jobs, M = jobs + (side == "j"), M + (side == "m")
    rs = np.random.RandomState(47000 + nbytes)
    p = rs.randint(1, 21, (2, M))
    a = instance("group-%d-%s" % (nbytes, side), [1, 1], p, [jobs - jobs // 3, jobs // 3])
    want = G if side == "on" else GROUP_OVER[nbytes]
    assert batch_group([a]) == want and (state_bytes(jobs, M) == nbytes) == (side == "on"), a.name
    if want == 0:
        return Case(a.name, 0, [a], 0, None, None)
    return _standard(a.name, 0, [a], 47000 + nbytes + len(side), max_moves=8)


BUILDERS = {}
for _rows in LONG_ROWS:
    BUILDERS["long-%d" % _rows] = (_long, (_rows,))
BUILDERS["far"] = (_far, ())
BUILDERS["kinds"] = (_kinds, ())
BUILDERS["stages-so"] = (_stages, ("so",))
BUILDERS["stages-two"] = (_stages, ("two",))
BUILDERS["clock-one"] = (_clock, ("one",))
BUILDERS["clock-two"] = (_clock, ("two",))
BUILDERS["late"] = (_late, ())
for _pat in ("gap7", "burst"):
    for _v in (0, 5):
        BUILDERS["orders-%s-v%d" % (_pat, _v)] = (_orders, (_pat, _v))
for _b in GROUP_BYTES:
    for _side in ("on", "m", "j"):
        BUILDERS["group-%d-%s" % (_b, _side)] = (_group, (_b, _side))
NAMES = list(BUILDERS)
_CASES, _REFS = {}, {}

# ---- generated handles: the parameter sets and seeds of tests/test_gpu_decode_limits.py ----------------------------------
GEN_INST, GEN_ENVS, GEN_CANDIDATES = 5, 7, 4
GEN_SEEDS = (9300, 9400, 9500)                    # create, regenerate, masked regenerate
PLAYABLE = (9027, 9075)                           # seeds whose redraw_exhausted shop (one type, 32 machines) leaves no machine idle


def gen_params():
    """{"single": GenParams, "orders": GenOrders with three orders}; built on call, so that importing this module loads no
    generator test module."""
    from tests import generator_limit_cases as LC
    return {"single": LC.gp(R_min=3, R_max=5, J_min=2, J_max=4, M=4, N_min=1, N_max=3),
            "orders": LC.go(3, 3, R_min=2, R_max=4, J_min=1, J_max=3, N_min=1, N_max=2, p_min=5, p_max=40, t_si_min=20.0, t_si_max=60.0)}


def case(name):
    if name not in _CASES:
        fn, args = BUILDERS[name]
        _CASES[name] = fn(*args)
    return _CASES[name]


# ---- the references' answers, once per case -------------------------------------------------------------------------------
def reference(c):
    """dict(decode={DKEYS: [N][Q]..}, tables=int32[N][Q][cap][6] (what critical reads), critical={R.KEYS: [N][Q]..},
    per_plan=[N][D] critical_one dicts, plain=[N][D] decode_one dicts, emitted=dict(d=[N][E], moves=int32[N][E][3],
    decode={DKEYS: [N][E]..}))."""
    if c.name in _REFS:
        return _REFS[c.name]
    cap, N = c.cap, c.N
    plain, per_plan, by_combo = [], [], []
    for i in range(N):
        a = c.inst(i)
        plain.append([D.decode_one(a, c.variant, pl, None, cap) for pl in c.plans[i]])
        per_plan.append([R.critical_one(a, one["table"], c.max_moves, cap) for one in plain[i]])
        by_combo.append([plain[i][d] if mv is None else R.decode_moved(a, c.variant, c.plans[i][d], mv, cap) for d, mv in c.combos[i]])
    decode = {key: np.array([[by_combo[i][k][key] for k in c.pick] for i in range(N)]) for key in DKEYS}
    d_of = [[c.combos[i][k][0] for k in c.pick] for i in range(N)]
    tables = np.stack([np.stack([plain[i][d]["table"] for d in d_of[i]]) for i in range(N)])
    critical = {key: np.array([[per_plan[i][d][key] for d in d_of[i]] for i in range(N)], np.uint8 if key == "flags" else np.int32)
                for key in R.KEYS}
    ds, mvs, ones = [], [], []
    for i in range(N):
        a = c.inst(i)
        row_d, row_m = [], []
        for d, cr in enumerate(per_plan[i]):
            written = min(int(cr["n_moves"]), c.max_moves)
            idx = range(written) if c.check_all else range(min(written, 1))
            some = [tuple(int(x) for x in cr["moves"][j]) for j in idx]
            some += [(0, 0, 0)] * ((c.max_moves if c.check_all else 1) - len(some))        # (MOVE_NONE where fewer were written)
            row_d += [d] * len(some)
            row_m += some
        ds.append(row_d)
        mvs.append(row_m)
        ones.append([R.decode_moved(a, c.variant, c.plans[i][d], mv, cap) for d, mv in zip(row_d, row_m)])
    emitted = dict(d=np.array(ds), moves=np.array(mvs, np.int32).reshape(N, -1, 3),
                   decode={key: np.array([[one[key] for one in per] for per in ones]) for key in DKEYS})
    _REFS[c.name] = dict(decode=decode, tables=tables, critical=critical, per_plan=per_plan, plain=plain, emitted=emitted)
    return _REFS[c.name]


# ---- the condition each case exists for, on the references' answers -------------------------------------------------------
def condition(c):
    """(holds, what was measured), on reference(c)."""
    ref = reference(c) if c.group else None
    plain, crit = (ref["plain"], ref["per_plan"]) if c.group else ([], [])
    ok0 = all(one["status"] == 0 and one["length"] == ops_total(c.inst(i)) for i, per in enumerate(plain) for one in per)
    fam = c.name.split("-")[0]
    if fam == "long":
        rows, a, pl = int(c.name.split("-")[1]), c.arrs[0], c.plans[0]
        st = ref["decode"]["status"][0]
        mine = np.flatnonzero((pl[0][:, 0] == 0) & (pl[0][:, 1] == 0))
        moved = [mv for _, mv in c.combos[0] if mv is not None]
        ok = (ok0 and c.cap == rows and all(D.plan_length(x) == rows and not (x == -1).all(1).any() for x in pl) and
              mine[0] == 0 and mine[-1] == rows - 1 and (rows < 65535 or mine[-1] - mine[0] > 32768) and
              sorted((k, u) for k, u, _ in moved) == [(1, rows - 2), (1, rows - 1), (2, rows - 2), (2, rows - 1)] and
              sorted(set(st.tolist())) == [0, 4] and (st == 4).sum() == (c.pick == 6).sum() and
              all(clock_rule(a)[1] <= INT_MAX for a in c.arrs) and int(a.p.max()) == clock_cap(rows, jobs_kind_max(a), 100))
        return ok, "rows %d, job (0, 0) in rows %d..%d, p up to %d, status %s" % (rows, mine[0], mine[-1], a.p.max(), sorted(set(st.tolist())))
    if fam == "far":
        what, ok = [], ok0
        for d, dw in enumerate(FAR_DW):
            cr, tab = crit[0][d], plain[0][d]["table"]
            v = int(np.flatnonzero((c.plans[0][d][:, 0] == 1))[1])
            path = cr["path"][:cr["path_len"]].tolist()
            between = c.plans[0][d][1:v]
            w = int(np.flatnonzero(between[:, 0] == 1)[-1]) + 1
            first = int(np.flatnonzero((between[:, 0] == 0) & (between[:, 1] == 0))[0]) + 1
            pairs = [tuple(m) for m in cr["moves"][:min(cr["n_moves"], c.max_moves)].tolist() if m[0] == MOVE_PAIR]
            emitted = dw <= 32767
            ok = (ok and path == [v + 1, v, 0] and cr["flags"][0] & R.MACHINE_ARC and not cr["flags"][v] & R.MACHINE_ARC and
                  w == dw and w < first and tab[v, 4] == tab[0, 5] == FAR_PA and cr["makespan"] == tab[v + 1, 5] and
                  cr["skipped"] == (0 if emitted else 1) and pairs == ([(MOVE_PAIR, 0, v | (dw << 16))] if emitted else []))
            what.append("w - u = %d: %d pair moves, %d skipped" % (w, len(pairs), cr["skipped"]))
        st = [by for by in ref["decode"]["status"][0][:7].tolist()]
        ok = ok and st == [0, 0, 0, 0, 0, 4, 4] and crit[0][3]["skipped"] == 0 and clock_rule(c.arrs[0])[1] <= INT_MAX
        return ok, "; ".join(what) + "; status of the combos %s" % st
    if fam == "kinds":
        ok, what = ok0, []
        for i, a in enumerate(c.arrs[:2]):
            tabs = [one["table"] for one in plain[i]]
            moves = np.concatenate([cr["moves"][:min(cr["n_moves"], c.max_moves)] for cr in crit[i]])
            st = ref["decode"]["status"][i]
            top_r = all((t[:, 0] == a.R - 1).any() for t in tabs)
            top_m = any((t[:, 3] == a.M - 1).any() for t in tabs)
            top_mv = bool(((moves[:, 0] == MOVE_MACHINE) & (moves[:, 2] == a.M - 1)).any())
            ok = ok and top_r and top_m and top_mv and (a.R, a.M) == ((255, 31), (256, 32))[i]
            what.append("R %d M %d: kind %s machine %s in tables, machine in moves %s, status %s" % (a.R, a.M, top_r, top_m, top_mv, sorted(set(st.tolist()))))
        # a move to machine 31 is status 3 on the M = 31 instance and on the M = 1 filler; nothing is asked of the M = 32 one
        ok = ok and 3 in ref["decode"]["status"][0].tolist() and 3 in ref["decode"]["status"][2].tolist()
        return ok, "; ".join(what)
    if fam == "stages":
        Ls = WC.STAGES_SINGLE if c.name == "stages-so" else WC.STAGES_ARRIVALS
        ok = ok0 and [int(a.Jr[0]) for a in c.arrs[:2]] == list(Ls) and c.arrs[0].S == (1 if c.name == "stages-so" else 2)
        for i, L in enumerate(Ls):
            ok = ok and all((one["table"][:, 1] == L - 1).any() for one in plain[i])
            if c.arrs[i].S == 2:
                t = plain[i][1]["table"]
                ok = ok and t[(t[:, 2] == 1) & (t[:, 1] == 0), 4].min() >= 40
        return ok, "stages %s" % (Ls,)
    if fam == "clock":
        a, one, cr = c.arrs[0], plain[0][0], crit[0][0]
        C, tard = (int(x) for x in one["objective"])
        L = ops_total(a)
        on = cr["flags"][:L] & R.CRITICAL != 0
        top = CLOCK_MAX[c.name.split("-")[1]]
        ends = one["table"][:L, 5].astype(np.int64)
        ok = (ok0 and C == top and tard > 2 ** 32 and clock_rule(a) == (top, top * a.S) and INT_MAX - 1 <= top * a.S <= INT_MAX and
              bool(np.all(ends[on] + cr["tail"][:L][on] == C)) and int(on.sum()) == L and
              cr["makespan"] == C and cr["path_len"] == L and one["table"][int(cr["path"][L - 1]), 4] == a.arrive[-1] > 0)
        if a.S == 1:                                             # the last int32, from a decode: every end + tail above 2^30
            ok = ok and C == INT_MAX and int(ends.min()) > 2 ** 30 and all(int(x["makespan"]) > 2 ** 30 for x in crit[0])
        return ok, "%d order(s): makespan %d = %d - %d, tardiness %d" % (a.S, C, top, top - C, tard)
    if fam == "late":
        tard = [int(one["objective"][1]) for one in plain[0]]
        a = c.arrs[0]
        return ok0 and min(tard) > 2 ** 38 and clock_rule(a)[0] == INT_MAX and int(a.p.max()) == P_MAX, "tardiness %s" % tard
    if fam == "orders":
        a = c.arrs[0]
        ends = 0
        for one, cr in zip(plain[0], crit[0]):
            t = one["table"]
            last = int(cr["path"][cr["path_len"] - 1])
            ends += int(t[last, 4] > 0 and t[last, 4] in a.arrive.tolist())
            order = t[:ops_total(a), 2]                          # one job per kind and order: job n arrives with order n
            first = t[:ops_total(a), 1] == 0
            if not np.all(t[:ops_total(a), 4][first] >= a.arrive[order[first]]):
                return False, "a job begins before its order arrives"
        late = lambda t: (t[:ops_total(a), 4] == a.arrive[t[:ops_total(a), 2]]) & (a.arrive[t[:ops_total(a), 2]] > 0)
        released = [int(late(one["table"]).sum()) for one in plain[0]]
        return ok0 and a.S == 64 and ends >= 1 and min(released) >= 1, "%d paths end at an arrival, %s rows begin at their late order's arrival" % (ends, released)
    if fam == "group":
        nbytes, side = int(c.name.split("-")[1]), c.name.split("-")[2]
        a = c.arrs[0]
        got = state_bytes(int(a.count.sum()), a.M)
        step = {"on": 0, "m": 4, "j": 80}[side]
        ok = got == nbytes + step and c.group == (GROUP_BYTES[nbytes][2] if side == "on" else GROUP_OVER[nbytes])
        lds = got * c.group
        ok = ok and (side != "on" or nbytes < 2560 or lds == 160 * 1024) and (c.group == 0 or ok0)
        return ok, "%d bytes, group %d, %d bytes of LDS" % (got, c.group, lds)
    raise KeyError(c.name)
