"""The device instance generator (csrc/fjsp_generate.hip) at the size limits check_worst_case accepts: the case table.

Shared by tests/test_generator_limit_cases_host.py (CPU: the host generator against the Python restatement of the stream on
every case, the edge each case exists for, the fluid LPs) and tests/test_gpu_generator_limits.py (the device generator against
the host path on the same seeds, bit for bit).  Importable without a GPU.

A case is a dict:
    params     GenParams (one order, fixed M and DDT), GenOrders (SO_FJSSP with order arrivals) or GenDynamic (MO_DFJSP)
    seed       seed base: instance i is made of seed + i
    n_inst     instances (= environments), 4 to 8
    variants   the variants the GPU test runs the case as (batch.VARIANT_*: 0 SO_FJSSP, 4 MO_DFJSP, 5 SO_DFJSP)
    family     kernel family asked for (None: the library's choice, 1: the row kernels)
    steps      None: the whole episode is compared (at most about 350 operations); n: its first n steps and read()
    route      None, or the one LP route every instance must take: "lds", "host"
    reaches    predicate on the list of the case's instance arrays: the edge the case exists for
Unless a case says otherwise: processing times 1..20, one job per kind, DDT 1.0.

    kinds_256          R = K = 256 kinds of one stage: four trips of the kind loops, kind byte 255, four chunks of 64 types;
                       258 LP rows, more than the global simplex takes: every LP on the host
    kinds_255          R = K = 255 kinds of one job: the largest single_job batch, whose kernels index the jobs by the kind byte
                       (254 at most) -- kinds_256 is not single_job and its episode never reads that byte
    kinds_256_orders   SO_FJSSP, two orders of 256 kinds with 1..2 jobs each: the arrival reads every kind's count by its kind
                       byte, up to 255; the whole episode (at most 1024 operations)
    kinds_spread       R 65..256: K in (64, 128], (128, 192] and (192, 256] in one batch (seeds 9000.. give 163, 117, 201, 154)
    stages_255         one kind of 255 stages: stage byte 254, J = 255 in kB and jinfo
    two_by_128         two kinds of 128 stages: K = 256 with koff[1] = 128
    machines_32        M = 32, 4 kinds x 2 stages: eligible lists of 32 entries, machine bit 31, lists beyond first4; LDS route
    machines_32_p_max  M = 32, 8 x 8 types, every p = 65535, 11..12 jobs per kind, DDT 1.5: 2048 (type, machine) pairs, a
                       delivery time above 2^20, due dates rint(dl * J / c) in the millions; also as SO_DFJSP (class_fjsp: the
                       operations-per-machine ballot over 32 lanes)
    jobs_many          2 kinds x 1 stage with 2047..2048 jobs each: about 4096 jobs -- u16 counts, s_jbeg, the kA totals, the
                       per-job due-date loop; seeds 9004.. hold 4095, 4094, 4096 and 4095 jobs.  (plan_layout's LDS rule admits 4864 jobs at KP = 64: 4 x (1776 + 8 JP + pad)
                       bytes <= 160 KiB; 4096 is well inside, tests/test_gpu_generator_limits.py holds the pair 4864 | 4928)
    rows_15_kinds      the row kernels (family 1), M = 8: 15 kinds x 4 stages, K = 60 -- the head line with R = 15
    rows_64_types      ... and 8 kinds x 8 stages, K = 64
    orders_16          SO_FJSSP, S = 16 orders of 5 kinds (1..2 stages, 1..2 jobs), M = 2, p 500..4000 (the orders' gaps then
                       differ by more than the arrivals lie apart: the delivery sort moves entries): S x R = 80 > 64 job
                       counts, a 16-entry sort, 15 arrivals
    windows_max        MO_DFJSP, M = 32, 8 x 8 types, W_max = 2047 windows of 1..30 every 40000..50000, p 20000..60000 (so the
                       first windows fall inside the episode): a machine with more than 2000 windows, u16 window offsets
                       beyond 2^15.  (A record's window total is a sum of 32 draws of U{0..2047}: mean 32752, sigma about 3340.
                       Of the seed bases 9000, 9004, .. the first whose four instances hold a total above 40000 and a machine
                       above 2000 windows is 9064; 60000 lies eight sigma out and no seed reaches it.)
    redraw_deep        MO_DFJSP, M = 16, 2 kinds x 2 stages, redraws = 16: about every second shop leaves a machine idle; of
                       seeds 9004..9011 the instances are made of attempts REDRAW_ATTEMPTS (found with fjsp_gen_dynamic_seed)
    redraw_exhausted   MO_DFJSP, M = 32, one operation type, redraws = 16: a shop plays only if the type draws all 32 machines
                       (1 in 32): seed 9003, instance 1 of base 9002, fails all 17 attempts
"""
import types

import numpy as np

from deep_reinforcement_learning_for_fjsp_amd._capi import GenDynamic, GenOrders, GenParams, GenRanges
from tests.test_generate_dynamic_host import REDRAW_STREAM, machine, machine_data_py
from tests.test_generate_host import MASK, draw, randint, replay
from tests.test_generate_orders_host import orders_py
from tests.test_generate_ranges_host import draw_py, uniform
from tests.test_gpu_generate import tableau_fits                  # (importing a GPU test module runs none of its tests)
from tests.test_gpu_generate_orders import unsorted_delivery

SEED = 9000
VARIANT_SO_FJSSP, VARIANT_MO_DFJSP, VARIANT_SO_DFJSP = 0, 4, 5
INT_KEYS = ("Jr", "p", "elig_n", "elig_list", "count", "arrive", "delivery")
REDRAW_ATTEMPTS = [0, 5, 0, 0, 2, 0, 1, 2]       # of seeds 9004 .. 9011 under redraw_deep
EXHAUSTED_INSTANCE = 1                            # of seed base 9002 under redraw_exhausted: seed 9003


def gp(**kw):
    d = dict(M=0, p_min=1, p_max=20, N_min=1, N_max=1, S=1, DDT=1.0, t_si_min=100.0, t_si_max=200.0)
    d.update(kw)
    return GenParams(**d)


def go(M, S, DDT=1.0, **kw):
    return GenOrders(GenRanges(gp(S=0, DDT=0.0, **kw), M, M, DDT, DDT), S, S)


def gd(M, mc, redraws, S=1, DDT=1.0, **kw):
    return GenDynamic(go(M, S, DDT, **kw), mc, redraws)


# ---- the restatement of the whole generator, every draw by its position -------------------------------------------------------
def replay_orders(seed, g, M, DDT, S):
    """generate(seed, g with M, DDT, S) of fjsp_instance.cpp: the shop of `replay`, then -- following pos_count, pos_interval,
    order and sort_deliveries of fjsp_gen_stream.h -- the S x R job counts order-major behind the chain, the S - 1 intervals
    behind them, every order's arrival (the truncated running sum of the intervals, summed from order 0 again) and gap (summed
    left to right over the operation types), the delivery times sorted ascending and then truncated."""
    seed &= MASK
    one = GenParams.from_buffer_copy(g)
    one.M, one.DDT, one.S = M, DDT, 1
    r = replay(seed, one)
    R, K, n, p, el = r["R"], r["K"], r["elig_n"], r["p"], r["elig_list"]
    end = 1 + R + K + 2 * int(n.sum())           # R, J_r, per type (n, n shuffle draws), n processing times
    count = np.array([[randint(seed, end + s * R + q, g.N_min, g.N_max) for q in range(R)] for s in range(S)], np.int32)
    kind_of = np.repeat(np.arange(R), r["Jr"])
    time_rj = [float(sum(int(p[k, m]) for m in el[k, :n[k]])) / float(n[k]) for k in range(K)]
    arrive, dl = [], []
    for s in range(S):
        acc, t = 0.0, 0.0
        for k in range(K):
            acc = acc + time_rj[k] * float(count[s, kind_of[k]])
        for q in range(1, s + 1):
            t = t + uniform(seed, end + S * R + (q - 1), g.t_si_min, g.t_si_max)
        arrive.append(int(t))
        dl.append(float(int(t)) + acc * DDT / float(M * 2))
    for i in range(1, S):                        # sort_deliveries: an insertion sort
        v, j = dl[i], i - 1
        while j >= 0 and dl[j] > v:
            dl[j + 1] = dl[j]
            j -= 1
        dl[j + 1] = v
    r.update(S=S, count=count, arrive=np.array(arrive, np.int32), delivery=np.array([int(v) for v in dl], np.int32))
    return r


def idle_machine(r):
    return bool(np.any((np.asarray(r["p"]) > 0).sum(0) == 0))


def restate(params, seed):
    """Instance `seed` under `params` from the Python restatements alone: its arrays; for a GenDynamic also the attempt it is
    made of, that attempt's seed and the machine data -- or None where every attempt leaves a machine idle."""
    seed &= MASK
    if isinstance(params, GenParams):
        r = replay_orders(seed, params, params.M, params.DDT, 1)
        assert all(np.array_equal(r[k], v) for k, v in replay(seed, params).items())        # one order: `replay` itself
        return r
    if isinstance(params, GenOrders):
        (M, DDT), S = draw_py(params.r, seed), orders_py(params, seed)
        return replay_orders(seed, params.r.base, M, DDT, S)
    for attempt in range(params.redraws + 1):
        used = seed if attempt == 0 else draw(seed ^ REDRAW_STREAM, attempt - 1)
        r = restate(params.o, used)
        if not idle_machine(r):
            break
    else:
        return None
    r.update(attempt=attempt, used=used)
    shop = types.SimpleNamespace(M=r["M"], K=r["K"], p=r["p"])
    r["power"], r["idle_power"], r["bk_n"], r["bk"] = machine_data_py(shop, used, params.m)
    return r


# ---- the edges ------------------------------------------------------------------------------------------------------------------
def jobs(a):
    return int(np.asarray(a.count).sum())


def operations(a):
    return int((np.asarray(a.count).reshape(a.S, a.R) * np.asarray(a.Jr)[None, :]).sum())


def _kinds_spread(arrs):
    ks = [a.K for a in arrs]
    return all(a.R == a.K for a in arrs) and all(any(lo < k <= lo + 64 for k in ks) for lo in (64, 128, 192))


def _machines_32(arrs):
    return (all((a.M, a.K) == (32, 8) and tableau_fits(a) for a in arrs) and any(a.elig_n.max() == 32 for a in arrs) and
            any((a.p[:, 31] > 0).any() for a in arrs) and any(4 < n < 32 for a in arrs for n in a.elig_n))


def _p_max(arrs):
    return all((a.M, a.K, a.K * a.M) == (32, 64, 2048) and set(np.unique(a.p)) == {0, 65535} and a.delivery[0] > 2 ** 20 and
               not np.any((a.p > 0).sum(0) == 0) for a in arrs)


def _orders_16(arrs):
    return (all(a.S == 16 and a.S * a.R == 80 and len(np.unique(a.arrive)) == 16 for a in arrs) and
            any(np.any(np.diff(unsorted_delivery(a)) < -1.0) for a in arrs))


def _windows_max(arrs):
    return (all((a.M, a.K) == (32, 64) for a in arrs) and any(a.bk_n.max() > 2000 for a in arrs) and
            any(a.bk_n.sum() > 40000 for a in arrs) and all(len(a.bk) == a.bk_n.sum() and a.bk[:, 0].min() <= 50000 for a in arrs))


WINDOWS = machine(2047, gap_min=40000, gap_max=50000, len_min=1, len_max=30)
CASES = {
    "kinds_256": dict(params=gp(R_min=256, R_max=256, J_min=1, J_max=1, M=2), route="host",
                      reaches=lambda arrs: all((a.R, a.K) == (256, 256) for a in arrs)),
    "kinds_255": dict(params=gp(R_min=255, R_max=255, J_min=1, J_max=1, M=2),
                      reaches=lambda arrs: all((a.R, a.K, jobs(a)) == (255, 255, 255) for a in arrs)),
    "kinds_256_orders": dict(params=go(2, 2, R_min=256, R_max=256, J_min=1, J_max=1, N_min=1, N_max=2), steps=1024,
                             reaches=lambda arrs: all((a.R, a.S) == (256, 2) and a.arrive[1] > 0 and set(np.unique(a.count[1, 128:])) == {1, 2} for a in arrs)),
    "kinds_spread": dict(params=gp(R_min=65, R_max=256, J_min=1, J_max=1, M=3), reaches=_kinds_spread),
    "stages_255": dict(params=gp(R_min=1, R_max=1, J_min=255, J_max=255, M=2),
                       reaches=lambda arrs: all(a.Jr.tolist() == [255] for a in arrs)),
    "two_by_128": dict(params=gp(R_min=2, R_max=2, J_min=128, J_max=128, M=2),
                       reaches=lambda arrs: all(a.koff.tolist() == [0, 128, 256] for a in arrs)),
    "machines_32": dict(params=gp(R_min=4, R_max=4, J_min=2, J_max=2, M=32), route="lds", reaches=_machines_32),
    "machines_32_p_max": dict(params=gp(R_min=8, R_max=8, J_min=8, J_max=8, M=32, p_min=65535, p_max=65535, N_min=11, N_max=12, DDT=1.5),
                              variants=(VARIANT_SO_FJSSP, VARIANT_SO_DFJSP), steps=64, route="host", reaches=_p_max),
    "jobs_many": dict(params=gp(R_min=2, R_max=2, J_min=1, J_max=1, M=2, N_min=2047, N_max=2048), seed=9004, steps=64, route="lds",
                      reaches=lambda arrs: all(jobs(a) >= 4094 for a in arrs) and any(jobs(a) == 4096 for a in arrs) and any(jobs(a) < 4096 for a in arrs)),
    "rows_15_kinds": dict(params=gp(R_min=15, R_max=15, J_min=4, J_max=4, M=8), family=1,
                          reaches=lambda arrs: all((a.R, a.K, a.M) == (15, 60, 8) for a in arrs)),
    "rows_64_types": dict(params=gp(R_min=8, R_max=8, J_min=8, J_max=8, M=8), family=1,
                          reaches=lambda arrs: all((a.R, a.K, a.M) == (8, 64, 8) for a in arrs)),
    "orders_16": dict(params=go(2, 16, R_min=5, R_max=5, J_min=1, J_max=2, p_min=500, p_max=4000, N_min=1, N_max=2), reaches=_orders_16),
    "windows_max": dict(params=gd(32, WINDOWS, 8, R_min=8, R_max=8, J_min=8, J_max=8, p_min=20000, p_max=60000), seed=9064,
                        variants=(VARIANT_MO_DFJSP,), steps=64, reaches=_windows_max),
    "redraw_deep": dict(params=gd(16, machine(3), 16, R_min=2, R_max=2, J_min=2, J_max=2, p_min=5, p_max=30, N_min=1, N_max=2), seed=9004,
                        n_inst=8, variants=(VARIANT_MO_DFJSP,),
                        reaches=lambda arrs: all(a.M == 16 and not np.any((a.p > 0).sum(0) == 0) for a in arrs)),
    "redraw_exhausted": dict(params=gd(32, machine(3), 16, R_min=1, R_max=1, J_min=1, J_max=1, p_min=5, p_max=30, N_min=1, N_max=2), seed=9002,
                             variants=(), reaches=None),
}
for _name, _c in CASES.items():
    _c["name"] = _name
    for _k, _v in dict(seed=SEED, n_inst=4, variants=(VARIANT_SO_FJSSP,), family=None, steps=None, route=None).items():
        _c.setdefault(_k, _v)

GENERATED = [n for n in CASES if n != "redraw_exhausted"]             # the cases whose instances exist
GPU_RUNS = [(n, v) for n in GENERATED for v in CASES[n]["variants"]]


def host_set(case, solve=True):
    """The host path's instances of a case (InstanceSet.generate_range, solve_fluid)."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    s = fi.InstanceSet(case["n_inst"]).generate_range(case["seed"], case["params"])
    return s.solve_fluid() if solve else s
