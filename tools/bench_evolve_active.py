"""Cost and result of the population search under the active decoder (fjsp_schedule_evolve_active: schedule.evolve_active,
policy_search.genetic_search(decoder="active")) beside fjsp_schedule_evolve, the parent's entry and the yardstick, in the
same process on the same populations, with the protocol of tools/bench_evolve.py: after a warm-up, --regions (at least 25)
timed regions of as many calls as fill --window seconds, between two device synchronisations on a host clock, the entries
taking turns region by region; median [min, max].  The shops are tools/bench_decode_active.py's: gen8801 (76 rows) and
industrial/DDT0.5_M20_S1 (249 rows) of tests/golden/schedule.npz, created as SO_DFJSP.

  a  per generation at 8 envs x 64 individuals (--generations per call) and at --envs (default 4096) x 64
     (--batch-generations per call), the call of no generations subtracted, of both entries, on both shops and on two kinds
     of start population: "random" plans (decode_reference.random_plan, --pool of them tiled over the individuals: many
     insertions) and "ordered" ones (policy_search.left_shift of those: none in generation 0).  In the same turns one
     decode_active and one decode call with q_plans = 64 on the start population: what the insertion costs a bare decode
     there, to set the added cost of a generation against.  The ratios are a report.
  c  for the record: gen8801 with 64 envs from the recorded schedule, 64 individuals from seed_population (8 shakes),
     mutation 0.1, seed 0: genetic_search as it is for --record-generations generations; the same generations in --chunks
     chunks (seeds 0 ..) with left_shift between; genetic_search(decoder="active") for as many generations; and for as many
     generations as fit the wall time of the first.  Each followed by tabu local_search (--rounds rounds, 64 neighbours).
One JSON line per measurement, also written to --out.

    python tools/bench_evolve_active.py [--envs 4096] [--out profiles/evolve_active_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd import schedule as sch  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch  # noqa: E402
from tests import decode_reference as D  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import schedule_fixture as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--regions", type=int, default=25)
ap.add_argument("--window", type=float, default=0.3)
ap.add_argument("--pool", type=int, default=256)
ap.add_argument("--generations", type=int, default=100)
ap.add_argument("--batch-generations", type=int, default=10)
ap.add_argument("--mut-rate", type=int, default=6554)
ap.add_argument("--record-generations", type=int, default=2000)
ap.add_argument("--chunks", type=int, default=20)
ap.add_argument("--rounds", type=int, default=500)
ap.add_argument("--tenure", type=int, default=8)
ap.add_argument("--parts", default="ac")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "evolve_active_bench.jsonl"))
args = ap.parse_args()
if args.regions < 25:
    ap.error("--regions must be at least 25")
if not torch.cuda.is_available():
    sys.exit("bench_evolve_active needs an MI355X: nothing here is measured on a CPU")
P = 64
VARIANT = sch.VARIANT_SO_DFJSP
lines = []


def emit(**kw):
    kw.update(gpu=torch.cuda.get_device_name(0))
    print(json.dumps(kw), flush=True)
    lines.append(kw)


def spread(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


def timed_in_turns(fns):
    """Seconds per call of every fn: warm-up, then --regions regions of about --window seconds each, the fns taking turns."""
    calls = []
    for fn in fns:
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        calls.append(max(1, int(args.window / max(time.perf_counter() - t0, 1e-6))))
    ts = [[] for _ in fns]
    for _ in range(args.regions):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls[i]):
                fn()
            torch.cuda.synchronize()
            ts[i].append((time.perf_counter() - t0) / calls[i])
    return ts, calls


_, eps = F.load()["mo_dfjsp"]
by_name = {ep["inst"].name: ep for ep in eps}
small, big = by_name["gen8801"], by_name["industrial/DDT0.5_M20_S1"]

if "a" in args.parts:
    for ep in (small, big):
        a = ep["inst"]
        rs = np.random.RandomState(len(ep["table"]))
        pool = torch.from_numpy(np.stack([D.random_plan(a, rs, len(ep["table"])) for _ in range(args.pool)])).cuda()
        for n, G in ((8, args.generations), (args.envs, args.batch_generations)):
            b = EnvBatch(H.instance_set_from([a]), n, variant=VARIANT, rng_seed=1)
            cap = b.decode_capacity()
            assert cap == len(ep["table"])
            g = torch.arange(n * P, device="cuda")
            random = pool[((g * 7 + g // P) % args.pool).reshape(n, P)].contiguous()
            ordered = PS.left_shift(b, random)["plan"]
            w = torch.tensor([[1, 0]], dtype=torch.int64).expand(n, 2).contiguous().cuda()
            for kind, pop in (("random", random), ("ordered", ordered)):
                act = sch.evolve_active(b, pop, G, w, args.mut_rate, 0)
                semi = sch.evolve(b, pop, G, w, args.mut_rate, 0)
                assert bool((act["status"] == 0).all()) and bool((semi["status"] == 0).all())
                assert bool((act["history"][0] <= semi["history"][0]).all())
                assert kind == "random" or torch.equal(act["history"][0], semi["history"][0])
                facts = dict(inserted_rows_mean_last_generation=float(act["inserted"].double().mean()),
                             makespan_mean=dict(active_start=float(act["history"][0].double().mean()), active_end=float(act["history"][-1].double().mean()),
                                                semi_active_start=float(semi["history"][0].double().mean()), semi_active_end=float(semi["history"][-1].double().mean())))
                del act, semi
                (ea, ea0, es, es0, da, ds), calls = timed_in_turns([
                    lambda: sch.evolve_active(b, pop, G, w, args.mut_rate, 0), lambda: sch.evolve_active(b, pop, 0, w, args.mut_rate, 0),
                    lambda: sch.evolve(b, pop, G, w, args.mut_rate, 0), lambda: sch.evolve(b, pop, 0, w, args.mut_rate, 0),
                    lambda: b.decode_active(pop, None, P), lambda: b.decode(pop, None, P)])
                per_active = [(t - float(np.median(ea0))) / G for t in ea]
                per_semi = [(t - float(np.median(es0))) / G for t in es]
                emit(what="generation_active_against_semi_active", instance=a.name, envs=n, population=P, rows=cap, machines=int(a.M), plans=kind,
                     generations=G, mut_rate=args.mut_rate, lds_bytes=b.evolve_lds(), resident_envs=b.evolve_active_resident(),
                     decode_active_resident=b.decode_active_resident(), calls_per_region=calls, regions=args.regions,
                     evolve_active_seconds_per_generation=spread(per_active), evolve_seconds_per_generation=spread(per_semi),
                     evolve_active_seconds_of_no_generations=spread(ea0), evolve_seconds_of_no_generations=spread(es0),
                     decode_active_seconds_per_call=spread(da), decode_seconds_per_call=spread(ds),
                     generation_active_over_semi_active_of_medians=float(np.median(per_active) / np.median(per_semi)),
                     decode_active_over_decode_of_medians=float(np.median(da) / np.median(ds)),
                     added_seconds_per_generation_of_medians=float(np.median(per_active) - np.median(per_semi)),
                     added_seconds_per_decode_call_of_medians=float(np.median(da) - np.median(ds)), **facts)
            del random, ordered, b
            torch.cuda.empty_cache()

if "c" in args.parts:
    n, G = 64, args.record_generations
    a = small["inst"]
    b = EnvBatch(H.instance_set_from([a]), n, variant=VARIANT, rng_seed=1)
    cap = b.decode_capacity()
    parent = np.ascontiguousarray(small["table"][:, [0, 2, 3]].astype(np.int32))
    plan = torch.from_numpy(parent)[None].expand(n, cap, 3).contiguous().cuda()
    pop = PS.seed_population(b, plan, P, shake=8, seed=1)
    stat = lambda x: dict(min=int(x.min()), mean=float(x.double().mean()), max=int(x.max()))
    tabu = lambda start: stat(PS.local_search(b, start, args.rounds, P, "makespan", 0, "tabu", args.tenure)["objective"][:, 0])
    start = int(b.decode(plan)["objective"][0, 0, 0])

    def clocked(fn):
        fn()                                                            # (the first call of an entry allocates)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    ga, plain_seconds = clocked(lambda: PS.genetic_search(b, pop, G, "makespan", mutation=0.1, seed=0))
    per = G // args.chunks

    def chunked():
        cur = pop
        for c in range(args.chunks):
            step = PS.genetic_search(b, cur, per, "makespan", mutation=0.1, seed=c)
            ls = PS.left_shift(b, step["population"])
            cur = ls["plan"]
        return cur, ls

    (cur, ls), chunk_seconds = clocked(chunked)
    best = ls["objective"][..., 0].argmin(1)
    every = torch.arange(n, device="cuda")
    act, active_seconds = clocked(lambda: PS.genetic_search(b, pop, G, "makespan", mutation=0.1, seed=0, decoder="active"))
    G_eq = max(1, int(G * plain_seconds / active_seconds))
    eq, eq_seconds = clocked(lambda: PS.genetic_search(b, pop, G_eq, "makespan", mutation=0.1, seed=0, decoder="active"))
    emit(what="genetic_search_under_either_decoder", instance=a.name, envs=n, population=P, generations=G, chunks=args.chunks,
         tabu_rounds=args.rounds, neighbours=P, start_makespan=start,
         semi_active=dict(makespan=stat(ga["objective"][:, 0]), then_tabu=tabu(ga["plan"]), seconds=plain_seconds),
         left_shift_between_chunks=dict(makespan=stat(ls["objective"][every, best, 0]), then_tabu=tabu(cur[every, best].contiguous()), seconds=chunk_seconds),
         active=dict(makespan=stat(act["objective"][:, 0]), then_tabu=tabu(act["active_plan"]), seconds=active_seconds,
                     inserted_rows_mean_last_generation=float(act["inserted"].double().mean())),
         active_at_equal_wall_time=dict(generations=G_eq, makespan=stat(eq["objective"][:, 0]), then_tabu=tabu(eq["active_plan"]), seconds=eq_seconds,
                                        inserted_rows_mean_last_generation=float(eq["inserted"].double().mean())))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for kw in lines:
        f.write(json.dumps(kw) + "\n")
