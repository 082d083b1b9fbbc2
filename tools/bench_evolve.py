"""Cost and result of the population search (fjsp_schedule_evolve: schedule.evolve, policy_search.genetic_search) beside the
decode and the single-trajectory search in the same process on the same arrays, with the protocol of
tools/bench_search_dyn.py: after a warm-up, --regions (at least 25) timed regions of as many calls as fill --window
seconds, between two device synchronisations on a host clock, the entries of a comparison taking turns region by region;
median [min, max].  The shops are that tool's: gen8801 (76 rows) and industrial/DDT0.5_M20_S1 (249 rows) of
tests/golden/schedule.npz, MO_DFJSP.

  a  per generation at 8 envs x 64 individuals (--generations per call) and at --envs (default 4096) x 64
     (--batch-generations per call), the call of no generations subtracted, on both shops; the population is
     seed_population's from the recorded schedule.  Beside it the call of twice the generations less the call itself.
     In the same turns: (a) one schedule.decode_dyn call with q_plans = 64 on that population, the floor a generation
     cannot beat -- it decodes what a generation decodes and recombines nothing --, and (b) a round of
     schedule.search_dyn with 64 neighbours from individual 0, its call of no rounds subtracted.  The ratios are a report.
  c  for the record: on gen8801 with 64 envs, the best makespan of genetic_search (64 individuals, --record-generations
     generations) against tabu local_search (64 neighbours, as many rounds) from the same start plans: an equal number of
     decodes.
One JSON line per measurement, also written to --out.

    python tools/bench_evolve.py [--envs 4096] [--generations 100] [--batch-generations 10] [--out profiles/evolve_bench.jsonl]
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
from tests import helpers as H  # noqa: E402
from tests import schedule_fixture as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--regions", type=int, default=25)
ap.add_argument("--window", type=float, default=0.3)
ap.add_argument("--generations", type=int, default=100)
ap.add_argument("--batch-generations", type=int, default=10)
ap.add_argument("--record-generations", type=int, default=2000)
ap.add_argument("--mut-rate", type=int, default=6554)
ap.add_argument("--tenure", type=int, default=8)
ap.add_argument("--parts", default="ac")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "evolve_bench.jsonl"))
args = ap.parse_args()
if args.regions < 25:
    ap.error("--regions must be at least 25")
if not torch.cuda.is_available():
    sys.exit("bench_evolve needs an MI355X: nothing here is measured on a CPU")
P = 64
TABU = sch.SEARCH_ACCEPT.index("tabu")
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


variant, eps = F.load()["mo_dfjsp"]
by_name = {ep["inst"].name: ep for ep in eps}
small, big = by_name["gen8801"], by_name["industrial/DDT0.5_M20_S1"]


def recorded(ep, n):
    """(batch of n envs on the episode's shop, its recorded schedule as every env's plan)."""
    b = EnvBatch(H.instance_set_from([ep["inst"]]), n, variant=variant, rng_seed=1)
    cap = b.decode_capacity()
    assert cap == len(ep["table"])
    parent = np.ascontiguousarray(ep["table"][:, [0, 2, 3]].astype(np.int32))
    return b, torch.from_numpy(parent)[None].expand(n, cap, 3).contiguous().cuda()


def unit(n):
    return torch.tensor([[1, 0, 0]], dtype=torch.int64).expand(n, 3).contiguous().cuda()


if "a" in args.parts:
    for ep in (small, big):
        for n, G in ((8, args.generations), (args.envs, args.batch_generations)):
            b, plan = recorded(ep, n)
            w = unit(n)
            pop = PS.seed_population(b, plan, P, shake=8, seed=1)
            res = sch.evolve(b, pop, G, w, args.mut_rate, 0)
            assert bool((res["status"] == 0).all()) and bool((b.decode_dyn(pop, None, P)["status"] == 0).all())
            gain = (res["history"][0] - res["history"][-1]).double().mean().item()
            del res
            (ev, ev0, ev2, dec, dyn, dyn0), calls = timed_in_turns([
                lambda: sch.evolve(b, pop, G, w, args.mut_rate, 0), lambda: sch.evolve(b, pop, 0, w, args.mut_rate, 0),
                lambda: sch.evolve(b, pop, 2 * G, w, args.mut_rate, 0),
                lambda: b.decode_dyn(pop, None, P),
                lambda: sch.search_dyn(b, plan, G, P, 0, TABU, args.tenure, 0), lambda: sch.search_dyn(b, plan, 0, P)])
            per_gen = [(t - float(np.median(ev0))) / G for t in ev]
            per_round = [(t - float(np.median(dyn0))) / G for t in dyn]
            # (a call of no generations also writes the start population out, which no other call does: the call of 2 G
            # generations less the call of G is the same figure without that copy)
            doubled = [(t - float(np.median(ev))) / G for t in ev2]
            emit(what="generation", instance=ep["inst"].name, envs=n, population=P, rows=b.decode_capacity(), generations=G, mut_rate=args.mut_rate,
                 lds_bytes=b.evolve_lds(), search_dyn_lds_bytes=b.search_dyn_lds(), calls_per_region=calls,
                 seconds_per_generation=spread(per_gen), seconds_of_no_generations=spread(ev0),
                 seconds_per_generation_by_doubling=spread(doubled), decode_dyn_seconds_per_call=spread(dec),
                 search_dyn_seconds_per_round=spread(per_round), search_dyn_seconds_of_no_rounds=spread(dyn0),
                 generation_over_decode_of_medians=float(np.median(per_gen) / np.median(dec)),
                 generation_over_search_round_of_medians=float(np.median(per_gen) / np.median(per_round)), mean_makespan_gain=gain)
            del pop, plan, b
            torch.cuda.empty_cache()

if "c" in args.parts:
    n, G = 64, args.record_generations
    b, plan = recorded(small, n)
    pop = PS.seed_population(b, plan, P, shake=8, seed=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ga = PS.genetic_search(b, pop, G, "makespan", mutation=args.mut_rate / 65536.0, seed=0)
    torch.cuda.synchronize()
    ga_seconds = time.perf_counter() - t0
    t0 = time.perf_counter()
    ls = PS.local_search(b, plan, G, P, "makespan", 0, "tabu", args.tenure)
    torch.cuda.synchronize()
    ls_seconds = time.perf_counter() - t0
    first = int(b.decode_dyn(plan)["objective"][0, 0, 0])
    emit(what="makespan_at_equal_decodes", instance=small["inst"].name, envs=n, population=P, generations=G, neighbours=P, rounds=G,
         start_makespan=first, genetic_search_seconds=ga_seconds, local_search_seconds=ls_seconds,
         genetic_search_makespan=dict(min=int(ga["objective"][:, 0].min()), mean=float(ga["objective"][:, 0].double().mean()), max=int(ga["objective"][:, 0].max())),
         tabu_local_search_makespan=dict(min=int(ls["objective"][:, 0].min()), mean=float(ls["objective"][:, 0].double().mean()), max=int(ls["objective"][:, 0].max())))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for kw in lines:
        f.write(json.dumps(kw) + "\n")
