"""Cost and result of policy_search.local_search (fjsp_schedule_search: the whole search in one launch) beside
policy_search.improve (a few dozen torch launches per round), with the protocol of tools/bench_decode.py: after a warm-up,
--regions (at least 25) timed regions of as many calls as fill --window seconds, between two device synchronisations on a
host clock; median [min, max].

  a  per round against improve: the 8 rule schedules of Mk10 and of Mk01, --rounds x 64 (default 400), every neighbourhood,
     sideways moves accepted, both in this process.  "fused_faster": the slowest local_search region is below the fastest
     improve region.
  b  per round at batch scale: --envs (default 4096) x 64 on the 10x5 bench instances and on the largest multijob instance
     (the shops of tools/bench_decode.py, whose decode of the same candidates is the line to compare with), --batch-rounds
     rounds per call of schedule.search, the seconds of a call of no rounds (the input decode and the launches) beside it.
  c  quality: final makespans on Mk01, Mk04, Mk06, Mk10 from the same 8 rule schedules, sideways descent at --rounds and tabu
     search (critical neighbourhood) at --tabu-rounds, beside improve's.  A report; the draws differ from improve's.
One JSON line per measurement, also written to --out.

    python tools/bench_search.py [--envs 4096] [--rounds 400] [--batch-rounds 20] [--tabu-rounds 20000] [--out profiles/search_bench.jsonl]
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
from deep_reinforcement_learning_for_fjsp_amd import instances as fi  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd import schedule as sch  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, global_actions  # noqa: E402
from tests import helpers as H  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--neighbours", type=int, default=64)
ap.add_argument("--regions", type=int, default=25)
ap.add_argument("--window", type=float, default=0.3)
ap.add_argument("--rounds", type=int, default=400)
ap.add_argument("--batch-rounds", type=int, default=20)
ap.add_argument("--tabu-rounds", type=int, default=20000)
ap.add_argument("--tenure", type=int, default=8)
ap.add_argument("--parts", default="abc")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "search_bench.jsonl"))
args = ap.parse_args()
if args.regions < 25:
    ap.error("--regions must be at least 25")
if not torch.cuda.is_available():
    sys.exit("bench_search needs an MI355X: nothing here is measured on a CPU")
N, Q = args.envs, args.neighbours
lines = []


def emit(**kw):
    kw.update(gpu=torch.cuda.get_device_name(0))
    print(json.dumps(kw), flush=True)
    lines.append(kw)


def spread(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


def timed(fn):
    """Seconds per call: a warm-up call, then --regions regions of about --window seconds each."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    calls = max(1, int(args.window / max(time.perf_counter() - t0, 1e-6)))
    ts = []
    for _ in range(args.regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / calls)
    return ts, calls


def rule_schedules(b, seed):
    """One episode of random rule pairs on every env, recorded: its plan."""
    T = b.record_schedule()
    acts = torch.from_numpy(global_actions(seed, 0, b.N, T, 6, 5)).cuda()
    b.reset()
    b.rollout(acts, trace=False, rewards=False, state=False)
    table, _ = b.schedule()
    b.record_schedule(False)
    return sch.plan_of(table).contiguous()


mk = {a.name: a for suite in ("mk01", "large") for a in H.load_suite(suite)[0] if "Mk" in a.name}


def brandimarte(tag):
    a = next(v for k, v in mk.items() if tag in k)
    b = EnvBatch(H.instance_set_from([a]), 8, rng_seed=2)
    return a, b, rule_schedules(b, 11)


if "a" in args.parts:
    for tag in ("Mk10", "Mk01"):
        a, b, plan = brandimarte(tag)
        for nbh in sch.SEARCH_NEIGHBOURHOODS:
            fused, _ = timed(lambda: PS.local_search(b, plan, args.rounds, Q, "makespan", 0, "sideways", args.tenure, nbh))
            loop, _ = timed(lambda: PS.improve(b, plan, args.rounds, Q, "makespan", 0, True, nbh))
            emit(what="round_against_improve", instance=a.name, envs=8, neighbours=Q, rounds=args.rounds, neighbourhood=nbh, lds_bytes=b.search_lds(),
                 local_search_seconds_per_round=spread([t / args.rounds for t in fused]), improve_seconds_per_round=spread([t / args.rounds for t in loop]),
                 fused_faster=bool(max(fused) < min(loop)), speedup_of_medians=float(np.median(loop) / np.median(fused)))

if "b" in args.parts:
    s10 = fi.InstanceSet(64).generate_range(1000, fi.bench_10x5_params()).solve_fluid()
    insts, _, _ = H.load_suite("multijob")
    big = max(insts, key=lambda x: int((np.asarray(x.count) * np.asarray(x.Jr)[None, :]).sum()))
    for name, s in (("10x5", s10), ("multijob " + big.name, H.instance_set_from([big]))):
        b = EnvBatch(s, N, rng_seed=1)
        plan = rule_schedules(b, 7)
        rows = b.decode_capacity()
        idle, _ = timed(lambda: sch.search(b, plan, 0, Q))
        for nbh in range(3):
            for accept in (1, 2):
                ts, calls = timed(lambda: sch.search(b, plan, args.batch_rounds, Q, 0, nbh, accept, args.tenure, 3))
                res = sch.search(b, plan, args.batch_rounds, Q, 0, nbh, accept, args.tenure, 3)
                assert bool((res["status"] == 0).all())
                emit(what="round_at_batch_scale", instances=name, envs=N, neighbours=Q, rows=rows, lds_bytes=b.search_lds(), rounds=args.batch_rounds,
                     neighbourhood=sch.SEARCH_NEIGHBOURHOODS[nbh], accept=sch.SEARCH_ACCEPT[accept], calls_per_region=calls,
                     seconds_per_round=spread([(t - float(np.median(idle))) / args.batch_rounds for t in ts]), seconds_of_no_rounds=spread(idle),
                     accepted_mean=float(res["accepted"].float().mean()))

if "c" in args.parts:
    for tag in ("Mk01", "Mk04", "Mk06", "Mk10"):
        a, b, plan = brandimarte(tag)
        out = dict(what="quality", instance=a.name, envs=8, neighbours=Q, rounds=args.rounds, tabu_rounds=args.tabu_rounds, tenure=args.tenure)
        out["start"] = sch.decode(b, plan)["objective"][:, 0, 0].tolist()
        for nbh in sch.SEARCH_NEIGHBOURHOODS:
            out["improve_" + nbh] = PS.improve(b, plan, args.rounds, Q, "makespan", 0, True, nbh)["history"][-1].tolist()
            out["sideways_" + nbh] = PS.local_search(b, plan, args.rounds, Q, "makespan", 0, "sideways", args.tenure, nbh)["objective"][:, 0].tolist()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tabu = PS.local_search(b, plan, args.tabu_rounds, Q, "makespan", 0, "tabu", args.tenure, "critical")
        torch.cuda.synchronize()
        out.update(tabu_critical=tabu["objective"][:, 0].tolist(), tabu_seconds=time.perf_counter() - t0, tabu_accepted=tabu["accepted"].tolist())
        out["tabu_critical_at_rounds"] = PS.local_search(b, plan, args.rounds, Q, "makespan", 0, "tabu", args.tenure, "critical")["objective"][:, 0].tolist()
        emit(**out)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for kw in lines:
        f.write(json.dumps(kw) + "\n")
