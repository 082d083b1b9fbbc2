"""Cost and result of the fused search on MO_DFJSP (fjsp_schedule_search_dyn: schedule.search_dyn, policy_search.local_search on
such a batch) beside policy_search.improve and beside one fjsp_schedule_decode_dyn call, with the protocol of
tools/bench_search.py: after a warm-up, --regions (at least 25) timed regions of as many calls as fill --window seconds,
between two device synchronisations on a host clock, the entries of a comparison taking turns region by region; median
[min, max].  The shops are recorded MO_DFJSP episodes of tests/golden/schedule.npz: gen8801 (76 rows, 6 machines, 19
windows, 3 orders) and industrial/DDT0.5_M20_S1 (249 rows, 20 machines, 63 windows: the shop of tools/bench_decode_dyn.py).

  a  per round against improve: 8 envs x 64 neighbours from the recorded schedule, --rounds rounds (default 400), sideways
     moves accepted, per objective, on both shops.  local_search includes its final decode_dyn.  "fused_faster": the slowest
     local_search region is below the fastest improve region.
  b  per round at batch scale: --envs (default 4096) x 64 on the 249-row shop, --batch-rounds rounds per call of
     schedule.search_dyn, the seconds of a call of no rounds subtracted, beside one schedule.decode_dyn call of the same
     envs x 64 candidates (bench_decode_dyn.py's moves).  The ratio is a report.
  c  quality, for the record: tabu search, --tenure, 64 neighbours, --tabu-rounds rounds on gen8801 from the recorded schedule
     and seven random plans, per objective: the chosen objective at the start and of the returned plans.
One JSON line per measurement, also written to --out.

    python tools/bench_search_dyn.py [--envs 4096] [--rounds 400] [--batch-rounds 20] [--tabu-rounds 20000] [--out profiles/search_dyn_bench.jsonl]
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
ap.add_argument("--neighbours", type=int, default=64)
ap.add_argument("--regions", type=int, default=25)
ap.add_argument("--window", type=float, default=0.3)
ap.add_argument("--rounds", type=int, default=400)
ap.add_argument("--batch-rounds", type=int, default=20)
ap.add_argument("--tabu-rounds", type=int, default=20000)
ap.add_argument("--tenure", type=int, default=8)
ap.add_argument("--parts", default="abc")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "search_dyn_bench.jsonl"))
args = ap.parse_args()
if args.regions < 25:
    ap.error("--regions must be at least 25")
if not torch.cuda.is_available():
    sys.exit("bench_search_dyn needs an MI355X: nothing here is measured on a CPU")
N, Q = args.envs, args.neighbours
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


if "a" in args.parts:
    for ep in (small, big):
        b, plan = recorded(ep, 8)
        for objective in sch.SEARCH_DYN_OBJECTIVES:
            (fused, loop), _ = timed_in_turns([lambda: PS.local_search(b, plan, args.rounds, Q, objective, 0, "sideways", args.tenure),
                                               lambda: PS.improve(b, plan, args.rounds, Q, objective, 0, True)])
            emit(what="round_against_improve", instance=ep["inst"].name, envs=8, neighbours=Q, rows=b.decode_capacity(), rounds=args.rounds,
                 objective=objective, lds_bytes=b.search_dyn_lds(), local_search_seconds_per_round=spread([t / args.rounds for t in fused]),
                 improve_seconds_per_round=spread([t / args.rounds for t in loop]), fused_faster=bool(max(fused) < min(loop)),
                 speedup_of_medians=float(np.median(loop) / np.median(fused)))

if "b" in args.parts:
    b, plan = recorded(big, N)
    cap = b.decode_capacity()
    gen = torch.Generator(device="cuda").manual_seed(3)
    odd = (torch.arange(Q, device="cuda") % 2 == 1)[None, :]
    span = torch.where(odd, cap - 1, cap).expand(N, Q)
    u = torch.minimum((torch.rand(N, Q, generator=gen, device="cuda", dtype=torch.float64) * span).to(torch.int64), span - 1)
    m = plan[torch.arange(N, device="cuda")[:, None], u, 2].to(torch.int64)
    moves = torch.stack([torch.where(odd, 2, 1).expand(N, Q), u, m], -1).to(torch.int32).contiguous()
    assert bool((b.decode_dyn(plan, moves, Q)["status"] == 0).all())
    for accept in (1, 2):
        res = sch.search_dyn(b, plan, args.batch_rounds, Q, 0, accept, args.tenure, 3)
        assert bool((res["status"] == 0).all())
        (ts, idle, dec), calls = timed_in_turns([lambda: sch.search_dyn(b, plan, args.batch_rounds, Q, 0, accept, args.tenure, 3),
                                                 lambda: sch.search_dyn(b, plan, 0, Q), lambda: b.decode_dyn(plan, moves, Q)])
        per_round = [(t - float(np.median(idle))) / args.batch_rounds for t in ts]
        emit(what="round_at_batch_scale", instance=big["inst"].name, envs=N, neighbours=Q, rows=cap, lds_bytes=b.search_dyn_lds(),
             rounds=args.batch_rounds, accept=sch.SEARCH_ACCEPT[accept], calls_per_region=calls, seconds_per_round=spread(per_round),
             seconds_of_no_rounds=spread(idle), decode_dyn_seconds_per_call=spread(dec), decode_dyn_group=b.decode_dyn_group(),
             round_over_decode_of_medians=float(np.median(per_round) / np.median(dec)), accepted_mean=float(res["accepted"].float().mean()))

if "c" in args.parts:
    b, plan = recorded(small, 8)
    rs = np.random.RandomState(7)
    plan[1:] = torch.from_numpy(np.stack([D.random_plan(small["inst"], rs, b.decode_capacity()) for _ in range(7)])).cuda()
    start = b.decode_dyn(plan)["objective"][:, 0]
    for col, objective in enumerate(sch.SEARCH_DYN_OBJECTIVES):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tabu = PS.local_search(b, plan, args.tabu_rounds, Q, objective, 0, "tabu", args.tenure)
        torch.cuda.synchronize()
        emit(what="quality", instance=small["inst"].name, envs=8, neighbours=Q, tabu_rounds=args.tabu_rounds, tenure=args.tenure, objective=objective,
             start=start[:, col].tolist(), end=tabu["objective"][:, col].tolist(), end_all_objectives=tabu["objective"].tolist(),
             seconds=time.perf_counter() - t0, accepted=tabu["accepted"].tolist())

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for kw in lines:
        f.write(json.dumps(kw) + "\n")
