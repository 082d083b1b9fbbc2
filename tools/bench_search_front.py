"""Cost and result of the front search (fjsp_schedule_search_front: schedule.search_front, policy_search.front_search) beside
fjsp_schedule_search_dyn in the same process on the same arrays, with the protocol of tools/bench_search_dyn.py: after a
warm-up, --regions (at least 25) timed regions of as many calls as fill --window seconds, between two device
synchronisations on a host clock, the entries of a comparison taking turns region by region; median [min, max].  The
shops are that tool's: gen8801 (76 rows) and industrial/DDT0.5_M20_S1 (249 rows) of tests/golden/schedule.npz.

  a  the archive's cost per round: 8 envs x 64 neighbours from the recorded schedule, --rounds rounds (default 400), tabu,
     schedule.search_front under the unit weight (1, 0, 0) with 64 slots and member plans beside schedule.search_dyn on the
     makespan -- the same draws, moves and plans, round by round --, on both shops.
  b  per round at batch scale: --envs (default 4096) x 64 on the 249-row shop, --batch-rounds rounds per call, each entry's
     own call of no rounds subtracted: search_dyn, search_front with 16 and 64 slots, with and without d_front_plan, and one
     schedule.decode_dyn call of the same envs x 64 candidates.  The ratios are a report.
  c  for the record: front_search(merge=True) on gen8801, 64 envs from the recorded schedule and 63 random plans, one
     weight vector each -- the lattice a + b + c = 10 scaled by (60, 6, 1) to the columns' magnitudes, the unit vectors
     first, its 64 first points --, 16 slots (64 x 16 = pareto.select's 1024 candidates), --tabu-rounds tabu rounds: the
     merged front's size, and pareto.gd / igd against the front of the plans that three single-objective local_search runs of
     the same budget return on the same 64 start plans.
One JSON line per measurement, also written to --out.

    python tools/bench_search_front.py [--envs 4096] [--rounds 400] [--batch-rounds 20] [--tabu-rounds 20000] [--out profiles/search_front_bench.jsonl]
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
from deep_reinforcement_learning_for_fjsp_amd import pareto  # noqa: E402
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
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "search_front_bench.jsonl"))
args = ap.parse_args()
if args.regions < 25:
    ap.error("--regions must be at least 25")
if not torch.cuda.is_available():
    sys.exit("bench_search_front needs an MI355X: nothing here is measured on a CPU")
N, Q = args.envs, args.neighbours
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
        b, plan = recorded(ep, 8)
        w = unit(8)
        one = sch.search_dyn(b, plan, args.rounds, Q, 0, TABU, args.tenure, 0, trace=True)
        arch = sch.search_front(b, plan, w, args.rounds, Q, 64, TABU, args.tenure, 0, trace=True)
        assert all(torch.equal(one[key], arch[key]) for key in one)                # the same search, round by round
        (front, dyn), _ = timed_in_turns([lambda: sch.search_front(b, plan, w, args.rounds, Q, 64, TABU, args.tenure, 0),
                                          lambda: sch.search_dyn(b, plan, args.rounds, Q, 0, TABU, args.tenure, 0)])
        emit(what="archive_cost_per_round", instance=ep["inst"].name, envs=8, neighbours=Q, rows=b.decode_capacity(), rounds=args.rounds,
             cap_front=64, lds_bytes=b.search_front_lds(64), search_dyn_lds_bytes=b.search_dyn_lds(),
             search_front_seconds_per_round=spread([t / args.rounds for t in front]), search_dyn_seconds_per_round=spread([t / args.rounds for t in dyn]),
             front_over_dyn_of_medians=float(np.median(front) / np.median(dyn)), members=arch["front_count"].tolist(),
             dropped=arch["front_dropped"].tolist())

if "b" in args.parts:
    b, plan = recorded(big, N)
    cap = b.decode_capacity()
    w = unit(N)
    gen = torch.Generator(device="cuda").manual_seed(3)
    odd = (torch.arange(Q, device="cuda") % 2 == 1)[None, :]
    span = torch.where(odd, cap - 1, cap).expand(N, Q)
    u = torch.minimum((torch.rand(N, Q, generator=gen, device="cuda", dtype=torch.float64) * span).to(torch.int64), span - 1)
    m = plan[torch.arange(N, device="cuda")[:, None], u, 2].to(torch.int64)
    moves = torch.stack([torch.where(odd, 2, 1).expand(N, Q), u, m], -1).to(torch.int32).contiguous()
    assert bool((b.decode_dyn(plan, moves, Q)["status"] == 0).all())
    R = args.batch_rounds
    (dyn, dyn0, dec), _ = timed_in_turns([lambda: sch.search_dyn(b, plan, R, Q, 0, TABU, args.tenure, 3), lambda: sch.search_dyn(b, plan, 0, Q),
                                          lambda: b.decode_dyn(plan, moves, Q)])
    dyn_round = [(t - float(np.median(dyn0))) / R for t in dyn]
    emit(what="round_at_batch_scale", entry="search_dyn", instance=big["inst"].name, envs=N, neighbours=Q, rows=cap, rounds=R,
         lds_bytes=b.search_dyn_lds(), seconds_per_round=spread(dyn_round), seconds_of_no_rounds=spread(dyn0), decode_dyn_seconds_per_call=spread(dec))
    for cap_front in (16, 64):
        for plans in (True, False):
            res = sch.search_front(b, plan, w, R, Q, cap_front, TABU, args.tenure, 3, want_plans=plans)
            assert bool((res["status"] == 0).all())
            members, dropped = float(res["front_count"].float().mean()), float(res["front_dropped"].float().mean())
            del res
            (ts, idle, base, base0), calls = timed_in_turns([
                lambda: sch.search_front(b, plan, w, R, Q, cap_front, TABU, args.tenure, 3, want_plans=plans),
                lambda: sch.search_front(b, plan, w, 0, Q, cap_front, TABU, args.tenure, 3, want_plans=plans),
                lambda: sch.search_dyn(b, plan, R, Q, 0, TABU, args.tenure, 3), lambda: sch.search_dyn(b, plan, 0, Q)])
            per_round = [(t - float(np.median(idle))) / R for t in ts]
            base_round = [(t - float(np.median(base0))) / R for t in base]
            emit(what="round_at_batch_scale", entry="search_front", instance=big["inst"].name, envs=N, neighbours=Q, rows=cap, rounds=R,
                 cap_front=cap_front, front_plan=plans, lds_bytes=b.search_front_lds(cap_front), calls_per_region=calls,
                 seconds_per_round=spread(per_round), seconds_of_no_rounds=spread(idle), search_dyn_seconds_per_round=spread(base_round),
                 front_over_dyn_of_medians=float(np.median(per_round) / np.median(base_round)),
                 round_over_decode_of_medians=float(np.median(per_round) / np.median(dec)), members_mean=members, dropped_mean=dropped)

if "c" in args.parts:
    n = 64
    b, plan = recorded(small, n)
    rs = np.random.RandomState(7)
    plan[1:] = torch.from_numpy(np.stack([D.random_plan(small["inst"], rs, b.decode_capacity()) for _ in range(n - 1)])).cuda()
    lattice = [(a, c, 10 - a - c) for a in range(10, -1, -1) for c in range(10 - a, -1, -1)]
    units = [(10, 0, 0), (0, 10, 0), (0, 0, 10)]
    grid = (units + [p for p in lattice if p not in units])[:n]
    w = torch.tensor(grid, dtype=torch.int64) * torch.tensor([60, 6, 1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = PS.front_search(b, plan, args.tabu_rounds, w, Q, 16, "tabu", args.tenure, 0, merge=True)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    singles = []
    t0 = time.perf_counter()
    for objective in sch.SEARCH_DYN_OBJECTIVES:
        singles.append(PS.local_search(b, plan, args.tabu_rounds, Q, objective, 0, "tabu", args.tenure)["objective"])
    torch.cuda.synchronize()
    single_seconds = time.perf_counter() - t0
    cand = torch.cat(singles).to(torch.float64)[:, None, :].contiguous()              # [192, 1, 3]
    index, count, _ = pareto.select(cand)
    base = pareto.front_points(cand, index)
    mf, mc = res["merged_front"], res["merged_count"]
    both = torch.cat([mf[0, :int(mc[0])], base[0, :int(count[0])]])[:, None, :].contiguous()
    bi, bc, bmask = pareto.select(both)
    ours_on_joint = int(bmask[:int(mc[0]), 0].sum())
    emit(what="front_quality", instance=small["inst"].name, envs=n, neighbours=Q, tabu_rounds=args.tabu_rounds, tenure=args.tenure, cap_front=16,
         seconds=seconds, single_objective_seconds=single_seconds, merged_front_size=int(mc[0]), per_env_members=res["count"].tolist(),
         dropped_total=int(res["dropped"].sum()), single_objective_front_size=int(count[0]),
         gd_against_single=float(pareto.gd(mf, mc, base, count)[0]), igd_against_single=float(pareto.igd(mf, mc, base, count)[0]),
         gd_of_single_against_front=float(pareto.gd(base, count, mf, mc)[0]), igd_of_single_against_front=float(pareto.igd(base, count, mf, mc)[0]),
         joint_front_size=int(bc[0]), joint_front_members_from_front_search=ours_on_joint,
         merged_front=mf[0, :int(mc[0])].tolist(), single_objective_front=base[0, :int(count[0])].tolist())

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for kw in lines:
        f.write(json.dumps(kw) + "\n")
