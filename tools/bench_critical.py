"""Cost of schedule.critical (fjsp_schedule_critical) beside schedule.decode of the same candidates, and
policy_search.improve's three neighbourhoods side by side.  Protocol of tools/bench_decode.py.

critical: N envs (default 4096) x 1 table (the parents' own, in begin order: what a round of improve analyses) and x 64
tables (the tables of 64 decoded neighbours per env) on
  10x5     the bench instances (instances.bench_10x5_params, 64 of them)
  multijob the largest instance of tests/golden/multijob.npz (305 operations, 10 machines),
with max_moves 0 and 128, and in the same run the decode of the same candidates without and with their tables.  After a
warm-up, --regions (at least 25) timed regions of as many calls as fill --window seconds, between two device
synchronisations on a host clock.  Reported: seconds per call and table rows per second (median [min, max]), and the ratio
of the medians critical / decode.

improve: --improve-rounds x 64 neighbours (default 400) from 8 rule schedules each of Mk01, Mk04, Mk06 and Mk10
(tests/golden), makespan, sideways moves accepted, seed 0, once per neighbourhood, with the seconds per round.
One JSON line per measurement, also written to --out.

    python tools/bench_critical.py [--envs 4096] [--regions 25] [--window 0.3] [--improve-rounds 400] [--out profiles/critical_bench.jsonl]
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
ap.add_argument("--improve-rounds", type=int, default=400)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "critical_bench.jsonl"))
args = ap.parse_args()
if args.regions < 25:
    ap.error("--regions must be at least 25")
if not torch.cuda.is_available():
    sys.exit("bench_critical needs an MI355X: nothing here is measured on a CPU")
N, Q = args.envs, args.neighbours
lines = []


def emit(**kw):
    kw.update(gpu=torch.cuda.get_device_name(0))
    print(json.dumps(kw), flush=True)
    lines.append(kw)


def spread(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


def timed(fn):
    """Seconds per call: warm-up, then --regions regions of about --window seconds each."""
    for _ in range(3):
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
    """One episode of random rule pairs on every env, recorded: (plan, table, length)."""
    T = b.record_schedule()
    acts = torch.from_numpy(global_actions(seed, 0, b.N, T, 6, 5)).cuda()
    b.reset()
    b.rollout(acts, trace=False, rewards=False, state=False)
    table, length = b.schedule()
    b.record_schedule(False)
    return sch.plan_of(table).contiguous(), table, length


def bench(name, s):
    b = EnvBatch(s, N, rng_seed=1)
    cap = b.decode_capacity()
    _, table, length = rule_schedules(b, 7)
    plan, table = sch.begin_order(table)
    plan = plan.contiguous()
    L = length.to(torch.int64)
    for q in (1, Q):
        if q == 1:
            moves, tables = None, table[:, None].contiguous()
        else:
            # the neighbours a round of improve("critical") decodes: uniform draws from each parent's critical moves
            crit = b.critical(table, 1, PS.CRITICAL_MOVES)
            listed = crit["n_moves"][:, 0].to(torch.int64).clamp(min=1, max=PS.CRITICAL_MOVES)[:, None]
            gen = torch.Generator(device="cuda").manual_seed(3)
            slot = (torch.rand(N, q, generator=gen, device="cuda", dtype=torch.float64) * listed).to(torch.int64).clamp(max=PS.CRITICAL_MOVES - 1)
            moves = crit["moves"][:, 0][torch.arange(N, device="cuda")[:, None], slot].contiguous()
            res = b.decode(plan, moves, q, want_table=True)
            tables = res["table"]
            emit(what="candidates", instances=name, envs=N, tables=q, decoded_fraction=float((res["status"] == 0).double().mean()))
        rows = float(L.sum()) * q
        med = {}
        for what, fn in (("decode", lambda: b.decode(plan, moves, q)), ("decode_with_table", lambda: b.decode(plan, moves, q, want_table=True)),
                         ("critical_no_moves", lambda: b.critical(tables, q, 0)), ("critical_128_moves", lambda: b.critical(tables, q, PS.CRITICAL_MOVES))):
            ts, calls = timed(fn)
            med[what] = float(np.median(ts))
            emit(what=what, instances=name, envs=N, tables=q, rows=cap, group=b.decode_group(), calls_per_region=calls, seconds=spread(ts),
                 rows_per_second=spread([rows / t for t in ts]))
        res = b.critical(tables, q, PS.CRITICAL_MOVES)
        ok = res["status"] == 0
        emit(what="ratio", instances=name, envs=N, tables=q, critical_128_over_decode=med["critical_128_moves"] / med["decode"],
             critical_128_over_decode_with_table=med["critical_128_moves"] / med["decode_with_table"],
             critical_0_over_decode=med["critical_no_moves"] / med["decode"],
             mean_path_len=float(res["path_len"][ok].double().mean()), mean_n_moves=float(res["n_moves"][ok].double().mean()),
             skipped=int(res["skipped"].sum()))


s = fi.InstanceSet(64).generate_range(1000, fi.bench_10x5_params()).solve_fluid()
bench("10x5", s)
insts, _, _ = H.load_suite("multijob")
big = max(insts, key=lambda a: int((np.asarray(a.count) * np.asarray(a.Jr)[None, :]).sum()))
bench("multijob " + big.name, H.instance_set_from([big]))

if args.improve_rounds > 0:
    mk = [a for suite in ("mk01", "large") for a in H.load_suite(suite)[0] if "Mk" in a.name]
    for a in mk:
        b = EnvBatch(H.instance_set_from([a]), 8, rng_seed=2)
        plan = rule_schedules(b, 11)[0]
        for nb in PS.IMPROVE_NEIGHBOURHOODS:
            PS.improve(b, plan, 2, Q, "makespan", seed=0, neighbourhood=nb)          # (warm-up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = PS.improve(b, plan, args.improve_rounds, Q, "makespan", seed=0, sideways=True, neighbourhood=nb)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            emit(what="improve", instance=a.name, neighbourhood=nb, envs=8, rounds=args.improve_rounds, neighbours=Q, seconds=dt,
                 seconds_per_round=dt / args.improve_rounds, makespan_start=res["history"][0].tolist(), makespan_end=res["history"][-1].tolist(),
                 accepted=res["accepted"].tolist())

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for kw in lines:
        f.write(json.dumps(kw) + "\n")
