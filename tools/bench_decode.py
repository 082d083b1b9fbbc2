"""Cost of schedule.decode (fjsp_schedule_decode) and what policy_search.improve makes of rule schedules.

decode: N envs (default 4096) x 64 neighbours of one parent plan per env -- the launch of one round of improve -- on
  10x5     the bench instances (instances.bench_10x5_params, 64 of them)
  multijob the largest instance of tests/golden/multijob.npz (305 operations, 10 machines).
The parents are the schedules of one episode of random rule pairs; even candidates reassign a uniform row to the machine it
has, odd ones swap a uniform row with its successor, so every candidate decodes its whole plan.  After a warm-up, --regions
(at least 25) timed regions of as many calls as fill --window seconds, between two device synchronisations on a host
clock.  Reported: decoded operations per second (median [min, max]); the HBM bytes per candidate the layout implies -- its
move, objective, status and length, and its share of what the env's candidates read together: the parent plan and the
instance's processing times, kind table, due dates and order rows -- and the fraction of the 8 TB/s HBM peak those bytes
per second are.  For context only: the numpy statement of the decoding (tests/decode_reference.py) on one core, and the
env kernels' own rollout of the same instances in env-steps (= dispatched operations) per second.

improve: --improve-rounds x 64 neighbours (default 400) from 8 rule schedules each of the Brandimarte instances the
repository holds (tests/golden: Mk01, Mk04, Mk06, Mk10), makespan, sideways moves accepted.
One JSON line per measurement, also written to --out.

    python tools/bench_decode.py [--envs 4096] [--regions 25] [--window 0.3] [--improve-rounds 400] [--out profiles/decode_bench.jsonl]
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
from tests import decode_reference as D  # noqa: E402
from tests import helpers as H  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--neighbours", type=int, default=64)
ap.add_argument("--regions", type=int, default=25)
ap.add_argument("--window", type=float, default=0.3)
ap.add_argument("--improve-rounds", type=int, default=400)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "decode_bench.jsonl"))
args = ap.parse_args()
if args.regions < 25:
    ap.error("--regions must be at least 25")
if not torch.cuda.is_available():
    sys.exit("bench_decode needs an MI355X: nothing here is measured on a CPU")
N, Q = args.envs, args.neighbours
HBM_PEAK = 8.0e12
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
    """One episode of random rule pairs on every env, recorded: (plan, table, length, actions u8[T, N, 2])."""
    T = b.record_schedule()
    acts = torch.from_numpy(global_actions(seed, 0, b.N, T, 6, 5)).cuda()
    b.reset()
    b.rollout(acts, trace=False, rewards=False, state=False)
    table, length = b.schedule()
    b.record_schedule(False)
    return sch.plan_of(table).contiguous(), table, length, acts


def shared_bytes(a, cap):
    """What the candidates of one env read together: the plan, p (u16 per pair), the kind table, due dates, order rows."""
    K, M = np.asarray(a.p).shape
    R, S = len(a.Jr), len(a.arrive)
    return cap * 12 + K * M * 2 + (R + 1) * 8 + int(np.asarray(a.count).sum()) * 4 + S * 4 + S * R * 2


def bench(name, s, arrs):
    b = EnvBatch(s, N, rng_seed=1)
    cap = b.decode_capacity()
    plan, table, length, acts = rule_schedules(b, 7)
    L = length.to(torch.int64)
    gen = torch.Generator(device="cuda").manual_seed(3)
    odd = (torch.arange(Q, device="cuda") % 2 == 1)[None, :]
    span = torch.where(odd, (L - 1)[:, None], L[:, None]).clamp(min=1)
    u = torch.minimum((torch.rand(N, Q, generator=gen, device="cuda", dtype=torch.float64) * span).to(torch.int64), span - 1)
    m = plan[torch.arange(N, device="cuda")[:, None], u, 2].to(torch.int64)
    moves = torch.stack([torch.where(odd, 2, 1).expand(N, Q), u, m], -1).to(torch.int32).contiguous()
    res = b.decode(plan, moves, Q)
    assert bool((res["status"] == 0).all()), "a benchmark candidate does not decode"
    assert torch.equal(b.decode(plan, None, 1, want_table=True)["table"][:, 0], table), "the parents do not decode to their recording"
    ops = float(L.sum()) * Q
    ts, calls = timed(lambda: b.decode(plan, moves, Q))
    per_cand = 12 + 16 + 4 + 4 + float(np.mean([shared_bytes(arrs[i % len(arrs)], cap) for i in range(min(N, len(arrs)))])) / Q
    rate = [ops / t for t in ts]
    emit(what="decode", instances=name, envs=N, neighbours=Q, candidates=N * Q, rows=cap, group=b.decode_group(), calls_per_region=calls,
         seconds=spread(ts), ops_per_second=spread(rate), hbm_bytes_per_candidate=per_cand,
         hbm_fraction_of_peak=spread([per_cand * N * Q / t / HBM_PEAK for t in ts]))
    # context: the env kernels' own rollout of the same instances
    def roll():
        b.reset()
        b.rollout(acts, trace=False, rewards=False, state=False)
    ts, calls = timed(roll)
    emit(what="env_rollout", instances=name, envs=N, calls_per_region=calls, seconds=spread(ts),
         env_steps_per_second=spread([float(L.sum()) / t for t in ts]))
    # context: numpy on one core, 64 candidates of env 0
    pl, mv = plan[:1].cpu().numpy(), moves[:1].cpu().numpy()
    t0 = time.perf_counter()
    ref = D.decode([arrs[0]], 0, pl, mv, Q)
    dt = time.perf_counter() - t0
    assert np.array_equal(ref["objective"], res["objective"][:1].cpu().numpy())
    emit(what="numpy_reference_one_core", instances=name, candidates=Q, seconds=dt, ops_per_second=float(L[0]) * Q / dt)


s = fi.InstanceSet(64).generate_range(1000, fi.bench_10x5_params()).solve_fluid()
bench("10x5", s, [s.arrays(i) for i in range(64)])
insts, _, _ = H.load_suite("multijob")
big = max(insts, key=lambda a: int((np.asarray(a.count) * np.asarray(a.Jr)[None, :]).sum()))
bench("multijob " + big.name, H.instance_set_from([big]), [big])

if args.improve_rounds > 0:
    mk = [a for suite in ("mk01", "large") for a in H.load_suite(suite)[0] if "Mk" in a.name]
    for a in mk:
        b = EnvBatch(H.instance_set_from([a]), 8, rng_seed=2)
        plan = rule_schedules(b, 11)[0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = PS.improve(b, plan, args.improve_rounds, Q, "makespan", seed=0, sideways=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        strict = PS.improve(b, plan, args.improve_rounds, Q, "makespan", seed=0, sideways=False)
        emit(what="improve", instance=a.name, envs=8, rounds=args.improve_rounds, neighbours=Q, seconds=dt,
             makespan_start=res["history"][0].tolist(), makespan_end=res["history"][-1].tolist(),
             makespan_end_strict=strict["history"][-1].tolist(), accepted=res["accepted"].tolist())

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for kw in lines:
        f.write(json.dumps(kw) + "\n")
