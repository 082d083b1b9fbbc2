"""Cost of decoding a policy on the device (policy_search): greedy play through play_policy_kernel and through the
per-step loop, best-of-16, and policy-lookahead decisions, next to the fused training rollout (rollout_policy_kernel)
for the same batch.

N generated SO_FJSSP 10x5 envs (256 instances), an ActorNet(20, 128, 2, 30) with seeded weights.  Kernel times come
from device events around the launch (median of --reps, reset between repeats, not timed); whole calls that read back
on the host (play with its default step bound, the per-step loop, best_of, policy_lookahead) from a synchronised wall
clock.  policy_lookahead plays one whole episode with the 20 deterministic pairs and reports the mean seconds per
decision, split into its parts.  One JSON line per measurement, also written to --out.

    python tools/time_policy_search.py [--envs 4096] [--reps 20] [--out profiles/policy_search_timing.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_reinforcement_learning_for_fjsp_amd import _capi  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd import instances as fi  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.MPPPO import ActorNet, native_actor_params  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd.lookahead import ops_per_env  # noqa: E402

DET_SO = [(a, b) for a in range(5) for b in range(4)]

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--loop-reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                              "policy_search_timing.jsonl"))
args = ap.parse_args()
N = args.envs
lines = []


def emit(**kw):
    kw.update(envs=N, gpu=torch.cuda.get_device_name(0))
    print(json.dumps(kw), flush=True)
    lines.append(kw)


def event_timed(prep, fn, reps):
    ts = []
    for _ in range(reps):
        prep()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def wall_timed(prep, fn, reps):
    ts, out = [], None
    for _ in range(reps):
        prep()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts)), out


s = fi.InstanceSet(256).generate_range(1000, fi.bench_10x5_params()).solve_fluid()
torch.manual_seed(0)
actor = ActorNet(20, 128, 2, 30).cuda()
b = EnvBatch(s, N, rng_seed=1)
T = int(ops_per_env(b).max().item())

# greedy play, kernel only (explicit step bound: no read-back), and the whole call
med, lo, hi = event_timed(b.reset, lambda: PS.play(b, actor, max_steps=T), args.reps)
emit(what="play_greedy_kernel", steps=T, seconds_median=med, seconds_min=lo, seconds_max=hi)
mk_greedy = b.read()["makespan"].double().mean().item()
med, lo, hi, _ = wall_timed(b.reset, lambda: PS.play(b, actor), args.reps)
emit(what="play_greedy_call", seconds_median=med, seconds_min=lo, seconds_max=hi, mean_makespan=mk_greedy)
med, lo, hi = event_timed(b.reset, lambda: PS.play(b, actor, greedy=False, seed=3, max_steps=T), args.reps)
emit(what="play_sampled_kernel", steps=T, seconds_median=med, seconds_min=lo, seconds_max=hi)

# the same batch through the per-step loop (one actor launch, one env step and one read-back per step)
# (random.choice rules go on drawing across resets, so repeats of a greedy play need not end alike)
med, lo, hi, _ = wall_timed(b.reset, lambda: PS.play(b, actor, fused=False), args.loop_reps)
emit(what="play_greedy_per_step_loop", seconds_median=med, seconds_min=lo, seconds_max=hi)

# the fused training rollout of the same actor over 40 steps, buffer rows included (fjsp_env_rollout_policy)
lib = _capi.lib()
buf = C.c_void_p()
_capi.check(lib.fjsp_rollout_create(40, N, 20, 0, C.byref(buf)))
p = _capi.ptr
eps = torch.zeros(1, dtype=torch.float32, device="cuda")
seed = torch.tensor([7], dtype=torch.int64, device="cuda")
flat = torch.zeros(40, N, dtype=torch.float32, device="cuda")
logp = torch.zeros(40, N, dtype=torch.float32, device="cuda")
st0 = torch.zeros(N, 20, dtype=torch.float64, device="cuda")
apar = native_actor_params(actor)


def prep_rollout():
    st0.copy_(b.reset())


def rollout_policy():
    _capi.check(lib.fjsp_env_rollout_policy(b._h, buf, C.byref(apar), p(eps), p(seed), 5, 40, None, p(st0), p(flat), p(logp),
                                            b._p_state, b._stream()))


med, lo, hi = event_timed(prep_rollout, rollout_policy, args.reps)
lib.fjsp_rollout_destroy(buf)
emit(what="rollout_policy_kernel_40_steps", steps=40, seconds_median=med, seconds_min=lo, seconds_max=hi)

# best-of-16: a 16 x N branch, block 0 greedy
branch = None


def run_best():
    global branch
    r = PS.best_of(b, actor, 16, "makespan", seed=5, branch=branch)
    branch = r["branch"]
    return r


b.reset(); branch = run_best()["branch"]                # (builds the branch batch once, outside the timing)
med, lo, hi, res = wall_timed(b.reset, run_best, args.loop_reps)
emit(what="best_of_16", seconds_median=med, seconds_min=lo, seconds_max=hi,
     mean_makespan=res["objective"].mean().item(), block0_wins=float((res["best"] == 0).double().mean().item()))
del branch

# policy lookahead: one whole episode, mean seconds per decision
b.reset()
timings = {}
t0 = time.perf_counter()
res = PS.policy_lookahead(b, actor, "makespan", candidates=DET_SO, timings=timings)
torch.cuda.synchronize()
total = time.perf_counter() - t0
D = int(res["steps"].max())
emit(what="policy_lookahead_decision", decisions=D, branch_envs=len(DET_SO) * N, seconds_per_decision=total / D,
     parts_per_decision={k: v / D for k, v in timings.items()}, mean_makespan=res["objective"].mean().item())

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for kw in lines:
        f.write(json.dumps(kw) + "\n")
