"""Cost of recording the dispatched schedule (fjsp_env_record_schedule): per-step launches and the fused rollout, with
recording off and on, at 4096 and 262 144 environments, for SO_FJSSP 10x5 (row family) and the training distribution of
tools/bench_training_dist.py (wave family).  Off and on are timed interleaved, repetition by repetition; prints one JSON
line per (workload, N) with both medians and the 10th / 90th percentile of the per-repetition ratio on / off.

    python tools/time_schedule.py [--envs 4096,262144] [--reps 15]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_reinforcement_learning_for_fjsp_amd import instances as fi  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, global_actions  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", default="4096,262144")
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--steps", type=int, default=40, help="per-step launches timed per repetition")
args = ap.parse_args()


def workloads():
    s10 = fi.InstanceSet(256).generate_range(1000, fi.bench_10x5_params()).solve_fluid()
    tr = fi.InstanceSet(64)
    for i in range(64):
        tr.generate(i, 5000 + i, fi.reference_generator_params(1.0, 15, 1))
    tr.solve_fluid()
    return [("so_fjssp_10x5", s10), ("training_dist", tr)]


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


def ab(fn_off, fn_on, reps):
    """Interleaved A/B: every repetition times both, in alternating order, so drifts of the clock or of the neighbours
    on the device hit both sides alike.  Returns (median off, median on, per-repetition ratios on / off)."""
    fn_off(); fn_on()
    off, on = [], []
    for r in range(reps):
        if r % 2:
            on.append(once(fn_on)); off.append(once(fn_off))
        else:
            off.append(once(fn_off)); on.append(once(fn_on))
    ratio = np.array(on) / np.array(off)
    return float(np.median(off)), float(np.median(on)), ratio


def summary(off, on, ratio):
    return dict(off_us=round(off, 1), on_us=round(on, 1), on_over_off_median=round(float(np.median(ratio)), 4),
                on_over_off_p10_p90=[round(float(np.percentile(ratio, 10)), 4), round(float(np.percentile(ratio, 90)), 4)])


for name, s in workloads():
    K = max(s.dims(i)["K"] for i in range(len(s)))
    for N in [int(x) for x in args.envs.split(",")]:
        acts = torch.from_numpy(global_actions(1, 0, N, max(K, args.steps), 6, 5)).cuda()
        b_off, b_on = EnvBatch(s, N, rng_seed=3), EnvBatch(s, N, rng_seed=3)
        b_on.record_schedule()

        def steps(b):
            # per-step launches from the start of an episode (the first `steps` dispatches), state returned
            def f():
                b.reset()
                for t in range(args.steps):
                    b.step(acts[t])
            return f

        def roll(b):
            # one fused launch of K steps (trace only)
            def f():
                b.reset()
                b.rollout(acts[:K], rewards=False, state=False)
            return f
        st = summary(*ab(steps(b_off), steps(b_on), args.reps))
        ro = summary(*ab(roll(b_off), roll(b_on), args.reps))
        print(json.dumps(dict(workload=name, N=N, family=b_off.kernel_family, reps=args.reps, step_launches=args.steps,
                              step_loop=st, rollout_T=K, rollout=ro)), flush=True)
        del b_off, b_on
        torch.cuda.empty_cache()
