"""Cost and quality of policy_search.beam_search next to the other decoders, on N generated SO_FJSSP 10x5 envs (one
instance each) with a seeded, untrained ActorNet(20, 128, 2, 30) and every action of the variant as candidate.

Per width: one warm-up episode (it also builds the beam and expansion batches), then --reps episodes per score with a
`timings` dict: the synchronised seconds of every part divided by the decisions of the episode, median [min, max] over the
repeats, and the whole call per decision from a synchronised wall clock.  fjsp_beam_select alone comes from device events
around the launch (median of 20) at the search's own shape and at the entry point's limits.  Quality: mean makespan of
greedy play, best_of(k = width) and both beam scores, every decoder from a reset of the same batch.  One JSON line per
measurement, also written to --out.

    python tools/time_beam_search.py [--envs 64] [--widths 1 4 16] [--reps 3] [--out profiles/beam_search_timing.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_reinforcement_learning_for_fjsp_amd import instances as fi  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.MPPPO import ActorNet  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=64)
ap.add_argument("--widths", type=int, nargs="+", default=[1, 4, 16])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                              "beam_search_timing.jsonl"))
args = ap.parse_args()
N = args.envs
lines = []


def emit(**kw):
    kw.update(envs=N, gpu=torch.cuda.get_device_name(0))
    print(json.dumps(kw), flush=True)
    lines.append(kw)


def spread(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


def select_kernel_seconds(W, n_src, A, Wo):
    cost = torch.randn(W, n_src, A, dtype=torch.float64, device="cuda")
    PS.beam_select(cost, None, Wo)
    ts = []
    for _ in range(20):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); PS.beam_select(cost, None, Wo); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return spread(ts)


s = fi.InstanceSet(N).generate_range(1000, fi.bench_10x5_params()).solve_fluid()
torch.manual_seed(0)
actor = ActorNet(20, 128, 2, 30).cuda()
b = EnvBatch(s, N, rng_seed=1)

b.reset(); PS.play(b, actor)
emit(what="greedy_play", mean_makespan=b.read()["makespan"].double().mean().item())

for W in args.widths:
    b.reset()
    emit(what="best_of", k=W, mean_makespan=PS.best_of(b, actor, W, "makespan", seed=5)["objective"].mean().item())
    emit(what="beam_select_kernel", width=W, n_src=N, n_actions=30, seconds=select_kernel_seconds(W, N, 30, W))
    for score in PS.BEAM_SCORES:
        b.reset()
        res = PS.beam_search(b, actor, W, objective="makespan", score=score)          # warm-up; builds the batches
        beams, expand = res["beams"], res["expand"]
        parts, whole = {}, []
        for _ in range(args.reps):
            b.reset()
            timings = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = PS.beam_search(b, actor, W, objective="makespan", score=score, beams=beams, expand=expand, timings=timings)
            torch.cuda.synchronize()
            D = int(res["steps"].max())
            whole.append((time.perf_counter() - t0) / D)
            for k, v in timings.items():
                parts.setdefault(k, []).append(v / D)
        emit(what="beam_search", score=score, width=W, decisions=D, beam_envs=W * N, expansion_envs=0 if expand is None else expand.N,
             seconds_per_decision=spread(whole), parts_per_decision={k: spread(v) for k, v in parts.items()},
             mean_makespan=res["objective"].mean().item(), winner_is_rank_0=float((res["best"] == 0).double().mean().item()))
        del beams, expand, res

emit(what="beam_select_kernel", width=64, n_src=4096, n_actions=128, seconds=select_kernel_seconds(64, 4096, 128, 64))
emit(what="beam_select_kernel", width=16, n_src=4096, n_actions=30, seconds=select_kernel_seconds(16, 4096, 30, 16))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for kw in lines:
        f.write(json.dumps(kw) + "\n")
