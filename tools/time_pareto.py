"""Cost of pareto.select (fjsp_pareto_select) next to an eager torch formulation of the same result, and the split of
policy_search.pareto_front between playing the episodes and selecting the front.

select: N source envs (default 4096), (C, D) = (80, 2), (80, 3), (1024, 3); integer-valued objectives drawn from 0..199
(makespans and tardiness sums are integers: ties and duplicates occur).  After a warm-up, --regions (at least 25) timed
regions, each --calls calls between two device synchronisations on a host clock; reported per call, median [min, max].
The eager formulation (the [N, C, C, D] comparisons, the duplicate rule, the lexicographic rank, the scatter into index)
runs at C = 80 only -- at 1024 its boolean intermediates alone are 4 GB each -- and is first checked to return the
kernel's index, count and mask.
pareto_front: N generated SO_FJSSP 10x5 envs over 64 instances, 5 seeded untrained ActorNet(20, 128, 2, 30), k = 16 (80
candidates), makespan and tardiness; the `timings` parts "play" and "select" of --reps calls after a warm-up.
One JSON line per measurement, also written to --out.

    python tools/time_pareto.py [--envs 4096] [--regions 25] [--calls 10] [--reps 5] [--out profiles/pareto_timing.jsonl]
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
from deep_reinforcement_learning_for_fjsp_amd import pareto  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.MPPPO import ActorNet  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--regions", type=int, default=25)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pareto_timing.jsonl"))
args = ap.parse_args()
if args.regions < 25:
    ap.error("--regions must be at least 25")
N = args.envs
lines = []


def emit(**kw):
    kw.update(envs=N, gpu=torch.cuda.get_device_name(0))
    print(json.dumps(kw), flush=True)
    lines.append(kw)


def spread(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


def eager_select(obj):
    """pareto.select(obj) in eager torch: (index i32[N, C], count i32[N], mask u8[C, N])."""
    C, n, D = obj.shape
    x = obj.permute(1, 0, 2)                                                 # [N, C, D]
    cand = ~torch.isnan(x).any(dim=2)
    a, b = x[:, :, None, :], x[:, None, :, :]                                # a = candidate j, b = candidate c
    le, lt = (a <= b).all(dim=3), (a < b).any(dim=3)
    ar = torch.arange(C, device=obj.device)
    out = (le & (lt | (ar[:, None] < ar[None, :]))).any(dim=1)
    front = cand & ~out                                                      # [N, C]
    below = torch.zeros_like(le)
    for d in range(D - 1, -1, -1):
        below = (a[..., d] < b[..., d]) | ((a[..., d] == b[..., d]) & below)
    rank = (below & front[:, :, None]).sum(dim=1)                            # front members lexicographically below c
    index = torch.full((n, C + 1), -1, dtype=torch.int32, device=obj.device)
    index.scatter_(1, torch.where(front, rank, torch.full_like(rank, C)), ar.to(torch.int32)[None, :].expand(n, C).contiguous())
    return index[:, :C].contiguous(), front.sum(dim=1).to(torch.int32), front.t().to(torch.uint8).contiguous()


def seconds_per_call(fn):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(args.regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / args.calls)
    return spread(ts)


for C, D in ((80, 2), (80, 3), (1024, 3)):
    gen = torch.Generator(device="cuda").manual_seed(100 * C + D)
    obj = torch.randint(0, 200, (C, N, D), device="cuda", generator=gen).double()
    index, count, mask = pareto.select(obj)
    emit(what="pareto_select_kernel", n_cand=C, n_obj=D, input_bytes=obj.numel() * 8, mean_front=count.double().mean().item(),
         max_front=int(count.max()), seconds=seconds_per_call(lambda: pareto.select(obj)))
    if C <= 80:
        for got, want in zip(eager_select(obj), (index, count, mask)):
            assert torch.equal(got, want), "the eager formulation differs from the kernel"
        emit(what="pareto_select_eager_torch", n_cand=C, n_obj=D, seconds=seconds_per_call(lambda: eager_select(obj)))
    del obj

P, k, n_inst = 5, 16, 64
s = fi.InstanceSet(n_inst).generate_range(1000, fi.bench_10x5_params()).solve_fluid()
actors = []
for p in range(P):
    torch.manual_seed(p)
    actors.append(ActorNet(20, 128, 2, 30).cuda())
b = EnvBatch(s, N, rng_seed=1)
b.reset()
res = PS.pareto_front(b, actors, k, seed=5)                                  # warm-up; builds the branch batch
parts = {}
for _ in range(args.reps):
    timings = {}
    res = PS.pareto_front(b, actors, k, seed=5, branch=res["branch"], timings=timings)
    for key, v in timings.items():
        parts.setdefault(key, []).append(v)
emit(what="pareto_front", actors=P, k=k, n_cand=P * k, n_obj=2, branch_envs=k * N, seconds={key: spread(v) for key, v in parts.items()},
     mean_front=res["count"].double().mean().item(), max_front=int(res["count"].max()))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for kw in lines:
        f.write(json.dumps(kw) + "\n")
