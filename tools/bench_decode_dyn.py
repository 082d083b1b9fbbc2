"""Cost of schedule.decode_dyn (fjsp_schedule_decode_dyn) beside schedule.decode on the same arrays.

The shop is the MO_DFJSP episode 0 of tests/golden/schedule.npz (industrial/DDT0.5_M20_S1: 249 operations, 20 machines, 63
breakdown windows).  N envs (default 4096) x 64 neighbours of one parent plan per env, the launch of one round of
policy_search.improve: the parent is the reference's recorded schedule; even candidates reassign a uniform row to the
machine it has, odd ones swap a uniform row with its successor, so every candidate decodes its whole plan.  The same plans
and moves are decoded by fjsp_schedule_decode on a batch of the same arrays created as SO_DFJSP (no windows, no energy), in
the same process: after a warm-up, --regions (at least 25) timed regions per entry, the two entries taking turns region by
region, each region as many calls as fill --window seconds between two device synchronisations on a host clock.
Reported per entry: seconds per call and decoded operations per second (median [min, max]), the candidates per workgroup and
the bytes of LDS state per candidate; then the ratio of the two medians.  One JSON line per measurement, also written to --out.

    python tools/bench_decode_dyn.py [--envs 4096] [--regions 25] [--window 0.3] [--out profiles/decode_dyn_bench.jsonl]
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
from deep_reinforcement_learning_for_fjsp_amd import schedule as sch  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch  # noqa: E402
from tests import decode_dyn_reference as DD  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import schedule_fixture as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--neighbours", type=int, default=64)
ap.add_argument("--regions", type=int, default=25)
ap.add_argument("--window", type=float, default=0.3)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "decode_dyn_bench.jsonl"))
args = ap.parse_args()
if args.regions < 25:
    ap.error("--regions must be at least 25")
if not torch.cuda.is_available():
    sys.exit("bench_decode_dyn needs an MI355X: nothing here is measured on a CPU")
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
        for _ in range(3):
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
ep = eps[0]
a = ep["inst"]
s = H.instance_set_from([a])
dyn = EnvBatch(s, N, variant=variant, rng_seed=1)
plain = EnvBatch(s, N, variant=sch.VARIANT_SO_DFJSP, rng_seed=1)
cap = dyn.decode_capacity()
assert cap == plain.decode_capacity() == len(ep["table"])
parent = np.ascontiguousarray(ep["table"][:, [0, 2, 3]].astype(np.int32))
plan = torch.from_numpy(parent)[None].expand(N, cap, 3).contiguous().cuda()
L = cap
gen = torch.Generator(device="cuda").manual_seed(3)
odd = (torch.arange(Q, device="cuda") % 2 == 1)[None, :]
span = torch.where(odd, L - 1, L).expand(N, Q)
u = torch.minimum((torch.rand(N, Q, generator=gen, device="cuda", dtype=torch.float64) * span).to(torch.int64), span - 1)
m = plan[torch.arange(N, device="cuda")[:, None], u, 2].to(torch.int64)
moves = torch.stack([torch.where(odd, 2, 1).expand(N, Q), u, m], -1).to(torch.int32).contiguous()

res = dyn.decode_dyn(plan, moves, Q)
assert bool((res["status"] == 0).all()), "a benchmark candidate does not decode"
assert np.array_equal(dyn.decode_dyn(plan[:1].expand(N, cap, 3).contiguous(), None, 1, want_table=True)["table"][0, 0].cpu().numpy(), ep["table"]), \
    "the parent does not decode to the reference's table"
ref = DD.decode([a], parent[None], moves[:1].cpu().numpy(), Q)
assert np.array_equal(ref["objective"], res["objective"][:1].cpu().numpy()), "the kernel and the numpy statement differ"
assert bool((plain.decode(plan, moves, Q)["status"] == 0).all())

ts, calls = timed_in_turns([lambda: dyn.decode_dyn(plan, moves, Q), lambda: plain.decode(plan, moves, Q)])
ops = float(L) * N * Q
jobs16 = (int(np.asarray(a.count).sum()) + 15) // 16 * 16
for name, t, c, group, state in (("decode_dyn", ts[0], calls[0], dyn.decode_dyn_group(), 5 * jobs16 + 8 * a.M),
                                 ("decode (the same arrays as SO_DFJSP)", ts[1], calls[1], plain.decode_group(), 5 * jobs16 + 4 * a.M)):
    emit(what=name, instance=a.name, envs=N, neighbours=Q, candidates=N * Q, rows=cap, machines=int(a.M), windows=int(np.sum(a.bk_n)),
         group=group, lds_state_bytes_per_candidate=state, calls_per_region=c, regions=args.regions, seconds=spread(t),
         ops_per_second=spread([ops / x for x in t]))
emit(what="ratio decode_dyn / decode", seconds_median_ratio=float(np.median(ts[0]) / np.median(ts[1])))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for kw in lines:
        f.write(json.dumps(kw) + "\n")
