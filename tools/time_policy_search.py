"""Cost of decoding a policy on the device (policy_search): greedy play through play_policy_kernel and through the
per-step loop, best-of-16, and policy-lookahead decisions, next to the fused training rollout (rollout_policy_kernel)
for the same batch.

N generated SO_FJSSP 10x5 envs (256 instances), an ActorNet(20, 128, 2, 30) with seeded weights -- or, with --suite
NAME[:INSTANCE] (for example large:Brandimarte_Data/Mk10), N envs on the single-order instances of a fixture suite of
tests/golden (one of them with :INSTANCE), in the suite's variant and with the actor width that variant needs.  Every play
line carries path = "kernel" or "loop": what policy_search.play ran (it falls back to the per-step loop where the kernel
refuses).  Where it fell back, a suite run stops after the play lines: the searches on top would only repeat the loop.
--lookahead-envs runs the lookahead episode on a smaller batch (a 240-decision episode at 20 x 4096 branch envs takes
minutes).  Kernel times come
from device events around the launch (median of --reps, reset between repeats, not timed); whole calls that read back
on the host (play with its default step bound, the per-step loop, best_of, policy_lookahead) from a synchronised wall
clock.  policy_lookahead plays one whole episode with the 20 deterministic pairs and reports the mean seconds per
decision, split into its parts.  One JSON line per measurement, also written to --out.

--orders NAME times play alone, on a generated order-arrival batch (instances.reference_order_ranges(NAME), or NAME =
compact: small shops that fit sixteen to a workgroup) whose arrival LPs take the route FJSP_LP_IMPL names (unset, device,
global; exit status 3 where the handle does not admit the route): greedy and sampled, bounded at --steps, through the
segments of fjsp_env_play_policy_orders and with fused=False, --runs wall-clock times each, appended to --out.  --tree DIR
imports the package from another checkout -- the parent commit's, whose play is the per-step loop -- so that both trees
are timed alternately by one script; --tag names the tree in the lines.

    python tools/time_policy_search.py [--envs 4096] [--reps 20] [--suite NAME[:INSTANCE]] [--lookahead-envs N]
                                       [--out profiles/policy_search_timing.jsonl]
    python tools/time_policy_search.py --orders da3c [--steps 128] [--runs 5] [--tree PARENT --tag parent] --out FILE
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--loop-reps", type=int, default=3)
ap.add_argument("--suite", default=None, help="NAME[:INSTANCE] of tests/golden instead of the generated 10x5 set")
ap.add_argument("--lookahead-envs", type=int, default=None, help="envs of the lookahead episode (default: --envs)")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                              "policy_search_timing.jsonl"))
ap.add_argument("--orders", default=None, help="NAME: time play on a generated order-arrival batch of instances.reference_order_ranges(NAME), or of the small shops of NAME = compact")
ap.add_argument("--steps", type=int, default=128, help="--orders: the step bound of every timed play")
ap.add_argument("--runs", type=int, default=5, help="--orders: timed runs of every play")
ap.add_argument("--tag", default="head", help="--orders: what the lines call this tree (parent / head)")
ap.add_argument("--tree", default=None, help="import the package from this checkout (the parent commit's) instead of the tool's own")
args = ap.parse_args()

sys.path.insert(0, os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_reinforcement_learning_for_fjsp_amd import _capi  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd import instances as fi  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.MPPPO import ActorNet, native_actor_params  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd import batch as fb  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch  # noqa: E402
from deep_reinforcement_learning_for_fjsp_amd.lookahead import ACTION_RANGES, ops_per_env  # noqa: E402

DET_SO = [(a, b) for a in range(5) for b in range(4)]

N = args.envs
lines = []


def emit(**kw):
    kw.setdefault("envs", N)
    kw.update(gpu=torch.cuda.get_device_name(0))
    if args.suite:
        kw.update(suite=args.suite)
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


if args.orders:
    # An order-arrival batch, generated on the device; FJSP_LP_IMPL (unset / device / global) picks the LP route of its
    # arrival service at create.  play bounded at --steps steps from reset, greedy and sampled: as policy_search.play runs it
    # in the tree imported (the segments of fjsp_env_play_policy_orders; the per-step loop in a tree without them) and, where
    # that was not the loop already, with fused=False.  One line per play with the --runs wall-clock seconds, APPENDED to
    # --out: run it alternately with and without --tree PARENT_CHECKOUT.
    if args.orders == "compact":      # small shops that fit sixteen to a workgroup: 3 kinds x 2..3 stages x 2..3 jobs, 3..6 machines, 1..3 orders
        from deep_reinforcement_learning_for_fjsp_amd._capi import GenOrders, GenParams, GenRanges  # noqa: E402
        prm = GenParams(R_min=3, R_max=3, J_min=2, J_max=3, M=0, p_min=5, p_max=30, N_min=2, N_max=3, S=0, DDT=0.0, t_si_min=100.0,
                        t_si_max=200.0)
        ranges = GenOrders(GenRanges(prm, 3, 6, 0.5, 1.5), 1, 3)
    else:
        ranges = fi.reference_order_ranges(args.orders)
    b = EnvBatch.generated(ranges, N, 1000, rng_seed=1)
    torch.manual_seed(0)
    actor = ActorNet(b.state_size, 128, 2, 30).cuda()
    calls, _loop = [0], PS._play_loop

    def _counted(*a, **k):
        calls[0] += 1
        return _loop(*a, **k)

    PS._play_loop = _counted
    info = dict(orders=args.orders, tree=args.tag, lp_impl=os.environ.get("FJSP_LP_IMPL", ""), lp_on_device=b.lp_on_device, steps=args.steps)
    if hasattr(b, "policy_orders_build"):
        info["policy_orders_build"] = b.policy_orders_build(b.state_size)
    if info["lp_impl"] in ("device", "global") and not b.lp_on_device:
        emit(what="route_not_admitted", **info)               # (the handle keeps the host service: nothing new to time)
        sys.exit(3)
    for fused in ("segments", False):                          # (warm-up of both paths: library handles, the host service's LP memo)
        b.reset(); PS.play(b, actor, max_steps=args.steps, fused=fused)
    for what, kw in (("play_greedy", {}), ("play_sampled", dict(greedy=False, seed=3))):
        for fused in ("segments", False):                      # ("segments": also where play's default keeps the loop)
            mark, secs = calls[0], []
            for _ in range(args.runs):
                secs.append(wall_timed(b.reset, lambda: PS.play(b, actor, max_steps=args.steps, fused=fused, **kw), 1)[0])
            was_loop = calls[0] > mark
            emit(what=what, fused=bool(fused), path="loop" if was_loop else "segments", seconds=secs, mean_steps=float(b.read()["step_count"].double().mean()), **info)
            if was_loop:
                break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")
    sys.exit(0)

variant, mo = fb.VARIANT_SO_FJSSP, None
if args.suite:
    from tests import helpers as H  # noqa: E402
    suite, _, inst = args.suite.partition(":")
    variant = (fb.VARIANT_SO_SFJSP if suite in H.SF_SUITES else fb.VARIANT_MO_FJSSP_DISCRETES if suite in H.MO_SUITES else
               fb.VARIANT_SO_DFJSP if suite in H.SOD_SUITES else fb.VARIANT_SO_FJSSP)
    if suite in H.DYN_SUITES:
        sys.exit("--suite: the MO_DFJSP suites have order arrivals; nothing for the kernel to play")
    insts = [a for a in H.load_suite(suite)[0] if a.S == 1 and (not inst or a.name == inst)]
    if not insts:
        sys.exit("--suite: no single-order instance %r in suite %r" % (inst, suite))
    s = H.instance_set_from(insts)
else:
    s = fi.InstanceSet(256).generate_range(1000, fi.bench_10x5_params()).solve_fluid()
torch.manual_seed(0)
b = EnvBatch(s, N, variant=variant, rng_seed=1)
S, A = b.state_size, int(np.prod(ACTION_RANGES[variant]))
pair_div = ACTION_RANGES[variant][1] if len(ACTION_RANGES[variant]) == 2 else 0
actor = ActorNet(S, 128, 2, A).cuda()
if variant == fb.VARIANT_MO_FJSSP_DISCRETES:
    mo = torch.tensor([[0.5, 0.5, 800.0, 300.0]], dtype=torch.float64, device="cuda").repeat(N, 1)
T = int(ops_per_env(b).max().item())

# which path play took: its per-step loop counts its calls
loop_calls = [0]
_loop = PS._play_loop


def _counted_loop(*a, **k):
    loop_calls[0] += 1
    return _loop(*a, **k)


PS._play_loop = _counted_loop


def path_since(mark):
    return "loop" if loop_calls[0] > mark else "kernel"


geometry = {}
if hasattr(b, "policy_build"):
    try:
        geometry = dict(policy_build=b.policy_build(S))
    except _capi.FjspError:
        pass

# greedy play, kernel only (explicit step bound: no read-back), and the whole call
# (a batch the kernel refuses plays the per-step loop here: fewer repeats, it is a thousand times slower)
mark = loop_calls[0]
b.reset(); PS.play(b, actor, mo=mo, max_steps=T)
fell_back = path_since(mark) == "loop"
reps = args.loop_reps if fell_back else args.reps
mark = loop_calls[0]
med, lo, hi = event_timed(b.reset, lambda: PS.play(b, actor, mo=mo, max_steps=T), reps)
emit(what="play_greedy_kernel", steps=T, seconds_median=med, seconds_min=lo, seconds_max=hi, path=path_since(mark), **geometry)
mk_greedy = b.read()["makespan"].double().mean().item()
mark = loop_calls[0]
med, lo, hi, _ = wall_timed(b.reset, lambda: PS.play(b, actor, mo=mo), reps)
emit(what="play_greedy_call", seconds_median=med, seconds_min=lo, seconds_max=hi, mean_makespan=mk_greedy, path=path_since(mark))
mark = loop_calls[0]
med, lo, hi = event_timed(b.reset, lambda: PS.play(b, actor, mo=mo, greedy=False, seed=3, max_steps=T), reps)
emit(what="play_sampled_kernel", steps=T, seconds_median=med, seconds_min=lo, seconds_max=hi, path=path_since(mark))

# the same batch through the per-step loop (one actor launch, one env step and one read-back per step)
# (random.choice rules go on drawing across resets, so repeats of a greedy play need not end alike)
med, lo, hi, _ = wall_timed(b.reset, lambda: PS.play(b, actor, mo=mo, fused=False), args.loop_reps)
emit(what="play_greedy_per_step_loop", seconds_median=med, seconds_min=lo, seconds_max=hi, path="loop")


def write_out():
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")


if args.suite and fell_back:
    write_out()
    sys.exit(0)

# the fused training rollout of the same actor over 40 steps, buffer rows included (fjsp_env_rollout_policy)
lib = _capi.lib()
buf = C.c_void_p()
_capi.check(lib.fjsp_rollout_create(40, N, S, 0, C.byref(buf)))
p = _capi.ptr
eps = torch.zeros(1, dtype=torch.float32, device="cuda")
seed = torch.tensor([7], dtype=torch.int64, device="cuda")
flat = torch.zeros(40, N, dtype=torch.float32, device="cuda")
logp = torch.zeros(40, N, dtype=torch.float32, device="cuda")
st0 = torch.zeros(N, S, dtype=torch.float64, device="cuda")
apar = native_actor_params(actor)


def prep_rollout():
    st0.copy_(b.reset())


def rollout_policy():
    _capi.check(lib.fjsp_env_rollout_policy(b._h, buf, C.byref(apar), p(eps), p(seed), pair_div, 40, p(mo), p(st0), p(flat), p(logp),
                                            b._p_state, b._stream()))


med, lo, hi = event_timed(prep_rollout, rollout_policy, args.reps)
lib.fjsp_rollout_destroy(buf)
emit(what="rollout_policy_kernel_40_steps", steps=40, seconds_median=med, seconds_min=lo, seconds_max=hi)

# best-of-16: a 16 x N branch, block 0 greedy
branch = None


def run_best():
    global branch
    r = PS.best_of(b, actor, 16, "makespan", seed=5, mo=mo, branch=branch)
    branch = r["branch"]
    return r


b.reset(); branch = run_best()["branch"]                # (builds the branch batch once, outside the timing)
med, lo, hi, res = wall_timed(b.reset, run_best, args.loop_reps)
emit(what="best_of_16", seconds_median=med, seconds_min=lo, seconds_max=hi,
     mean_makespan=res["objective"].mean().item(), block0_wins=float((res["best"] == 0).double().mean().item()))
del branch

# policy lookahead: one whole episode, mean seconds per decision
NL = args.lookahead_envs or N
if NL != N:
    b = EnvBatch(s, NL, variant=variant, rng_seed=1)
    mo = None if mo is None else mo[:1].repeat(NL, 1)
cands = DET_SO if pair_div else list(range(A))
b.reset()
timings = {}
t0 = time.perf_counter()
res = PS.policy_lookahead(b, actor, "makespan", candidates=cands, mo=mo, timings=timings)
torch.cuda.synchronize()
total = time.perf_counter() - t0
D = int(res["steps"].max())
emit(what="policy_lookahead_decision", envs=NL, decisions=D, branch_envs=len(cands) * NL, seconds_per_decision=total / D,
     parts_per_decision={k: v / D for k, v in timings.items()}, mean_makespan=res["objective"].mean().item())

write_out()
