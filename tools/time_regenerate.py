#!/usr/bin/env python3
"""What a training loop spends on the NEXT batch of instances: the host path against a regenerate on the device.

    python tools/time_regenerate.py [--reps 5] [--out profiles/regenerate_timing.jsonl] [--ranges mpppo|ddqn] [--orders da3c|hmpsac]
                                    [--dynamic] [--envs 4096] [--lp-impl host|device|global] [--masked FRACTION]

For 4096 and 32768 bench_10x5_params instances and 4096 of reference_generator_params(1.0, 10, 1), alternately in one
process, wall clock between device synchronisations:
  (a) InstanceSet(N).generate_range(s, prm).solve_fluid() on 16 threads, EnvBatch(...), up to a finished reset();
  (b) regenerate(s) + reset() on a live EnvBatch.generated handle.
Each repetition uses seeds of its own (the same for (a) and (b)).  Prints one JSON line per (workload, path) with every
repetition, median [min, max], and for (b) the library's own split (generated_stats()["ms"], medians) and LP routes.
--ranges NAME times instances.reference_training_ranges(NAME) instead (M and DDT drawn per instance), --envs of them;
--orders NAME times instances.reference_order_ranges(NAME) (the number of orders drawn too: a multi-order handle; the
reset alone plays no order arrival, so the arrival service is not in the figure); --dynamic times MO_DFJSP batches of
instances.reference_dynamic_ranges("hmpsac") (machine data generated too), and its host path (a) is the route
examples/train_hmpsac.py's make_train_env runs without --generated: a Python loop per instance with its redraw loop, NumPy
machine data, solve_fluid, a new BatchedMODFJSP; --envs alone times that many 10x5 instances.  --lp-impl sets FJSP_LP_IMPL around the create of the live handle (the
library reads it there and nowhere else) and is recorded in the device line.  --masked FRACTION times (b) as
regenerate_masked(s, mask) + reset(mask) instead, over that share of the instances -- round(FRACTION x N) of them at a fixed
stride -- with the same split; the host path (a) has no such call and is not run.
"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


@contextlib.contextmanager
def lp_impl(value):
    """FJSP_LP_IMPL = value around a create (None: left as it is)."""
    old = os.environ.get("FJSP_LP_IMPL")
    if value is not None:
        os.environ["FJSP_LP_IMPL"] = value
    try:
        yield
    finally:
        if value is not None:
            if old is None:
                del os.environ["FJSP_LP_IMPL"]
            else:
                os.environ["FJSP_LP_IMPL"] = old


def hmpsac_host_route(fi, prm, n, seed_base):
    """examples/train_hmpsac.py's make_train_env without --generated, on the parameters instance seed draws under prm.o."""
    from deep_reinforcement_learning_for_fjsp_amd.environments import BatchedMODFJSP
    s = fi.InstanceSet(n)
    for i in range(n):
        seed = seed_base + i
        p = fi.draw_params(prm.o, seed)
        s.generate(i, seed, p)
        while not (s.arrays(i).p > 0).any(axis=0).all():
            seed += 7919
            s.generate(i, seed, p)
        s.generate_machine_data(i, seed, max_windows=prm.m.W_max, window_gap=(prm.m.gap_min, prm.m.gap_max), window_len=(prm.m.len_min, prm.m.len_max))
    return BatchedMODFJSP(s.solve_fluid(n_threads=16), rng_seed=1).batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--ranges", choices=("mpppo", "ddqn"), default=None, help="the reference's training distribution instead of the three workloads")
    ap.add_argument("--orders", choices=("da3c", "hmpsac"), default=None, help="the reference's multi-order training distribution instead")
    ap.add_argument("--dynamic", action="store_true", help="MO_DFJSP batches of reference_dynamic_ranges('hmpsac') against make_train_env's host route")
    ap.add_argument("--envs", type=int, default=None, help="instances of the --ranges / --orders workload (4096), or of a single 10x5 workload")
    ap.add_argument("--lp-impl", choices=("host", "device", "global"), default=None, help="FJSP_LP_IMPL of the live handle (default: not set)")
    ap.add_argument("--masked", type=float, default=None, metavar="FRACTION", help="time regenerate_masked + reset(mask) over this share of the instances (0 < FRACTION <= 1)")
    args = ap.parse_args()
    if args.masked is not None and not 0.0 < args.masked <= 1.0:
        ap.error("--masked takes a share of the instances in (0, 1]")
    import torch
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, VARIANT_MO_DFJSP, VARIANT_SO_FJSSP

    workloads = [("10x5", fi.bench_10x5_params(), 4096), ("10x5", fi.bench_10x5_params(), 32768),
                 ("reference M=10", fi.reference_generator_params(1.0, 10, 1), 4096)]
    if sum(1 for x in (args.ranges, args.orders, args.dynamic) if x) > 1:
        ap.error("--ranges, --orders and --dynamic are three workloads: give one")
    if args.dynamic:
        workloads = [("dynamic hmpsac", fi.reference_dynamic_ranges("hmpsac"), args.envs or 4096)]
    elif args.orders:
        workloads = [("orders " + args.orders, fi.reference_order_ranges(args.orders), args.envs or 4096)]
    elif args.ranges:
        workloads = [("ranges " + args.ranges, fi.reference_training_ranges(args.ranges), args.envs or 4096)]
    elif args.envs:
        workloads = [("10x5", fi.bench_10x5_params(), args.envs)]
    lines = []
    for name, prm, N in workloads:
        with lp_impl(args.lp_impl):
            live = EnvBatch.generated(prm, N, 1, variant=VARIANT_MO_DFJSP if args.dynamic else VARIANT_SO_FJSSP)
        live.reset()
        torch.cuda.synchronize()
        host_ms, dev_ms, parts, routes = [], [], [], None
        mask = None
        if args.masked is not None:
            k = max(1, int(round(args.masked * N)))
            mask = torch.zeros(N, dtype=torch.uint8, device=live.device)
            mask[torch.div(torch.arange(k, device=live.device) * N, k, rounding_mode="floor")] = 1
        for rep in range(args.reps):
            seed = 1_000_000 * (rep + 1)
            torch.cuda.synchronize()
            if mask is not None:
                t0 = time.perf_counter()
                live.regenerate_masked(seed, mask)
                live.reset(mask)
                torch.cuda.synchronize()
                dev_ms.append((time.perf_counter() - t0) * 1e3)
                st = live.generated_stats()
                assert st["instances"] == int(mask.sum()), st
                parts.append(st["ms"])
                routes = dict(refreshed=st["instances"], lp_device=st["lp_device"], lp_host=st["lp_host"], lp_global=st["lp_global"],
                              device_pivots=st["device_pivots"], global_pivots=st["global_pivots"])
                continue
            t0 = time.perf_counter()
            if args.dynamic:
                s, b = None, hmpsac_host_route(fi, prm, N, seed)
            else:
                s = fi.InstanceSet(N).generate_range(seed, prm).solve_fluid(n_threads=16)
                b = EnvBatch(s, N)
            b.reset()
            torch.cuda.synchronize()
            host_ms.append((time.perf_counter() - t0) * 1e3)
            del b, s
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            live.regenerate(seed)
            live.reset()
            torch.cuda.synchronize()
            dev_ms.append((time.perf_counter() - t0) * 1e3)
            st = live.generated_stats()
            parts.append(st["ms"])
            routes = dict(lp_device=st["lp_device"], lp_host=st["lp_host"], lp_global=st["lp_global"], device_pivots=st["device_pivots"],
                          global_pivots=st["global_pivots"])
        split = {k: statistics.median(p[k] for p in parts) for k in parts[0]}
        if mask is not None:
            lines.append(dict(workload=name, instances=N, path="device: regenerate_masked + reset(mask)", masked=args.masked, lp_impl=args.lp_impl,
                              ms=dev_ms, split_ms_median=split, **routes, **summary(dev_ms)))
            del live
            continue
        lines.append(dict(workload=name, instances=N, path="host: make_train_env's loop (generate, redraw, NumPy machine data) + solve_fluid(16 threads) + BatchedMODFJSP + reset"
                          if args.dynamic else "host: generate_range + solve_fluid(16 threads) + EnvBatch + reset",
                          ms=host_ms, **summary(host_ms)))
        lines.append(dict(workload=name, instances=N, path="device: regenerate + reset", lp_impl=args.lp_impl, ms=dev_ms, split_ms_median=split,
                          **routes, **summary(dev_ms)))
        del live
    for ln in lines:
        print(json.dumps(ln))
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
