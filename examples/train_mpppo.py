#!/usr/bin/env python3
"""agents/MPPPO/MPPPO.py of the reference, batched: five policies with weight vectors (1,0) .. (0,1) on
MO_FJSSP_discretes environments (makespan + tardiness), a fresh batch of random instances per epoch
(generated_new_environment, MPPPO.py:149-154), the single-objective policies' results normalising the
rewards of the weighted ones (:159-164), periodic evolution towards the best policy per weight vector
(:192-205).

    python examples/train_mpppo.py --envs 1024 --epochs 3
    python examples/train_mpppo.py --envs 1024 --epochs 3 --device-instances    # one env, refilled on the device per epoch
    python examples/train_mpppo.py --envs 256 --epochs 1 --device-instances --reference-distribution

The default training instances are 10 kinds x 1 job on 5 machines.  --reference-distribution draws them as the reference's
loop does (instances.reference_training_ranges("mpppo"): 3-12 kinds of 5-50 jobs, and per instance 10-20 machines and a
due-date tightness in [0.5, 1.5]), on either path; an episode then has up to 3 000 operations.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--device-instances", action="store_true",
                    help="keep one training env and regenerate its instances (and their fluid LPs) on the device every epoch, "
                         "instead of a new InstanceSet + env per epoch; the instances are the same")
    ap.add_argument("--reference-distribution", action="store_true",
                    help="training instances from the reference's distribution (M 10-20 and DDT 0.5-1.5 drawn per instance) "
                         "instead of 10x5 shops with M = 5")
    args = ap.parse_args()
    import torch
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd.environments import BatchedMOFJSSP
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.MPPPO import MPPPO

    test_env = BatchedMOFJSSP(fi.InstanceSet(64).generate_range(900000, fi.bench_10x5_params()).solve_fluid(), rng_seed=1)
    prm = fi.reference_training_ranges("mpppo") if args.reference_distribution else fi.bench_10x5_params()
    # a rollout holds a whole episode: the operations of the largest instance the parameters can make
    max_steps = prm.base.R_max * prm.base.J_max * prm.base.N_max if args.reference_distribution else 56
    epoch = [0]

    live = []

    def make_train_env():
        epoch[0] += 1
        if args.device_instances:
            if not live:
                live.append(BatchedMOFJSSP(prm, args.envs, seed_base=10_000_000 * epoch[0], rng_seed=epoch[0]))
            else:
                live[0].batch.regenerate(10_000_000 * epoch[0], rng_seed=epoch[0])
            return live[0]
        s = fi.InstanceSet(args.envs).generate_range(10_000_000 * epoch[0], prm).solve_fluid()
        return BatchedMOFJSSP(s, rng_seed=epoch[0])

    torch.manual_seed(0)
    agent = MPPPO(make_train_env, test_env, actor_number=5, hidden_size=200, hidden_layer=5, critic_layer=3, max_steps=max_steps,
                  evolve_every=2)
    agent.run_n_episodes(1)                      # warm-up epoch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hist = agent.run_n_episodes(args.epochs)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"workload": "MPPPO, 5 policies, %d MO_FJSSP_discretes %s envs per epoch" % (args.envs, "reference-distribution" if args.reference_distribution else "10x5"),
                      "epochs": args.epochs, "device_instances": bool(args.device_instances), "s_per_epoch": dt / args.epochs,
                      "test_objectives_last_epoch": {str(p): {"completion_time": c, "tardiness": t} for p, (c, t) in hist[-1].items()},
                      "completion_min": agent.completion_min, "tardiness_min": agent.tardiness_min}))


if __name__ == "__main__":
    main()
