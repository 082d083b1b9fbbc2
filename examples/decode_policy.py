#!/usr/bin/env python3
"""Decode a trained PPO actor on generated SO_FJSSP 10x5 instances: mean makespan and wall time of the best fixed rule
pair per env, greedy play, best-of-16 and the policy lookahead (deep_reinforcement_learning_for_fjsp_amd.policy_search).

    python examples/decode_policy.py --rounds 5 [--envs 1024]           # train PPO for a few rounds first
    python examples/decode_policy.py --actor actor.pt                   # or load an ActorNet(20, 128, 2, 30) state dict
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5, help="PPO rounds to train when no --actor is given")
    ap.add_argument("--actor", default=None, help="state dict of an ActorNet(20, 128, 2, 30)")
    args = ap.parse_args()
    import torch
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.MPPPO import PPO, ActorNet
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    from deep_reinforcement_learning_for_fjsp_amd.environments import BatchedSOFJSSP
    from deep_reinforcement_learning_for_fjsp_amd.lookahead import ops_per_env

    N = args.envs
    if args.actor:
        actor = ActorNet(20, 128, 2, 30).cuda()
        actor.load_state_dict(torch.load(args.actor, map_location="cuda"))
    else:
        train = BatchedSOFJSSP(fi.InstanceSet(N).generate_range(1000, fi.bench_10x5_params()).solve_fluid(), rng_seed=7)
        torch.manual_seed(1234)
        agent = PPO(train, hidden_size=128, hidden_layer=2, seed=1, max_steps=56, use_graph=True, fused_sampling=True,
                    fused_rollout=True)
        for _ in range(args.rounds):
            agent.run_one_policy_network()
        actor = agent.learner.actor_new
    # held-out instances
    s = fi.InstanceSet(N).generate_range(900000, fi.bench_10x5_params()).solve_fluid()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    def report(name, makespan, seconds):
        print("%-22s mean makespan %8.2f   %8.3f s" % (name, float(makespan.double().mean()), seconds))

    pairs = [(a, m) for a in range(6) for m in range(5)]
    ev = EnvBatch(s, len(pairs) * N, rng_seed=3)
    ev.reset()
    T = int(ops_per_env(ev).max())
    acts = torch.tensor(pairs, dtype=torch.uint8, device="cuda")[:, None, :].expand(len(pairs), N, 2).reshape(1, -1, 2)
    _, sec = timed(lambda: ev.rollout(acts.expand(T, -1, 2).contiguous(), trace=False, rewards=False, state=False))
    report("best fixed rule pair", ev.read()["makespan"].reshape(len(pairs), N).min(0).values, sec)

    b = EnvBatch(s, N, rng_seed=3)
    b.reset()
    _, sec = timed(lambda: PS.play(b, actor))
    report("greedy", b.read()["makespan"], sec)
    b.reset()
    res, sec = timed(lambda: PS.best_of(b, actor, 16, "makespan", seed=1))
    report("best-of-16", res["objective"], sec)
    b.reset()
    res, sec = timed(lambda: PS.policy_lookahead(b, actor, "makespan"))
    report("policy lookahead", res["objective"], sec)


if __name__ == "__main__":
    main()
