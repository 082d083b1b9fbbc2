"""Recorded PPO rollouts on every collection path: tests/golden/ppo_rollout_paths.npz.

A PPO round collects a [T, N] rollout and hands it to PPOLearner.learn().  The collection runs one of three ways -- the
whole loop inside one launch, a captured HIP graph replayed, an eager loop of T vector steps -- with the action drawn by
torch or by the library's sampler, and keeps a buffer, a sampler, a log-probability table and a graph between rounds.
This file pins what each path hands to the learner and leaves behind, round after round, as recorded at commit
48b820983c274cbe340f3f1d5741352432f7e846, the last one at which the collection was written as `collect_and_learn`
over a dict of cached state.  tests/test_gpu_ppo_rollout_paths.py runs the same cases (cases() below) and compares.
Needs the GPU.

    python tests/golden/make_ppo_rollout_golden.py --commit <hash>          # (re)write ppo_rollout_paths.npz
    python tests/golden/make_ppo_rollout_golden.py --compare                # run the cases and check them against the file
    python tests/golden/make_ppo_rollout_golden.py --out a.npz --spread b.npz   # write a.npz, report how it differs from b.npz

The file in the tree was written at 48b8209 on an MI355X, and the maker was run there again in fresh processes
(--spread, then that case alone: six in all).  Eight cases came out byte-identical every time and are compared by digest, every key, no
tolerance.  The ninth, in_launch_refused, did not: one process of the six left other parameters (relative 1e-5 in the
actor, 1e-8 in the critic) and another actor loss (0.0421088 against 0.0421100) after round 3, the round in which the
learner's own captured graph is replayed for the first time on 2 x 64 networks; what the collection handed to learn() in
all three rounds, the buffer, the sampler, read() and rounds 1 and 2 were identical in all six.  That is the learner's
trainer, pinned by make_ppo_round_golden.py on the shapes it supports, not the collection, so UNPINNED leaves the case's
`param/*` keys and its losses out of the file; no tolerance is invented for them.

Every case drives the public agents only (PPO.run_one_policy_network, MPPPO.run_n_episodes) for several rounds, so the
caches, the graph's capture and replays and the sampler's round counter carry over.  What is recorded is taken where
learn() is called (wrapped through `patch`): the rollout is complete there.  Per round, each by SHA-256 plus an f64 sum
and largest magnitude (the keys of a case, in order, are in <case>_keys):
    learn/states, learn/actions, learn/old_log_prob, learn/returns     what learn() was called with, zeroed where
    learn/valid                                                        valid is 0 (what the kernels leave in the rows of
    memory/actions, memory/rewards, memory/dones, memory/next_states   finished environments is not a contract)
    sampler/flat_actions        the sampler's flat_actions[:len(memory)], where the path has a sampler
    read/<field>                every field of env.read(), status without its "stepped after done" bit (& ~4)
    param/<tensor>              every parameter tensor of the learner, after the round
Every row of the states, next states and log-probabilities, masked or not, must be finite.

Layout of ppo_rollout_paths.npz: commit, cases (their names) and per case, with R rounds and K keys
    <case>_keys     str[K]
    <case>_sha256   u8[R, K, 32]
    <case>_sum      f64[R, K]      } what makes a mismatch readable
    <case>_maxabs   f64[R, K]      }
    <case>_losses   f32[R, 2]      (critic loss, actor loss) learn() returned (where pinned)
    <case>_len      i64[R]         len(memory)
    <case>_made     i64[R, 2]      rollout buffers and samplers constructed so far (the remake rules)
No rows and no weights are stored.

150 environments of bench_10x5_params() (no multiple of 16: the last workgroup is partial), T = 56, 2 x 128 networks and
three rounds unless stated; 150 x ~50 samples stay below the fused trainer's threshold, so every learner is on the eager
trainer (the trainers are pinned by make_ppo_round_golden.py).  torch is seeded at the start of every case.  The cases:
    eager_torch        PPO(use_graph=False, fused_sampling=False): learner.act, torch's generator, the early exit
    eager_sampler      PPO(fused_sampling=True)
    graph_torch        PPO(use_graph=True): the exploration rate is a device scalar; warm-up, capture, replay
    graph_sampler      PPO(use_graph=True, fused_sampling=True)
    in_launch          PPO(use_graph=True, fused_rollout=True): fjsp_env_rollout_policy
    in_launch_orders   a generated 64-env SO_DFJSP handle with 1..3 orders per instance, max_steps=81, fused_rollout=True:
                       fjsp_env_rollout_policy_orders, through the segments
    in_launch_refused  PPO(hidden_size=64, fused_rollout=True, use_graph=True): the kernel refuses the actor, the round
                       falls to the graphed per-step loop
    regrown            eager_sampler with max_steps 40, 56, 56: the buffer is remade in round 2 and with it the sampler
                       and its round counter
    mpppo              MPPPO on 128 MO_FJSSP_discretes envs, 5 policies of 2 x 64, evolve_every=1, two epochs: one buffer
                       and one sampler serve five learners and a fresh env per epoch, the sampler's round counter runs
                       across the learners; recorded per learn() call, 10 in all
"""
import argparse
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests.golden.make_ppo_round_golden import _head, differences, patched, serialise      # noqa: E402

OUT = os.path.join(HERE, "ppo_rollout_paths.npz")
N, T = 150, 56
NETS = ("actor_new", "actor_old", "critic")
UNPINNED = {"in_launch_refused": ("param/", "losses")}     # case -> key prefixes the recorded commit does not reproduce (see above)


def _digest(a):
    a = np.ascontiguousarray(a)
    f = a.astype(np.float64)
    return (np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8), f.sum() if f.size else 0.0,
            np.abs(f).max() if f.size else 0.0)


class Recorder(object):
    """Wraps learn() of every learner of an agent and notes the buffers and samplers the agent constructs; every learn()
    call becomes one recorded round.  env: callable giving the environment of the round."""

    def __init__(self, torch, patch, case):
        from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO import Buffer, MPPPO as M
        self.torch, self.case = torch, case
        self.buffers, self.samplers, self.rounds = [], [], []
        for mod in (Buffer, M):                      # wherever the collection looks the buffer's class up
            if hasattr(mod, "RolloutBuffer"):
                patch(mod, "RolloutBuffer", self._noting(mod.RolloutBuffer, self.buffers))
        patch(M, "FusedSampler", self._noting(M.FusedSampler, self.samplers))

    @staticmethod
    def _noting(cls, made):
        class Noting(cls):
            def __init__(self, *a, **k):
                cls.__init__(self, *a, **k)
                made.append(self)
        Noting.__name__ = cls.__name__
        return Noting

    def watch(self, patch, learner, env, sampler=True):
        real = learner.learn

        def learn(states, actions, old_log_prob, returns, valid):
            entry = self._collected(env(), states, actions, old_log_prob, returns, valid, sampler)
            losses = real(states, actions, old_log_prob, returns, valid)
            self.torch.cuda.synchronize()
            for net in NETS:
                for name, p in getattr(learner, net).named_parameters():
                    entry["param/%s.%s" % (net, name)] = p.detach().cpu().numpy()
            self.rounds.append((entry, losses, len(self.buffers[-1]), (len(self.buffers), len(self.samplers))))
            return losses
        patch(learner, "learn", learn)

    def _collected(self, env, states, actions, old_log_prob, returns, valid, sampler):
        torch = self.torch
        memory = self.buffers[-1]
        n = len(memory)
        assert states.shape[0] == n and valid.shape == (n, env.N)
        assert all(bool(torch.isfinite(x).all()) for x in (states, memory.next_states[:n], old_log_prob))
        keep = lambda x: torch.where((valid if x.dim() == 2 else valid.unsqueeze(-1)) > 0, x, torch.zeros_like(x))
        entry = {"learn/states": keep(states), "learn/actions": keep(actions), "learn/old_log_prob": keep(old_log_prob),
                 "learn/returns": keep(returns), "learn/valid": valid}
        for name in ("actions", "rewards", "dones", "next_states"):
            entry["memory/" + name] = keep(getattr(memory, name)[:n])
        if sampler:
            entry["sampler/flat_actions"] = self.samplers[-1].flat_actions[:n]
        else:
            assert not self.samplers
        for k, v in env.read().items():
            entry["read/" + k] = (v & ~4) if k == "status" else v
        return {k: v.detach().cpu().numpy() for k, v in entry.items()}

    def arrays(self):
        """The file's arrays of the case."""
        keys = [k for k in self.rounds[0][0] if not k.startswith(UNPINNED.get(self.case, ()))]
        assert all(list(r[0]) == list(self.rounds[0][0]) for r in self.rounds)
        d = [[_digest(r[0][k]) for k in keys] for r in self.rounds]
        out = dict(keys=np.array(keys), sha256=np.array([[x[0] for x in row] for row in d], np.uint8),
                   sum=np.array([[x[1] for x in row] for row in d], np.float64),
                   maxabs=np.array([[x[2] for x in row] for row in d], np.float64),
                   losses=np.array([r[1] for r in self.rounds], np.float32), len=np.array([r[2] for r in self.rounds], np.int64),
                   made=np.array([r[3] for r in self.rounds], np.int64))
        if "losses" in UNPINNED.get(self.case, ()):
            del out["losses"]
        return out


def _so_env():
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd.environments import BatchedSOFJSSP
    return BatchedSOFJSSP(fi.InstanceSet(N).generate_range(3000, fi.bench_10x5_params()).solve_fluid(), rng_seed=9)


def _ppo(torch, patch, case, env=None, max_steps=(T, T, T), sampler=True, **kw):
    """PPO(**kw) on `env` for len(max_steps) rounds: (the file's arrays of the case, the agent)."""
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.MPPPO import PPO
    torch.manual_seed(0)
    rec = Recorder(torch, patch, case)
    env = env or _so_env()
    agent = PPO(env, hidden_size=kw.pop("hidden_size", 128), hidden_layer=2, seed=1, max_steps=max_steps[0], **kw)
    rec.watch(patch, agent.learner, lambda: env, sampler)
    for steps in max_steps:
        agent.max_steps = steps
        agent.run_one_policy_network()
    assert agent.memory is rec.buffers[-1] and len(rec.rounds) == len(max_steps)
    return rec.arrays(), agent


def _eager_torch(torch, patch):
    return _ppo(torch, patch, "eager_torch", sampler=False, use_graph=False, fused_sampling=False)


def _eager_sampler(torch, patch):
    return _ppo(torch, patch, "eager_sampler", fused_sampling=True)


def _graph_torch(torch, patch):
    return _ppo(torch, patch, "graph_torch", sampler=False, use_graph=True)


def _graph_sampler(torch, patch):
    return _ppo(torch, patch, "graph_sampler", use_graph=True, fused_sampling=True)


def _in_launch(torch, patch):
    return _ppo(torch, patch, "in_launch", use_graph=True, fused_rollout=True)


def _in_launch_orders(torch, patch):
    from deep_reinforcement_learning_for_fjsp_amd._capi import GenOrders, GenParams, GenRanges
    from deep_reinforcement_learning_for_fjsp_amd.environments import BatchedSODFJSP
    prm = GenParams(R_min=3, R_max=3, J_min=2, J_max=3, M=0, p_min=5, p_max=30, N_min=2, N_max=3, S=0, DDT=0.0,
                    t_si_min=100.0, t_si_max=200.0)
    env = BatchedSODFJSP(GenOrders(GenRanges(prm, 3, 6, 0.5, 1.5), 1, 3), n_envs=64, seed_base=900, rng_seed=3)
    assert env.batch.policy_orders_build(20)["segments"] == 3
    return _ppo(torch, patch, "in_launch_orders", env=env, max_steps=(81, 81, 81), fused_rollout=True)


def _in_launch_refused(torch, patch):
    return _ppo(torch, patch, "in_launch_refused", hidden_size=64, fused_rollout=True, use_graph=True)


def _regrown(torch, patch):
    got, agent = _ppo(torch, patch, "regrown", max_steps=(40, T, T), fused_sampling=True)
    assert got["made"].tolist() == [[1, 1], [2, 2], [2, 2]], got["made"]
    return got, agent


def _mpppo(torch, patch):
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd.environments import BatchedMOFJSSP
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.MPPPO import MPPPO
    torch.manual_seed(0)
    rec = Recorder(torch, patch, "mpppo")
    test_env = BatchedMOFJSSP(fi.InstanceSet(16).generate_range(5000, fi.bench_10x5_params()).solve_fluid(), rng_seed=1)
    envs = []

    def make_train_env():       # a fresh random batch per epoch
        s = fi.InstanceSet(128).generate_range(10000 * (len(envs) + 1), fi.bench_10x5_params()).solve_fluid()
        envs.append(BatchedMOFJSSP(s, rng_seed=len(envs) + 1))
        return envs[-1]

    agent = MPPPO(make_train_env, test_env, actor_number=5, hidden_size=64, hidden_layer=2, critic_layer=2, max_steps=T,
                  evolve_every=1)
    for learner in agent.learners.values():
        rec.watch(patch, learner, lambda: envs[-1])
    agent.run_n_episodes(2)
    got = rec.arrays()
    assert got["made"].tolist() == [[1, 1]] * 10, got["made"]
    return got, agent


def cases():
    """name -> callable(torch, patch) returning (the file's arrays of the case, its agent)."""
    return {"eager_torch": _eager_torch, "eager_sampler": _eager_sampler, "graph_torch": _graph_torch,
            "graph_sampler": _graph_sampler, "in_launch": _in_launch, "in_launch_orders": _in_launch_orders,
            "in_launch_refused": _in_launch_refused, "regrown": _regrown, "mpppo": _mpppo}


def learners(agent):
    return list(agent.learners.values()) if hasattr(agent, "learners") else [agent.learner]


def build(commit):
    import torch
    store = {"commit": np.array(commit), "cases": np.array(sorted(cases()))}
    for name, run in sorted(cases().items()):
        with patched() as patch:
            got, agent = run(torch, patch)
        assert all(ln.path == "eager" for ln in learners(agent)), name
        for k, v in got.items():
            store["%s_%s" % (name, k)] = v
        print("%-17s rounds %d  len %s  made %s" % (name, got["len"].shape[0], got["len"].tolist(), got["made"][-1].tolist()))
    return store


def of_case(keys, name):
    """Those of the file's keys that belong to case `name` (a case's name may begin with another's)."""
    return [k for k in keys if k.rsplit("_", 1)[0] == name]


def report(old, new, name):
    """The keys and rounds of a case that differ between two recordings, readably."""
    for what in ("losses", "len", "made"):
        if "%s_%s" % (name, what) in new and not np.array_equal(old["%s_%s" % (name, what)], new["%s_%s" % (name, what)]):
            print("  %s %s: %s vs %s" % (name, what, old["%s_%s" % (name, what)].tolist(), np.asarray(new["%s_%s" % (name, what)]).tolist()))
    keys = [str(k) for k in new[name + "_keys"]]
    if keys != [str(k) for k in old[name + "_keys"]]:
        print("  %s: other keys" % name)
        return
    for r, k in zip(*np.nonzero((old[name + "_sha256"] != new[name + "_sha256"]).any(-1))):
        print("  %s round %d %s: sum %.17g vs %.17g, max |.| %.17g vs %.17g"
              % (name, r + 1, keys[k], old[name + "_sum"][r, k], new[name + "_sum"][r, k], old[name + "_maxabs"][r, k],
                 new[name + "_maxabs"][r, k]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit the tree is at (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--compare", action="store_true", help="run the cases and check them against ppo_rollout_paths.npz")
    ap.add_argument("--spread", default=None, help="another recording: report the cases that differ from it and where")
    args = ap.parse_args()
    if args.compare:
        old = np.load(OUT, allow_pickle=False)
        new = build(str(old["commit"]))
        bad = differences(old, new)
        if bad:
            print("ppo_rollout_paths.npz DIFFERS from this tree's rollouts: %s" % ", ".join(bad))
            for name in sorted(cases()):
                if of_case(bad, name):
                    report(old, new, name)
            sys.exit(1)
        print("ppo_rollout_paths.npz (written at %s) holds this tree's rollouts" % str(old["commit"]))
        return
    commit = args.commit or _head()
    if not commit:
        sys.exit("--commit is needed: this tree is no git checkout")
    store = build(commit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "wb") as f:
        f.write(serialise(store))
    print("wrote %s at %s" % (args.out, commit))
    if args.spread:
        other = np.load(args.spread, allow_pickle=False)
        bad = differences(other, store)
        for name in sorted(cases()):
            if of_case(bad, name):
                print("SPREAD %s" % name)
                report(other, store, name)
        print("every case is byte-identical to %s" % args.spread if not bad else "DIFFERENT: %s" % ", ".join(bad))


if __name__ == "__main__":
    main()
