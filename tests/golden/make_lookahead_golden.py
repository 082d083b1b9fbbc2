"""Recorded choices of the two rollout lookaheads: tests/golden/lookahead_choices.npz.

The lookahead tests assert "never worse than the fixed policy" and "the returned actions replay to the objective"; a
change that picked another, equally good candidate would pass both.  This file pins the choices themselves: for a few
small cases it holds what lookahead.rollout_dispatch and policy_search.policy_lookahead returned -- the action applied
at every decision, the decisions each env took and the objective by bits -- at the commit named in it, and
tests/test_gpu_lookahead_choices.py runs the same cases (cases() below) and compares.  Needs the GPU.

    python tests/golden/make_lookahead_golden.py --commit <hash>     # (re)write lookahead_choices.npz
    python tests/golden/make_lookahead_golden.py --compare           # run the cases and check them against the file

--commit defaults to `git rev-parse HEAD` where the tree is a git checkout; --out writes somewhere else.

Layout of lookahead_choices.npz: commit (the commit the file was written at), cases (their names) and per case
    <case>_actions    u8[D, N, 2]  the action applied at decision d
    <case>_steps      i64[N]       decisions each env took
    <case>_objective  u64[N]       bits of the f64 objective of the finished episodes

The cases (every one a few seconds):
    rule_so_rows, rule_so_wave   rollout_dispatch on SO_FJSSP in both kernel families: 4 generated instances with 4
                                 different operation counts (envs finish at different decisions: the live / last
                                 masking), N = 8, four deterministic pairs plus (5, 4), both random.choice rules; the
                                 batch is first stepped 3 times with seeded actions, so the start is mid-episode
    rule_mo                      rollout_dispatch on MO_FJSSP_discretes, N = 2 x n_inst, four flat candidates,
                                 "tardiness", mo rows that differ per env (the order of the branch batch's repeat)
    policy_so                    policy_lookahead on SO_FJSSP, N = 8, candidates=None (all 30 actions), a callable
                                 objective, an actor of the in-kernel shape with parameters from numpy's RandomState
    policy_so_wrapper            the same through a Batched wrapper that carries `.mo` (the wrapper's mo is picked up)
    policy_mo_wrapper            policy_lookahead on MO_FJSSP_discretes through BatchedMOFJSSP with per-env objectives
"""
import argparse
import io
import os
import subprocess
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from tests import helpers as H  # noqa: E402

OUT = os.path.join(HERE, "lookahead_choices.npz")
SO_SEED = 4110                                        # generate_range seed of the 4 SO_FJSSP instances
SO_CANDIDATES = [(0, 0), (1, 2), (3, 1), (4, 3), (5, 4)]            # (5, 4): both random.choice rules
MO_CANDIDATES = [1, 4, 8, 16]                         # flat = task rule * 3 + machine rule; 16: the random task rule


def so_instances():
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    return fi.InstanceSet(4).generate_range(SO_SEED, fi.bench_10x5_params()).solve_fluid()


def operation_counts(s, n):
    out = []
    for i in range(n):
        a = s.arrays(i)
        out.append(int((np.asarray(a.count).reshape(a.S, a.R) * np.asarray(a.Jr)[None, :]).sum()))
    return out


def mo_instances():
    insts, _, _ = H.load_suite("mo_discretes")
    insts = [a for a in insts if a.S == 1 and a.K <= 64]        # what the in-kernel actor takes ...
    insts = [a for a in insts if int((a.count.reshape(a.S, a.R) * a.Jr[None, :]).sum()) <= 64]      # ... and short episodes
    return H.instance_set_from(insts), len(insts)


def mo_rows(torch, N):
    """f64[N, 4] = (w0, w1, completion, tardiness) with every row different."""
    i = torch.arange(N, dtype=torch.float64, device="cuda")
    w0 = (1.0 + i) / (N + 1.0)
    return torch.stack([w0, 1.0 - w0, 800.0 + 10.0 * i, 300.0 + 5.0 * i], 1).contiguous()


def actor(torch, S, A, seed):
    """An ActorNet of the in-kernel shape whose parameters come from numpy (not from torch's initialiser)."""
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.MPPPO import ActorNet
    net = ActorNet(S, 128, 2, A).cuda()
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.from_numpy((0.1 * rs.standard_normal(tuple(p.shape))).astype(np.float32)))
    return net


def weighted(r):
    return r["makespan"].double() + 0.25 * r["delay_time_sum"].double()


def _rule_so(torch, family):
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, global_actions
    from deep_reinforcement_learning_for_fjsp_amd.lookahead import rollout_dispatch
    s, N = so_instances(), 8
    assert len(set(operation_counts(s, 4))) == 4, "the instances must differ in their operation counts"
    b = EnvBatch(s, N, rng_seed=21, kernel_family=family)
    assert b.kernel_family == family
    b.reset()
    pre = torch.from_numpy(global_actions(5, 0, N, 3, 6, 5)).cuda()
    for t in range(3):
        b.step(pre[t])
    return rollout_dispatch(b, SO_CANDIDATES, "makespan")


def _rule_mo(torch):
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, VARIANT_MO_FJSSP_DISCRETES
    from deep_reinforcement_learning_for_fjsp_amd.lookahead import rollout_dispatch
    s, n_inst = mo_instances()
    N = 2 * n_inst
    b = EnvBatch(s, N, variant=VARIANT_MO_FJSSP_DISCRETES, rng_seed=22)
    b.reset()
    return rollout_dispatch(b, MO_CANDIDATES, "tardiness", mo=mo_rows(torch, N))


def _policy_so(torch, wrapper):
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    from deep_reinforcement_learning_for_fjsp_amd.environments.SO_FJSSP import BatchedSOFJSSP
    from deep_reinforcement_learning_for_fjsp_amd.policy_search import policy_lookahead
    s, N = so_instances(), 8
    if wrapper:
        b = BatchedSOFJSSP(s, N, rng_seed=23)
        b.mo = mo_rows(torch, N)
    else:
        b = EnvBatch(s, N, rng_seed=23)
    b.reset()
    return policy_lookahead(b, actor(torch, 20, 30, 31), weighted)


def _policy_mo_wrapper(torch):
    from deep_reinforcement_learning_for_fjsp_amd.environments.MO_FJSSP_discretes import BatchedMOFJSSP
    from deep_reinforcement_learning_for_fjsp_amd.policy_search import policy_lookahead
    s, n_inst = mo_instances()
    N = 2 * n_inst
    b = BatchedMOFJSSP(s, N, rng_seed=24)
    b.mo.copy_(mo_rows(torch, N))
    b.reset()
    return policy_lookahead(b, actor(torch, 25, 18, 32), "tardiness", candidates=MO_CANDIDATES)


def cases():
    """name -> callable(torch) returning the lookahead's dict."""
    return {"rule_so_wave": lambda torch: _rule_so(torch, 0), "rule_so_rows": lambda torch: _rule_so(torch, 1),
            "rule_mo": _rule_mo, "policy_so": lambda torch: _policy_so(torch, False),
            "policy_so_wrapper": lambda torch: _policy_so(torch, True), "policy_mo_wrapper": _policy_mo_wrapper}


def outcome(res):
    """What the file keeps of a lookahead's result."""
    return dict(actions=np.ascontiguousarray(res["actions"], np.uint8), steps=np.asarray(res["steps"], np.int64),
                objective=H.bits(res["objective"].cpu().numpy()))


def build(commit):
    import torch
    store = {"commit": np.array(commit), "cases": np.array(sorted(cases()))}
    for name, run in sorted(cases().items()):
        got = outcome(run(torch))
        for k, v in got.items():
            store["%s_%s" % (name, k)] = v
        print("%-18s decisions %3d  steps %s  distinct actions %d" % (name, got["actions"].shape[0], got["steps"].tolist(),
                                                                       len(np.unique(got["actions"].reshape(-1, 2), axis=0))))
    return store


def serialise(store):
    """npz bytes with fixed member timestamps and order (np.savez stamps the current time: not reproducible)."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(store):
            arr = io.BytesIO()
            np.lib.format.write_array(arr, np.asanyarray(store[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, arr.getvalue())
    return buf.getvalue()


def _head():
    try:
        return subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=REPO, stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit the tree is at (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--compare", action="store_true", help="run the cases and check them against lookahead_choices.npz")
    args = ap.parse_args()
    if args.compare:
        old = np.load(OUT, allow_pickle=False)
        new = build(str(old["commit"]))
        bad = [k for k in sorted(new) if k not in old.files or not np.array_equal(old[k], new[k])]
        bad += [k for k in old.files if k not in new]
        if bad:
            print("lookahead_choices.npz DIFFERS from this tree's choices: %s" % ", ".join(bad))
            sys.exit(1)
        print("lookahead_choices.npz (written at %s) holds this tree's choices" % str(old["commit"]))
        return
    commit = args.commit or _head()
    if not commit:
        sys.exit("--commit is needed: this tree is no git checkout")
    store = build(commit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "wb") as f:
        f.write(serialise(store))
    print("wrote %s at %s" % (args.out, commit))


if __name__ == "__main__":
    main()
