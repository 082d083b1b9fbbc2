"""Recorded learning rounds of PPOLearner on every trainer path: tests/golden/ppo_round_paths.npz.

The learner's round (advantages from the critic before the round, n critic and n actor iterations, equalise_policies)
runs through several launch sequences: two chains on two streams, one stream, library GEMMs, gradient reduction
between pass and step, an untrained critic, a replayed HIP graph, eager autograd.  This file pins what each of them
computes -- the two losses of every round and a digest of every parameter tensor after every round -- as recorded at
commit d9f633ef091b1abeea37b74a7b9e25b563d678b2, the last one at which PPOLearner wrote the round five times in one
function.  tests/test_gpu_ppo_round_paths.py runs the same cases (cases() below) and compares.  Needs the GPU.

    python tests/golden/make_ppo_round_golden.py --commit <hash>          # (re)write ppo_round_paths.npz
    python tests/golden/make_ppo_round_golden.py --compare                # run the cases and check them against the file
    python tests/golden/make_ppo_round_golden.py --out a.npz --spread b.npz   # write a.npz, report how it differs from b.npz

The file in the tree was written at d9f633e on an MI355X.  The maker was then run again there in a fresh process
(--spread): every case came out byte-identical, the two files are equal byte for byte, so every case is compared by
digest and none needs a tolerance.

Layout of ppo_round_paths.npz: commit, cases (their names), tensors (the names of the P = 18 parameter tensors, in
the order of the digests) and per case, with R rounds
    <case>_losses   f32[R, 2]      (critic loss, actor loss) learn() returned
    <case>_sha256   u8[R, P, 32]   SHA-256 of each parameter tensor's bytes after the round
    <case>_sum      f64[R, P]      its f64 sum   } what makes a mismatch readable
    <case>_maxabs   f64[R, P]      its max |.|   }
No weights are stored.

Inputs come from a CPU torch.Generator (seed per case and round) and move to the GPU; S = 20, A = 30, 2 x 128 networks,
32 775 valid samples (just over the fused threshold, no multiple of the one-launch pass's 32-sample tile) and two rounds
(so Adam moments and step counts carry over) unless stated.  The cases:
    two_chains        the default learner: critic and actor chains on two streams
    one_stream        two_chains = False
    library_gemm      mfma_learn = False: forward, loss, backward and step as separate launches
    critic_untrained  train_critic=False (the critic's parameters must not move)
    reduced           the distributed round on ONE process: distributed.is_distributed patched to True and
                      torch.distributed.all_reduce to a recorder that leaves its argument alone (see reduced_calls())
    graphed           graph_learn = True: rounds 1-3 of one sample count (eager, capture, replay), round 4 of 33 000
                      samples (back to eager)
    ragged            a [T, N] = [56, 900] call with valid[t, e] = t < len_e, len_e cycling over 30..56: the row dropping
    eager_gpu         fused_learn = False, 2 000 rows of which a quarter is invalid: masked autograd arithmetic on the GPU
    fused_then_small  two_chains' two rounds, then one all-valid batch of 2 000: the learner stays on the fused trainer
"""
import argparse
import hashlib
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

OUT = os.path.join(HERE, "ppo_round_paths.npz")
S, A, N_FUSED = 20, 30, 32775
NETS = ("actor_new", "actor_old", "critic")


def samples(torch, seed, n):
    """(states, actions, old log-probabilities, returns) of n samples from a CPU generator, on the GPU."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    states = torch.randn(n, S, generator=g)
    actions = torch.randint(0, A, (n,), generator=g)
    old_lp = -torch.rand(n, generator=g) * 3 - 0.2
    returns = torch.randn(n, generator=g)
    return tuple(t.cuda() for t in (states, actions, old_lp, returns))


def learner(**kw):
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.MPPPO import PPOLearner
    return PPOLearner(S, A, 128, 2, 2, device="cuda", seed=17, **kw)


def tensor_names(L):
    return ["%s.%s" % (net, name) for net in NETS for name, _ in getattr(L, net).named_parameters()]


def digest(torch, L):
    """(sha256 u8[P, 32], f64 sum [P], max |.| [P]) of the learner's parameter tensors."""
    torch.cuda.synchronize()
    sha, tot, big = [], [], []
    for net in NETS:
        for _, p in getattr(L, net).named_parameters():
            a = np.ascontiguousarray(p.detach().cpu().numpy())
            sha.append(np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8))
            tot.append(a.astype(np.float64).sum())
            big.append(np.abs(a.astype(np.float64)).max())
    return np.stack(sha), np.array(tot, np.float64), np.array(big, np.float64)


def rounds(torch, L, batches):
    """learn() on every batch (states, actions, old_lp, returns, valid): (the file's four arrays, the learner)."""
    losses, sha, tot, big = [], [], [], []
    for b in batches:
        losses.append(L.learn(*b))
        d = digest(torch, L)
        sha.append(d[0]); tot.append(d[1]); big.append(d[2])
    return dict(losses=np.array(losses, np.float32), sha256=np.stack(sha), sum=np.stack(tot), maxabs=np.stack(big)), L


def flat_batches(torch, seed, sizes):
    out = []
    for r, n in enumerate(sizes):
        out.append(samples(torch, seed + r, n) + (torch.ones(n, device="cuda"),))
    return out


def _two_chains(torch, patch):
    return rounds(torch, learner(), flat_batches(torch, 100, (N_FUSED, N_FUSED)))


def _one_stream(torch, patch):
    L = learner()
    L.two_chains = False
    return rounds(torch, L, flat_batches(torch, 100, (N_FUSED, N_FUSED)))


def _library_gemm(torch, patch):
    L = learner()
    L.mfma_learn = False
    return rounds(torch, L, flat_batches(torch, 100, (N_FUSED, N_FUSED)))


def _critic_untrained(torch, patch):
    L = learner(train_critic=False)
    before = digest(torch, L)[0]
    got, _ = rounds(torch, L, flat_batches(torch, 100, (N_FUSED, N_FUSED)))
    critic = [i for i, name in enumerate(tensor_names(L)) if name.startswith("critic.")]
    assert np.array_equal(got["sha256"][-1][critic], before[critic]), "train_critic=False moved the critic"
    return got, L


def reduced_calls(torch, patch, seed):
    """The `reduced` case with data seed `seed`: (the file's arrays, the learner, numel of every all_reduce in call
    order, (critic numel, actor numel), iterations).  `patch(object, name, value)` is monkeypatch.setattr or patched() below."""
    from deep_reinforcement_learning_for_fjsp_amd import distributed as fdist
    calls = []
    patch(fdist, "is_distributed", lambda: True)
    patch(torch.distributed, "all_reduce", lambda t, op=None, **kw: calls.append(int(t.numel())))
    L = learner()
    got, _ = rounds(torch, L, flat_batches(torch, seed, (N_FUSED, N_FUSED)))
    sizes = tuple(sum(p.numel() for p in getattr(L, net).parameters()) for net in ("critic", "actor_new"))
    return got, L, calls, sizes, L.hp["learning_iterations_per_round_critic"]


def check_reduced_calls(calls, sizes, n):
    """Round 1: the two scalar reductions (smallest sample count, global sample count), then n critic-sized and n
    actor-sized ones in whatever order; round 2: the global sample count, then the same 2 n."""
    assert len(calls) == 3 + 4 * n, calls
    first, second = calls[:2 + 2 * n], calls[2 + 2 * n:]
    assert first[:2] == [1, 1] and second[:1] == [1], calls
    want = sorted([sizes[0]] * n + [sizes[1]] * n)
    assert sorted(first[2:]) == want and sorted(second[1:]) == want, calls


def _reduced(torch, patch):
    got, L, calls, sizes, n = reduced_calls(torch, patch, 100)
    check_reduced_calls(calls, sizes, n)
    assert reduced_calls(torch, patch, 300)[2] == calls, "the sequence of reductions depends on the data"
    return got, L


def _graphed(torch, patch):
    L = learner()
    L.graph_learn = True
    return rounds(torch, L, flat_batches(torch, 100, (N_FUSED, N_FUSED, N_FUSED, 33000)))


def _ragged(torch, patch):
    T, N = 56, 900
    length = 30 + torch.arange(N) % 27                                       # 30 .. 56
    valid = (torch.arange(T)[:, None] < length[None, :]).to(torch.float32)
    assert int(valid.sum()) >= (1 << 15)
    batches = []
    for r in range(2):
        st, ac, lp, ret = samples(torch, 500 + r, T * N)
        batches.append((st.reshape(T, N, S), ac.reshape(T, N), lp.reshape(T, N), ret.reshape(T, N), valid.cuda()))
    return rounds(torch, learner(), batches)


def _eager_gpu(torch, patch):
    L = learner()
    L.fused_learn = False
    n = 2000
    valid = (torch.arange(n) % 4 != 3).to(torch.float32).cuda()
    got, _ = rounds(torch, L, [samples(torch, 700 + r, n) + (valid,) for r in range(2)])
    assert len(L.actor_optimizer.state) > 0
    return got, L


def _fused_then_small(torch, patch):
    L = learner()
    got, _ = rounds(torch, L, flat_batches(torch, 100, (N_FUSED, N_FUSED)) + flat_batches(torch, 900, (2000,)))
    assert len(L.actor_optimizer.state) == 0 and len(L.critic_optimizer.state) == 0
    return got, L


def cases():
    """name -> callable(torch, patch) returning (the file's arrays of the case, its learner)."""
    return {"two_chains": _two_chains, "one_stream": _one_stream, "library_gemm": _library_gemm,
            "critic_untrained": _critic_untrained, "reduced": _reduced, "graphed": _graphed, "ragged": _ragged,
            "eager_gpu": _eager_gpu, "fused_then_small": _fused_then_small}


class patched(object):
    """setattr that is undone on exit (what pytest's monkeypatch does in the test)."""

    def __init__(self):
        self.undo = []

    def __call__(self, obj, name, value):
        self.undo.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for obj, name, value in reversed(self.undo):
            setattr(obj, name, value)


def build(commit):
    import torch
    store = {"commit": np.array(commit), "cases": np.array(sorted(cases())), "tensors": np.array(tensor_names(learner()))}
    for name, run in sorted(cases().items()):
        with patched() as patch:
            got, _ = run(torch, patch)
        for k, v in got.items():
            store["%s_%s" % (name, k)] = v
        print("%-17s rounds %d  losses %s" % (name, got["losses"].shape[0], got["losses"].tolist()))
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


def differences(old, new):
    """Keys of two recordings that differ."""
    bad = [k for k in sorted(new) if k not in old.files or not np.array_equal(old[k], np.asanyarray(new[k]))]
    return bad + [k for k in old.files if k not in new]


def _head():
    try:
        return subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=REPO, stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit the tree is at (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--compare", action="store_true", help="run the cases and check them against ppo_round_paths.npz")
    ap.add_argument("--spread", default=None, help="another recording: report the cases that differ from it and by how much")
    args = ap.parse_args()
    if args.compare:
        old = np.load(OUT, allow_pickle=False)
        bad = differences(old, build(str(old["commit"])))
        if bad:
            print("ppo_round_paths.npz DIFFERS from this tree's rounds: %s" % ", ".join(bad))
            sys.exit(1)
        print("ppo_round_paths.npz (written at %s) holds this tree's rounds" % str(old["commit"]))
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
            if any(k.startswith(name + "_") for k in bad):
                print("SPREAD %s: max |sum difference| %.3e, max |loss difference| %.3e"
                      % (name, np.abs(other[name + "_sum"] - store[name + "_sum"]).max(),
                         np.abs(other[name + "_losses"] - store[name + "_losses"]).max()))
        print("every case is byte-identical to %s" % args.spread if not bad else "DIFFERENT: %s" % ", ".join(bad))


if __name__ == "__main__":
    main()
