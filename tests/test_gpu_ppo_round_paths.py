"""GPU: PPOLearner's learning round on every trainer path against a recording (tests/golden/ppo_round_paths.npz).

The file was written by tests/golden/make_ppo_round_golden.py at commit d9f633ef091b1abeea37b74a7b9e25b563d678b2, the
last one at which the learner wrote its round once per launch sequence.  Every case of that module runs again here; the
losses of every round and the SHA-256 of every parameter tensor after every round must equal the file's (the f64 sums
and largest magnitudes it also holds are there to make a mismatch readable)."""
import os

import numpy as np
import pytest

from tests import helpers as H
from tests.golden import make_ppo_round_golden as G

pytestmark = pytest.mark.gpu

COMMIT = "d9f633ef091b1abeea37b74a7b9e25b563d678b2"
CASES = {"two_chains": "fused", "one_stream": "fused", "library_gemm": "fused", "critic_untrained": "fused", "reduced": "fused",
         "graphed": "fused", "ragged": "fused", "eager_gpu": "eager", "fused_then_small": "fused"}      # case -> learner.path


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(H.GOLDEN, "ppo_round_paths.npz"), allow_pickle=False)


def test_the_file_holds_every_case(golden):
    assert tuple(sorted(CASES)) == tuple(sorted(G.cases())) == tuple(str(c) for c in golden["cases"])
    assert str(golden["commit"]) == COMMIT


@pytest.mark.parametrize("case", sorted(CASES))
def test_rounds_are_the_recorded_ones(torch_gpu, golden, monkeypatch, case):
    got, learner = G.cases()[case](torch_gpu, monkeypatch.setattr)
    names = [str(t) for t in golden["tensors"]]
    assert names == G.tensor_names(learner)
    assert learner.path == CASES[case]
    for key in ("losses", "sha256", "sum", "maxabs"):
        assert got[key].dtype == golden["%s_%s" % (case, key)].dtype and got[key].shape == golden["%s_%s" % (case, key)].shape, key
    want_sum, want_big = golden[case + "_sum"], golden[case + "_maxabs"]
    for r, p in zip(*np.nonzero((got["sha256"] != golden[case + "_sha256"]).any(-1))):
        pytest.fail("%s: %s after round %d differs: sum %.17g (recorded %.17g), max |.| %.17g (recorded %.17g)"
                    % (case, names[p], r + 1, got["sum"][r, p], want_sum[r, p], got["maxabs"][r, p], want_big[r, p]))
    assert np.array_equal(got["losses"], golden[case + "_losses"]), (got["losses"], golden[case + "_losses"])
    assert np.array_equal(got["sum"], want_sum) and np.array_equal(got["maxabs"], want_big)


def test_a_fused_learner_never_trains_on_invalid_rows(torch_gpu):
    """A learner on the fused trainer gets a batch below the size at which learn() used to drop the rows of finished
    environments: 2 000 rows, 500 of them invalid.  Its parameters equal, bit for bit, those of an identically built and
    warmed learner that is given the 1 500 valid rows only."""
    torch = torch_gpu
    warm = G.flat_batches(torch, 100, (G.N_FUSED,))[0]
    states, actions, old_lp, returns = G.samples(torch, 1100, 2000)
    valid = (torch.arange(2000, device="cuda") % 4 != 1).to(torch.float32)
    keep = valid > 0
    assert int(keep.sum()) == 1500
    masked, dense = G.learner(), G.learner()
    for ln in (masked, dense):
        ln.learn(*warm)
        assert ln.path == "fused"
    masked.learn(states, actions, old_lp, returns, valid)
    dense.learn(states[keep], actions[keep], old_lp[keep], returns[keep], valid[keep])
    torch.cuda.synchronize()
    for net in G.NETS:
        for (name, p), (_, q) in zip(getattr(masked, net).named_parameters(), getattr(dense, net).named_parameters()):
            assert torch.equal(p, q), "%s.%s" % (net, name)


def test_iterate_refuses_values_it_cannot_hand_out(torch_gpu):
    """V(s) comes out of train_step()'s forward pass only: an iteration that has to reduce the gradient between pass and
    step, or that does not update, raises instead of leaving values_out unwritten."""
    torch = torch_gpu
    _, critic = G.learner()._fused_nets()
    states, _, _, returns = G.samples(torch, 1200, 100)
    count, values = torch.full((1,), 100.0, device="cuda"), torch.empty(100, device="cuda")
    assert critic.hands_out_values()
    for how in (dict(reduce=lambda g: None), dict(update=False), dict(one_launch=False)):
        assert not critic.hands_out_values(**how)
        with pytest.raises(ValueError):
            critic.iterate(1, states, returns, None, None, count, values_out=values, **how)
