"""GPU: the PPO rollout on every collection path against a recording (tests/golden/ppo_rollout_paths.npz).

The file was written by tests/golden/make_ppo_rollout_golden.py at commit 48b820983c274cbe340f3f1d5741352432f7e846, the
last one at which the collection was `collect_and_learn` over a dict of cached state.  Every case of that module runs
again here: what learn() is handed, what the buffer, the sampler and the environments hold, the losses and every
parameter tensor, after every round, must equal the file's by SHA-256 (the f64 sums and largest magnitudes it also holds
are there to make a mismatch readable), and so must the rollout's length and the number of buffers and samplers
constructed.  One case, in_launch_refused, is held to everything but its parameters and losses, which that commit did not
reproduce from process to process (the maker's docstring has the figures)."""
import os

import numpy as np
import pytest

from tests import helpers as H
from tests.golden import make_ppo_rollout_golden as G

pytestmark = pytest.mark.gpu

COMMIT = "48b820983c274cbe340f3f1d5741352432f7e846"
CASES = ("eager_sampler", "eager_torch", "graph_sampler", "graph_torch", "in_launch", "in_launch_orders", "in_launch_refused",
         "mpppo", "regrown")


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(H.GOLDEN, "ppo_rollout_paths.npz"), allow_pickle=False)


def test_the_file_holds_every_case(golden):
    assert CASES == tuple(sorted(G.cases())) == tuple(str(c) for c in golden["cases"])
    assert str(golden["commit"]) == COMMIT


@pytest.mark.parametrize("case", CASES)
def test_rollouts_are_the_recorded_ones(torch_gpu, golden, monkeypatch, case):
    got, agent = G.cases()[case](torch_gpu, monkeypatch.setattr)
    assert all(ln.path == "eager" for ln in G.learners(agent))
    keys = [str(k) for k in golden[case + "_keys"]]
    assert keys == [str(k) for k in got["keys"]]
    assert sorted("%s_%s" % (case, key) for key in got) == sorted(G.of_case(golden.files, case))
    for key in got:
        assert got[key].dtype == golden["%s_%s" % (case, key)].dtype and got[key].shape == golden["%s_%s" % (case, key)].shape, key
    assert np.array_equal(got["len"], golden[case + "_len"]), (got["len"], golden[case + "_len"])
    assert np.array_equal(got["made"], golden[case + "_made"]), (got["made"], golden[case + "_made"])
    want_sum, want_big = golden[case + "_sum"], golden[case + "_maxabs"]
    for r, k in zip(*np.nonzero((got["sha256"] != golden[case + "_sha256"]).any(-1))):
        pytest.fail("%s: %s of round %d differs: sum %.17g (recorded %.17g), max |.| %.17g (recorded %.17g)"
                    % (case, keys[k], r + 1, got["sum"][r, k], want_sum[r, k], got["maxabs"][r, k], want_big[r, k]))
    for key in got:          # (the losses, where the case pins them; the sums and magnitudes follow from the digests)
        assert np.array_equal(got[key], golden["%s_%s" % (case, key)]), (key, got[key], golden["%s_%s" % (case, key)])
