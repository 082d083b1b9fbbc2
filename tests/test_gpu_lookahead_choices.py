"""GPU: the choices of the two rollout lookaheads against a recording (tests/golden/lookahead_choices.npz).

The file was written by tests/golden/make_lookahead_golden.py at commit 2441d87caed8e3465c994a9afbf8586fb16e01d7, the
last one at which lookahead.rollout_dispatch and policy_search.policy_lookahead each had a decision loop of their own.
Every case of that module runs again here; the action applied at every decision, the decisions each env took and the
objective (by bits) must equal the file's."""
import os

import numpy as np
import pytest

from tests import helpers as H
from tests.golden import make_lookahead_golden as G

pytestmark = pytest.mark.gpu

CASES = ("rule_so_wave", "rule_so_rows", "rule_mo", "policy_so", "policy_so_wrapper", "policy_mo_wrapper")


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(H.GOLDEN, "lookahead_choices.npz"), allow_pickle=False)


def test_the_file_holds_every_case(golden):
    assert tuple(sorted(CASES)) == tuple(sorted(G.cases())) == tuple(str(c) for c in golden["cases"])
    assert str(golden["commit"]) == "2441d87caed8e3465c994a9afbf8586fb16e01d7"


@pytest.mark.parametrize("case", CASES)
def test_choices_are_the_recorded_ones(torch_gpu, golden, case):
    got = G.outcome(G.cases()[case](torch_gpu))
    for key in ("actions", "steps", "objective"):
        want = golden["%s_%s" % (case, key)]
        assert got[key].dtype == want.dtype and got[key].shape == want.shape, key
        assert np.array_equal(got[key], want), key
    if case.startswith("rule_so"):      # envs finish at different decisions: rows past an env's end repeat its last choice
        steps = got["steps"]
        assert len(set(steps[:4].tolist())) == 4 and got["actions"].shape[0] == steps.max()
        for e in range(len(steps)):
            assert np.all(got["actions"][steps[e]:, e] == got["actions"][steps[e] - 1, e])
