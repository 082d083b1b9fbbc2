"""CPU: the numpy restatement of the beam selection on hand-worked cases, the argument errors of fjsp_beam_select (refused
before any device call) and the argument checks of policy_search.beam_search that run before anything is launched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import beam_reference as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = np.inf, np.nan


def _check(cost, done, width_out, parent, action, out):
    p, a, c = R.beam_select(np.asarray(cost, np.float64), None if done is None else np.asarray(done, np.uint8), width_out)
    assert p.dtype == np.int32 and a.dtype == np.int32 and c.dtype == np.float64
    assert np.array_equal(p, np.asarray(parent).reshape(width_out, -1))
    assert np.array_equal(a, np.asarray(action).reshape(width_out, -1))
    want = np.asarray(out, np.float64).reshape(width_out, -1)
    assert np.array_equal(c.view(np.uint64), want.view(np.uint64))


def test_reference_orders_by_cost():
    # one source env, 2 beams x 3 actions
    _check([[[5.0, 1.0, 3.0]], [[2.0, 6.0, 0.5]]], None, 4, [1, 0, 1, 0], [2, 1, 0, 2], [0.5, 1.0, 2.0, 3.0])


def test_reference_tie_by_parent():
    # cost 1.0 in beam 1 action 0 and in beam 0 action 2: the lower parent first, whatever the action
    _check([[[4.0, 4.5, 1.0]], [[1.0, 9.0, 9.0]]], None, 3, [0, 1, 0], [2, 0, 0], [1.0, 1.0, 4.0])


def test_reference_tie_by_action_and_signed_zero():
    # -0.0 and 0.0 are one cost: action 1 (0.0) stays ahead of action 2 (-0.0); the output keeps the input's bits
    _check([[[7.0, 0.0, -0.0, 0.0]]], None, 3, [0, 0, 0], [1, 2, 3], [0.0, -0.0, 0.0])


def test_reference_done_beam_is_one_candidate():
    # beam 0 is done: only its entry 0 counts (cost 2.0, action -1), its 0.1 and 0.2 are ignored
    _check([[[2.0, 0.1, 0.2]], [[3.0, 1.0, 2.0]]], [[1], [0]], 4, [1, 0, 1, 1], [1, -1, 2, 0], [1.0, 2.0, 2.0, 3.0])


def test_reference_all_inf_source_and_padding():
    # source 0 has no candidate at all (+inf and NaN), source 1 has two: ranks past them are (-1, -1, +inf)
    cost = [[[INF, NAN], [4.0, INF]], [[NAN, INF], [NAN, 3.0]]]
    _check(cost, None, 3, [[-1, 1], [-1, 0], [-1, -1]], [[-1, 1], [-1, 0], [-1, -1]], [[INF, 3.0], [INF, 4.0], [INF, INF]])
    # -inf is a candidate, and the best one
    _check([[[1.0, -INF]]], None, 2, [0, 0], [1, 0], [-INF, 1.0])
    # a done beam whose entry 0 is +inf contributes nothing
    _check([[[INF, 1.0]]], [[1]], 1, [-1], [-1], [INF])


def test_beam_select_is_exported_and_declared(built):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    from deep_reinforcement_learning_for_fjsp_amd._build import LIB_PATH
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "fjsp_beam_select" in set(line.split()[-1] for line in out.splitlines() if line.strip())
    header = open(os.path.join(REPO, "include", "fjsp_amd.h")).read()
    assert re.search(r"\bfjsp_beam_select\s*\(", header)
    vp, i32 = C.c_void_p, C.c_int32
    assert _capi.SIGNATURES["fjsp_beam_select"] == (C.c_int, [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp])


def test_beam_select_bad_args_error_without_a_gpu(built):
    """Every limit violation and null pointer is refused before any device call: no GPU needed."""
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    lib = _capi.lib()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)        # never dereferenced

    def call(cost=dummy, n_src=4, width_in=4, n_actions=30, width_out=4, parent=dummy, action=dummy, out=dummy):
        return lib.fjsp_beam_select(cost, None, n_src, width_in, n_actions, width_out, parent, action, out, None)

    assert call(cost=None) == _capi.FJSP_E_ARG
    assert b"fjsp_beam_select" in lib.fjsp_last_error()
    assert call(parent=None) == _capi.FJSP_E_ARG
    assert call(action=None) == _capi.FJSP_E_ARG
    assert call(out=None) == _capi.FJSP_E_ARG
    for bad in (0, -1):
        assert call(n_src=bad) == _capi.FJSP_E_ARG
    for bad in (0, -1, 65):
        assert call(width_in=bad) == _capi.FJSP_E_ARG
        assert call(width_out=bad) == _capi.FJSP_E_ARG
    for bad in (0, -1, 129):
        assert call(n_actions=bad) == _capi.FJSP_E_ARG


def test_parent_of_identity_holds_over_the_limits():
    """csrc/fjsp_beam.hip parent_of: the high word of (c << 12) * ceil(2^20 / d) is c // d for every candidate index
    c < 64 * 128 and action count d <= 128."""
    c = np.arange(64 * 128, dtype=np.uint64)
    assert int(c[-1]) << 12 < 2 ** 32
    for d in range(1, 129):
        m = np.uint64(((1 << 20) + d - 1) // d)
        assert np.array_equal(((c << np.uint64(12)) * m) >> np.uint64(32), c // np.uint64(d)), d


class _FakeBatch(object):
    """What the argument checks look at: no handle, nothing to launch on."""

    def __init__(self, variant=0, state_size=20, N=8):
        self.variant, self.state_size, self.N, self.n_inst = variant, state_size, N, 4


def test_beam_search_argument_checks():
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.MPPPO import ActorNet
    b, actor = _FakeBatch(0, 20), ActorNet(20, 128, 2, 30)
    for width in (0, -1, 65):
        with pytest.raises(ValueError, match="width"):
            PS.beam_search(b, actor, width)
    with pytest.raises(ValueError, match="score"):
        PS.beam_search(b, actor, 4, score="entropy")
    with pytest.raises(ValueError, match="objective"):
        PS.beam_search(b, actor, 4, score="rollout")
    with pytest.raises(ValueError):
        PS.beam_search(b, actor, 4, objective="throughput")
    with pytest.raises(ValueError):
        PS.beam_search(b, ActorNet(20, 128, 2, 31), 4)              # an actor of another action count
    with pytest.raises(ValueError):
        PS.beam_search(b, actor, 4, candidates=[(6, 0)])            # not an action of SO_FJSSP
