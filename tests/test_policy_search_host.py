"""CPU: the policy play entry point of the C ABI (export, header, ctypes signature, argument errors) and the argument
checks of policy_search that run before anything is launched."""
import ctypes as C
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_play_policy_is_exported_and_declared(built):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    from deep_reinforcement_learning_for_fjsp_amd._build import LIB_PATH
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "fjsp_env_play_policy" in set(line.split()[-1] for line in out.splitlines() if line.strip())
    header = open(os.path.join(REPO, "include", "fjsp_amd.h")).read()
    assert re.search(r"\bfjsp_env_play_policy\s*\(", header)
    vp, i32 = C.c_void_p, C.c_int32
    assert _capi.SIGNATURES["fjsp_env_play_policy"] == (
        C.c_int, [vp, C.POINTER(_capi.ActorParams), i32, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp])
    assert _capi.lib().fjsp_abi_version() == 1


def test_play_policy_bad_args_error_without_a_gpu(built):
    """Null env, T = 0 and the other argument errors are refused before the env is looked at: no device needed."""
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    lib = _capi.lib()
    fake = C.create_string_buffer(256)            # never dereferenced: every call below fails its argument check first
    env = C.cast(fake, C.c_void_p)
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)

    def call(e, T=10, n_greedy=0, pair_div=5, state_in=dummy, n_state_in=4, outs=True):
        o = dummy if outs else None
        return lib.fjsp_env_play_policy(e, None, pair_div, n_greedy, dummy, T, None, state_in, n_state_in, None, None, None,
                                        o, o, o, o, None)

    assert call(None) == -1
    assert b"fjsp_env_play_policy" in lib.fjsp_last_error()
    assert call(env, T=0) == -1
    assert call(env, T=-3) == -1
    assert call(env, n_greedy=-1) == -1
    assert call(env, pair_div=-1) == -1
    assert call(env, state_in=None) == -1
    assert call(env, n_state_in=0) == -1
    assert call(env, outs=False) == -1


class _FakeBatch(object):
    """What the argument checks look at: no handle, nothing to launch on."""

    def __init__(self, variant=0, state_size=20, N=8):
        self.variant, self.state_size, self.N, self.n_inst = variant, state_size, N, 4


def _actor(S, A, hidden=128, layers=2):
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.MPPPO import ActorNet
    return ActorNet(S, hidden, layers, A)


def test_action_encoding_follows_the_variant():
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    assert PS.action_encoding(_actor(20, 30), _FakeBatch(0, 20)) == (30, 5)      # SO_FJSSP: 6 x 5 pairs
    assert PS.action_encoding(_actor(20, 30), _FakeBatch(5, 20)) == (30, 5)      # SO_DFJSP
    assert PS.action_encoding(_actor(18, 20), _FakeBatch(1, 18)) == (20, 0)      # SO_SFJSP: 20 flat actions
    assert PS.action_encoding(_actor(25, 18), _FakeBatch(2, 25)) == (18, 0)      # MO_FJSSP_discretes: 18 flat actions
    assert PS.action_encoding(_actor(30, 120, 200, 5), _FakeBatch(4, 30)) == (120, 10)   # MO_DFJSP: 12 x 10


@pytest.mark.parametrize("call", ["play", "best_of", "policy_lookahead"])
def test_actor_that_does_not_fit_the_variant_is_refused(call):
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    b = _FakeBatch(0, 20)
    for actor in (_actor(20, 20), _actor(20, 31), _actor(18, 30)):        # wrong action count, wrong state size
        with pytest.raises(ValueError):
            if call == "play":
                PS.play(b, actor)
            elif call == "best_of":
                PS.best_of(b, actor, 4, "makespan")
            else:
                PS.policy_lookahead(b, actor, "makespan")


def test_best_of_and_lookahead_argument_checks():
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    b, actor = _FakeBatch(0, 20), _actor(20, 30)
    for k in (0, -1):
        with pytest.raises(ValueError):
            PS.best_of(b, actor, k, "makespan")
    with pytest.raises(ValueError):
        PS.best_of(b, actor, 4, "throughput")
    with pytest.raises(ValueError):
        PS.policy_lookahead(b, actor, "throughput")
    for bad in ([(6, 0)], [(0, 5)], [7], []):                # not an action of SO_FJSSP (or no candidate at all)
        with pytest.raises(ValueError):
            PS.policy_lookahead(b, actor, "makespan", candidates=bad)
    with pytest.raises(ValueError):
        PS.policy_lookahead(_FakeBatch(1, 18), _actor(18, 20), "makespan", candidates=[20])
