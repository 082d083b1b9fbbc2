"""GPU: what the six in-launch policy entries answer to arguments they refuse -- fjsp_env_rollout_policy, fjsp_env_play_policy,
fjsp_env_policy_build and their _orders twins.  EXPECTED is the (return code, fjsp_last_error()) of every call below as the
library answered before the entries were put on one body per kind; the test asserts exactly that table, so the order in
which an entry checks its arguments (which decides the text when two things are wrong at once) stays what it was.

Batches of three envs on tiny shops: single-order SO_FJSSP (generated 10 x 5), two-order SO_FJSSP (gen6601 of the so_dfjsp
suite: S = 2, 15 kinds, 9 machines) and MO_DFJSP with order arrivals (gen8800 of the mo_dfjsp suite: S = 2).  Every batch
gets every case on every entry the case applies to, so each single fault is also met together with the wrong route.
A refused call launches nothing; the only launches are those of the case "none" on the entries of the batch's own route."""
import ctypes as C

import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

N, T = 3, 10
BATCHES = ("single", "two_orders", "mo_dfjsp")
ROLLOUTS = ("fjsp_env_rollout_policy", "fjsp_env_rollout_policy_orders")
PLAYS = ("fjsp_env_play_policy", "fjsp_env_play_policy_orders")
BUILDS = ("fjsp_env_policy_build", "fjsp_env_policy_orders_build")
# case -> the faults it puts into an otherwise valid call
ROLLOUT_CASES = {
    "none": (), "T0": ("T0",), "null_state_in": ("null_state_in",), "hidden200": ("hidden200",),
    "actor_state_size": ("actor_state_size",), "buffer_N": ("buffer_N",),
}
PLAY_CASES = {
    "none": (), "T0": ("T0",), "null_state_in": ("null_state_in",), "hidden200": ("hidden200",),
    "actor_state_size": ("actor_state_size",), "pair_div": ("pair_div",), "no_seed": ("no_seed",), "few_rows": ("few_rows",),
    "hidden200+pair_div": ("hidden200", "pair_div"), "pair_div+no_seed": ("pair_div", "no_seed"),
}
BUILD_CASES = {"state_size_0": 0, "state_size_33": 33, "state_size_batch": None}

E_ARG, E_UNSUPPORTED = -1, -5
ARGS = (E_ARG, "bad arguments")
BUFFER = (E_ARG, "the rollout buffer does not match the batch (N, state_size, T, device)")
PAIR_DIV = (E_ARG, "pair_div does not divide n_actions")
SEED = (E_ARG, "sampling envs need d_seed")
ROWS = (E_ARG, "d_state_in has fewer rows than the batch")
STATE_SIZE = (E_ARG, "state_size outside 1..32")
ACTOR = (E_UNSUPPORTED, "the in-kernel actor is state_size (<= 32) -> 128 -> 128 -> n_actions (<= 32)")
HAS_ORDERS = (E_UNSUPPORTED, "the batch has order arrivals (their LPs are served between launches): single-order batches only")
NO_ORDERS = (E_UNSUPPORTED, "the batch has no order arrivals: fjsp_env_play_policy / fjsp_env_rollout_policy run it in one launch")
MO_DFJSP = (E_UNSUPPORTED, "MO_DFJSP batches are not played inside the launch (their 12 x 10 actions do not fit the in-kernel actor)")
RAN = (0, None)
# The recorded table: batch -> the two entries of a kind -> case -> (the one-launch entry's answer, its _orders twin's); an
# error text is the entry's name, ": " and the text above.
EXPECTED = {
    "single": {
        ROLLOUTS: {
            "none": (RAN, NO_ORDERS), "T0": (ARGS, ARGS), "null_state_in": (ARGS, ARGS), "hidden200": (ACTOR, NO_ORDERS),
            "actor_state_size": (ACTOR, NO_ORDERS), "buffer_N": (BUFFER, BUFFER),
        },
        PLAYS: {
            "none": (RAN, NO_ORDERS), "T0": (ARGS, ARGS), "null_state_in": (ARGS, ARGS), "hidden200": (ACTOR, NO_ORDERS),
            "actor_state_size": (ACTOR, NO_ORDERS), "pair_div": (PAIR_DIV, NO_ORDERS), "no_seed": (SEED, NO_ORDERS),
            "few_rows": (ROWS, NO_ORDERS), "hidden200+pair_div": (ACTOR, NO_ORDERS), "pair_div+no_seed": (PAIR_DIV, NO_ORDERS),
        },
        BUILDS: {
            "state_size_0": (STATE_SIZE, STATE_SIZE), "state_size_33": (STATE_SIZE, STATE_SIZE),
            "state_size_batch": ((0, (16, 139520, 1)), NO_ORDERS),
        },
    },
    "two_orders": {
        ROLLOUTS: {
            "none": (HAS_ORDERS, RAN), "T0": (ARGS, ARGS), "null_state_in": (ARGS, ARGS), "hidden200": (ACTOR, ACTOR),
            "actor_state_size": (ACTOR, ACTOR), "buffer_N": (BUFFER, BUFFER),
        },
        PLAYS: {
            "none": (HAS_ORDERS, RAN), "T0": (ARGS, ARGS), "null_state_in": (ARGS, ARGS), "hidden200": (ACTOR, ACTOR),
            "actor_state_size": (ACTOR, ACTOR), "pair_div": (PAIR_DIV, PAIR_DIV), "no_seed": (SEED, SEED),
            "few_rows": (ROWS, ROWS), "hidden200+pair_div": (ACTOR, ACTOR), "pair_div+no_seed": (PAIR_DIV, PAIR_DIV),
        },
        BUILDS: {
            "state_size_0": (STATE_SIZE, STATE_SIZE), "state_size_33": (STATE_SIZE, STATE_SIZE),
            "state_size_batch": (HAS_ORDERS, (0, (16, 143616, 1, 2))),
        },
    },
    "mo_dfjsp": {
        ROLLOUTS: {
            "none": (HAS_ORDERS, MO_DFJSP), "T0": (ARGS, ARGS), "null_state_in": (ARGS, ARGS), "hidden200": (ACTOR, MO_DFJSP),
            "actor_state_size": (ACTOR, MO_DFJSP), "buffer_N": (BUFFER, BUFFER),
        },
        PLAYS: {
            "none": (HAS_ORDERS, MO_DFJSP), "T0": (ARGS, ARGS), "null_state_in": (ARGS, ARGS), "hidden200": (ACTOR, MO_DFJSP),
            "actor_state_size": (ACTOR, MO_DFJSP), "pair_div": (PAIR_DIV, MO_DFJSP), "no_seed": (SEED, MO_DFJSP),
            "few_rows": (ROWS, MO_DFJSP), "hidden200+pair_div": (ACTOR, MO_DFJSP), "pair_div+no_seed": (PAIR_DIV, MO_DFJSP),
        },
        BUILDS: {
            "state_size_0": (STATE_SIZE, STATE_SIZE), "state_size_33": (STATE_SIZE, STATE_SIZE),
            "state_size_batch": (HAS_ORDERS, MO_DFJSP),
        },
    },
}


def expected(name):
    """EXPECTED[name] in the shape of observe(): {(entry, case): (return code, full error text or what a success leaves)}."""
    out = {}
    for entries, cases in EXPECTED[name].items():
        for case, answers in cases.items():
            for entry, (rc, what) in zip(entries, answers):
                out[(entry, case)] = (rc, "%s: %s" % (entry, what) if rc != 0 else what)
    return out


def _batch(torch, name):
    """(batch, mo, pair_div of a valid call) of the named batch, reset."""
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, VARIANT_MO_DFJSP
    if name == "single":
        return EnvBatch(H.gen_10x5(N, 360), N, rng_seed=11), None, 5
    suite, inst, variant = ("so_dfjsp", "gen6601", 0) if name == "two_orders" else ("mo_dfjsp", "gen8800", VARIANT_MO_DFJSP)
    insts = [a for a in H.load_suite(suite)[0] if a.name == inst]
    assert len(insts) == 1 and insts[0].S == 2
    mo = None
    if name == "mo_dfjsp":
        mo = torch.zeros(N, 4, dtype=torch.float64, device="cuda"); mo[:, 0] = 1.0
    return EnvBatch(H.instance_set_from(insts), N, variant=variant, rng_seed=12), mo, 5 if name == "two_orders" else 10


def observe(torch, name):
    """{(entry, case): (return code, error text; of a call that succeeds: None, or what a _build entry reported)} of one batch."""
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.Buffer import RolloutBuffer
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.MPPPO import ActorNet
    from deep_reinforcement_learning_for_fjsp_amd.agents.native_actor import native_actor_params
    lib, p = _capi.lib(), _capi.ptr
    b, mo, div = _batch(torch, name)
    b.reset()
    S = b.state_size
    torch.manual_seed(8)
    net = ActorNet(S, 128, 2, 30).cuda()
    good = native_actor_params(net)
    assert good is not None and b.N == N

    def actor(faults):
        ap = _capi.ActorParams.from_buffer_copy(good)
        if "hidden200" in faults:
            ap.hidden = 200
        if "actor_state_size" in faults:
            ap.state_size = S - 1
        return ap

    def answer(rc, ok=None):
        return (rc, lib.fjsp_last_error().decode() if rc != 0 else ok)

    out = {}
    eps = torch.zeros(1, dtype=torch.float32, device="cuda")
    seed = torch.tensor([7], dtype=torch.int64, device="cuda")
    flat, logp = torch.zeros(T, N, device="cuda"), torch.zeros(T, N, device="cuda")
    steps = torch.zeros(N, dtype=torch.int32, device="cuda")
    buffers = {False: RolloutBuffer(T, N, S, device=0), True: RolloutBuffer(T, N + 1, S, device=0)}
    for entry in ROLLOUTS:
        for case, faults in ROLLOUT_CASES.items():
            st0 = b.state.clone()
            rc = getattr(lib, entry)(b._h, buffers["buffer_N" in faults]._h, C.byref(actor(faults)), p(eps), p(seed), div,
                                     0 if "T0" in faults else T, p(mo), None if "null_state_in" in faults else p(st0), p(flat),
                                     p(logp), b._p_state, b._stream())
            out[(entry, case)] = answer(rc)
    for entry in PLAYS:
        for case, faults in PLAY_CASES.items():
            st0 = b.state.clone()
            rc = getattr(lib, entry)(b._h, C.byref(actor(faults)), 7 if "pair_div" in faults else div,
                                     N - 1 if "no_seed" in faults else N, None if "no_seed" in faults else p(seed),
                                     0 if "T0" in faults else T, p(mo), None if "null_state_in" in faults else p(st0),
                                     N - 1 if "few_rows" in faults else N, None, None, None, p(steps), b._p_state, b._p_reward,
                                     b._p_done, b._stream())
            out[(entry, case)] = answer(rc)
    for entry, n_out in zip(BUILDS, (3, 4)):
        for case, state_size in BUILD_CASES.items():
            got = (C.c_int32 * n_out)()
            rc = getattr(lib, entry)(b._h, S if state_size is None else state_size, got)
            out[(entry, case)] = answer(rc, tuple(got))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", BATCHES)
def test_entries_answer_as_recorded(built, name):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    got = observe(torch, name)
    want = expected(name)
    assert got.keys() == want.keys()
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
