"""The generator's size-limit cases (tests/generator_limit_cases.py), the part that needs no GPU: the host generator
(fjsp_instance.cpp, the reference of tests/test_gpu_generator_limits.py) against the Python restatement of the stream on every
case, array by array -- the shop, the orders' counts, arrivals and sorted delivery times, the machine data, the attempt an
MO_DFJSP instance is made of --; the edge every case exists for, on the host's instances; their fluid LPs; and that every
case's parameters pass each worst-case check of the generated creates (they stop at "no HIP device" here).  The refusals one
step past each limit are rows of the REFUSED tables of tests/test_generate*_host.py; their accepted twins one step inside are
the cases themselves and ACCEPTED below."""
import ctypes as C

import numpy as np
import pytest

from deep_reinforcement_learning_for_fjsp_amd import _capi, instances as fi
from deep_reinforcement_learning_for_fjsp_amd._capi import GenDynamic, GenOrders, GenParams
from tests import generator_limit_cases as LC
from tests import test_generate_dynamic_host as TDH
from tests import test_generate_host as TH
from tests import test_generate_orders_host as TOH

_SETS = {}


def instances_of(name):
    """The case's host instances with their fluid LPs solved, made once."""
    if name not in _SETS:
        _SETS[name] = LC.host_set(LC.CASES[name])
    return _SETS[name]


@pytest.mark.parametrize("name", LC.GENERATED)
def test_host_generator_matches_the_restatement(name):
    c = LC.CASES[name]
    s = instances_of(name)
    for i in range(c["n_inst"]):
        seed = c["seed"] + i
        a, r = s.arrays(i), LC.restate(c["params"], seed)
        assert (a.R, a.M, a.K, a.S) == (r["R"], r["M"], r["K"], r["S"]), (name, i)
        for key in LC.INT_KEYS:
            got, want = getattr(a, key), r[key]
            assert got.shape == want.shape and np.array_equal(got, want), (name, i, key)
        if isinstance(c["params"], GenDynamic):
            assert fi.dynamic_seed(c["params"], seed) == r["used"], (name, i)
            for key in TDH.DYN_KEYS:
                got, want = getattr(a, key), r[key]
                assert got.shape == want.shape and np.array_equal(got, want), (name, i, key)
        elif not isinstance(c["params"], GenParams):
            assert a.ddt == c["params"].r.DDT_min, (name, i)


@pytest.mark.parametrize("name", LC.GENERATED)
def test_case_reaches_its_edge_and_its_lps_are_solved(name):
    c = LC.CASES[name]
    s = instances_of(name)                      # solve_fluid raised if an LP had failed
    arrs = [s.arrays(i) for i in range(c["n_inst"])]
    assert c["reaches"](arrs), name
    assert 4 <= c["n_inst"] <= 8
    for a in arrs:
        assert np.all(np.isfinite(a.x)) and np.all((a.x * (a.p > 0)).sum(1) > 0.0), name     # a fluid rate for every operation type
        assert c["steps"] is not None or LC.operations(a) <= 350, name
    if c["route"]:
        assert all(LC.tableau_fits(a) == (c["route"] == "lds") for a in arrs), name


def test_redraw_deep_attempts():
    c = LC.CASES["redraw_deep"]
    q = c["params"]
    got = []
    for i in range(c["n_inst"]):
        seed = c["seed"] + i
        attempts = [seed] + [TH.draw(seed ^ TDH.REDRAW_STREAM, j) for j in range(q.redraws)]
        used = fi.dynamic_seed(q, seed)
        assert used in attempts, i
        got.append(attempts.index(used))
        assert all(TDH.idle_in_attempt_0(q, t) for t in attempts[:got[-1]]) and not TDH.idle_in_attempt_0(q, used), i
        assert LC.restate(q, seed)["attempt"] == got[-1], i
    assert got == LC.REDRAW_ATTEMPTS and max(got) >= 3


def test_redraw_exhausted_names_the_seed():
    c = LC.CASES["redraw_exhausted"]
    q, bad = c["params"], LC.EXHAUSTED_INSTANCE
    assert q.redraws == _capi.FJSP_GEN_MAX_REDRAWS == 16
    state = [LC.restate(q, c["seed"] + i) is None for i in range(c["n_inst"])]
    assert state.index(True) == bad and not all(state[bad:]), state         # the first one that fails; a playable one behind it
    seed = c["seed"] + bad
    assert all(TDH.idle_in_attempt_0(q, t) for t in [seed] + [TH.draw(seed ^ TDH.REDRAW_STREAM, j) for j in range(16)])
    with pytest.raises(_capi.FjspError) as err:
        LC.host_set(c, solve=False)
    assert err.value.code == _capi.FJSP_E_UNSUPPORTED
    assert "instance %d (seed %d)" % (bad, seed) in str(err.value) and "in each of 17 attempts (redraws = 16)" in str(err.value)
    used = C.c_uint64()
    assert _capi.lib().fjsp_gen_dynamic_seed(C.byref(q), seed, C.byref(used)) == _capi.FJSP_E_UNSUPPORTED
    assert "seed %d" % seed in _capi.lib().fjsp_last_error().decode()


# ---- one step inside every limit: the creates get past every check -----------------------------------------------------------
def create(params, variant, family):
    if isinstance(params, GenDynamic):
        return TDH.create(params)
    return (TOH.create if isinstance(params, GenOrders) else TH.create)(params, variant=variant, family=-1 if family is None else family)


def accepted(rc, msg):
    return rc == 0 or (rc == _capi.FJSP_E_HIP and "no HIP device" in msg)


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_every_case_passes_the_worst_case_checks(name):
    c = LC.CASES[name]
    for variant in c["variants"] or (LC.VARIANT_MO_DFJSP,):
        if name == "redraw_exhausted":           # (where a device exists the create fails at the instance, not at a check)
            rc, msg = create(c["params"], variant, c["family"])
            assert accepted(rc, msg) or (rc == _capi.FJSP_E_UNSUPPORTED and "in each of 17 attempts" in msg), (rc, msg)
        else:
            assert accepted(*create(c["params"], variant, c["family"])), (name, variant)


# the twins of the REFUSED rows, one step inside: 254 stages where a handle has order arrivals, and the rows' own parameters
# (the job count at plan_layout's LDS rule is applied after the device is found: tests/test_gpu_generator_limits.py)
ACCEPTED = [
    ("J_max = 254 with two orders", LC.go(2, 2, R_min=1, R_max=1, J_min=254, J_max=254), 0),
    ("J_max = 254, MO_DFJSP", LC.gd(2, TDH.machine(), 8, R_min=1, R_max=1, J_min=254, J_max=254), 4),
    ("p_max = 65535", TH.params(p_max=65535), 0),
    ("M = 32", TH.params(M=32), 0),
    ("S_max = 16", TOH.orders(S_max=16), 0),
    ("W_max = 2047", TDH.dyn(mc=TDH.machine(2047)), 4),
    ("redraws = 16", TDH.dyn(redraws=16), 4),
]


@pytest.mark.parametrize("what,params,variant", ACCEPTED, ids=[r[0] for r in ACCEPTED])
def test_one_step_inside_each_limit_is_accepted(what, params, variant):
    assert accepted(*create(params, variant, None)), what
