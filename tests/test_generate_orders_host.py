"""The number of orders drawn per instance (fjsp_gen_orders), the part that needs no GPU: the three new calls exist in
header, library and binding; fjsp_gen_draw_orders against fjsp_gen_draw and a restatement of draw 2 of the auxiliary
stream; a point range against fjsp_instances_generate with the fixed parameter set; and fjsp_env_create_generated_orders
refuses what it cannot play before it looks for a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from deep_reinforcement_learning_for_fjsp_amd import _capi, instances as fi
from deep_reinforcement_learning_for_fjsp_amd._capi import GenOrders, GenParams, GenRanges
from tests.test_generate_host import MASK, randint
from tests.test_generate_ranges_host import AUX_STREAM, SEEDS, same_arrays, small_base

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("fjsp_gen_draw_orders", "fjsp_instances_generate_orders", "fjsp_env_create_generated_orders")


def orders_py(q, seed):
    """S of instance `seed` under q: draw 2 of the stream seeded seed ^ AUX_STREAM, the integer formula of M."""
    return randint((seed & MASK) ^ AUX_STREAM, 2, q.S_min, q.S_max)


def test_new_calls_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "fjsp_amd.h")).read()
    lib = _capi.lib()
    for name in NEW_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1], name
    assert re.search(r"}\s*fjsp_gen_orders\s*;", header) and "#define FJSP_GEN_MAX_ORDERS 16" in re.sub(r"[ \t]+", " ", header)
    assert "#define FJSP_ABI_VERSION 1" in re.sub(r"[ \t]+", " ", header)
    assert lib.fjsp_abi_version() == 1
    # the two older structs keep their layout; the order range follows the ranges
    assert C.sizeof(GenParams) == 64 and C.sizeof(GenRanges) == 88
    assert GenOrders.S_min.offset == 88 and GenOrders.S_max.offset == 92 and C.sizeof(GenOrders) == 96


def test_reference_order_ranges():
    for agent in ("da3c", "hmpsac"):
        q = fi.reference_order_ranges(agent)
        assert (q.r.M_min, q.r.M_max, q.r.DDT_min, q.r.DDT_max, q.S_min, q.S_max) == (10, 20, 0.5, 1.5, 1, 5)
        ref = fi.reference_generator_params(1.0, 0, 1)
        for f, _ in GenParams._fields_:
            assert getattr(q.r.base, f) == getattr(ref, f), f
    with pytest.raises(ValueError):
        fi.reference_order_ranges("mpppo")
    m = fi.reference_training_ranges("mpppo")              # unchanged
    assert (m.M_min, m.M_max, m.base.S) == (10, 20, 1)


def test_draw_orders_keeps_m_and_ddt_and_adds_draw_2():
    q = fi.reference_order_ranges("da3c")
    for seed in SEEDS:
        p, p2 = fi.draw_params(q, seed), fi.draw_params(q.r, seed)
        assert (p.M, p.DDT) == (p2.M, p2.DDT), seed
        assert p.S == orders_py(q, seed), seed
        for f, _ in GenParams._fields_:
            if f not in ("M", "DDT", "S"):
                assert getattr(p, f) == getattr(q.r.base, f), (seed, f)


def test_every_order_count_of_the_range_occurs():
    q = fi.reference_order_ranges("da3c")
    got = [fi.draw_params(q, 77000 + s).S for s in range(2000)]
    assert set(got) == {1, 2, 3, 4, 5}
    assert got == [orders_py(q, 77000 + s) for s in range(2000)]


def test_generate_orders_is_draw_then_generate():
    q = GenOrders(GenRanges(small_base(), 3, 6, 0.5, 1.5), 1, 4)
    drawn = fi.InstanceSet(len(SEEDS))
    for i, seed in enumerate(SEEDS):
        drawn.generate(i, seed, q)
        a = drawn.arrays(i)
        same_arrays(a, fi.InstanceSet(1).generate(0, seed, fi.draw_params(q, seed)).arrays(0), seed)
        assert a.S == orders_py(q, seed) and a.count.shape == (a.S, a.R) and len(a.arrive) == a.S == len(a.delivery), seed
    assert {drawn.arrays(i).S for i in range(len(SEEDS))} == {1, 2, 3, 4}


@pytest.mark.parametrize("S", [1, 3])
def test_point_range_reproduces_the_fixed_parameter_generator(S):
    q = GenOrders(GenRanges(small_base(), 6, 6, 1.25, 1.25), S, S)
    fixed_prm = small_base(M=6, DDT=1.25, S=S)
    for seed in SEEDS:
        p = fi.draw_params(q, seed)
        assert (p.M, p.DDT, p.S) == (6, 1.25, S), seed
        a = fi.InstanceSet(1).generate(0, seed, q).arrays(0)
        same_arrays(a, fi.InstanceSet(1).generate(0, seed, fixed_prm).arrays(0), seed)
        assert a.S == S
    if S == 1:       # ... and so the instances of the ranges without an order count
        for seed in SEEDS[:32]:
            same_arrays(fi.InstanceSet(1).generate(0, seed, q).arrays(0), fi.InstanceSet(1).generate(0, seed, q.r).arrays(0), seed)


# ---- refusals before any device is looked for ------------------------------------------------------------------------------
def orders(S_min=1, S_max=3, M_min=3, M_max=8, DDT_min=0.5, DDT_max=1.5, **kw):
    d = dict(R_min=3, R_max=5, J_min=2, J_max=3, M=0, p_min=1, p_max=20, N_min=1, N_max=3, S=0, DDT=0.0, t_si_min=100.0, t_si_max=200.0)
    d.update(kw)
    return GenOrders(GenRanges(GenParams(**d), M_min, M_max, DDT_min, DDT_max), S_min, S_max)


def create(q, n_inst=4, n_envs=4, variant=0, family=-1):
    lib, h = _capi.lib(), C.c_void_p()
    rc = lib.fjsp_env_create_generated_orders(C.byref(q), n_inst, n_envs, variant, 0, 0, family, 1000, C.byref(h))
    msg = lib.fjsp_last_error().decode()
    if rc == 0:                      # (a GPU machine: the handle exists)
        lib.fjsp_env_destroy(h)
    return rc, msg


INF, NAN = float("inf"), float("nan")
ARRIVALS = "only SO_FJSSP handles order arrivals"
REFUSED = [
    ("S_min = 0", dict(q=orders(S_min=0)), _capi.FJSP_E_ARG, "S_min"),
    ("S_min < 0", dict(q=orders(S_min=-1)), _capi.FJSP_E_ARG, "S_min"),
    ("S_max < S_min", dict(q=orders(S_min=3, S_max=2)), _capi.FJSP_E_ARG, "S_max < S_min"),
    ("S_max = 17", dict(q=orders(S_max=17)), _capi.FJSP_E_UNSUPPORTED, "16 orders (S_max)"),
    ("t_si_min = nan", dict(q=orders(t_si_min=NAN)), _capi.FJSP_E_ARG, "t_si_min"),
    ("t_si_min < 0", dict(q=orders(t_si_min=-1.0)), _capi.FJSP_E_ARG, "t_si_min"),
    ("t_si_max = inf", dict(q=orders(t_si_max=INF)), _capi.FJSP_E_ARG, "t_si_max"),
    ("t_si_max < t_si_min", dict(q=orders(t_si_min=200.0, t_si_max=100.0)), _capi.FJSP_E_ARG, "t_si_max < t_si_min"),
    ("M_max < M_min", dict(q=orders(M_min=6, M_max=5)), _capi.FJSP_E_ARG, "M_max < M_min"),
    ("DDT_max = nan", dict(q=orders(DDT_max=NAN)), _capi.FJSP_E_ARG, "DDT_max"),
    ("base: p_min = 0", dict(q=orders(p_min=0)), _capi.FJSP_E_ARG, "bad parameters"),
    ("n_inst <= 0", dict(q=orders(), n_inst=0), _capi.FJSP_E_ARG, "bad arguments"),
    ("SO_SFJSP with S_max = 2", dict(q=orders(S_max=2), variant=1), _capi.FJSP_E_UNSUPPORTED, ARRIVALS),
    ("MO_FJSSP_discretes with S_max = 2", dict(q=orders(S_max=2), variant=2), _capi.FJSP_E_UNSUPPORTED, ARRIVALS),
    ("MO_DFJSP", dict(q=orders(), variant=4), _capi.FJSP_E_UNSUPPORTED, "MO_DFJSP needs machine data"),
    ("MO_DFJSP with one order", dict(q=orders(S_max=1), variant=4), _capi.FJSP_E_UNSUPPORTED, "MO_DFJSP needs machine data"),
    # 40 kinds x 110 jobs x 15 orders = 66 000 jobs, of one operation each
    ("65536 jobs over the orders", dict(q=orders(S_max=15, R_min=40, R_max=40, J_min=1, J_max=1, N_max=110)), _capi.FJSP_E_UNSUPPORTED,
     "65535 jobs (R_max x N_max x S_max)"),
    # 20 kinds x 10 operations x 30 jobs x 11 orders = 66 000 operations of 6 600 jobs
    ("65536 operations over the orders", dict(q=orders(S_max=11, R_min=20, R_max=20, J_min=10, J_max=10, N_max=30)), _capi.FJSP_E_UNSUPPORTED,
     "65535 operations (R_max x J_max x N_max x S_max)"),
    # one operation of one job per order: only the last arrival, 15 x 2e8 > 2^31, can break the clock
    ("32-bit clock: the last arrival", dict(q=orders(S_max=16, R_min=1, R_max=1, J_min=1, J_max=1, N_max=1, t_si_max=2e8)),
     _capi.FJSP_E_UNSUPPORTED, "(S_max - 1) x t_si_max"),
    # 16 operation types x 4 jobs of up to 65 535: 4.2e6 x 4 jobs per kind with one order, 6.7e7 x 64 > 2^31 with 16
    ("32-bit clock: the work of all orders", dict(q=orders(S_max=16, R_min=4, R_max=4, J_min=4, J_max=4, N_max=4, p_max=65535)),
     _capi.FJSP_E_UNSUPPORTED, "operations of all orders"),
    # a job's next-stage byte keeps 255 for an order still to come (the twin with 254: tests/test_generator_limit_cases_host.py)
    ("J_max = 255 with S_max = 2", dict(q=orders(S_max=2, R_min=1, R_max=1, J_min=255, J_max=255)), _capi.FJSP_E_UNSUPPORTED,
     "more than 254 operations in a kind (J_max)"),
]


@pytest.mark.parametrize("what,kw,code,text", REFUSED, ids=[r[0] for r in REFUSED])
def test_create_generated_orders_refuses_before_it_looks_for_a_device(what, kw, code, text):
    rc, msg = create(**kw)
    assert rc == code, (what, rc, msg)
    assert text in msg, (what, msg)
    assert "no HIP device" not in msg


def test_accepted_parameters_pass_every_check():
    """The same small parameters pass: a handle, or no device here.  One order through the new entry point takes the three
    single-order variants as well, and the work-of-all-orders case above passes with one order."""
    ok = lambda rc, msg: rc == 0 or (rc == _capi.FJSP_E_HIP and "no HIP device" in msg)
    for variant in (0, 5):
        assert ok(*create(orders(), variant=variant)), variant
    for variant in (0, 1, 2, 5):
        assert ok(*create(orders(S_max=1), variant=variant)), variant
    assert ok(*create(orders(S_max=1, R_min=4, R_max=4, J_min=4, J_max=4, N_max=4, p_max=65535)))


def test_the_older_entry_points_keep_refusing_several_orders():
    lib, h = _capi.lib(), C.c_void_p()
    q = orders()
    q.r.base.S = 2
    assert lib.fjsp_env_create_generated_ranges(C.byref(q.r), 4, 4, 0, 0, 0, -1, 1000, C.byref(h)) == _capi.FJSP_E_UNSUPPORTED
    assert "one order only" in lib.fjsp_last_error().decode()
    prm = small_base(M=4, DDT=1.0, S=2)
    assert lib.fjsp_env_create_generated(C.byref(prm), 4, 4, 0, 0, 0, -1, 1000, C.byref(h)) == _capi.FJSP_E_UNSUPPORTED
    assert "one order only" in lib.fjsp_last_error().decode()


def test_draw_and_generate_orders_refuse_bad_bounds():
    lib = _capi.lib()
    out = GenParams()
    s = fi.InstanceSet(1)
    for q, text in ((orders(S_min=0), "S_min"), (orders(S_min=4, S_max=3), "S_max < S_min"), (orders(M_min=0), "M_min"),
                    (orders(t_si_max=NAN), "t_si_max"), (orders(t_si_min=3.0, t_si_max=2.0), "t_si_max < t_si_min")):
        assert lib.fjsp_gen_draw_orders(C.byref(q), 1, C.byref(out)) == _capi.FJSP_E_ARG and text in lib.fjsp_last_error().decode()
        assert lib.fjsp_instances_generate_orders(s.handle, 0, 1, C.byref(q)) == _capi.FJSP_E_ARG and text in lib.fjsp_last_error().decode()
    assert lib.fjsp_gen_draw_orders(None, 1, C.byref(out)) == _capi.FJSP_E_ARG
    assert lib.fjsp_instances_generate_orders(s.handle, 0, 1, C.byref(orders(R_min=0))) == _capi.FJSP_E_ARG
