"""Machine count and due-date tightness drawn per instance (fjsp_gen_ranges), the part that needs no GPU: the three new
calls exist in header, library and binding; fjsp_gen_draw against a Python restatement of the auxiliary stream;
fjsp_instances_generate_drawn against fjsp_instances_generate with what fjsp_gen_draw returned; and
fjsp_env_create_generated_ranges refuses what it cannot play before it looks for a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from deep_reinforcement_learning_for_fjsp_amd import _capi, instances as fi
from deep_reinforcement_learning_for_fjsp_amd._capi import GenParams, GenRanges
from tests.test_generate_host import MASK, draw, randint, replay

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("fjsp_gen_draw", "fjsp_instances_generate_drawn", "fjsp_env_create_generated_ranges")
AUX_STREAM = 0xD1B54A32D192ED03
KEYS = ("Jr", "p", "elig_n", "elig_list", "count", "arrive", "delivery", "x")
# 256 seeds: a run next to 2^64 - 1 (the seed wraps inside the library), the rest from an ordinary base
SEEDS = [MASK - 3 + q for q in range(4)] + [424242 + q for q in range(252)]


def uniform(seed, i, a, b):
    """Rng::uniform (fjsp_instance.cpp) on draw i: a + (b - a) * ((z >> 11) * 2^-53), every operation rounded to f64."""
    return a + (b - a) * (float(draw(seed, i) >> 11) * (1.0 / 9007199254740992.0))


def draw_py(q, seed):
    """(M, DDT) of instance `seed` under ranges q: draws 0 and 1 of the stream seeded seed ^ AUX_STREAM."""
    aux = (seed & MASK) ^ AUX_STREAM
    return randint(aux, 0, q.M_min, q.M_max), uniform(aux, 1, q.DDT_min, q.DDT_max)


def small_base(**kw):
    d = dict(R_min=3, R_max=5, J_min=2, J_max=3, M=0, p_min=1, p_max=20, N_min=1, N_max=3, S=1, DDT=0.0, t_si_min=100.0, t_si_max=200.0)
    d.update(kw)
    return GenParams(**d)


RANGES = {
    "mpppo": fi.reference_training_ranges("mpppo"),
    "ddqn": fi.reference_training_ranges("ddqn"),
    "point": GenRanges(small_base(), 6, 6, 1.25, 1.25),
}


def same_arrays(a, b, what):
    assert (a.R, a.M, a.K, a.S) == (b.R, b.M, b.K, b.S), what
    assert a.ddt == b.ddt, what
    for key in KEYS:
        assert np.array_equal(getattr(a, key), getattr(b, key)), (what, key)


def test_new_calls_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "fjsp_amd.h")).read()
    lib = _capi.lib()
    for name in NEW_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1], name
    assert "0xD1B54A32D192ED03" in header
    assert "#define FJSP_ABI_VERSION 1" in re.sub(r"[ \t]+", " ", header)
    assert lib.fjsp_abi_version() == 1
    # fjsp_gen_params keeps its layout; the ranges follow it
    assert C.sizeof(GenParams) == 64 and GenRanges.M_min.offset == 64 and GenRanges.DDT_min.offset == 72 and C.sizeof(GenRanges) == 88


def test_reference_training_ranges():
    m, d = RANGES["mpppo"], RANGES["ddqn"]
    assert (m.M_min, m.M_max, d.M_min, d.M_max) == (10, 20, 3, 8)
    for q in (m, d):
        assert (q.DDT_min, q.DDT_max, q.base.S) == (0.5, 1.5, 1)
        assert (q.base.R_min, q.base.R_max, q.base.J_min, q.base.J_max, q.base.p_min, q.base.p_max) == (3, 12, 3, 5, 40, 400)
    assert (m.base.N_min, m.base.N_max, d.base.N_min, d.base.N_max) == (5, 50, 1, 2)
    with pytest.raises(ValueError):
        fi.reference_training_ranges("a3c")


@pytest.mark.parametrize("name", sorted(RANGES))
def test_draw_matches_the_restated_auxiliary_stream(name):
    q = RANGES[name]
    for seed in SEEDS:
        p = fi.draw_params(q, seed)
        assert (p.M, p.DDT) == draw_py(q, seed), (name, seed)
        for f, _ in GenParams._fields_:
            if f not in ("M", "DDT"):
                assert getattr(p, f) == getattr(q.base, f), (name, seed, f)


@pytest.mark.parametrize("name", sorted(RANGES))
def test_generate_drawn_is_draw_then_generate(name):
    q = RANGES[name]
    n = len(SEEDS)
    drawn, fixed = fi.InstanceSet(n), fi.InstanceSet(n)
    for i, seed in enumerate(SEEDS):
        drawn.generate(i, seed, q)
        fixed.generate(i, seed, fi.draw_params(q, seed))
    for i, seed in enumerate(SEEDS):
        a = drawn.arrays(i)
        same_arrays(a, fixed.arrays(i), (name, seed))
        assert (a.M, a.ddt) == draw_py(q, seed), (name, seed)


@pytest.mark.parametrize("name", sorted(RANGES))
def test_addressable_replay_with_the_drawn_parameters(name):
    """The stream csrc/fjsp_generate.hip follows draw by index (replay, tests/test_generate_host.py), with the instance's own
    M and DDT in place of the handle's."""
    q = RANGES[name]
    for seed in SEEDS[:64]:
        M, DDT = draw_py(q, seed)
        g = GenParams.from_buffer_copy(q.base)
        g.M, g.DDT = M, DDT
        a, r = fi.InstanceSet(1).generate(0, seed, q).arrays(0), replay(seed, g)
        assert (a.R, a.M, a.K, a.S) == (r["R"], M, r["K"], 1), (name, seed)
        for key in ("Jr", "p", "elig_n", "elig_list", "count", "arrive", "delivery"):
            assert np.array_equal(getattr(a, key), r[key]), (name, seed, key)


def test_generate_range_takes_ranges():
    q = RANGES["ddqn"]
    s = fi.InstanceSet(8).generate_range(5000, q)
    for i in range(8):
        same_arrays(s.arrays(i), fi.InstanceSet(1).generate(0, 5000 + i, fi.draw_params(q, 5000 + i)).arrays(0), i)


def test_point_range_reproduces_the_fixed_parameter_generator():
    q = RANGES["point"]
    fixed_prm = small_base(M=6, DDT=1.25)
    for i, seed in enumerate(SEEDS):
        p = fi.draw_params(q, seed)
        assert p.M == 6 and p.DDT == 1.25, seed
        same_arrays(fi.InstanceSet(1).generate(0, seed, q).arrays(0), fi.InstanceSet(1).generate(0, seed, fixed_prm).arrays(0), seed)


def test_both_ends_of_a_wide_range_occur():
    q = GenRanges(small_base(), 1, 32, -0.75, 2.5)
    got = [fi.draw_params(q, seed) for seed in SEEDS]
    ms = {p.M for p in got}
    assert min(ms) == 1 and max(ms) == 32 and ms <= set(range(1, 33))
    assert all(q.DDT_min <= p.DDT <= q.DDT_max for p in got)
    assert len({p.DDT for p in got}) == len(got)


# ---- refusals before any device is looked for ------------------------------------------------------------------------------
def ranges(M_min=3, M_max=8, DDT_min=0.5, DDT_max=1.5, **kw):
    d = dict(R_min=10, R_max=10, J_min=3, J_max=5, M=0, p_min=1, p_max=20, N_min=1, N_max=1, S=1, DDT=0.0, t_si_min=100.0, t_si_max=200.0)
    d.update(kw)
    return GenRanges(GenParams(**d), M_min, M_max, DDT_min, DDT_max)


def create(q, n_inst=4, n_envs=4, variant=0, family=-1):
    lib, h = _capi.lib(), C.c_void_p()
    rc = lib.fjsp_env_create_generated_ranges(C.byref(q), n_inst, n_envs, variant, 0, 0, family, 1000, C.byref(h))
    msg = lib.fjsp_last_error().decode()
    if rc == 0:                      # (a GPU machine: the handle exists)
        lib.fjsp_env_destroy(h)
    return rc, msg


INF, NAN = float("inf"), float("nan")
REFUSED = [
    ("M_min = 0", dict(q=ranges(M_min=0)), _capi.FJSP_E_ARG, "M_min"),
    ("M_min < 0", dict(q=ranges(M_min=-2, M_max=4)), _capi.FJSP_E_ARG, "M_min"),
    ("M_max < M_min", dict(q=ranges(M_min=6, M_max=5)), _capi.FJSP_E_ARG, "M_max < M_min"),
    ("DDT_min = -inf", dict(q=ranges(DDT_min=-INF)), _capi.FJSP_E_ARG, "DDT_min"),
    ("DDT_min = nan", dict(q=ranges(DDT_min=NAN)), _capi.FJSP_E_ARG, "DDT_min"),
    ("DDT_max = inf", dict(q=ranges(DDT_max=INF)), _capi.FJSP_E_ARG, "DDT_max"),
    ("DDT_max = nan", dict(q=ranges(DDT_max=NAN)), _capi.FJSP_E_ARG, "DDT_max"),
    ("DDT_max < DDT_min", dict(q=ranges(DDT_min=1.5, DDT_max=0.5)), _capi.FJSP_E_ARG, "DDT_max < DDT_min"),
    ("base: R_max < R_min", dict(q=ranges(R_min=5, R_max=4)), _capi.FJSP_E_ARG, "bad parameters"),
    ("base: p_min = 0", dict(q=ranges(p_min=0)), _capi.FJSP_E_ARG, "bad parameters"),
    ("n_inst <= 0", dict(q=ranges(), n_inst=0), _capi.FJSP_E_ARG, "bad arguments"),
    ("n_envs <= 0", dict(q=ranges(), n_envs=0), _capi.FJSP_E_ARG, "bad arguments"),
    ("family = 2", dict(q=ranges(), family=2), _capi.FJSP_E_ARG, "family"),
    ("unknown variant", dict(q=ranges(), variant=3), _capi.FJSP_E_ARG, "unknown variant"),
    ("M_max = 33", dict(q=ranges(M_min=20, M_max=33)), _capi.FJSP_E_UNSUPPORTED, "M_max"),
    ("S = 2", dict(q=ranges(S=2)), _capi.FJSP_E_UNSUPPORTED, "one order only"),
    ("MO_DFJSP", dict(q=ranges(), variant=4), _capi.FJSP_E_UNSUPPORTED, "MO_DFJSP needs machine data"),
    ("257 operation types", dict(q=ranges(R_min=1, R_max=257, J_min=1, J_max=1)), _capi.FJSP_E_UNSUPPORTED,
     "more than 256 operation types"),
    # one operation of up to 65 535: the delivery time p x DDT / (2 M) reaches 65 535 x 1e5 / 2 > 2^31 on M_min = 1 machine
    ("32-bit clock over the ranges", dict(q=ranges(M_min=1, M_max=32, DDT_min=1.0, DDT_max=1e5, R_min=1, R_max=1, J_min=1, J_max=1, p_max=65535)),
     _capi.FJSP_E_UNSUPPORTED, "DDT_max"),
]


@pytest.mark.parametrize("what,kw,code,text", REFUSED, ids=[r[0] for r in REFUSED])
def test_create_generated_ranges_refuses_before_it_looks_for_a_device(what, kw, code, text):
    rc, msg = create(**kw)
    assert rc == code, (what, rc, msg)
    assert text in msg, (what, msg)
    assert "no HIP device" not in msg


def test_the_clock_bound_is_taken_at_ddt_max_over_m_min():
    """The case above is refused for M_min alone: with 32 machines in every instance the same DDT_max passes the checks."""
    rc, msg = create(ranges(M_min=32, M_max=32, DDT_min=1.0, DDT_max=1e5, R_min=1, R_max=1, J_min=1, J_max=1, p_max=65535))
    assert rc == 0 or (rc == _capi.FJSP_E_HIP and "no HIP device" in msg), (rc, msg)      # a handle, or no device here


def test_draw_and_generate_drawn_refuse_bad_ranges():
    lib = _capi.lib()
    out = GenParams()
    s = fi.InstanceSet(1)
    for q, text in ((ranges(M_min=0), "M_min"), (ranges(M_min=4, M_max=3), "M_max < M_min"), (ranges(DDT_max=NAN), "DDT_max"),
                    (ranges(DDT_min=2.0, DDT_max=1.0), "DDT_max < DDT_min")):
        assert lib.fjsp_gen_draw(C.byref(q), 1, C.byref(out)) == _capi.FJSP_E_ARG and text in lib.fjsp_last_error().decode()
        assert lib.fjsp_instances_generate_drawn(s.handle, 0, 1, C.byref(q)) == _capi.FJSP_E_ARG and text in lib.fjsp_last_error().decode()
    assert lib.fjsp_gen_draw(None, 1, C.byref(out)) == _capi.FJSP_E_ARG
    assert lib.fjsp_instances_generate_drawn(s.handle, 0, 1, C.byref(ranges(R_min=0))) == _capi.FJSP_E_ARG
