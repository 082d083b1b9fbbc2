"""MO_DFJSP instances with their machine data from a seed (fjsp_gen_dynamic), the part that needs no GPU: the new calls
exist in header, library and binding; the shop of fjsp_instances_generate_dynamic is fjsp_instances_generate_orders of the seed
it was made of; the machine data against a restatement of the stream's positions, their ranges and their shape; the redraw
of instances that leave a machine idle; and what the generators and fjsp_env_create_generated_dynamic refuse before any
device is looked for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from deep_reinforcement_learning_for_fjsp_amd import _capi, instances as fi
from deep_reinforcement_learning_for_fjsp_amd._capi import GenDynamic, GenMachine, GenOrders, GenParams, GenRanges
from tests.test_generate_host import MASK, draw, randint
from tests.test_generate_ranges_host import same_arrays

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("fjsp_gen_dynamic_seed", "fjsp_gen_draw_dynamic", "fjsp_instances_generate_dynamic", "fjsp_env_create_generated_dynamic",
             "fjsp_env_instance_read_dynamic")
MACHINE_STREAM, REDRAW_STREAM = 0xA0761D6478BD642F, 0xE7037ED1A0B428DB
DYN_KEYS = ("power", "idle_power", "bk_n", "bk")


def machine(W_max=3, **kw):
    d = dict(pw_min=10, pw_max=200, idle_min=1, idle_max=9, W_max=W_max, gap_min=1, gap_max=60, len_min=1, len_max=30)
    d.update(kw)
    return GenMachine(**d)


def dyn(S_min=1, S_max=3, M_min=3, M_max=6, DDT_min=0.5, DDT_max=1.5, redraws=8, mc=None, **kw):
    d = dict(R_min=3, R_max=3, J_min=2, J_max=3, M=0, p_min=5, p_max=30, N_min=2, N_max=3, S=0, DDT=0.0, t_si_min=100.0, t_si_max=200.0)
    d.update(kw)
    return GenDynamic(GenOrders(GenRanges(GenParams(**d), M_min, M_max, DDT_min, DDT_max), S_min, S_max), mc or machine(), redraws)


def redraw_shape(redraws=8, W_max=3):
    """Two kinds of two operations on eight machines: about three instances in ten leave a machine idle."""
    return dyn(S_min=1, S_max=2, M_min=8, M_max=8, DDT_min=1.0, DDT_max=1.0, redraws=redraws, mc=machine(W_max),
               R_min=2, R_max=2, J_min=2, J_max=2, N_min=1, N_max=2)


# Found by find_redraw_base() below over seed bases 1000, 1008, ...: the first whose eight instances hold at least two with an
# idle machine in attempt 0; the test states which ones it found
REDRAW_BASE, REDRAW_N = 1000, 8


def idle_in_attempt_0(q, seed):
    a = fi.InstanceSet(1).generate(0, seed, q.o).arrays(0)
    return bool(np.any((a.p > 0).sum(0) == 0))


def find_redraw_base(first=1000, n=REDRAW_N):
    q = redraw_shape()
    base = first
    while sum(idle_in_attempt_0(q, base + i) for i in range(n)) < 2:
        base += n
    return base


def same_dynamic(a, b, what):
    for key in DYN_KEYS:
        x, y = getattr(a, key), getattr(b, key)
        assert x.shape == y.shape and np.array_equal(x, y), (what, key)


def machine_data_py(a, seed, g):
    """The machine data of the shop `a` of seed `seed`, every draw taken by its position (fjsp_gen_machine, include/fjsp_amd.h)."""
    ms = (seed & MASK) ^ MACHINE_STREAM
    M, K, W = a.M, a.K, g.W_max
    idle = np.array([randint(ms, m, g.idle_min, g.idle_max) for m in range(M)], np.int32)
    bk_n = np.array([randint(ms, M + m, 0, W) for m in range(M)], np.int32)
    power = np.array([[randint(ms, 2 * M + k * M + m, g.pw_min, g.pw_max) if a.p[k, m] > 0 else 0 for m in range(M)] for k in range(K)], np.int32)
    bk = []
    for m in range(M):
        t = 0
        for w in range(int(bk_n[m])):
            pos = 2 * M + K * M + 2 * (m * W + w)
            st = t + randint(ms, pos, g.gap_min, g.gap_max)
            t = st + randint(ms, pos + 1, g.len_min, g.len_max)
            bk.append((st, t))
    return power, idle, bk_n, np.array(bk, np.int32).reshape(-1, 2)


def test_new_calls_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "fjsp_amd.h")).read()
    flat = re.sub(r"[ \t]+", " ", header)
    lib = _capi.lib()
    for name in NEW_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1], name
    assert re.search(r"}\s*fjsp_gen_machine\s*;", header) and re.search(r"}\s*fjsp_gen_dynamic\s*;", header)
    assert "#define FJSP_GEN_MACHINE_STREAM 0x%XULL" % MACHINE_STREAM in flat and "#define FJSP_GEN_REDRAW_STREAM 0x%XULL" % REDRAW_STREAM in flat
    assert "#define FJSP_GEN_MAX_WINDOWS %d" % _capi.FJSP_GEN_MAX_WINDOWS in flat and "#define FJSP_GEN_MAX_REDRAWS %d" % _capi.FJSP_GEN_MAX_REDRAWS in flat
    assert 32 * _capi.FJSP_GEN_MAX_WINDOWS <= 65535            # M_max x W_max indexes the record's u16 window offsets
    assert "#define FJSP_ABI_VERSION 1" in flat and lib.fjsp_abi_version() == 1
    assert C.sizeof(GenOrders) == 96 and C.sizeof(GenMachine) == 36
    assert GenDynamic.m.offset == 96 and GenDynamic.redraws.offset == 132 and C.sizeof(GenDynamic) == 136


def test_reference_dynamic_ranges():
    q = fi.reference_dynamic_ranges("hmpsac")
    m = q.m
    assert (m.pw_min, m.pw_max, m.idle_min, m.idle_max, m.W_max) == (10, 200, 1, 9, 0) and q.redraws > 0
    assert (m.gap_min, m.gap_max, m.len_min, m.len_max) == (50, 400, 5, 60)
    assert bytes(q.o) == bytes(fi.reference_order_ranges("hmpsac"))
    w = fi.reference_dynamic_ranges("hmpsac", max_windows=2, window_gap=(3, 4), window_len=(5, 6)).m
    assert (w.W_max, w.gap_min, w.gap_max, w.len_min, w.len_max) == (2, 3, 4, 5, 6)
    assert bytes(fi.reference_machine_params(2, (3, 4), (5, 6))) == bytes(w)
    with pytest.raises(ValueError):
        fi.reference_dynamic_ranges("da3c")


# ---- 1: the shop ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["drawn", "redraw"])
def test_base_arrays_are_those_of_the_order_generator(name):
    q = dyn() if name == "drawn" else redraw_shape()
    redrawn = 0
    for seed in [MASK - 1, MASK] + list(range(5000, 5062)):
        a = fi.InstanceSet(1).generate(0, seed, q).arrays(0)
        used = fi.dynamic_seed(q, seed)
        assert (used == seed & MASK) == (not idle_in_attempt_0(q, seed)), seed
        redrawn += used != seed & MASK
        same_arrays(a, fi.InstanceSet(1).generate(0, used, q.o).arrays(0), seed)
        assert bytes(fi.draw_params(q, seed)) == bytes(fi.draw_params(q.o, used)), seed
        assert not np.any((a.p > 0).sum(0) == 0), seed
    print("%s: %d of 64 instances were drawn again" % (name, redrawn))
    assert name == "drawn" or redrawn > 0


# ---- 2: ranges and shape ----------------------------------------------------------------------------------------------------
def test_machine_data_positions_ranges_and_shape():
    q = dyn()
    g = q.m
    counts = []
    for seed in range(7000, 7064):
        a = fi.InstanceSet(1).generate(0, seed, q).arrays(0)
        power, idle, bk_n, bk = machine_data_py(a, fi.dynamic_seed(q, seed), g)
        for key, want in zip(DYN_KEYS, (power, idle, bk_n, bk)):
            got = getattr(a, key)
            assert got.shape == want.shape and np.array_equal(got, want), (seed, key)
        el = a.p > 0
        assert np.all((a.power[el] >= g.pw_min) & (a.power[el] <= g.pw_max)) and np.all(a.power[~el] == 0), seed
        assert a.idle_power.shape == (a.M,) and np.all((a.idle_power >= g.idle_min) & (a.idle_power <= g.idle_max)), seed
        assert np.all((a.bk_n >= 0) & (a.bk_n <= g.W_max)) and a.bk.shape == (int(a.bk_n.sum()), 2), seed
        off = 0
        for m in range(a.M):
            end = 0
            for st, en in a.bk[off:off + a.bk_n[m]]:
                assert g.gap_min <= st - end <= g.gap_max and g.len_min <= en - st <= g.len_max, (seed, m)
                end = en
            off += int(a.bk_n[m])
        counts += list(a.bk_n)
    assert 0 in counts and g.W_max in counts


# ---- 3: purity --------------------------------------------------------------------------------------------------------------
def test_machine_data_are_a_pure_function_of_the_seed():
    q0, q3 = dyn(mc=machine(0)), dyn(mc=machine(3))
    for seed in range(7000, 7016):
        a, b = fi.InstanceSet(1).generate(0, seed, q3).arrays(0), fi.InstanceSet(1).generate(0, seed, q3).arrays(0)
        same_arrays(a, b, seed); same_dynamic(a, b, seed)
        z = fi.InstanceSet(1).generate(0, seed, q0).arrays(0)
        same_arrays(z, a, seed)
        assert np.array_equal(z.power, a.power) and np.array_equal(z.idle_power, a.idle_power), seed
        assert z.bk.shape == (0, 2) and not z.bk_n.any(), seed


# ---- 4: redraw --------------------------------------------------------------------------------------------------------------
def test_redraw():
    assert find_redraw_base() == REDRAW_BASE
    q = redraw_shape()
    idle = [i for i in range(REDRAW_N) if idle_in_attempt_0(q, REDRAW_BASE + i)]
    print("seed base %d: attempt 0 leaves a machine idle in instances %s" % (REDRAW_BASE, idle))
    assert len(idle) >= 2
    s = fi.InstanceSet(REDRAW_N).generate_range(REDRAW_BASE, q)
    for i in range(REDRAW_N):
        seed = REDRAW_BASE + i
        a, used = s.arrays(i), fi.dynamic_seed(q, seed)
        assert (used != seed) == (i in idle), i
        assert not np.any((a.p > 0).sum(0) == 0), i
        if i in idle:       # the seeds of the attempts: draws of the redraw stream, never a neighbour's seed
            attempts = [draw(seed ^ REDRAW_STREAM, j) for j in range(q.redraws)]
            assert used in attempts and all(idle_in_attempt_0(q, t) for t in attempts[:attempts.index(used)]), i
            assert abs(used - seed) > REDRAW_N
        twin = fi.InstanceSet(1).generate(0, used, q).arrays(0)         # the whole instance of that seed, machine data included
        same_arrays(a, twin, i); same_dynamic(a, twin, i)
        assert fi.dynamic_seed(q, used) == used
    lib, none = _capi.lib(), redraw_shape(redraws=0)
    t = fi.InstanceSet(REDRAW_N)
    for i in range(REDRAW_N):
        rc = lib.fjsp_instances_generate_dynamic(t.handle, i, REDRAW_BASE + i, C.byref(none))
        msg = lib.fjsp_last_error().decode()
        if i in idle:
            assert rc == _capi.FJSP_E_UNSUPPORTED and "instance %d (seed %d)" % (i, REDRAW_BASE + i) in msg and "redraws = 0" in msg, (i, rc, msg)
        else:
            assert rc == 0, (i, msg)
    with pytest.raises(_capi.FjspError) as err:
        fi.InstanceSet(REDRAW_N).generate_range(REDRAW_BASE, none)
    assert err.value.code == _capi.FJSP_E_UNSUPPORTED and "instance %d (seed %d)" % (idle[0], REDRAW_BASE + idle[0]) in str(err.value)


# ---- 5: refusals before any device is looked for ------------------------------------------------------------------------------
def create(q, n_inst=4, n_envs=4):
    lib, h = _capi.lib(), C.c_void_p()
    rc = lib.fjsp_env_create_generated_dynamic(C.byref(q), n_inst, n_envs, 0, 0, 1000, C.byref(h))
    msg = lib.fjsp_last_error().decode()
    if rc == 0:                      # (a GPU machine: the handle exists)
        lib.fjsp_env_destroy(h)
    return rc, msg


ARG, UNS = _capi.FJSP_E_ARG, _capi.FJSP_E_UNSUPPORTED
# (name, parameters, code, text, refused by the host generator too: a bound of the parameters alone)
REFUSED = [
    ("W_max above FJSP_GEN_MAX_WINDOWS", dyn(mc=machine(2048)), UNS, "W_max above 2047", True),
    ("W_max < 0", dyn(mc=machine(-1)), ARG, "W_max", True),
    ("gap_min < 1", dyn(mc=machine(gap_min=0)), ARG, "gap_min", True),
    ("gap_max < gap_min", dyn(mc=machine(gap_min=5, gap_max=4)), ARG, "gap_max < gap_min", True),
    ("len_min < 1", dyn(mc=machine(len_min=0)), ARG, "len_min", True),
    ("len_max < len_min", dyn(mc=machine(len_min=5, len_max=4)), ARG, "len_max < len_min", True),
    ("idle_min < 0", dyn(mc=machine(idle_min=-1)), ARG, "idle_min", True),
    ("idle_max < idle_min", dyn(mc=machine(idle_min=5, idle_max=4)), ARG, "idle_max < idle_min", True),
    ("pw_min < 1", dyn(mc=machine(pw_min=0)), ARG, "pw_min", True),
    ("pw_max < pw_min", dyn(mc=machine(pw_min=20, pw_max=10)), ARG, "pw_max < pw_min", True),
    ("pw_max > 65535", dyn(mc=machine(pw_max=65536)), UNS, "pw_max above 65535", True),
    ("pw_max x p_max > 2^31 - 1", dyn(mc=machine(pw_max=65535), p_max=32769), UNS, "pw_max x p_max", True),         # 65535 x 32769 = 2^31 + 32767
    ("last window end > 2^31 - 1", dyn(mc=machine(2047, gap_max=1000000, len_max=50000)), UNS, "W_max x (gap_max + len_max)", True),
    ("redraws < 0", dyn(redraws=-1), ARG, "redraws", True),
    ("redraws above the cap", dyn(redraws=17), UNS, "redraws above 16", True),
    ("the order range's own bounds", dyn(S_min=0), ARG, "S_min", True),
    # 9 operation types x 3 jobs x 3 orders of 30: without windows the clock is 2 430 + 400; 6 x 2047 x 170 000 = 2.09e9 of windows,
    # times 9 jobs per kind, pass 2^31 (the last window ends at 2047 x 170 060 < 2^31)
    ("32-bit clock with every window", dyn(mc=machine(2047, len_max=170000)), UNS, "M_max x W_max x len_max", False),
    ("S_max = 17", dyn(S_max=17), UNS, "16 orders (S_max)", False),
    ("more than 32 machines", dyn(M_max=33), UNS, "32 machines", False),
    ("J_max = 255", dyn(R_min=1, R_max=1, J_min=255, J_max=255), UNS, "more than 254 operations in a kind (J_max)", False),
]


@pytest.mark.parametrize("what,q,code,text,host", REFUSED, ids=[r[0] for r in REFUSED])
def test_refusals_name_the_field(what, q, code, text, host):
    rc, msg = create(q)
    assert rc == code and text in msg and "no HIP device" not in msg, (what, rc, msg)
    if host:
        lib, s, out, used = _capi.lib(), fi.InstanceSet(1), GenParams(), C.c_uint64()
        for call in (lambda: lib.fjsp_instances_generate_dynamic(s.handle, 0, 1, C.byref(q)),
                     lambda: lib.fjsp_gen_draw_dynamic(C.byref(q), 1, C.byref(out)),
                     lambda: lib.fjsp_gen_dynamic_seed(C.byref(q), 1, C.byref(used))):
            assert call() == code and text in lib.fjsp_last_error().decode(), what


def test_accepted_parameters_and_bad_arguments():
    ok = lambda rc, msg: rc == 0 or (rc == _capi.FJSP_E_HIP and "no HIP device" in msg)
    assert ok(*create(dyn()))
    assert ok(*create(dyn(mc=machine(0))))
    assert ok(*create(dyn(mc=machine(2047, len_max=1000))))      # the clock case above with shorter windows
    assert ok(*create(redraw_shape(redraws=16)))
    rc, msg = create(dyn(), n_inst=0)
    assert rc == ARG and "bad arguments" in msg
    lib, h = _capi.lib(), C.c_void_p()
    assert lib.fjsp_env_create_generated_dynamic(None, 4, 4, 0, 0, 1000, C.byref(h)) == ARG
    assert lib.fjsp_instances_generate_dynamic(fi.InstanceSet(1).handle, 0, 1, None) == ARG
    assert lib.fjsp_gen_dynamic_seed(C.byref(dyn()), 1, None) == ARG


def test_the_older_entry_points_name_the_new_one():
    lib, h = _capi.lib(), C.c_void_p()
    q = dyn()
    prm = GenParams.from_buffer_copy(q.o.r.base)
    prm.M, prm.S, prm.DDT = 4, 1, 1.0
    for call, arg in ((lib.fjsp_env_create_generated, prm), (lib.fjsp_env_create_generated_ranges, q.o.r), (lib.fjsp_env_create_generated_orders, q.o)):
        assert call(C.byref(arg), 4, 4, 4, 0, 0, -1, 1000, C.byref(h)) == UNS
        msg = lib.fjsp_last_error().decode()
        assert "MO_DFJSP needs machine data" in msg and "fjsp_env_create_generated_dynamic" in msg, msg
