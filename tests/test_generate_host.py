"""Device-generated batches, the part that needs no GPU: the four new calls exist in header, library and binding;
fjsp_env_create_generated refuses what it cannot play before it looks for a device; and the generator's draw order,
restated in Python as an ADDRESSABLE stream (draw i is a pure function of (seed, i)), against the host library --
the stream csrc/fjsp_generate.hip follows."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from deep_reinforcement_learning_for_fjsp_amd import _capi, instances as fi
from deep_reinforcement_learning_for_fjsp_amd._capi import GenParams

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("fjsp_env_create_generated", "fjsp_env_regenerate", "fjsp_env_generated_stats", "fjsp_env_instance_read")
MASK = (1 << 64) - 1


# ---- the generator as an addressable stream (fjsp_instance.cpp: Rng, generate) ------------------------------------------
def draw(seed, i):
    """Draw i (0-based) of the splitmix64 stream seeded `seed`: the state advances by a constant per draw."""
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def randint(seed, i, a, b):
    return a + (((draw(seed, i) >> 32) * (b - a + 1)) >> 32)


def replay(seed, g):
    """generate(seed, g) for S == 1 with every draw taken by its index."""
    seed &= MASK
    M = g.M
    R = randint(seed, 0, g.R_min, g.R_max)
    Jr = [randint(seed, 1 + r, g.J_min, g.J_max) for r in range(R)]
    K = sum(Jr)
    n, off, pos = [], [], 1 + R
    for k in range(K):                       # the one serial chain: n[k] places the draws of k + 1
        n.append(randint(seed, pos, 1, M)); off.append(pos + 1)
        pos += 1 + n[k]
    poff = [pos + sum(n[:k]) for k in range(K)]
    elig_list, p = np.zeros((K, M), np.int32), np.zeros((K, M), np.int32)
    for k in range(K):                       # independent of each other given off / poff
        perm = list(range(M))
        for i in range(n[k]):
            j = randint(seed, off[k] + i, i, M - 1)      # randint(a, a) still takes its draw
            perm[i], perm[j] = perm[j], perm[i]
        elig_list[k, :n[k]] = perm[:n[k]]
        for i in range(n[k]):
            p[k, perm[i]] = randint(seed, poff[k] + i, g.p_min, g.p_max)
    base = pos + sum(n)
    count = [randint(seed, base + r, g.N_min, g.N_max) for r in range(R)]
    acc, k = 0.0, 0
    for r in range(R):
        for _ in range(Jr[r]):
            t = float(sum(int(p[k, m]) for m in elig_list[k, :n[k]])) / float(n[k])
            acc = acc + t * float(count[r])
            k += 1
    delivery = int(acc * g.DDT / float(M * 2))
    return dict(R=R, M=M, K=K, Jr=np.array(Jr, np.int32), p=p, elig_n=np.array(n, np.int32), elig_list=elig_list,
                count=np.array(count, np.int32).reshape(1, R), arrive=np.zeros(1, np.int32),
                delivery=np.array([delivery], np.int32))


def empty_machine(a):
    """SO_DFJSP cannot play an instance with a machine no operation type is eligible on (check_instance)."""
    return bool(np.any((np.asarray(a["p"]) > 0).sum(0) == 0))


PARAM_SETS = {
    "bench_10x5": fi.bench_10x5_params(),
    "reference_m10": fi.reference_generator_params(1.0, 10, 1),
    "multi_job": GenParams(R_min=3, R_max=5, J_min=2, J_max=3, M=6, p_min=1, p_max=20, N_min=2, N_max=4, S=1, DDT=1.5,
                           t_si_min=100.0, t_si_max=200.0),
}


@pytest.mark.parametrize("name", sorted(PARAM_SETS))
def test_replay_of_the_draw_order_matches_the_host_generator(name):
    g = PARAM_SETS[name]
    s = fi.InstanceSet(64).generate_range(123456789, g)
    for i in range(64):
        a, r = s.arrays(i), replay(123456789 + i, g)
        assert (a.R, a.M, a.K, a.S) == (r["R"], r["M"], r["K"], 1), (name, i)
        for key in ("Jr", "p", "elig_n", "elig_list", "count", "arrive", "delivery"):
            assert np.array_equal(getattr(a, key), r[key]), (name, i, key)


def test_replay_wraps_the_seed_like_the_library():
    g = PARAM_SETS["bench_10x5"]
    s = fi.InstanceSet(1).generate(0, MASK - 2, g)
    assert np.array_equal(s.arrays(0).p, replay(MASK - 2, g)["p"])


# ---- header, library, binding ---------------------------------------------------------------------------------------------
def test_new_calls_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "fjsp_amd.h")).read()
    lib = _capi.lib()
    for name in NEW_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1], name
    assert "#define FJSP_ABI_VERSION 1" in re.sub(r"[ \t]+", " ", header)
    assert lib.fjsp_abi_version() == 1


# ---- refusals before any device is looked for --------------------------------------------------------------------------------
def params(**kw):
    d = dict(R_min=10, R_max=10, J_min=3, J_max=5, M=5, p_min=1, p_max=20, N_min=1, N_max=1, S=1, DDT=1.0,
             t_si_min=100.0, t_si_max=200.0)
    d.update(kw)
    return GenParams(**d)


def create(prm, n_inst=4, n_envs=4, variant=0, family=-1):
    lib, h = _capi.lib(), C.c_void_p()
    rc = lib.fjsp_env_create_generated(C.byref(prm), n_inst, n_envs, variant, 0, 0, family, 1000, C.byref(h))
    msg = lib.fjsp_last_error().decode()
    if rc == 0:                      # (a GPU machine: the handle exists)
        lib.fjsp_env_destroy(h)
    return rc, msg


REFUSED = [
    ("R_max < R_min", dict(prm=params(R_min=5, R_max=4)), _capi.FJSP_E_ARG, "bad parameters"),
    ("M <= 0", dict(prm=params(M=0)), _capi.FJSP_E_ARG, "bad parameters"),
    ("n_inst <= 0", dict(prm=params(), n_inst=0), _capi.FJSP_E_ARG, "bad arguments"),
    ("n_envs <= 0", dict(prm=params(), n_envs=0), _capi.FJSP_E_ARG, "bad arguments"),
    ("unknown variant", dict(prm=params(), variant=3), _capi.FJSP_E_ARG, "unknown variant"),
    ("S = 2", dict(prm=params(S=2)), _capi.FJSP_E_UNSUPPORTED, "one order only"),
    ("MO_DFJSP", dict(prm=params(), variant=4), _capi.FJSP_E_UNSUPPORTED, "MO_DFJSP needs machine data"),
    ("257 operation types", dict(prm=params(R_min=1, R_max=257, J_min=1, J_max=1)), _capi.FJSP_E_UNSUPPORTED,
     "more than 256 operation types"),
    # 50 kinds x 5 operations x 200 jobs = 50 000 operations of up to 60 000: the clock can pass 2^31
    ("32-bit clock", dict(prm=params(R_min=50, R_max=50, J_max=5, N_max=200, p_max=60000)), _capi.FJSP_E_UNSUPPORTED,
     "32-bit clocks"),
    # one step past the limits of the record's fields (their accepted twins: tests/test_generator_limit_cases_host.py)
    ("M = 33", dict(prm=params(M=33)), _capi.FJSP_E_UNSUPPORTED, "more than 32 machines"),
    ("p_max = 65536", dict(prm=params(p_max=65536)), _capi.FJSP_E_UNSUPPORTED, "processing time above 65535"),
    ("J_max = 256", dict(prm=params(R_min=1, R_max=1, J_min=256, J_max=256)), _capi.FJSP_E_UNSUPPORTED, "more than 255 operations in a kind"),
]


@pytest.mark.parametrize("what,kw,code,text", REFUSED, ids=[r[0] for r in REFUSED])
def test_create_generated_refuses_before_it_looks_for_a_device(what, kw, code, text):
    rc, msg = create(**kw)
    assert rc == code, (what, rc, msg)
    assert text in msg, (what, msg)
    assert "no HIP device" not in msg


def test_regenerate_and_stats_need_a_handle():
    lib = _capi.lib()
    out = (C.c_int64 * 4)()
    assert lib.fjsp_env_regenerate(None, 1, 2) == _capi.FJSP_E_ARG
    assert lib.fjsp_env_generated_stats(None, C.byref(out)) == _capi.FJSP_E_ARG
    assert lib.fjsp_env_instance_read(None, 0, None, None, None, None, None, None, None, None, None, None) == _capi.FJSP_E_ARG
