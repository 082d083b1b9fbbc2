"""CPU: the saved-state entry points of the C ABI (exports, header, ctypes signatures) and the lookahead's argument
checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNAPSHOT_FUNCS = ("fjsp_snapshot_create", "fjsp_snapshot_destroy", "fjsp_snapshot_size", "fjsp_snapshot_capacity",
                  "fjsp_snapshot_save", "fjsp_snapshot_load", "fjsp_snapshot_errors", "fjsp_snapshot_to_host",
                  "fjsp_snapshot_from_host")


def test_snapshot_symbols_are_exported_and_declared(built):
    from deep_reinforcement_learning_for_fjsp_amd._build import LIB_PATH
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    header = open(os.path.join(REPO, "include", "fjsp_amd.h")).read()
    for f in SNAPSHOT_FUNCS:
        assert f in exported, f
        assert re.search(r"\b%s\s*\(" % f, header), f
    assert "typedef struct fjsp_snapshot fjsp_snapshot;" in header


def test_create_family_is_exported_and_checks_its_argument(built):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    S = _capi.SIGNATURES
    assert S["fjsp_env_create_family"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                    C.c_uint64, C.c_int32, C.POINTER(C.c_void_p)])
    header = open(os.path.join(REPO, "include", "fjsp_amd.h")).read()
    assert re.search(r"\bfjsp_env_create_family\s*\(", header)
    lib = _capi.lib()
    h = C.c_void_p()
    for family in (-2, 2):          # checked before anything else, no device needed
        assert lib.fjsp_env_create_family(None, 0, 1, 4, 0, 0, 0, family, C.byref(h)) == -1
    assert not h.value


def test_snapshot_capi_signatures():
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    S = _capi.SIGNATURES
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    pp = C.POINTER(C.c_void_p)
    assert S["fjsp_snapshot_create"] == (C.c_int, [vp, i32, pp])
    assert S["fjsp_snapshot_destroy"] == (None, [vp])
    assert S["fjsp_snapshot_save"] == (C.c_int, [vp, vp, vp, vp])
    assert S["fjsp_snapshot_load"] == (C.c_int, [vp, vp, vp, vp])
    assert S["fjsp_snapshot_errors"] == (C.c_int, [vp, C.POINTER(i64)])
    assert S["fjsp_snapshot_to_host"] == (C.c_int, [vp, vp, C.POINTER(i64)])
    assert S["fjsp_snapshot_from_host"] == (C.c_int, [vp, vp, i64, pp])
    for f in SNAPSHOT_FUNCS:
        assert f in S


def test_snapshot_source_is_in_the_build():
    from deep_reinforcement_learning_for_fjsp_amd import _build
    assert "fjsp_snapshot.hip" in _build.HIP_SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, "fjsp_snapshot.hip"))


def test_lookahead_candidates():
    from deep_reinforcement_learning_for_fjsp_amd import lookahead as L
    from deep_reinforcement_learning_for_fjsp_amd.batch import VARIANT_MO_FJSSP_DISCRETES, VARIANT_SO_FJSSP, VARIANT_SO_SFJSP
    p = L.candidate_pairs([(0, 1), (4, 3)], VARIANT_SO_FJSSP)
    assert p.dtype == np.uint8 and p.tolist() == [[0, 1], [4, 3]]
    assert L.candidate_pairs([3, 17], VARIANT_MO_FJSSP_DISCRETES).tolist() == [[3, 0], [17, 0]]
    with pytest.raises(ValueError):
        L.candidate_pairs([], VARIANT_SO_FJSSP)
    with pytest.raises(ValueError):
        L.candidate_pairs([3], VARIANT_SO_FJSSP)                 # pairs needed
    with pytest.raises(ValueError):
        L.candidate_pairs([(1, 2)], VARIANT_SO_SFJSP)             # flat actions needed
    with pytest.raises(ValueError):
        L.candidate_pairs([(1, 300)], VARIANT_SO_FJSSP)


@pytest.mark.parametrize("variant,good,bad", [
    (0, [(5, 4), (0, 0)], [(6, 0), (0, 5), (6, 5)]),              # SO_FJSSP: task rules 0..5, machine rules 0..4
    (5, [(5, 4)], [(6, 0), (0, 5)]),                              # SO_DFJSP: the same actions
    (4, [(11, 9), (0, 0)], [(12, 0), (0, 10)]),                   # MO_DFJSP: 12 x 10
    (1, [19, 0], [20, 255]),                                      # SO_SFJSP: 20 flat actions
    (2, [17, 0], [18, 19]),                                       # MO_FJSSP_discretes: 18 flat actions
])
def test_lookahead_rejects_actions_the_variant_does_not_have(variant, good, bad):
    """A candidate outside the variant's rules would leave its branch envs with an error bit and never done: refused
    before anything is created or launched."""
    from deep_reinforcement_learning_for_fjsp_amd import lookahead as L
    assert len(L.candidate_pairs(good, variant)) == len(good)
    for c in bad:
        with pytest.raises(ValueError):
            L.candidate_pairs([c], variant)
    with pytest.raises(ValueError):
        L.candidate_pairs(good, 3)                                # no such variant


def test_lookahead_branch_shape():
    from deep_reinforcement_learning_for_fjsp_amd import lookahead as L
    assert L.check_branch_shape(512, 64, 20) == 10240
    with pytest.raises(ValueError):
        L.check_branch_shape(100, 64, 20)                         # N not a multiple of the instance count
    with pytest.raises(ValueError):
        L.check_branch_shape(128, 64, 0)


def test_lookahead_objective_names():
    import torch
    from deep_reinforcement_learning_for_fjsp_amd import lookahead as L

    class _B(object):
        N = 3

        def read(self):
            return dict(makespan=torch.tensor([5, 6, 7], dtype=torch.int32),
                        delay_time_sum=torch.tensor([1, 2, 3], dtype=torch.int64))

    assert L.objective_values(_B(), "makespan").tolist() == [5.0, 6.0, 7.0]
    assert L.objective_values(_B(), "tardiness").tolist() == [1.0, 2.0, 3.0]
    assert L.objective_values(_B(), lambda r: r["makespan"] + r["delay_time_sum"]).tolist() == [6.0, 8.0, 10.0]
    with pytest.raises(ValueError):
        L.objective_values(_B(), "energy")                       # not a MO_DFJSP batch
    with pytest.raises(ValueError):
        L.objective_values(_B(), "throughput")
