"""CPU: the masked refill's two entry points (fjsp_env_regenerate_masked, fjsp_env_instance_seed) are declared, exported and
bound, and refuse a null handle before any HIP call.  What they do on a device: tests/test_gpu_regenerate_masked.py."""
import ctypes as C
import os
import re

from deep_reinforcement_learning_for_fjsp_amd import _capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("fjsp_env_regenerate_masked", "fjsp_env_instance_seed")


def test_new_calls_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "fjsp_amd.h")).read()
    lib = _capi.lib()
    for name in NEW_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1], name
    assert lib.fjsp_abi_version() == 1


def test_a_null_handle_is_refused_before_any_device_is_looked_for():
    lib = _capi.lib()
    seed = C.c_uint64(17)
    assert lib.fjsp_env_regenerate_masked(None, None, 1, None) == _capi.FJSP_E_ARG
    msg = lib.fjsp_last_error().decode()
    assert "fjsp_env_regenerate_masked" in msg and "no HIP device" not in msg and "hip" not in msg.lower(), msg
    assert lib.fjsp_env_instance_seed(None, 0, C.byref(seed)) == _capi.FJSP_E_ARG
    assert seed.value == 17
    assert "fjsp_env_instance_seed" in lib.fjsp_last_error().decode()


def test_the_python_methods_exist_and_regenerate_is_unchanged():
    import inspect
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    assert list(inspect.signature(EnvBatch.regenerate_masked).parameters) == ["self", "seed_base", "mask"]
    assert inspect.signature(EnvBatch.regenerate_masked).parameters["mask"].default is None
    assert list(inspect.signature(EnvBatch.instance_seed).parameters) == ["self", "i"]
    assert list(inspect.signature(EnvBatch.regenerate).parameters) == ["self", "seed_base", "rng_seed"]
