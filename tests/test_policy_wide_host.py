"""CPU: fjsp_env_policy_build, the accessor of the in-launch policy kernels' workgroup geometry: export, header, ctypes
signature, and the argument errors that need no device."""
import ctypes as C
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_policy_build_is_exported_and_declared(built):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    from deep_reinforcement_learning_for_fjsp_amd._build import LIB_PATH
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "fjsp_env_policy_build" in set(line.split()[-1] for line in out.splitlines() if line.strip())
    header = open(os.path.join(REPO, "include", "fjsp_amd.h")).read()
    assert re.search(r"\bint\s+fjsp_env_policy_build\s*\(\s*const\s+fjsp_env\s*\*\s*e\s*,\s*int32_t\s+state_size\s*,\s*int32_t\s*\*\s*out3\s*\)",
                     header)
    assert _capi.SIGNATURES["fjsp_env_policy_build"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p])
    fn = _capi.lib().fjsp_env_policy_build
    assert fn.restype == C.c_int and fn.argtypes == _capi.SIGNATURES["fjsp_env_policy_build"][1]


def test_policy_build_bad_args_error_without_a_gpu(built):
    """A null handle, a null output and a state size outside 1..32 are FJSP_E_ARG before the handle is looked at."""
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    lib = _capi.lib()
    out3 = (C.c_int32 * 3)(-7, -7, -7)
    assert lib.fjsp_env_policy_build(None, 20, out3) == _capi.FJSP_E_ARG
    assert b"fjsp_env_policy_build" in lib.fjsp_last_error()
    fake = C.cast(C.create_string_buffer(256), C.c_void_p)      # never dereferenced: the calls below fail their argument check
    assert lib.fjsp_env_policy_build(fake, 20, None) == _capi.FJSP_E_ARG
    for S in (0, -1, 33):
        assert lib.fjsp_env_policy_build(fake, S, out3) == _capi.FJSP_E_ARG, S
        assert b"state_size" in lib.fjsp_last_error()
    assert list(out3) == [-7, -7, -7]


def test_documents_name_the_new_limits():
    """The header no longer states the 64-operation-type limit of the policy entries, and INTEGRATION.md lists the accessor."""
    header = open(os.path.join(REPO, "include", "fjsp_amd.h")).read()
    assert "at most 64 operation types" not in header and "more than 64 operation types" not in header
    assert "fjsp_env_policy_build" in open(os.path.join(REPO, "INTEGRATION.md")).read()
