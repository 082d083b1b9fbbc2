"""ctypes binding of include/fjsp_amd.h (libfjsp_amd.so).

The library is the product: if it is missing or a symbol is absent this module
raises -- there is no Python/CPU fallback for the accelerated path.
"""
import ctypes as C
import os

# PyTorch-ROCm ships its own libamdhip64; the process must hold ONE HIP runtime, the one torch's device tensors and
# streams belong to.  Importing torch before the library is loaded makes the loader resolve the library's HIP symbols
# against that runtime (loaded the other way round, the system runtime under /opt/rocm comes up next to torch's and
# sees no device).
import torch

from ._build import LIB_PATH

_lib = None

# name -> (restype, argtypes); keep in step with include/fjsp_amd.h
_vp, _i32, _i64, _u64, _dbl, _cp = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double, C.c_char_p
_pp = C.POINTER(C.c_void_p)

# fjsp_status (include/fjsp_amd.h): what a call returns instead of 0
FJSP_E_ARG, FJSP_E_IO, FJSP_E_FORMAT, FJSP_E_LP, FJSP_E_UNSUPPORTED, FJSP_E_HIP, FJSP_E_STATE = -1, -2, -3, -4, -5, -6, -7


class GenParams(C.Structure):
    """fjsp_gen_params (Instance_generate.py:39-66 distributions)."""
    _fields_ = [("R_min", _i32), ("R_max", _i32), ("J_min", _i32), ("J_max", _i32), ("M", _i32),
                ("p_min", _i32), ("p_max", _i32), ("N_min", _i32), ("N_max", _i32), ("S", _i32),
                ("DDT", _dbl), ("t_si_min", _dbl), ("t_si_max", _dbl)]


class GenRanges(C.Structure):
    """fjsp_gen_ranges: GenRanges(base, M_min, M_max, DDT_min, DDT_max) -- the machine count and the due-date tightness are
    drawn per instance (base.M and base.DDT are not read)."""
    _fields_ = [("base", GenParams), ("M_min", _i32), ("M_max", _i32), ("DDT_min", _dbl), ("DDT_max", _dbl)]


class GenOrders(C.Structure):
    """fjsp_gen_orders: GenOrders(r, S_min, S_max) -- a GenRanges and the number of orders, drawn per instance as well
    (r.base.S is not read)."""
    _fields_ = [("r", GenRanges), ("S_min", _i32), ("S_max", _i32)]


class GenMachine(C.Structure):
    """fjsp_gen_machine: the machine data of an MO_DFJSP shop -- processing power per eligible pair, idle power per machine,
    up to W_max breakdown windows per machine, each a gap of working time and a length."""
    _fields_ = [("pw_min", _i32), ("pw_max", _i32), ("idle_min", _i32), ("idle_max", _i32), ("W_max", _i32),
                ("gap_min", _i32), ("gap_max", _i32), ("len_min", _i32), ("len_max", _i32)]


class GenDynamic(C.Structure):
    """fjsp_gen_dynamic: GenDynamic(o, m, redraws) -- a GenOrders, a GenMachine and the number of further attempts for an
    instance with a machine that no operation is eligible on (0 ... FJSP_GEN_MAX_REDRAWS)."""
    _fields_ = [("o", GenOrders), ("m", GenMachine), ("redraws", _i32)]


FJSP_GEN_MAX_WINDOWS, FJSP_GEN_MAX_REDRAWS = 2047, 16


class ActorParams(C.Structure):
    """fjsp_actor_params: device pointers to the f32 parameters of a state_size -> 128 -> 128 -> n_actions actor."""
    _fields_ = [("w1", _vp), ("b1", _vp), ("w2", _vp), ("b2", _vp), ("w3", _vp), ("b3", _vp),
                ("state_size", _i32), ("hidden", _i32), ("n_actions", _i32)]


SIGNATURES = {
    "fjsp_last_error": (_cp, []),
    "fjsp_abi_version": (C.c_int, []),
    "fjsp_instances_create": (C.c_int, [_i32, _pp]),
    "fjsp_instances_destroy": (None, [_vp]),
    "fjsp_instances_count": (C.c_int, [_vp]),
    "fjsp_instances_load_csv": (C.c_int, [_vp, _i32, _cp, _cp]),
    "fjsp_instances_generate": (C.c_int, [_vp, _i32, _u64, C.POINTER(GenParams)]),
    "fjsp_gen_draw": (C.c_int, [C.POINTER(GenRanges), _u64, C.POINTER(GenParams)]),
    "fjsp_instances_generate_drawn": (C.c_int, [_vp, _i32, _u64, C.POINTER(GenRanges)]),
    "fjsp_gen_draw_orders": (C.c_int, [C.POINTER(GenOrders), _u64, C.POINTER(GenParams)]),
    "fjsp_instances_generate_orders": (C.c_int, [_vp, _i32, _u64, C.POINTER(GenOrders)]),
    "fjsp_gen_dynamic_seed": (C.c_int, [C.POINTER(GenDynamic), _u64, C.POINTER(_u64)]),
    "fjsp_gen_draw_dynamic": (C.c_int, [C.POINTER(GenDynamic), _u64, C.POINTER(GenParams)]),
    "fjsp_instances_generate_dynamic": (C.c_int, [_vp, _i32, _u64, C.POINTER(GenDynamic)]),
    "fjsp_instances_set_raw": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _dbl]),
    "fjsp_instances_dims": (C.c_int, [_vp, _i32, C.POINTER(_i32 * 6)]),
    "fjsp_instances_get": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_dbl), _vp]),
    "fjsp_instances_dynamic_dims": (C.c_int, [_vp, _i32, C.POINTER(_i32 * 2)]),
    "fjsp_instances_get_dynamic": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp]),
    "fjsp_instances_set_dynamic": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp]),
    "fjsp_instances_solve_fluid": (C.c_int, [_vp, _i32, _i32, _i32]),
    "fjsp_instances_set_x": (C.c_int, [_vp, _i32, _vp]),
    "fjsp_fluid_lp": (C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, C.POINTER(_dbl)]),
    "fjsp_env_create": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _u64, _pp]),
    "fjsp_env_create_family": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _u64, _i32, _pp]),
    "fjsp_env_create_generated": (C.c_int, [C.POINTER(GenParams), _i32, _i32, _i32, _i32, _u64, _i32, _u64, _pp]),
    "fjsp_env_create_generated_ranges": (C.c_int, [C.POINTER(GenRanges), _i32, _i32, _i32, _i32, _u64, _i32, _u64, _pp]),
    "fjsp_env_create_generated_orders": (C.c_int, [C.POINTER(GenOrders), _i32, _i32, _i32, _i32, _u64, _i32, _u64, _pp]),
    "fjsp_env_create_generated_dynamic": (C.c_int, [C.POINTER(GenDynamic), _i32, _i32, _i32, _u64, _u64, _pp]),
    "fjsp_env_instance_read_dynamic": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, C.POINTER(_u64), C.POINTER(_i32 * 2)]),
    "fjsp_env_regenerate": (C.c_int, [_vp, _u64, _u64]),
    "fjsp_env_regenerate_masked": (C.c_int, [_vp, _vp, _u64, _vp]),
    "fjsp_env_instance_seed": (C.c_int, [_vp, _i32, C.POINTER(_u64)]),
    "fjsp_env_generated_stats": (C.c_int, [_vp, C.POINTER(_i64 * 4)]),
    "fjsp_env_generated_times": (C.c_int, [_vp, C.POINTER(_dbl * 5)]),
    "fjsp_env_generated_stats2": (C.c_int, [_vp, C.POINTER(_i64 * 6), C.POINTER(_dbl * 6)]),
    "fjsp_env_instance_read": (C.c_int, [_vp, _i32, C.POINTER(_i32 * 6), _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_dbl), _vp]),
    "fjsp_env_destroy": (None, [_vp]),
    "fjsp_env_num_envs": (C.c_int, [_vp]),
    "fjsp_env_state_size": (C.c_int, [_vp]),
    "fjsp_env_device": (C.c_int, [_vp]),
    "fjsp_env_reset": (C.c_int, [_vp, _vp, _vp, _vp]),
    "fjsp_env_step": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "fjsp_env_step_traced": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "fjsp_env_step_async": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "fjsp_env_arrivals_flush": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fjsp_env_parked": (_i64, [_vp]),
    "fjsp_env_async_stats": (C.c_int, [_vp, C.POINTER(_i64 * 4)]),
    "fjsp_env_lp_cache_hits": (_i64, [_vp]),
    "fjsp_env_rollout": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "fjsp_env_read": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fjsp_env_machine_time_end": (C.c_int, [_vp, _vp, _i32, _vp]),
    "fjsp_env_record_schedule": (C.c_int, [_vp, _i32]),
    "fjsp_env_schedule_capacity": (C.c_int, [_vp]),
    "fjsp_env_schedule": (C.c_int, [_vp, _vp, _vp, _vp]),
    "fjsp_env_energy": (C.c_int, [_vp, _vp, _vp]),
    "fjsp_snapshot_create": (C.c_int, [_vp, _i32, _pp]),
    "fjsp_snapshot_destroy": (None, [_vp]),
    "fjsp_snapshot_size": (C.c_int, [_vp]),
    "fjsp_snapshot_capacity": (C.c_int, [_vp]),
    "fjsp_snapshot_save": (C.c_int, [_vp, _vp, _vp, _vp]),
    "fjsp_snapshot_load": (C.c_int, [_vp, _vp, _vp, _vp]),
    "fjsp_snapshot_errors": (C.c_int, [_vp, C.POINTER(_i64)]),
    "fjsp_snapshot_to_host": (C.c_int, [_vp, _vp, C.POINTER(_i64)]),
    "fjsp_snapshot_from_host": (C.c_int, [_vp, _vp, _i64, _pp]),
    "fjsp_env_fluid_tables": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp]),
    "fjsp_env_step_bytes": (_i64, [_vp]),
    "fjsp_env_kernel_family": (_i32, [_vp]),
    "fjsp_env_row_build": (C.c_int, [_vp, _i32, _vp]),
    "fjsp_env_policy_build": (C.c_int, [_vp, _i32, _vp]),
    "fjsp_env_policy_orders_build": (C.c_int, [_vp, _i32, _vp]),
    "fjsp_env_set_lp_threads": (C.c_int, [_vp, _i32]),
    "fjsp_env_lp_solves": (_i64, [_vp]),
    "fjsp_env_lp_on_device": (_i32, [_vp]),
    "fjsp_lp_global_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "fjsp_env_lp_device_pivots": (_i64, [_vp]),
    "fjsp_env_lp_device_solve": (_i32, [_vp, _i32, _vp, _vp, _vp]),
    "fjsp_pyset_and_order": (C.c_int, [C.c_uint32, _vp, _i32, _i32, _vp]),
    "fjsp_rollout_create": (C.c_int, [_i32, _i32, _i32, _i32, _pp]),
    "fjsp_rollout_destroy": (None, [_vp]),
    "fjsp_rollout_append": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fjsp_rollout_returns": (C.c_int, [_vp, _dbl, _vp]),
    "fjsp_rollout_returns_normalised": (C.c_int, [_vp, C.c_double, _i32, _i32, _vp, _vp]),
    "fjsp_rollout_clear": (C.c_int, [_vp]),
    "fjsp_rollout_len": (C.c_int, [_vp]),
    "fjsp_rollout_ptr": (_vp, [_vp, _i32]),
    "fjsp_actor_forward": (C.c_int, [C.POINTER(ActorParams), _vp, _i32, _vp, _vp]),
    "fjsp_env_rollout_policy": (C.c_int, [_vp, _vp, C.POINTER(ActorParams), _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fjsp_env_play_policy": (C.c_int, [_vp, C.POINTER(ActorParams), _i32, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _vp]),
    "fjsp_env_rollout_policy_orders": (C.c_int, [_vp, _vp, C.POINTER(ActorParams), _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fjsp_env_play_policy_orders": (C.c_int, [_vp, C.POINTER(ActorParams), _i32, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp,
                                              _vp, _vp, _vp]),
    "fjsp_ppo_partials": (C.c_int, [_i32]),
    "fjsp_ppo_actor_loss": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, C.c_float, _vp, _vp, _vp, _vp, _vp]),
    "fjsp_ppo_critic_loss": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "fjsp_relu_bwd_bias": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp]),
    "fjsp_adam_clip_step": (C.c_int, [_vp, _vp, _vp, _vp, _i32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _vp, _vp, _vp]),
    "fjsp_mlp_train_groups": (C.c_int, [_i32]),
    "fjsp_mlp_train_pass": (C.c_int, [_i32, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, C.c_float, _vp, _i32, _vp, _vp, _vp, _vp]),
    "fjsp_mlp_train_step": (C.c_int, [_i32, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, C.c_float, _vp, _i32, _vp, _vp, _vp, _vp, _vp,
                                      C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _vp, _vp, _vp]),
    "fjsp_mlp_train_step_values": (C.c_int, [_i32, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, C.c_float, _vp, _i32, _vp, _vp, _vp, _vp, _vp,
                                             C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _vp, _vp, _vp, _vp]),
    "fjsp_policy_sample": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, C.c_uint64, _vp, _vp, _vp, _vp]),
    "fjsp_beam_select": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "fjsp_pareto_select": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "fjsp_schedule_decode": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "fjsp_schedule_decode_capacity": (C.c_int, [_vp]),
    "fjsp_schedule_decode_group": (C.c_int, [_vp]),
    "fjsp_schedule_decode_active": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fjsp_schedule_decode_active_group": (C.c_int, [_vp]),
    "fjsp_schedule_decode_active_resident": (C.c_int, [_vp]),
    "fjsp_schedule_decode_dyn": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "fjsp_schedule_decode_dyn_group": (C.c_int, [_vp]),
    "fjsp_schedule_critical": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "fjsp_schedule_search": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _u64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fjsp_schedule_search_lds": (C.c_int, [_vp]),
    "fjsp_schedule_search_dyn": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _u64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fjsp_schedule_search_dyn_lds": (C.c_int, [_vp]),
    "fjsp_schedule_search_front": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i32, _i32, _u64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                             _vp, _vp, _vp, _vp]),
    "fjsp_schedule_search_front_lds": (C.c_int, [_vp, _i32]),
    "fjsp_schedule_evolve": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i32, _u64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fjsp_schedule_evolve_lds": (C.c_int, [_vp]),
    "fjsp_schedule_evolve_active": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i32, _u64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fjsp_schedule_evolve_active_resident": (C.c_int, [_vp]),
    "fjsp_search_draws": (C.c_int, [_u64, _i64, C.c_uint32, _i32, C.POINTER(C.c_uint64)]),
    "fjsp_policy_pair_sample": (C.c_int, [_i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
}


class FjspError(RuntimeError):
    """A C-ABI call returned a negative FJSP_E_* code."""

    def __init__(self, code, message):
        super().__init__("libfjsp_amd error %d: %s" % (code, message))
        self.code = code


def lib():
    """Load libfjsp_amd.so (built in-tree by __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: the HIP extension is the product and there is no fallback. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` from the repo root." % LIB_PATH)
    handle = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(handle, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if handle.fjsp_abi_version() != 1:
        raise ImportError("libfjsp_amd.so ABI version mismatch")
    _lib = handle
    return _lib


def check(rc):
    if rc < 0:
        raise FjspError(rc, lib().fjsp_last_error().decode("utf-8", "replace"))
    return rc


def ptr(t):
    """The device pointer argument of a tensor, or None (NULL) for None."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream(device_index):
    """The stream argument: the raw handle of torch's CURRENT stream on the device, looked up per call (callers switch
    streams and capture graphs; torch.cuda.current_stream() builds a Stream object first, five times the cost)."""
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(device_index))
