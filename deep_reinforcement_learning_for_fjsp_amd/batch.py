"""EnvBatch: N environments resident in HBM, driven through the C ABI.

PyTorch is plumbing here: it owns the device tensors handed to the library
(`.data_ptr()`) and the stream the kernels are queued on
(`torch.cuda.current_stream()`).  All environment arithmetic happens in
libfjsp_amd.so (csrc/fjsp_kernels.hip); nothing in this module computes a step
on the host.
"""
import ctypes as C
import functools

import numpy as np

import torch

from . import _capi
from ._capi import check, ptr as _ptr

VARIANT_SO_FJSSP = 0
VARIANT_SO_SFJSP = 1
VARIANT_MO_FJSSP_DISCRETES = 2
VARIANT_MO_DFJSP = 4
VARIANT_SO_DFJSP = 5

ST_BAD_TASK_RULE = 1
ST_BAD_MACHINE_RULE = 2
ST_STEP_AFTER_DONE = 4
ST_NO_EVENT = 8
ST_SCHEDULE_OVERFLOW = 16


ENV_SEED_STRIDE = 1000003          # env e draws random.choice from the stream seeded rng_seed + e * ENV_SEED_STRIDE


def _splitmix64(z):
    """numpy uint64 vector form of the splitmix64 finaliser the kernels use (fjsp_kernels.hip)."""
    import numpy as np
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def global_actions(seed, first_env, n_envs, T, n_task_rules, n_machine_rules):
    """uint8[T, n_envs, 2] random rule pairs that are a pure function of (seed, GLOBAL env id, step): a shard
    [first_env, first_env + n_envs) of a larger batch draws exactly what the unsharded batch draws for those
    environments, whatever the number of GPUs."""
    import numpy as np
    g = (np.arange(n_envs, dtype=np.uint64) + np.uint64(first_env))[None, :]
    t = np.arange(T, dtype=np.uint64)[:, None]
    with np.errstate(over="ignore"):
        u = _splitmix64(_splitmix64(np.uint64(seed) + g * np.uint64(0x632BE59BD9B4E019)) + t)
    a0 = ((u >> np.uint64(40)) % np.uint64(n_task_rules)).astype(np.uint8)
    a1 = ((u >> np.uint64(8)) % np.uint64(max(n_machine_rules, 1))).astype(np.uint8)
    return np.ascontiguousarray(np.stack([a0, a1], 2))


def _as_input(name, t, shape, dtype, device):
    """An INPUT tensor of the C ABI: converted to the dtype / device / layout the kernels read, shape enforced
    (the library takes raw pointers: a wrong extent would be an out-of-bounds device access, not an exception)."""
    if t is None:
        return None
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must have shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    if t.dtype != dtype or t.device != device or not t.is_contiguous():
        t = t.to(device=device, dtype=dtype).contiguous()
    return t


def _check_output(name, t, shape, dtype, device):
    """An OUTPUT tensor of the C ABI is written in place: it cannot be converted, only checked."""
    if t is None:
        return None
    if not torch.is_tensor(t):
        raise ValueError("%s must be a torch tensor" % name)
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != device or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s tensor of shape %s on %s, got %s %s on %s%s"
                         % (name, dtype, tuple(shape), device, t.dtype, tuple(t.shape), t.device,
                            "" if t.is_contiguous() else " (not contiguous)"))
    return t


class EnvSnapshot(object):
    """Saved states of n environments (fjsp_snapshot_*; EnvBatch.snapshot / restore).

    On the device: every entry's env record -- the whole episode state the kernels keep -- and, when the batch recorded
    its schedule, the entry's dispatch records.  Next to them, as device tensors: the rows of the batch's `state`,
    `reward` and `done` tensors AS THE LAST CALL LEFT THEM (after step(state=False) or rollout(state=False) the state
    rows are stale, as the record's obs_stale flag says; the next call that returns a state rebuilds it), and `instance`
    int32[n], the instance index (env % n_inst) of every entry.  `env_ids` is the saved env of every entry (numpy, None
    when the snapshot was taken with a device index tensor).  A snapshot loads into any batch that plays the same
    instances with the same variant and kernel family, whatever its N (FJSP_E_ARG otherwise)."""

    def __init__(self, lib, handle, n, n_inst, device, env_ids, instance, state, reward, done):
        self._lib, self._h = lib, handle
        self.n, self.n_inst, self.device = int(n), int(n_inst), device
        self.env_ids, self.instance = env_ids, instance
        self.state, self.reward, self.done = state, reward, done

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.fjsp_snapshot_destroy(h)
            self._h = None

    @property
    def capacity(self):
        """Dispatch-record slots per entry (0: the snapshot holds no schedule records)."""
        return int(self._lib.fjsp_snapshot_capacity(self._h))

    def errors(self):
        """Loads refused since the last call because the entry came from another instance (fjsp_snapshot_errors;
        synchronises)."""
        n = C.c_int64(0)
        check(self._lib.fjsp_snapshot_errors(self._h, C.byref(n)))
        return int(n.value)

    def instance_host(self):
        """int64 numpy array: the instance index of every entry."""
        return self.instance.cpu().numpy().astype(np.int64)

    def to_bytes(self):
        """The snapshot as bytes (device buffer + compatibility fingerprint + the state / reward / done rows)."""
        import io
        n = C.c_int64(0)
        check(self._lib.fjsp_snapshot_to_host(self._h, None, C.byref(n)))
        blob = np.empty(int(n.value), np.uint8)
        check(self._lib.fjsp_snapshot_to_host(self._h, blob.ctypes.data_as(C.c_void_p), C.byref(n)))
        f = io.BytesIO()
        np.savez(f, blob=blob, state=self.state.cpu().numpy(), reward=self.reward.cpu().numpy(), done=self.done.cpu().numpy(),
                 instance=self.instance.cpu().numpy(), n_inst=np.int64(self.n_inst),
                 env_ids=self.env_ids if self.env_ids is not None else np.full(0, -1, np.int64))
        return f.getvalue()

    @classmethod
    def from_bytes(cls, batch, data):
        """A snapshot on `batch`'s device from to_bytes() output; FJSP_E_ARG unless `batch` plays the instances (variant,
        kernel family) the bytes were saved from."""
        import io
        z = np.load(io.BytesIO(data), allow_pickle=False)
        blob = np.ascontiguousarray(z["blob"])
        h = C.c_void_p()
        check(batch._lib.fjsp_snapshot_from_host(batch._h, blob.ctypes.data_as(C.c_void_p), int(blob.size), C.byref(h)))
        dev = batch.device
        env_ids = z["env_ids"] if z["env_ids"].size else None
        return cls(batch._lib, h, int(batch._lib.fjsp_snapshot_size(h)), int(z["n_inst"]), dev, env_ids,
                   torch.as_tensor(z["instance"]).to(dev), torch.as_tensor(z["state"]).to(dev),
                   torch.as_tensor(z["reward"]).to(dev), torch.as_tensor(z["done"]).to(dev))


class EnvBatch(object):
    """fjsp_env handle + the device tensors it writes into."""

    def __init__(self, instances, n_envs, first=0, n_inst=None, variant=VARIANT_SO_FJSSP, device=0, rng_seed=0,
                 first_env=0, kernel_family=None):
        """first_env: GLOBAL id of this batch's environment 0 when the batch is one shard of a larger job (one
        rank of `bench.py --gpus N` / examples/train_ppo.py).  The random.choice stream of an environment is a
        function of its global id, so the traces of a sharded job equal the unsharded job's bit for bit.
        kernel_family: None = the library's choice (row kernels where the batch fits them, unless FJSP_STEP_IMPL=wave),
        0 = one wave per environment, 1 = the row kernels (fjsp_env_create_family; FjspError if the batch does not fit)."""
        if not torch.cuda.is_available():
            raise RuntimeError("EnvBatch needs an MI355X: the environment kernels have no CPU path")
        self._lib = _capi.lib()
        self.instances = instances
        n_inst = len(instances) - first if n_inst is None else n_inst
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        # the stream argument of this batch's calls, self._stream(): _capi.stream on its device, bound as a partial
        # (no Python frame of its own: the per-step call is launch-bound on the host)
        self._stream = functools.partial(_capi.stream, self.device_index)
        self._h = C.c_void_p()
        self.first_env = int(first_env)
        # the kernels seed env e (local) with seed + e * ENV_SEED_STRIDE: shift the base by the shard's offset
        lib_seed = (int(rng_seed) + self.first_env * ENV_SEED_STRIDE) & (2 ** 64 - 1)
        if kernel_family is None:
            check(self._lib.fjsp_env_create(instances.handle, int(first), int(n_inst), int(n_envs), int(variant),
                                            self.device_index, lib_seed, C.byref(self._h)))
        else:
            if kernel_family not in (0, 1):
                raise ValueError("kernel_family must be None, 0 or 1, got %r" % (kernel_family,))
            check(self._lib.fjsp_env_create_family(instances.handle, int(first), int(n_inst), int(n_envs), int(variant),
                                                   self.device_index, lib_seed, int(kernel_family), C.byref(self._h)))
        self.first = int(first)
        self.gen_params = None
        self._bind(n_envs, n_inst, variant, rng_seed)

    def _bind(self, n_envs, n_inst, variant, rng_seed):
        """What every constructor does once the handle exists: sizes, kernel family, the output tensors."""
        self.N = int(n_envs)
        self.n_inst = int(n_inst)
        self.variant = int(variant)
        self.rng_seed = int(rng_seed)
        self.state_size = self._lib.fjsp_env_state_size(self._h)
        self.step_bytes = int(self._lib.fjsp_env_step_bytes(self._h))
        # 1: stepped by the 16-lane-row kernels (csrc/fjsp_group.hip), 0: one wavefront per environment
        self.kernel_family = int(self._lib.fjsp_env_kernel_family(self._h))
        # 1: the fluid LPs of order arrivals are solved on the device with the tableau in LDS (csrc/fjsp_lp_device.hip),
        # 2: on the device with the tableau in global memory (csrc/fjsp_lp_global.hip; FJSP_LP_IMPL=global at create and a
        # tableau beyond the LDS rule but within 256 rows x 1536 columns), 0: on the host
        self.lp_on_device = int(self._lib.fjsp_env_lp_on_device(self._h))
        f64 = dict(dtype=torch.float64, device=self.device)
        self.state = torch.zeros(self.N, self.state_size, **f64)
        self.reward = torch.zeros(self.N, **f64)
        self.done = torch.ones(self.N, dtype=torch.uint8, device=self.device)
        # the per-step call is launch-bound on the host (a few us): pointers of the default outputs and the shape
        # the action tensor must have are prepared once
        self._p_state, self._p_reward, self._p_done = _ptr(self.state), _ptr(self.reward), _ptr(self.done)
        self._act_shape = torch.Size((self.N, 2))

    @classmethod
    def generated(cls, params, n_envs, seed_base, n_inst=None, variant=VARIANT_SO_FJSSP, device=0, rng_seed=0, first_env=0,
                  family=-1):
        """A batch whose instances are generated and solved on the device (fjsp_env_create_generated): env q plays
        instance q % n_inst = what InstanceSet.generate_range(seed_base, params) + solve_fluid() make of seed
        seed_base + first_env + q % n_inst.  params: GenParams, GenRanges (fjsp_env_create_generated_ranges: every
        instance draws its own machine count and due-date tightness; the batch is sized for M_max) or GenOrders
        (fjsp_env_create_generated_orders: its number of orders too; with S_max > 1 the batch plays order arrivals, their
        LPs served as lp_on_device says).  first_env shifts the instance seeds and the env random streams alike, so a
        shard [first_env, first_env + n_envs) is a slice of the one-GPU batch.  There is no InstanceSet (`instances` is
        None; instance_arrays(i) reads an instance back); regenerate() refills the batch in place.  Several orders only
        through GenOrders, and then VARIANT_SO_FJSSP / VARIANT_SO_DFJSP.  VARIANT_MO_DFJSP only with a GenDynamic
        (fjsp_env_create_generated_dynamic: the machine data are generated too, an unplayable instance is drawn again;
        instance_arrays(i) then carries power, idle_power, bk_n, bk and seed_used) and a GenDynamic only with it; with any
        other parameters FjspError(FJSP_E_UNSUPPORTED)."""
        if not torch.cuda.is_available():
            raise RuntimeError("EnvBatch needs an MI355X: the environment kernels have no CPU path")
        if family not in (-1, 0, 1):
            raise ValueError("family must be -1, 0 or 1, got %r" % (family,))
        self = cls.__new__(cls)
        self._lib = _capi.lib()
        self.instances = None
        n_inst = int(n_envs) if n_inst is None else int(n_inst)
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        self._stream = functools.partial(_capi.stream, self.device_index)
        self._h = C.c_void_p()
        self.first_env, self.first = int(first_env), 0
        self.gen_params, self.seed_base, self.family = params, int(seed_base), int(family)
        mask = 2 ** 64 - 1
        lib_seed, lib_base = (int(rng_seed) + self.first_env * ENV_SEED_STRIDE) & mask, (self.seed_base + self.first_env) & mask
        if isinstance(params, _capi.GenDynamic):
            if int(variant) != VARIANT_MO_DFJSP:
                raise _capi.FjspError(_capi.FJSP_E_UNSUPPORTED, "EnvBatch.generated: a GenDynamic makes VARIANT_MO_DFJSP batches only")
            if family == 1:
                raise _capi.FjspError(_capi.FJSP_E_UNSUPPORTED, "EnvBatch.generated: the row kernels do not play MO_DFJSP")
            check(self._lib.fjsp_env_create_generated_dynamic(C.byref(params), n_inst, int(n_envs), self.device_index, lib_seed, lib_base,
                                                              C.byref(self._h)))
            self._bind(n_envs, n_inst, variant, rng_seed)
            return self
        create = (self._lib.fjsp_env_create_generated_orders if isinstance(params, _capi.GenOrders) else
                  self._lib.fjsp_env_create_generated_ranges if isinstance(params, _capi.GenRanges) else self._lib.fjsp_env_create_generated)
        check(create(C.byref(params), n_inst, int(n_envs), int(variant), self.device_index, lib_seed, int(family), lib_base, C.byref(self._h)))
        self._bind(n_envs, n_inst, variant, rng_seed)
        return self

    def regenerate(self, seed_base, rng_seed=None):
        """New instances in place (fjsp_env_regenerate): instance i becomes that of seed seed_base + first_env + i, its
        fluid LP is solved, the fluid tables are rebuilt; every env is left done (call reset()) with its random stream
        restarted from rng_seed (None: the batch's).  No allocation, no host instance set.  Synchronises.  If an
        instance cannot be played (FjspError names it and its seed) the batch refuses every call until a regenerate
        succeeds."""
        if self.gen_params is None:
            raise _capi.FjspError(_capi.FJSP_E_STATE, "regenerate(): the batch was not made by EnvBatch.generated")
        rng_seed = self.rng_seed if rng_seed is None else int(rng_seed)
        mask = 2 ** 64 - 1
        rc = self._lib.fjsp_env_regenerate(self._h, (int(seed_base) + self.first_env) & mask,
                                           (rng_seed + self.first_env * ENV_SEED_STRIDE) & mask)
        # the cached rows are those of the old instances, whatever the outcome
        self.state.zero_(); self.reward.zero_(); self.done.fill_(1)
        check(rc)
        self.seed_base, self.rng_seed = int(seed_base), rng_seed
        self.step_bytes = int(self._lib.fjsp_env_step_bytes(self._h))
        return self

    def regenerate_masked(self, seed_base, mask=None):
        """New instances in place for part of the batch (fjsp_env_regenerate_masked): instance i with mask[i] != 0 (a bool /
        uint8 tensor [n_inst] on the batch's device) becomes that of seed seed_base + first_env + i, and the envs that play it
        are left done with their random streams started over (call reset(mask_of_those_envs)); every other env plays on
        undisturbed.  mask=None: the finished ones -- instance i iff every env q with q % n_inst == i is done.  Returns the
        applied mask, a uint8 device tensor [n_inst].  Synchronises.  After a failure (FjspError names the instance and its
        seed) the batch refuses every call until a regenerate succeeds; the next regenerate_masked makes the failed call's
        instances too."""
        if self.gen_params is None:
            raise _capi.FjspError(_capi.FJSP_E_STATE, "regenerate_masked(): the batch was not made by EnvBatch.generated")
        p_mask = None
        if mask is not None:
            if not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (self.n_inst,) \
                    or mask.device != self.device:
                raise ValueError("regenerate_masked(): mask must be a bool / uint8 tensor [%d] on %s" % (self.n_inst, self.device))
            mask = mask.to(torch.uint8).contiguous()
            p_mask = _ptr(mask)
        applied = torch.zeros(self.n_inst, dtype=torch.uint8, device=self.device)
        # (the call synchronises the device first, so the mask and the zeros above are there when its own stream reads them)
        rc = self._lib.fjsp_env_regenerate_masked(self._h, p_mask, (int(seed_base) + self.first_env) & (2 ** 64 - 1), _ptr(applied))
        # the cached rows of the refreshed envs are those of the old instances, whatever the outcome
        envs = applied.to(torch.bool).repeat((self.N + self.n_inst - 1) // self.n_inst)[:self.N]
        self.state[envs] = 0.0; self.reward[envs] = 0.0; self.done[envs] = 1
        check(rc)
        self.step_bytes = int(self._lib.fjsp_env_step_bytes(self._h))
        return applied

    def instance_seed(self, i):
        """The seed instance i of a generated batch was made of last (fjsp_env_instance_seed), without the first_env shift:
        seed_base + i of the generated() / regenerate() / regenerate_masked() that made it."""
        out = C.c_uint64()
        check(self._lib.fjsp_env_instance_seed(self._h, int(i), C.byref(out)))
        return (int(out.value) - self.first_env) & (2 ** 64 - 1)

    def instance_dims(self, i):
        """dict(R, M, K, S, jobs0, jobs) of instance i, from the InstanceSet or, for a generated batch, the device."""
        if self.instances is not None:
            return self.instances.dims(self.first + int(i))
        d = (C.c_int32 * 6)()
        check(self._lib.fjsp_env_instance_read(self._h, int(i), C.byref(d), None, None, None, None, None, None, None, None, None))
        return dict(R=d[0], M=d[1], K=d[2], S=d[3], jobs0=d[4], jobs=d[5])

    def instance_arrays(self, i):
        """instances.InstanceArrays (with x) of instance i of a generated batch, read back from the device
        (fjsp_env_instance_read); of any other batch, its InstanceSet's arrays."""
        from .instances import InstanceArrays
        if self.instances is not None:
            return self.instances.arrays(self.first + int(i))
        d = self.instance_dims(i)
        R, M, K, S = d["R"], d["M"], d["K"], d["S"]
        Jr, p, elig_n = np.zeros(R, np.int32), np.zeros((K, M), np.int32), np.zeros(K, np.int32)
        elig_list, count = np.zeros((K, M), np.int32), np.zeros((S, R), np.int32)
        arrive, delivery, x = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros((K, M), np.float64)
        ddt = C.c_double()
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        check(self._lib.fjsp_env_instance_read(self._h, int(i), None, ptr(Jr), ptr(p), ptr(elig_n), ptr(elig_list), ptr(count),
                                               ptr(arrive), ptr(delivery), C.byref(ddt), ptr(x)))
        out = InstanceArrays(R, M, K, S, Jr, p, elig_n, elig_list, count, arrive, delivery, ddt.value, x)
        if isinstance(self.gen_params, _capi.GenDynamic):       # the machine data and the seed the instance was made of
            dd, used = (C.c_int32 * 2)(), C.c_uint64()
            check(self._lib.fjsp_env_instance_read_dynamic(self._h, int(i), None, None, None, None, None, C.byref(dd)))
            out.power, out.idle_power, out.bk_n = np.zeros((K, M), np.int32), np.zeros(M, np.int32), np.zeros(M, np.int32)
            out.bk = np.zeros((max(dd[1], 1), 2), np.int32)
            check(self._lib.fjsp_env_instance_read_dynamic(self._h, int(i), ptr(out.power), ptr(out.idle_power), ptr(out.bk_n), ptr(out.bk),
                                                           C.byref(used), None))
            out.bk, out.seed_used = out.bk[:dd[1]], int(used.value)
        return out

    def generated_stats(self):
        """Of the last generated() / regenerate(): dict(instances, lp_device, lp_host, device_pivots, lp_global,
        global_pivots), and `ms`: the milliseconds of the generate kernel, the LP launches, the host LP route, fluid
        tables + reset, the whole call, and the launches of the global-memory simplex (FJSP_LP_IMPL=global; they run on
        the second stream beside lp_device and lp_host).  lp_device counts the LDS simplex alone; device_pivots both."""
        out, ms = (C.c_int64 * 6)(), (C.c_double * 6)()
        check(self._lib.fjsp_env_generated_stats2(self._h, C.byref(out), C.byref(ms)))
        return dict(instances=int(out[0]), lp_device=int(out[1]), lp_host=int(out[2]), device_pivots=int(out[3]),
                    lp_global=int(out[4]), global_pivots=int(out[5]),
                    ms=dict(generate=ms[0], lp_device=ms[1], lp_host=ms[2], tables_reset=ms[3], total=ms[4], lp_global=ms[5]))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.fjsp_env_destroy(h)
            self._h = None

    def row_build(self, fused=False):
        """The row-kernel build (kernel_family 1) that a step (fused=False) or a rollout (fused=True) of this batch runs,
        as the launcher decides it (fjsp_env_row_build): dict(early=0/1, mpc=5/8, resident=0/1).  FjspError for a batch
        of the one-wave-per-environment family."""
        out = (C.c_int32 * 3)()
        check(self._lib.fjsp_env_row_build(self._h, 1 if fused else 0, out))
        return dict(early=int(out[0]), mpc=int(out[1]), resident=int(out[2]))

    def policy_build(self, state_size):
        """The workgroup the in-launch policy kernels (fjsp_env_rollout_policy, fjsp_env_play_policy) run for this batch with
        an actor of `state_size` inputs, as their launchers decide it (fjsp_env_policy_build): dict(envs_per_workgroup=16/8/
        4/2/1, lds_bytes=..., kc=1/2/4).  FjspError (FJSP_E_UNSUPPORTED) for a batch they refuse: order arrivals."""
        out = (C.c_int32 * 3)()
        check(self._lib.fjsp_env_policy_build(self._h, int(state_size), out))
        return dict(envs_per_workgroup=int(out[0]), lds_bytes=int(out[1]), kc=int(out[2]))

    def policy_orders_build(self, state_size):
        """policy_build for a batch with order arrivals, which the segmented entries play (fjsp_env_play_policy_orders,
        fjsp_env_rollout_policy_orders; fjsp_env_policy_orders_build): dict(envs_per_workgroup, lds_bytes, kc, segments = the
        policy launches of one call at most, the largest order count of the batch).  FjspError (FJSP_E_UNSUPPORTED) for a batch
        they refuse: no order arrivals, MO_DFJSP."""
        out = (C.c_int32 * 4)()
        check(self._lib.fjsp_env_policy_orders_build(self._h, int(state_size), out))
        return dict(envs_per_workgroup=int(out[0]), lds_bytes=int(out[1]), kc=int(out[2]), segments=int(out[3]))

    def env_seed(self, e):
        """random.choice stream seed of (local) env e (matches open_env() in fjsp_kernels.hip)."""
        return (self.rng_seed + (self.first_env + e) * ENV_SEED_STRIDE) & (2 ** 64 - 1)

    # -- reset / step ------------------------------------------------------------
    def reset(self, mask=None, out=None):
        """reset(): SO_FJSSP.py:51-76 for every env (or those with mask != 0). Returns f64[N, S]."""
        out = self.state if out is None else _check_output("out", out, (self.N, self.state_size), torch.float64, self.device)
        if mask is not None:
            if torch.is_tensor(mask) and mask.dtype == torch.bool:
                mask = mask.to(torch.uint8)
            mask = _as_input("mask", mask, (self.N,), torch.uint8, self.device)
        check(self._lib.fjsp_env_reset(self._h, _ptr(mask), _ptr(out), self._stream()))
        if mask is None:
            self.done.zero_()
        else:
            self.done.masked_fill_(mask.bool(), 0)
        return out

    def step(self, actions, autoreset=False, state_out=None, reward_out=None, done_out=None, mo=None, state=True,
             trace_out=None):
        """step(action): SO_FJSSP.py:168-265.  actions: uint8[N, 2] device tensor.  For the MO variant
        actions[:, 0] is the flat action and `mo` (f64[N, 4] = w0, w1, completion, tardiness; <= 0 = None)
        carries step()'s extra arguments (MO_FJSSP_discretes.py:88); for MO_DFJSP `mo` is f64[N, 4] =
        reward_policy, completion, tardiness, energy_consumption (MO_DFJSP_breakdown.py:189).
        state=False: no state is returned and the kernel skips the observation (rule policies that never look at
        it); later calls that do return a state are unaffected (the library rebuilds v(t-1) first).
        trace_out: int16[N, 2] tensor that receives the chosen (operation type k, machine m) of every env."""
        if not (torch.is_tensor(actions) and actions.dtype is torch.uint8 and actions.shape == self._act_shape
                and actions.device == self.device and actions.is_contiguous()):
            actions = _as_input("actions", actions, (self.N, 2), torch.uint8, self.device)
        if actions.data_ptr() & 1:                # the kernels read an action pair as one 16-bit word
            actions = actions.clone()
        p_mo = None
        if mo is not None:
            mo = _as_input("mo", mo, (self.N, 4), torch.float64, self.device)
            p_mo = _ptr(mo)
        if state_out is None:
            state_out, p_state = self.state, self._p_state
        else:
            p_state = _ptr(_check_output("state_out", state_out, (self.N, self.state_size), torch.float64, self.device))
        if reward_out is None:
            reward_out, p_reward = self.reward, self._p_reward
        else:
            p_reward = _ptr(_check_output("reward_out", reward_out, (self.N,), torch.float64, self.device))
        if done_out is None:
            done_out, p_done = self.done, self._p_done
        else:
            p_done = _ptr(_check_output("done_out", done_out, (self.N,), torch.uint8, self.device))
        if not state:
            state_out, p_state = None, None
        if trace_out is not None:
            _check_output("trace_out", trace_out, (self.N, 2), torch.int16, self.device)
            rc = self._lib.fjsp_env_step_traced(self._h, C.c_void_p(actions.data_ptr()), p_mo, 1 if autoreset else 0, p_state,
                                                p_reward, p_done, _ptr(trace_out), self._stream())
        else:
            rc = self._lib.fjsp_env_step(self._h, C.c_void_p(actions.data_ptr()), p_mo, 1 if autoreset else 0, p_state,
                                         p_reward, p_done, self._stream())
        if rc < 0:
            check(rc)
        return state_out, reward_out, done_out

    def lp_device_solve(self, env, Q, n_now):
        """Test hook (fjsp_env_lp_device_solve): the device LP solver on one LP of env's instance; returns x[K, M] (numpy)."""
        Q = np.ascontiguousarray(Q, dtype=np.int32); n_now = np.ascontiguousarray(n_now, dtype=np.int32)
        K = Q.shape[0]
        x = np.zeros(K * 64, np.float64)
        check(self._lib.fjsp_env_lp_device_solve(self._h, int(env), Q.ctypes.data_as(C.c_void_p), n_now.ctypes.data_as(C.c_void_p),
                                                 x.ctypes.data_as(C.c_void_p)))
        return x

    def step_async(self, actions, autoreset=False, mo=None):
        """fjsp_env_step_async: like step(), but envs that reach an order arrival park (their fluid LP is solved by
        host threads in the background) while the others keep stepping.  Returns (state, reward, done, ready):
        ready[i] = 1 where this call completed a step of env i.  The action a parked step applies is the one of the
        call in which the env parked (the first ready = 0): that call ran the step up to the arrival.  While the env
        stays parked, and in the call where it comes back with ready = 1, its entry of `actions` is not looked at --
        pair the returned row with the (state, action) of the parking call.
        Call flush_arrivals() before read() / reset() / step() / rollout()."""
        actions = _as_input("actions", actions, (self.N, 2), torch.uint8, self.device)
        if actions.data_ptr() & 1:
            actions = actions.clone()
        mo = _as_input("mo", mo, (self.N, 4), torch.float64, self.device)
        if getattr(self, "ready", None) is None:
            self.ready = torch.zeros(self.N, dtype=torch.uint8, device=self.device)
        check(self._lib.fjsp_env_step_async(self._h, _ptr(actions), _ptr(mo), 1 if autoreset else 0, self._p_state, self._p_reward,
                                            self._p_done, _ptr(self.ready), self._stream()))
        self._last_mo = mo
        return self.state, self.reward, self.done, self.ready

    def flush_arrivals(self, mo=None):
        """Wait for every parked env and finish its step (rows of state / reward / done, ready = 1)."""
        mo = _as_input("mo", mo, (self.N, 4), torch.float64, self.device) if mo is not None else getattr(self, "_last_mo", None)
        if getattr(self, "ready", None) is None:
            self.ready = torch.zeros(self.N, dtype=torch.uint8, device=self.device)
        check(self._lib.fjsp_env_arrivals_flush(self._h, _ptr(mo), self._p_state, self._p_reward, self._p_done, _ptr(self.ready),
                                                self._stream()))
        return self.state, self.reward, self.done, self.ready

    @property
    def lp_cache_hits(self):
        return int(self._lib.fjsp_env_lp_cache_hits(self._h))

    @property
    def parked(self):
        return int(self._lib.fjsp_env_parked(self._h))

    @property
    def async_stats(self):
        """fjsp_env_async_stats, host-side counters of the asynchronous arrival service: (launches whose parked envs went
        to the LP workers, those of them with more than 64 parked envs (second copy), step_async calls that found every
        batch of the ring in flight and waited, most envs parked by one launch).  Zeros before the first step_async
        and on batches without order arrivals.  The ring's length is FJSP_ASYNC_RING (1 ... 32) when the batch is created."""
        out = (C.c_int64 * 4)()
        check(self._lib.fjsp_env_async_stats(self._h, C.byref(out)))
        return tuple(int(v) for v in out)

    def rollout(self, actions, trace=True, rewards=True, mo=None, state=True):
        """T fused steps in one launch. actions: uint8[T, N, 2]. Returns (trace_km i16[T,N,2], reward f64[T,N], state).
        state=False: no final state (the fused kernel then skips the observation)."""
        if not torch.is_tensor(actions):
            actions = torch.as_tensor(actions)
        if actions.dim() != 3:
            raise ValueError("actions must have shape (T, %d, 2), got %s" % (self.N, tuple(actions.shape)))
        actions = _as_input("actions", actions, (actions.shape[0], self.N, 2), torch.uint8, self.device)
        if actions.data_ptr() & 1:
            actions = actions.clone()
        mo = _as_input("mo", mo, (self.N, 4), torch.float64, self.device)
        T = actions.shape[0]
        tr = torch.full((T, self.N, 2), -1, dtype=torch.int16, device=self.device) if trace else None
        rw = torch.zeros(T, self.N, dtype=torch.float64, device=self.device) if rewards else None
        check(self._lib.fjsp_env_rollout(self._h, _ptr(actions), _ptr(mo), int(T), _ptr(tr), _ptr(rw),
                                         _ptr(self.state) if state else None, self._stream()))
        return tr, rw, (self.state if state else None)

    # -- saved states ----------------------------------------------------------------
    def snapshot(self, envs=None, out=None):
        """Save the episode state of envs (None: every env; a host sequence / numpy array, or an int device tensor,
        of env indices) into a new EnvSnapshot, or into `out` (an EnvSnapshot of this fingerprint with as many entries).
        Stream-ordered: no host synchronisation unless `envs` is on the host.  The dispatch records are saved too while
        the batch records its schedule (record_schedule).  Host indices outside [0, N) raise ValueError; a device index
        outside [0, N) leaves an empty entry (instance -1, zero rows) that every restore refuses, and the kernel counts it
        (snap.errors())."""
        valid = None
        if envs is None:
            n, idx, env_ids = self.N, None, np.arange(self.N, dtype=np.int64)
            rows = slice(None)
        elif torch.is_tensor(envs) and envs.device.type != "cpu":
            idx = envs.to(device=self.device, dtype=torch.int32).contiguous().reshape(-1)
            n, env_ids = idx.numel(), None
            valid = (idx >= 0) & (idx < self.N)
            rows = idx.long().clamp(0, self.N - 1)
        else:
            env_ids = np.asarray(envs.cpu() if torch.is_tensor(envs) else envs, dtype=np.int64).reshape(-1)
            if env_ids.size == 0 or env_ids.min() < 0 or env_ids.max() >= self.N:
                raise ValueError("snapshot(): env indices must lie in [0, %d)" % self.N)
            n = env_ids.size
            idx = torch.as_tensor(env_ids.astype(np.int32)).to(self.device)
            rows = idx.long()
        if out is None:
            h = C.c_void_p()
            check(self._lib.fjsp_snapshot_create(self._h, int(n), C.byref(h)))
            snap = EnvSnapshot(self._lib, h, n, self.n_inst, self.device, None, None, None, None, None)
        else:
            if not isinstance(out, EnvSnapshot) or out.n != n:
                raise ValueError("snapshot(out=...): an EnvSnapshot with %d entries is needed" % n)
            snap = out
        check(self._lib.fjsp_snapshot_save(snap._h, self._h, _ptr(idx), self._stream()))
        snap.env_ids = env_ids
        if idx is None:
            snap.instance = torch.arange(self.N, dtype=torch.int32, device=self.device) % self.n_inst
        else:
            snap.instance = idx % self.n_inst
        snap.state, snap.reward, snap.done = self.state[rows].clone(), self.reward[rows].clone(), self.done[rows].clone()
        if valid is not None:          # (the same rule as the kernel: an entry of a bad index is never loaded)
            snap.instance = torch.where(valid, snap.instance, torch.full_like(snap.instance, -1))
            snap.state.masked_fill_(~valid[:, None], 0.0); snap.reward.masked_fill_(~valid, 0.0); snap.done.masked_fill_(~valid, 0)
        return snap

    def restore(self, snap, src=None, check=False, rows=True):
        """Load saved states: env i <- entry src[i] wherever src[i] >= 0 (src: int[N], -1 = keep env i; None: entry i
        for i < snap.n).  The entry must come from an env of the same instance (i % n_inst): a host `src` (or None) is
        checked here, before anything is launched (ValueError); a device `src` is checked by the kernel, which leaves a
        mismatched env untouched and counts it (snap.errors(); check=True calls it and raises ValueError).  The rows of
        `state` / `reward` / `done` are restored with the envs (see EnvSnapshot); rows=False skips them (they are then
        left as they were, not those of the loaded states: for callers that go on with state=False and read(), such as
        the lookahead's branch batch).  Random rules replay bit for bit only in the env slot (and batch rng_seed /
        first_env) the entry was saved from; deterministic rules anywhere."""
        if not isinstance(snap, EnvSnapshot):
            raise ValueError("restore(): an EnvSnapshot is needed")
        if snap.n_inst != self.n_inst:
            raise ValueError("restore(): the snapshot was taken from a batch of %d instances, this one has %d" % (snap.n_inst, self.n_inst))
        if src is None or not (torch.is_tensor(src) and src.device.type != "cpu"):
            if src is None:
                h_src = np.full(self.N, -1, np.int64)
                m = min(self.N, snap.n)
                h_src[:m] = np.arange(m)
            else:
                h_src = np.asarray(src.cpu() if torch.is_tensor(src) else src, dtype=np.int64).reshape(-1)
                if h_src.shape != (self.N,):
                    raise ValueError("restore(): src must have %d entries, got %d" % (self.N, h_src.size))
            use = h_src >= 0
            if np.any(h_src[use] >= snap.n):
                raise ValueError("restore(): src entries must lie in [-1, %d)" % snap.n)
            inst = snap.env_ids % self.n_inst if snap.env_ids is not None else snap.instance_host()
            bad = np.nonzero(use & (inst[np.where(use, h_src, 0)] != np.arange(self.N) % self.n_inst))[0]
            if bad.size:
                raise ValueError("restore(): env %d plays instance %d, entry %d holds instance %d"
                                 % (bad[0], bad[0] % self.n_inst, h_src[bad[0]], inst[h_src[bad[0]]]))
            d_src = None if src is None else torch.as_tensor(h_src.astype(np.int32)).to(self.device)
            s = torch.as_tensor(h_src).to(self.device) if rows else None
        else:
            d_src = src.to(dtype=torch.int32).contiguous().reshape(-1)
            if d_src.numel() != self.N:
                raise ValueError("restore(): src must have %d entries, got %d" % (self.N, d_src.numel()))
            s = d_src.long()
        rc = self._lib.fjsp_snapshot_load(snap._h, self._h, _ptr(d_src), self._stream())
        if rc < 0:
            _capi.check(rc)
        if rows:        # the rows of state / reward / done follow the same rule as the kernel
            ar = torch.arange(self.N, dtype=torch.int64, device=self.device)
            sc = s.clamp(0, snap.n - 1)
            take = (s >= 0) & (s < snap.n) & (snap.instance.long()[sc] == ar % self.n_inst)
            self.state.copy_(torch.where(take[:, None], snap.state[sc], self.state))
            self.reward.copy_(torch.where(take, snap.reward[sc], self.reward))
            self.done.copy_(torch.where(take, snap.done[sc], self.done))
        if check:
            bad = snap.errors()
            if bad:
                raise ValueError("restore(): %d envs were given an entry of another instance and kept their state" % bad)
        return self

    # -- read back -----------------------------------------------------------------
    def read(self):
        """dict of per-env attributes the reference's agents / harnesses read."""
        i32 = dict(dtype=torch.int32, device=self.device)
        out = dict(delay_time_sum=torch.zeros(self.N, dtype=torch.int64, device=self.device),
                   makespan=torch.zeros(self.N, **i32), completion_time=torch.zeros(self.N, **i32),
                   step_time=torch.zeros(self.N, **i32), step_count=torch.zeros(self.N, **i32),
                   done=torch.zeros(self.N, dtype=torch.uint8, device=self.device),
                   status=torch.zeros(self.N, dtype=torch.int32, device=self.device))
        check(self._lib.fjsp_env_read(self._h, _ptr(out["delay_time_sum"]), _ptr(out["makespan"]),
                                      _ptr(out["completion_time"]), _ptr(out["step_time"]), _ptr(out["step_count"]),
                                      _ptr(out["done"]), _ptr(out["status"]), self._stream()))
        if self.variant == VARIANT_MO_DFJSP:
            out["energy_consumption"] = torch.zeros(self.N, dtype=torch.int64, device=self.device)
            check(self._lib.fjsp_env_energy(self._h, _ptr(out["energy_consumption"]), self._stream()))
        return out

    def record_schedule(self, on=True):
        """Start (on=True) or stop recording the dispatched schedule (fjsp_env_record_schedule).  Every env must be
        between episodes: right after construction, after reset() or once every env is done (FJSP_E_STATE otherwise).
        While recording is on, every step / step_async / rollout / fused policy rollout stores one record per dispatch.
        Synchronises the device first, so steps still queued on any stream count."""
        check(self._lib.fjsp_env_record_schedule(self._h, 1 if on else 0))
        self.schedule_capacity = int(self._lib.fjsp_env_schedule_capacity(self._h))
        return self.schedule_capacity

    def schedule(self, out=None):
        """The recorded schedule of every env's current episode (fjsp_env_schedule; SO_FJSSP.py:182-184 per dispatched
        operation).  Returns (table int32[N, cap, 6], length int32[N]) on the device: table[i, s] = (r, j, n, m,
        time_begin, time_end) of env i's s-th dispatch -- kind r, stage j, job number n within kind r, machine m --
        and -1 for s >= length[i].  A finished episode stays readable until the env is reset (explicitly or by
        autoreset at its next step).  deep_reinforcement_learning_for_fjsp_amd.schedule works on it on the host."""
        cap = int(self._lib.fjsp_env_schedule_capacity(self._h))
        if cap == 0:
            raise RuntimeError("schedule(): recording is off; call record_schedule() first")
        if out is None:
            table = torch.empty(self.N, cap, 6, dtype=torch.int32, device=self.device)
        else:
            table = _check_output("out", out, (self.N, cap, 6), torch.int32, self.device)
        length = torch.empty(self.N, dtype=torch.int32, device=self.device)
        check(self._lib.fjsp_env_schedule(self._h, _ptr(table), _ptr(length), self._stream()))
        return table, length

    def decode_capacity(self):
        """Rows of a plan of schedule.decode: the operations of the batch's largest instance (fjsp_schedule_decode_capacity;
        record_schedule()'s capacity, recording on or off)."""
        return int(self._lib.fjsp_schedule_decode_capacity(self._h))

    def decode_group(self):
        """Candidates one workgroup of the decode kernel takes (fjsp_schedule_decode_group); 0: the batch is not decoded."""
        return int(self._lib.fjsp_schedule_decode_group(self._h))

    def decode(self, plan, moves=None, n_cand=1, want_table=False):
        """schedule.decode on this batch's instances: explicit schedules -> objectives, status, tables, lengths."""
        from . import schedule
        return schedule.decode(self, plan, moves, n_cand, want_table)

    def decode_active_group(self):
        """Candidates one workgroup of the active decode kernel takes (fjsp_schedule_decode_active_group): decode_group()."""
        return int(self._lib.fjsp_schedule_decode_active_group(self._h))

    def decode_active_resident(self):
        """Candidates of a decode_active call that are resident at once (fjsp_schedule_decode_active_resident): the bounded
        grid's workgroups x decode_active_group(); the handle's workspace holds 8 x decode_capacity() bytes for each."""
        return int(self._lib.fjsp_schedule_decode_active_resident(self._h))

    def decode_active(self, plan, moves=None, n_cand=1, want_table=False):
        """schedule.decode_active on this batch's instances: explicit schedules decoded with insertion into machine gaps ->
        objectives, status, tables, lengths, inserted rows."""
        from . import schedule
        return schedule.decode_active(self, plan, moves, n_cand, want_table)

    def decode_dyn_group(self):
        """Candidates one workgroup of the MO_DFJSP decode kernel takes (fjsp_schedule_decode_dyn_group); 0: the batch is
        not MO_DFJSP, or a candidate's state exceeds the limit."""
        return int(self._lib.fjsp_schedule_decode_dyn_group(self._h))

    def decode_dyn(self, plan, moves=None, n_cand=1, want_table=False):
        """schedule.decode_dyn on this MO_DFJSP batch's instances: explicit schedules -> (makespan, tardiness, energy),
        status, tables, lengths."""
        from . import schedule
        return schedule.decode_dyn(self, plan, moves, n_cand, want_table)

    def critical(self, table, n_cand=1, max_moves=0):
        """schedule.critical on this batch's instances: tables -> tails, critical flags, one critical path and its moves."""
        from . import schedule
        return schedule.critical(self, table, n_cand, max_moves)

    def search_lds(self):
        """LDS bytes a workgroup of policy_search.local_search takes on this batch (fjsp_schedule_search_lds); 0: the batch
        is not searched (MO_DFJSP, or a working set beyond a CU's LDS)."""
        return int(self._lib.fjsp_schedule_search_lds(self._h))

    def search_dyn_lds(self):
        """LDS bytes a workgroup of policy_search.local_search takes on this MO_DFJSP batch (fjsp_schedule_search_dyn_lds);
        0: the batch is not MO_DFJSP, or an env's working set exceeds a CU's LDS."""
        return int(self._lib.fjsp_schedule_search_dyn_lds(self._h))

    def search_front_lds(self, cap_front=64):
        """LDS bytes a workgroup of policy_search.front_search takes on this batch with cap_front archive slots
        (fjsp_schedule_search_front_lds, either family); 0: an env's working set exceeds a CU's LDS, or cap_front is outside 1..64."""
        return int(self._lib.fjsp_schedule_search_front_lds(self._h, int(cap_front)))

    def evolve_lds(self):
        """LDS bytes a workgroup of policy_search.genetic_search takes on this batch (fjsp_schedule_evolve_lds, either
        family); 0: an env's working set exceeds a CU's LDS."""
        return int(self._lib.fjsp_schedule_evolve_lds(self._h))

    def evolve_active_resident(self):
        """Envs of an evolve_active call that are resident at once (fjsp_schedule_evolve_active_resident):
        decode_active_resident() // 64, the workgroups of its bounded grid; 0 on MO_DFJSP."""
        return int(self._lib.fjsp_schedule_evolve_active_resident(self._h))

    def evolve_active(self, pop_plans, generations, weights=None, mut_rate=6554, seed=0, trace=False):
        """schedule.evolve_active on this batch's instances: the genetic algorithm of schedule.evolve with every individual
        scored by the active decoder -> evolve's dict and the rows each individual of the last generation inserted."""
        from . import schedule
        return schedule.evolve_active(self, pop_plans, generations, weights, mut_rate, seed, trace)

    def set_lp_threads(self, n_threads):
        """Host threads of the order-arrival LP service (0 = all cores).  The asynchronous service builds its worker pool
        at the first step_async and reads this once, there: call it before that."""
        check(self._lib.fjsp_env_set_lp_threads(self._h, int(n_threads)))

    @property
    def lp_solves(self):
        return int(self._lib.fjsp_env_lp_solves(self._h))

    @property
    def lp_device_pivots(self):
        """Simplex pivots executed by the device LP service so far (0 with the host service)."""
        return int(self._lib.fjsp_env_lp_device_pivots(self._h))

    def machine_time_end(self):
        if self.instances is None:
            g = self.gen_params
            mp = int(g.o.r.M_max if isinstance(g, _capi.GenDynamic) else g.r.M_max if isinstance(g, _capi.GenOrders) else
                     g.M_max if isinstance(g, _capi.GenRanges) else g.M)
        else:
            d = self.instances.dims(self.first)
            mp = max(self.instances.dims(self.first + i)["M"] for i in range(self.n_inst)) if self.n_inst > 1 else d["M"]
        out = torch.zeros(self.N, mp, dtype=torch.int32, device=self.device)
        check(self._lib.fjsp_env_machine_time_end(self._h, _ptr(out), int(mp), self._stream()))
        return out

    def fluid_tables(self, i):
        import numpy as np
        d = self.instance_dims(i % self.n_inst)
        K, M = d["K"], d["M"]
        rate = np.zeros((K, M)); arr = np.zeros((K, M)); rs = np.zeros(K); ts = np.zeros(K)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        check(self._lib.fjsp_env_fluid_tables(self._h, int(i), p(rate), p(arr), p(rs), p(ts)))
        return rate, arr, rs, ts
