"""What the environment classes share; the variant modules hold only what differs.

* ``BatchedEnv``  N environments of one variant stepped by one launch (the fast path);
* ``DropInEnv``   the reference's single-environment class (same constructor / reset() / step() / attributes,
  SURVEY.md 8b) as an N = 1 view of a batch, so the reference's agent loops run against it unchanged.

No environment arithmetic is done in Python.
"""
import random

import numpy as np
import torch

from .. import instances as _inst
from ..batch import EnvBatch, EnvSnapshot, ST_BAD_MACHINE_RULE, ST_BAD_TASK_RULE, ST_NO_EVENT, ST_STEP_AFTER_DONE
from ..utilities.Utility_Class import MyError


def _raise_for_status(status):
    """Per-env status bits -> the exception the reference would have raised."""
    if status & ST_BAD_TASK_RULE:
        raise MyError("报错：未定义该工序动作规则")          # SO_FJSSP.py:297
    if status & ST_BAD_MACHINE_RULE:
        raise MyError("报错：未定义该机器分配规则。")        # SO_FJSSP.py:321
    if status & ST_STEP_AFTER_DONE:
        raise ValueError("step() called on a finished episode (reference: max() arg is an empty sequence)")
    if status & ST_NO_EVENT:
        raise ValueError("min() arg is an empty sequence")   # SO_FJSSP.py:207


class _MachineView(object):
    def __init__(self, time_end):
        self.time_end = time_end


def _instance_set(arrays):
    """An InstanceSet of one instance from the arrays a pickled env carries (fluid solution included)."""
    Jr, p, elig_n, elig_list, count, arrive, delivery, ddt, x = arrays
    return _inst.InstanceSet(1).set_raw(0, Jr, p, elig_n, elig_list, count, arrive, delivery, ddt).set_x(0, x)


# -- pickling / deepcopy with the episode (DropInEnv) ------------------------------------------------------------------
_DEVICE_ATTRS = ("_set", "_batch", "_arrays")          # rebuilt on load
_TENSOR_ATTRS = ("_act", "_mo")                        # staging tensors: travel as host tensors
_OLD_TENSOR_NAMES = {"_actions": "_act"}               # SO_FJSSP_Environment's staging tensor had its own name


class BatchedEnv(object):
    """N environments over one EnvBatch of the subclass's ``variant``.  A subclass sets its class attributes
    (state_size, actions_size or action_space, action_types, variant), _staging() and step()."""

    variant = None

    def __init__(self, instance_set, n_envs=None, first=0, n_inst=None, device=0, rng_seed=0, first_env=0, seed_base=0):
        """instance_set: an InstanceSet, or the generator's parameters (instances.GenParams, instances.GenRanges with
        the machine count and the due-date tightness drawn per instance, or instances.GenOrders with the number of orders
        drawn too -- BatchedSOFJSSP / BatchedSODFJSP then play order arrivals): the batch's instances are
        then generated and solved on the device from seed_base (EnvBatch.generated; n_envs is needed), and
        ``self.batch.regenerate(seed_base)`` refills them in place.  BatchedMODFJSP takes an instances.GenDynamic -- the shop of a
        GenOrders with its machine data -- and only that; the other classes refuse one."""
        if isinstance(instance_set, (_inst.GenParams, _inst.GenRanges, _inst.GenOrders, _inst.GenDynamic)):
            if n_envs is None:
                raise ValueError("n_envs is needed with generator parameters")
            self.batch = EnvBatch.generated(instance_set, n_envs, seed_base, n_inst=n_inst, variant=self.variant, device=device,
                                            rng_seed=rng_seed, first_env=first_env)
            self.N, self.device = self.batch.N, self.batch.device
            self._staging()
            return
        n_inst = len(instance_set) - first if n_inst is None else n_inst
        n_envs = n_inst if n_envs is None else n_envs
        self.batch = EnvBatch(instance_set, n_envs, first=first, n_inst=n_inst, variant=self.variant,
                              device=device, rng_seed=rng_seed, first_env=first_env)
        self.N, self.device = self.batch.N, self.batch.device
        self._staging()

    def _staging(self):
        """Hook: the subclass's staging tensors (its actions as u8 pairs, its step arguments)."""

    def reset(self, mask=None):
        return self.batch.reset(mask)

    def read(self):
        return self.batch.read()

    def record_schedule(self, on=True):
        return self.batch.record_schedule(on)

    def schedule(self, out=None):
        return self.batch.schedule(out)

    def snapshot(self, envs=None, out=None):
        return self.batch.snapshot(envs, out)

    def restore(self, snap, src=None, check=False, rows=True):
        return self.batch.restore(snap, src, check, rows)

    def check_status(self):
        """Raise what the reference would have raised for the first env with an error bit."""
        st = self.batch.read()["status"].cpu().numpy()
        bad = np.nonzero(st)[0]
        if len(bad):
            _raise_for_status(int(st[bad[0]]))


class DropInEnv(object):
    """The reference's environment class as an N = 1 view of a batch of the subclass's ``variant``.

    ``Env(use_instance=True, DDT=..., M=..., S=...)`` draws a random instance (Instance_generate.py:24; pass
    ``seed=`` to make it reproducible), ``Env(use_instance=False, path=..., file_name=...)`` reads a CSV folder
    (SO_DFJSP_instance_read.py:7).  The fluid LP (class_FJSSP.py:246-280) is solved by the library at
    construction; its solution is an input of the kernels.  Without ``seed`` / ``rng_seed`` both are drawn from
    ``random``, in that order.

    A subclass extends _start() with its own attributes and writes step() as: check the action, stage it in
    ``self._act`` (and its step arguments in ``self._mo``), return ``self._step(cast[, self._mo])``.
    """

    variant = None
    keeps_ddt = False                   # the generator's DDT argument becomes self.DDT
    counters = ("step_time", "step_count", "delay_time_sum", "completion_time")      # read() -> attributes

    def __init__(self, use_instance=True, device=0, **kwargs):
        self._set = _inst.InstanceSet(1)
        if use_instance:
            seed = kwargs.get("seed", None)
            seed = random.getrandbits(63) if seed is None else seed
            if self.keeps_ddt:
                self.DDT = kwargs["DDT"]
            self.file_name = "DDT" + str(kwargs["DDT"]) + "_M" + str(kwargs["M"]) + "_S" + str(kwargs["S"])
            self._set.generate(0, seed, _inst.reference_generator_params(kwargs["DDT"], kwargs["M"], kwargs["S"]))
            self._generated(seed)
        else:
            self.path, self.file_name = kwargs["path"], kwargs["file_name"]
            self._set.load_csv(0, self.path, self.file_name)
        self._set.solve_fluid(0, 1, 1)
        rng_seed = kwargs.get("rng_seed", None)
        self._start(random.getrandbits(63) if rng_seed is None else rng_seed, device)

    def _generated(self, seed):
        """Hook: further data a generated instance needs."""

    def _start(self, rng_seed, device):
        """The batch of one env over self._set, and the attributes every variant has."""
        a = self._arrays = self._set.arrays(0)
        self.kind_count, self.machine_count, self.order_count = a.R, a.M, a.S
        self.machine_tuple = tuple(range(a.M))
        self._batch = EnvBatch(self._set, 1, variant=self.variant, device=device, rng_seed=rng_seed)
        self._act = torch.zeros(1, 2, dtype=torch.uint8, device=self._batch.device)
        self.step_count, self.step_time, self.done, self.state = 0, 0, False, None
        self.reward_sum, self.delay_time_sum, self.completion_time = 0, 0, 0

    # pickling: A3C hands whole env objects to worker processes (A3C_v5.1.py:147-156).  The copy carries the episode:
    # it continues from the same point, independently of the original (copy.deepcopy goes the same way)
    def __getstate__(self):
        """The env's instance (arrays, machine data), its batch's construction arguments, its Python-side attributes
        and a snapshot of the episode on the device (EnvSnapshot.to_bytes)."""
        a = self._set.arrays(0)
        dyn = (a.power, a.idle_power, a.bk_n, a.bk) if hasattr(a, "power") else None
        b = self._batch
        attrs = {k: v for k, v in self.__dict__.items() if k not in _DEVICE_ATTRS and k not in _TENSOR_ATTRS}
        tensors = {k: getattr(self, k).cpu() for k in _TENSOR_ATTRS if hasattr(self, k)}
        return dict(arrays=(a.Jr, a.p, a.elig_n, a.elig_list, a.count, a.arrive, a.delivery, a.ddt, a.x), dynamic=dyn,
                    variant=b.variant, device=b.device_index, rng_seed=b.rng_seed, attrs=attrs, tensors=tensors,
                    episode=b.snapshot().to_bytes())

    def __setstate__(self, st):
        """A new batch of one env on the same instance and random stream (slot 0, same rng_seed: random rules
        continue bit for bit), the attributes, and the episode loaded into it."""
        self._set = _instance_set(st["arrays"])
        if st["dynamic"] is not None:
            self._set.set_dynamic(0, *st["dynamic"])
        self._arrays = self._set.arrays(0)
        self._batch = EnvBatch(self._set, 1, variant=st["variant"], device=st["device"], rng_seed=st["rng_seed"])
        self.__dict__.update(st["attrs"])
        for k, v in st["tensors"].items():
            setattr(self, _OLD_TENSOR_NAMES.get(k, k), v.to(self._batch.device))
        self._batch.restore(EnvSnapshot.from_bytes(self._batch, st["episode"]))

    def _refresh(self):
        vals = {k: int(v.item()) for k, v in self._batch.read().items()}
        for k in self.counters:
            setattr(self, k, vals[k])
        return vals

    def reset(self):
        self.state = self._batch.reset()[0].cpu().numpy().copy()
        self.done, self.reward_sum = False, 0
        self._refresh()
        return self.state

    def _step(self, cast, mo=None):
        """One step of the staged action, then the reference's step tail: the error it would have raised, the new
        state, the reward as ``cast`` makes it, the reward sum and done."""
        st, rw, dn = self._batch.step(self._act, mo=mo)
        vals = self._refresh()
        if vals["status"]:
            _raise_for_status(vals["status"])
        self.state = st[0].cpu().numpy().copy()
        self.reward = cast(float(rw[0].item()))
        self.reward_sum += self.reward
        self.done = bool(dn[0].item())
        return self.state, self.reward, self.done

    @property
    def machine_dict(self):
        te = self._batch.machine_time_end()[0].cpu().numpy()
        return {m: _MachineView(int(te[m])) for m in self.machine_tuple}
