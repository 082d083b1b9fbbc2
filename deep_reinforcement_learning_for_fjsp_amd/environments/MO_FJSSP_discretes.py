"""Host-side mirror of the reference's environments/MO_FJSSP_discretes.py (the
environment agents/MPPPO/MPPPO.py instantiates): makespan + total tardiness,
18 flat actions = 6 task rules x 3 machine rules (:26), 25-dim state = 7 static
+ 9 observed + 9 deltas (:17-21,48), step(action, weight_vector, completion,
tardiness) (:88), weighted reward (:232-244).  Same kernels as SO_FJSSP with the
variant switch (csrc/fjsp_kernels.hip); nothing is computed in Python.
"""
import torch

from ..batch import VARIANT_MO_FJSSP_DISCRETES
from ..utilities.Utility_Class import MyError
from ._common import BatchedEnv, DropInEnv


class BatchedMOFJSSP(BatchedEnv):
    """Vectorised MO_FJSSP_discretes.  step(actions i64/u8[N], mo f64[N,4]) -> (state[N,25], reward[N], done[N])."""

    action_space = 18
    action_types = "DISCRETE"
    state_size = 25
    variant = VARIANT_MO_FJSSP_DISCRETES

    def _staging(self):
        self._act = torch.zeros(self.N, 2, dtype=torch.uint8, device=self.device)
        self.mo = torch.zeros(self.N, 4, dtype=torch.float64, device=self.device)
        self.mo[:, 1] = 1.0
        self.mo[:, 2:] = -1.0

    def set_objective(self, weight_vector, completion=None, tardiness=None):
        """weight_vector (w_completion, w_tardiness); completion / tardiness: normalisers or None
        (scalars or per-env tensors), as MPPPO.py:161-164 passes them."""
        self.mo[:, 0], self.mo[:, 1] = float(weight_vector[0]), float(weight_vector[1])
        self.mo[:, 2] = -1.0 if completion is None else completion
        self.mo[:, 3] = -1.0 if tardiness is None else tardiness

    def step(self, actions, autoreset=False):
        self._act[:, 0] = actions.to(torch.uint8)
        return self.batch.step(self._act, autoreset=autoreset, mo=self.mo)


class MO_FJSSP_Environment(DropInEnv):
    """Drop-in for environments/MO_FJSSP_discretes.py:12 (N = 1 view of the batched kernels); reset() is
    MO_FJSSP_discretes.py:28-53."""
    variant = VARIANT_MO_FJSSP_DISCRETES
    keeps_ddt = True

    def _start(self, rng_seed, device):
        super()._start(rng_seed, device)
        self.state_size = 25
        self.action_types = "DISCRETE"
        self.action_space = 18
        self.observation_space = 9
        self.static_state_space = 7
        self.actions = tuple((t, m) for t in range(6) for m in range(3))          # :26
        self._mo = torch.zeros(1, 4, dtype=torch.float64, device=self._batch.device)

    def step(self, action, weight_vector=None, completion=None, tardiness=None):
        """MO_FJSSP_discretes.py:88-174"""
        if not 0 <= int(action) < 18:
            raise IndexError("tuple index out of range")                              # self.actions[action] :92
        if weight_vector is None:
            raise TypeError("'NoneType' object is not subscriptable")                 # :240
        w0, w1 = float(weight_vector[0]), float(weight_vector[1])
        unscaled = completion is None or tardiness is None
        if unscaled and w1 != 1 and w0 != 1:
            raise MyError("未定义该回报函数")                                          # :244
        self._act[0, 0] = int(action)
        self._mo[0, 0], self._mo[0, 1] = w0, w1
        self._mo[0, 2] = -1.0 if unscaled else float(completion)
        self._mo[0, 3] = -1.0 if unscaled else float(tardiness)
        return self._step(int if unscaled else float, self._mo)
