"""Host-side mirror of the reference's environments/SO_SFJSP.py (the environment
agents/DDQN/DDQN.py instantiates): makespan objective, 20 flat actions = 4 task
rules x 5 machine rules (:25), 18-dim state = 9 observed + 9 deltas (:14-17,64-83),
reward -(delta completion_time) / fluid_completed_time (:216-220).  Same kernels
as SO_FJSSP, instantiated for this variant (csrc/fjsp_kernels.hip).
"""
import torch

from ..batch import VARIANT_SO_SFJSP
from ._common import BatchedEnv, DropInEnv


class BatchedSOSFJSP(BatchedEnv):
    """Vectorised SO_SFJSP.  step(actions[N]) -> (state[N,18], reward[N], done[N]) device tensors."""

    action_space = 20
    action_types = "DISCRETE"
    state_size = 18
    variant = VARIANT_SO_SFJSP

    def _staging(self):
        self._act = torch.zeros(self.N, 2, dtype=torch.uint8, device=self.device)

    def step(self, actions, autoreset=False):
        self._act[:, 0] = actions.to(torch.uint8)
        return self.batch.step(self._act, autoreset=autoreset)


class SO_SFJSP_Environment(DropInEnv):
    """Drop-in for environments/SO_SFJSP.py:11 (N = 1 view of the batched kernels); reset() is SO_SFJSP.py:27-52."""
    variant = VARIANT_SO_SFJSP

    def _start(self, rng_seed, device):
        super()._start(rng_seed, device)
        self.state_size = 18
        self.action_types = "DISCRETE"
        self.observation_space = 9
        self.static_state_space = 0
        self.action_space = 20
        self.actions = tuple((t, m) for t in range(4) for m in range(5))          # :25

    def step(self, action):
        """SO_SFJSP.py:85-167"""
        if not 0 <= int(action) < 20:
            raise IndexError("tuple index out of range")                              # self.actions[action] :87
        self._act[0, 0] = int(action)
        return self._step(float)
