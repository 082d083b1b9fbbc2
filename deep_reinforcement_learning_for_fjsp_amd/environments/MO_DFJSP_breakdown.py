"""Host-side mirror of the reference's environments/MO_DFJSP_breakdown.py (and of
environments/MO_DFJSP.py, which is the same environment without breakdown windows):
the dynamic multi-objective shop -- new orders arrive mid-episode (:281-296),
machines break down (:204-231), objectives are makespan, total tardiness and
energy (:249-256), 12 task rules x 10 machine rules (:32,357-428), 30-dim state
= 15 observed + 15 deltas (:35,94-118), step(action, reward_policy, completion,
tardiness, energy_consumption) (:189), reward policies 0..3 (:430-447).

Same kernels as SO_FJSSP with the MO_DFJSP variant switch (csrc/fjsp_kernels.hip);
an order arrival inside a step re-solves the fluid LP on the host, which makes
step() blocking for this environment.  Nothing is computed in Python.
"""
import torch

from ..batch import VARIANT_MO_DFJSP
from ..utilities.Utility_Class import MyError
from ._common import BatchedEnv, DropInEnv


class BatchedMODFJSP(BatchedEnv):
    """Vectorised MO_DFJSP_breakdown.  step(actions u8[N,2]) -> (state[N,30], reward[N], done[N])."""

    actions_size = [12, 10]
    action_types = "DISCRETE"
    state_size = 30
    variant = VARIANT_MO_DFJSP

    def _staging(self):
        self.mo = torch.zeros(self.N, 4, dtype=torch.float64, device=self.device)
        self.mo[:, 0] = 1.0

    def set_objective(self, reward_policy, completion=None, tardiness=None, energy_consumption=None):
        """reward_policy 0 makespan / 1 tardiness / 2 energy / 3 normalised sum; the normalisers
        (scalars or per-env tensors) are only read by policy 3 (MO_DFJSP_breakdown.py:430-447)."""
        self.mo[:, 0] = float(reward_policy)
        self.mo[:, 1] = 0.0 if completion is None else completion
        self.mo[:, 2] = 0.0 if tardiness is None else tardiness
        self.mo[:, 3] = 0.0 if energy_consumption is None else energy_consumption

    def step(self, actions, autoreset=False):
        return self.batch.step(actions, autoreset=autoreset, mo=self.mo)


class MO_DFJSP_Environment(DropInEnv):
    """Drop-in for environments/MO_DFJSP_breakdown.py:12 (N = 1 view of the batched kernels); reset() is
    MO_DFJSP_breakdown.py:58-90.

    ``use_instance=False, path=..., file_name=...`` reads a CSV folder with a machine_data.csv
    (MO_DFJSP_instance_read.py); ``use_instance=True, DDT=..., M=..., S=...`` draws a random instance
    with the generator's power ranges (Instance_generate.py:61-66) and no breakdown windows, i.e. what
    environments/MO_DFJSP.py plays.
    """
    variant = VARIANT_MO_DFJSP
    counters = DropInEnv.counters + ("energy_consumption",)

    def _generated(self, seed):
        self._set.generate_machine_data(0, seed)                          # p_rjm / p_m_idle, Instance_generate.py:61-66

    def _start(self, rng_seed, device):
        super()._start(rng_seed, device)
        self.DDT = self._arrays.ddt
        self.actions_size = [12, 10]                                                 # :32
        self.action_tuple = tuple((a1, a2) for a1 in range(12) for a2 in range(10))  # :33
        self.action_space = list(range(12))
        self.state_size = 30
        self.action_types = "DISCRETE"
        self.observation_space = 15
        self.energy_consumption = 0
        self.reward = None
        self._mo = torch.zeros(1, 4, dtype=torch.float64, device=self._batch.device)

    def step(self, action, reward_policy=None, completion=None, tardiness=None, energy_consumption=None):
        """MO_DFJSP_breakdown.py:189-328"""
        if len(action) == 1:
            action = self.action_tuple[action[0]]                                    # :191-192
        if reward_policy not in (0, 1, 2, 3):
            raise MyError("未定义该回报函数")                                         # :447
        if reward_policy == 3 and (completion is None or tardiness is None or energy_consumption is None):
            raise TypeError("unsupported operand type(s) for /: 'int' and 'NoneType'")
        self._act[0, 0], self._act[0, 1] = int(action[0]), int(action[1])
        self._mo[0, 0] = float(reward_policy)
        for i, v in enumerate((completion, tardiness, energy_consumption)):
            self._mo[0, 1 + i] = 0.0 if v is None else float(v)
        return self._step(float if reward_policy == 3 else int, self._mo)           # integer differences :433-437
