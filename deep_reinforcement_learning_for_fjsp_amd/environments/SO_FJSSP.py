"""Host-side mirror of the reference's environments/SO_FJSSP.py: ``BatchedSOFJSSP`` (N environments stepped by one
launch) and ``SO_FJSSP_Environment`` (the reference's single-environment class as an N = 1 view of a batch).  The
parts every variant shares are in _common.py.
"""
from ..batch import VARIANT_SO_FJSSP
from ..utilities.Utility_Class import MyError
from ._common import BatchedEnv, DropInEnv, _instance_set


class BatchedSOFJSSP(BatchedEnv):
    """Vectorised SO_FJSSP: reset() -> f64[N,20]; step(actions u8[N,2]) -> (state, reward, done) device tensors."""

    actions_size = [6, 5]
    action_types = "DISCRETE"
    state_size = 20
    variant = VARIANT_SO_FJSSP          # (environments/SO_DFJSP.py subclasses with its own variant)

    def step(self, actions, autoreset=False):
        return self.batch.step(actions, autoreset=autoreset)

    def rollout(self, actions):
        return self.batch.rollout(actions)


def _reference_reward(r):
    return int(r) if r == int(r) else r      # the reference's reward is a Python int (:328)


class SO_FJSSP_Environment(DropInEnv):
    """Drop-in for environments/SO_FJSSP.py:12 (same names, argument meaning and error behaviour)."""
    variant = VARIANT_SO_FJSSP
    keeps_ddt = True

    def _start(self, rng_seed, device):
        super()._start(rng_seed, device)
        a = self._arrays
        self.DDT = a.ddt if not hasattr(self, "DDT") else self.DDT
        self.kind_tuple, self.order_tuple = tuple(range(a.R)), tuple(range(a.S))
        self.kind_task_tuple = a.kind_task_tuple
        # SO_FJSSP.py:17-33
        self.next_state = None
        self.reward = None
        self.actions_size = [6, 5]
        self.action_tuple = tuple((a1, a2) for a1 in range(6) for a2 in range(5))
        self.state_size = 20
        self.action_types = "DISCRETE"
        self.observation_space = 10
        self.delay_time_sum_last = 0

    def __getstate__(self):
        st = super().__getstate__()
        st.update(file_name=self.file_name)
        return st

    def __setstate__(self, st):
        if "episode" in st:
            super().__setstate__(st)
            return
        # a state dict without an episode (instance arrays, file name, device, seed): a fresh env, as before
        self.file_name = st["file_name"]
        self._set = _instance_set(st["arrays"])
        self._start(st["rng_seed"], st["device"])

    def reset(self):
        """SO_FJSSP.py:51-76: returns a fresh float64 array of 20."""
        super().reset()
        self.next_state, self.reward, self.delay_time_sum_last = None, None, 0
        return self.state

    def step(self, action):
        """SO_FJSSP.py:168-265: action = indexable pair (task rule index, machine rule index)."""
        a0, a1 = int(action[0]), int(action[1])
        if not 0 <= a0 < 6:
            raise MyError("报错：未定义该工序动作规则")
        if not 0 <= a1 < 5:
            raise MyError("报错：未定义该机器分配规则。")
        self._act[0, 0], self._act[0, 1] = a0, a1
        self._step(_reference_reward)
        self.delay_time_sum_last = self.delay_time_sum
        self.next_state = self.state
        return self.state, self.reward, self.done
