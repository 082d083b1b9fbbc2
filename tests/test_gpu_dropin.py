"""GPU: the surface the environment classes show their users -- the drop-in classes' attribute names, the order in
which they draw omitted seeds, state dicts pickled under older staging names -- and the batched classes' methods."""
import csv
import random

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

_STEP = {
    "SO_FJSSP_Environment": lambda e, t: e.step([t % 6, (t * 7) % 5]),
    "SO_DFJSP_Environment": lambda e, t: e.step([t % 6, (t * 7) % 5]),
    "SO_SFJSP_Environment": lambda e, t: e.step((t * 3) % 20),
    "MO_FJSSP_Environment": lambda e, t: e.step((t * 5) % 18, weight_vector=(0.5, 0.5), completion=900.0,
                                                tardiness=400.0),
    "MO_DFJSP_Environment": lambda e, t: e.step([t % 12, (t * 3) % 10], reward_policy=1),
}

# The public attributes of a generated instance's env (what the reference's users read), after construction, reset()
# and step() alike, except where _AFTER_STEP adds one.  Names with a leading underscore are this port's own.
_SO_FJSSP_ATTRS = {"DDT", "action_tuple", "action_types", "actions_size", "completion_time", "delay_time_sum",
                   "delay_time_sum_last", "done", "file_name", "kind_count", "kind_task_tuple", "kind_tuple",
                   "machine_count", "machine_tuple", "next_state", "observation_space", "order_count", "order_tuple",
                   "reward", "reward_sum", "state", "state_size", "step_count", "step_time"}
_ATTRS = {
    "SO_FJSSP_Environment": _SO_FJSSP_ATTRS,
    "SO_DFJSP_Environment": _SO_FJSSP_ATTRS,
    "SO_SFJSP_Environment": {"action_space", "action_types", "actions", "completion_time", "delay_time_sum", "done",
                             "file_name", "kind_count", "machine_count", "machine_tuple", "observation_space",
                             "order_count", "reward_sum", "state", "state_size", "static_state_space", "step_count",
                             "step_time"},
    "MO_FJSSP_Environment": {"DDT", "action_space", "action_types", "actions", "completion_time", "delay_time_sum",
                             "done", "file_name", "kind_count", "machine_count", "machine_tuple", "observation_space",
                             "order_count", "reward_sum", "state", "state_size", "static_state_space", "step_count",
                             "step_time"},
    "MO_DFJSP_Environment": {"DDT", "action_space", "action_tuple", "action_types", "actions_size", "completion_time",
                             "delay_time_sum", "done", "energy_consumption", "file_name", "kind_count",
                             "machine_count", "machine_tuple", "observation_space", "order_count", "reward",
                             "reward_sum", "state", "state_size", "step_count", "step_time"},
}
_AFTER_STEP = {"SO_SFJSP_Environment": {"reward"}, "MO_FJSSP_Environment": {"reward"}}
_CSV_ADDS, _CSV_DROPS = {"path"}, {"MO_FJSSP_Environment": {"DDT"}}     # a CSV folder instead of the generator

# the public methods of each batched class before they shared a base (check_status was BatchedSOFJSSP's alone)
_BATCHED = {
    "BatchedSOFJSSP": {"check_status", "read", "record_schedule", "reset", "restore", "rollout", "schedule", "snapshot",
                       "step"},
    "BatchedSODFJSP": {"check_status", "read", "record_schedule", "reset", "restore", "rollout", "schedule", "snapshot",
                       "step"},
    "BatchedSOSFJSP": {"read", "record_schedule", "reset", "restore", "schedule", "snapshot", "step"},
    "BatchedMOFJSSP": {"read", "record_schedule", "reset", "restore", "schedule", "set_objective", "snapshot", "step"},
    "BatchedMODFJSP": {"read", "record_schedule", "reset", "restore", "schedule", "set_objective", "snapshot", "step"},
}


@pytest.fixture(scope="module")
def envs(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from deep_reinforcement_learning_for_fjsp_amd import environments
    return environments


def _write_csv(a, folder):
    """A reference CSV folder of instance arrays a, machine data included (what MO_DFJSP_instance_read.py reads)."""
    folder.mkdir()
    koff = np.concatenate(([0], np.cumsum(a.Jr)))
    with open(folder / "based_data.csv", "w", newline="") as f:
        csv.writer(f).writerows([["kind_count", "machine_count", "order_count", "DDT"], [a.R, a.M, a.S, a.ddt]])
    with open(folder / "process_data.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["kind", "task", "machine_selectable", "process_time", "power"])
        for r in range(a.R):
            for j in range(int(a.Jr[r])):
                k = int(koff[r]) + j
                ms = tuple(int(m) for m in a.elig_list[k, :a.elig_n[k]])
                w.writerow([r, j, ms, tuple(int(a.p[k, m]) for m in ms), tuple(int(a.power[k, m]) for m in ms)])
    with open(folder / "order_data.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["order", "time_arrive", "time_delivery", "kind_number"])
        for so in range(a.S):
            w.writerow([so, int(a.arrive[so]), int(a.delivery[so]), tuple(int(c) for c in a.count[so])])
    with open(folder / "machine_data.csv", "w", newline="") as f:
        csv.writer(f).writerows([["machine", "idle_power"]] + [[m, int(a.idle_power[m])] for m in range(a.M)])


def _public(env):
    return {k for k in vars(env) if not k.startswith("_")}


@pytest.mark.parametrize("name", sorted(_ATTRS))
@pytest.mark.parametrize("source", ["generate", "csv"])
def test_dropin_attribute_names(envs, tmp_path, name, source):
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    if source == "generate":
        env = getattr(envs, name)(use_instance=True, DDT=1.0, M=6, S=1, seed=3, rng_seed=4)
        want = _ATTRS[name]
    else:
        s = fi.InstanceSet(1).generate(0, 77, fi.reference_generator_params(1.0, 6, 1))
        s.generate_machine_data(0, 77)
        _write_csv(s.arrays(0), tmp_path / "D0")
        env = getattr(envs, name)(use_instance=False, path=str(tmp_path), file_name="D0", rng_seed=4)
        want = (_ATTRS[name] | _CSV_ADDS) - _CSV_DROPS.get(name, set())
    assert _public(env) == want, "construction"
    env.reset()
    assert _public(env) == want, "reset"
    _STEP[name](env, 1)
    assert _public(env) == want | _AFTER_STEP.get(name, set()), "step"


@pytest.mark.parametrize("name", sorted(_ATTRS))
def test_omitted_seeds_are_drawn_seed_then_rng_seed(envs, name):
    cls, step = getattr(envs, name), _STEP[name]
    random.seed(123)
    implicit = cls(use_instance=True, DDT=1.0, M=6, S=1)
    random.seed(123)
    seed = random.getrandbits(63)
    explicit = cls(use_instance=True, DDT=1.0, M=6, S=1, seed=seed, rng_seed=random.getrandbits(63))
    assert np.array_equal(H.bits(implicit.reset()), H.bits(explicit.reset()))
    t = 0
    while not explicit.done:
        got, want = step(implicit, t), step(explicit, t)
        assert np.array_equal(H.bits(got[0]), H.bits(want[0])) and got[1:] == want[1:], t
        t += 1
    assert implicit.done and implicit.reward_sum == explicit.reward_sum


def test_state_dict_with_the_old_staging_name_loads(envs):
    """SO_FJSSP_Environment pickles used to carry its staging tensor as "_actions" (and its device and rng_seed as
    attributes of its own): such a state dict still loads and continues the episode."""
    cls, step = envs.SO_FJSSP_Environment, _STEP["SO_FJSSP_Environment"]
    orig = cls(use_instance=True, DDT=1.0, M=6, S=1, seed=8, rng_seed=9)
    orig.reset()
    for t in range(5):
        step(orig, t)
    st = orig.__getstate__()
    st["tensors"] = {"_actions": st["tensors"].pop("_act")}
    st["attrs"].update(_device=0, _rng_seed=9)
    env = cls.__new__(cls)
    env.__setstate__(st)
    assert env.step_count == 5 and np.array_equal(H.bits(env.state), H.bits(orig.state))
    t = 5
    while not orig.done:
        got, want = step(env, t), step(orig, t)
        assert np.array_equal(H.bits(got[0]), H.bits(want[0])) and got[1:] == want[1:], t
        t += 1
    assert env.done and env.reward_sum == orig.reward_sum and env.delay_time_sum == orig.delay_time_sum


@pytest.mark.parametrize("name", sorted(_BATCHED))
def test_batched_methods(envs, name):
    cls = getattr(envs, name)
    have = {n for n in dir(cls) if not n.startswith("_") and callable(getattr(cls, n))}
    assert have == _BATCHED[name] | {"check_status"}


def test_check_status_on_a_flat_action_variant(envs):
    import torch
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    env = envs.BatchedMOFJSSP(fi.InstanceSet(1).generate(0, 5, fi.bench_10x5_params()).solve_fluid(), rng_seed=1)
    env.set_objective((0.5, 0.5), 900.0, 400.0)
    env.reset()
    acts = torch.zeros(1, dtype=torch.int64, device=env.device)
    while not bool(env.batch.done[0]):
        env.step(acts)
        env.check_status()                      # no error bit while the episodes run
    env.step(acts)
    with pytest.raises(ValueError):
        env.check_status()
