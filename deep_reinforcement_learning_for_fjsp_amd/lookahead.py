"""Rollout lookahead over fixed dispatching rules (the rollout algorithm with fixed actions as base heuristics).

At every decision each environment of the source batch is branched once per candidate action: the episode state is
saved (EnvBatch.snapshot) and loaded into a branch batch of P x N envs on the same instances (EnvBatch.restore, branch
env p * N + i <- source env i), branch block p plays candidate p to the end of the episode in one fused launch, and the
source env takes the candidate whose branch ended with the lowest objective (the first one on ties).

That decision loop (decide_by_rollouts) is written once, with two ways of playing a branch to the end: rollout_dispatch
keeps every block on its candidate (the fused rule rollout), policy_search.policy_lookahead applies the candidate once
and goes on with a greedy actor.  What they and policy_search.best_of share around it is here too.

With deterministic candidates the dynamics and the objective are functions of the action sequence, so following the
chosen candidate from the next state reproduces its branch's objective: the objective the lookahead reaches is never
above the best fixed candidate's.  Random-rule candidates (SO_FJSSP task rule 6 / machine rule 5 style
random.choice rules) are allowed, but a branch continues on its own slot's random stream, so the bound does not hold
for them.  Out of scope: truncated horizons.

rule_front does not decide step by step: it plays every candidate from the current state to the end once and returns,
per env, the Pareto front of the finished episodes over several objectives (pareto.select).
"""
import time

import numpy as np
import torch

from . import pareto
from .batch import (EnvBatch, ST_BAD_MACHINE_RULE, ST_BAD_TASK_RULE, ST_NO_EVENT, ST_SCHEDULE_OVERFLOW, VARIANT_MO_DFJSP,
                    VARIANT_MO_FJSSP_DISCRETES, VARIANT_SO_DFJSP, VARIANT_SO_FJSSP, VARIANT_SO_SFJSP)

OBJECTIVES = ("makespan", "tardiness", "energy")
_FLAT = (VARIANT_SO_SFJSP, VARIANT_MO_FJSSP_DISCRETES)
# valid actions per variant: (task rules, machine rules) of the pair variants, flat action count of the flat ones
ACTION_RANGES = {VARIANT_SO_FJSSP: (6, 5), VARIANT_SO_DFJSP: (6, 5), VARIANT_MO_DFJSP: (12, 10),     # SO_FJSSP.py:30, MO_DFJSP_breakdown.py:32
                 VARIANT_SO_SFJSP: (20,), VARIANT_MO_FJSSP_DISCRETES: (18,)}                       # SO_SFJSP.py:25, MO_FJSSP_discretes.py:26
# status bits that stop an env for good (it will never be done): a rule index the env does not have, no next event,
# a dispatch record with no slot
_ERR_BITS = ST_BAD_TASK_RULE | ST_BAD_MACHINE_RULE | ST_NO_EVENT | ST_SCHEDULE_OVERFLOW


def objective_values(batch, objective, r=None):
    r = batch.read() if r is None else r
    if callable(objective):
        v = objective(r)
        if not torch.is_tensor(v) or v.shape != (batch.N,):
            raise ValueError("objective(read()) must return a tensor of shape (%d,)" % batch.N)
        return v.to(torch.float64)
    if objective == "makespan":
        return r["makespan"].to(torch.float64)
    if objective == "tardiness":
        return r["delay_time_sum"].to(torch.float64)
    if objective == "energy":
        if "energy_consumption" not in r:
            raise ValueError("objective 'energy' needs a MO_DFJSP batch")
        return r["energy_consumption"].to(torch.float64)
    raise ValueError("objective must be one of %s or a callable on read()" % (OBJECTIVES,))


def candidate_pairs(candidates, variant):
    """uint8[P, 2] action pairs of the candidates: (task rule, machine rule) pairs, or flat action indices for the
    flat-action variants (SO_SFJSP, MO_FJSSP_discretes).  Every candidate must be an action of the variant (ValueError
    otherwise): an env given an undefined rule stops with an error bit and would never finish its rollout."""
    if variant not in ACTION_RANGES:
        raise ValueError("unknown variant %r" % (variant,))
    rng = ACTION_RANGES[variant]
    if len(candidates) == 0:
        raise ValueError("rollout_dispatch: at least one candidate is needed")
    out = np.zeros((len(candidates), 2), np.int64)
    for p, c in enumerate(candidates):
        if variant in _FLAT:
            if np.ndim(c) != 0:
                raise ValueError("this variant takes flat actions (ints), got %r" % (c,))
            out[p, 0] = int(c)
        else:
            if np.ndim(c) != 1 or len(c) != 2:
                raise ValueError("this variant takes (task rule, machine rule) pairs, got %r" % (c,))
            out[p] = [int(c[0]), int(c[1])]
        if not all(0 <= out[p, q] < rng[q] for q in range(len(rng))):
            raise ValueError("candidate %r is not an action of this variant (%s)"
                             % (c, "flat actions 0..%d" % (rng[0] - 1) if len(rng) == 1 else
                                "task rules 0..%d, machine rules 0..%d" % (rng[0] - 1, rng[1] - 1)))
    return out.astype(np.uint8)


def check_branch_shape(n_envs, n_inst, n_candidates, who="rollout_dispatch"):
    """The branch batch holds n_candidates x n_envs envs; branch env p * N + i plays instance (p * N + i) % n_inst,
    which is source env i's instance only when N is a multiple of n_inst."""
    if n_candidates <= 0:
        raise ValueError("%s: at least one candidate is needed" % who)
    if n_envs % n_inst != 0:
        raise ValueError("%s: the source batch's N (%d) must be a multiple of its instance count (%d)" % (who, n_envs, n_inst))
    return n_candidates * n_envs


def make_branch(batch, n_candidates):
    """An EnvBatch of n_candidates x N envs on the source batch's instances, variant and kernel family (asked for
    explicitly: the record layouts of the two families differ, and the snapshot fingerprint includes the family)."""
    n = check_branch_shape(batch.N, batch.n_inst, n_candidates)
    if batch.instances is None:         # a generated source (EnvBatch.generated): the same parameters and seeds once more
        return EnvBatch.generated(batch.gen_params, n, batch.seed_base, n_inst=batch.n_inst, variant=batch.variant,
                                  device=batch.device_index, rng_seed=batch.rng_seed, first_env=batch.first_env,
                                  family=batch.kernel_family)
    return EnvBatch(batch.instances, n, first=batch.first, n_inst=batch.n_inst, variant=batch.variant,
                    device=batch.device_index, rng_seed=batch.rng_seed, first_env=batch.first_env,
                    kernel_family=batch.kernel_family)


def branch_for(batch, n_blocks, branch, who):
    """`branch` if it is a batch of n_blocks x N envs on the source's instances and family, a new one for None."""
    if branch is None:
        return make_branch(batch, n_blocks)
    if (not isinstance(branch, EnvBatch) or branch.N != n_blocks * batch.N or branch.n_inst != batch.n_inst
            or branch.kernel_family != batch.kernel_family):
        raise ValueError("%s: branch must be an EnvBatch of %d envs on the source's instances and kernel family" % (who, n_blocks * batch.N))
    return branch


def mo_rows(mo, N, dev, blocks=1):
    """The step arguments `mo` as f64[N, 4] on the device; for a branch batch, f64[blocks x N, 4] with row p * N + i =
    mo[i].  None stays None."""
    if mo is None:
        return None
    mo = torch.as_tensor(mo, dtype=torch.float64, device=dev).reshape(N, 4).contiguous()
    return mo if blocks == 1 else mo.repeat(blocks, 1)


def check_status(r, who, caller):
    """RuntimeError if an env of read()'s `r` cannot finish.  who: "source" / "branch"; caller: the user's call."""
    bad = (r["status"].long() & _ERR_BITS) != 0
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0, 0].item())
        raise RuntimeError("%s: %s env %d carries error status %d (FJSP_ST_* bits): it cannot finish its episode"
                           % (caller, who, i, int(r["status"][i].item())))


def ops_per_env(batch):
    """i64[N] device tensor: the operations of every env's instance = the steps of its episode."""
    ops = []
    for i in range(batch.n_inst):
        a = batch.instance_arrays(i)
        ops.append(int((np.asarray(a.count).reshape(a.S, a.R) * np.asarray(a.Jr)[None, :]).sum()))
    ops = np.asarray(ops, np.int64)
    return torch.as_tensor(ops[np.arange(batch.N) % batch.n_inst], device=batch.device)


class Clock(object):
    """Seconds per named part into the dict `timings`, synchronised at every lap; nothing for timings=None."""

    def __init__(self, timings, dev):
        self.t, self.dev, self.t0 = timings, dev, None

    def start(self):
        if self.t is not None:
            torch.cuda.synchronize(self.dev)
            self.t0 = time.perf_counter()

    def lap(self, what):
        if self.t is not None:
            torch.cuda.synchronize(self.dev)
            now = time.perf_counter()
            self.t[what] = self.t.get(what, 0.0) + now - self.t0
            self.t0 = now


def decide_by_rollouts(batch, pairs, objective, mo, branch, timings, who, state, play_branch):
    """Play the source EnvBatch `batch` to the end by rollout decisions (the module docstring's loop); returns
    rollout_dispatch's dict.  pairs: candidate_pairs' uint8[P, 2]; objective, mo, branch, timings: as rollout_dispatch
    takes them; who: the function the user called, for error messages; state: whether the source step returns a state
    (the next decision's actor input).  play_branch(branch, T, mo_branch, src_dev, clock) plays the restored branch
    batch to the end and returns its read(): T bounds the steps any env has left, mo_branch is mo per branch env,
    src_dev the device map branch env -> source env; it calls clock.lap("rollout") between its launch and its read."""
    P, N, dev = len(pairs), batch.N, batch.device
    check_branch_shape(N, batch.n_inst, P, who)
    branch = branch_for(batch, P, branch, who)
    mo = mo_rows(mo, N, dev)
    mo_branch = mo_rows(mo, N, dev, P)
    pairs_dev = torch.as_tensor(pairs, device=dev)                                  # [P, 2]
    src = np.tile(np.arange(N, dtype=np.int64), P)
    src_dev = torch.as_tensor(src.astype(np.int32), device=dev)
    ops = ops_per_env(batch)
    snap, restored = None, False
    chosen_all, steps = [], torch.zeros(N, dtype=torch.int64, device=dev)
    last = torch.zeros(N, 2, dtype=torch.uint8, device=dev)
    clock = Clock(timings, dev)
    prev_live, prev_count = None, None
    while True:
        r = batch.read()
        check_status(r, "source", who)
        live = r["done"] == 0
        count = r["step_count"].long()
        if prev_live is not None and bool((prev_live & live & (count <= prev_count)).any()):
            raise RuntimeError("%s: a source env did not advance in its step" % who)
        if not bool(live.any()):
            break
        prev_live, prev_count = live, count
        T = int(torch.where(live, ops - count, torch.zeros_like(ops)).max().item())
        clock.start()
        snap = batch.snapshot(out=snap)
        clock.lap("snapshot")
        branch.restore(snap, src_dev if restored else src, rows=False)      # (the host map is validated once)
        restored = True
        clock.lap("restore")
        rb = play_branch(branch, T, mo_branch, src_dev, clock)
        cost = objective_values(branch, objective, rb).reshape(P, N)
        best = torch.argmin(cost, dim=0)                                             # first minimum over candidates
        clock.lap("read")
        act = torch.where(live[:, None], pairs_dev[best], last)
        batch.rollout(act[None].contiguous(), trace=False, rewards=False, mo=mo, state=state)
        clock.lap("step")
        steps += live.long()
        last = act
        chosen_all.append(act)
    actions = torch.stack(chosen_all).cpu().numpy() if chosen_all else np.zeros((0, N, 2), np.uint8)
    return dict(actions=actions, steps=steps.cpu().numpy(), objective=objective_values(batch, objective), branch=branch)


def play_rules(branch, acts, mo_branch, who, lap=None):
    """Play the restored branch batch to the end with the given actions, acts u8[T, P x N, 2] (the fused rule rollout; T
    bounds the steps any env has left), and return its read().  lap() is called between the launch and the read."""
    branch.rollout(acts, trace=False, rewards=False, mo=mo_branch, state=False)
    if lap is not None:
        lap()
    rb = branch.read()
    check_status(rb, "branch", who)
    while not bool((rb["done"] != 0).all()):       # (a step dispatches one operation: not expected to run; T still bounds it)
        before = rb["step_count"].long()
        branch.rollout(acts, trace=False, rewards=False, mo=mo_branch, state=False)
        rb = branch.read()
        check_status(rb, "branch", who)
        if not bool(((rb["done"] != 0) | (rb["step_count"].long() > before)).all()):
            raise RuntimeError("%s: a branch env neither finished nor advanced" % who)
    return rb


def rollout_dispatch(batch, candidates, objective, mo=None, branch=None, timings=None):
    """Play every env of `batch` (an EnvBatch or a Batched* wrapper, reset and not yet stepped, or mid-episode) to the end,
    choosing at every decision the candidate whose rollout to the end gives the lowest objective.

    candidates: P action pairs (task rule, machine rule), or flat actions for SO_SFJSP / MO_FJSSP_discretes.
    objective: "makespan", "tardiness" (delay_time_sum), "energy" (MO_DFJSP) or a callable taking read()'s dict and
    returning a tensor[N] to minimise.  mo: f64[N, 4] step arguments of the MO variants (as EnvBatch.step takes them);
    a wrapper's own `mo` is NOT picked up when none is given (policy_search's functions do pick it up): pass it.
    branch: an EnvBatch of P x N envs made by make_branch (reused across calls), or None to build one.
    timings: a dict that receives the seconds spent per part (snapshot, restore, rollout, read, step), synchronised.

    Returns dict(actions=uint8[D, N, 2] numpy, the action applied at decision d (env i's d-th step from here; rows past
    an env's end repeat its last choice and are not applied), steps=int[N] decisions each env took, objective=tensor[N]
    of the finished episodes, branch=the branch batch)."""
    batch = getattr(batch, "batch", batch)
    pairs = candidate_pairs(candidates, batch.variant)
    P, N = len(pairs), batch.N
    branch_act = torch.as_tensor(pairs, device=batch.device)[:, None, :].expand(P, N, 2).reshape(P * N, 2)   # candidate p in block p
    act_buf = []                  # [branch_act repeated over the steps]: built at the first decision, T only shrinks

    def play_branch(branch, T, mo_branch, src_dev, clock):
        if not act_buf or act_buf[0].shape[0] < T:
            act_buf[:] = [branch_act[None].expand(T, P * N, 2).contiguous()]
        return play_rules(branch, act_buf[0][:T], mo_branch, "rollout_dispatch", lambda: clock.lap("rollout"))

    return decide_by_rollouts(batch, pairs, objective, mo, branch, timings, "rollout_dispatch", False, play_branch)


def objective_vectors(branch, objectives, r, blocks):
    """f64[blocks, N, D]: the `objectives` (each as objective_values takes it) of a finished blocks x N branch batch."""
    if len(objectives) < 1:
        raise ValueError("at least one objective is needed")
    return torch.stack([objective_values(branch, o, r) for o in objectives], dim=1).reshape(blocks, branch.N // blocks, len(objectives))


def rule_front(batch, candidates, objectives=("makespan", "tardiness"), mo=None, branch=None, cap=None):
    """The Pareto front, per env, of P fixed candidates each played from the env's current state to the end of its
    episode: branch block p plays candidate p (one fused rule rollout of the P x N branch batch), the finished
    episodes' objective vectors go through one pareto.select.

    candidates, mo, branch: as rollout_dispatch (P at most 1024).  objectives: 1..4 of "makespan", "tardiness", "energy"
    (MO_DFJSP) or callables on read(), lower is better.  cap: the front members kept per env (default P).
    The source batch is only read: its state rows, read() and schedule stay as they were.

    Returns dict(objectives=f64[P, N, D], index=i32[N, cap] the front's candidates in ascending lexicographic order of
    their vectors (-1 past the front), count=i32[N], mask=u8[P, N], front=f64[N, cap, D] (NaN past the front),
    branch=the branch batch, holding the finished episodes)."""
    who = "rule_front"
    batch = getattr(batch, "batch", batch)
    pairs = candidate_pairs(candidates, batch.variant)
    P, N, dev = len(pairs), batch.N, batch.device
    if P > pareto.MAX_CANDIDATES:
        raise ValueError("%s: at most %d candidates, got %d" % (who, pareto.MAX_CANDIDATES, P))
    check_branch_shape(N, batch.n_inst, P, who)
    branch = branch_for(batch, P, branch, who)
    r = batch.read()
    check_status(r, "source", who)
    left = torch.where(r["done"] == 0, ops_per_env(batch) - r["step_count"].long(), torch.zeros(N, dtype=torch.int64, device=dev))
    T = max(int(left.max().item()), 1)
    branch.restore(batch.snapshot(), np.tile(np.arange(N, dtype=np.int64), P), rows=False)
    acts = torch.as_tensor(pairs, device=dev)[None, :, None, :].expand(T, P, N, 2).reshape(T, P * N, 2).contiguous()   # candidate p in block p
    rb = play_rules(branch, acts, mo_rows(mo, N, dev, P), who)
    obj = objective_vectors(branch, objectives, rb, P)
    index, count, mask = pareto.select(obj, cap=cap)
    return dict(objectives=obj, index=index, count=count, mask=mask, front=pareto.front_points(obj, index), branch=branch)
