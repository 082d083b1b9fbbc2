"""Decoding a trained dispatching policy on the device: greedy play, best-of-K sampling, a policy rollout lookahead,
beam search, and the Pareto front of several policies' sampled episodes.

The first three share one launch, fjsp_env_play_policy (play_policy_kernel, csrc/fjsp_kernels_policy.inc): every env plays to
the end of its episode with the actor evaluated inside the environment kernel and no rollout-buffer traffic.  The actor is
an agents.MPPPO ActorNet; the kernel takes those of the in-kernel shape (state_size <= 32 -> 128 -> 128 -> n_actions
<= 32) on every single-order batch, whatever its operation types and jobs (EnvBatch.policy_build reports the workgroup it
runs).  A batch with order arrivals (SO_FJSSP / SO_DFJSP instances of several orders) takes fjsp_env_play_policy_orders: the
same kernel once per segment of the episode, the arrival service (fluid LPs, arrival_kernel) between the launches -- at most
as many launches as the batch's largest order count (EnvBatch.policy_orders_build).  Other actors (MPPPO's 200 x 5 nets) and
MO_DFJSP batches run the same decoding as a per-step loop (actor, argmax or fjsp_policy_sample, one env step), only more
slowly.

- play: every env to the end, greedy (argmax of the actor's probabilities) or sampled (epsilon 0).
- best_of: k episodes per env in a k x N branch batch, block 0 greedy and the others sampled; each source env ends its
  episode with the best one.
- policy_lookahead: the rollout algorithm of lookahead.rollout_dispatch with the greedy actor as base policy: the same
  decision loop (lookahead.decide_by_rollouts), in which branch block p applies candidate p and plays greedily to the
  end, all in one launch.
- beam_search: `width` partial schedules per env in a width x N beam batch.  At every decision each beam is scored under
  every action (score="logp": the cumulative -log probability of the actor, one forward pass; score="rollout": the
  objective of the episode that applies the action and follows the greedy actor to the end, policy_lookahead's
  evaluation in a width x P x N expansion batch), fjsp_beam_select (csrc/fjsp_beam.hip) keeps the `width` best of an
  env's width x A candidates under a stated total order (cost, then parent beam, then action), the beam batch is
  gathered through a snapshot pair and takes one step.  The search is reproducible bit for bit; width 1 is greedy play
  (logp) or policy_lookahead (rollout).
- pareto_front: P actors x k episodes per env, played as best_of plays them, and the non-dominated set of their
  objective vectors per env (pareto.select, fjsp_pareto_select, csrc/fjsp_pareto.hip) instead of one minimum.
- improve: no policy at all -- hill climbing on explicit schedules (an operation sequence and a machine per operation, for
  instance a recorded table's): every round decodes `neighbours` random moves of each env's plan in one launch
  (schedule.decode, fjsp_schedule_decode, csrc/fjsp_decode.hip) and keeps the best if it is no worse; the moves are uniform
  reassignments and adjacent swaps, or drawn from the neighbourhood of the plan's critical path (schedule.critical,
  fjsp_schedule_critical).  A MO_DFJSP batch is decoded with its breakdown windows and energy (schedule.decode_dyn,
  fjsp_schedule_decode_dyn): "energy" is an objective there, and the moves are the uniform ones.
- left_shift: the active schedule of a plan -- every operation in the earliest idle interval of its machine that is long
  enough (schedule.decode_active, fjsp_schedule_decode_active) -- handed back as a begin-ordered plan that every search here
  takes; for one plan per env or a whole population.
- local_search: improve's search, descent or tabu, as one launch for all its rounds (schedule.search, fjsp_schedule_search;
  on a MO_DFJSP batch schedule.search_dyn, fjsp_schedule_search_dyn: uniform neighbourhood, "energy" an objective):
  a wavefront per env, a lane per neighbour, the plan in LDS, on a counter-based draw stream that shards reproduce.
- front_search: local_search steered by a weighted sum of the objectives, one weight vector per env, that keeps the Pareto
  archive of every schedule it decodes in the same launch (schedule.search_front, fjsp_schedule_search_front), and with
  merge=True the front per instance over its envs' archives (pareto.select).
- seed_population, genetic_search: a population search on the same plans -- the GA baseline of the FJSP literature -- with all
  its generations in one launch (schedule.evolve, fjsp_schedule_evolve): a lane per individual, which decodes its child
  while it merges it from two parents; seeded from recorded or sampled schedules.  decoder="active" scores every
  individual with left_shift's decoder inside the same launch (schedule.evolve_active, fjsp_schedule_evolve_active).

Every function takes an EnvBatch or a Batched* wrapper (whose `mo` is used when none is given).  The source's state rows
must hold its envs' current states, as reset() and step() / rollout() with a state leave them: the actor reads them.
"""
import ctypes as C

import numpy as np
import torch

from . import _capi, pareto
from ._capi import ptr as _ptr
from .agents.native_actor import native_actor_forward, native_actor_params
from .batch import ST_BAD_MACHINE_RULE, ST_BAD_TASK_RULE, ST_NO_EVENT
from .lookahead import (ACTION_RANGES, OBJECTIVES, Clock, branch_for, candidate_pairs, check_branch_shape, check_status,
                        decide_by_rollouts, mo_rows, objective_values, objective_vectors, ops_per_env)

# the status bits at which an env stops playing (the kernel's and fjsp_env_rollout's `live` test)
_STOP_BITS = ST_BAD_TASK_RULE | ST_BAD_MACHINE_RULE | ST_NO_EVENT


def _unwrap(batch, mo):
    return getattr(batch, "batch", batch), (getattr(batch, "mo", None) if mo is None else mo)


def action_encoding(actor, batch):
    """(n_actions, pair_div) of the batch's variant for `actor`: pair_div = the machine-rule count of the pair variants,
    0 for the flat ones (lookahead.ACTION_RANGES).  ValueError unless the actor maps state_size inputs to n_actions."""
    if batch.variant not in ACTION_RANGES:
        raise ValueError("unknown variant %r" % (batch.variant,))
    rng = ACTION_RANGES[batch.variant]
    n_actions, pair_div = int(np.prod(rng)), (rng[1] if len(rng) == 2 else 0)
    lin = [m for m in actor.modules() if isinstance(m, torch.nn.Linear)]
    if not lin:
        raise ValueError("the actor has no nn.Linear layers")
    if lin[0].in_features != batch.state_size or lin[-1].out_features != n_actions:
        raise ValueError("the actor maps %d inputs to %d actions; this batch has states of %d and %d actions"
                         % (lin[0].in_features, lin[-1].out_features, batch.state_size, n_actions))
    return n_actions, pair_div


def _every_action(variant):
    """Every action of the variant as candidates (lookahead.candidate_pairs): pairs, or flat actions."""
    rng = ACTION_RANGES[variant]
    return [(a, m) for a in range(rng[0]) for m in range(rng[1])] if len(rng) == 2 else list(range(rng[0]))


def _check_objective(objective):
    if not callable(objective) and objective not in OBJECTIVES:
        raise ValueError("objective must be one of %s or a callable on read()" % (OBJECTIVES,))


def _recording(b):
    return b._lib.fjsp_env_schedule_capacity(b._h) > 0


def _seed_tensor(seed, dev):
    return torch.tensor([int(np.array(int(seed) & (2 ** 64 - 1), dtype=np.uint64).view(np.int64))], dtype=torch.int64, device=dev)


def play(batch, actor, greedy=True, seed=0, mo=None, max_steps=None, first=None, state_src=None, state_in=None,
         record_actions=False, fused=True):
    """Play every live env of `batch` from its current state to the end of its episode with `actor`.

    greedy: True = the first index of the largest probability (torch.argmax), False = a draw from the stream of
    fjsp_policy_sample with epsilon 0 and `seed` (counter = step index within this call, env = local index).
    mo: f64[N, 4] step arguments of the MO variants (as EnvBatch.step takes them).  max_steps: upper bound on the steps
    (default: the largest count of remaining operations).  first: u8[N, 2] actions in the env encoding that step 0
    applies instead of the actor's.  state_in / state_src: env i starts from row state_src[i] of state_in (f64[M, S];
    default: the batch's own state rows, row i).  record_actions: also return the applied actions.
    A batch with order arrivals is played in segments (fjsp_env_play_policy_orders) -- but through the loop, unless
    fused="segments", where the segments measured no gain: host arrival LPs and fewer than four envs per workgroup
    (EnvBatch.policy_orders_build; _segments_pay).  fused=False, or what the kernels
    refuse (an actor of another shape than state_size <= 32 -> 128 -> 128 -> n_actions <= 32, a MO_DFJSP batch), runs the
    per-step loop instead; with an actor of the in-kernel shape it takes the probabilities from the same device code
    (fjsp_actor_forward), so both give the same episode bit for bit.

    The batch's state / reward / done rows end as a step leaves them after each env's last step.  Returns
    dict(actions=u8[T, N, 2] device tensor or None -- the action applied at each step, zero past an env's end --,
    steps=i32[N] device tensor of the steps each env took)."""
    batch, mo = _unwrap(batch, mo)
    _, pair_div = action_encoding(actor, batch)
    return _play(batch, actor, pair_div, batch.N if greedy else 0, seed, mo, max_steps, first, state_src, state_in,
                 record_actions, fused)


def _play(b, actor, pair_div, n_greedy, seed, mo, T, first, src, state_in, record_actions, fused):
    N, dev = b.N, b.device
    mo = mo_rows(mo, N, dev)
    if first is not None:
        first = torch.as_tensor(first, device=dev).to(torch.uint8).reshape(N, 2).contiguous()
    state_in = b.state if state_in is None else state_in
    if state_in.dim() != 2 or state_in.shape[1] != b.state_size:
        raise ValueError("play: state_in must have shape (M, %d)" % b.state_size)
    state_in = state_in.to(device=dev, dtype=torch.float64).contiguous()
    if src is not None:
        src = torch.as_tensor(src, device=dev).to(torch.int32).reshape(-1).contiguous()
        if src.numel() != N or int(src.min()) < 0 or int(src.max()) >= state_in.shape[0]:
            raise ValueError("play: state_src must hold %d rows of state_in (0..%d)" % (N, state_in.shape[0] - 1))
        if state_in.data_ptr() == b.state.data_ptr():
            state_in = state_in.clone()          # (the kernel writes the batch's rows while other waves read the map)
    elif state_in.shape[0] != N:
        raise ValueError("play: without state_src, state_in must have %d rows" % N)
    if T is None:
        r = b.read()
        left = torch.where(r["done"] == 0, ops_per_env(b) - r["step_count"].long(), torch.zeros(N, dtype=torch.int64, device=dev))
        T = int(left.max().item())
    T = max(int(T), 1)           # (one launch even when every env is done: it still hands back the start rows)
    acts = torch.zeros(T, N, 2, dtype=torch.uint8, device=dev) if record_actions else None
    steps = torch.zeros(N, dtype=torch.int32, device=dev)
    seed_t = _seed_tensor(seed, dev)
    ap = native_actor_params(actor) if fused else None
    if ap is not None:
        args = (b._h, C.byref(ap), int(pair_div), int(n_greedy), _ptr(seed_t), T, _ptr(mo), _ptr(state_in), int(state_in.shape[0]),
                _ptr(src), _ptr(first), _ptr(acts), _ptr(steps), b._p_state, b._p_reward, b._p_done, b._stream())
        rc = b._lib.fjsp_env_play_policy(*args)
        if rc == _capi.FJSP_E_UNSUPPORTED and (fused == "segments" or _segments_pay(b)):
            rc = b._lib.fjsp_env_play_policy_orders(*args)     # order arrivals: one launch per segment, the arrival service between them
        if rc != _capi.FJSP_E_UNSUPPORTED:
            _capi.check(rc)
            return dict(actions=acts, steps=steps)
    _play_loop(b, actor, pair_div, n_greedy, seed_t, T, mo, state_in, src, first, acts, steps)
    return dict(actions=acts, steps=steps)


def _segments_pay(b):
    """Whether play takes fjsp_env_play_policy_orders by default for a batch the one-launch entry refused.  Not where it
    measured no gain over the per-step loop ("Order arrivals between policy launches"): arrival LPs on the
    host and shops so large that fewer than four envs fit a workgroup -- two waves per CU then play 4096 DA3C shops no faster
    than the loop's full-occupancy step kernel.  fused="segments" plays the segments there all the same."""
    if b.lp_on_device:
        return True
    out = (C.c_int32 * 4)()
    if b._lib.fjsp_env_policy_orders_build(b._h, int(b.state_size), out) != 0:
        return True                               # (not a batch the segments play: their entry says so itself)
    return out[0] >= 4


def _play_loop(b, actor, pair_div, n_greedy, seed_t, T, mo, state_in, src, first, acts, steps):
    """The per-step form of play_policy_kernel.  Each step goes through fjsp_env_rollout with T = 1, which steps only the
    envs that are neither done nor stopped by an error bit (EnvBatch.step would flag a done env with STEP_AFTER_DONE)."""
    N, dev = b.N, b.device
    x = state_in[src.long()] if src is not None else state_in
    if x.data_ptr() != b.state.data_ptr():
        b.state.copy_(x)
    native = native_actor_params(actor) is not None
    A = [m for m in actor.modules() if isinstance(m, torch.nn.Linear)][-1].out_features
    eps = torch.zeros((), dtype=torch.float32, device=dev)
    pair = torch.zeros(N, 2, dtype=torch.uint8, device=dev)
    flat = torch.zeros(N, dtype=torch.float32, device=dev)
    logp = torch.zeros(N, dtype=torch.float32, device=dev)
    r = b.read()
    for t in range(T):
        live = (r["done"] == 0) & ((r["status"].long() & _STOP_BITS) == 0)
        if not bool(live.any()):
            break
        if t == 0 and first is not None:
            a = first
        else:
            with torch.no_grad():
                probs = native_actor_forward(actor, b.state) if native else actor(b.state.float())
            probs = probs.float().contiguous()
            if n_greedy < N:
                _capi.check(b._lib.fjsp_policy_sample(_ptr(probs), N, A, int(pair_div), _ptr(eps), _ptr(seed_t), t, _ptr(pair),
                                                      _ptr(flat), _ptr(logp), b._stream()))
            if n_greedy > 0:
                g = torch.argmax(probs[:n_greedy], dim=1)
                pair[:n_greedy, 0] = (g // pair_div if pair_div else g).to(torch.uint8)
                pair[:n_greedy, 1] = (g % pair_div if pair_div else torch.zeros_like(g)).to(torch.uint8)
            a = pair
        _, rw, _ = b.rollout(a[None], trace=False, rewards=True, mo=mo, state=True)
        b.reward.copy_(torch.where(live, rw[0], b.reward))
        if acts is not None:
            acts[t] = torch.where(live[:, None], a, acts[t])
        steps += live.to(torch.int32)
        r = b.read()
    b.done.copy_(r["done"])


def best_of(batch, actor, k, objective, seed=0, mo=None, branch=None):
    """Decode every env k times and keep the best episode.  A branch batch of k x N envs (recording iff the source
    records) starts from the source's saved states; block 0 plays greedily in the source's own env slots, so it is
    exactly the source's greedy episode, random rules included, and blocks 1..k-1 sample (seed as in play).  Each source
    env then takes the first block with the lowest objective (its state, objective and, if recording, schedule).

    objective: as lookahead.rollout_dispatch.  branch: an EnvBatch of k x N envs (lookahead.make_branch), reused across
    calls, or None.  Returns dict(objective=tensor[N] of the source's finished episodes, best=i64[N] winning block,
    branch=the branch batch)."""
    batch, mo = _unwrap(batch, mo)
    k = int(k)
    if k < 1:
        raise ValueError("best_of: k must be at least 1, got %d" % k)
    _check_objective(objective)
    _, pair_div = action_encoding(actor, batch)
    N, dev = batch.N, batch.device
    branch = branch_for(batch, k, branch, "best_of")
    if _recording(branch) != _recording(batch):
        branch.record_schedule(_recording(batch))
    src = np.tile(np.arange(N, dtype=np.int64), k)
    branch.restore(batch.snapshot(), src, rows=False)
    _play(branch, actor, pair_div, N, seed, mo_rows(mo, N, dev, k), None, None, torch.as_tensor(src, device=dev), batch.state, False, True)
    rb = branch.read()
    check_status(rb, "branch", "best_of")
    if not bool((rb["done"] != 0).all()):
        raise RuntimeError("best_of: a branch env did not finish its episode")
    best = torch.argmin(objective_values(branch, objective, rb).reshape(k, N), dim=0)            # first minimum
    win = branch.snapshot(best * N + torch.arange(N, device=dev))
    batch.restore(win, rows=True)
    return dict(objective=objective_values(batch, objective), best=best, branch=branch)


def pareto_front(batch, actors, k, objectives=("makespan", "tardiness"), seed=0, mos=None, branch=None, keep_branches=False, cap=None,
                 timings=None):
    """The Pareto front, per env, of the P x k episodes that P actors decode: actor p plays a k x N branch exactly as
    best_of does (block 0 greedy in the source's own slots, blocks 1..k-1 sampled with `seed`), so candidate p * k + j is
    the episode best_of(batch, actors[p], k, ..., seed) plays in its block j; the finished episodes' objective vectors go
    through one pareto.select (P x k at most 1024).

    actors: one actor or a list of P (MPPPO's five policies along a weight vector).  objectives: 1..4 of "makespan",
    "tardiness", "energy" (MO_DFJSP) or callables on read(), lower is better.  mos: None (a wrapper's own `mo`), one
    f64[N, 4] for every actor, or a list of P of them.  branch: an EnvBatch of k x N envs (lookahead.make_branch) that
    every actor plays in turn, or None; with keep_branches=True each actor gets its own (branch: a list of P, or None)
    and they are returned still holding their finished episodes, recording iff the source records: a front member's
    schedule is branches[p].schedule() of env j * N + i.  cap: the front members kept per env (default P x k).
    timings: a dict that receives the synchronised seconds of the parts "play" and "select".
    The source batch is only read: its state rows, read() and schedule stay as they were.

    Returns dict(objectives=f64[P x k, N, D], index=i32[N, cap] the front's candidates in ascending lexicographic order
    of their vectors (-1 past the front), count=i32[N], mask=u8[P x k, N], front=f64[N, cap, D] (NaN past the front),
    policy=index // k and block=index % k (i32[N, cap], -1 past the front), branch=the branch batch or, with
    keep_branches, branches=the list of P)."""
    who = "pareto_front"
    batch, mo_own = _unwrap(batch, None)
    actors = list(actors) if isinstance(actors, (list, tuple)) else [actors]
    P, k = len(actors), int(k)
    if P < 1 or k < 1 or P * k > pareto.MAX_CANDIDATES:
        raise ValueError("%s: needs at least one actor, k >= 1 and at most %d episodes per env, got %d x %d" % (who, pareto.MAX_CANDIDATES, P, k))
    for o in objectives:
        _check_objective(o)
    if isinstance(mos, (list, tuple)):
        if len(mos) != P:
            raise ValueError("%s: mos must be None, one mo or one per actor (%d), got %d" % (who, P, len(mos)))
    else:
        mos = [mo_own if mos is None else mos] * P
    if keep_branches:
        branches = list(branch) if branch is not None else [None] * P
        if len(branches) != P:
            raise ValueError("%s: with keep_branches, branch must be None or one branch per actor (%d)" % (who, P))
    else:
        branches = [branch_for(batch, k, branch, who)] * P
    N, dev = batch.N, batch.device
    src = np.tile(np.arange(N, dtype=np.int64), k)
    src_dev = torch.as_tensor(src, device=dev)
    snap = batch.snapshot()
    clock = Clock(timings, dev)
    clock.start()
    obj = []
    for p, actor in enumerate(actors):
        _, pair_div = action_encoding(actor, batch)
        br = branches[p] = branch_for(batch, k, branches[p], who)
        if _recording(br) != _recording(batch):
            br.record_schedule(_recording(batch))
        br.restore(snap, src, rows=False)
        _play(br, actor, pair_div, N, seed, mo_rows(mos[p], N, dev, k), None, None, src_dev, batch.state, False, True)
        rb = br.read()
        check_status(rb, "branch", who)
        if not bool((rb["done"] != 0).all()):
            raise RuntimeError("%s: a branch env did not finish its episode" % who)
        obj.append(objective_vectors(br, objectives, rb, k))
    obj = torch.cat(obj, dim=0)
    clock.lap("play")
    index, count, mask = pareto.select(obj, cap=cap)
    clock.lap("select")
    on = index >= 0
    none = torch.full_like(index, -1)
    out = dict(objectives=obj, index=index, count=count, mask=mask, front=pareto.front_points(obj, index),
               policy=torch.where(on, index // k, none), block=torch.where(on, index % k, none))
    if keep_branches:
        out["branches"] = branches
    else:
        out["branch"] = branches[0]
    return out


def policy_lookahead(batch, actor, objective, candidates=None, mo=None, branch=None, timings=None):
    """lookahead.rollout_dispatch with the greedy actor as base policy: at every decision, branch block p applies
    candidate p through play's `first` and plays greedily to the end, all in one launch; each source env takes the
    candidate whose branch ended with the lowest objective (the first one on ties).

    candidates: as rollout_dispatch; None = every action of the variant.  Arguments, error handling, `timings` parts and
    the returned dict are those of rollout_dispatch.  When neither the candidates nor the actor's greedy choices use a
    random.choice rule, the dynamics are deterministic and the greedy choice is always among the candidates, so by the
    rollout algorithm's improvement property the objective reached is never above the greedy play's.  Random-rule
    actions continue on their branch slot's random stream, and the bound does not hold for them."""
    batch, mo = _unwrap(batch, mo)
    _check_objective(objective)
    _, pair_div = action_encoding(actor, batch)
    pairs = candidate_pairs(_every_action(batch.variant) if candidates is None else candidates, batch.variant)
    P, N = len(pairs), batch.N
    first = torch.as_tensor(pairs, device=batch.device)[:, None, :].expand(P, N, 2).reshape(P * N, 2).contiguous()   # candidate p in block p

    def play_branch(branch, T, mo_branch, src_dev, clock):
        _play(branch, actor, pair_div, P * N, 0, mo_branch, T, first, src_dev, batch.state, False, True)
        clock.lap("rollout")
        rb = branch.read()
        check_status(rb, "branch", "policy_lookahead")
        if not bool((rb["done"] != 0).all()):
            raise RuntimeError("policy_lookahead: a branch env did not finish its episode")
        return rb

    # (the source step returns a state: the next decision's actor input)
    return decide_by_rollouts(batch, pairs, objective, mo, branch, timings, "policy_lookahead", True, play_branch)


BEAM_SCORES = ("logp", "rollout")
BEAM_TIMINGS = ("forward", "select", "snapshot", "restore", "rollout", "step")


def beam_select(cost, done=None, width_out=None):
    """fjsp_beam_select (include/fjsp_amd.h) on the current stream: cost f64[W, N, A] on the device (beam-major: entry
    (b, i, a) = the cost of action a in beam b of source env i, NaN / +inf = no candidate), done u8[W, N] or None,
    width_out (default W) -> (parent i32, action i32, cost f64), each [width_out, N]: source env i's candidates in
    ascending (cost, parent, action), ranks past the last candidate (-1, -1, +inf)."""
    if not torch.is_tensor(cost) or cost.dim() != 3 or cost.dtype != torch.float64 or cost.device.type != "cuda":
        raise ValueError("beam_select: cost must be an f64[W, N, A] device tensor")
    W, N, A = cost.shape
    width_out = W if width_out is None else int(width_out)
    dev = cost.device
    cost = cost.contiguous()
    if done is not None:
        done = torch.as_tensor(done, device=dev).to(torch.uint8).reshape(W, N).contiguous()
    shape = (max(width_out, 0), N)
    parent = torch.empty(shape, dtype=torch.int32, device=dev)
    action = torch.empty(shape, dtype=torch.int32, device=dev)
    out = torch.empty(shape, dtype=torch.float64, device=dev)
    index = torch.cuda.current_device() if dev.index is None else dev.index
    _capi.check(_capi.lib().fjsp_beam_select(_ptr(cost), _ptr(done), N, W, A, width_out, _ptr(parent), _ptr(action), _ptr(out),
                                             _capi.stream(index)))
    return parent, action, out


def beam_search(batch, actor, width, objective=None, score="logp", candidates=None, mo=None, beams=None, expand=None, timings=None):
    """Play every env of `batch` (reset or mid-episode) to the end by beam search: `width` partial schedules per env,
    each expanded by every candidate action at every decision, the `width` best kept (fjsp_beam_select: ascending cost,
    equal costs by lower parent beam, then lower action -- the same result in every run).

    score="logp": a candidate's cost is its beam's cumulative cost minus the log (taken in f64) of the actor's
    probability of the action, so rank 0 ends as the most likely sequence the beam has kept and width 1 is greedy play.
    score="rollout": the cost is the `objective` (required) of the episode that applies the action in the beam and
    follows the greedy actor to the end, policy_lookahead's evaluation; width 1 is policy_lookahead.
    candidates: as policy_lookahead; None = every action of the variant; the others are never applied.
    beams: an EnvBatch of width x N envs (lookahead.make_branch), reused across calls, or None; it records its schedule
    iff the source does.  expand (rollout mode): one of width x P x N envs for the P candidates, or None.
    timings: a dict that receives the synchronised seconds per part: forward (the actor, logp mode), rollout (the
    expansion's play to the end, rollout mode), select, snapshot, restore, step.

    Beam 0 starts from the source's state with cost 0 and the others with cost +inf, so the first selection fans out
    from one beam.  A rank with no candidate left (fewer than `width` candidates) copies rank 0 and keeps cost +inf: it
    is never chosen.  When every beam has finished, each source env takes the first rank with the lowest objective
    (objective=None in logp mode: rank 0) with its rows and, when recording, its schedule.  Beams change slots at every
    decision, so, as restore() states, random-rule actions continue on another slot's random stream: with them the
    returned actions need not replay to the same episode; with deterministic rules they do, bit for bit.

    Returns dict(objective=tensor[N] of the source's finished episodes or None, best=i64[N] the winning rank, cost=
    f64[width, N] the ranks' final costs, actions=uint8[T, N, 2] numpy, the winner's action at each decision (zero past an
    env's end), steps=int[N] numpy decisions each env took, beams=the beam batch, expand=the expansion batch or None)."""
    who = "beam_search"
    W = int(width)
    if not 1 <= W <= 64:
        raise ValueError("beam_search: width must be 1..64, got %d" % W)
    if score not in BEAM_SCORES:
        raise ValueError("beam_search: score must be one of %s, got %r" % (BEAM_SCORES, score))
    if objective is None and score == "rollout":
        raise ValueError("beam_search: score='rollout' needs an objective")
    if objective is not None:
        _check_objective(objective)
    batch, mo = _unwrap(batch, mo)
    A, pair_div = action_encoding(actor, batch)
    pairs = candidate_pairs(_every_action(batch.variant) if candidates is None else candidates, batch.variant)
    P, N, dev = len(pairs), batch.N, batch.device
    check_branch_shape(N, batch.n_inst, W, who)
    beams = branch_for(batch, W, beams, who)
    expand = branch_for(batch, W * P, expand, who) if score == "rollout" else expand
    if _recording(beams) != _recording(batch):
        beams.record_schedule(_recording(batch))
    inf = float("inf")
    flat = torch.arange(A, device=dev)
    table = torch.stack([flat // pair_div, flat % pair_div] if pair_div else [flat, torch.zeros_like(flat)], 1).to(torch.uint8)   # action -> pair
    pairs_dev = torch.as_tensor(pairs, device=dev)
    cand = pairs_dev[:, 0].long() * pair_div + pairs_dev[:, 1].long() if pair_div else pairs_dev[:, 0].long()       # i64[P]
    allowed = torch.zeros(A, dtype=torch.bool, device=dev)
    allowed[cand] = True
    ar = torch.arange(N, device=dev)
    mo_beams = mo_rows(mo, N, dev, W)
    ops = ops_per_env(beams)
    beams.restore(batch.snapshot(), np.tile(np.arange(N, dtype=np.int64), W), rows=True)
    cum = torch.full((W, N), inf, dtype=torch.float64, device=dev)
    cum[0] = 0.0
    clock = Clock(timings, dev)
    if timings is not None:
        for part in BEAM_TIMINGS:
            timings.setdefault(part, 0.0)

    if score == "logp":
        native = native_actor_params(actor) is not None

        def costs(T, snap):
            with torch.no_grad():
                probs = native_actor_forward(actor, beams.state) if native else actor(beams.state.float())
            c = cum[:, :, None] - torch.log(probs.double()).reshape(W, N, A)
            c = torch.where(allowed, c, torch.full_like(c, inf))
            clock.lap("forward")
            return c
    else:
        src_h = (np.arange(W)[:, None, None] * N + np.zeros((1, P, 1), np.int64) + np.arange(N)[None, None, :]).reshape(-1)
        src_dev = torch.as_tensor(src_h.astype(np.int32), device=dev)        # expansion env (b * P + p) * N + i <- beam env b * N + i
        first = pairs_dev[None, :, None, :].expand(W, P, N, 2).reshape(W * P * N, 2).contiguous()          # ... applies candidate p
        mo_expand = mo_rows(mo, N, dev, W * P)
        restored = []

        def costs(T, snap):
            expand.restore(snap, src_dev if restored else src_h, rows=False)       # (the host map is validated once)
            restored.append(True)
            clock.lap("restore")
            _play(expand, actor, pair_div, W * P * N, 0, mo_expand, T, first, src_dev, beams.state, False, True)
            clock.lap("rollout")
            re = expand.read()
            check_status(re, "expansion", who)
            if not bool((re["done"] != 0).all()):
                raise RuntimeError("beam_search: an expansion env did not finish its episode")
            c = torch.full((W, N, A), inf, dtype=torch.float64, device=dev)
            c[:, :, cand] = objective_values(expand, objective, re).reshape(W, P, N).permute(0, 2, 1)
            return c

    snap, back_parent, back_action = None, [], []
    prev_live, prev_count = None, None
    r = beams.read()
    while True:
        check_status(r, "beam", who)
        live = r["done"] == 0
        count = r["step_count"].long()
        if prev_live is not None and bool((prev_live & live & (count <= prev_count)).any()):
            raise RuntimeError("beam_search: a beam env did not advance in its step")
        if not bool(live.any()):
            break
        T = int(torch.where(live, ops - count, torch.zeros_like(ops)).max().item())
        clock.start()
        snap = beams.snapshot(out=snap)
        clock.lap("snapshot")
        cost = costs(T, snap)
        done = r["done"].reshape(W, N)
        cost = torch.where((cum < inf)[:, :, None], cost, torch.full_like(cost, inf))     # a rank without a beam expands nothing
        cost[:, :, 0] = torch.where(done != 0, cum, cost[:, :, 0])                        # a finished beam stays, at its cost
        parent, action, cum = beam_select(cost, done, W)
        none = parent < 0
        if bool((none[0] & live[:N]).any()):
            raise RuntimeError("beam_search: a source env has no candidate left (every candidate's cost is +inf or NaN)")
        parent, action = torch.where(none, parent[:1], parent), torch.where(none, action[:1], action)
        clock.lap("select")
        beams.restore(snap, (parent.long() * N + ar).reshape(-1), rows=True)
        clock.lap("restore")
        live = torch.gather(live.reshape(W, N), 0, parent.long()).reshape(-1)
        count = torch.gather(count.reshape(W, N), 0, parent.long()).reshape(-1)
        act = table[action.clamp(min=0).long().reshape(-1)]
        _, rw, _ = beams.rollout(act[None].contiguous(), trace=False, rewards=True, mo=mo_beams, state=True)
        beams.reward.copy_(torch.where(live, rw[0], beams.reward))
        clock.lap("step")
        back_parent.append(parent)
        back_action.append(action)
        prev_live, prev_count = live, count
        r = beams.read()
    beams.done.copy_(r["done"])

    if objective is None:
        best = torch.zeros(N, dtype=torch.int64, device=dev)
    else:
        final = objective_values(beams, objective, r).reshape(W, N)
        best = torch.argmin(torch.where(cum < inf, final, torch.full_like(final, inf)), dim=0)          # first minimum
    batch.restore(beams.snapshot(best * N + ar), rows=True)

    # the winner's actions: follow the back-pointers from its final rank to the first decision
    D = len(back_parent)
    actions, steps = np.zeros((D, N, 2), np.uint8), np.zeros(N, np.int64)
    if D:
        bp, ba, tab = torch.stack(back_parent).cpu().numpy(), torch.stack(back_action).cpu().numpy(), table.cpu().numpy()
        rank, cols = best.cpu().numpy(), np.arange(N)
        for t in range(D - 1, -1, -1):
            a = ba[t, rank, cols]
            took = a >= 0                        # (-1: the env had finished before this decision)
            actions[t, took] = tab[a[took]]
            steps += took
            rank = bp[t, rank, cols]
    return dict(objective=None if objective is None else objective_values(batch, objective), best=best, cost=cum, actions=actions,
                steps=steps, beams=beams, expand=expand)


IMPROVE_OBJECTIVES = ("makespan", "tardiness")


def _machine_tables(b):
    """(koff int64[n_inst, R_max] first operation type of a kind, elig bool[n_inst, K_max, M_max] p > 0) on the device,
    from the batch's instance arrays (read back from the device for a generated batch)."""
    arrs = [b.instance_arrays(i) for i in range(b.n_inst)]
    R, K, M = max(len(a.Jr) for a in arrs), max(np.asarray(a.p).shape[0] for a in arrs), max(np.asarray(a.p).shape[1] for a in arrs)
    koff, elig = np.zeros((b.n_inst, R), np.int64), np.zeros((b.n_inst, K, M), bool)
    for i, a in enumerate(arrs):
        p = np.asarray(a.p)
        koff[i, :len(a.Jr)] = np.concatenate(([0], np.cumsum(np.asarray(a.Jr, np.int64))))[:-1]
        elig[i, :p.shape[0], :p.shape[1]] = p > 0
    return torch.from_numpy(koff).to(b.device), torch.from_numpy(elig).to(b.device)


IMPROVE_NEIGHBOURHOODS = ("uniform", "critical", "mixed")
CRITICAL_MOVES = 128          # moves of a critical path that improve draws from (schedule.critical's max_moves)


def _uniform_moves(sch, draw, L, k, elig, inst, odd):
    """int32[N, Q, 3] from draw f64[2, N, Q]: candidate q even -- a uniform row on a machine drawn uniformly from its
    operation's eligible ones; q odd -- a uniform row exchanged with its successor.  k int[N, cap]: the rows' operation types."""
    N, Q = draw.shape[1], draw.shape[2]
    env = torch.arange(N, device=draw.device)
    span = torch.where(odd, (L - 1)[:, None], L[:, None]).clamp(min=1)
    u = torch.minimum((draw[0] * span).to(torch.int64), span - 1)
    e = elig[inst[:, None], k[env[:, None], u].to(torch.int64).clamp(min=0)]                       # [N, Q, M]
    pick = torch.minimum((draw[1] * e.sum(-1)).to(torch.int64), e.sum(-1) - 1).clamp(min=0)
    m_new = ((e.cumsum(-1) == (pick + 1)[..., None]) & e).to(torch.int8).argmax(-1)
    return torch.stack([torch.where(odd, sch.MOVE_SWAP, sch.MOVE_MACHINE).expand(N, Q), u, m_new], -1).to(torch.int32)


def improve(batch, plan, rounds, neighbours=64, objective="makespan", seed=0, sideways=True, neighbourhood="uniform"):
    """Hill climbing on explicit schedules (schedule.decode, fjsp_schedule_decode): from one plan per env, `rounds` rounds
    of `neighbours` random neighbours per env, all N x neighbours of a round decoded by one launch.

    plan: int32[N, cap, 3] rows (r, n, m), e.g. schedule.plan_of(batch.schedule()[0]); every plan must decode.  A round
    draws on the device, from a torch.Generator seeded with `seed`: candidate q even -- a uniform row runs on a machine
    drawn uniformly from its operation's eligible ones (MOVE_MACHINE); q odd -- a uniform row changes places with its
    successor (MOVE_SWAP).  Of the candidates that decode (status 0) the env takes the one of least `objective`
    ("makespan" or "tardiness"), the lowest q among equals, if it is better than its plan, or as good with sideways=True,
    and applies that move to its plan (schedule.apply_moves).  Nothing synchronises with the host inside the loop.

    neighbourhood: "uniform" -- the draws above; "critical" (objective "makespan" only) -- every round puts the plan and
    its table into begin order (schedule.begin_order), takes the moves of its critical path (schedule.critical, the first
    CRITICAL_MOVES of them: the exchange of two operations that follow each other on a machine of the path, then the path's
    operations on their other machines) and draws every candidate uniformly from that list; an env whose list is empty
    has no candidates in the round; "mixed" -- candidates q < neighbours // 2 from the critical list, the others as
    "uniform" draws them.  Both decode the accepted plans once more per round, for the next round's table.

    A MO_DFJSP batch decodes through schedule.decode_dyn (fjsp_schedule_decode_dyn): objective may also be "energy", the
    returned objective has that third column, and neighbourhood must be "uniform" -- the critical-path analysis adds
    durations along a path, and the shift a breakdown window gives an operation depends on when it is dispatched.

    Returns dict(plan=int32[N, cap, 3], objective=int64[N, 2] (makespan, tardiness) of it, history=int64[rounds + 1, N] the
    chosen objective of the input plan and after every round, accepted=int64[N] moves taken, table=int32[N, cap, 6] and
    length=int32[N] of the final plans); rounds=0 returns the input plan."""
    from . import schedule as sch
    b, _ = _unwrap(batch, None)
    dyn = b.variant == sch.VARIANT_MO_DFJSP
    objectives = IMPROVE_OBJECTIVES + (("energy",) if dyn else ())
    decode = sch.decode_dyn if dyn else sch.decode
    if objective not in objectives:
        raise ValueError("objective must be one of %s" % (objectives,))
    if neighbourhood not in IMPROVE_NEIGHBOURHOODS:
        raise ValueError("neighbourhood must be one of %s" % (IMPROVE_NEIGHBOURHOODS,))
    if dyn and neighbourhood != "uniform":
        raise ValueError("neighbourhood %r: critical paths are not analysed on MO_DFJSP (breakdown shifts are not additive in the "
                         "durations): neighbourhood must be 'uniform'" % (neighbourhood,))
    if neighbourhood != "uniform" and objective != "makespan":
        raise ValueError("neighbourhood %r follows the critical path of the makespan: objective must be 'makespan'" % (neighbourhood,))
    rounds, Q = int(rounds), int(neighbours)
    if rounds < 0 or Q < 1:
        raise ValueError("improve needs rounds >= 0 and neighbours >= 1")
    col = objectives.index(objective)
    dev, N = b.device, b.N
    first = decode(b, plan, want_table=True)
    if bool((first["status"] != 0).any()):
        raise ValueError("improve: a plan does not decode (status %s)" % sorted(set(first["status"].flatten().tolist()) - {0}))
    koff, elig = _machine_tables(b)
    inst = torch.arange(N, device=dev) % b.n_inst
    tab = first["table"][:, 0].to(torch.int64)
    L = first["length"][:, 0].to(torch.int64)
    # the operation type of a table's rows
    op_types = lambda tab: torch.where(tab[..., 0] >= 0, koff[inst[:, None], tab[..., 0].clamp(min=0)] + tab[..., 1], torch.full_like(tab[..., 0], -1))
    cur = first["objective"][:, 0, col].clone()
    history = torch.empty(rounds + 1, N, dtype=torch.int64, device=dev)
    history[0] = cur
    accepted = torch.zeros(N, dtype=torch.int64, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    odd = (torch.arange(Q, device=dev) % 2 == 1)[None, :]
    worst = torch.iinfo(torch.int64).max
    env = torch.arange(N, device=dev)

    def select(moves, res, masked=None):
        """(chosen int32[N, 3], take bool[N], best int64[N]): the round's winner per env, MOVE_NONE where none is taken."""
        ok = res["status"] == 0 if masked is None else (res["status"] == 0) & ~masked
        obj = torch.where(ok, res["objective"][..., col], torch.full((), worst, dtype=torch.int64, device=dev))
        best, q = obj.min(1)
        q = (obj == best[:, None]).to(torch.int8).argmax(1)                                             # the lowest q among equals
        take = (best != worst) & ((best < cur) | ((best == cur) & bool(sideways)))
        chosen = moves[env, q].clone()
        chosen[~take, 0] = sch.MOVE_NONE
        return chosen, take, best

    if neighbourhood == "uniform":
        # rows (r, n, m, k): the operation type travels with its row (neither move changes a row's stage)
        rows = torch.cat([sch.plan_of(tab), op_types(tab)[..., None]], -1).to(torch.int32)
        for t in range(rounds):
            draw = torch.rand(2, N, Q, generator=gen, device=dev, dtype=torch.float64)
            moves = _uniform_moves(sch, draw, L, rows[..., 3], elig, inst, odd)
            res = decode(b, rows[..., :3].contiguous(), moves, Q)
            chosen, take, best = select(moves, res)
            rows = sch.apply_moves(rows, chosen[:, None])[:, 0]
            cur = torch.where(take, best, cur)
            accepted += take
            history[t + 1] = cur
        last = decode(b, rows[..., :3].contiguous(), want_table=True)
        return dict(plan=rows[..., :3].contiguous(), objective=last["objective"][:, 0], history=history, accepted=accepted,
                    table=last["table"][:, 0], length=last["length"][:, 0])

    last, out_plan = first, None
    from_path = (torch.arange(Q, device=dev) < (Q if neighbourhood == "critical" else Q // 2))[None, :].expand(N, Q)
    for t in range(rounds):
        pl, tab = sch.begin_order(last["table"][:, 0])
        crit = sch.critical(b, tab, 1, CRITICAL_MOVES)
        listed = crit["n_moves"][:, 0].to(torch.int64).clamp(max=CRITICAL_MOVES)[:, None]              # [N, 1]
        draw = torch.rand(3, N, Q, generator=gen, device=dev, dtype=torch.float64)
        slot = torch.minimum((draw[2] * listed).to(torch.int64), listed - 1).clamp(min=0)
        moves = crit["moves"][:, 0][env[:, None], slot]
        if neighbourhood == "mixed":
            moves = torch.where(from_path[..., None], moves, _uniform_moves(sch, draw[:2], L, op_types(tab.to(torch.int64)), elig, inst, odd))
        res = sch.decode(b, pl.contiguous(), moves, Q)
        chosen, take, best = select(moves, res, from_path & (listed == 0))
        out_plan = sch.apply_moves(pl, chosen[:, None])[:, 0].contiguous()
        last = sch.decode(b, out_plan, want_table=True)
        cur = torch.where(take, best, cur)
        accepted += take
        history[t + 1] = cur
    if out_plan is None:
        out_plan = torch.as_tensor(plan, device=dev).to(torch.int32).contiguous()
    return dict(plan=out_plan, objective=last["objective"][:, 0], history=history, accepted=accepted,
                table=last["table"][:, 0], length=last["length"][:, 0])


def local_search(batch, plan, rounds, neighbours=64, objective="makespan", seed=0, accept="sideways", tenure=8, neighbourhood="uniform",
                 trace=False):
    """improve's search as ONE launch for all its rounds (schedule.search, fjsp_schedule_search, csrc/fjsp_decode.hip): one
    wavefront owns an env, each lane decodes one neighbour, the round's winner is a reduction over the wave and the plan
    stays on the CU.  The moves, the neighbourhoods and the selection are improve's; the draws are not -- a counter-based
    splitmix64 stream of (seed, global env id, round, candidate) that include/fjsp_amd.h states and schedule.search_draws
    returns, so a shard of a batch (EnvBatch first_env) searches exactly as those envs of the whole batch do.

    plan: int32[N, cap, 3], every plan must decode.  neighbours: 1..64.  accept: "strict" -- the round's best neighbour is
    taken if it is better than the plan; "sideways" -- or as good (improve's sideways=True); "tabu" -- the best neighbour
    that is not tabu is taken, better or worse: a move makes the rows it moved tabu for `tenure` further rounds, a tabu
    move is admissible only where it beats the best plan seen (aspiration), moves that change nothing are not candidates,
    and the best plan seen is returned.  neighbourhood: as improve; "critical" and "mixed" need objective "makespan".

    A MO_DFJSP batch is searched by schedule.search_dyn (fjsp_schedule_search_dyn) and decoded by schedule.decode_dyn:
    objective may also be "energy", the returned objective has that third column, and neighbourhood must be "uniform", as
    in improve.

    Returns improve's dict -- plan=int32[N, cap, 3], objective=int64[N, 2] of it ([N, 3] on MO_DFJSP), history=int64[rounds
    + 1, N] the chosen objective of the input plan and of the current plan after every round, accepted=int64[N], table=
    int32[N, cap, 6] and length=int32[N] of the returned plans (one schedule.decode or decode_dyn) -- and status=int32[N]
    (zeros), with trace=True also trace=int32[rounds, N, 3], the move each round took ((0, 0, 0): none; indices into the
    plan the round started from).
    ValueError for arguments improve refuses, neighbours > 64, tenure < 0 and a plan that does not decode; FjspError
    where the library refuses (an env's working set beyond a CU's LDS: EnvBatch.search_lds, search_dyn_lds)."""
    from . import schedule as sch
    b, _ = _unwrap(batch, None)
    dyn = b.variant == sch.VARIANT_MO_DFJSP
    objectives = sch.SEARCH_DYN_OBJECTIVES if dyn else sch.SEARCH_OBJECTIVES
    if objective not in objectives:
        raise ValueError("objective must be one of %s" % (objectives,))
    if neighbourhood not in sch.SEARCH_NEIGHBOURHOODS:
        raise ValueError("neighbourhood must be one of %s" % (sch.SEARCH_NEIGHBOURHOODS,))
    if accept not in sch.SEARCH_ACCEPT:
        raise ValueError("accept must be one of %s" % (sch.SEARCH_ACCEPT,))
    if dyn and neighbourhood != "uniform":
        raise ValueError("neighbourhood %r: critical paths are not analysed on MO_DFJSP (breakdown shifts are not additive in the "
                         "durations): neighbourhood must be 'uniform'" % (neighbourhood,))
    if neighbourhood != "uniform" and objective != "makespan":
        raise ValueError("neighbourhood %r follows the critical path of the makespan: objective must be 'makespan'" % (neighbourhood,))
    rounds, Q, tenure = int(rounds), int(neighbours), int(tenure)
    if rounds < 0 or not 1 <= Q <= sch.SEARCH_MAX_NEIGHBOURS or tenure < 0:
        raise ValueError("local_search needs rounds >= 0, neighbours in 1..%d and tenure >= 0" % sch.SEARCH_MAX_NEIGHBOURS)
    if dyn:
        res = sch.search_dyn(b, plan, rounds, Q, objectives.index(objective), sch.SEARCH_ACCEPT.index(accept), tenure, seed, trace)
    else:
        res = sch.search(b, plan, rounds, Q, objectives.index(objective), sch.SEARCH_NEIGHBOURHOODS.index(neighbourhood),
                         sch.SEARCH_ACCEPT.index(accept), tenure, seed, trace)
    if bool((res["status"] != 0).any()):
        raise ValueError("local_search: a plan does not decode (status %s)" % sorted(set(res["status"].tolist()) - {0}))
    last = (sch.decode_dyn if dyn else sch.decode)(b, res["plan"], want_table=True)
    out = dict(plan=res["plan"], objective=res["objective"], history=res["history"], accepted=res["accepted"].to(torch.int64),
               table=last["table"][:, 0], length=last["length"][:, 0], status=res["status"])
    if trace:
        out["trace"] = res["trace"]
    return out


def left_shift(batch, plan):
    """The active schedules of explicit plans, as plans every other entry takes: schedule.decode_active
    (fjsp_schedule_decode_active: each operation goes into the earliest idle interval of its machine that is long enough and
    begins no earlier than its job is ready), then schedule.begin_order of its tables.

    plan: int32[N, cap, 3] or [N, K, cap, 3] (for instance genetic_search's population), every plan must decode.
    Returns dict(plan=int32 of plan's shape, the begin-ordered plan of the active table; table=int32[..., cap, 6] in begin
    order; objective=int64[..., 2] of it; inserted=int32[...] the rows that went into a gap; before=int64[..., 2], what
    schedule.decode makes of the input plan), device tensors.  No entry of objective exceeds before's: every row ends no
    later than in the semi-active decode of the same plan.
    The returned plan decodes through schedule.decode to exactly `table` and `objective`.  Closure: sorting stably by begin
    keeps every job's and every machine's sequence of the active table, because begin increases strictly along both (p >
    0); the semi-active decode of that plan gives every row max(end of its job predecessor or its arrival, end of its
    machine predecessor), which is at most its active begin (induction over the rows), and no less: the machine is idle
    from that time to the row's active begin in the finished table, so it was when the row was placed, and the row, ready
    by then, would have started there.  So improve, local_search, front_search, seed_population and
    genetic_search can start from a left-shifted plan without knowing this function.
    ValueError for a plan of another shape or one that does not decode; FjspError where the library refuses (MO_DFJSP)."""
    from . import schedule as sch
    b, _ = _unwrap(batch, None)
    if not torch.is_tensor(plan):
        plan = torch.as_tensor(np.asarray(plan))
    if plan.dim() not in (3, 4):
        raise ValueError("plan must be [N, cap, 3] or [N, K, cap, 3], got %s" % (tuple(plan.shape),))
    K = 1 if plan.dim() == 3 else int(plan.shape[1])
    act = sch.decode_active(b, plan, None, K, want_table=True)
    if bool((act["status"] != 0).any()):
        raise ValueError("left_shift: a plan does not decode (status %s)" % sorted(set(act["status"].flatten().tolist()) - {0}))
    before = sch.decode(b, plan, None, K)["objective"]
    new_plan, table = sch.begin_order(act["table"])
    out = dict(plan=new_plan.contiguous(), table=table, objective=act["objective"], inserted=act["inserted"], before=before)
    return {k: v[:, 0] for k, v in out.items()} if plan.dim() == 3 else out


def merge_fronts(front_obj, held, n_inst):
    """The front per instance over the archives of its envs (front_search's merge=True): front_obj int64[N, F, NO], held
    bool[N, F] (the slot has a member), env e on instance e % n_inst -> (merged_front f64[n_inst, C, NO], NaN past the front,
    merged_count int32[n_inst]) through pareto.select, C = ceil(N / n_inst) x F.  ValueError if C exceeds pareto.select's 1024
    candidates or a member is 2^53 or more (the vectors go through f64)."""
    N, F, n_obj = front_obj.shape
    n_group, dev = -(-N // n_inst), front_obj.device
    if n_group * F > pareto.MAX_CANDIDATES:
        raise ValueError("merge: %d envs of an instance x cap_front %d exceed pareto.select's %d candidates" % (n_group, F, pareto.MAX_CANDIDATES))
    if bool(((front_obj >= 2 ** 53) & held[..., None]).any()):
        raise ValueError("merge: an objective of 2^53 or more does not pass through f64")
    pad = n_group * n_inst - N
    held = torch.cat([held, torch.zeros(pad, F, dtype=torch.bool, device=dev)])
    vec = torch.cat([front_obj, torch.full((pad, F, n_obj), -1, dtype=torch.int64, device=dev)]).to(torch.float64)
    # candidate-major: candidate k * F + s of instance i is slot s of env k * n_inst + i
    vec = vec.reshape(n_group, n_inst, F, n_obj).permute(0, 2, 1, 3).reshape(n_group * F, n_inst, n_obj).contiguous()
    held = held.reshape(n_group, n_inst, F).permute(0, 2, 1).reshape(n_group * F, n_inst)
    index, count, _ = pareto.select(vec, held)
    return pareto.front_points(vec, index), count


def front_search(batch, plan, rounds, weights=None, neighbours=64, cap_front=64, accept="tabu", tenure=8, seed=0, merge=False):
    """local_search for a front, not a minimum (schedule.search_front, fjsp_schedule_search_front, csrc/fjsp_decode.hip): the
    same one-launch search on either family, steered per env by the key sum_c weights[e, c] * objective[c], and every
    vector it decodes -- the input plan, every neighbour of every round, taken or not -- offered to the env's Pareto
    archive of `cap_front` slots (1..64), which the wave keeps in LDS.  Envs that share an instance and differ in their
    weights sweep the weight simplex over it.

    weights: None (ones), a vector of NO non-negative integers that are not all zero (every env's), or [N, NO]; NO = 3
    (makespan, tardiness, energy) on MO_DFJSP, 2 elsewhere.  The other arguments are local_search's; the neighbourhood is
    the uniform one.

    Returns local_search's dict, history holding the key, and
      front      int64[N, cap_front, NO]  the archive's members first, in ascending lexicographic order of their vectors
                                          (fjsp_pareto_select's order), -1 past count
      front_plan int32[N, cap_front, cap, 3], front_src int32[N, cap_front, 2]  their plans and the (round, q) that found
                                          them ((-1, 0): the input plan), permuted alike, -1 past count
      count      int32[N]                 members;  dropped int32[N]: entrants that found no free slot and were lost --
                                          raise cap_front or split the weights over more envs
    and with merge=True, per instance, merged_front f64[n_inst, C, NO] (NaN past the front) and merged_count int32[n_inst]:
    the front (pareto.select) of the archives of all envs i with i % n_inst the instance, C = envs of an instance x
    cap_front, which must not exceed 1024.
    ValueError for arguments local_search refuses, cap_front outside 1..64, weights of another shape, negative or all zero,
    a plan that does not decode, and with merge C > 1024 or a member >= 2^53 (the vectors go through f64); FjspError where
    the library refuses (EnvBatch.search_front_lds)."""
    from . import schedule as sch
    b, _ = _unwrap(batch, None)
    n_obj = 3 if b.variant == sch.VARIANT_MO_DFJSP else 2
    if accept not in sch.SEARCH_ACCEPT:
        raise ValueError("accept must be one of %s" % (sch.SEARCH_ACCEPT,))
    rounds, Q, F, tenure = int(rounds), int(neighbours), int(cap_front), int(tenure)
    if rounds < 0 or not 1 <= Q <= sch.SEARCH_MAX_NEIGHBOURS or not 1 <= F <= 64 or tenure < 0:
        raise ValueError("front_search needs rounds >= 0, neighbours in 1..%d, cap_front in 1..64 and tenure >= 0" % sch.SEARCH_MAX_NEIGHBOURS)
    dev, N = b.device, b.N
    w = torch.ones(n_obj, dtype=torch.int64) if weights is None else torch.as_tensor(weights)
    if w.is_floating_point() or w.dim() not in (1, 2) or w.shape[-1] != n_obj or (w.dim() == 2 and w.shape[0] != N):
        raise ValueError("weights must be integers of shape (%d,) or (%d, %d)" % (n_obj, N, n_obj))
    w = w.to(device=dev, dtype=torch.int64).expand(N, n_obj).contiguous()
    if bool(((w < 0).any(1) | (w == 0).all(1)).any()):
        raise ValueError("weights must be non-negative and not all zero in every env")
    n_group = -(-N // b.n_inst)
    if merge and n_group * F > pareto.MAX_CANDIDATES:
        raise ValueError("merge: %d envs of an instance x cap_front %d exceed pareto.select's %d candidates" % (n_group, F, pareto.MAX_CANDIDATES))
    res = sch.search_front(b, plan, w, rounds, Q, F, sch.SEARCH_ACCEPT.index(accept), tenure, seed)
    if bool((res["status"] != 0).any()):
        raise ValueError("front_search: a plan does not decode (status %s)" % sorted(set(res["status"].tolist()) - {0}))
    last = (sch.decode_dyn if n_obj == 3 else sch.decode)(b, res["plan"], want_table=True)
    # members first, in ascending lexicographic order: stable sorts from the least significant column up, free slots last
    obj, src = res["front_obj"], res["front_src"]
    order = torch.arange(F, device=dev).expand(N, F)
    for key in [obj[..., c] for c in range(n_obj - 1, -1, -1)] + [(src[..., 1] < 0).to(torch.int64)]:
        order = torch.gather(order, 1, torch.sort(torch.gather(key, 1, order), dim=1, stable=True).indices)
    out = dict(plan=res["plan"], objective=res["objective"], history=res["history"], accepted=res["accepted"].to(torch.int64),
               table=last["table"][:, 0], length=last["length"][:, 0], status=res["status"],
               front=torch.gather(obj, 1, order[..., None].expand(N, F, n_obj)),
               front_plan=torch.gather(res["front_plan"], 1, order[..., None, None].expand(N, F, *res["front_plan"].shape[2:])),
               front_src=torch.gather(src, 1, order[..., None].expand(N, F, 2)), count=res["front_count"], dropped=res["front_dropped"])
    if merge:
        out["merged_front"], out["merged_count"] = merge_fronts(obj, src[..., 1] >= 0, b.n_inst)
    return out


def seed_population(batch, plan, population, shake=4, seed=0):
    """A start population for genetic_search from one or a few plans per env: int32[N, population, cap, 3].  plan: int32[N,
    cap, 3] or [N, P0, cap, 3] (e.g. schedule.plan_of of a recorded schedule, or the K schedules best_of / pareto_front
    sampled); individual q is plan q mod P0, and for q >= P0 that plan after `shake` successive random moves of improve's
    uniform neighbourhood (_uniform_moves: a uniform row on a machine drawn uniformly from its operation's eligible ones, or
    a uniform row exchanged with its successor, in turns), applied by schedule.apply_moves.  Drawn on the device from a
    torch.Generator seeded with `seed`: the same arguments give the same population.  Neither move can make a plan invalid,
    so every individual decodes when the sources do.  ValueError for population outside 1..64, shake < 0, a plan of
    another shape or one that does not decode."""
    from . import schedule as sch
    b, _ = _unwrap(batch, None)
    P, shake = int(population), int(shake)
    if not 1 <= P <= sch.EVOLVE_MAX_POPULATION or shake < 0:
        raise ValueError("seed_population needs population in 1..%d and shake >= 0" % sch.EVOLVE_MAX_POPULATION)
    dev, N, cap = b.device, b.N, b.decode_capacity()
    plan = torch.as_tensor(plan).to(device=dev, dtype=torch.int32)
    if plan.dim() == 3:
        plan = plan[:, None]
    if plan.dim() != 4 or tuple(plan.shape) != (N, plan.shape[1], cap, 3) or plan.shape[1] < 1:
        raise ValueError("plan must have shape %s or %s, got %s" % ((N, cap, 3), (N, "P0", cap, 3), tuple(plan.shape)))
    P0 = int(plan.shape[1])
    pop = plan[:, torch.arange(P, device=dev) % P0].contiguous()
    first = (sch.decode_dyn if b.variant == sch.VARIANT_MO_DFJSP else sch.decode)(b, pop, n_cand=P, want_table=True)
    if bool((first["status"] != 0).any()):
        raise ValueError("seed_population: a plan does not decode (status %s)" % sorted(set(first["status"].flatten().tolist()) - {0}))
    if shake == 0 or P <= P0:
        return pop
    koff, elig = _machine_tables(b)
    inst = (torch.arange(N, device=dev) % b.n_inst).repeat_interleave(P)
    tab = first["table"].reshape(N * P, cap, 6).to(torch.int64)
    L = first["length"].reshape(N * P).to(torch.int64)
    k = torch.where(tab[..., 0] >= 0, koff[inst[:, None], tab[..., 0].clamp(min=0)] + tab[..., 1], torch.full_like(tab[..., 0], -1))
    # rows (r, n, m, k): the operation type travels with its row (neither move changes a row's stage)
    rows = torch.cat([pop.reshape(N * P, cap, 3).to(torch.int64), k[..., None]], -1).to(torch.int32)
    q = torch.arange(P, device=dev).repeat(N)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    for s in range(shake):
        draw = torch.rand(2, N * P, 1, generator=gen, device=dev, dtype=torch.float64)
        moves = _uniform_moves(sch, draw, L, rows[..., 3], elig, inst, ((q + s) % 2 == 1)[:, None])
        moves[q < P0, 0, 0] = sch.MOVE_NONE                                                             # the given plans stay
        rows = sch.apply_moves(rows, moves)[:, 0]
    return rows[..., :3].reshape(N, P, cap, 3).contiguous()


def genetic_search(batch, population, generations, objective="makespan", weights=None, mutation=0.1, seed=0, merge=False,
                   decoder="semi_active"):
    """A genetic algorithm on explicit schedules, every generation of every env in ONE launch (schedule.evolve,
    fjsp_schedule_evolve, csrc/fjsp_decode.hip): a wavefront owns an env, a lane an individual.  Per generation child 0 is
    the best individual unchanged (the elite); every other child draws two parents by binary tournaments, takes the rows of
    a random set of jobs from the first in place and the remaining rows from the second in its order (precedence-preserving
    order crossover; a row keeps its machine), is mutated with probability `mutation` (one uniform row on a machine drawn
    uniformly from its operation's eligible ones), and is decoded by the lane while it is built.  Draws are a counter-based
    splitmix64 stream of (seed, global env id, generation, child): a shard of a batch evolves exactly as those envs of the
    whole batch do.

    population: int32[N, P, cap, 3], P in 1..64, every plan must decode (seed_population makes one).  objective: the
    single objective minimised, "makespan" or "tardiness", on MO_DFJSP also "energy"; weights, if given, replace it as in
    front_search: a vector of NO non-negative integers that are not all zero, or [N, NO], the key being their weighted sum.

    Returns dict(plan=int32[N, cap, 3] and objective=int64[N, NO] of the best individual of the last generation,
    history=int64[generations + 1, N] the least key of every generation (it never increases), population=int32[N, P, cap, 3]
    and population_objective=int64[N, P, NO] the last generation, status=int32[N] (zeros)) and with merge=True, per instance,
    merged_front f64[n_inst, C, NO] (NaN past the front) and merged_count int32[n_inst]: the front (pareto.select) of the
    last generations of all envs i with i % n_inst the instance, C = envs of an instance x P, which must not exceed 1024.
    decoder: "semi_active" scores every individual with schedule.decode (decode_dyn on MO_DFJSP): a row starts behind
    everything its machine holds.  "active" scores it with schedule.decode_active, the decoder of the FJSP literature: a
    row takes the earliest idle interval of its machine that fits (schedule.evolve_active, fjsp_schedule_evolve_active, the
    same one launch).  The chromosomes are not rewritten: plan and population hold the rows as the crossover merged them,
    objective, population_objective and history are their ACTIVE objectives, and the dict gains inserted=int32[N, P] (the rows
    each individual of the last generation placed in a gap) and active_plan=int32[N, cap, 3], table=int32[N, cap, 6]: the
    left_shift of `plan`, in begin order, which schedule.decode decodes to `objective` -- the form the other searches take.
    RuntimeError if left_shift's objective is not `objective` (the two entries disagree).

    ValueError for an unknown objective or decoder, generations < 0, mutation outside 0..1, a population or weights of
    another shape, bad weights, a plan that does not decode, and with merge C > 1024 or an objective >= 2^53; FjspError
    where the library refuses (EnvBatch.evolve_lds; decoder="active" on MO_DFJSP)."""
    from . import schedule as sch
    b, _ = _unwrap(batch, None)
    if decoder not in ("semi_active", "active"):
        raise ValueError("decoder must be \"semi_active\" or \"active\", got %r" % (decoder,))
    objectives = sch.SEARCH_DYN_OBJECTIVES if b.variant == sch.VARIANT_MO_DFJSP else sch.SEARCH_OBJECTIVES
    n_obj = len(objectives)
    if weights is None and objective not in objectives:
        raise ValueError("objective must be one of %s" % (objectives,))
    generations, mutation = int(generations), float(mutation)
    if generations < 0 or not 0.0 <= mutation <= 1.0:
        raise ValueError("genetic_search needs generations >= 0 and mutation in 0..1")
    dev, N = b.device, b.N
    population = torch.as_tensor(population)
    if population.dim() != 4 or not 1 <= population.shape[1] <= sch.EVOLVE_MAX_POPULATION:
        raise ValueError("population must be [N, P, cap, 3] with P in 1..%d, got %s" % (sch.EVOLVE_MAX_POPULATION, tuple(population.shape)))
    P = int(population.shape[1])
    w = torch.eye(n_obj, dtype=torch.int64)[objectives.index(objective)] if weights is None else torch.as_tensor(weights)
    if w.is_floating_point() or w.dim() not in (1, 2) or w.shape[-1] != n_obj or (w.dim() == 2 and w.shape[0] != N):
        raise ValueError("weights must be integers of shape (%d,) or (%d, %d)" % (n_obj, N, n_obj))
    w = w.to(device=dev, dtype=torch.int64).expand(N, n_obj).contiguous()
    if bool(((w < 0).any(1) | (w == 0).all(1)).any()):
        raise ValueError("weights must be non-negative and not all zero in every env")
    n_group = -(-N // b.n_inst)
    if merge and n_group * P > pareto.MAX_CANDIDATES:
        raise ValueError("merge: %d envs of an instance x population %d exceed pareto.select's %d candidates" % (n_group, P, pareto.MAX_CANDIDATES))
    run = sch.evolve_active if decoder == "active" else sch.evolve
    res = run(b, population, generations, w, int(round(mutation * sch.EVOLVE_MUT_ONE)), seed)
    if bool((res["status"] != 0).any()):
        raise ValueError("genetic_search: a plan does not decode (status %s)" % sorted(set(res["status"].tolist()) - {0}))
    out = dict(plan=res["plan"], objective=res["objective"], history=res["history"], population=res["population"],
               population_objective=res["population_objective"], status=res["status"])
    if decoder == "active":
        shifted = left_shift(b, res["plan"])
        if not torch.equal(shifted["objective"], res["objective"]):
            raise RuntimeError("genetic_search: decode_active of the winner does not give evolve_active's objective")
        out.update(inserted=res["inserted"], active_plan=shifted["plan"], table=shifted["table"])
    if merge:
        held = torch.ones(N, P, dtype=torch.bool, device=dev)
        out["merged_front"], out["merged_count"] = merge_fronts(res["population_objective"], held, b.n_inst)
    return out
