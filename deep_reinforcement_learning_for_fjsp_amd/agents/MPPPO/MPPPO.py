"""Batched counterpart of the reference's agents/MPPPO/MPPPO.py (on-policy update
path).  The MLPs, the return normalisation and the
clipped-PPO update stay in PyTorch-ROCm (MFMA only in the dense GEMMs); rollouts
come from the HIP environment batch and land in the C-ABI rollout buffer.

What is kept from the reference, by line:
  ActorNet / CriticNet                 MPPPO.py:31-67   (Linear+ReLU stack, softmax head)
  pick_action_and_log_prob             :272-284         (Categorical sample, epsilon-random override)
  calculate_discounted_returns         :301-312         (reverse scan, f32 element arithmetic)
  normalise to [0,1] then standardise  :258-261         (+1e-8, unbiased std)
  advantages = G - V(s)                :263
  ratio / clipped surrogate            :325-352         (exp(new) / (exp(old) + 1e-8), clip 0.2)
  Adam(lr 3e-4, eps 1e-4), grad-clip 1 :145-147,358-370
  equalise_policies                    :372-375
Two defects of the shipped script are fixed rather than replicated (SURVEY.md row
a21): the critic loss is not detached before backward (:319 makes the critic
never train), and equalise_policies copies `.data` (:375 `algorithm_means`
raises AttributeError at the end of the first episode).
Kept as the reference has them (tests/test_ppo_update.py pins both):
  exploration rate of a round          :240-241         eps = 1 / (1 + episode / denominator), then ONE draw
                                                        max(0, uniform(eps / 3, eps * 3)) per round -- from the
                                                        agent's own seeded `random.Random` (the reference uses the
                                                        unseeded global one), shared by every env of the batch
  multi_policy_update                  :192-203         policy P scores ITS OWN test objectives under every
                                                        policy's weight vector and moves towards the policy at
                                                        the arg-min index (see MPPPO.multi_policy_update)
"""
import ctypes as C
import random
import torch
import torch.nn.functional as F
from torch import nn, optim
from torch.distributions import Categorical

from .Buffer import RolloutBuffer
from ..Base_Agent import Base_Agent
from ..linear import run_layers
from ..native_actor import native_actor_forward, native_actor_params
from ... import _capi
from ... import distributed as fdist

HYPER = {   # utilities/data_structures/Config.py "MP_PPO"
    "learning_rate": 0.0003, "discount_rate": 0.99, "clip_epsilon": 0.2, "gradient_clipping_norm": 1.0,
    "learning_iterations_per_round_actor": 10, "learning_iterations_per_round_critic": 10,
    "epsilon_decay_rate_denominator": 10, "normalized_rewards": True, "standardized_rewards": True, "tau": 0.005,
}


class ActorNet(nn.Module):
    """MPPPO.py:31-48"""

    def __init__(self, input_size, hidden_size, hidden_layer, output_size):
        super().__init__()
        self.layers = nn.ModuleList([nn.Linear(input_size, hidden_size), nn.ReLU()])
        for _ in range(hidden_layer - 1):
            self.layers.append(nn.Linear(hidden_size, hidden_size))
            self.layers.append(nn.ReLU())
        self.layers.append(nn.Linear(hidden_size, output_size))

    def forward(self, x):
        return F.softmax(run_layers(self.layers, x), dim=-1)

    def log_prob(self, x, actions):
        """log of the softmax probability of `actions` -- what Categorical(self(x)).log_prob(actions) returns
        (MPPPO.py:327-328), computed as log_softmax + gather: two passes over the [samples, actions] matrix
        instead of softmax, renormalisation, clamp, log and gather."""
        return F.log_softmax(run_layers(self.layers, x), dim=-1).gather(1, actions.unsqueeze(1)).squeeze(1)


class CriticNet(nn.Module):
    """MPPPO.py:51-67"""

    def __init__(self, input_size, hidden_size, hidden_layer, output_size):
        super().__init__()
        self.layers = nn.ModuleList([nn.Linear(input_size, hidden_size), nn.ReLU()])
        for _ in range(hidden_layer - 1):
            self.layers.append(nn.Linear(hidden_size, hidden_size))
            self.layers.append(nn.ReLU())
        self.layers.append(nn.Linear(hidden_size, output_size))

    def forward(self, x):
        return run_layers(self.layers, x)


# ----------------------------------------------------------------------------- math
def discounted_returns(rewards, valid, gamma):
    """MPPPO.py:301-312 for [T, N] f32 tensors: G_t = r_t + gamma * G_{t+1} per env, walking back over
    valid rows, f32 multiply then f32 add (the reference's tensor-element arithmetic)."""
    T = rewards.shape[0]
    g = torch.zeros_like(rewards[0])
    out = torch.zeros_like(rewards)
    gam = torch.tensor(gamma, dtype=rewards.dtype, device=rewards.device)
    for t in range(T - 1, -1, -1):
        g_new = rewards[t] + gam * g
        g = torch.where(valid[t] > 0, g_new, g)
        out[t] = torch.where(valid[t] > 0, g, torch.zeros_like(g))
    return out


def normalise_returns(G, valid, normalized=True, standardized=True):
    """MPPPO.py:258-261 applied per env (each env's episode is one reference episode)."""
    m = valid > 0
    if normalized:
        big = torch.finfo(G.dtype).max
        gmin = torch.where(m, G, torch.full_like(G, big)).min(0).values
        gmax = torch.where(m, G, torch.full_like(G, -big)).max(0).values
        G = (G - gmin) / (gmax - gmin + 1e-8)
    if standardized:
        n = m.sum(0).clamp(min=1).to(G.dtype)
        mean = (G * m).sum(0) / n
        var = (((G - mean) ** 2) * m).sum(0) / (n - 1).clamp(min=1)    # torch .std() is unbiased
        G = (G - mean) / (var.sqrt() + 1e-8)
    return G * m


def actor_loss_terms(new_log_prob, old_log_prob, advantages, clip_epsilon):
    """MPPPO.py:325-352 per sample (the caller takes -mean over valid samples)."""
    ratio = torch.exp(new_log_prob) / (torch.exp(old_log_prob) + 1e-8)
    return torch.min(advantages * ratio, advantages * torch.clamp(ratio, 1.0 - clip_epsilon, 1.0 + clip_epsilon))


class PPOLearner(object):
    """Networks + optimisers + one clipped-PPO learning round over a [T, N] rollout.

    Data parallel over env shards: every rank holds the same parameters, computes the
    gradient of (sum of its samples' losses) / (global sample count), the flat gradient
    bucket is all-reduced (ONE RCCL call per optimiser step) and clipped
    after the reduction so all ranks apply the identical update."""

    def __init__(self, state_size, action_size, hidden_size=128, hidden_layer=2, critic_hidden_layer=2,
                 device="cpu", seed=0, hyper=None, train_critic=True):
        self.hp = dict(HYPER)
        self.hp.update(hyper or {})
        self.device = torch.device(device)
        self.fused_learn = True            # GPU batches of >= 32 k samples train through agents/fused_mlp.py
        self.mfma_learn = True             # ... with forward + loss + backward of a network in ONE launch (csrc/fjsp_mlp_train.hip)
        self.two_chains = True             # ... and the actor's iterations on a stream of their own where _fused_trainer allows it
        self._fused = None
        gen_state = torch.random.get_rng_state()
        torch.manual_seed(seed)            # identical initial parameters on every rank
        self.actor_new = ActorNet(state_size, hidden_size, hidden_layer, action_size).to(self.device)
        self.actor_old = ActorNet(state_size, hidden_size, hidden_layer, action_size).to(self.device)
        self.critic = CriticNet(state_size, hidden_size, critic_hidden_layer, 1).to(self.device)
        torch.random.set_rng_state(gen_state)
        Base_Agent.copy_model_over_dict(self.actor_new, self.actor_old)
        fused = self.device.type == "cuda"       # one multi-tensor kernel per optimiser step instead of one per parameter
        adam = dict(lr=self.hp["learning_rate"], eps=1e-4, fused=fused, capturable=fused)   # capturable: step count on the device
        self.actor_optimizer = optim.Adam(self.actor_new.parameters(), **adam)
        self.critic_optimizer = optim.Adam(self.critic.parameters(), **adam)
        self._path = None                # see `path`
        self.graph_learn = False         # replay the learning round from a HIP graph once its sample count repeats
        if self.device.type == "cuda":
            self._fused_nets()           # re-homes the parameters into flat buffers NOW: before any graph captures their addresses
        self._actor_stream = torch.cuda.Stream(device=self.critic.layers[0].weight.device) if self.device.type == "cuda" else None
        self._learn_graph = None
        self.action_size = action_size
        self.train_critic = train_critic
        self.actor_bucket = fdist.FlatGradBucket(self.actor_new.parameters())
        self.critic_bucket = fdist.FlatGradBucket(self.critic.parameters())

    @torch.no_grad()
    def act(self, states, epsilon=0.0, generator=None):
        """pick_action_and_log_prob (:272-284) for a batch of states [N, S] (f32)."""
        probs = self.actor_new(states)
        dist = Categorical(probs, validate_args=False)      # (the validation syncs with the host: illegal in a graph capture)
        action = dist.sample()
        if torch.is_tensor(epsilon) or epsilon > 0.0:
            u = torch.rand(action.shape, device=action.device, generator=generator)
            rnd = torch.randint(0, self.action_size, action.shape, device=action.device, generator=generator)
            action = torch.where(u <= epsilon, rnd, action)
        return action, dist.log_prob(action)

    @property
    def path(self):
        """Which trainer owns the optimiser state: "fused" (agents/fused_mlp.py, its own Adam moments) or "eager" (the torch
        optimisers).  Decided ONCE, at the first learn() (None until then), from the smallest sample count over the ranks:
        a learner that switched per call would alternate between two sets of Adam moments, and ranks that decided from
        their own shard could take different paths and drift apart."""
        return self._path

    def learn(self, states, actions, old_log_prob, returns, valid):
        """critic_actor_learn (:314-323) on flattened [T*N] samples; returns (critic_loss, actor_loss).  The fused round
        takes no mask, it sees valid samples only: a learner on the fused path drops the other rows from every batch."""
        states = states.reshape(-1, states.shape[-1])
        actions = actions.reshape(-1)
        old_log_prob = old_log_prob.reshape(-1).detach()
        returns = returns.reshape(-1).detach()
        vmask = valid.reshape(-1) > 0
        if self._path == "fused" or (states.is_cuda and states.shape[0] >= (1 << 15)):
            # rows of finished environments carry no sample (up to a third of a [T, N] rollout): drop them once
            # per round instead of pushing them through every one of the 20 forward/backward passes
            idx = torch.nonzero(vmask).reshape(-1)
            states, actions, old_log_prob, returns = states[idx], actions[idx], old_log_prob[idx], returns[idx]
            vmask = torch.ones(idx.shape[0], dtype=torch.bool, device=states.device)
        m = vmask.to(states.dtype)
        if self._path is None:
            n_min = fdist.all_reduce_scalar_min(torch.tensor(float(states.shape[0]), device=states.device))
            want = self.fused_learn and states.is_cuda and self._fused_nets() is not None
            self._path = "fused" if (want and float(n_min) >= float(1 << 15)) else "eager"
        if self.graph_learn and states.is_cuda and not fdist.is_distributed():
            c_loss, a_loss = self._learn_graphed(states, actions, old_log_prob, returns, m)
        else:
            count = fdist.all_reduce_scalar_sum(m.sum())          # global number of samples
            c_loss, a_loss = self._learn_body(states, actions, old_log_prob, returns, m, count)
        return float(c_loss), float(a_loss)

    def _learn_body(self, states, actions, old_log_prob, returns, m, count):
        """One learning round on the trainer that owns the optimiser state; returns the last (critic, actor) losses as tensors.
        count: the global sample count as a tensor (single process: m.sum(), a device scalar without a host round trip)."""
        trainer = self._fused_trainer if self._path == "fused" else self._autograd_trainer
        return self._round(returns, *trainer(states, actions, old_log_prob, returns, m, count))

    def _round(self, returns, critic_start, critic_iterate, actor_iterate, scalar, side=None, side_reads=()):
        """critic_actor_learn (:314-323): advantages from the critic as it is BEFORE the round, n iterations of each network,
        equalise_policies; returns the last two losses, each through scalar().  What an iteration launches is the trainer's
        business.  critic_start() gives (V(s), loss): the critic's first iteration where its forward pass hands V(s) out,
        else a forward pass alone and loss None.  Once the advantages exist the two chains share no written tensor (the actor
        never reads the critic's new parameters inside a round), so with a stream `side` the actor's is issued there."""
        n = self.hp["learning_iterations_per_round_critic"]
        values, c_loss = critic_start()
        advantages = returns - values                                                              # :263
        if side is not None:
            side.wait_stream(torch.cuda.current_stream(side.device))
        with torch.cuda.stream(side):                  # (None: the current stream)
            for _ in range(n):
                a_loss = actor_iterate(advantages)                                                 # :325-352
        for _ in range(n - (c_loss is not None)):
            c_loss = critic_iterate()                                                              # F.mse_loss, :318
        if side is not None:
            torch.cuda.current_stream(side.device).wait_stream(side)
            for t in (advantages,) + side_reads:
                t.record_stream(side)
        self.equalise_policies()
        return scalar(c_loss), scalar(a_loss)

    def _autograd_trainer(self, states, actions, old_log_prob, returns, m, count):
        """_round's callables on autograd and the torch optimisers; `m` masks the rows that carry no sample."""
        def update(net, bucket, optimizer, loss):
            bucket.zero_()               # (gradients live in the all-reduce bucket)
            loss.backward()
            bucket.all_reduce()
            torch.nn.utils.clip_grad_norm_(net.parameters(), self.hp["gradient_clipping_norm"])
            optimizer.step()

        def critic_start():
            with torch.no_grad():
                return self.critic(states).squeeze(1), None

        def critic_iterate():
            c_loss = (((self.critic(states).squeeze(1) - returns) ** 2) * m).sum() / count     # F.mse_loss, :318
            if self.train_critic:
                update(self.critic, self.critic_bucket, self.critic_optimizer, c_loss)
            return c_loss

        def actor_iterate(advantages):
            terms = actor_loss_terms(self.actor_new.log_prob(states, actions), old_log_prob, advantages, self.hp["clip_epsilon"])
            a_loss = -(terms * m).sum() / count                                                 # -torch.mean(...), :351
            update(self.actor_new, self.actor_bucket, self.actor_optimizer, a_loss)
            return a_loss

        return critic_start, critic_iterate, actor_iterate, torch.Tensor.detach

    def _learn_graphed(self, states, actions, old_log_prob, returns, m):
        """A learning round is ~1 200 small launches whose host cost rivals their device time.  With a fixed set
        of environments the number of valid samples (one per operation) is the same every round, so the whole
        round is captured once for that sample count and replayed: the first round of a given size runs eagerly
        (it also creates the optimiser state the capture needs), the second is captured, later ones replay."""
        n = states.shape[0]
        g = self._learn_graph
        if g is None or g["n"] != n:
            self._learn_graph = {"n": n, "graph": None}
            return self._learn_body(states, actions, old_log_prob, returns, m, m.sum())
        if g["graph"] is None:
            g["in"] = [t.clone() for t in (states, actions, old_log_prob, returns, m)]
            torch.cuda.synchronize(self.device)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="relaxed"):
                g["out"] = self._learn_body(*g["in"], g["in"][4].sum())
            g["graph"] = graph
        for dst, src in zip(g["in"], (states, actions, old_log_prob, returns, m)):
            dst.copy_(src)
        g["graph"].replay()
        return g["out"]

    def _fused_nets(self):
        """(actor trainer, critic trainer) of agents/fused_mlp.py, created on first use; None when a network has another
        shape than Linear-ReLU-Linear-ReLU-Linear or lives on the CPU."""
        from .. import fused_mlp
        if self._fused is None:
            if not (fused_mlp.supported(self.actor_new.layers, self.device) and fused_mlp.supported(self.critic.layers, self.device)):
                self._fused = False
            else:
                hp = self.hp
                mk = lambda net: fused_mlp.FusedMLP(net.layers, lr=hp["learning_rate"], eps=1e-4, max_norm=hp["gradient_clipping_norm"])
                self._fused = (mk(self.actor_new), mk(self.critic))
        return self._fused or None

    def _fused_trainer(self, states, actions, old_log_prob, returns, m, count):
        """_round's callables on agents/fused_mlp.py: FusedMLP.iterate chooses the launches; every sample is valid (learn() dropped
        the others).  Where the critic's first iteration hands V(s) out and `two_chains` is set, the actor's chain gets the side
        stream: one chain's small launches (gradient finish, clip + Adam: 0.28 ms of a round) then run under the other's pass."""
        actor, critic = self._fused_nets()
        count = count.to(torch.float32).reshape(1)
        reduce = (lambda g: torch.distributed.all_reduce(g, op=torch.distributed.ReduceOp.SUM)) if fdist.is_distributed() else None
        how = dict(reduce=reduce, one_launch=self.mfma_learn)
        actions_f = actions.to(torch.float32).contiguous()
        states, returns, old_log_prob = states.contiguous(), returns.contiguous(), old_log_prob.contiguous()
        from_first_pass = critic.hands_out_values(update=self.train_critic, **how)

        def critic_iterate(values_out=None):
            return critic.iterate(1, states, returns, None, None, count, update=self.train_critic, values_out=values_out, **how)

        def critic_start():
            if not from_first_pass:
                return critic.forward(states).squeeze(1), None
            values = torch.empty(states.shape[0], dtype=torch.float32, device=states.device)
            return values, critic_iterate(values)

        def actor_iterate(advantages):
            return actor.iterate(0, states, actions_f, old_log_prob, advantages, count, self.hp["clip_epsilon"], **how)

        side = self._actor_stream if from_first_pass and self.two_chains else None
        return critic_start, critic_iterate, actor_iterate, lambda loss: loss[0].clone(), side, (actions_f, states, old_log_prob, count)

    def equalise_policies(self):
        """:372-375 with the AttributeError fixed."""
        with torch.no_grad():
            torch._foreach_copy_([p.data for p in self.actor_old.parameters()], [p.data for p in self.actor_new.parameters()])


class FusedSampler(object):
    """pick_action_and_log_prob (MPPPO.py:272-284) of a whole vector step in one launch of the library's
    `fjsp_policy_sample` (csrc/fjsp_rollout_buffer.hip) instead of ~15 small torch kernels: Categorical sample,
    epsilon override, log-probability, and the action already in the environment's u8 encoding.
    pair_div = size of the machine-rule axis for pair-action environments ([6, 5] -> 5), 0 for flat actions."""

    def __init__(self, N, T, n_actions, pair_div, device):
        self._lib, self._check, self._ptr, self._stream = _capi.lib(), _capi.check, _capi.ptr, _capi.stream
        self.N, self.A, self.div = int(N), int(n_actions), int(pair_div)
        self.eps = torch.zeros((), dtype=torch.float32, device=device)
        self.seed = torch.zeros((), dtype=torch.int64, device=device)
        self.pair = torch.zeros(N, 2, dtype=torch.uint8, device=device)
        self.flat_actions = torch.zeros(T, N, dtype=torch.float32, device=device)
        self.rounds = 0

    def new_round(self, exploration):
        """Fresh random stream + exploration rate for the next rollout (device scalars: a captured graph reads them)."""
        self.rounds += 1
        self.eps.fill_(float(exploration))
        self.seed.fill_((torch.initial_seed() * 0x9E3779B1 + self.rounds * 0x85EBCA77) & 0x7FFFFFFFFFFFFFFF)

    def sample(self, probs, t, log_prob_row):
        p, ptr = probs.contiguous(), self._ptr
        self._check(self._lib.fjsp_policy_sample(ptr(p), self.N, self.A, self.div, ptr(self.eps), ptr(self.seed), int(t),
                                                 ptr(self.pair), ptr(self.flat_actions[t]), ptr(log_prob_row),
                                                 self._stream(p.device.index)))
        return self.pair


def fused_policy_rollout(env, learner, memory, fused, old_log_prob, exploration, T):
    """The whole rollout loop (MPPPO.py:245-252) in ONE launch of fjsp_env_rollout_policy: the actor runs inside the
    environment kernel, rows go straight into `memory`.  A batch with order arrivals takes fjsp_env_rollout_policy_orders:
    one such launch per segment of the episode, the arrival service between them.  Returns False when the batch / network
    shape is not supported (MO_DFJSP, another network size): the caller falls back to the per-step loop."""
    ap = native_actor_params(learner.actor_new)
    if ap is None or ap.state_size != env.state_size:
        return False
    batch = env.batch
    mo = getattr(env, "mo", None)
    p = _capi.ptr
    memory.clear()
    state = env.reset()
    fused.new_round(exploration)
    args = (batch._h, memory._h, C.byref(ap), p(fused.eps), p(fused.seed), fused.div, int(T), p(mo), p(state), p(fused.flat_actions),
            p(old_log_prob), p(batch.state), _capi.stream(batch.device_index))
    rc = _capi.lib().fjsp_env_rollout_policy(*args)
    if rc == _capi.FJSP_E_UNSUPPORTED:
        rc = _capi.lib().fjsp_env_rollout_policy_orders(*args)
    if rc == _capi.FJSP_E_UNSUPPORTED:
        return False
    _capi.check(rc)
    batch.done.fill_(1)               # (read() reports the per-env flags; the vector mirror is refreshed lazily)
    return True


def _rollout_steps(env, memory, T, choose, early_exit):
    """T vector steps (MPPPO.py:245-252): action choice, HIP env step, rollout-buffer append.  choose(t, state) gives the
    step's action pair u8[N, 2] in the environment's encoding, the pair the buffer row stores, and the flat action index
    to write over the row's column 0 (None: the stored pair holds it).  early_exit: stop once every env is done, looked
    at every 8 steps (a host read, so not under graph capture)."""
    memory.clear()
    state = env.reset().clone()
    done = torch.zeros(env.N, dtype=torch.uint8, device=env.device)
    mo = getattr(env, "mo", None)
    for t in range(T):
        active = (done == 0).to(torch.uint8)
        pair, stored, flat = choose(t, state)
        nxt, rew, dn = env.batch.step(pair, mo=mo)
        memory.add_experience(state, stored, rew, nxt, dn, active)
        if flat is not None:
            memory.actions[t, :, 0] = flat.float()
        state, done = nxt.clone(), dn.clone()
        if early_exit and t % 8 == 7 and bool((done != 0).all()):
            break


def _sampled_choice(learner, sampler, old_log_prob, native_actor):
    """choose() of _rollout_steps: the actor's forward pass, then the sampler's one launch (pair, flat action and
    log-probability of step t).  native_actor: the actor as fjsp_env_rollout_policy evaluates it, not torch's."""
    def choose(t, state):
        if native_actor:
            probs = native_actor_forward(learner.actor_new, state)
        else:
            with torch.no_grad():
                probs = learner.actor_new(state.float())
        pair = sampler.sample(probs, t, old_log_prob[t])
        return pair, pair, None
    return choose


def per_step_rollout(env, learner, memory, sampler, old_log_prob, exploration, T, native_actor=False):
    """What fused_policy_rollout computes, one launch at a time: actor, fjsp_policy_sample, fjsp_env_step and
    fjsp_rollout_append per step, all T steps.  With native_actor=True the actor is fjsp_actor_forward, the in-launch
    kernels' arithmetic, and the two agree bit for bit: the reference path of those kernels' tests.  With
    native_actor=False it is the rollout a PPO agent with fused_sampling and no fused_rollout collects."""
    sampler.new_round(exploration)
    _rollout_steps(env, memory, T, _sampled_choice(learner, sampler, old_log_prob, native_actor), early_exit=False)


class RolloutCollector(object):
    """The rollout half of a PPO round (MPPPO.py:230-270) and what it keeps from round to round: the rollout buffer
    `memory`, the `sampler` (with fused_sampling), the log-probabilities `old_log_prob` [T, N] and, with use_graph, the
    captured `graph` of the T-step loop.  remake() says what is made anew when.  A round collects in one of three ways:
    in one launch (in_launch, where fused_policy_rollout takes the batch and the actor), by replaying the graph
    (use_graph), or step by step with an early exit.  pair_div: the size of the machine-rule axis of a pair-action
    environment ([6, 5] -> 5), 0 for flat actions."""

    def __init__(self, pair_div, fused_sampling=False, use_graph=False, in_launch=False):
        self.pair_div, self.use_graph, self.in_launch = int(pair_div), use_graph, in_launch
        self.fused_sampling = fused_sampling or in_launch
        self.memory = self.sampler = self.old_log_prob = None
        self.pair = self.blank = None                    # torch's sampling: see remake()
        self.graph = self.graph_of = self.eps = None     # use_graph: the graph, what it was captured for, its exploration rate

    def remake(self, env, learner, T):
        """The buffer when T grows or N or the state size changes; the sampler with the buffer, or when N, the action
        count, pair_div or T no longer fit; old_log_prob (and the pairs of torch's sampling) when the shape no longer
        fits; the graph when the env, the learner, the buffer, the sampler or T is another than at its capture."""
        N, device = env.N, env.device
        memory, sampler = self.memory, self.sampler
        if memory is None or memory.T < T or memory.N != N or memory.S != env.state_size:
            self.memory, sampler = RolloutBuffer(T, N, env.state_size, device=device.index or 0), None
        if self.fused_sampling and (sampler is None or sampler.N != N or sampler.A != learner.action_size
                                    or sampler.div != self.pair_div or sampler.flat_actions.shape[0] < T):
            sampler = FusedSampler(N, T, learner.action_size, self.pair_div, device)
        self.sampler = sampler
        if self.old_log_prob is None or self.old_log_prob.shape != (T, N):
            self.old_log_prob = torch.zeros(T, N, device=device)
            if not self.fused_sampling:    # the step's pair, and the zero pair the buffer rows store under the flat action
                self.pair, self.blank = torch.zeros(2, N, 2, dtype=torch.uint8, device=device)
        now = (env, learner, self.memory, sampler)
        if self.graph is not None and not (self.graph_of[4] == T and all(a is b for a, b in zip(self.graph_of, now))):
            self.graph = None

    def _choice(self, learner, exploration):
        """choose() of _rollout_steps: the sampler's, or learner.act on torch's generator with `exploration`, a float
        or (under graph capture: no host branch on its value) a 0-dim device tensor."""
        if self.sampler is not None:
            return _sampled_choice(learner, self.sampler, self.old_log_prob, native_actor=False)
        pair, blank, div, old_log_prob = self.pair, self.blank, self.pair_div, self.old_log_prob

        def choose(t, state):
            a, lp = learner.act(state.float(), exploration)
            old_log_prob[t] = lp
            if div:
                pair[:, 0] = (a // div).to(torch.uint8)
                pair[:, 1] = (a % div).to(torch.uint8)
            else:
                pair[:, 0] = a.to(torch.uint8)
            return pair, blank, a          # the flat action index is what the policy is trained on
        return choose

    def _capture(self, env, learner, T):
        """The whole T-step rollout captured ONCE into a HIP graph and replayed every round: a vector step is a chain
        of ~20 small launches (MLP, sampling, env kernel, buffer append), and replaying the chain from a graph removes
        the per-launch host cost that dominates the eager loop (rocprofv3: 31 ms of a 82 ms PPO round at 4096 envs).
        The exploration rate lives in a device scalar so that it can change between replays; there is no early exit,
        every replay plays T steps (finished environments idle, their rows are masked by `valid`)."""
        device = env.device
        self.eps = torch.zeros((), device=device)
        choose = self._choice(learner, self.eps)
        body = lambda: _rollout_steps(env, self.memory, T, choose, early_exit=False)
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):               # warm-up outside the capture (library handles, allocator)
            body()
        torch.cuda.current_stream(device).wait_stream(side)
        torch.cuda.synchronize(device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode="relaxed"):
            body()
        self.graph_of = (env, learner, self.memory, self.sampler, T)

    def collect(self, env, learner, exploration, T):
        """One batched episode of `learner`'s policy on `env` into self.memory and self.old_log_prob."""
        self.remake(env, learner, T)
        sampler = self.sampler
        if self.in_launch and fused_policy_rollout(env, learner, self.memory, sampler, self.old_log_prob, exploration, T):
            return
        if self.use_graph and self.graph is None:
            self._capture(env, learner, T)
        if sampler is not None:
            sampler.new_round(exploration)
        if self.use_graph:
            self.eps.fill_(float(exploration))
            self.graph.replay()
        else:
            _rollout_steps(env, self.memory, T, self._choice(learner, exploration), early_exit=True)

    def collect_and_learn(self, env, learner, exploration, T):
        """collect() + one learning round (MPPPO.py:230-270).  Returns (critic_loss, actor_loss)."""
        self.collect(env, learner, exploration, T)
        hp, memory = learner.hp, self.memory
        n = len(memory)
        flat = self.sampler.flat_actions[:n] if self.sampler is not None else memory.actions[:n, :, 0]
        G = memory.normalised_returns(hp["discount_rate"], hp["normalized_rewards"], hp["standardized_rewards"])
        return learner.learn(memory.states[:n], flat.long(), self.old_log_prob[:n], G, memory.valid[:n])


def jittered_exploration(episode_number, denominator, rng):
    """MPPPO.py:240-241: the round's epsilon-random rate, one draw per round."""
    eps = 1.0 / (1.0 + episode_number / denominator)
    return max(0.0, rng.uniform(eps / 3.0, eps * 3.0))


class PPO(Base_Agent):
    """The agent loop of MPPPO.py:230-270 over a batch of SO_FJSSP environments (BASELINE config 3).

    `environment` is a BatchedSOFJSSP; the flat action a in [0, 30) is the rule pair
    (a // 5, a % 5) of SO_FJSSP's [6, 5] action space."""

    def __init__(self, environment, hidden_size=128, hidden_layer=2, seed=0, hyper=None, max_steps=None, use_graph=False,
                 fused_sampling=False, fused_rollout=False):
        super().__init__()
        self.environment = environment
        # fused_rollout: the whole rollout loop in one launch with the actor inside the environment kernel
        # (fjsp_env_rollout_policy: every single-order batch, up to 256 operation types and as many jobs as create
        # admits; batches with order arrivals through fjsp_env_rollout_policy_orders, one launch per segment between
        # arrival services); falls back to the per-step loop for an actor of another shape than S -> 128 -> 128 -> A
        self.rollout = RolloutCollector(environment.actions_size[1], fused_sampling, use_graph, in_launch=fused_rollout)
        self.device = environment.device
        self.state_size = environment.state_size
        self.action_size = environment.actions_size[0] * environment.actions_size[1]
        self.learner = PPOLearner(self.state_size, self.action_size, hidden_size, hidden_layer, hidden_layer,
                                  device=self.device, seed=seed, hyper=hyper)
        self.learner.graph_learn = bool(use_graph)
        self.hyper_parameters = self.learner.hp
        self.max_steps = max_steps
        self.global_step_number = 0
        self._rng = random.Random(seed)

    @property
    def memory(self):
        return self.rollout.memory

    def run_one_policy_network(self, exploration=None):
        """One batched episode + one learning round. Returns (mean delay_time_sum, mean makespan, losses)."""
        hp = self.hyper_parameters
        if exploration is None:                                                         # :240-241
            exploration = jittered_exploration(self.episode_number, hp["epsilon_decay_rate_denominator"], self._rng)
        losses = self.rollout.collect_and_learn(self.environment, self.learner, exploration, self.max_steps or 64)
        memory = self.memory
        self.global_step_number += int(memory.valid[:len(memory)].sum().item())
        self.episode_number += 1
        r = self.environment.read()
        return float(r["delay_time_sum"].double().mean()), float(r["makespan"].double().mean()), losses


class MPPPO(Base_Agent):
    """Multi-policy PPO of agents/MPPPO/MPPPO.py:70-212 on batches of MO_FJSSP_discretes environments.

    actor_number policies share the environment; policy p is trained on the weight vector
    (1 - p/(n-1), p/(n-1)) (:111).  One epoch (:159-164): the completion policy (p = 0) and the tardiness
    policy (p = n-1) run first on the training batch and their per-environment objective values
    normalise the rewards of the weighted policies; every `evolve_every` epochs the policies are pulled
    towards the best policy for their weight vector (:192-205).

    Two defects of the shipped script are fixed, not replicated: completion_min / tardiness_min stay +inf
    there (:134-135, never updated), which zeroes every score of the evolution step; here they track the
    best test objectives seen.  `make_train_env()` is called once per epoch like
    generated_new_environment() (:149-154,160)."""

    def __init__(self, make_train_env, test_env, actor_number=5, hidden_size=200, hidden_layer=5, critic_layer=3,
                 seed=0, hyper=None, max_steps=64, evolve_every=30, fused_sampling=True):
        super().__init__()
        self.make_train_env, self.test_env = make_train_env, test_env
        self.rollout = RolloutCollector(0, fused_sampling)        # one buffer and one sampler serve every policy
        self.device = test_env.device
        self.actor_number = actor_number
        self.policy_tuple = tuple(range(actor_number))
        self.policy_completion, self.policy_tardiness = self.policy_tuple[0], self.policy_tuple[-1]
        self.policy_weight_tuple = self.policy_tuple[1:-1]
        self.weight_vector_dict = {p: (1 - 1 / (actor_number - 1) * p, 1 / (actor_number - 1) * p)
                                   for p in self.policy_tuple}                            # :111
        self.learners = {p: PPOLearner(25, 18, hidden_size, hidden_layer, critic_layer, device=self.device,
                                       seed=seed + p, hyper=hyper) for p in self.policy_tuple}
        self.hyper_parameters = self.learners[0].hp
        self.max_steps, self.evolve_every = max_steps, evolve_every
        self.completion_min = float("inf")
        self.tardiness_min = float("inf")
        self._rng = random.Random(seed)

    def run_one_policy_network(self, environment, policy_number, completion=None, tardiness=None):
        """:230-270 for every environment of the batch. Returns per-env (delay_time_sum, completion_time)."""
        hp = self.hyper_parameters
        eps = jittered_exploration(self.episode_number, hp["epsilon_decay_rate_denominator"], self._rng)   # :240-241
        environment.set_objective(self.weight_vector_dict[policy_number], completion, tardiness)
        self.rollout.collect_and_learn(environment, self.learners[policy_number], eps, self.max_steps)
        r = environment.read()
        return r["delay_time_sum"].double(), r["completion_time"].double()

    @torch.no_grad()
    def run_one_epoch(self, environment, policy_number, completion=None, tardiness=None):
        """:214-228: evaluation episode (epsilon 0, no learning). Returns mean (delay_time_sum, completion_time)."""
        environment.set_objective(self.weight_vector_dict[policy_number], completion, tardiness)
        state = environment.reset()
        done = torch.zeros(environment.N, dtype=torch.uint8, device=self.device)
        for t in range(self.max_steps):
            a, _ = self.learners[policy_number].act(state.float(), 0.0)
            state, _, done = environment.step(a)
            if t % 8 == 7 and bool((done != 0).all()):
                break
        r = environment.read()
        return float(r["delay_time_sum"].double().mean()), float(r["completion_time"].double().mean())

    def run_n_episodes(self, n):
        """:156-190. Returns the list of per-epoch {policy: (completion, tardiness)} test objectives."""
        history = []
        for _ in range(n):
            env = self.make_train_env()
            _, completion = self.run_one_policy_network(env, self.policy_completion)
            tardiness, _ = self.run_one_policy_network(env, self.policy_tardiness)
            completion, tardiness = completion.clamp(min=1.0), tardiness.clamp(min=1.0)
            for p in self.policy_weight_tuple:
                self.run_one_policy_network(env, p, completion=completion, tardiness=tardiness)
            objs = {}
            t_c, c = self.run_one_epoch(self.test_env, self.policy_completion)
            objs[self.policy_completion] = (c, t_c)
            t, c_t = self.run_one_epoch(self.test_env, self.policy_tardiness)
            objs[self.policy_tardiness] = (c_t, t)
            for p in self.policy_weight_tuple:
                t_p, c_p = self.run_one_epoch(self.test_env, p, completion=max(c, 1.0), tardiness=max(t, 1.0))
                objs[p] = (c_p, t_p)
            self.completion_min = min(self.completion_min, min(v[0] for v in objs.values()))
            self.tardiness_min = min(self.tardiness_min, min(v[1] for v in objs.values()))
            history.append(objs)
            self.episode_number += 1
            if self.episode_number % self.evolve_every == 0:
                self.multi_policy_update(objs)
        return history

    def multi_policy_update(self, policy_objectives, selection="reference"):
        """:192-203.  selection="reference": as the reference computes it -- for policy P the list
        [w_p[0] * C_P / C_min + w_p[1] * T_P / T_min for p in policies] scores P's OWN test objectives under every
        policy's weight vector, and P moves (soft update, tau) towards the policy at the arg-min index.
        selection="own_weight": the transposed reading (every policy's objectives under P's weight vector; P moves
        towards the policy that serves P's weights best) -- arguably what was meant, not what the reference does.
        Returns {policy: index it moved towards}."""
        import copy
        actors = {p: copy.deepcopy(self.learners[p].actor_new) for p in self.policy_tuple}
        critics = {p: copy.deepcopy(self.learners[p].critic) for p in self.policy_tuple}
        tau = self.hyper_parameters["tau"]
        cmin, tmin = max(self.completion_min, 1e-9), max(self.tardiness_min, 1e-9)
        chosen = {}
        for policy in self.policy_tuple:
            if selection == "reference":
                c, t = policy_objectives[policy]
                scores = [self.weight_vector_dict[p][0] * (c / cmin) + self.weight_vector_dict[p][1] * (t / tmin)
                          for p in self.policy_tuple]
            elif selection == "own_weight":
                w = self.weight_vector_dict[policy]
                scores = [w[0] * (policy_objectives[q][0] / cmin) + w[1] * (policy_objectives[q][1] / tmin)
                          for q in self.policy_tuple]
            else:
                raise ValueError("selection must be 'reference' or 'own_weight'")
            best = scores.index(min(scores))
            chosen[policy] = best
            self.soft_update_of_target_network(actors[best], self.learners[policy].actor_new, tau)
            self.soft_update_of_target_network(critics[best], self.learners[policy].critic, tau)
        return chosen
