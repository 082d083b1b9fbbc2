"""The asynchronous order-arrival service (fjsp_env_step_async, csrc/fjsp_arrivals.hip) at its edges.

Reference of every comparison: a second, identically created batch driven by the blocking fjsp_env_step with the same
applied actions (the blocking path is itself pinned to the C oracle by tests/test_gpu_parity.py), and for an env's first
episode the C oracle through helpers.play_oracle.  Comparison is per env, by a cursor over that env's applied actions:
state rows, rewards and done bit for bit against the blocking batch (against the oracle with helpers.assert_state_close:
the project's tolerance on the pow()-derived entries), read() totals where no autoreset is involved.

While an env is parked, and in the call where it resumes, it is shown the variant's random.choice rule pair, not its
own action, and every env's own actions include the random rules: a draw consumed for an action that must be ignored
moves the env's random stream and with it the trajectory.

The instances, and what makes the counts below exact, are tests/async_cases.py and tests/test_async_cases_host.py.
FJSP_ASYNC_RING and fjsp_env_async_stats (include/fjsp_amd.h) force and observe the paths: counters [0] batches handed to
the workers, [1] of them with a tail copy (more than 64 parked envs), [2] calls that found no free batch and waited,
[3] the largest batch.
"""
import numpy as np
import pytest

from tests import async_cases as AC
from tests import helpers as H

pytestmark = pytest.mark.gpu

STATE_KW = {AC.SO_FJSSP: {}, AC.SO_DFJSP: {}, AC.MO_DFJSP: dict(dyn=True)}


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _create(s, N, variant, ring=None, lp_threads=None):
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    with H.env_var("FJSP_ASYNC_RING", ring):
        b = EnvBatch(s, N, variant=variant, rng_seed=AC.RNG_SEED)
    for e in (0, N - 1):
        assert b.env_seed(e) == AC.env_seed(e)
    if lp_threads is not None:
        b.set_lp_threads(lp_threads)          # before the first step_async: the service sizes its worker pool there, once
    assert b.async_stats == (0, 0, 0, 0)
    b.reset()
    return b


def _play_blocking(torch, b, acts, mo, autoreset, target):
    """target[e] blocking steps of env e (all envs step in every call; without autoreset a finished env idles): rows
    [T, N, ...] of state / reward / done, valid where t < target[e]."""
    T, N = acts.shape[0], b.N
    st = torch.zeros(T, N, b.state_size, dtype=torch.float64, device=b.device)
    rw = torch.zeros(T, N, dtype=torch.float64, device=b.device)
    dn = torch.zeros(T, N, dtype=torch.uint8, device=b.device)
    for t in range(T):
        s, r, d = b.step(acts[t], autoreset=autoreset, mo=mo)
        st[t], rw[t], dn[t] = s, r, d
    tt = torch.arange(T, device=b.device)[:, None]
    valid = tt < target[None, :]
    return dict(state=st, reward=rw, done=dn, valid=valid)


def _play_async(torch, b, acts, mo, autoreset, target, junk_pair, each_call=None):
    """step_async until every env has applied target[e] actions.  Env e is shown acts[cursor[e], e], except while it is
    parked and in the call where it resumes: the junk pair there.  The row of a call counts for env e where ready[e] = 1.
    Returns the rows by cursor, the call in which each env first showed ready = 0 and the call in which it then first
    showed ready = 1 again.  each_call(call, ready, parked_prev): the caller's per-call checks (host tensors)."""
    T, N = acts.shape[0], b.N
    dev = b.device
    idx = torch.arange(N, device=dev)
    cursor = torch.zeros(N, dtype=torch.int64, device=dev)
    parked_prev = torch.zeros(N, dtype=torch.bool, device=dev)
    junk = torch.tensor(junk_pair, dtype=torch.uint8, device=dev).repeat(N, 1)
    st = torch.zeros(T, N, b.state_size, dtype=torch.float64, device=dev)
    rw = torch.zeros(T, N, dtype=torch.float64, device=dev)
    dn = torch.zeros(T, N, dtype=torch.uint8, device=dev)
    first_park = torch.full((N,), -1, dtype=torch.int64, device=dev)
    first_back = torch.full((N,), -1, dtype=torch.int64, device=dev)
    call, cap = 0, 20 * T + 20000
    while True:
        at = cursor.clamp(max=T - 1)
        shown = torch.where(parked_prev[:, None], junk, acts[at, idx])
        s, r, d, ready = b.step_async(shown, autoreset=autoreset, mo=mo)
        is_ready = ready != 0
        took = is_ready & (cursor < target)
        rows = at[took]
        st[rows, idx[took]] = s[took]; rw[rows, idx[took]] = r[took]; dn[rows, idx[took]] = d[took]
        first_back = torch.where((first_back < 0) & (first_park >= 0) & is_ready, torch.full_like(first_back, call), first_back)
        first_park = torch.where((first_park < 0) & ~is_ready, torch.full_like(first_park, call), first_park)
        if each_call is not None:
            each_call(call, is_ready.cpu().numpy(), parked_prev.cpu().numpy())
        cursor += took.long()
        parked_prev = ~is_ready
        call += 1
        if bool((cursor >= target).all()):
            break
        assert call < cap, "step_async: %d calls and %d envs still short of their steps" % (call, int((cursor < target).sum()))
    b.flush_arrivals(mo)
    assert b.parked == 0
    return dict(state=st, reward=rw, done=dn, first_park=first_park.cpu().numpy(), first_back=first_back.cpu().numpy(), calls=call)


def _assert_same_rows(torch, got, want, what):
    v = want["valid"]
    for key in ("state", "reward", "done"):
        g, w = got[key][v], want[key][v]
        if g.dtype == torch.float64:
            g, w = g.view(torch.int64), w.view(torch.int64)
        if not torch.equal(g, w):
            bad = (got[key] != want[key])
            bad = (bad.any(-1) if bad.dim() == 3 else bad) & v
            t, e = [int(x) for x in bad.nonzero()[0]]
            raise AssertionError("%s: %s differs from the blocking step's, first at applied step %d of env %d (%d rows differ)"
                                 % (what, key, t, e, int(bad.sum())))


def _assert_first_episode_matches_oracle(arrs_of_env, envs, acts_h, mo_rows, variant, got, what):
    st, rw, dn = got["state"].cpu().numpy(), got["reward"].cpu().numpy(), got["done"].cpu().numpy()
    for e in envs:
        a = arrs_of_env(e)
        want = H.play_oracle(a, a.x, acts_h[:, e], AC.env_seed(e), variant=variant, mo=None if mo_rows is None else mo_rows[e])
        Te = want["T"]
        tag = "%s env %d" % (what, e)
        assert Te == AC.ops_total(a), tag
        assert np.array_equal(H.bits(rw[:Te, e]), H.bits(want["reward"])), tag + " reward"
        assert np.array_equal(dn[:Te, e], want["done"].astype(np.uint8)), tag + " done"
        H.assert_state_close(st[:Te, e], want["states"], tag, **STATE_KW[variant])


# --------------------------------------------------------------------------------------------- lock-step: cases a, b, d, e

def _lockstep_actions(torch, variant, T, N):
    """Random rule pairs over the whole action space; every third env plays the random.choice pair throughout."""
    acts_h = AC.actions(variant, T, N, 500 + N)
    acts_h[:, ::3] = AC.RANDOM_PAIR[variant]
    return acts_h, torch.from_numpy(acts_h).cuda()


def _lockstep(torch, N, names, lp_threads=None, ring=None):
    """One episode of N envs over the lock-step instances `names`, asynchronous against blocking and oracle.  The envs of
    instance i all park in call ops_first(i) - 1 (tests/test_async_cases_host.py) and nowhere else.  Returns the
    asynchronous batch and its blocking twin."""
    variant = AC.SO_FJSSP
    s = AC.instance_set(names, variant)
    n_inst = len(names)
    arrs = [s.arrays(i) for i in range(n_inst)]
    inst_of = np.arange(N) % n_inst
    ops = np.array([AC.ops_total(a) for a in arrs])[inst_of]
    T = int(ops.max())
    acts_h, acts = _lockstep_actions(torch, variant, T, N)
    target = torch.from_numpy(ops).cuda()
    a = _create(s, N, variant)
    want = _play_blocking(torch, a, acts, None, False, target)
    b = _create(s, N, variant, ring=ring, lp_threads=lp_threads)
    park_call = {AC.ops_first(arrs[i]) - 1: i for i in range(n_inst)}
    assert len(park_call) == n_inst
    seen = []

    def each_call(call, ready, parked_prev):
        # ready = 0 for the first time exactly in the parking call of the env's instance: there for all of its envs, and
        # every env that is not parked (still, from an earlier call) shows ready = 1
        newly = ~ready & ~parked_prev
        expect = (inst_of == park_call[call]) if call in park_call else np.zeros(N, bool)
        assert np.array_equal(newly, expect), "call %d: envs %s parked, expected %s" % (call, np.nonzero(newly)[0], np.nonzero(expect)[0])
        if call in park_call:
            seen.append(call)
    got = _play_async(torch, b, acts, None, False, target, AC.RANDOM_PAIR[variant], each_call)
    assert sorted(seen) == sorted(park_call)
    what = "lock-step N=%d" % N
    _assert_same_rows(torch, got, want, what)
    _assert_first_episode_matches_oracle(lambda e: arrs[inst_of[e]], range(0, N, max(1, N // 40)), acts_h, None, variant, got, what)
    fa, fb = a.read(), b.read()
    for k in fa:
        assert k == "status" or torch.equal(fa[k], fb[k]), k
    assert int(((fb["status"] & ~4) != 0).sum()) == 0            # (4: finished envs kept receiving actions)
    assert b.lp_solves == a.lp_solves == N
    return a, b


@pytest.mark.parametrize("N,names", [(7, ("lock3",)), (64, ("lock3",)), (65, ("lock3",)), (300, AC.LOCKSTEP)])
def test_park_count_boundaries(torch_gpu, N, names):
    """N < 64 (the head copy and the pinned mirrors are capped at N), exactly 64 (no tail copy), 65 (a tail copy of one
    env) and 150 + 150 envs of two instances that park in two different calls (two tail copies, mirrors grown), one LP
    worker: every env keeps its trajectory, the counters name the path, and the memo answers all but n_inst LPs."""
    n_inst = len(names)
    a, b = _lockstep(torch_gpu, N, names, lp_threads=1)
    group = N // n_inst
    batches, tails, waits, largest = b.async_stats
    assert largest == group
    assert batches == n_inst
    assert tails == (n_inst if group > 64 else 0)
    assert waits == 0                                            # a handful of calls cannot fill a ring of 32
    assert b.lp_cache_hits == b.lp_solves - n_inst               # one worker: no concurrent misses
    assert a.async_stats == (0, 0, 0, 0)                         # the blocking twin never used the service


def test_default_threads(torch_gpu):
    """The 150 + 150 case on the default worker pool: same trajectories and LP count; several workers may miss the memo at
    once, so the hits are only bounded."""
    a, b = _lockstep(torch_gpu, 300, AC.LOCKSTEP)
    assert b.async_stats[:2] == (2, 2) and b.async_stats[3] == 150
    assert 0 <= b.lp_cache_hits <= b.lp_solves - len(AC.LOCKSTEP)


@pytest.mark.parametrize("ring", [None, "0", "33", "1"])
def test_ring_variable_outside_its_range_is_the_default(torch_gpu, ring):
    """FJSP_ASYNC_RING unset, 0 or 33: the ring of 32, which the nine calls of this episode cannot fill -- no call waits.
    1: the call after the parking call finds its one batch in flight and waits."""
    a, b = _lockstep(torch_gpu, 7, ("lock3",), ring=ring)
    assert b.async_stats[0] == 1 and b.async_stats[3] == 7
    if ring == "1":
        assert b.async_stats[2] >= 1
    else:
        assert b.async_stats[2] == 0


def test_flush_right_after_parking(torch_gpu):
    """65 envs park in one call and fjsp_env_arrivals_flush runs at once: head copy, tail copy, LPs, upload and
    arrival_kernel all inside the flush.  Every env ready, none parked, the rows are the blocking batch's of that step,
    and the blocking step is accepted afterwards and agrees to the end of the episode."""
    torch = torch_gpu
    variant, N = AC.SO_FJSSP, 65
    s = AC.instance_set(("lock3",), variant)
    arr = s.arrays(0)
    T, park = AC.ops_total(arr), AC.ops_first(arr) - 1
    acts_h, acts = _lockstep_actions(torch, variant, T, N)
    a = _create(s, N, variant)
    want = _play_blocking(torch, a, acts, None, False, torch.full((N,), T, dtype=torch.int64, device="cuda"))
    b = _create(s, N, variant, lp_threads=1)

    def same(t, s_, r_, d_, what):
        assert torch.equal(s_.view(torch.int64), want["state"][t].view(torch.int64)), what + " state"
        assert torch.equal(r_.view(torch.int64), want["reward"][t].view(torch.int64)), what + " reward"
        assert torch.equal(d_, want["done"][t]), what + " done"
    for t in range(park):
        s_, r_, d_, ready = b.step_async(acts[t])
        assert bool((ready == 1).all())
        same(t, s_, r_, d_, "call %d" % t)
    s_, r_, d_, ready = b.step_async(acts[park])
    assert bool((ready == 0).all())
    same(park - 1, s_, r_, d_, "rows of parked envs are untouched:")
    s_, r_, d_, ready = b.flush_arrivals()
    assert bool((ready == 1).all()) and b.parked == 0
    same(park, s_, r_, d_, "after the flush")
    assert b.async_stats == (1, 1, 0, 65)
    for t in range(park + 1, T):
        s_, r_, d_ = b.step(acts[t])
        same(t, s_, r_, d_, "blocking step %d after the flush" % t)
    fa, fb = a.read(), b.read()
    for k in fa:
        assert k == "status" or torch.equal(fa[k], fb[k]), k
    assert int((fb["status"] != 0).sum()) == 0
    assert b.lp_solves == a.lp_solves == N


# --------------------------------------------------------------------------------------------- staggered: cases c, d

def _staggered(torch, chunks, variant, N, ring=None):
    """Two episodes + AC.EXTRA_STEPS applied steps per env with autoreset on the staggered instance of `chunks` chunks, a
    random rule pair per env per step: asynchronous against blocking (all of it) and against the oracle (first episode).
    Returns the asynchronous batch, what _play_async returned and the oracle's arrival step of every env."""
    name = AC.STAGGERED[chunks]
    s = AC.instance_set([name], variant)
    arr = s.arrays(0)
    acts_h = AC.staggered_actions(chunks, variant, N)
    acts = torch.from_numpy(acts_h).cuda()
    T = acts_h.shape[0]
    mo_rows = AC.mo_rows(variant, N)
    mo = None if mo_rows is None else torch.tensor(mo_rows, dtype=torch.float64).cuda()
    target = torch.full((N,), T, dtype=torch.int64, device="cuda")
    a = _create(s, N, variant)
    assert a.state_size == (30 if variant == AC.MO_DFJSP else 20)
    want = _play_blocking(torch, a, acts, mo, True, target)
    b = _create(s, N, variant, ring=ring)
    got = _play_async(torch, b, acts, mo, True, target, AC.RANDOM_PAIR[variant])
    what = "%s variant %d" % (name, variant)
    _assert_same_rows(torch, got, want, what)
    _assert_first_episode_matches_oracle(lambda e: arr, range(N), acts_h, mo_rows, variant, got, what)
    # the blocking twin played exactly two episodes and EXTRA_STEPS steps per env
    ops = AC.ops_total(arr)
    assert bool((want["done"][ops - 1] == 1).all()) and bool((want["done"][2 * ops - 1] == 1).all())
    assert int(want["done"].sum()) == 2 * N
    # every env parks where the oracle's LP hook was called (until then it took one step per call)
    arrive = np.array([AC.arrivals(arr, acts_h[:, e], AC.env_seed(e), variant, None if mo_rows is None else mo_rows[e])[1][0][0]
                       for e in range(N)])
    assert np.array_equal(got["first_park"], arrive)
    assert b.lp_solves >= 2 * N                          # one arrival per episode, two full episodes
    assert b.async_stats[0] >= max(3, len(set(arrive.tolist())))        # parking really was spread over calls
    return b, got, arrive


@pytest.mark.parametrize("chunks,variant,N", AC.STAGGERED_SETS)
def test_staggered_with_autoreset(torch_gpu, chunks, variant, N):
    """The 1-, 2- and 4-chunk builds of the step kernel's `ready` branches and of arrival_kernel under the asynchronous
    service, SO_FJSSP / SO_DFJSP / MO_DFJSP (per-env reward policies and normalisers), across two episode boundaries."""
    _staggered(torch_gpu, chunks, variant, N)


@pytest.mark.parametrize("variant", [AC.SO_FJSSP, AC.MO_DFJSP])
def test_ring_of_one(torch_gpu, variant):
    """A ring of one batch: the call after a parking call finds no free batch, waits for the LPs and resumes the parked
    envs itself (mark_resumed), then launches -- every parked env is back, untouched by that launch, one call later.
    Each launch that parked envs is followed by a call that waits, except possibly the run's last."""
    b, got, arrive = _staggered(torch_gpu, 1, variant, 40, ring="1")
    batches, _, waits, _ = b.async_stats
    assert waits >= batches - 1
    assert waits >= len(set(arrive.tolist())) >= 3       # the first episode alone: one wait per distinct arrival step
    assert np.array_equal(got["first_back"], arrive + 1)


@pytest.mark.parametrize("variant", [AC.SO_FJSSP, AC.MO_DFJSP])
def test_ring_of_two(torch_gpu, variant):
    _staggered(torch_gpu, 1, variant, 40, ring="2")


# --------------------------------------------------------------------------------------------- case f

def test_single_order_batch(torch_gpu):
    """A batch without order arrivals: step_async is the plain step, every env ready, and the service is never built."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    N, T = 10, 12
    s = H.gen_10x5(3, 1000)
    acts = torch.from_numpy(AC.actions(AC.SO_FJSSP, T, N, 9)).cuda()
    a, b = EnvBatch(s, N, rng_seed=3), EnvBatch(s, N, rng_seed=3)
    a.reset(); b.reset()
    for t in range(T):
        sa, ra, da = a.step(acts[t])
        sb, rb, db, ready = b.step_async(acts[t])
        assert bool((ready == 1).all())
        assert torch.equal(sa.view(torch.int64), sb.view(torch.int64)) and torch.equal(ra.view(torch.int64), rb.view(torch.int64))
        assert torch.equal(da, db)
    b.flush_arrivals()
    assert b.async_stats == (0, 0, 0, 0) and b.parked == 0 and b.lp_solves == 0
    fa, fb = a.read(), b.read()
    for k in fa:
        assert k == "status" or torch.equal(fa[k], fb[k]), k
