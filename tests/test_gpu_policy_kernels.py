"""GPU: the policy-side kernels -- the ones every rollout, HMPSAC controller step and decode goes through -- against
host restatements and float64 references (tests/policy_reference.py, tests/learning_reference.py).

Checks are componentwise, |got - ref| <= K u mag (u = 2^-24), or bit-exact where the kernel's arithmetic is restated:

  policy_pair_kernel (fjsp_policy_pair_sample through fused_policy.PolicyPairSampler, task and task + machine)
    shapes    1, 2, 3, 6 linear layers; hidden widths 1, 3, 4, 5 (the 4-wide inner loop's remainders), 255, 256 (every
              thread of the block); outputs 1, 2, 10, 12, 63, 64; S = 1, 30, 255 (machine input 256); rows 1, 15, 16,
              17, 4097 (16 rows per workgroup, the tail clamped); one net whose logits spread by more than 120 (some
              f32 probabilities exactly 0).
    probs     against softmax(forward_layers) in f64 on the rows keep_samples keeps (the machine network's reference
              input uses the kernel's own a_t): mag_j = p_j (m_out_j + max m_out + 1) + TINY, K = K_L + 8,
              K_L = forward_layers_k(dims)[-1].
    draws     every draw equals the fixed expected_draw (vector form pair_draws) on the kernel's probabilities, lies in
              its f64 CDF interval (cdf_interval_ok, p_bound = K u mag) and never has a kernel probability of 0; draw
              counters advance by 2 per task + machine call, by 1 per task-only call.
    fall-through  exact logits whose f32 probabilities sum below 1 and a seed whose u lies in [c_final, 1): the draw is
              the last action with p > 0 (before the fix: the last action, of probability 0).
    refusals  7 layers, width 257, 65 outputs, an input width that does not match the state, a 256-wide state: refused
              before any launch, by supported() / PolicyPairSampler and by the C ABI alike.
  fjsp::sample_action (fjsp_policy_sample through the C ABI)
    shapes    A in {1, 2, 5, 30, 32, 33, 64, 255, 256} x N in {1, 255, 256, 257, 8193} x eps in {0, 0.3, 1} x
              pair_div in {0, 1, 5, A}; rows: random, one-hot first / middle / last, leading and trailing zeros,
              totals 1e-3 and 7, uniform, an exact zero in the middle.
    checks    action and pair encoding bit-equal to the host restatement; log-prob within K = A + 4, mag = 1 + |lp| of
              log(clamp(p_a / sum p)) in f64; at eps = 0 (but for the documented v == 0 override) the draw lies in its
              f64 CDF interval and never has p = 0.  A = 0 and A = 257 are FJSP_E_ARG.
  greedy branch of fjsp_env_play_policy
    an actor with three identical output rows (exact ties that dominate): play(greedy=True) takes the lowest tied index
    at every step, equal to the per-step loop (torch.argmax of fjsp_actor_forward), on a pair-action and a flat-action env.
  returns_normalise_regs_kernel (T <= 64) / returns_normalise_kernel (T > 64) through RolloutBuffer
    shapes    T in {1, 2, 63, 64, 65, 130} x N in {1, 63, 64, 65, 4097} x gamma in {0, 0.5, 0.99, 1} x the four
              (normalized, standardized) combinations; episodes with no valid row, one valid row, a valid prefix, holes;
              rewards env-like integers in [-300, 0], magnitudes of 1e6, constants.
    checks    the raw scan bit-equal to the f32 restatement; invalid rows exactly 0; no NaN / inf; normalised outputs
              within the f64 bound of policy_reference.normalise_returns (min-max: K = 5, mag = |x|; standardised:
              K = 2 K_x + 1.5 T + 12, mag = (X / sd)(1 + 1.5 |y|) + |y|; neither: exact) on the episodes it does not flag
              as ill-conditioned (how many it flags is printed); a T = 65 buffer whose last row is invalid everywhere
              gives outputs bit-identical to the same T = 64 buffer (memory walk against register kernel).

Largest err / (u mag) observed on the MI355X, per kernel, is printed at the end of the module (run with -s) and quoted
in each test's docstring: policy_pair probs 4.38, policy_sample log_prob 20.4, returns_normalise_regs 3.85,
returns_normalise 6.51.
"""
import ctypes as C
import json

import numpy as np
import pytest

from tests import learning_reference as R
from tests import policy_reference as P

pytestmark = pytest.mark.gpu

OBSERVED = {}          # kernel -> largest err / (u mag)
DROPPED = {}           # configuration -> rows the ReLU filter dropped
FLAGGED = {}           # configuration -> ill-conditioned episodes not checked

E_ARG, E_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    yield torch
    print("\npolicy kernels, largest err/(u mag): " + json.dumps({k: round(v, 3) for k, v in sorted(OBSERVED.items())}))
    print("policy kernels, rows dropped by the ReLU filter: " + json.dumps(DROPPED))
    print("policy kernels, ill-conditioned episodes flagged: " + json.dumps(FLAGGED))


def _check(kernel, what, got, ref, mag, K):
    ok, r, msg = R.ratio_report(got, ref, mag, K)
    OBSERVED[kernel] = max(OBSERVED.get(kernel, 0.0), r)
    assert ok, "%s, %s: %s" % (kernel, what, msg)


def _host(t):
    return t.detach().cpu().numpy()


# ================================================================================================ pair kernel
def _stack(torch, dims, seed, spread=False):
    """Linear-ReLU-...-Linear on cuda:0, weights ~ N(0, 1/fan_in), biases ~ N(0, 0.01); spread: the last layer's biases
    run from 0 down to -150, so the logits spread by more than 120 and some f32 probabilities are exactly 0."""
    nn = torch.nn
    g = torch.Generator().manual_seed(seed)
    mods = []
    for i in range(len(dims) - 1):
        l = nn.Linear(dims[i], dims[i + 1])
        with torch.no_grad():
            l.weight.copy_(torch.randn(l.weight.shape, generator=g) / np.sqrt(dims[i]))
            l.bias.copy_(torch.randn(l.bias.shape, generator=g) * 0.1)
        mods += [l, nn.ReLU()]
    last = mods[-2]
    if spread:
        with torch.no_grad():
            last.bias.copy_(torch.linspace(0.0, -150.0, dims[-1]))
    return nn.Sequential(*mods[:-1]).to("cuda:0")


def _params(net):
    import torch
    return [R.as64(t) for m in net if isinstance(m, torch.nn.Linear) for t in (m.weight, m.bias)]


def _dims(net):
    import torch
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    return [lin[0].in_features] + [m.out_features for m in lin]


def _check_network(tag, net, x, probs_k, actions, seed, rows, draw):
    """One network's kernel probabilities (f32[n, outputs]) and draws against the f64 reference and the restated stream."""
    dims = _dims(net)
    ks = R.forward_layers_k(dims)
    fw = R.forward_layers(_params(net), x)
    keep, DROPPED[tag] = R.keep_samples(fw, ks[:-1])
    assert keep.any(), tag + ": the ReLU filter dropped every row"
    p = R.softmax(fw["out"])
    mag = p * (fw["m_out"] + fw["m_out"].max(1, keepdims=True) + 1.0) + R.TINY
    K = ks[-1] + 8
    _check("policy_pair probs", tag, probs_k[keep], p[keep], mag[keep], K)
    want, u, _ = P.pair_draws(probs_k, seed, rows, draw)
    np.testing.assert_array_equal(actions, want, err_msg=tag + ": draws against the restated stream")
    from deep_reinforcement_learning_for_fjsp_amd.agents import fused_policy
    for r in sorted({0, len(rows) - 1, len(rows) // 2}):
        assert actions[r] == fused_policy.expected_draw(probs_k[r], seed, rows[r], draw), (tag, r)
    n = len(rows)
    assert np.all(probs_k[np.arange(n), actions] > 0), tag + ": a draw of probability 0"
    ok = P.cdf_interval_ok(u[keep], p[keep], K * R.U * mag[keep], actions[keep])
    assert ok.all(), "%s: draw outside its f64 CDF interval at rows %s" % (tag, np.nonzero(~ok)[0][:8])
    return p


# (S, task hidden widths, task outputs, machine hidden widths, machine outputs, rows, spread)
PAIR_CASES = [
    (1, [], 1, [], 2, 1, False),
    (30, [1], 2, [3], 10, 15, False),
    (30, [4, 5], 12, [5, 3], 63, 16, False),
    (255, [255, 256, 3, 4, 5], 64, [256, 3, 4, 5, 256], 12, 17, False),
    (30, [256, 256], 10, [255, 255], 64, 4097, False),
    (1, [5, 5, 5, 5, 5], 63, [1, 4], 1, 4097, False),
    (30, [64], 12, [64, 64], 64, 4097, True),
]


@pytest.mark.parametrize("case", range(len(PAIR_CASES)))
def test_policy_pair_kernel_matches_f64_reference(torch_gpu, case):
    """Probabilities componentwise against f64 (K = K_L + 8), draws bit-equal to the fixed restatement, inside their f64
    CDF interval and never of probability 0, draw counters +2 (task + machine) and +1 (task only) per call.
    Largest err/(u mag) observed on the MI355X: 4.38 (K = K_L + 8 >= 11)."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.agents import fused_policy
    S, th, to, mh, mo, rows, spread = PAIR_CASES[case]
    task = _stack(torch, [S] + th + [to], 100 + case, spread)
    machine = _stack(torch, [S + 1] + mh + [mo], 200 + case, spread)
    assert fused_policy.supported(task, "cuda:0") and fused_policy.supported(machine, "cuda:0")
    rs = np.random.RandomState(case)
    state = rs.randn(rows, S) * 10.0 ** rs.uniform(-1, 1, (rows, 1))
    st = torch.from_numpy(state).to("cuda:0").contiguous()
    x = state.astype(np.float32)
    idx = np.arange(rows)
    seed = 0x5EED0000 + case
    sm = fused_policy.PolicyPairSampler(task, machine, seed=seed)
    for call in range(2):
        a_t, a_m, p_t, p_m = sm.sample(st, probs=True)
        torch.cuda.synchronize()
        at, am, pt, pm = _host(a_t), _host(a_m), _host(p_t), _host(p_m)
        tag = "case %d call %d" % (case, call)
        p64 = _check_network(tag + " task", task, x, pt, at, seed, idx, 2 * call)
        xm = np.concatenate([x, at.astype(np.float32)[:, None]], 1)
        _check_network(tag + " machine", machine, xm, pm, am, seed, idx, 2 * call + 1)
        assert np.all(_host(sm.draws(rows)) == 2 * (call + 1))
        if spread:
            assert (pt == 0).any() and (pm == 0).any(), "the spread case must have f32 probabilities of exactly 0"
            assert float(np.ptp(np.log(np.maximum(p64, 1e-300)), 1).min()) > 120.0
    solo = fused_policy.PolicyPairSampler(task, None, seed=seed + 1)
    for call in range(2):
        a_t, none, p_t, _ = solo.sample(st, probs=True)
        torch.cuda.synchronize()
        assert none is None
        _check_network("case %d task-only call %d" % (case, call), task, x, _host(p_t), _host(a_t), seed + 1, idx, call)
        assert np.all(_host(solo.draws(rows)) == call + 1)


def _one_layer(torch, W, b):
    lin = torch.nn.Linear(W.shape[1], W.shape[0])
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(W))
        lin.bias.copy_(torch.from_numpy(b))
    return torch.nn.Sequential(lin).to("cuda:0")


def _fall_through(torch, net, state, what):
    """Row 0, draw 0 of a seed whose u lies in [c_final, 1): the draw is the last action with p > 0."""
    from deep_reinforcement_learning_for_fjsp_amd.agents import fused_policy
    st = torch.from_numpy(state).to("cuda:0").contiguous()
    _, _, p, _ = fused_policy.PolicyPairSampler(net, None, seed=0).sample(st, probs=True)
    p = _host(p)[0]
    c = P.pair_c_final(p)
    assert c < 1.0, "%s: the f32 probabilities sum to 1 on this device" % what
    seed = P.seeds_with_u_at_least(c)
    assert seed is not None
    assert P.pair_u(seed, [0], [0])[0] >= c
    a, _, q, _ = fused_policy.PolicyPairSampler(net, None, seed=seed).sample(st, probs=True)
    torch.cuda.synchronize()
    assert np.array_equal(_host(q)[0], p)
    last = int(np.nonzero(p > 0)[0][-1])
    assert last < p.size - 1 and p[-1] == 0.0
    assert int(_host(a)[0]) == last, "%s: u = %r >= c_final = %r drew %d, the last action with p > 0 is %d" % (
        what, float(P.pair_u(seed, [0], [0])[0]), float(c), int(_host(a)[0]), last)


def test_policy_pair_draw_falls_through_to_the_last_non_zero_probability(torch_gpu):
    """Exact logits (one linear layer, W = 0, b = the logits; or W = the candidates' logits against one-hot states, b = 0:
    fma chains of 0 * w and 1 * w are exact).  64 outputs, 62 logits at 0 and 2 at -200: c_final = 1 - 12 2^-24; the
    HMPSAC task-head width of 12 with its last two logits at -200 and ten random ones, of which the first whose device
    probabilities sum below 1 is kept.  With u in [c_final, 1) the kernel must draw the last action with p > 0 -- the
    kernel before the fix drew the last action, of probability 0."""
    torch = torch_gpu
    b = np.array([0.0] * 62 + [-200.0, -200.0], dtype=np.float32)
    _fall_through(torch, _one_layer(torch, np.zeros((64, 1), np.float32), b), np.zeros((1, 1)), "64 outputs")
    rs = np.random.RandomState(12)
    n = 64
    logits = np.concatenate([rs.randn(n, 10) * 2.0, np.full((n, 2), -200.0)], 1).astype(np.float32)
    net = _one_layer(torch, np.ascontiguousarray(logits.T), np.zeros(12, np.float32))
    from deep_reinforcement_learning_for_fjsp_amd.agents import fused_policy
    _, _, p, _ = fused_policy.PolicyPairSampler(net, None).sample(torch.eye(n, dtype=torch.float64, device="cuda:0"), probs=True)
    c = P.pair_c_final(_host(p))
    below = np.nonzero(c < 1.0)[0]
    assert below.size > 0, "none of %d candidates sums below 1" % n
    FLAGGED["fall-through candidates summing below 1"] = "%d of %d" % (below.size, n)
    _fall_through(torch, net, np.eye(n)[below[:1]], "12 outputs, candidate %d" % below[0])


def _abi_pair(torch, task_dims, machine_dims, S, rows=4):
    """fjsp_policy_pair_sample called directly with real parameter tensors of the given shapes; returns its code and
    whether the draw counters moved."""
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    keep = []

    def arrays(dims):
        if not dims:
            return 0, None, None, None
        n = len(dims) - 1
        w, b = (C.c_void_p * n)(), (C.c_void_p * n)()
        for l in range(n):
            wt = torch.zeros(dims[l], dims[l + 1], device="cuda:0")
            bt = torch.zeros(dims[l + 1], device="cuda:0")
            keep.extend([wt, bt])
            w[l], b[l] = wt.data_ptr(), bt.data_ptr()
        d = np.array(dims, dtype=np.int32)
        keep.extend([d, w, b])
        return n, d.ctypes.data, C.addressof(w), C.addressof(b)
    tn, td, tw, tb = arrays(task_dims)
    mn, md, mw, mb = arrays(machine_dims)
    state = torch.zeros(rows, max(S, 1), dtype=torch.float64, device="cuda:0")
    draws = torch.zeros(rows, dtype=torch.int32, device="cuda:0")
    a_t = torch.zeros(rows, dtype=torch.int64, device="cuda:0")
    a_m = torch.zeros(rows, dtype=torch.int64, device="cuda:0")
    rc = _capi.lib().fjsp_policy_pair_sample(tn, td, tw, tb, mn, md, mw, mb, state.data_ptr(), rows, S, 1, draws.data_ptr(),
                                            a_t.data_ptr(), a_m.data_ptr(), None, None, None, None, 0,
                                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, bool((draws != 0).any())


def test_policy_pair_refusals_agree_with_the_c_abi(torch_gpu):
    """What supported() / PolicyPairSampler refuse, the C ABI refuses too, before any launch (draw counters untouched):
    7 layers, a width of 257, 65 outputs, an input width that does not match the state, a 256-wide state.  The largest
    accepted shapes run."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.agents import fused_policy
    refused = [  # (task dims, machine dims, S, C ABI code, supported(task), supported(machine))
        ([10] + [8] * 6 + [4], None, 10, E_ARG, False, None),
        ([10, 257, 4], None, 10, E_UNSUPPORTED, False, None),
        ([10, 8, 65], None, 10, E_UNSUPPORTED, False, None),
        ([10, 8, 4], [11, 8, 65], 10, E_UNSUPPORTED, True, False),
        ([11, 8, 4], None, 10, E_ARG, True, None),                       # refused by sample(): the state is 10 wide
        ([10, 8, 4], [10, 8, 4], 10, E_ARG, True, True),                 # the machine network must take S + 1
        ([256, 8, 4], None, 256, E_ARG, True, None),                     # a fitting stack, but the state is too wide
    ]
    for td, md, S, code, sup_t, sup_m in refused:
        rc, moved = _abi_pair(torch, td, md, S)
        assert rc == code and not moved, (td, md, S, rc)
        task = _stack(torch, td, 1)
        machine = _stack(torch, md, 2) if md else None
        assert fused_policy.supported(task) == sup_t and (md is None or fused_policy.supported(machine) == sup_m), (td, md)
        with pytest.raises(ValueError):
            sm = fused_policy.PolicyPairSampler(task, machine)
            sm.sample(torch.zeros(4, S, dtype=torch.float64, device="cuda:0"))
    for td, md, S in (([255] + [256] * 5 + [64], [256] * 6 + [64], 255), ([1, 1], None, 1)):
        rc, moved = _abi_pair(torch, td, md, S, rows=17)
        assert rc == 0 and moved


# ================================================================================================ sample_action
def _rows(rs, N, A):
    """Probability rows by pattern (row index mod 12): random at three sharpnesses, one-hot first / middle / last,
    leading zeros, trailing zeros, total 1e-3, total 7, uniform, an exact zero in the middle."""
    p = np.exp(rs.randn(N, A) * rs.choice([0.3, 1.5, 5.0], (N, 1)))
    p /= p.sum(1, keepdims=True)
    kind = np.arange(N) % 12
    for k, col in ((3, 0), (4, A // 2), (5, A - 1)):
        p[kind == k] = 0.0
        p[kind == k, col] = 1.0
    if A >= 2:
        p[kind == 6, : A // 2] = 0.0
        p[kind == 7, A - A // 2:] = 0.0
    p[kind == 8] *= 1e-3
    p[kind == 9] *= 7.0
    p[kind == 10] = 1.0 / A
    if A >= 3:
        p[kind == 11, A // 2] = 0.0
    return p.astype(np.float32)


@pytest.mark.parametrize("A", [1, 2, 5, 30, 32, 33, 64, 255, 256])
def test_policy_sample_kernel_matches_host_restatement(torch_gpu, A):
    """fjsp_policy_sample: actions and pair encodings bit-equal to policy_reference.sample_action for every N, epsilon
    and pair_div; log-probabilities within K = A + 4, mag = 1 + |lp| of the f64 log(clamp(p_a / sum p)); at epsilon 0
    every draw but the v == 0 overrides lies in its f64 CDF interval and has p > 0.
    Largest err/(u mag) observed on the MI355X: 20.4 (A = 256: K = 260)."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    lib = _capi.lib()
    rs = np.random.RandomState(A)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    seed_v = 0x0123456789ABCDEF ^ A
    seed = torch.tensor([int(np.array(seed_v, dtype=np.uint64).view(np.int64))], dtype=torch.int64, device="cuda:0")
    counter = 0
    for N in (1, 255, 256, 257, 8193):
        p = _rows(rs, N, A)
        pd = torch.from_numpy(p).to("cuda:0")
        p64, pb = P.sample_action_p_bound(p)
        for eps in (0.0, 0.3, 1.0):
            e = torch.tensor([eps], dtype=torch.float32, device="cuda:0")
            for div in sorted({0, 1, 5, A}):
                counter += 1
                pair = torch.full((N, 2), 255, dtype=torch.uint8, device="cuda:0")
                act = torch.full((N,), -1.0, device="cuda:0")
                lp = torch.full((N,), np.nan, device="cuda:0")
                _capi.check(lib.fjsp_policy_sample(ptr(pd), N, A, div, ptr(e), ptr(seed), counter, ptr(pair), ptr(act), ptr(lp),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
                torch.cuda.synchronize()
                tag = "A=%d N=%d eps=%g div=%d" % (A, N, eps, div)
                ref = P.sample_action(p, eps, seed_v, counter)
                got = _host(act)
                assert np.array_equal(got, ref["action"].astype(np.float32)), tag
                a = ref["action"]
                want_pair = np.stack([a // div, a % div], 1) if div > 0 else np.stack([a, np.zeros_like(a)], 1)
                assert np.array_equal(_host(pair), want_pair.astype(np.uint8)), tag
                _check("policy_sample log_prob", tag, _host(lp), ref["lp"], ref["lp_mag"], ref["K"])
                if eps == 1.0:
                    assert ref["override"].all()
                if eps == 0.0:
                    drawn = ~ref["override"]
                    assert np.all(p[np.arange(N), a][drawn] > 0), tag
                    assert P.cdf_interval_ok(ref["u"], p64, pb, a)[drawn].all(), tag
    for bad in (0, 257):
        one = torch.zeros(4, 1, device="cuda:0")
        pair = torch.zeros(4, 2, dtype=torch.uint8, device="cuda:0")
        out = torch.zeros(4, device="cuda:0")
        e = torch.zeros(1, device="cuda:0")
        rc = lib.fjsp_policy_sample(ptr(one), 4, bad, 0, ptr(e), ptr(seed), 0, ptr(pair), ptr(out), ptr(out),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == E_ARG, bad


# ================================================================================================ greedy ties
@pytest.fixture
def kernel_only(monkeypatch):
    """The kernel path must run: the per-step loop raises if play falls back to it."""
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    loop = PS._play_loop

    def boom(*a, **k):
        raise AssertionError("play fell back to the per-step loop")

    def on(flag):
        monkeypatch.setattr(PS, "_play_loop", boom if flag else loop)
    return on


def _tied_actor(torch, S, A, tied):
    """An ActorNet whose output rows `tied` are copies of the first of them with a bias raised by 30: their
    probabilities tie exactly and are the largest at every state."""
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.MPPPO import ActorNet
    torch.manual_seed(S + A)
    actor = ActorNet(S, 128, 2, A).cuda()
    last = [m for m in actor.layers if isinstance(m, torch.nn.Linear)][-1]
    with torch.no_grad():
        last.bias[tied[0]] += 30.0
        for j in tied[1:]:
            last.weight[j] = last.weight[tied[0]]
            last.bias[j] = last.bias[tied[0]]
    return actor


@pytest.mark.parametrize("suite", ["so_fjssp", "so_sfjsp"])
def test_greedy_decode_takes_the_first_of_tied_probabilities(torch_gpu, kernel_only, suite):
    """fjsp_env_play_policy's greedy branch on exact ties: every step applies the lowest tied index (torch.argmax),
    kernel == per-step loop, on a pair-action env (SO_FJSSP, 30 actions) and a flat-action env (SO_SFJSP, 20)."""
    torch = torch_gpu
    from tests import helpers as H
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, VARIANT_SO_SFJSP
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.MPPPO import native_actor_forward
    if suite == "so_fjssp":
        s, N, S, A, div, tied = H.gen_10x5(16, 320), 256, 20, 30, 5, [7, 13, 22]
        make = lambda: EnvBatch(s, N, rng_seed=9)
    else:
        insts, _, _ = H.load_suite("so_sfjsp")
        insts = [a for a in insts if a.S == 1 and a.K <= 64]
        s, N, S, A, div, tied = H.instance_set_from(insts), 8 * len(insts), 18, 20, 0, [3, 4, 17]
        make = lambda: EnvBatch(s, N, variant=VARIANT_SO_SFJSP, rng_seed=9)
    actor = _tied_actor(torch, S, A, tied)
    states = torch.randn(512, S, dtype=torch.float64, device="cuda:0") * 3.0
    probs = native_actor_forward(actor, states)
    torch.cuda.synchronize()
    pr = _host(probs)
    assert np.array_equal(pr[:, tied[0]], pr[:, tied[1]]) and np.array_equal(pr[:, tied[0]], pr[:, tied[2]])
    assert np.all(_host(torch.argmax(probs, 1)) == tied[0])
    got = H.kernel_vs_loop(make, actor, kernel_only)
    acts, steps = got["actions"], got["steps"]
    want = (tied[0] // div, tied[0] % div) if div else (tied[0], 0)
    T = acts.shape[0]
    live = np.arange(T)[:, None] < steps[None, :]
    assert live.any()
    assert np.all(acts[..., 0][live] == want[0]) and np.all(acts[..., 1][live] == want[1])


# ================================================================================================ returns
def _buffer(torch, T, N):
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO.Buffer import RolloutBuffer
    buf = RolloutBuffer(T, N, 1)
    z = torch.zeros(N, 1, dtype=torch.float64, device="cuda:0")
    a = torch.zeros(N, 2, dtype=torch.uint8, device="cuda:0")
    done = torch.zeros(N, dtype=torch.uint8, device="cuda:0")
    r = torch.zeros(N, dtype=torch.float64, device="cuda:0")
    for _ in range(T):
        buf.add_experience(z, a, r, z, done)
    return buf


def _episodes(rs, T, N):
    """valid and reward [T, N] f32: per env one of no valid row / one valid row / a valid prefix / holes, and rewards
    env-like integers in [-300, 0] / magnitudes of 1e6 / a constant."""
    valid = np.zeros((T, N), np.float32)
    reward = np.zeros((T, N), np.float32)
    for j in range(N):
        kind = (j + T) % 4
        if kind == 1:
            valid[rs.randint(T), j] = 1.0
        elif kind == 2:
            valid[: rs.randint(1, T + 1), j] = 1.0
        elif kind == 3:
            valid[:, j] = rs.rand(T) < 0.6
        rk = (j // 4 + T) % 3
        if rk == 0:
            reward[:, j] = -rs.randint(0, 301, T)
        elif rk == 1:
            reward[:, j] = rs.randn(T) * 1e6
        else:
            reward[:, j] = -float(rs.randint(0, 301))
    return reward, valid


def _run_returns(torch, buf, reward, valid, gamma, nz, st):
    T = reward.shape[0]
    buf.rewards[:T].copy_(torch.from_numpy(reward))
    buf.valid[:T].copy_(torch.from_numpy(valid))
    out = _host(buf.normalised_returns(gamma, nz, st)).copy()
    raw = _host(buf.returns[:T]).copy()
    return raw, out


@pytest.mark.parametrize("N", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 130])
def test_returns_and_normalisation_match_f64_reference(torch_gpu, T, N):
    """Raw scan bit-equal to the f32 restatement (both kernels' scans and fjsp_rollout_returns), invalid rows exactly 0,
    no NaN / inf, normalised outputs within the f64 bound on the episodes not flagged as ill-conditioned.
    Largest err/(u mag) observed on the MI355X: 3.85 (register kernel), 6.51 (memory walk)."""
    torch = torch_gpu
    rs = np.random.RandomState(T * 1000 + N)
    reward, valid = _episodes(rs, T, N)
    buf = _buffer(torch, T, N)
    kernel = "returns_normalise_regs" if T <= 64 else "returns_normalise"
    inv = valid == 0
    for gamma in (0.0, 0.5, 0.99, 1.0):
        G = P.returns_scan_f32(reward, valid, gamma)
        for nz in (True, False):
            for st in (True, False):
                tag = "T=%d N=%d gamma=%g normalized=%s standardized=%s" % (T, N, gamma, nz, st)
                raw, out = _run_returns(torch, buf, reward, valid, gamma, nz, st)
                assert np.array_equal(raw.view(np.uint32), G.view(np.uint32)), tag + ": raw scan"
                assert np.all(np.isfinite(out)), tag
                assert np.all(out[inv] == 0.0) and np.all(raw[inv] == 0.0), tag
                ref = P.normalise_returns(G, valid, nz, st)
                ok = ~ref["flagged"]
                if ref["flagged"].any():
                    FLAGGED[tag] = int(ref["flagged"].sum())
                _check(kernel, tag, out[:, ok], ref["out"][:, ok], ref["mag"][:, ok], ref["K"])
        scan = _host(buf.compute_returns(gamma))
        assert np.array_equal(scan.view(np.uint32), G.view(np.uint32)), "fjsp_rollout_returns T=%d N=%d gamma=%g" % (T, N, gamma)


@pytest.mark.parametrize("N", [65, 4097])
def test_returns_kernels_agree_across_the_switch(torch_gpu, N):
    """A T = 65 buffer (memory walk) whose last row is invalid for every env gives the raw and normalised returns of the
    same T = 64 buffer (register kernel) bit for bit, and 0 on the last row."""
    torch = torch_gpu
    rs = np.random.RandomState(N)
    reward, valid = _episodes(rs, 64, N)
    r65 = np.concatenate([reward, rs.randn(1, N).astype(np.float32) * 100], 0)
    v65 = np.concatenate([valid, np.zeros((1, N), np.float32)], 0)
    b64, b65 = _buffer(torch, 64, N), _buffer(torch, 65, N)
    for gamma in (0.0, 0.99, 1.0):
        for nz in (True, False):
            for st in (True, False):
                raw64, out64 = _run_returns(torch, b64, reward, valid, gamma, nz, st)
                raw65, out65 = _run_returns(torch, b65, r65, v65, gamma, nz, st)
                tag = "N=%d gamma=%g normalized=%s standardized=%s" % (N, gamma, nz, st)
                assert np.array_equal(raw65[:64].view(np.uint32), raw64.view(np.uint32)), tag
                assert np.array_equal(out65[:64].view(np.uint32), out64.view(np.uint32)), tag
                assert np.all(out65[64] == 0.0) and np.all(raw65[64] == 0.0), tag
