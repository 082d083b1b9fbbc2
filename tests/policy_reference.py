"""Host restatements and float64 references of the policy-side kernels (numpy, CPU): the two action samplers and the
per-episode return normalisation.  Same conventions as tests/learning_reference.py (U, TINY, ratio_report).

Samplers.  Both kernels draw by inverse CDF from a counter-based splitmix64 stream; the restatements below repeat the
stream bit for bit (uint64 numpy) and the draw in exact f32 arithmetic (np.float32 element ops: one rounding each, no
fused multiply-add), so a kernel's actions must equal them exactly.

  sample_action (csrc/fjsp_policy.h: fjsp_policy_sample, the fused rollout, sampled decoding)
      r = mix64(seed ^ mix64(counter * 0x100000001B3 + env)),  u = (r >> 40) 2^-24,  v = ((r >> 16) & 0xFFFFFF) 2^-24
      total = p_0 + p_1 + ... (f32, in action order), target = u * total (f32); the first a whose f32 running sum
      exceeds target.  target < total for every u < 1 under round-to-nearest, and the running sum reaches total at the
      last action, so a draw always fires and never at an action whose p is 0 (the running sum does not move there).
      Then, if v <= epsilon, the action is mix64(r) % A.  v takes the value 0 (once in 2^24 draws), so the override also
      fires at epsilon = 0: this restates the reference's `random.random() <= epsilon`, and such a draw may be an action
      of probability 0.  log_prob = log(clamp(p_a / total, 2^-23, 1 - 2^-23)).
  the pair kernel (csrc/fjsp_policy_mlp.hip: fjsp_policy_pair_sample, softmax_sample)
      h = splitmix64(seed + row * 0x9E3779B97F4A7C15 + draw * 1000003),  u = (h >> 40) 2^-24; the first a with u < c_a,
      c the f32 running sum of the kernel's probabilities; when the final c is below 1 and u >= c, the last action with
      p > 0.

  cdf_interval_ok checks a draw against the f64 CDF without reading the kernel's probabilities: C_(a-1) <= u < C_a,
  each side widened by the summed error bound of the probabilities up to it plus (A + 2) u C for the running sum, and
  the action's f64 probability at least UNDERFLOW (below that its f32 probability is 0).

Log-probability of sample_action: p_a / total carries the relative error of an A-term sum of non-negative terms and
one division, A u; the clamp keeps it; logf adds at most 2 ulp of its result.  So |got - ref| <= K u mag with
mag = 1 + |ref|, K = A + 4.

Returns.  The discounted scan G_t = r_t + gamma G_(t+1) (two f32 roundings per step, valid rows only) is restated
bit for bit (returns_scan_f32).  The normalisation (MPPPO.normalise_returns: min-max to [0, 1], then (x - mean) /
(unbiased std + 1e-8)) is computed in f64 from the kernel's own f32 returns, per episode of n valid rows:

  min-max only     x = (G - min) / (max - min + 1e-8): a subtraction, a sum of two non-negative terms and a division,
                   K = 5 (4 roundings and a spare), mag = |x|.
  standardisation  with X = max |x| over the episode, K_x = 5 after min-max and 0 without it, sd = std + 1e-8:
                   x - mean is off by at most E = u X (2 K_x + n + 4) (x, the n-term sum, the subtraction); the sum of
                   squares then by 2 E sum |d| + n u sum d^2, which puts at most sqrt(2) E + (n / 2 + 2) u std on std;
                   the output y = (x - mean) / sd is off by u [(2 K_x + n + 4) (X / sd) (1 + sqrt(2) |y|) + (n / 2 + 4) |y|].
                   Hence mag = (X / sd) (1 + 1.5 |y|) + |y|, K = 2 K_x + 1.5 n + 12 (taken at n = T).
  neither          y = G exactly: K = 0.

These are first-order bounds: they need E / std small.  An episode whose std is within 64 E of 0 (with n >= 2 and
X > 0; one valid row is exact, the mean being the row, and so is an episode of zeros) is ill-conditioned -- a constant return without min-max, say, where the f32
mean differs from G by an ulp and the output is O(1) noise while the f64 answer is 0 -- and is flagged, reported and not
checked, as keep_samples does for ReLU edges.
"""
import numpy as np

from deep_reinforcement_learning_for_fjsp_amd.batch import _splitmix64 as mix64
from tests.learning_reference import TINY, U, as64, f32, ratio_report  # noqa: F401  (re-exported for the tests)

UNDERFLOW = 2.0 ** -150            # an f64 probability below half the smallest f32 subnormal is 0 in f32
EPS_CLAMP = 2.0 ** -23             # torch's clamp of a Categorical probability (f32 epsilon)
_M64 = (1 << 64) - 1


def _unit(bits24):
    """24 random bits as the kernels turn them into [0, 1): exact in f32."""
    return bits24.astype(np.float32) * np.float32(1.0 / 16777216.0)


# ---------------------------------------------------------------------------------------------------------- sample_action
def sample_action(p, epsilon, seed, counter, envs=None):
    """fjsp::sample_action for every row of p (f32[n, A], the kernel's input), env index = row (or `envs`).
    Returns dict(action, u, v, override, lp, lp_mag, K): lp the f64 log-probability of the action, lp_mag its mag."""
    p = np.asarray(p)
    assert p.dtype == np.float32 and p.ndim == 2
    n, A = p.shape
    env = np.arange(n, dtype=np.uint64) if envs is None else np.asarray(envs, dtype=np.uint64)
    with np.errstate(over="ignore"):
        inner = mix64(np.uint64(int(counter) & _M64) * np.uint64(0x100000001B3) + env)
        r = mix64(np.uint64(int(seed) & _M64) ^ inner)
    u = _unit(r >> np.uint64(40))
    v = _unit((r >> np.uint64(16)) & np.uint64(0xFFFFFF))
    total = np.zeros(n, dtype=np.float32)
    for a in range(A):
        total = total + p[:, a]
    target = u * total
    action = np.full(n, A - 1, dtype=np.int64)
    found = np.zeros(n, dtype=bool)
    acc = np.zeros(n, dtype=np.float32)
    for a in range(A):
        acc = acc + p[:, a]
        hit = ~found & (acc > target)
        action[hit] = a
        found |= hit
    override = v <= np.float32(epsilon)
    action = np.where(override, (mix64(r) % np.uint64(A)).astype(np.int64), action)
    p64 = p.astype(np.float64)
    pn = p64[np.arange(n), action] / p64.sum(1)
    lp = np.log(np.clip(pn, EPS_CLAMP, 1.0 - EPS_CLAMP))
    return dict(action=action, u=u.astype(np.float64), v=v.astype(np.float64), override=override, lp=lp,
                lp_mag=1.0 + np.abs(lp), K=A + 4.0, found=found)


def sample_action_p_bound(p):
    """The p_bound of cdf_interval_ok for sample_action: p normalised by the f64 sum, relative error (A + 2) u
    (the f32 total and target = u * total)."""
    p64 = np.asarray(p).astype(np.float64)
    p64 = p64 / p64.sum(1, keepdims=True)
    return p64, (p64.shape[1] + 2) * U * p64


# ---------------------------------------------------------------------------------------------------------- pair kernel
def pair_u(seed, rows, draws):
    """u of the pair kernel's stream for (row, draw) pairs (uint64 vector arithmetic)."""
    rows = np.asarray(rows, dtype=np.uint64)
    draws = np.asarray(draws, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & _M64) + rows * np.uint64(0x9E3779B97F4A7C15) + draws * np.uint64(1000003)
        return _unit(mix64(z) >> np.uint64(40))


def pair_draws(probs, seed, rows, draws):
    """fused_policy.expected_draw for every row of probs (f32[n, outputs] as the kernel returned them) at once.
    Returns (action, u, fell_through)."""
    probs = np.asarray(probs)
    assert probs.dtype == np.float32 and probs.ndim == 2
    n, no = probs.shape
    u = pair_u(seed, rows, np.broadcast_to(np.asarray(draws), (n,)))
    c = np.zeros(n, dtype=np.float32)
    action = np.full(n, -1, dtype=np.int64)
    last = np.full(n, no - 1, dtype=np.int64)
    for a in range(no):
        c = c + probs[:, a]
        hit = (action < 0) & (u < c)
        action[hit] = a
        last = np.where(probs[:, a] > 0, a, last)
    fell = action < 0
    action = np.where(fell, last, action)
    return action, u.astype(np.float64), fell


def pair_c_final(probs):
    """The f32 running sum of a row's probabilities after the last output, in the kernel's order."""
    probs = np.asarray(probs, dtype=np.float32)
    c = np.zeros(probs.shape[:-1], dtype=np.float32)
    for a in range(probs.shape[-1]):
        c = c + probs[..., a]
    return c


def seeds_with_u_at_least(c, row=0, draw=0, start=0, limit=1 << 27, chunk=1 << 22):
    """The first seed >= start whose pair-stream u for (row, draw) lies in [c, 1), or None below start + limit."""
    for s0 in range(start, start + limit, chunk):
        seeds = np.arange(s0, s0 + chunk, dtype=np.uint64)
        with np.errstate(over="ignore"):
            z = seeds + np.uint64(row) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(draw) * np.uint64(1000003)
            u = _unit(mix64(z) >> np.uint64(40))
        hit = np.nonzero(u >= np.float32(c))[0]
        if hit.size:
            return int(seeds[hit[0]])
    return None


# ---------------------------------------------------------------------------------------------------------- CDF check
def cdf_interval_ok(u, p64, p_bound, action):
    """Per row: does `action` hold u in the f64 CDF?  C_(a-1) - slack_(a-1) <= u < C_a + slack_a, with slack the summed
    p_bound up to the action plus (A + 2) u C (the running sum's roundings), and p64[action] >= UNDERFLOW."""
    p64 = np.asarray(p64, dtype=np.float64)
    n, A = p64.shape
    a = np.asarray(action, dtype=np.int64)
    rows = np.arange(n)
    C = np.cumsum(p64, 1)
    slack = np.cumsum(np.asarray(p_bound, dtype=np.float64), 1) + (A + 2) * U * C
    hi = C[rows, a] + slack[rows, a]
    prev = np.maximum(a - 1, 0)
    lo = np.where(a > 0, C[rows, prev] - slack[rows, prev], -np.inf)
    u = np.asarray(u, dtype=np.float64)
    return (u >= lo) & (u < hi) & (p64[rows, a] >= UNDERFLOW)


# ---------------------------------------------------------------------------------------------------------- returns
def returns_scan_f32(reward, valid, gamma):
    """The kernels' discounted scan, bit for bit: f32[T, N] rewards and validity flags, G_t = f32(r_t + f32(gamma G_(t+1)))
    walking back over the valid rows; 0 on the others."""
    reward = np.asarray(reward, dtype=np.float32)
    valid = np.asarray(valid, dtype=np.float32)
    g = np.zeros(reward.shape[1], dtype=np.float32)
    out = np.zeros_like(reward)
    gam = np.float32(gamma)
    for t in range(reward.shape[0] - 1, -1, -1):
        m = valid[t] != 0
        g = np.where(m, reward[t] + gam * g, g).astype(np.float32)
        out[t] = np.where(m, g, np.float32(0.0))
    return out


def normalise_returns(G, valid, normalized, standardized, eps=f32(1e-8)):
    """MPPPO.normalise_returns in f64 from the kernel's f32 returns G[T, N] (eps: the kernel's f32 1e-8; pass 1e-8 to
    compare with the torch f64 version).  Returns dict(out, mag, K, flagged[N]) -- see the module docstring."""
    G = as64(G)
    T, N = G.shape
    m = np.asarray(valid) != 0
    cnt = m.sum(0)
    x = G
    if normalized:
        gmin = np.where(m, G, np.inf).min(0)
        gmax = np.where(m, G, -np.inf).max(0)
        with np.errstate(invalid="ignore"):
            x = np.where(m, (G - gmin) / (gmax - gmin + eps), 0.0)
    x = np.where(m, x, 0.0)
    X = np.abs(x).max(0)
    kx = 5.0 if normalized else 0.0
    flagged = np.zeros(N, dtype=bool)
    if standardized:
        n = np.maximum(cnt, 1)
        mean = x.sum(0) / n
        d = np.where(m, x - mean, 0.0)
        std = np.sqrt((d * d).sum(0) / np.maximum(cnt - 1, 1))
        sd = std + eps
        y = d / sd
        mag = (X / sd) * (1.0 + 1.5 * np.abs(y)) + np.abs(y)
        K = 2.0 * kx + 1.5 * T + 12.0
        flagged = (cnt >= 2) & (X > 0) & (std <= 64.0 * (2.0 * kx + cnt + 4.0) * U * X)
    else:
        y = x
        mag = np.abs(x)
        K = kx
    return dict(out=np.where(m, y, 0.0), mag=np.where(m, mag, 0.0), K=K, flagged=flagged)
