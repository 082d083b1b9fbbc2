"""Float64 reference of the PPO learning kernels (numpy, CPU).

Every function takes the kernels' exact f32 inputs (parameters, samples, hyperparameters as f32 values), computes the
same operation in float64 and returns, next to each result, an abs-magnitude `mag` of the same shape: the same sums and
products taken over |W|, |x|, |d out| and the float64 ReLU masks.  A kernel result is then checked componentwise as

    |got - ref| <= K * u * mag,      u = 2^-24,

where K is the depth of the quantity's accumulation chain in f32 (error of an n-term sum in any order: (n - 1) u
sum |term|; products of quantities with their own bounds add their K).  The K of each quantity is built from the
depth functions below; the tests state the depths of the kernels they run.

The bound holds only for samples that no f32 rounding can push to the other side of a branch (a ReLU pre-activation
within K u mag of 0, a probability ratio within its error of 1 +- eps, s1 ~ s2): `keep_samples` drops those and
reports how many.  Exact structural zeros (an all-zero row with zero biases, an advantage of 0) have mag 0 and are
kept: they are exact in both precisions.
"""
import numpy as np

U = 2.0 ** -24                 # unit roundoff of f32
TINY = 2.0 ** -102             # K * u * TINY = K * 2^-126: absolute floor for values that underflow (or flush) in f32


def f32(v):
    """A hyperparameter as the kernel sees it: the f32 value, widened."""
    return float(np.float32(v))


def as64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    assert a.dtype == np.float32, "the reference takes the kernels' exact f32 inputs"
    return a.astype(np.float64)


# ---------------------------------------------------------------------------------------------------------- network
def unflatten(flat, S, H, A):
    """The flat parameter buffer (W1[H][S] b1[H] W2[H][H] b2[H] W3[A][H] b3[A]) -> six f64 arrays."""
    flat = as64(flat).reshape(-1)
    shapes = [(H, S), (H,), (H, H), (H,), (A, H), (A,)]
    out, off = [], 0
    for shp in shapes:
        k = int(np.prod(shp))
        out.append(flat[off:off + k].reshape(shp))
        off += k
    assert off == flat.size
    return out


def forward_k(S, H):
    """K of the pre-activations z1, z2, z3: each an (inputs + 1)-term sum of products, on top of its inputs' K."""
    k1 = S + 2
    k2 = k1 + H + 2
    k3 = k2 + H + 2
    return k1, k2, k3


def forward(params, x):
    """Linear-ReLU-Linear-ReLU-Linear.  x: f32[n, S] -> dict of f64 pre-activations z1, z2, out, their abs-magnitudes
    m1, m2, m_out, the ReLU masks and each hidden pre-activation's distance from 0 relative to its magnitude."""
    W1, b1, W2, b2, W3, b3 = params
    x = as64(x)
    z1 = x @ W1.T + b1
    m1 = np.abs(x) @ np.abs(W1).T + np.abs(b1)
    k1 = z1 > 0
    h1 = np.where(k1, z1, 0.0)
    z2 = h1 @ W2.T + b2
    m2 = np.where(k1, m1, 0.0) @ np.abs(W2).T + np.abs(b2)
    k2 = z2 > 0
    h2 = np.where(k2, z2, 0.0)
    out = h2 @ W3.T + b3
    m_out = np.where(k2, m2, 0.0) @ np.abs(W3).T + np.abs(b3)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel1 = np.where(m1 > 0, np.abs(z1) / m1, np.inf)
        rel2 = np.where(m2 > 0, np.abs(z2) / m2, np.inf)
    return dict(x=x, z1=z1, m1=m1, k1=k1, h1=h1, z2=z2, m2=m2, k2=k2, h2=h2, out=out, m_out=m_out, rel1=rel1, rel2=rel2,
                ms=[m1, m2], rels=[rel1, rel2])


def forward_layers_k(dims):
    """forward_k for any depth: dims = [inputs, widths..., outputs] -> K of every layer's pre-activations,
    K_1 = dims[0] + 2, K_l = K_(l-1) + dims[l-1] + 2."""
    ks = [dims[0] + 2]
    for l in range(2, len(dims)):
        ks.append(ks[-1] + dims[l - 1] + 2)
    return ks


def forward_layers(params, x):
    """Linear-ReLU-...-Linear with 1..6 linear layers, params = [W1, b1, ..., WL, bL] (f64, torch layout [out][in]).
    x: f32[n, inputs] -> dict of the f64 logits `out`, their abs-magnitudes `m_out`, and per hidden layer its
    pre-activations `zs`, magnitudes `ms`, ReLU masks `masks` and distances from 0 relative to the magnitude `rels`."""
    assert len(params) % 2 == 0 and 1 <= len(params) // 2 <= 6
    h = as64(x)
    mh = np.abs(h)
    zs, ms, masks, rels = [], [], [], []
    n_layers = len(params) // 2
    for l in range(n_layers):
        W, b = params[2 * l], params[2 * l + 1]
        z = h @ W.T + b
        m = mh @ np.abs(W).T + np.abs(b)
        if l + 1 == n_layers:
            return dict(x=as64(x), out=z, m_out=m, zs=zs, ms=ms, masks=masks, rels=rels)
        k = z > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            rels.append(np.where(m > 0, np.abs(z) / m, np.inf))
        zs.append(z); ms.append(m); masks.append(k)
        h = np.where(k, z, 0.0)
        mh = np.where(k, m, 0.0)


def softmax(out):
    z = out - out.max(1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(1, keepdims=True)


# ---------------------------------------------------------------------------------------------------------- losses
def _log_softmax_parts(out, m_out, actions):
    n = out.shape[0]
    mx = out.max(1, keepdims=True)
    e = np.exp(out - mx)
    s = e.sum(1, keepdims=True)
    lse = (mx + np.log(s))[:, 0]
    p = e / s
    rows = np.arange(n)
    new_lp = out[rows, actions] - lse
    # magnitude of new_lp's error in units of the logits' K: the taken logit, the largest logit (the shift), |lse|
    L = m_out[rows, actions] + m_out.max(1) + np.abs(lse) + 1.0
    return p, new_lp, L


def surrogate(ratio, adv, eps):
    """Per-sample clipped surrogate min(adv ratio, adv clamp(ratio, 1 - eps, 1 + eps)) and its derivative g = d term /
    d ratio with autograd's conventions: minimum splits a tie in half, clamp passes the gradient on [1 - eps, 1 + eps]."""
    lo, hi = 1.0 - eps, 1.0 + eps
    clipped = np.clip(ratio, lo, hi)
    s1, s2 = adv * ratio, adv * clipped
    inside = ((ratio >= lo) & (ratio <= hi)).astype(np.float64)
    g = np.where(s1 < s2, adv, np.where(s2 < s1, adv * inside, 0.5 * adv + 0.5 * adv * inside))
    return np.minimum(s1, s2), g, s1, s2, clipped, lo, hi


def actor_loss(out, m_out, actions, old_log_prob, advantages, clip_eps, count):
    """MPPPO.actor_loss_terms, loss = -sum(terms) / count, and d loss / d logits under autograd's conventions
    (minimum splits a tie in half, clamp passes the gradient on the closed interval [1 - eps, 1 + eps]).
    The log-softmax is max-shifted.  Returns loss, dout and their magnitudes (K of both: K(out) + 8 + the depth of
    the loss sum) plus the per-sample ratio and the bounds of its rounding error relative to ratio (in units of K u)."""
    actions = np.asarray(actions).astype(np.int64)
    old = as64(old_log_prob)
    adv = as64(advantages)
    eps, count = f32(clip_eps), f32(count)
    n, A = out.shape
    p, new_lp, L = _log_softmax_parts(out, m_out, actions)
    ratio = np.exp(new_lp) / (np.exp(old) + f32(1e-8))
    terms, g, s1, s2, clipped, lo, hi = surrogate(ratio, adv, eps)
    loss = -terms.sum() / count
    onehot = np.zeros_like(out)
    onehot[np.arange(n), actions] = 1.0
    c = -g * ratio / count
    dout = c[:, None] * (onehot - p)
    # d_j = c (delta_j - p_j): c carries ratio's relative error (~ L), p_j carries (m_out_j + max m_out) + A
    # (+ TINY: exponentials, probabilities and their products that underflow in f32)
    gm = (np.abs(g) / count)[:, None]
    dout_mag = gm * ratio[:, None] * (np.abs(onehot - p) + p) * (L[:, None] + A + 4.0) + TINY
    loss_terms_mag = np.abs(adv) * np.maximum(ratio, clipped) * (L + 4.0) + TINY
    return dict(loss=loss, loss_mag=loss_terms_mag.sum() / count, dout=dout, dout_mag=dout_mag, ratio=ratio, ratio_L=L,
                s1=s1, s2=s2, lo=lo, hi=hi, new_lp=new_lp, probs=p)


def critic_loss(out, m_out, returns, count):
    """F.mse_loss as sum((v - G)^2) / count and d loss / d v.  K of dout: K(out) + 4; of the loss: K(out) + 4 + depth."""
    v = out[:, 0]
    ret = as64(returns)
    count = f32(count)
    d = v - ret
    dmag = m_out[:, 0] + np.abs(ret)
    dout = (2.0 * d / count)[:, None]
    dout_mag = (2.0 * dmag / count)[:, None]
    loss = (d * d).sum() / count
    loss_mag = (2.0 * np.abs(d) * dmag + d * d).sum() / count
    return dict(loss=loss, loss_mag=loss_mag, dout=dout, dout_mag=dout_mag)


# ---------------------------------------------------------------------------------------------------------- backward
def backward(params, fw, dout, dout_mag, k_dout, depth_w, depth_b):
    """All six parameter gradients of sum over samples, with their abs-magnitudes and K.
    depth_w / depth_b: depth of the kernel's sums over the samples for the weight / bias gradients."""
    W1, b1, W2, b2, W3, b3 = params
    H, A = W2.shape[0], W3.shape[0]
    k_h1, k_h2, _ = forward_k(W1.shape[1], H)
    x, h1, h2, k1, k2 = fw["x"], fw["h1"], fw["h2"], fw["k1"], fw["k2"]
    mh1, mh2 = np.where(k1, fw["m1"], 0.0), np.where(k2, fw["m2"], 0.0)
    gW3, gb3 = dout.T @ h2, dout.sum(0)
    mW3, mb3 = dout_mag.T @ mh2, dout_mag.sum(0)
    dz2 = np.where(k2, dout @ W3, 0.0)
    mz2 = np.where(k2, dout_mag @ np.abs(W3), 0.0)
    k_dz2 = k_dout + A + 1
    gW2, gb2 = dz2.T @ h1, dz2.sum(0)
    mW2, mb2 = mz2.T @ mh1, mz2.sum(0)
    dz1 = np.where(k1, dz2 @ W2, 0.0)
    mz1 = np.where(k1, mz2 @ np.abs(W2), 0.0)
    k_dz1 = k_dz2 + H + 1
    gW1, gb1 = dz1.T @ x, dz1.sum(0)
    mW1, mb1 = mz1.T @ np.abs(x), mz1.sum(0)
    grads = [gW1, gb1, gW2, gb2, gW3, gb3]
    mags = [mW1, mb1, mW2, mb2, mW3, mb3]
    ks = [k_dz1 + depth_w + 1, k_dz1 + depth_b, k_dz2 + k_h1 + depth_w + 1, k_dz2 + depth_b, k_dout + k_h2 + depth_w + 1, k_dout + depth_b]
    return grads, mags, ks


# ---------------------------------------------------------------------------------------------------------- sample filter
def keep_samples(fw, k1, k2=None, k_out=None, act=None, s_tol=64.0):
    """Boolean mask of the samples whose branches f32 rounding cannot flip, and the number dropped.
    Drops a sample when a hidden pre-activation lies within K u mag of 0 (mag > 0: exact structural zeros stay), or,
    with `act` (an actor_loss result), its ratio lies within its error of 1 - eps or 1 + eps, or s1 and s2 differ by
    less than their error without being equal.  fw: a forward() result with the K of its two hidden layers (k1, k2), or
    a forward_layers() result with k1 the list of K of its hidden layers (forward_layers_k(dims)[:-1])."""
    ks = list(k1) if k2 is None else [k1, k2]
    assert len(ks) == len(fw["rels"])
    keep = np.ones(fw["x"].shape[0], dtype=bool)
    for rel, m, k in zip(fw["rels"], fw["ms"], ks):
        keep &= ~((rel <= k * U) & (m > 0)).any(1)
    if act is not None:
        r, band = act["ratio"], (k_out + s_tol) * U * act["ratio_L"] * act["ratio"]
        keep &= np.abs(r - act["lo"]) > band
        keep &= np.abs(r - act["hi"]) > band
        s1, s2 = act["s1"], act["s2"]
        keep &= (s1 == s2) | (np.abs(s1 - s2) > (k_out + s_tol) * U * act["ratio_L"] * np.abs(s1))
    return keep, int((~keep).sum())


# ---------------------------------------------------------------------------------------------------------- optimiser
def clip_coef(grad, max_norm):
    """clip_grad_norm_'s coefficient: max_norm / (norm + 1e-6) clamped to 1; 1 when max_norm <= 0 (clip off)."""
    max_norm = f32(max_norm)
    if max_norm <= 0:
        return 1.0
    norm = np.sqrt((grad * grad).sum())
    return min(max_norm / (norm + f32(1e-6)), 1.0)


def adam_clip(params0, grads, lr, betas, eps, max_norm, sumsq_depth=None):
    """clip_grad_norm_ + torch.optim.Adam (no weight decay, no amsgrad) over a sequence of f32 gradients.
    Returns one dict per step: p, m, v, coef, and mags / K of p, m, v for the componentwise bound (sumsq_depth: depth
    of the kernel's sum of squares; None: no bounds)."""
    p = as64(params0).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    lr, b1, b2, eps = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps)
    states = []
    mag_m, mag_v, mag_p = np.zeros_like(p), np.zeros_like(p), np.abs(p).copy()
    k_p = 0.0
    for t, g in enumerate(grads, 1):
        g = as64(g)
        coef = clip_coef(g, max_norm)
        gc = g * coef
        m = b1 * m + (1.0 - b1) * gc
        v = b2 * v + (1.0 - b2) * gc * gc
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        upd = (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
        p = p - upd
        st = dict(p=p.copy(), m=m.copy(), v=v.copy(), coef=coef, step=t)
        if sumsq_depth is not None:
            # the coefficient: sum of squares (depth), sqrt, + 1e-6, divide; the moments add ~2-3 roundings per step
            k_coef = (sumsq_depth + 2) / 2.0 + 4.0 if (f32(max_norm) > 0 and coef < 1.0) else 1.0
            mag_m = b1 * mag_m + (1.0 - b1) * np.abs(gc)
            mag_v = b2 * mag_v + (1.0 - b2) * gc * gc
            k_m = k_coef + 2.0 * t + 4.0
            k_v = 2.0 * k_coef + 3.0 * t + 4.0
            # 1 - beta^t from powf (2 ulp of beta^t), relative to 1 - beta^t
            k_bc = 2.0 * b1 ** t / bc1 + 0.5 * 2.0 * b2 ** t / bc2
            k_upd = k_m + 0.5 * k_v + k_bc + 8.0
            mag_p = mag_p + np.abs(upd)
            k_p = max(k_p, k_upd + 1.0)
            st.update(mag_m=mag_m.copy(), mag_v=mag_v.copy(), k_m=k_m, k_v=k_v, mag_p=mag_p + np.abs(p), k_p=k_p)
        states.append(st)
    return states


# ---------------------------------------------------------------------------------------------------------- checking
def ratio_report(got, ref, mag, K):
    """(ok, message): |got - ref| <= K u mag everywhere; the message names the worst element and its err / (u mag)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    mag = np.broadcast_to(np.asarray(mag, dtype=np.float64), ref.shape)
    err = np.abs(got - ref)
    if not np.all(np.isfinite(got)):
        i = np.unravel_index(int(np.argmax(~np.isfinite(got))), got.shape) if got.ndim else ()
        return False, float("inf"), "non-finite value at %s" % (i,)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / (U * mag))
    worst = np.unravel_index(int(np.argmax(r)), r.shape) if r.ndim else ()
    rw = float(r[worst]) if r.ndim else float(r)
    msg = "worst element %s: got %.9g ref %.9g mag %.3g err/(u mag) %.4g (K %.4g)" % (
        worst, float(got[worst]), float(ref[worst]), float(mag[worst]), rw, K)
    return rw <= K, rw, msg
