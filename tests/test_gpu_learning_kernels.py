"""GPU: the PPO learning kernels against the float64 reference (tests/learning_reference.py).

Every check is componentwise, |got - ref| <= K u mag (u = 2^-24), on the whole tensor and on the loss; `mag` is the
reference's abs-magnitude of the quantity and K the depth of its f32 accumulation chain in the kernel under test:

    forward pre-activations   K1 = S + 2, K2 = K1 + H + 2, K3 = K2 + H + 2            (sums of S + 1 / H + 1 terms)
    d loss / d out            K3 + 8 (actor: ratio and softmax roundings), K3 + 4 (critic)
    dH2 / dH1                 + A + 1 / + H + 1
    weight / bias gradients   K(d pre-activation) [+ K(activation)] + depth of the sum over the samples:
      MFMA pass               32 * ceil(tiles / G) + G + 8     (a workgroup's accumulators over its tiles, then G partials)
      library trainer         weights: n // 128 + 128 + tail + 2 (split-K products), biases: rows per band + 256 + ...
    loss                      K(d out) + depth of the loss sum
    optimiser                 see learning_reference.adam_clip (sum of squares, powf bias corrections, 2-3 roundings a step)

Samples that f32 rounding could push to the other side of a branch are dropped by the reference's filter before the
kernels see them; how many is printed (run with -s).  Largest err / (u mag) observed on the MI355X, per kernel, is
printed at the end of the module and quoted in each test's docstring.
"""
import ctypes as C
import json

import numpy as np
import pytest

from tests import learning_reference as R

pytestmark = pytest.mark.gpu

OBSERVED = {}          # kernel -> largest err / (u mag)
DROPPED = {}           # configuration -> samples the filter dropped


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    yield torch
    print("\nlearning kernels, largest err/(u mag): " + json.dumps({k: round(v, 3) for k, v in sorted(OBSERVED.items())}))
    print("learning kernels, samples dropped by the filter: " + json.dumps(DROPPED))


def _check(kernel, what, got, ref, mag, K):
    ok, r, msg = R.ratio_report(got, ref, mag, K)
    OBSERVED[kernel] = max(OBSERVED.get(kernel, 0.0), r)
    assert ok, "%s, %s: %s" % (kernel, what, msg)


def _host(t):
    return t.detach().cpu().numpy()


def _layers(torch, S, H, A, seed, zero_b1=False):
    """Linear(S,H)-ReLU-Linear(H,H)-ReLU-Linear(H,A) on cuda:0; weights ~ N(0, 1/fan_in), biases ~ N(0, 0.01), every
    other first-layer bias exactly 0 with zero_b1 (all-zero rows then give exact zero pre-activations)."""
    nn = torch.nn
    g = torch.Generator().manual_seed(seed)
    layers = [nn.Linear(S, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(), nn.Linear(H, A)]
    with torch.no_grad():
        for l in layers[::2]:
            l.weight.copy_(torch.randn(l.weight.shape, generator=g) / np.sqrt(l.in_features))
            l.bias.copy_(torch.randn(l.bias.shape, generator=g) * 0.1)
        if zero_b1:
            layers[0].bias[::2] = 0.0
    return [l.to("cuda:0") for l in layers]


def _cdiv(a, b):
    return -(-a // b)


def _first_kept(keep, n):
    """Indices of the first n candidates the filter keeps, and how many it dropped before the n-th."""
    idx = np.nonzero(keep)[0]
    assert idx.size >= n, "the filter dropped too many candidates"
    idx = idx[:n]
    return idx, int(idx[-1] + 1 - n)


def _actor_samples(rs, params, S, A, n, eps, zeros, big):
    k1, k2, k3 = R.forward_k(S, params[2].shape[0])
    m = n + n // 3 + 64
    x = rs.randn(m, S).astype(np.float32)
    if zeros:
        x[rs.rand(m) < 0.05] = 0.0
    fw = R.forward(params, x)
    out = fw["out"]
    actions = rs.randint(0, A, m)
    if big:
        actions[::2] = out[::2].argmax(1)                 # a taken action near the top too: its ratio does not underflow
    lp = out[np.arange(m), actions] - (out.max(1) + np.log(np.exp(out - out.max(1, keepdims=True)).sum(1)))
    old = (lp + rs.randn(m) * 0.3).astype(np.float32)
    adv = rs.randn(m).astype(np.float32)
    if zeros:
        adv[rs.rand(m) < 0.05] = 0.0
    act = R.actor_loss(out, fw["m_out"], actions, old, adv, eps, 1.0)
    idx, dropped = _first_kept(R.keep_samples(fw, k1, k2, k3, act)[0], n)
    return x[idx], actions[idx], old[idx], adv[idx], dropped


def _critic_samples(rs, params, S, n, zeros):
    k1, k2, _ = R.forward_k(S, params[2].shape[0])
    m = n + n // 3 + 64
    x = rs.randn(m, S).astype(np.float32)
    if zeros:
        x[rs.rand(m) < 0.05] = 0.0
    idx, dropped = _first_kept(R.keep_samples(R.forward(params, x), k1, k2)[0], n)
    return x[idx], rs.randn(n).astype(np.float32), dropped


def _reference(params, x, mode, aux, count, eps, depth_w, depth_b, depth_loss):
    """f64 loss, d out, gradients with magnitudes and K."""
    S, H = params[0].shape[1], params[0].shape[0]
    _, _, k3 = R.forward_k(S, H)
    fw = R.forward(params, x)
    if mode == 0:
        lo = R.actor_loss(fw["out"], fw["m_out"], aux[0], aux[1], aux[2], eps, count)
        k_dout = k3 + 8
    else:
        lo = R.critic_loss(fw["out"], fw["m_out"], aux[0], count)
        k_dout = k3 + 4
    grads, mags, ks = R.backward(params, fw, lo["dout"], lo["dout_mag"], k_dout, depth_w, depth_b)
    return fw, lo, k_dout, k_dout + depth_loss, grads, mags, ks


NAMES = ["dW1", "db1", "dW2", "db2", "dW3", "db3"]


def _check_grads(kernel, tag, tr, grads, mags, ks):
    for view, name, g, mg, K in zip(tr.views, NAMES, grads, mags, ks):
        _check(kernel, "%s %s" % (tag, name), _host(view), g, mg, K)


# ------------------------------------------------------------------------------------------------ one-launch MFMA pass
def _groups(n):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    return _capi.lib().fjsp_mlp_train_groups(n)


# n as a function of G, the device's workgroup count (fjsp_mlp_train_groups of a large n: one workgroup per CU)
N_OF = {"1": lambda G: 1, "31": lambda G: 31, "32": lambda G: 32, "33": lambda G: 33, "32G": lambda G: 32 * G,
        "32G+1": lambda G: 32 * G + 1, "96G-5": lambda G: 3 * 32 * G - 5, "200000": lambda G: 200000}

# (S, A, n, count / n, eps, zero rows + zero advantages, logits to +-100): every value of each axis at least once,
# S = 31 with A = 32 and with n = 32 G + 1.
MFMA_CASES = [
    (1, 1, "1", 1, 0.2, True, False),
    (2, 2, "31", 3, 0.0, False, False),
    (31, 32, "32", 1, 0.2, True, False),
    (2, 31, "33", 3, 0.2, False, True),
    (31, 2, "32G+1", 1, 0.0, True, False),
    (1, 32, "32G", 3, 0.2, False, False),
    (2, 1, "96G-5", 1, 0.2, True, False),
    (31, 31, "200000", 3, 0.2, True, False),
]


@pytest.mark.parametrize("S,A,nspec,cmul,eps,zeros,big", MFMA_CASES)
def test_mfma_training_pass_matches_f64_reference(torch_gpu, S, A, nspec, cmul, eps, zeros, big):
    """fjsp_mlp_train_pass (csrc/fjsp_mlp_train.hip) and the gradient finish, actor and critic, against the f64
    reference: loss and all six gradients componentwise, K = K(d pre-activation) [+ K(activation)] + 32 ceil(tiles/G)
    + G + 8 (K3 + 8 + ceil(tiles/G) + G + 16 for the loss); the critic's train_step values_out against the f64 forward
    (K3).  Largest err/(u mag) observed on the MI355X: 0.12 (actor), 1.25 (critic), 0.34 (values_out)."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.agents import fused_mlp
    n = N_OF[nspec](_groups(1 << 30))
    H = 128
    G = _groups(n)
    tpg = _cdiv(_cdiv(n, 32), G)                   # tiles per workgroup
    depth_w = min(n, 32 * tpg + G + 8)
    depth_loss = min(n, tpg + G + 16)
    count = float(cmul * n)
    rs = np.random.RandomState(S * 100 + A + n % 997)
    for mode in (0, 1):
        layers = _layers(torch, S, H, A if mode == 0 else 1, seed=S + 7 * A + mode, zero_b1=zeros)
        if big and mode == 0:
            # the final layer scaled so that half of the samples have a logit beyond +-100 (exp overflows f32 past 88.7)
            probe = R.forward([_host(t).astype(np.float64) for l in layers[::2] for t in (l.weight, l.bias)],
                              np.random.RandomState(0).randn(256, S).astype(np.float32))
            s = 100.0 / float(np.median(np.abs(probe["out"]).max(1)))
            with torch.no_grad():
                layers[4].weight.mul_(s)
                layers[4].bias.mul_(s)
        tr = fused_mlp.FusedMLP(layers, lr=1e-3)
        assert tr.mfma_pass_supported()
        Ao = A if mode == 0 else 1
        params = R.unflatten(_host(tr.flat), S, H, Ao)
        if mode == 0:
            x, actions, old, adv, dropped = _actor_samples(rs, params, S, A, n, eps, zeros, big)
            aux_h = (actions, old, adv)
            aux_d = [torch.from_numpy(a).to("cuda:0") for a in (actions.astype(np.float32), old, adv)]
        else:
            x, ret, dropped = _critic_samples(rs, params, S, n, zeros)
            aux_h = (ret,)
            aux_d = [torch.from_numpy(ret).to("cuda:0"), None, None]
        DROPPED["mfma S%d A%d n%d mode%d" % (S, A, n, mode)] = dropped
        xd = torch.from_numpy(x).to("cuda:0")
        cd = torch.full((1,), count, device="cuda:0")
        loss = tr.train_pass(mode, xd, aux_d[0], aux_d[1], aux_d[2], cd, eps)
        torch.cuda.synchronize()
        fw, lo, k_dout, k_loss, grads, mags, ks = _reference(params, x, mode, aux_h, count, eps, depth_w, depth_w, depth_loss)
        if big and mode == 0:
            assert np.abs(fw["out"]).max() > 100.0
        kernel = "mfma_pass_actor" if mode == 0 else "mfma_pass_critic"
        tag = "S=%d A=%d n=%d count=%g eps=%g" % (S, Ao, n, count, eps)
        _check(kernel, tag + " loss", float(loss), lo["loss"], lo["loss_mag"], k_loss)
        _check_grads(kernel, tag, tr, grads, mags, ks)
        if mode == 1:
            g_pass = tr.grad.clone()
            values = torch.empty(n, dtype=torch.float32, device="cuda:0")
            tr.train_step(1, xd, aux_d[0], None, None, cd, values_out=values)
            torch.cuda.synchronize()
            assert torch.equal(tr.grad, g_pass)            # the step's pass is the same pass
            _check("mfma_step_values", tag + " values_out", _host(values), fw["out"][:, 0], fw["m_out"][:, 0], R.forward_k(S, H)[2])


# ------------------------------------------------------------------------------------------------ library-GEMM trainer
LIB_CASES = [(64, 200, 7), (130, 200, 32), (256, 868, 7), (130, 868, 7), (64, 131075, 32), (130, 131075, 7), (256, 131075, 32)]


@pytest.mark.parametrize("H,n,A", LIB_CASES)
def test_library_trainer_matches_f64_reference(torch_gpu, H, n, A):
    """FusedMLP.forward (library GEMMs, bias + ReLU epilogues) -> actor_loss / critic_loss (fjsp_ppo_actor_loss,
    fjsp_ppo_critic_loss) -> backward (split-K weight products, fjsp_relu_bwd_bias both variants: H = 130 is not a
    multiple of 4) against the f64 reference: loss, d out and all six gradients.  n = 200 (one band), 868 (a partial
    last band), 131075 (the 512-band cap).  K: weights K(dz) + K(h) + n//128 + 128 + tail + 3, biases K(dz) + rows +
    256 + blocks/256 + 12, loss K(d out) + 8 + blocks/256 + 12 (critic: + 256).  Largest err/(u mag) observed on
    the MI355X: 0.26 (actor), 0.62 (critic)."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.agents import fused_mlp
    S, eps = 20, 0.2
    per = n // 128
    depth_w = min(n, n if per == 0 else per + 128 + (n - 128 * per) + 2)
    nparts = min(512, max(1, n // 256))
    rows = _cdiv(n, nparts)
    blocks = _cdiv(n, rows)
    depth_b = min(n, rows + 256 + _cdiv(blocks, 256) + 12)
    count = float(n)
    rs = np.random.RandomState(H + n)
    for mode in (0, 1):
        Ao = A if mode == 0 else 1
        layers = _layers(torch, S, H, Ao, seed=H + n + mode, zero_b1=(n == 868))
        assert fused_mlp.supported(layers, "cuda:0")
        tr = fused_mlp.FusedMLP(layers, lr=1e-3)
        params = R.unflatten(_host(tr.flat), S, H, Ao)
        cd = torch.full((1,), count, device="cuda:0")
        if mode == 0:
            x, actions, old, adv, dropped = _actor_samples(rs, params, S, A, n, eps, n == 868, False)
            aux_h = (actions, old, adv)
        else:
            x, ret, dropped = _critic_samples(rs, params, S, n, n == 868)
            aux_h = (ret,)
        DROPPED["library H%d n%d mode%d" % (H, n, mode)] = dropped
        xd = torch.from_numpy(x).to("cuda:0")
        tr.forward(xd)
        if mode == 0:
            d = [torch.from_numpy(a).to("cuda:0") for a in (actions.astype(np.float32), old, adv)]
            loss = tr.actor_loss(d[0], d[1], d[2], eps, cd)
            depth_loss = min(n, 8 + _cdiv(_cdiv(n, 8), 256) + 12)
        else:
            loss = tr.critic_loss(torch.from_numpy(ret).to("cuda:0"), cd)
            depth_loss = min(n, 256 + _cdiv(_cdiv(n, 256), 256) + 12)
        tr.backward()
        torch.cuda.synchronize()
        b = tr._buf[n]
        fw, lo, k_dout, k_loss, grads, mags, ks = _reference(params, x, mode, aux_h, count, eps, depth_w, depth_b, depth_loss)
        kernel = "library_actor" if mode == 0 else "library_critic"
        tag = "H=%d A=%d n=%d" % (H, Ao, n)
        _check(kernel, tag + " loss", float(loss), lo["loss"], lo["loss_mag"], k_loss)
        _check(kernel, tag + " dout", _host(b["dout"]), lo["dout"], lo["dout_mag"], k_dout)
        _check_grads(kernel, tag, tr, grads, mags, ks)


# ------------------------------------------------------------------------------------------------ fjsp_relu_bwd_bias
@pytest.mark.parametrize("width", [1, 3, 4, 128, 130, 256])
def test_relu_bwd_bias_matches_f64_reference(torch_gpu, width):
    """fjsp_relu_bwd_bias through the C ABI, n in {1, 255, 256, 257, 50000}, with h and with h = NULL, on aligned
    pointers (the 16-byte variant where the width allows) and on pointers one float off (the scalar variant): the masked
    dh bit for bit, the bias gradient within K = rows per band + 256 + ceil(blocks / 256) + 12 (error-free inputs).
    Largest err/(u mag) observed on the MI355X: 2.8."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    lib = _capi.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rs = np.random.RandomState(width)
    for n in (1, 255, 256, 257, 50000):
        dh = rs.randn(n, width).astype(np.float32)
        h = np.maximum(rs.randn(n, width), 0.0).astype(np.float32)
        h[rs.rand(n, width) < 0.1] = -0.0
        nparts = min(512, max(1, n // 256))
        rows = _cdiv(n, nparts)
        blocks = _cdiv(n, rows)
        K = min(n, rows + 256 + _cdiv(blocks, 256) + 12)
        for with_h in (True, False):
            want = np.where(h > 0, dh, np.float32(0.0)) if with_h else dh
            ref = want.astype(np.float64).sum(0)
            mag = np.abs(want).astype(np.float64).sum(0)
            for off in (0, 1):
                dbuf = torch.zeros(n * width + 4, device="cuda:0")
                hbuf = torch.zeros(n * width + 4, device="cuda:0")
                dbuf[off:off + n * width] = torch.from_numpy(dh.reshape(-1)).to("cuda:0")
                hbuf[off:off + n * width] = torch.from_numpy(h.reshape(-1)).to("cuda:0")
                partial = torch.empty(nparts * width, device="cuda:0")
                out = torch.full((width,), float("nan"), device="cuda:0")
                hp = C.c_void_p(hbuf.data_ptr() + 4 * off) if with_h else None
                _capi.check(lib.fjsp_relu_bwd_bias(C.c_void_p(dbuf.data_ptr() + 4 * off), hp, n, width, C.c_void_p(partial.data_ptr()),
                                                   nparts, C.c_void_p(out.data_ptr()), stream))
                torch.cuda.synchronize()
                got_dh = _host(dbuf)
                tag = "width %d n %d h %s offset %d" % (width, n, with_h, off)
                assert np.array_equal(got_dh[off:off + n * width].reshape(n, width), want), tag + ": masked dh differs"
                assert not got_dh[:off].any() and not got_dh[off + n * width:].any(), tag + ": wrote outside dh"
                _check("relu_bwd_bias", tag, _host(out), ref, mag, K)


# ------------------------------------------------------------------------------------------------ optimiser step
OPT_CASES = [("active", 1.0, 30.0), ("inactive", 1e6, 1.0), ("off", 0.0, 1.0), ("small_norm", 5e-3, 1e-2)]


def _check_opt(kernel, tag, st, flat, m, v, step):
    _check(kernel, tag + " params", flat, st["p"], st["mag_p"], st["k_p"])
    _check(kernel, tag + " exp_avg", m, st["m"], st["mag_m"], st["k_m"])
    _check(kernel, tag + " exp_avg_sq", v, st["v"], st["mag_v"], st["k_v"])
    assert step == st["step"], "%s: device step count %g, expected %d" % (tag, step, st["step"])


def _sumsq_depth(numel):
    return _cdiv(numel, 16384) + 80


@pytest.mark.parametrize("case,max_norm,norm", OPT_CASES)
def test_adam_clip_step_matches_f64_optimiser(torch_gpu, case, max_norm, norm):
    """fjsp_adam_clip_step (FusedMLP.step) over 40 fixed gradients (79 392 parameters: the grid-stride loop runs) with
    the clip active, inactive (coefficient clamped to exactly 1), off (max_norm = 0), and active at a gradient norm of
    1e-2 against max_norm 5e-3, where the + 1e-6 of the coefficient is 1e-4 relative: parameters, exp_avg, exp_avg_sq
    and the device step count after every step.  K from learning_reference.adam_clip (sum of squares of depth
    numel/16384 + 80).  Largest err/(u mag) observed on the MI355X: 45."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.agents import fused_mlp
    layers = _layers(torch, 20, 256, 32, seed=3)
    tr = fused_mlp.FusedMLP(layers, lr=1e-3, max_norm=max_norm)
    p0 = _host(tr.flat).copy()
    rs = np.random.RandomState(len(case))
    grads = []
    for t in range(40):
        g = rs.randn(tr.numel) * rs.choice([0.1, 1.0, 10.0], tr.numel)
        grads.append((g * (norm * (1.0 + 0.05 * t) / np.linalg.norm(g))).astype(np.float32))
    ref = R.adam_clip(p0, grads, 1e-3, tr.betas, tr.eps, max_norm, sumsq_depth=_sumsq_depth(tr.numel))
    if case in ("active", "small_norm"):
        assert max(st["coef"] for st in ref) < 1.0
    else:
        assert all(st["coef"] == 1.0 for st in ref)
    for t, g in enumerate(grads):
        tr.grad.copy_(torch.from_numpy(g))
        tr.step()
        torch.cuda.synchronize()
        _check_opt("adam_clip_step", "%s step %d" % (case, t + 1), ref[t], _host(tr.flat), _host(tr.exp_avg), _host(tr.exp_avg_sq),
                   float(tr.step_count))


@pytest.mark.parametrize("case,max_norm,norm", OPT_CASES)
def test_train_step_optimiser_matches_f64_optimiser(torch_gpu, case, max_norm, norm):
    """fjsp_mlp_train_step's adam_apply_kernel (clip coefficient from the gradient finish's sums of squares, step count
    advanced by the finish) over 40 actor steps: after each, the gradient it applied is read back and the f64 optimiser
    replays the sequence; parameters, exp_avg, exp_avg_sq and the step count are compared after every step.  Clip
    active, inactive, off, and active at a gradient norm of ~1e-2 against max_norm 5e-3 (advantages scaled to it).
    Largest err/(u mag) observed on the MI355X: 23."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.agents import fused_mlp
    n, S, A = 5000, 20, 24
    rs = np.random.RandomState(11)
    x = torch.from_numpy(rs.randn(n, S).astype(np.float32)).to("cuda:0")
    actions = torch.from_numpy(rs.randint(0, A, n).astype(np.float32)).to("cuda:0")
    old = torch.from_numpy((-rs.rand(n) * 3 - 0.2).astype(np.float32)).to("cuda:0")
    adv = torch.from_numpy(rs.randn(n).astype(np.float32)).to("cuda:0")
    count = torch.full((1,), float(n), device="cuda:0")
    layers = _layers(torch, S, 128, A, seed=5)
    probe = fused_mlp.FusedMLP(_layers(torch, S, 128, A, seed=5), lr=1e-3)
    probe.train_pass(0, x, actions, old, adv, count, 0.2)
    n0 = float(probe.grad.norm())
    adv = adv * (norm / n0)                                             # the first step's gradient norm ~ `norm`
    tr = fused_mlp.FusedMLP(layers, lr=1e-3, max_norm=max_norm)
    p0 = _host(tr.flat).copy()
    grads, seen = [], []
    for t in range(40):
        tr.train_step(0, x, actions, old, adv, count, 0.2)
        torch.cuda.synchronize()
        grads.append(_host(tr.grad).copy())
        if t == 0:
            n1 = float(np.linalg.norm(grads[0].astype(np.float64)))
            assert abs(n1 / norm - 1.0) < 1e-3, "first gradient norm %g, wanted %g (unscaled %g)" % (n1, norm, n0)
        seen.append((_host(tr.flat).copy(), _host(tr.exp_avg).copy(), _host(tr.exp_avg_sq).copy(), float(tr.step_count)))
    ref = R.adam_clip(p0, grads, 1e-3, tr.betas, tr.eps, max_norm, sumsq_depth=_sumsq_depth(tr.numel))
    if case in ("active", "small_norm"):
        assert ref[0]["coef"] < 1.0                # (the gradient norm changes as the parameters move)
    else:
        assert all(st["coef"] == 1.0 for st in ref)
    for t, (st, (flat, m, v, step)) in enumerate(zip(ref, seen)):
        _check_opt("train_step_adam", "%s step %d" % (case, t + 1), st, flat, m, v, step)


# ------------------------------------------------------------------------------------------------ in-kernel actor
@pytest.mark.parametrize("S", [1, 31, 32])
@pytest.mark.parametrize("A", [1, 2, 32])
def test_native_actor_forward_matches_f64_reference(torch_gpu, S, A):
    """fjsp_actor_forward (the fused rollout's actor: f64 states rounded to f32, fmaf chains, max-shifted softmax) at
    n in {1, 15, 16, 17, 4097} (16 states per workgroup), states with entries up to ~1e3, against the f64 forward +
    softmax: probabilities componentwise with mag_j = p_j (m_out_j + max m_out + 1) + TINY, K = K3 + 8.
    Largest err/(u mag) observed on the MI355X: 0.68."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO import MPPPO as M
    torch.manual_seed(S * 40 + A)
    actor = M.ActorNet(S, 128, 2, A).to("cuda:0")
    lin = [l for l in actor.layers if isinstance(l, torch.nn.Linear)]
    params = [R.as64(t) for l in lin for t in (l.weight, l.bias)]
    k1, k2, k3 = R.forward_k(S, 128)
    rs = np.random.RandomState(S + 3 * A)
    for n in (1, 15, 16, 17, 4097):
        m = n + n // 4 + 32
        st = rs.randn(m, S) * 10.0 ** rs.uniform(-1, 3, (m, 1))
        x = st.astype(np.float32)
        idx, DROPPED["actor_forward S%d A%d n%d" % (S, A, n)] = _first_kept(R.keep_samples(R.forward(params, x), k1, k2)[0], n)
        fw = R.forward(params, x[idx])
        p = R.softmax(fw["out"])
        mag = p * (fw["m_out"] + fw["m_out"].max(1, keepdims=True) + 1.0) + R.TINY
        probs = M.native_actor_forward(actor, torch.from_numpy(st[idx]).to("cuda:0"))
        torch.cuda.synchronize()
        _check("actor_forward", "S=%d A=%d n=%d" % (S, A, n), _host(probs), p, mag, k3 + 8)


# ------------------------------------------------------------------------------------------------ trainer dispatch fix
@pytest.mark.parametrize("hidden,A", [(512, 30), (128, 64)])
def test_learner_with_shapes_the_kernels_refuse_trains_eagerly(torch_gpu, hidden, A):
    """A PPOLearner whose network the library kernels refuse (hidden > 256: fjsp_relu_bwd_bias; > 32 actions:
    fjsp_ppo_actor_loss) learns from 40 000 GPU samples without error, on the eager path, and its parameters after the
    round equal those of a learner with fused_learn = False bit for bit."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO import MPPPO as M
    T, N, S = 40, 1000, 20
    g = torch.Generator(device="cuda:0").manual_seed(hidden + A)
    states = torch.randn(T, N, S, device="cuda:0", generator=g)
    actions = torch.randint(0, A, (T, N), device="cuda:0", generator=g)
    old_lp = -torch.rand(T, N, device="cuda:0", generator=g) * 3 - 0.2
    returns = torch.randn(T, N, device="cuda:0", generator=g)
    valid = torch.ones(T, N, device="cuda:0")
    learners = []
    for fused in (True, False):
        ln = M.PPOLearner(S, A, hidden_size=hidden, device="cuda:0", seed=4)
        ln.fused_learn = fused
        before = [p.detach().clone() for p in ln.actor_new.parameters()]
        c_loss, a_loss = ln.learn(states, actions, old_lp, returns, valid)
        assert np.isfinite(c_loss) and np.isfinite(a_loss)
        assert ln.path == "eager"
        assert any(not torch.equal(b, p) for b, p in zip(before, ln.actor_new.parameters()))
        learners.append(ln)
    torch.cuda.synchronize()
    for net in ("actor_new", "critic"):
        for p, q in zip(getattr(learners[0], net).parameters(), getattr(learners[1], net).parameters()):
            assert torch.equal(p, q), net
