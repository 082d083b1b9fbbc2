"""CPU: the float64 reference of the PPO learning kernels (tests/learning_reference.py) against torch in float64, and
which networks the fused trainer accepts.  The GPU kernel tests (test_gpu_learning_kernels.py) trust the reference
because of these tests."""
import numpy as np
import pytest
import torch
from torch import nn

from tests import learning_reference as R
from deep_reinforcement_learning_for_fjsp_amd.agents.MPPPO import MPPPO as M
from deep_reinforcement_learning_for_fjsp_amd.agents import fused_mlp


def _close(got, ref, what, rtol=1e-12):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=rtol * scale, err_msg=what)


def _net_f32(S, H, A, seed):
    g = torch.Generator().manual_seed(seed)
    layers = [nn.Linear(S, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(), nn.Linear(H, A)]
    with torch.no_grad():
        for l in layers[::2]:
            l.weight.copy_(torch.randn(l.weight.shape, generator=g) / np.sqrt(l.in_features))
            l.bias.copy_(torch.randn(l.bias.shape, generator=g) * 0.1)
    flat = torch.cat([t.reshape(-1) for l in layers[::2] for t in (l.weight, l.bias)]).detach()
    return layers, flat


def _autograd64(layers, x, loss_fn):
    """loss, d loss / d out and the six parameter gradients by torch autograd in float64."""
    lin = [l for l in layers if isinstance(l, nn.Linear)]
    ps = [t.detach().double().requires_grad_(True) for l in lin for t in (l.weight, l.bias)]
    h = torch.relu(torch.from_numpy(x).double() @ ps[0].T + ps[1])
    h = torch.relu(h @ ps[2].T + ps[3])
    out = h @ ps[4].T + ps[5]
    out.retain_grad()
    loss = loss_fn(out)
    loss.backward()
    return float(loss.detach()), out.grad.numpy(), [p.grad.numpy() for p in ps]


# the shapes of the GPU tests: MFMA pass (hidden 128, S and A at their edges), library trainer (hidden 64 / 130 / 256)
SHAPES = [(1, 128, 1), (2, 128, 2), (31, 128, 32), (2, 128, 31), (20, 64, 7), (20, 130, 32), (20, 256, 7)]


@pytest.mark.parametrize("S,H,A", SHAPES)
@pytest.mark.parametrize("eps", [0.0, 0.2])
def test_reference_actor_pass_equals_autograd_f64(S, H, A, eps):
    n = 300
    layers, flat = _net_f32(S, H, A, seed=S * 1000 + H + A)
    rs = np.random.RandomState(S + A)
    x = rs.randn(n, S).astype(np.float32)
    x[::17] = 0.0                                                                   # all-zero rows
    actions = rs.randint(0, A, n)
    params = R.unflatten(flat.numpy(), S, H, A)
    fw = R.forward(params, x)
    lp_ref = fw["out"][np.arange(n), actions] - np.log(np.exp(fw["out"]).sum(1))
    old = (lp_ref + rs.randn(n) * 0.3).astype(np.float32)
    adv = rs.randn(n).astype(np.float32)
    adv[::11] = 0.0                                                                 # advantage exactly 0
    count = 3.0 * n
    act = R.actor_loss(fw["out"], fw["m_out"], actions, old, adv, eps, count)
    grads, _, _ = R.backward(params, fw, act["dout"], act["dout_mag"], 0, 0, 0)

    def loss_fn(out):
        new_lp = torch.log_softmax(out, -1).gather(1, torch.from_numpy(actions).unsqueeze(1)).squeeze(1)
        terms = M.actor_loss_terms(new_lp, torch.from_numpy(old).double(), torch.from_numpy(adv).double(), R.f32(eps))
        return -terms.sum() / R.f32(count)
    loss, dout, ag = _autograd64(layers, x, loss_fn)
    _close(act["loss"], loss, "actor loss")
    _close(act["dout"], dout, "d loss / d logits")
    for i, (a, b) in enumerate(zip(grads, ag)):
        _close(a, b, "gradient %d" % i)


@pytest.mark.parametrize("S,H", [(1, 128), (31, 128), (20, 130), (20, 256)])
def test_reference_critic_pass_equals_autograd_f64(S, H):
    n = 257
    layers, flat = _net_f32(S, H, 1, seed=S + H)
    rs = np.random.RandomState(H)
    x = rs.randn(n, S).astype(np.float32)
    ret = rs.randn(n).astype(np.float32)
    params = R.unflatten(flat.numpy(), S, H, 1)
    fw = R.forward(params, x)
    cr = R.critic_loss(fw["out"], fw["m_out"], ret, n)
    grads, _, _ = R.backward(params, fw, cr["dout"], cr["dout_mag"], 0, 0, 0)
    loss, dout, ag = _autograd64(layers, x, lambda out: ((out.squeeze(1) - torch.from_numpy(ret).double()) ** 2).sum() / n)
    _close(cr["loss"], loss, "critic loss")
    _close(cr["dout"], dout, "d loss / d value")
    for i, (a, b) in enumerate(zip(grads, ag)):
        _close(a, b, "gradient %d" % i)


@pytest.mark.parametrize("eps", [0.0, 0.2])
def test_reference_surrogate_ties_equal_autograd_f64(eps):
    """The constructed ties: ratio exactly at 1 - eps and 1 + eps, inside the band, outside it, advantage 0 -- d term /
    d ratio as autograd takes it (torch.minimum splits a tie in half, clamp passes the gradient on the closed interval)."""
    e = R.f32(eps)
    ratio = np.array([1.0 - e, 1.0 + e, 1.0, 1.0 - e / 2, 1.0 + e / 2, 0.5, 1.7, 1.0 - e, 1.0 + e, 0.9, 1.3], dtype=np.float64)
    adv = np.array([1.5, 1.5, -2.0, 0.7, -0.7, 1.0, 1.0, -1.5, -1.5, 0.0, 0.0], dtype=np.float64)
    terms, g, *_ = R.surrogate(ratio, adv, e)
    rt = torch.from_numpy(ratio).requires_grad_(True)
    # MPPPO.actor_loss_terms's surrogate on the ratio itself (from log-probabilities the ties would not be exact)
    at = torch.min(torch.from_numpy(adv) * rt, torch.from_numpy(adv) * torch.clamp(rt, 1.0 - e, 1.0 + e))
    (grad,) = torch.autograd.grad(at.sum(), [rt])
    np.testing.assert_array_equal(terms, at.detach().numpy())
    np.testing.assert_array_equal(g, grad.numpy())
    assert g[0] == 1.5 and g[9] == 0.0 and g[10] == 0.0


def _torch_adam(p0, grads, lr, betas, eps, max_norm):
    p = torch.from_numpy(R.as64(p0)).requires_grad_(True)
    opt = torch.optim.Adam([p], lr=R.f32(lr), betas=(R.f32(betas[0]), R.f32(betas[1])), eps=R.f32(eps))
    out = []
    for g in grads:
        p.grad = torch.from_numpy(R.as64(g))
        if R.f32(max_norm) > 0:
            torch.nn.utils.clip_grad_norm_([p], R.f32(max_norm))
        opt.step()
        st = opt.state[p]
        out.append((p.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()))
    return out


@pytest.mark.parametrize("max_norm,gscale", [(1.0, 3.0), (1e6, 1.0), (0.0, 1.0), (5e-3, 1e-2 / 40.0)])
def test_reference_optimiser_equals_torch_adam_f64(max_norm, gscale):
    """clip active, clip inactive (coefficient clamped to exactly 1), clip off (max_norm = 0), and a small norm where the
    + 1e-6 in the coefficient is visible, over 30 steps."""
    rs = np.random.RandomState(int(max_norm * 7) + 1)
    numel = 1600
    p0 = rs.randn(numel).astype(np.float32)
    grads = [(rs.randn(numel) * gscale * (1 + 0.1 * t)).astype(np.float32) for t in range(30)]
    ref = R.adam_clip(p0, grads, 1e-3, (0.9, 0.999), 1e-4, max_norm)
    tor = _torch_adam(p0, grads, 1e-3, (0.9, 0.999), 1e-4, max_norm)
    for t, (st, (p, m, v)) in enumerate(zip(ref, tor)):
        _close(st["p"], p, "params after step %d" % (t + 1))
        _close(st["m"], m, "exp_avg after step %d" % (t + 1))
        _close(st["v"], v, "exp_avg_sq after step %d" % (t + 1))
    coefs = [st["coef"] for st in ref]
    if max_norm == 1.0 or max_norm == 5e-3:
        assert max(coefs) < 1.0
    else:
        assert all(c == 1.0 for c in coefs)


def test_reference_sample_filter_keeps_structural_zeros():
    """All-zero rows with zero first-layer biases give pre-activations of exactly 0 with magnitude 0: kept.  A unit
    whose pre-activation is a tiny non-zero sum of large terms is dropped."""
    S, H, A = 4, 8, 3
    rs = np.random.RandomState(0)
    params = [rs.randn(H, S), np.zeros(H), rs.randn(H, H), rs.randn(H) * 0.1, rs.randn(A, H), rs.randn(A) * 0.1]
    params = [p.astype(np.float32).astype(np.float64) for p in params]
    x = rs.randn(6, S).astype(np.float32)
    x[0] = 0.0
    # row 1: its first unit's pre-activation cancels to (nearly) 0 against a large magnitude
    w = params[0][0]
    x[1] = np.float32(0.0)
    x[1, 0], x[1, 1] = np.float32(1000.0), np.float32(-1000.0 * w[0] / w[1])
    fw = R.forward(params, x)
    k1, k2, _ = R.forward_k(S, H)
    keep, dropped = R.keep_samples(fw, k1, k2)
    assert keep[0] and fw["m1"][0].max() == 0.0
    assert abs(fw["z1"][1, 0]) <= k1 * R.U * fw["m1"][1, 0] and not keep[1]
    assert dropped == int((~keep).sum()) >= 1


def test_fused_trainer_accepts_only_the_kernels_shapes():
    """agents/fused_mlp.supported(): the library-GEMM trainer's kernels take hidden widths <= 256 (fjsp_relu_bwd_bias)
    and <= 32 outputs (fjsp_ppo_actor_loss); other networks keep the eager path."""
    cuda = "cuda"
    assert not fused_mlp.supported(M.ActorNet(20, 512, 2, 30).layers, cuda)
    assert not fused_mlp.supported(M.ActorNet(20, 300, 2, 30).layers, cuda)
    assert not fused_mlp.supported(M.ActorNet(20, 257, 2, 30).layers, cuda)
    assert not fused_mlp.supported(M.ActorNet(20, 128, 2, 64).layers, cuda)
    assert not fused_mlp.supported(M.ActorNet(20, 128, 2, 33).layers, cuda)
    assert not fused_mlp.supported(M.CriticNet(20, 512, 2, 1).layers, cuda)
    for H, A in [(128, 30), (128, 32), (128, 1), (64, 7), (130, 32), (256, 32), (1, 1)]:
        assert fused_mlp.supported(M.ActorNet(20, H, 2, A).layers, cuda), (H, A)
    assert fused_mlp.supported(M.CriticNet(20, 256, 2, 1).layers, cuda)
    assert not fused_mlp.supported(M.ActorNet(20, 128, 2, 30).layers, "cpu")
    assert not fused_mlp.supported(M.ActorNet(20, 128, 3, 30).layers, cuda)       # three hidden layers
