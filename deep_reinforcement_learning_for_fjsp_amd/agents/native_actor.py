"""The in-kernel actor: an ActorNet-shaped network (Linear-ReLU-Linear-ReLU-Linear in `.layers`) as the library's
fjsp_actor_params, and its forward pass through the library (fjsp_actor_forward).  The fused policy rollout of
agents.MPPPO and the decoding launches of policy_search hand the same parameters to the environment kernels."""
import ctypes as C

import torch
from torch import nn

from .. import _capi


def native_actor_params(actor):
    """fjsp_actor_params for an ActorNet of the in-kernel shape (state_size <= 32 -> 128 -> 128 -> n_actions <= 32, on
    the GPU), or None when the network has another shape: device pointers into the nn.Linear parameters themselves
    (the optimiser updates them in place, so the kernels always read the current policy)."""
    lin = [l for l in actor.layers if isinstance(l, nn.Linear)]
    if len(lin) != 3 or not lin[0].weight.is_cuda:
        return None
    S, H, A = lin[0].in_features, lin[0].out_features, lin[2].out_features
    if H != 128 or lin[1].in_features != 128 or lin[1].out_features != 128 or lin[2].in_features != 128 or S > 32 or A > 32:
        return None
    tensors = [lin[0].weight, lin[0].bias, lin[1].weight, lin[1].bias, lin[2].weight, lin[2].bias]
    if any(t.dtype != torch.float32 or not t.is_contiguous() for t in tensors):
        return None
    return _capi.ActorParams(*[_capi.ptr(t) for t in tensors], S, H, A)


def native_actor_forward(actor, states64, out=None):
    """ActorNet.forward through the library's actor kernel (fjsp_actor_forward): f64[n, S] states -> f32[n, A]
    probabilities, the arithmetic the fused policy rollout performs inside the environment kernel."""
    ap = native_actor_params(actor)
    if ap is None:
        raise ValueError("the in-kernel actor is state_size (<= 32) -> 128 -> 128 -> n_actions (<= 32) on the GPU")
    states64 = states64.contiguous()
    n = states64.shape[0]
    probs = torch.empty(n, ap.n_actions, dtype=torch.float32, device=states64.device) if out is None else out
    _capi.check(_capi.lib().fjsp_actor_forward(C.byref(ap), _capi.ptr(states64), n, _capi.ptr(probs),
                                               _capi.stream(states64.device.index)))
    return probs
