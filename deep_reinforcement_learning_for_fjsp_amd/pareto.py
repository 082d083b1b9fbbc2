"""Pareto fronts of the candidates of every env, on the device: the selection (fjsp_pareto_select, csrc/fjsp_pareto.hip)
and the reference's front metrics GD / IGD / Spread (utilities/Utility_Class.py:119-227, DataProcess) per env.

A front is a padded tensor f64[N, cap, D] with a count i32[N]: env i's points are front[i, :min(count[i], cap)], in
ascending lexicographic order (objective 0 most significant, np.unique(axis=0)'s order, so the array
filter_pareto_front returns); the rows past them are NaN.  Lower is better in every objective.  The metrics are
batched torch ops over the padded fronts (fronts are small; no kernel), device tensors in and out, f64 throughout.
lookahead.rule_front and policy_search.pareto_front are the searches that end in `select`.
"""
import torch

from . import _capi
from ._capi import ptr as _ptr

MAX_CANDIDATES, MAX_OBJECTIVES = 1024, 4        # the limits of fjsp_pareto_select (include/fjsp_amd.h)


def select(obj, valid=None, cap=None):
    """fjsp_pareto_select (include/fjsp_amd.h) on the current stream: obj f64[C, N, D] on the device (candidate-major:
    entry (c, i) = the objective vector of candidate c of source env i), valid u8[C, N] or None (every candidate
    valid), cap (default C) -> (index i32[N, cap], count i32[N], mask u8[C, N]).

    A candidate with valid == 0 or a NaN objective is not one.  Candidate c is on env i's front iff no candidate is <=
    in every objective and < in one, and no candidate of lower index has the same vector.  index[i] = the front members
    in ascending lexicographic order of their vectors, -1 past the front; count[i] = the front's size, which may exceed
    cap (index then holds the first cap members); mask = 1 on the front."""
    if not torch.is_tensor(obj) or obj.dim() != 3 or obj.dtype != torch.float64 or obj.device.type != "cuda":
        raise ValueError("pareto.select: obj must be an f64[C, N, D] device tensor")
    C, N, D = obj.shape
    cap = C if cap is None else int(cap)
    dev = obj.device
    obj = obj.contiguous()
    if valid is not None:
        valid = torch.as_tensor(valid, device=dev).to(torch.uint8).reshape(C, N).contiguous()
    index = torch.empty((N, max(cap, 0)), dtype=torch.int32, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    mask = torch.empty((C, N), dtype=torch.uint8, device=dev)
    dev_index = torch.cuda.current_device() if dev.index is None else dev.index
    _capi.check(_capi.lib().fjsp_pareto_select(_ptr(obj), _ptr(valid), N, C, D, cap, _ptr(index), _ptr(count), _ptr(mask),
                                               _capi.stream(dev_index)))
    return index, count, mask


def front_points(obj, index):
    """obj f64[C, N, D], index i32[N, cap] of select -> f64[N, cap, D]: the objective vectors of the front members (the
    input's bits), NaN past the front."""
    C, N, D = obj.shape
    rows = torch.gather(obj.permute(1, 0, 2), 1, index.clamp(min=0).long()[:, :, None].expand(N, index.shape[1], D))
    return torch.where((index >= 0)[:, :, None], rows, torch.full_like(rows, float("nan")))


def normalise(front, max_values):
    """DataProcess.normalized_data (:124-130): front / max_values; max_values f64[D] or, per env, f64[N, D]."""
    max_values = torch.as_tensor(max_values, dtype=torch.float64, device=front.device)
    return front / (max_values[:, None, :] if max_values.dim() == 2 else max_values)


def _points(front, count):
    """(front f64[N, P, D], present bool[N, P], n i64[N]) of a padded front: its first min(count, P) rows."""
    if not torch.is_tensor(front) or front.dim() != 3:
        raise ValueError("pareto: a front must be a tensor [N, points, D]")
    front = front.to(torch.float64)
    n = torch.as_tensor(count, device=front.device).long().reshape(front.shape[0]).clamp(max=front.shape[1])
    return front, torch.arange(front.shape[1], device=front.device)[None, :] < n[:, None], n


def _distance_square(a, b):
    """DataProcess.distance_square (:164-166) between every point of a [N, P, D] and of b [N, Q, D] -> [N, P, Q],
    summed over the objectives in order."""
    d2 = None
    for d in range(a.shape[2]):
        t = (a[:, :, None, d] - b[:, None, :, d]) ** 2
        d2 = t if d2 is None else d2 + t
    return d2


def _masked_min(x, present, dim):
    return torch.where(present, x, torch.full_like(x, float("inf"))).min(dim=dim).values


def _masked_sum(x, present):
    return torch.where(present, x, torch.zeros_like(x)).sum(dim=1)


def gd(front, count, true_front, true_count):
    """DataProcess.calculate_gd (:184-198) per env -> f64[N]: the square root of the SUM over the front's points of the
    squared distance to the nearest point of the true front, divided by the number of points (the reference's form,
    not the root of the mean).  NaN for an empty front, inf against an empty true front."""
    p, pp, pn = _points(front, count)
    t, tp, _ = _points(true_front, true_count)
    nearest = _masked_min(_distance_square(p, t), tp[:, None, :], 2)
    return torch.sqrt(_masked_sum(nearest, pp)) / pn.double()


def igd(front, count, true_front, true_count):
    """DataProcess.calculate_igd (:168-182) per env -> f64[N]: the mean over the true front's points of the distance to
    the nearest point of the front.  NaN for an empty true front, inf for an empty front."""
    p, pp, _ = _points(front, count)
    t, tp, tn = _points(true_front, true_count)
    nearest = _masked_min(torch.sqrt(_distance_square(t, p)), pp[:, None, :], 2)
    return _masked_sum(nearest, tp) / tn.double()


def _first_argmin_rows(x, present):
    """x [N, P, D], present [N, P] -> [N, D, D]: for each objective i the first present row with the smallest x[:, :, i]
    (np.argmin's choice)."""
    N, P, D = x.shape
    col = torch.where(present[:, :, None], x, torch.full_like(x, float("inf")))
    least = col.min(dim=1, keepdim=True).values
    pos = torch.arange(P, device=x.device)[None, :, None].expand(N, P, D)
    first = torch.where((col == least) & present[:, :, None], pos, torch.full_like(pos, P)).min(dim=1).values      # [N, D]
    return torch.gather(x, 1, first.clamp(max=P - 1)[:, :, None].expand(N, D, D))


def spread(front, count, true_front, true_count):
    """DataProcess.calculate_spread (:200-227) per env -> f64[N]: with d_a = the distance from point a of the front to its
    nearest other point, m = their mean and E = the sum over the objectives of the distance between the front's and the
    true front's extreme point of that objective (the first point with the smallest value), (E + sum |d_a - m|) / (E +
    n m).  NaN for a front of fewer than two points or an empty true front."""
    p, pp, pn = _points(front, count)
    t, tp, tn = _points(true_front, true_count)
    dist = torch.sqrt(_distance_square(p, p))
    other = pp[:, None, :] & (dist != 0.0)
    diaa = _masked_min(dist, other, 2)                                     # inf for a point with no other point
    daa = _masked_sum(diaa, pp) / pn.double()
    sq = (_first_argmin_rows(p, pp) - _first_argmin_rows(t, tp)) ** 2       # [N, objective i, D]
    e = None
    for i in range(sq.shape[1]):
        d2 = None
        for d in range(sq.shape[2]):
            d2 = sq[:, i, d] if d2 is None else d2 + sq[:, i, d]
        e = torch.sqrt(d2) if e is None else e + torch.sqrt(d2)
    out = (e + _masked_sum((diaa - daa[:, None]).abs(), pp)) / (e + pn.double() * daa)
    return torch.where((pn >= 2) & (tn >= 1), out, torch.full_like(out, float("nan")))
