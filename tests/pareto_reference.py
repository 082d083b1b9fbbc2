"""Numpy restatements of fjsp_pareto_select (include/fjsp_amd.h) -- the O(C^2) statement of its contract -- and of the
reference's front metrics (utilities/Utility_Class.py:168-227) in f64, with the error bounds the tests hold pareto.gd /
igd / spread to."""
import os

import numpy as np

EPS = 2.0 ** -53
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pareto_reference.npz")


def select(obj, valid=None, cap=None):
    """obj f64[C, N, D], valid u8[C, N] or None, cap (default C) -> (index i32[N, cap], count i32[N], mask u8[C, N])."""
    obj = np.asarray(obj, np.float64)
    C, N, D = obj.shape
    cap = C if cap is None else cap
    valid = np.ones((C, N), bool) if valid is None else np.asarray(valid).reshape(C, N) != 0
    index = np.full((N, cap), -1, np.int32)
    count = np.zeros(N, np.int32)
    mask = np.zeros((C, N), np.uint8)
    for i in range(N):
        ids = np.flatnonzero(valid[:, i] & ~np.isnan(obj[:, i, :]).any(axis=1))      # the candidates, ascending
        x = np.ascontiguousarray(obj[ids, i, :].T)                     # [D, candidates]
        le = np.ones((ids.size, ids.size), bool)                       # le[j, c]: j <= c in every objective
        for d in range(D):
            le &= np.less_equal.outer(x[d], x[d])
        # no NaN among the candidates, so "j < c in at least one objective" is "not c <= j in every one" = ~le[c, j], and
        # "<= everywhere and < nowhere" is "the same vector"; np.tri(...).T[j, c]: j before c
        out = (le & (~le.T | np.tri(ids.size, k=-1, dtype=bool).T)).any(axis=0)
        front = ids[~out]
        x = obj[:, i, :]
        below = np.zeros((front.size, front.size), bool)               # below[a, b]: a's vector lexicographically below b's
        for d in range(D - 1, -1, -1):
            xa, xb = x[front, d][:, None], x[front, d][None, :]
            below = (xa < xb) | ((xa == xb) & below)
        rank = below.sum(axis=0)
        assert np.array_equal(np.sort(rank), np.arange(front.size))    # distinct vectors: the ranks are positions
        ordered = np.empty(front.size, np.int64)
        ordered[rank] = front
        n = min(front.size, cap)
        index[i, :n] = ordered[:n]
        count[i] = front.size
        mask[front, i] = 1
    return index, count, mask


def front_points(obj, index):
    """f64[N, cap, D]: the front members' vectors, NaN past the front."""
    obj = np.asarray(obj, np.float64)
    N, cap = index.shape
    out = np.full((N, cap, obj.shape[2]), np.nan)
    for i in range(N):
        n = int((index[i] >= 0).sum())
        out[i, :n] = obj[index[i, :n], i]
    return out


def _d2(a, b):
    return float(np.sum((a - b) ** 2))


def gd(true_front, population):
    """calculate_gd (:184-198): (value, bound)."""
    population, true_front = np.asarray(population, np.float64), np.asarray(true_front, np.float64)
    n, D = len(population), population.shape[1] if population.ndim == 2 else 0
    if n == 0:
        return np.nan, 0.0
    total = sum(min([_d2(p, t) for t in true_front], default=np.inf) for p in population)
    value = np.sqrt(total) / n
    # the sum has n terms, each a squared distance of D terms; sqrt and the division add one rounding each: the
    # relative error of the result is within (n + D + 3) * 2^-53 (all terms are non-negative, so mag is the value)
    return value, (n + D + 3) * EPS * abs(value)


def igd(true_front, population):
    """calculate_igd (:168-182): (value, bound)."""
    population, true_front = np.asarray(population, np.float64), np.asarray(true_front, np.float64)
    n, D = len(true_front), true_front.shape[1] if true_front.ndim == 2 else 0
    if n == 0:
        return np.nan, 0.0
    value = sum(min([np.sqrt(_d2(t, p)) for p in population], default=np.inf) for t in true_front) / n
    return value, (n + D + 3) * EPS * abs(value)


def spread(population, true_front):
    """calculate_spread (:200-227): (value, bound); NaN for fewer than two points or an empty true front."""
    population, true_front = np.asarray(population, np.float64), np.asarray(true_front, np.float64)
    n = len(population)
    if n < 2 or len(true_front) == 0:
        return np.nan, 0.0
    D = population.shape[1]
    diaa = np.array([min([d for d in (np.sqrt(_d2(p, q)) for q in population) if d != 0.0], default=np.inf) for p in population])
    daa = diaa.sum() / n
    ends = sum(np.sqrt(_d2(population[np.argmin(population[:, i])], true_front[np.argmin(true_front[:, i])])) for i in range(D))
    dev = np.abs(diaa - daa).sum()
    value = (ends + dev) / (ends + n * daa)
    # numerator and denominator are sums of n + D non-negative terms, each a distance (D + 2 roundings) or a deviation
    # from the mean (n + D + 3 roundings relative to the distances' magnitude daa): mag is the ratio taken with the
    # deviations replaced by their magnitude bound, |d_a| + daa
    K = 2 * (n + D) + n + D + 3
    mag = (ends + diaa.sum() + n * daa) / (ends + n * daa)
    return value, K * EPS * mag


def capped(full, cap):
    """What select(obj, valid, cap) returns, from select(obj, valid)'s result: the first cap columns of index."""
    index, count, mask = full
    return np.ascontiguousarray(index[:, :cap]), count, mask


def golden_sets():
    """One dict per recorded set: points [C, D], other [B, D], front [F, D], true_front [T, D], normalised [F, D], gd, igd,
    spread."""
    g = np.load(GOLDEN)
    sets, at = [], dict(points=0, other=0, front=0, true_front=0, normalised=0)

    def take(key, rows, D):
        a = g[key][at[key]:at[key] + rows * D].astype(np.float64).reshape(rows, D)
        at[key] += rows * D
        return a

    for (C, D, rng, seed, B, F, T), m in zip(g["meta"], g["metrics"]):
        sets.append(dict(C=int(C), D=int(D), range=int(rng), seed=int(seed), points=take("points", C, D), other=take("other", B, D),
                         front=take("front", F, D), true_front=take("true_front", T, D), normalised=take("normalised", F, D),
                         gd=m[0], igd=m[1], spread=m[2]))
    assert all(at[k] == g[k].size for k in at)
    return sets
