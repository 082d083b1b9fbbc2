"""A numpy restatement of fjsp_beam_select (include/fjsp_amd.h): per source env, the width_out best of the width_in x
n_actions candidates in ascending (cost, parent, action)."""
import numpy as np


def beam_select(cost, done, width_out):
    """cost f64[W, N, A], done u8[W, N] or None -> (parent i32, action i32, cost f64), each [width_out, N]."""
    cost = np.asarray(cost, np.float64)
    W, N, A = cost.shape
    done = np.zeros((W, N), bool) if done is None else np.asarray(done).reshape(W, N) != 0
    parent = np.full((width_out, N), -1, np.int32)
    action = np.full((width_out, N), -1, np.int32)
    out = np.full((width_out, N), np.inf, np.float64)
    for i in range(N):
        b, a = [x.reshape(-1) for x in np.meshgrid(np.arange(W), np.arange(A), indexing="ij")]      # flattened candidates
        c = cost[:, i, :].reshape(-1)
        # a done beam collapses to its single candidate (b, -1) at cost[b, i, 0]
        keep = ~done[b, i] | (a == 0)
        a = np.where(done[b, i], -1, a)
        with np.errstate(invalid="ignore"):
            keep &= c < np.inf                   # drops NaN and +inf
        b, a, c = b[keep], a[keep], c[keep]
        key = np.where(c == 0.0, 0.0, c)         # -0.0 and 0.0 are one cost
        order = np.lexsort((a, b, key))[:width_out]
        n = order.size
        parent[:n, i], action[:n, i], out[:n, i] = b[order], a[order], c[order]
    return parent, action, out
