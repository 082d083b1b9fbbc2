"""Instrumented float64 restatement of the fluid-LP simplex (numpy, CPU).

`fluid_lp_reference(Jr, p, Q, n_now)` takes the inputs of `instances.fluid_lp` and follows csrc/fjsp_lp.cpp operation for
operation: the same tableau (rows: operation types, machines, precedence constraints; columns: eligible (m, k) pairs in
(m, k) order, t, the slacks, the right-hand side), the same Dantzig rule (the first smallest reduced cost below -1e-9),
the same sequential lexicographic ratio scan with its tolerances, the same elimination -- one rounding for the product and
one for the difference (numpy evaluates `a - f * b` through a temporary: no FMA) --, the same clean-up of a tiny negative
right-hand side and the same extraction of x.  Its x and objective must therefore equal the host solver's BIT FOR BIT
(tests/test_lp_reference.py); it is a second, independently written statement of the solver, not a tolerance oracle.

What it adds is a record per pivot that classifies the pivot the way csrc/fjsp_lp_simplex.h BRANCHES on it.  The device
file chooses the leaving row without the scan wherever it can (lp_leaving_row, "lexicographic ratio test"); `_device_ratio_test`
below evaluates that choice with the device file's own expressions (the line numbers cited are those of
csrc/fjsp_lp_simplex.h; lp_pivots is csrc/fjsp_lp_device.hip's) and reports

    nt         chunks of 64 columns, ceil(nc / 64): which lp_pivots<NT> runs (2, 3, 4, 6 or 8; lp_device_kernel)
    nr, nc     rows and columns of the solved tableau
    s, s_chunk the entering column and its chunk (the lane and register fz is read from, lp_pivots)
    r, half    the leaving row and its half: 0 = rows 0-63 (row group 0), 1 = rows 64-127 (row group 1; :351-357)
    n_elig     rows with a > 1e-9 (:238)
    n_tied     rows whose ratio equals the smallest exactly (k[g], :253), tied_lo / tied_hi of them per half
    bad        some eligible row is neither exactly at the minimum nor beyond the scan's tolerance from it (:254-255):
               the device falls back to the sequential scan (:361-395)
    steps      16-column tie-break steps taken (:259)
    decided    how the race among the tied rows ended:
                 "single"     one row at the minimum, nothing to break
                 "signature"  by sign signatures alone (:281-303)
                 "sign"       the per-column walk ran and was settled by a lone negative entry or the zeros of a column
                              (:317-340) without a division
                 "magnitude"  at least one column was decided by quotients (:342-348)
                 "scan"       bad, or more than 128 rows: no order-independent choice was made
    n_sign, n_div   columns of the per-column walk settled by signs / by a division
    small      the underflow guard fired in some step (:276, exact_signs false)
    lex_row    the row the order-independent narrowing ends on (None for "scan").  The device file's central claim is
               lex_row == r, the sequential scan's row, on every pivot with a clean split.
"""
import numpy as np

EPS_COST = 1e-9     # csrc/fjsp_lp.cpp kEpsCost
EPS_PIV = 1e-9      # kEpsPiv
EPS_ZERO = 1e-11    # kEpsZero
LEX_COLS = 16       # csrc/fjsp_lp_simplex.h kLexCols
INF = float("inf")


class LpFailure(Exception):
    """The solver refuses the LP (the messages are csrc/fjsp_lp.cpp's)."""


def tableau_shape(Jr, p, n_now):
    """(nr, nc, nx, nprec) of the LP of a live state: nr = K + M + nprec, nc = nx + 1 + nr + 1 (fjsp_lp.cpp:64-65)."""
    Jr = np.asarray(Jr, np.int64)
    K = int(Jr.sum())
    p = np.asarray(p).reshape(K, -1)
    M = p.shape[1]
    koff = np.concatenate(([0], np.cumsum(Jr)))
    nprec = sum(1 for r in range(len(Jr)) for j in range(int(Jr[r]) - 1) if n_now[koff[r] + j + 1] == 0)
    nx = int((p > 0).sum())
    nr = K + M + nprec
    return nr, nx + 1 + nr + 1, nx, nprec


def _sequential_scan(T, s, nv, nr, rhs):
    """fjsp_lp.cpp:110-126, row by row.  Returns the leaving row (-1: unbounded)."""
    col = T[:, s]
    r = -1
    for i in np.nonzero(col > EPS_PIV)[0]:
        i = int(i)
        if r < 0:
            r = i
            continue
        a, ar = col[i], col[r]
        vi, vr = T[i, rhs] / a, T[r, rhs] / ar
        tol = 1e-12 * (abs(vr) if abs(vr) > 1.0 else 1.0)
        if vi < vr - tol:
            r = i
            continue
        if vi > vr + tol:
            continue
        wi, wr = T[i, nv:nv + nr] / a, T[r, nv:nv + nr] / ar
        ne = np.nonzero(wi != wr)[0]
        if ne.size and wi[ne[0]] < wr[ne[0]]:
            r = i
    return r


def _device_ratio_test(T, s, nv, nr, rhs):
    """The leaving row as csrc/fjsp_lp_simplex.h:225-360 (lp_leaving_row, two row groups) derives it, rows as array entries instead of lanes."""
    out = dict(n_elig=0, n_tied=0, tied_lo=0, tied_hi=0, bad=False, steps=0, decided="scan", n_sign=0, n_div=0,
               small=False, lex_row=None)
    a = T[:, s].copy()
    el = a > EPS_PIV                                                                  # :238
    out["n_elig"] = int(el.sum())
    if nr > 128 or not el.any():                                                     # lp_device_kernel's refusal, :242
        return out
    v = np.zeros(nr)
    v[el] = T[el, rhs] / a[el]                                                        # :239
    vmin = v[el].min()                                                                # :243-247
    tolmin = 1e-12 * (abs(vmin) if abs(vmin) > 1.0 else 1.0)                          # :209, :247
    hi = vmin + tolmin
    tied = el & (v == vmin)                                                           # :253
    tol = 1e-12 * np.where(np.abs(v) > 1.0, np.abs(v), 1.0)                           # :209
    far = (v > hi) & (vmin < v - tol)                                                 # :254
    out["n_tied"], out["tied_lo"], out["tied_hi"] = int(tied.sum()), int(tied[:64].sum()), int(tied[64:].sum())
    if (el & ~tied & ~far).any():                                                     # :255
        out["bad"] = True
        return out
    k = tied.copy()
    cnt = int(k.sum())
    cend = nv + nr
    c = nv
    while c < cend and cnt > 1:                                                       # :259
        out["steps"] += 1
        t = np.zeros((nr, LEX_COLS))
        w = min(LEX_COLS, cend - c)
        t[k, :w] = T[k, c:c + w]                                                      # :272
        small = bool(((t != 0.0) & ~(np.abs(t) >= 1e-280)).any())                     # :276
        out["small"] = out["small"] or small
        exact_signs = not small                                                       # :281
        if exact_signs:
            code = (t == 0.0).astype(np.uint64) + 2 * (t > 0.0).astype(np.uint64)     # :277
            sig = np.zeros(nr, np.uint64)
            for u in range(LEX_COLS):
                sig = (sig << np.uint64(2)) | code[:, u]
            sig[~k] = 0xFFFFFFFF                                                      # :267, :279
            smin = int(sig.min())                                                     # :283-286
            d = smin ^ 0x55555555                                                     # :287
            keep = (~((1 << (2 * ((d.bit_length() - 1) >> 1))) - 1)) & 0xFFFFFFFF if d else 0xFFFFFFFF   # :289
            pk = k & (((sig ^ np.uint64(smin)) & np.uint64(keep)) == 0)               # :294
            npk = int(pk.sum())
            if d == 0 or npk == 1:                                                    # :297
                k, cnt = pk, npk
                c += LEX_COLS
                continue
        for u in range(LEX_COLS):                                                     # :305
            if c + u >= cend or cnt <= 1:
                break
            x = t[:, u]
            sel = k.copy()                                                            # :312
            if exact_signs:
                g = k & (x < 0.0)                                                     # :319
                nn = int(g.sum())
                if nn == 1:                                                           # :320
                    k, cnt = g, 1
                    out["n_sign"] += 1
                    continue
                if nn == 0:
                    z = k & (x == 0.0)                                                # :330
                    nz = int(z.sum())
                    if nz > 0:                                                        # :331
                        k, cnt = z, nz
                        out["n_sign"] += 1
                        continue
                else:
                    sel = g                                                           # :339
            wq = np.full(nr, INF)
            wq[sel] = x[sel] / a[sel]                                                 # :344
            wm = wq.min()                                                             # :345
            k = sel & (wq == wm)                                                      # :348
            cnt = int(k.sum())
            out["n_div"] += 1
        c += LEX_COLS
    if k.any():                                                                       # :351-357: row group 0 before 1, lowest lane first
        out["lex_row"] = int(np.nonzero(k)[0][0])
        out["decided"] = ("magnitude" if out["n_div"] else "sign" if out["n_sign"] else
                          "signature" if out["steps"] else "single")
    return out


def fluid_lp_reference(Jr, p, Q, n_now):
    """x[K, M], objective, per-pivot record (a list of dicts, see the module docstring).  The line numbers cited in this
    function are those of csrc/fjsp_lp.cpp."""
    Jr = np.asarray(Jr, np.int64)
    R = len(Jr)
    K = int(Jr.sum())
    p = np.asarray(p, np.int64).reshape(K, -1)
    M = p.shape[1]
    Q = np.asarray(Q, np.int64)
    n_now = np.asarray(n_now, np.int64)
    koff = np.concatenate(([0], np.cumsum(Jr)))
    col_of = -np.ones((K, M), np.int64)                    # columns: eligible (m, k) pairs sorted by (m, k), then t (:50-58)
    nx = 0
    for m in range(M):
        for k in range(K):
            if p[k, m] > 0:
                col_of[k, m] = nx
                nx += 1
    tcol, nv = nx, nx + 1
    prec = [int(koff[r]) + j for r in range(R) for j in range(int(Jr[r]) - 1) if n_now[koff[r] + j + 1] == 0]   # :60-63
    nr = K + M + len(prec)
    nc = nv + nr + 1
    rhs = nc - 1
    T = np.zeros((nr, nc))
    z = np.zeros(nc)
    basis = np.zeros(nr, np.int64)
    for k in range(K):                                                                # :70-82
        if Q[k] <= 0:
            raise LpFailure("fluid LP: Q[k] <= 0")
        if not (p[k] > 0).any():
            raise LpFailure("fluid LP: operation type without eligible machine")
        for m in range(M):
            if p[k, m] > 0:
                rate = 1.0 / float(p[k, m])
                T[k, col_of[k, m]] = -(rate / float(Q[k]))
        T[k, tcol] = 1.0
    for m in range(M):                                                                # :83-89
        for k in range(K):
            if p[k, m] > 0:
                T[K + m, col_of[k, m]] = 1.0
        T[K + m, rhs] = 1.0
    for q, k in enumerate(prec):                                                      # :90-97
        row = K + M + q
        for m in range(M):
            if p[k + 1, m] > 0:
                T[row, col_of[k + 1, m]] += 1.0 / float(p[k + 1, m])
            if p[k, m] > 0:
                T[row, col_of[k, m]] -= 1.0 / float(p[k, m])
    for i in range(nr):                                                               # :98
        T[i, nv + i] = 1.0
        basis[i] = nv + i
    z[tcol] = -1.0
    record = []
    max_iter = 200 * (nr + nc) + 1000
    it = 0
    while True:
        if it > max_iter:
            raise LpFailure("fluid LP: iteration limit")
        zz = z[:nc - 1]                                                               # :104-108
        s = int(np.argmin(zz))
        if not (zz[s] < -EPS_COST):
            break
        cls = _device_ratio_test(T, s, nv, nr, rhs)
        r = _sequential_scan(T, s, nv, nr, rhs)
        if r < 0:
            raise LpFailure("fluid LP: unbounded")
        cls.update(it=it, s=s, s_chunk=s >> 6, r=r, half=r >> 6, nr=nr, nc=nc, nt=(nc + 63) >> 6)
        record.append(cls)
        piv = T[r, s]                                                                 # :129-141
        rowr = T[r] / piv
        rowr[s] = 1.0
        T[r] = rowr
        f = T[:, s].copy()
        f[r] = 0.0
        rows = np.nonzero(f != 0.0)[0]
        if rows.size:
            prod = f[rows, None] * rowr[None, :]
            T[rows] = T[rows] - prod
            T[rows, s] = 0.0
            b = T[rows, rhs]
            T[rows[(b < 0.0) & (b > -1e-12)], rhs] = 0.0
        fz = z[s]                                                                     # :142-146
        if fz != 0.0:
            prod = fz * rowr
            z = z - prod
            z[s] = 0.0
        basis[r] = s
        it += 1
    val = np.zeros(nv)                                                                # :149-162
    for i in range(nr):
        if basis[i] < nv:
            val[basis[i]] = T[i, rhs]
    x = np.zeros((K, M))
    for k in range(K):
        for m in range(M):
            if col_of[k, m] >= 0:
                v = val[col_of[k, m]]
                if v < EPS_ZERO:
                    v = 0.0
                if v > 1.0:
                    v = 1.0
                x[k, m] = v
    for k in range(K):                                                                # :164-169
        sacc = 0.0
        for m in range(M):
            if p[k, m] > 0:
                sacc += x[k, m] / float(p[k, m])
        if not sacc > 0.0:
            raise LpFailure("fluid LP: zero rate for an operation type")
    return x, float(val[tcol]), record


def lp_highs(a, Q, now):
    """Independent formulation of class_FJSSP.py:246-280 solved by scipy/HiGHS: (optimum, A, b, column index of (k, m))."""
    from scipy.optimize import linprog
    K, M = a.p.shape
    cols = [(k, m) for k in range(K) for m in range(M) if a.p[k, m] > 0]
    idx = {km: i for i, km in enumerate(cols)}
    n = len(cols) + 1
    A, b = [], []
    for k in range(K):
        row = np.zeros(n); row[-1] = 1.0
        for m in range(M):
            if a.p[k, m] > 0:
                row[idx[(k, m)]] = -(1.0 / a.p[k, m]) / Q[k]
        A.append(row); b.append(0.0)
    for m in range(M):
        row = np.zeros(n)
        for k in range(K):
            if a.p[k, m] > 0:
                row[idx[(k, m)]] = 1.0
        A.append(row); b.append(1.0)
    koff = np.concatenate(([0], np.cumsum(a.Jr)))
    for r in range(len(a.Jr)):
        for j in range(int(a.Jr[r]) - 1):
            k = int(koff[r]) + j
            if now[k + 1] == 0:
                row = np.zeros(n)
                for m in range(M):
                    if a.p[k + 1, m] > 0:
                        row[idx[(k + 1, m)]] += 1.0 / a.p[k + 1, m]
                    if a.p[k, m] > 0:
                        row[idx[(k, m)]] -= 1.0 / a.p[k, m]
                A.append(row); b.append(0.0)
    c = np.zeros(n); c[-1] = -1.0
    res = linprog(c, A_ub=np.array(A), b_ub=np.array(b), bounds=[(0, 1)] * len(cols) + [(None, None)], method="highs")
    assert res.status == 0
    return -res.fun, np.array(A), np.array(b), idx
