"""CPU: what the device simplex with its tableau in global memory (csrc/fjsp_lp_global.hip) rests on beyond the LDS kernel.

Order-independent row choice at any row count.  csrc/fjsp_lp_device.hip holds two row groups per lane and refuses anything
beyond 128 rows; the global-memory kernel holds four (256 rows).  The claim that makes the choice
legal -- on a clean split the sequential scan ends on the first lexicographic minimum among the rows exactly at the smallest
ratio, in row order -- does not depend on the row count.  `_ratio_test_groups` restates the classifier of
tests/lp_reference.py (`_device_ratio_test`) without its `nr > 128` exit and counts the tied rows per group of 64; the
simplex around it is tests/lp_reference.py's own (`fluid_lp_reference`, which also checks nothing by itself: x is compared
with the host solver bit for bit here).  The cases are tests/lp_global_cases.py's; the coverage they must keep is asserted.

Size rule.  fjsp_lp_global_bytes against its restatement on the limit pairs and on every fixture instance beyond the LDS.
"""
import numpy as np
import pytest

from tests import helpers as H
from tests import lp_cases as LC
from tests import lp_global_cases as GC
from tests import lp_reference as LR


def _ratio_test_groups(T, s, nv, nr, rhs):
    """tests/lp_reference.py `_device_ratio_test` for up to four row groups: the same expressions, no `nr > 128` exit
    (csrc/fjsp_lp_simplex.h lp_leaving_row<4>, "lexicographic ratio test")."""
    out = dict(n_elig=0, n_tied=0, tied_lo=0, tied_hi=0, tied_group=[0, 0, 0, 0], bad=False, steps=0, decided="scan",
               n_sign=0, n_div=0, small=False, lex_row=None)
    assert nr <= 256
    a = T[:, s].copy()
    el = a > LR.EPS_PIV
    out["n_elig"] = int(el.sum())
    if not el.any():
        return out
    v = np.zeros(nr)
    v[el] = T[el, rhs] / a[el]
    vmin = v[el].min()
    tolmin = 1e-12 * (abs(vmin) if abs(vmin) > 1.0 else 1.0)
    hi = vmin + tolmin
    tied = el & (v == vmin)
    tol = 1e-12 * np.where(np.abs(v) > 1.0, np.abs(v), 1.0)
    far = (v > hi) & (vmin < v - tol)
    out["n_tied"], out["tied_lo"], out["tied_hi"] = int(tied.sum()), int(tied[:64].sum()), int(tied[64:].sum())
    out["tied_group"] = [int(tied[64 * g:64 * g + 64].sum()) for g in range(4)]
    if (el & ~tied & ~far).any():
        out["bad"] = True
        return out
    k = tied.copy()
    cnt = int(k.sum())
    cend = nv + nr
    c = nv
    while c < cend and cnt > 1:
        out["steps"] += 1
        t = np.zeros((nr, LR.LEX_COLS))
        w = min(LR.LEX_COLS, cend - c)
        t[k, :w] = T[k, c:c + w]
        small = bool(((t != 0.0) & ~(np.abs(t) >= 1e-280)).any())
        out["small"] = out["small"] or small
        exact_signs = not small
        if exact_signs:
            code = (t == 0.0).astype(np.uint64) + 2 * (t > 0.0).astype(np.uint64)
            sig = np.zeros(nr, np.uint64)
            for u in range(LR.LEX_COLS):
                sig = (sig << np.uint64(2)) | code[:, u]
            sig[~k] = 0xFFFFFFFF
            smin = int(sig.min())
            d = smin ^ 0x55555555
            keep = (~((1 << (2 * ((d.bit_length() - 1) >> 1))) - 1)) & 0xFFFFFFFF if d else 0xFFFFFFFF
            pk = k & (((sig ^ np.uint64(smin)) & np.uint64(keep)) == 0)
            npk = int(pk.sum())
            if d == 0 or npk == 1:
                k, cnt = pk, npk
                c += LR.LEX_COLS
                continue
        for u in range(LR.LEX_COLS):
            if c + u >= cend or cnt <= 1:
                break
            x = t[:, u]
            sel = k.copy()
            if exact_signs:
                g = k & (x < 0.0)
                nn = int(g.sum())
                if nn == 1:
                    k, cnt = g, 1
                    out["n_sign"] += 1
                    continue
                if nn == 0:
                    z = k & (x == 0.0)
                    nz = int(z.sum())
                    if nz > 0:
                        k, cnt = z, nz
                        out["n_sign"] += 1
                        continue
                else:
                    sel = g
            wq = np.full(nr, LR.INF)
            wq[sel] = x[sel] / a[sel]
            wm = wq.min()
            k = sel & (wq == wm)
            cnt = int(k.sum())
            out["n_div"] += 1
        c += LR.LEX_COLS
    if k.any():                                                   # groups in order, lowest lane first: the first row
        out["lex_row"] = int(np.nonzero(k)[0][0])
        out["decided"] = ("magnitude" if out["n_div"] else "sign" if out["n_sign"] else
                          "signature" if out["steps"] else "single")
    return out


@pytest.fixture(scope="module")
def records(built):
    """{(case, state): per-pivot records} of every case and state, classified for four row groups; x checked against the
    host solver on the way.  Computed once for the tests below."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    saved = LR._device_ratio_test
    LR._device_ratio_test = _ratio_test_groups                    # (fluid_lp_reference looks the classifier up at call time)
    try:
        out = {}
        for c in GC.cases():
            a = c.arr
            assert not LC.fits_device([a]) and GC.within_global(a), c.name
            for name, Q, now in c.states:
                x, obj, rec = LR.fluid_lp_reference(a.Jr, a.p, Q, now)
                want, want_obj = fi.fluid_lp(a.Jr, a.p, Q, now)
                assert np.array_equal(H.bits(x), H.bits(want)) and H.bits(obj) == H.bits(want_obj), (c.name, name)
                out[(c.name, name)] = rec
    finally:
        LR._device_ratio_test = saved
    return out


def test_shapes_of_the_generated_cases():
    want = {"g_rows3": (138, 280), "g_rows4": (200, 402), "g_cols9": (56, 538), "g_wide": (128, 1330), "g_both": (138, 536)}
    for c in GC.cases():
        assert GC.shape(c.arr) == want[c.name], c.name
        name, Q, now = c.states[0]
        assert name == "reset" and LR.tableau_shape(c.arr.Jr, c.arr.p, now)[:2] == want[c.name], c.name
    lim = {c.name: (GC.shape(c.arr), ok) for c, ok in GC.limit_cases()}
    assert lim["l_rows256"] == ((256, 508), True) and lim["l_rows257"][0][0] == 257 and not lim["l_rows257"][1]
    assert lim["l_cols1536"] == ((78, 1536), True) and lim["l_cols1537"] == ((78, 1537), False)
    for c, ok in GC.limit_cases():
        assert GC.within_global(c.arr) == ok and not LC.fits_device([c.arr]), c.name


def test_order_independent_row_choice_equals_the_scan_at_any_row_count(records):
    """On every clean-split pivot of every case, the first lexicographic minimum among the exactly tied rows is the row the
    sequential scan ends on -- beyond 128 rows as below."""
    clean = beyond = 0
    for (case, state), rec in records.items():
        for pv in rec:
            if pv["bad"]:
                assert pv["lex_row"] is None and pv["decided"] == "scan"
                continue
            clean += 1
            beyond += pv["r"] >= 128
            assert pv["lex_row"] == pv["r"], "%s state %s pivot %d: narrowing gives row %r, the scan row %d" % (
                case, state, pv["it"], pv["lex_row"], pv["r"])
    assert clean > 1000 and beyond > 50


def test_generated_cases_keep_their_coverage(records):
    """What the kernel's new paths need from the cases: leaving rows in the third and fourth row group, entering columns
    beyond 512 and beyond 1024 (chunks 8 ... 20), ties among rows of the later groups, magnitude ties and bad splits."""
    pivots = [pv for rec in records.values() for pv in rec]
    assert any(128 <= pv["r"] < 192 for pv in pivots)
    assert any(192 <= pv["r"] < 256 for pv in pivots)
    assert any(pv["s"] >= 512 for pv in pivots)
    assert any(pv["s"] >= 1024 for pv in pivots)
    assert any(pv["decided"] == "magnitude" for pv in pivots)         # (every tableau here is beyond the LDS)
    assert any(pv["bad"] for pv in pivots)
    assert any(pv["tied_group"][2] > 0 and pv["n_tied"] > 1 for pv in pivots)
    assert any(pv["tied_group"][3] > 0 and pv["n_tied"] > 1 for pv in pivots)
    assert {pv["decided"] for pv in records[("g_wide", "reset")] + records[("g_wide", "spread0")] + records[("g_wide", "spread1")]
            + records[("g_wide", "noprec")]} >= {"signature", "magnitude", "scan"}
    reset = {c: records[(c, "reset")] for c in ("g_rows3", "g_rows4", "g_wide")}
    assert len(reset["g_rows3"]) == 85 and sum(pv["r"] >= 128 for pv in reset["g_rows3"]) == 12
    assert len(reset["g_rows4"]) == 126 and sum(pv["r"] >= 128 for pv in reset["g_rows4"]) == 85
    assert sum(pv["r"] >= 192 for pv in reset["g_rows4"]) == 9
    assert len(reset["g_wide"]) == 123 and sum(pv["s"] >= 512 for pv in reset["g_wide"]) == 86
    assert sum(pv["s"] >= 1024 for pv in reset["g_wide"]) == 16
    assert {pv["nr"] for s in ("spread0", "spread1") for pv in records[("g_rows4", s)]} <= set(range(138, 141))


def _beyond_lds_fixtures():
    """The fixture instances whose largest tableau does not fit the LDS rule, by name (each once)."""
    out = {}
    for suite in ("mo_dfjsp", "multiorder", "so_dfjsp", "large", "mo_discretes"):
        for a in H.load_suite(suite)[0]:
            if not LC.fits_device([a]):
                out.setdefault(a.name.split("/")[-1], a)
    return out


def test_size_rule(built):
    """fjsp_lp_global_bytes equals its restatement on the four limit cases and on every fixture instance beyond the LDS; Mk06
    (305 x 797) and Mk10 (475 x 1193) are beyond the limits."""
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    lib = _capi.lib()

    def both(a):
        nx = int((a.p > 0).sum())
        got = int(lib.fjsp_lp_global_bytes(a.K, a.M, nx, a.R))
        assert got == GC.global_bytes(a.K, a.M, nx, a.R), a.name
        return got

    for c, ok in GC.limit_cases():
        got = both(c.arr)
        assert (got > 0) == ok, c.name
        if ok:
            nr, nc = GC.shape(c.arr)
            assert nr * nc * 8 <= got < nr * nc * 8 + 256
    fx = _beyond_lds_fixtures()
    want = {"DDT0.5_M10_S1": (91, 328), "DDT1.0_M15_S3": (113, 538), "DDT0.5_M20_S3": (71, 384), "DDT1.0_M15_R10": (133, 673),
            "DDT0.5_M20_R5": (81, 407), "DDT0.5_M10_R5": (87, 310), "DDT1.5_M15_R5": (80, 379), "Mk01": (106, 223), "Mk04": (173, 347)}
    for name, (nr, nc) in want.items():
        assert GC.shape(fx[name]) == (nr, nc), name
        assert nr * nc * 8 <= both(fx[name]) < nr * nc * 8 + 256, name
    assert both(fx["Mk06"]) == 0 and both(fx["Mk10"]) == 0
    for c in GC.cases():
        assert both(c.arr) > 0
    assert int(lib.fjsp_lp_global_bytes(0, 4, 0, 0)) == 0 and int(lib.fjsp_lp_global_bytes(4, 4, 8, 5)) == 0
