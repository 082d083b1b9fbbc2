"""CPU: the instrumented f64 restatement of the fluid-LP simplex (tests/lp_reference.py) against the host solver
(csrc/fjsp_lp.cpp through instances.fluid_lp) and against scipy/HiGHS, on every fixture instance that has an LP and on the
generated cases of tests/lp_cases.py; the coverage of the device simplex's branches those cases must keep; and the sweep
behind "no admissible batch reaches the 128-row refusal of csrc/fjsp_lp_device.hip".  No GPU is needed: what the
device file branches on is evaluated with its own expressions on the CPU (tests/lp_reference.py cites the lines).

Ratio-test classes.  A pivot of the device simplex either finds one row at the smallest ratio ("single"), breaks the tie by
sign signatures ("signature"), walks columns and decides by quotients ("magnitude"), or -- near-ties with different
ratios, `bad` -- leaves it to the sequential scan ("scan").  The committed cases take every one of these, each at 4 or more
chunks as well.  Two branches are NOT reached by any LP found, and stay untested on the device: the `small` underflow
guard (a nonzero slack entry below 1e-280 in magnitude) and, with it, a per-column walk that ends on signs alone ("sign":
with exact signs the walk only starts when the signatures left several rows with the same nonzero sign, so it always
divides).  The search of tests/lp_cases.py (seeds 0 ... 99 999, three states each) met neither; its counts are in
lp_cases.SEARCH_RESULT.
"""
import numpy as np

from tests import helpers as H
from tests import lp_cases as LC
from tests import lp_reference as LR


def _fixture_cases():
    """Every fixture instance with an LP: the mo_dfjsp and multiorder suites (data/industrial, data/HMPSAC and generated
    instances, tableaus up to 113 x 538), mk01, multijob and six of synth10x5 -- each with its reset-time state, a state
    with jobs at later stages and one with jobs spread over all stages."""
    out = []
    rs = np.random.RandomState(23)
    for suite, first in (("mo_dfjsp", None), ("multiorder", None), ("mk01", None), ("multijob", None), ("synth10x5", 6)):
        for a in H.load_suite(suite)[0][:first]:
            koff = np.concatenate(([0], np.cumsum(a.Jr)))
            Q0 = np.repeat(a.count[0], a.Jr).astype(np.int32)
            now0 = np.array([a.count[0][r] if j == 0 else 0 for r in range(a.R) for j in range(a.Jr[r])], np.int32)
            states = [("reset", Q0, now0)]
            now = now0.copy()
            for r in range(a.R):
                now[koff[r] + rs.randint(0, a.Jr[r])] += 1
            states.append(("mid", Q0.copy(), now))
            st = [rs.randint(0, a.Jr[r], int(rs.randint(1, 25))) for r in range(a.R)]
            states.append(("spread",) + LC.state_from_stages(a, st))
            out.append(("%s/%s" % (suite, a.name), a, states))
    return out


def _check_against_host(label, a, states):
    """x and objective bit for bit, and the clean-split claim on every pivot.  Returns the per-LP records."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    recs = []
    for name, Q, now in states:
        want, want_obj = fi.fluid_lp(a.Jr, a.p, Q, now)
        x, obj, rec = LR.fluid_lp_reference(a.Jr, a.p, Q, now)
        what = "%s state %s" % (label, name)
        assert np.array_equal(H.bits(x), H.bits(want)), what
        assert H.bits(obj) == H.bits(want_obj), what
        assert rec and (rec[0]["nr"], rec[0]["nc"]) == LR.tableau_shape(a.Jr, a.p, now)[:2], what
        for pv in rec:
            # csrc/fjsp_lp_simplex.h:213-222 (lp_leaving_row): on a clean split the first lexicographic minimum among the rows exactly at the
            # smallest ratio IS the row the sequential scan ends on
            if pv["nr"] <= 128 and not pv["bad"]:
                assert pv["lex_row"] == pv["r"], "%s pivot %d: narrowing gives row %r, the scan row %d" % (what, pv["it"], pv["lex_row"], pv["r"])
            else:
                assert pv["lex_row"] is None and pv["decided"] == "scan"
        recs.append(rec)
    return recs


def test_restatement_equals_the_host_solver_on_every_fixture_lp(built):
    cases = _fixture_cases()
    assert len(cases) >= 20
    shapes = set()
    for label, a, states in cases:
        for rec in _check_against_host(label, a, states):
            shapes.add((rec[0]["nr"], rec[0]["nc"]))
    assert (79, 137) in shapes and (113, 538) in shapes      # data/industrial; data/HMPSAC M15_S3 (too wide for the device)


def test_restatement_equals_the_host_solver_on_the_generated_cases(built):
    for c in LC.cases():
        _check_against_host(c.name, c.arr, c.states)


def test_host_solver_is_optimal_and_feasible_on_the_generated_cases(built):
    """The thresholds of test_host.py::test_fluid_lp_is_optimal_and_deterministic: 1e-9 on the relative objective gap to
    the independent HiGHS optimum and on feasibility."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    for c in LC.cases():
        a = c.arr
        for name, Q, now in c.states:
            x, obj = fi.fluid_lp(a.Jr, a.p, Q, now)
            best, A, b, idx = LR.lp_highs(a, Q, now)
            assert abs(best - obj) <= 1e-9 * max(1.0, abs(best)), (c.name, name, best, obj)
            v = np.zeros(A.shape[1]); v[-1] = obj
            for (k, m), i in idx.items():
                v[i] = x[k, m]
            assert (A @ v - b).max() < 1e-9 and x.min() >= 0.0 and x.max() <= 1.0, (c.name, name)
            assert (x[a.p == 0] == 0).all()


def test_generated_cases_keep_their_coverage(built):
    """What the generated cases exist for, counted by the restatement: a change to the generator cannot quietly lose a
    class.  (Where a requirement cannot be met by ANY admissible LP the reason is stated instead.)"""
    cases = LC.cases()
    pivots = []
    for c in cases:
        a = c.arr
        assert LC.fits_device([a]), c.name                               # the worst-case tableau passes the create rule
        for name, Q, now in c.states:
            _, _, rec = LR.fluid_lp_reference(a.Jr, a.p, Q, now)
            nr, nc = LR.tableau_shape(a.Jr, a.p, now)[:2]
            assert nr * nc * 8 <= LC.LDS_LIMIT and nc <= LC.MAX_COLUMNS
            pivots += [dict(pv, case=c.name, state=name) for pv in rec]
    count = lambda f: sum(1 for pv in pivots if f(pv))
    # every compiled pivot loop at the ACTUAL width of a solved LP: chunk counts 2, 3, 4, 6 and 8 (and 7: lp_pivots<8>)
    for nt in (2, 3, 4, 6, 7, 8):
        assert count(lambda pv: pv["nt"] == nt) >= 100, nt
    # rows: up to 64, and 65-128 at four chunks, with leaving rows in both halves there
    assert count(lambda pv: pv["nr"] <= 64) > 0
    assert count(lambda pv: pv["nr"] > 64 and pv["nt"] == 4 and pv["half"] == 0) >= 20
    assert count(lambda pv: pv["nr"] > 64 and pv["nt"] == 4 and pv["half"] == 1) >= 20
    # the leaving row chosen from the second half while no row of the first half is at the minimum, and against tied rows of
    # the first half
    assert count(lambda pv: pv["half"] == 1 and pv["tied_lo"] == 0) >= 5
    assert count(lambda pv: pv["half"] == 1 and pv["tied_lo"] > 0) >= 5
    # the entering column (and the lane fz is read from) in the last chunk.  x and t columns end at nx = nc - nr - 2, and the
    # last chunk starts at 64 (nt - 1) >= nc - 64: with more than 62 rows only slack columns lie there, and at 8 chunks
    # nx >= 448 needs K M >= 448, so nr >= K + M >= 43 and nr nc 8 >= 43 * 493 * 8 B, beyond the 156 KB of the create rule --
    # there the highest chunk an x or t column can have is the last but one.
    for nt, chunk in ((4, 3), (6, 5), (7, 6), (8, 6)):
        assert count(lambda pv: pv["nt"] == nt and pv["s_chunk"] == chunk) > 0, (nt, chunk)
    # degenerate sizes
    dims = set((c.arr.R, c.arr.K, c.arr.M) for c in cases)
    assert (1, 1, 1) in dims and any(M == 1 and K > 1 for _, K, M in dims) and any(K == 1 and M > 1 for _, K, M in dims)
    # number ranges: job counts of the training distribution and up to 65 535; processing times 1 and 65 535 in one machine row
    qmax = [int(Q.max()) for c in cases for _, Q, _ in c.states]
    assert max(qmax) == 65535 and sum(1 for q in qmax if 100 <= q <= 600) >= 8
    assert any(((c.arr.p == 1).any(0) & (c.arr.p == 65535).any(0)).any() for c in cases)
    # states: precedence rows present, partly present, absent
    for c in cases:
        if c.arr.K > c.arr.R and len(c.states) >= 4:        # (the search's cases keep their three searched states)
            nprec = [LR.tableau_shape(c.arr.Jr, c.arr.p, now)[3] for _, _, now in c.states]
            assert max(nprec) == c.arr.K - c.arr.R and min(nprec) == 0, c.name
    # ratio-test classes: every class the search found at all, and each of them at more than four chunks too
    for cls, n in LC.SEARCH_RESULT.items():
        if cls != "pivots" and n > 0:
            assert LC.SEARCH_SEEDS.get(cls), cls
    assert count(lambda pv: pv["decided"] == "magnitude") >= 3 and count(lambda pv: pv["decided"] == "magnitude" and pv["nt"] > 4) >= 1
    assert count(lambda pv: pv["bad"]) >= 5 and count(lambda pv: pv["bad"] and pv["nt"] > 4) >= 1
    assert count(lambda pv: pv["decided"] == "signature" and pv["steps"] >= 2) >= 20
    for cls, seeds in LC.SEARCH_SEEDS.items():
        for seed in seeds:
            assert count(lambda pv: pv["case"] == "s%d" % seed and (pv["bad"] if cls == "bad" else pv["decided"] == cls)) > 0, (cls, seed)
    # never found (module docstring): the device's `small` guard and the sign-only end of a column walk
    assert LC.SEARCH_RESULT["small"] == 0 and LC.SEARCH_RESULT["sign"] == 0
    assert count(lambda pv: pv["small"]) == 0 and count(lambda pv: pv["decided"] == "sign") == 0


def test_no_admissible_device_tableau_has_more_than_128_rows():
    """csrc/fjsp_lp_device.hip holds two row groups of 64 in a lane and refuses an LP of more than 128 rows (error code 5,
    before any tableau write).  Creation admits K <= 256 operation types, M <= 32 machines, 1 <= R <= K kinds of at most 255
    operations (254 in a batch with order arrivals, the only batches that pose LPs on the device; the sweep below keeps the
    wider 255) and K <= nx <= K M eligible pairs (csrc/fjsp_env.hip check_instance, csrc/fjsp_instance.cpp), and puts the
    LPs on the device only when lp_device_lds_bytes(K, M, nx, R, MP >= M) <= 156 KB and the tableau has at most 512
    columns (choose_lp_service).  The worst-case tableau has nr = K + M + (K - R) rows.  Over every such shape: none with
    nr > 128 is admitted, so no batch reaches that refusal.  (nr >= 129 needs K >= 49, hence nc >= K + nr + 2 >= 180 and
    129 * 180 * 8 = 185 760 B of tableau alone.)"""
    # lp_device_lds_bytes (csrc/fjsp_lp_limits.h) by hand for K 2, M 1, nx 2, R 1: 4 rows x 8 columns
    assert LC.lds_bytes(2, 1, 2, 1, 1) == (4 * 8 * 8 + 8 * 8 + 2 * 4 * 8 + 4 * 4 + 2 * 1 * 2 + 2 * 2 + 4 * 2 + 2 * 1 * 2 + 2 * 8 + 128 + 15) // 16 * 16 == 576
    largest, widest, checked = 0, 0, 0
    for K in range(1, 257):
        M = np.arange(1, 33)[:, None, None]
        R = np.arange(max(1, -(-K // 255)), K + 1)[None, :, None]
        nx = np.arange(K, min(K * 32, LC.MAX_COLUMNS) + 1)[None, None, :]      # (beyond 512 pairs the tableau is wider than 512 columns)
        nr = K + M + (K - R)
        nc = nx + 1 + nr + 1
        admitted = (nx <= K * M) & (LC.lds_bytes(K, M, nx, R, M) <= LC.LDS_LIMIT) & (nc <= LC.MAX_COLUMNS)
        checked += int((nx <= K * M).sum()) * R.size
        assert not (admitted & (nr > 128)).any(), "K %d: an admitted shape with more than 128 rows" % K
        if admitted.any():
            largest = max(largest, int(np.where(admitted, nr, 0).max()))
            widest = max(widest, int(np.where(admitted, nc, 0).max()))
    assert checked > 10 ** 7
    assert 100 <= largest <= 128        # (the rule does admit tableaus that use both halves: 116 rows at the most)
    assert 449 <= widest < 512          # (and 8-chunk tableaus, 463 columns at the most: the 512-column limit never binds)
