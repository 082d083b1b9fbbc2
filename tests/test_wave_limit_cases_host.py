"""What tests/test_gpu_wave_limits.py leans on, proven on the CPU: the C oracle plays every case of
tests/wave_limit_cases.py to its end and the case reaches the condition it exists for, so that a later edit of a builder
cannot silently lose the edge; and the create-time limits on both sides, through fjsp_env_create, which refuses before
any device is touched."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests import wave_limit_cases as WC

E_UNSUPPORTED = -5
# _digest of the 63 cases that were there before the chunk_orders family, computed before it was added
LEGACY_DIGEST = "b426acf99dd8cac207988a416b56caf05e81209febbaf9d83eea3d8f7e1ba771"


@pytest.fixture(scope="module")
def oracle(built):
    from oracle import pyoracle
    pyoracle.lib()
    return pyoracle


def test_case_list_covers_every_family_and_variant():
    ids = WC.case_ids()
    assert len(ids) == len(set(ids)) == 69
    assert {c[0] for c in ids} == {"chunks", "kinds", "stages", "machines", "jobs", "orders", "late", "chunk_orders"}
    assert {c[2] for c in ids} == {0, 1, 2, 4, 5}
    # families added after the first 63 cases go last: actions() seeds a case by its position
    assert [c[0] for c in ids[63:]] == ["chunk_orders"] * 6 and "chunk_orders" not in {c[0] for c in ids[:63]}
    assert WC.N_ENVS % 4 != 0 and WC.FIRST == 2


def _digest(cids):
    """sha256 over the instance arrays (the arguments of set_raw) and the actions of the cases."""
    h = hashlib.sha256()
    for cid in cids:
        c = WC.case(cid)
        for a in c.arrs:
            for key in ("Jr", "p", "elig_n", "elig_list", "count", "arrive", "delivery"):
                x = np.ascontiguousarray(getattr(a, key))
                h.update(("%s %s %s|" % (key, x.dtype, x.shape)).encode())
                h.update(x.tobytes())
        h.update(WC.actions(c).tobytes())
    return h.hexdigest()


def test_a_new_family_leaves_the_older_cases_where_they_were():
    """_build seeds a case by the sorted position of its (family, shape) among the first 63 and actions() by its position in
    case_ids(): a family added in the wrong place would silently re-draw every older case."""
    assert _digest(WC.case_ids()[:63]) == LEGACY_DIGEST


@pytest.mark.parametrize("cid", WC.case_ids(), ids=WC.case_name)
def test_oracle_plays_the_case_into_its_condition(oracle, cid):
    c = WC.case(cid)
    arrs = WC.set_arrays(c)
    acts = WC.actions(c)
    n0, n1 = WC.ACTION_SPACE[c.variant]
    assert acts.shape == (c.T, WC.N_ENVS, 2) and c.T <= WC.MAX_STEPS
    assert len(set(acts[:, :, 0].ravel())) == n0 and len(set(acts[:, :, 1].ravel())) == n1      # the whole action space
    assert set(e % c.n_inst for e in range(WC.N_ENVS)) >= set(c.edge)
    for a in arrs:
        assert (a.p > 0).any(axis=0).all(), a.name                    # every machine has an eligible operation
        assert c.family in ("stages", "orders", "late") or (a.p.max() <= 5 and a.p[a.p > 0].min() >= 1), a.name
    want = WC.replay(c, arrs, acts)
    for e, w in enumerate(want):
        a = arrs[e % c.n_inst]
        assert w["T"] == WC.ops_total(a) and bool(w["done"][-1]), (c.name, e)
        assert np.isfinite(w["state0"]).all() and np.isfinite(w["states"]).all(), (c.name, e)
        if e % c.n_inst in c.edge:
            holds, what = WC.condition(c, e, a, w, acts[:, e])
            assert holds, "%s env %d misses its condition: %s" % (c.name, e, what)


def test_case_shapes_sit_on_the_limits(oracle):
    """The sizes the cases are named for, read back from the product's instance set."""
    for cid in WC.case_ids():
        c = WC.case(cid)
        edge = [c.arrs[i] for i in c.edge]
        if c.family == "chunks":
            assert [a.K for a in c.arrs] == [1, 64, int(c.shape)]
            assert all(1 <= j <= 16 for a in c.arrs for j in a.Jr) and all((a.count == 2).all() for a in c.arrs)
        elif c.family == "kinds":
            # check_instance: single_job needs one order, one job per kind and R <= 255
            assert all(a.R == int(c.shape) and a.S == 1 and (a.count == 1).all() and (a.Jr == 1).all() for a in edge)
        elif c.family == "stages":
            single = c.shape == "so" and c.variant != 4
            assert [int(a.Jr[0]) for a in c.arrs] == list(WC.STAGES_SINGLE if single else WC.STAGES_ARRIVALS)
            assert all(a.S == (2 if c.shape == "two" else 1) and list(a.Jr[1:]) == [1] for a in c.arrs)
        elif c.family == "machines":
            a = edge[0]
            assert a.M == int(c.shape) and list(a.Jr) == [4] * 6 and (a.count == 3).all()
            assert (a.elig_n == a.M).any() and (a.elig_n == 1).any()
        elif c.family == "jobs":
            a = edge[0]
            assert tuple(a.count[0]) == WC.JOB_TOTALS[c.shape] and (a.Jr == 1).all()
        elif c.family == "orders":
            assert all(a.S == WC.ORDERS_S and list(a.Jr) == [1, 2] and (a.count == 1).all() for a in edge)
        elif c.family == "late":
            a = edge[0]
            assert a.R == 256 and int(a.p.max()) == 5 and int(a.delivery[0]) == -(2 ** 31 - 1 - 256 * 5)
        elif c.family == "chunk_orders":
            assert [(a.K, a.S) for a in c.arrs] == [(1, 1), (64, 2), (int(c.shape), 3)]
            assert all(1 <= j <= 16 for a in c.arrs for j in a.Jr) and all((a.count == 1).all() for a in c.arrs[1:])
            assert c.record == (c.shape == "128")
    # MO_DFJSP machines cases: windows on the highest machine, at most four per machine
    for M in WC.MACHINE_M:
        a = WC.set_arrays(WC.case(("machines", str(M), 4)))[0]
        assert a.bk_n[M - 1] == 4 and a.bk_n.max() <= 4 and (a.idle_power > 0).all() and ((a.power > 0) == (a.p > 0)).all()


def test_dispatch_rows_restate_the_schedule(oracle):
    """WC.dispatch_rows: schedule.from_trace where there are no windows; with windows its latest end is the oracle's
    completion_time and some dispatch is moved."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    c = WC.case(("machines", "32", 0))
    arrs, acts = WC.set_arrays(c), WC.actions(c)
    w = WC.replay(c, arrs, acts)[0]
    rows, delayed = WC.dispatch_rows(arrs[0], w)
    assert np.array_equal(rows, sch.from_trace(arrs[0], w["k"], w["m"], w["job_n"], w["step_time"])) and not delayed.any()
    c = WC.case(("machines", "32", 4))
    arrs, acts = WC.set_arrays(c), WC.actions(c)
    for e, w in enumerate(WC.replay(c, arrs, acts)):
        rows, delayed = WC.dispatch_rows(arrs[e % c.n_inst], w)
        assert rows[:, 5].max() == w["completion_time"] and (e % c.n_inst != 0 or delayed.any())


# ---- the create-time limits, both sides ----------------------------------------------------------------------------

def _create(Jr, M, count, arrive, delivery, variant=0, p=5, machine_data=False):
    """fjsp_env_create on one instance with every operation type eligible everywhere: (return code, message)."""
    from deep_reinforcement_learning_for_fjsp_amd import _capi, instances as fi
    lib = _capi.lib()
    Jr = np.asarray(Jr, np.int32)
    K = int(Jr.sum())
    s = fi.InstanceSet(1)
    s.set_raw(0, Jr, np.full((K, M), p, np.int32), np.full(K, M, np.int32), np.tile(np.arange(M, dtype=np.int32), (K, 1)),
              count, np.asarray(arrive, np.int32), np.asarray(delivery, np.int32))
    s.set_x(0, np.full((K, M), 1.0 / M))
    if machine_data:
        s.generate_machine_data(0, 1)
    h = C.c_void_p()
    rc = lib.fjsp_env_create(s.handle, 0, 1, 1, variant, 0, 0, C.byref(h))
    msg = lib.fjsp_last_error() if rc else b""
    if rc == 0:
        lib.fjsp_env_destroy(h)
    return rc, msg


LATE = WC.late_delivery(256, 5)
ARRIVAL_STAGES = b"more than 254 operations in a kind of a batch with order arrivals"
# name: (refused side, its message, admitted side); a side = the arguments of _create
LIMIT_PAIRS = {
    "K 256|257": (dict(Jr=[16] * 16 + [1], M=2, count=[1] * 17, arrive=[0], delivery=[100]), b"more than 256 operation types",
                  dict(Jr=[16] * 16, M=2, count=[1] * 16, arrive=[0], delivery=[100])),
    "M 32|33": (dict(Jr=[2], M=33, count=[1], arrive=[0], delivery=[100]), b"more than 32 machines",
                dict(Jr=[2], M=32, count=[1], arrive=[0], delivery=[100])),
    "S 64|65": (dict(Jr=[2], M=2, count=np.ones((65, 1)), arrive=np.arange(65), delivery=np.arange(65) + 9), b"more than 64 orders",
                dict(Jr=[2], M=2, count=np.ones((64, 1)), arrive=np.arange(64), delivery=np.arange(64) + 9)),
    "stages 255|256": (dict(Jr=[256], M=2, count=[1], arrive=[0], delivery=[100]), b"more than 255 operations in a kind",
                       dict(Jr=[255], M=2, count=[1], arrive=[0], delivery=[100])),
    "late delivery": (dict(Jr=[1] * 256, M=2, count=[1] * 256, arrive=[0], delivery=[LATE - 1], variant=5), b"32-bit clocks",
                      dict(Jr=[1] * 256, M=2, count=[1] * 256, arrive=[0], delivery=[LATE], variant=5)),
    # a batch with order arrivals keeps 255 in a job's next-stage byte for the orders still to come (kAbsent)
    "stages 254|255, two orders": (dict(Jr=[255, 1], M=2, count=np.ones((2, 2)), arrive=[0, 40], delivery=[100, 140]), ARRIVAL_STAGES,
                                   dict(Jr=[254, 1], M=2, count=np.ones((2, 2)), arrive=[0, 40], delivery=[100, 140])),
    "stages 254|255, MO_DFJSP": (dict(Jr=[255, 1], M=2, count=[1, 1], arrive=[0], delivery=[100], variant=4, machine_data=True), ARRIVAL_STAGES,
                                 dict(Jr=[254, 1], M=2, count=[1, 1], arrive=[0], delivery=[100], variant=4, machine_data=True)),
}


@pytest.mark.parametrize("name", list(LIMIT_PAIRS))
def test_create_limits_on_both_sides(built, name):
    """One step beyond the limit: FJSP_E_UNSUPPORTED with the limit's message, before any device is touched.  At the
    limit: anything but that (0 on a GPU machine, FJSP_E_HIP without one)."""
    refused, message, admitted = LIMIT_PAIRS[name]
    rc, msg = _create(**refused)
    assert rc == E_UNSUPPORTED and message in msg, (name, rc, msg)
    rc, msg = _create(**admitted)
    assert rc != E_UNSUPPORTED, (name, rc, msg)


def test_a_kind_of_255_stages_is_refused_beside_an_instance_with_arrivals(built):
    """The batch, not the instance, decides: a single-order instance with a kind of 255 stages is played alone and refused in
    one batch with a two-order instance, which puts every environment on the kernels with order arrivals."""
    from deep_reinforcement_learning_for_fjsp_amd import _capi, instances as fi
    lib = _capi.lib()
    s = fi.InstanceSet(2)
    for i, (Jr, S) in enumerate((([255], 1), ([2], 2))):
        K, M = sum(Jr), 2
        s.set_raw(i, Jr, np.full((K, M), 5, np.int32), np.full(K, M, np.int32), np.tile(np.arange(M, dtype=np.int32), (K, 1)),
                  np.ones((S, 1)), np.arange(S) * 40, np.arange(S) * 40 + 100)
        s.set_x(i, np.full((K, M), 1.0 / M))
    for first, n_inst, refused in ((0, 1, False), (1, 1, False), (0, 2, True)):
        h = C.c_void_p()
        rc = lib.fjsp_env_create(s.handle, first, n_inst, 2, 0, 0, 0, C.byref(h))
        if rc == 0:
            lib.fjsp_env_destroy(h)
        assert (rc == E_UNSUPPORTED) == refused, (first, n_inst, rc, lib.fjsp_last_error())
        assert not refused or ARRIVAL_STAGES in lib.fjsp_last_error()


def test_generated_handles_with_arrivals_stop_at_254_stages():
    """The generators' worst-case check: J_max = 255 is refused for a handle with order arrivals (S_max > 1, MO_DFJSP) and
    passes for one order; J_max = 254 passes everywhere."""
    from tests import test_generate_dynamic_host as GD, test_generate_orders_host as GO
    shape = lambda J: dict(R_min=1, R_max=1, J_min=J, J_max=J, N_min=1, N_max=1)
    text = "more than 254 operations in a kind (J_max)"
    for J, S_max, refused in ((255, 2, True), (254, 2, False), (255, 1, False)):
        rc, msg = GO.create(GO.orders(S_min=1, S_max=S_max, **shape(J)))
        assert (rc == E_UNSUPPORTED and text in msg) if refused else rc != E_UNSUPPORTED, (J, S_max, rc, msg)
    for J, refused in ((255, True), (254, False)):
        rc, msg = GD.create(GD.dyn(S_min=1, S_max=1, **shape(J)))
        assert (rc == E_UNSUPPORTED and text in msg) if refused else rc != E_UNSUPPORTED, (J, rc, msg)
