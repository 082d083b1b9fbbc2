"""What tests/test_gpu_policy_orders_wide.py leans on, proven on the CPU: the C oracle plays every case of
tests/policy_orders_wide_cases.py under seeded random actions to its end, through every order arrival while the shop is
busy and into the last chunk of operation types afterwards; and the slice / workgroup / LP-route arithmetic, restated in
that module, gives the builds its table names -- the GPU test asserts the same values from the library."""
import numpy as np
import pytest

from tests import async_cases as AC
from tests import helpers as H
from tests import policy_orders_wide_cases as PW
from tests import wave_limit_cases as WC

N_HOST = 6                       # two environments per instance


@pytest.fixture(scope="module")
def oracle(built):
    from oracle import pyoracle
    pyoracle.lib()
    return pyoracle


def test_the_table_is_the_shape_of_the_instances():
    assert PW.NAMES == ("k65", "k65flat", "k128", "k129", "k256", "k129x2")
    for name in PW.NAMES:
        sp, (edge, one, k64) = PW.SPECS[name], PW.instances(name)
        assert (edge.K, edge.R, edge.S, edge.M) == (sp["K"], sp["kinds"], len(sp["arrive"]), 3), name
        assert sp["K"] == sp["kinds"] * sp["stages"] and int(edge.count.sum()) == sp["n_jobs"] == sp["kinds"] * sp["jobs"] * edge.S, name
        assert WC.ops_total(edge) == sp["steps"] == sp["n_jobs"] * sp["stages"], name
        assert (edge.count == sp["jobs"]).all() and tuple(edge.arrive) == sp["arrive"], name
        assert (one.S, one.M) == (1, 3) and one.K <= 8, name
        assert (k64.S, k64.K, k64.M) == (2, 64, 3), name
        # the fillers share the padded sizes: they never decide the batch's
        assert max(int(a.count.sum()) for a in (one, k64)) <= sp["n_jobs"] and edge.S >= 2, name
        for a in (edge, one, k64):
            assert (a.p > 0).any(axis=0).all() and a.p.max() <= 5 and a.p[a.p > 0].min() >= 1, a.name
        assert sp["N"] == (6 if name == "k129x2" else 12) and sp["N"] % 3 == 0 and sp["N"] % sp["envs_per_wg"] != 0, name


@pytest.mark.parametrize("name", PW.NAMES)
def test_build_arithmetic_gives_the_table(name):
    """(d): chunk count, slice, environments per workgroup, segments and the LP service of every create route."""
    sp, arrs = PW.SPECS[name], PW.instances(name)
    assert PW.actor_bytes(20) == 93440
    assert PW.expected_build(arrs) == (sp["kc"], sp["envs_per_wg"], sp["slice"], len(sp["arrive"])), name
    # the edge instance alone decides: the fillers change nothing
    assert PW.expected_build(arrs[:1]) == PW.expected_build(arrs), name
    for route in PW.LP_ROUTES:
        assert PW.expected_lp(arrs, route) == PW.lp_expected(name, route), (name, route)


def test_build_arithmetic_on_the_shapes_the_suite_already_pins():
    """The restated arithmetic on shapes whose build other GPU tests assert (test_gpu_policy_orders.py: 204 jobs -> 8,
    1920 jobs -> 2; test_gpu_policy_wide.py: slices of 2880, 3904, 4416 and 8512 bytes), and on the one-env shape."""
    assert [PW.slice_bytes(j, 6) for j in (96, 210, 280, 810)] == [2880, 3904, 4416, 8512]
    assert [PW.envs_per_workgroup(j, 8) for j in (134, 204, 1920)] == [16, 8, 2]
    assert PW.slice_bytes(4044, 8) == 34624 and PW.envs_per_workgroup(4044, 8) == 1


@pytest.mark.parametrize("variant", PW.VARIANTS)
@pytest.mark.parametrize("name", PW.NAMES)
def test_oracle_plays_the_case_through_its_arrivals(oracle, name, variant):
    """(a) every episode is as long as its operation count; (b) the edge instance re-solves exactly S - 1 times after reset,
    each time with operations of the earlier orders still to dispatch; (c) an operation type of its last chunk is
    dispatched after the first arrival."""
    sp = PW.SPECS[name]
    arrs = PW.set_arrays(name)
    acts = PW.actions(name, variant, N_HOST)
    assert len(set(acts[:, :, 0].ravel())) == 6 and len(set(acts[:, :, 1].ravel())) == 5         # the whole action space
    for e in range(N_HOST):
        a = arrs[e % 3]
        w = H.play_oracle(a, a.x, acts[:, e], PW.env_seed(e), variant=variant)
        assert w["T"] == WC.ops_total(a) and bool(w["done"][-1]), (name, e)                                # (a)
        assert np.isfinite(w["states"]).all(), (name, e)
        T, calls = AC.arrivals(a, acts[:, e], PW.env_seed(e), variant)
        steps = sorted(step for step, _, _ in calls)
        assert T == w["T"] and len(steps) == a.S - 1, (name, e, steps)                               # (b)
        before = np.cumsum((a.count * a.Jr[None, :]).sum(1))        # operations of orders 0 .. s
        for s, t in enumerate(steps):
            assert t + 1 < before[s], "%s env %d: order %d arrives at step %d, after the shop ran empty" % (name, e, s + 1, t)
        if e % 3 == 0:
            last = (a.K - 1) // 64
            assert PW.chunks(a.K) == sp["kc"] and last >= 1
            n = int((w["k"][steps[0] + 1:] // 64 == last).sum())
            assert n > 0 and int(w["k"].max()) == a.K - 1, "%s env %d: %d dispatches in chunk %d after step %d" % (name, e, n, last, steps[0])   # (c)
