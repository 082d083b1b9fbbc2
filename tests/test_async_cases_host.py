"""What tests/test_gpu_async_arrivals.py leans on, proven on the CPU: the C oracle with a recording LP hook plays the
instances of tests/async_cases.py and shows when, and with which LP, every environment reaches its order arrival.

A later edit of the cases that loses one of these conditions fails here, not silently on the GPU."""
import numpy as np
import pytest

from tests import async_cases as AC


@pytest.fixture(scope="module")
def oracle(built):
    from oracle import pyoracle
    pyoracle.lib()
    return pyoracle


def _set_arrays(names, variant):
    s = AC.instance_set(names, variant)
    return [s.arrays(i) for i in range(len(names))]


def test_case_shapes_reach_the_chunk_counts_and_layouts(oracle):
    """One, two and four chunks of 64 operation types, M > 8 in the multi-chunk cases, two orders everywhere; MO_DFJSP:
    every machine has an eligible operation (the reference divides by zero otherwise) and breakdown windows exist."""
    want = {1: (lambda K: K <= 64), 2: (lambda K: 65 <= K <= 128), 4: (lambda K: 129 <= K <= 256)}
    for chunks, name in AC.STAGGERED.items():
        a = AC.arr(name)
        assert want[chunks](a.K) and a.S == 2, name
        assert chunks == 1 or a.M > 8, name
        assert (a.p > 0).any(axis=0).all(), name
    for chunks, variant, _ in AC.STAGGERED_SETS:
        if variant == AC.MO_DFJSP:
            a = _set_arrays([AC.STAGGERED[chunks]], variant)[0]
            assert int(np.asarray(a.bk_n).sum()) > 0
    assert [AC.ops_first(AC.arr(n)) for n in AC.LOCKSTEP] == [3, 4]
    assert [AC.ops_total(AC.arr(n)) for n in AC.LOCKSTEP] == [6, 8]


@pytest.mark.parametrize("name", AC.LOCKSTEP)
def test_lockstep_cases_arrive_in_one_step_with_one_lp(oracle, name):
    """Every rule pair of SO_FJSSP's action space played throughout, the random.choice pair under several env seeds,
    and random pairs per step: the one arrival of the episode falls in the step that dispatches the last operation of
    the first order, and its LP inputs are the same for all of them -- all envs of an instance park in one call and a
    batch of it poses n_inst different LPs ("hits = N - n_inst")."""
    variant = AC.SO_FJSSP
    a = _set_arrays([name], variant)[0]
    T, first = AC.ops_total(a), AC.ops_first(a)
    n0, n1 = AC.ACTION_SPACE[variant]
    plays = [(np.tile(np.array([r0, r1], np.uint8), (T, 1)), AC.env_seed(0)) for r0 in range(n0) for r1 in range(n1)]
    plays += [(np.tile(np.array(AC.RANDOM_PAIR[variant], np.uint8), (T, 1)), AC.env_seed(e)) for e in (1, 7, 64, 149, 299)]
    rnd = AC.actions(variant, T, 16, 31)
    plays += [(rnd[:, e], AC.env_seed(e)) for e in range(16)]
    seen = set()
    for acts, seed in plays:
        Te, calls = AC.arrivals(a, acts, seed, variant)
        assert Te == T
        assert len(calls) == a.S - 1 == 1
        step, Q, now = calls[0]
        assert step == first - 1
        seen.add((Q.tobytes(), now.tobytes()))
    assert len(seen) == 1
    # the shop had run empty: every job of the new order waits at its first operation
    koff = np.concatenate(([0], np.cumsum(a.Jr)))[:-1]
    assert (now[koff] > 0).all() and int(now.sum()) == int(now[koff].sum())
    assert np.array_equal(Q, np.repeat(np.asarray(a.count).reshape(a.S, a.R)[1], a.Jr))      # nothing of the first order is left


def staggered_arrivals(chunks, variant, N):
    """[(step, Q, n_now)] of env 0 .. N - 1's first episode under the actions the GPU case assigns."""
    a = _set_arrays([AC.STAGGERED[chunks]], variant)[0]
    acts = AC.staggered_actions(chunks, variant, N)
    mo = AC.mo_rows(variant, N)
    out = []
    for e in range(N):
        Te, calls = AC.arrivals(a, acts[:, e], AC.env_seed(e), variant, None if mo is None else mo[e])
        assert Te == AC.ops_total(a)
        assert len(calls) == a.S - 1 == 1, "env %d got through an episode without exactly one arrival LP" % e
        out.append(calls[0])
    return a, out


@pytest.mark.parametrize("chunks,variant,N", AC.STAGGERED_SETS)
def test_staggered_cases_spread_their_arrivals(oracle, chunks, variant, N):
    """Under the per-env random rule pairs of the GPU case every env parks exactly once per episode, the arrivals fall
    in at least three different steps with at least three different (Q, n_now), and at least one arrival finds jobs
    in process (n_now != Q; the lock-step family has the other branch: an empty shop and a clock jump)."""
    a, calls = staggered_arrivals(chunks, variant, N)
    steps = {c[0] for c in calls}
    lps = {(c[1].tobytes(), c[2].tobytes()) for c in calls}
    assert len(steps) >= 3, sorted(steps)
    assert len(lps) >= 3
    assert any(not np.array_equal(c[1], c[2]) for c in calls)
    # ... and the LP really holds work of both orders: more unprocessed tasks of an operation type than the new order brings
    new = np.repeat(np.asarray(a.count).reshape(a.S, a.R)[1], a.Jr)
    assert any((c[1] > new).any() for c in calls)
    assert max(steps) < AC.ops_total(a) - 1          # the arrival is never the episode's last step
