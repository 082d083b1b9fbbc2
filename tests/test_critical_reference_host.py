"""CPU: tests/critical_reference.py against answers written out by hand, and the two properties that make the pair move the
critical swap, on all seven golden suites (recorded plans and three random plans per episode): a table in begin order
skips no machine arc, and every pair move decodes to the schedule with its two operations exchanged on their machine and
every other machine's sequence unchanged.  Also: every path operation is critical and tail + end never exceeds C."""
import numpy as np
import pytest

from tests import critical_cases as K
from tests import critical_reference as R
from tests import decode_reference as D
from tests import schedule_fixture as F

SUITES = ("mk01", "synth10x5", "multijob", "so_sfjsp", "mo_discretes", "multiorder", "so_dfjsp")


@pytest.mark.parametrize("name", sorted(K.HAND))
def test_hand_made_tables(name):
    a = K.hand_arrays()
    n = len(K.HAND[name][1]["moves"])
    for max_moves in sorted({0, 1, n, n + 1}):
        got, want = R.critical_one(a, K.table(K.HAND[name][0]), max_moves), K.hand_answer(name, max_moves)
        for key in R.KEYS:
            assert np.array_equal(got[key], want[key]), (name, max_moves, key, got[key], want[key])


def test_status_codes():
    a = K.hand_arrays()
    assert R.critical_one(a, K.table(K.VALID), 4)["status"] == R.OK
    empty = R.critical_one(a, K.table([]), 4)
    assert empty["status"] == R.EMPTY
    for name in K.BAD_ROWS:
        one = R.critical_one(a, K.bad_table(name), 4)
        assert one["status"] == R.BAD_ROW, name
        for res in (one, empty):
            assert np.all(res["tail"] == -1) and np.all(res["path"] == -1) and res["makespan"] == -1, name
            assert not res["flags"].any() and not res["moves"].any() and res["path_len"] == res["n_moves"] == res["skipped"] == 0, name


def test_pair_move_materialised():
    plan = np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 0, 1), (1, 0, 1), (2, 0, 1), (-1, -1, -1)], np.int32)
    rows = lambda mv: R.materialise_pair(plan, mv)[:6, 0].tolist()
    first = lambda mv: R.materialise_pair(plan, mv)[:, 0].tolist()
    assert first((4, 1, 3 | (1 << 16))) == [0, 2, 1, 1, 0, 2, -1]          # rows 1 and 4 behind row 2, row 4 first
    assert first((4, 1, 3 | (0 << 16))) == [0, 1, 1, 2, 0, 2, -1]          # dw = 0: v in front of u
    assert first((4, 1, 3 | (2 << 16))) == [0, 2, 0, 1, 1, 2, -1]          # dw = dv - 1: u behind v
    assert rows((4, 0, 5 | (4 << 16))) == [1, 2, 0, 1, 2, 0]               # u = 0, v = L - 1
    assert np.array_equal(R.materialise_pair(plan, (4, 2, 1))[:6], D.materialise(plan, (2, 2, 0))[:6])   # dv = 1: the swap
    for bad in ((4, 1, 5), (4, -1, 1), (4, 1, 0), (4, 1, 2 | (2 << 16)), (4, 1, -1), (4, 5, 1), (4, 1, 3 | (3 << 16))):
        assert not R.pair_ok(plan, bad) and np.array_equal(R.materialise_pair(plan, bad), plan), bad


@pytest.fixture(scope="module")
def suites():
    return F.load()


def _tables(variant, ep, rs):
    """Decoded tables of the episode's recorded plan and of three random plans."""
    a = ep["inst"]
    plans = [D.plan_from_table(ep["table"])] + [D.random_plan(a, rs) for _ in range(3)]
    out = []
    for pl in plans:
        one = D.decode_one(a, variant, pl)
        assert one["status"] == 0
        out.append(one["table"])
    return out


@pytest.mark.parametrize("suite", SUITES)
def test_begin_order_skips_nothing_and_pair_moves_are_the_swaps(suites, suite):
    variant, eps = suites[suite]
    rs = np.random.RandomState(len(suite))
    arcs = 0
    for ep in eps:
        a = ep["inst"]
        for given in _tables(variant, ep, rs):
            tab = R.begin_order(given)
            plan = D.plan_from_table(tab[:R.table_length(tab)], len(tab))
            same = D.decode_one(a, variant, plan)
            assert same["status"] == 0 and R.machine_sequences(same["table"]) == R.machine_sequences(given)
            assert np.array_equal(same["table"], tab)                              # begin order is the same schedule
            for t, res in ((given, R.critical_one(a, given, 0)), (tab, R.critical_one(a, tab, 0))):
                L, C = R.table_length(t), res["makespan"]
                assert res["status"] == 0 and C == same["objective"][0]
                assert np.all(res["tail"][:L] + t[:L, 5] <= C)
                path = res["path"][:res["path_len"]]
                assert np.all(res["flags"][path] & R.CRITICAL) and np.all(np.diff(path) < 0)
            res = R.critical_one(a, tab, res["n_moves"])
            assert res["skipped"] == 0
            base = R.machine_sequences(tab)
            for mv in res["moves"][res["moves"][:, 0] == R.MOVE_PAIR]:
                u, v = int(mv[1]), int(mv[1]) + (int(mv[2]) & 0xFFFF)
                op = lambda t: (int(tab[t, 0]), int(tab[t, 1]), int(tab[t, 2]))
                m = int(tab[u, 3])
                assert m == int(tab[v, 3]) and res["flags"][u] & R.MACHINE_ARC
                moved = R.decode_pair(a, variant, plan, mv)
                assert moved["status"] == 0
                want = {k: list(s) for k, s in base.items()}
                i = want[m].index(op(u))
                assert want[m][i + 1] == op(v)
                want[m][i], want[m][i + 1] = want[m][i + 1], want[m][i]
                assert R.machine_sequences(moved["table"]) == want, (suite, mv)
                arcs += 1
    assert arcs > 0
