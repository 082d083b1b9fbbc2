"""Hand-made plans with known answers for fjsp_schedule_decode_active, shared by tests/test_decode_active_reference_host.py
(the numpy statement) and tests/test_gpu_decode_active.py (the kernel): each is an instance, a variant, a complete plan,
the begin every row must get, and the rows that must count as inserted."""
import numpy as np

from tests import decode_limit_cases as DL


class Hand(object):
    def __init__(self, name, inst, variant, rows, begins, inserted):
        self.name, self.inst, self.variant = name, inst, variant
        self.plan = np.asarray(rows, np.int32).reshape(-1, 3)
        self.begins, self.inserted = list(begins), int(inserted)


def _gap_shop():
    """Kind 0: two stages, machine 1 (4) then machine 0 (2): its second stage leaves machine 0 idle in [0, 4).  Kinds 1 and
    2: one stage on machine 0, 4 and 5 long."""
    return DL.instance("gap", [2, 1, 1], [[0, 4], [2, 0], [4, 0], [5, 0]], [1, 1, 1])


def _four_gaps():
    """Kinds 0..3: a first stage on machine 1 (2, 3, 3, 4 long, one after the other) and a second on machine 0 (1 long), which
    leave machine 0 idle in [0, 2), [3, 5), [6, 8), [9, 12); kind 4: one stage of 3 on machine 0."""
    p = [[0, 2], [1, 0], [0, 3], [1, 0], [0, 3], [1, 0], [0, 4], [1, 0], [3, 0]]
    return DL.instance("four-gaps", [2, 2, 2, 2, 1], p, [1] * 5)


def cases():
    gap = _gap_shop()
    head = [(0, 0, 1), (0, 0, 0)]                                          # [0, 4) on machine 1, [4, 6) on machine 0
    two = DL.instance("late-order", [1], [[3]], [[1], [1]], arrive=[0, 10], delivery=[20, 30])
    mid = DL.instance("mid", [2, 1], [[0, 3], [2, 0], [5, 0]], [1, 1])
    four = _four_gaps()
    chain = [(r, 0, m) for r in range(4) for m in (1, 0)]
    lone = DL.instance("lone", [1], [[6]], [1], arrive=[7], delivery=[9])
    return [
        Hand("a gap exactly as long as the operation", gap, 0, head + [(1, 0, 0), (2, 0, 0)], [0, 4, 0, 6], 1),
        Hand("a gap one unit too short", gap, 0, head + [(2, 0, 0), (1, 0, 0)], [0, 4, 6, 0], 1),
        Hand("a gap in front of the first interval, opened by a later order", two, 0, [(0, 1, 0), (0, 0, 0)], [10, 0], 1),
        Hand("a job ready in the middle of a busy interval", mid, 0, [(1, 0, 0), (0, 0, 1), (0, 0, 0)], [0, 0, 5], 0),
        Hand("three gaps skipped, placed in the fourth", four, 0, chain + [(4, 0, 0)], [0, 2, 2, 5, 5, 8, 8, 12, 9], 1),
        Hand("one job, one operation, one machine", lone, 0, [(0, 0, 0)], [7], 0),
    ]
