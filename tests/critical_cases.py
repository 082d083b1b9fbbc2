"""Hand-made tables for fjsp_schedule_critical with their answers written out, and the rows that fail each range check;
shared by the host test of tests/critical_reference.py and the GPU test of the kernel."""
import numpy as np

from tests import helpers as H

# three kinds of one job and two stages each, two machines; operation type 0 runs on machine 0 only
HAND_JR = [2, 2, 2]
HAND_P = [[3, 0], [2, 2], [3, 3], [2, 2], [1, 1], [2, 2]]
HAND_JOBS = [1, 1, 1]
CAP = 6


def hand_arrays():
    a = H.Arrays()
    a.Jr, a.p = np.array(HAND_JR, np.int32), np.array(HAND_P, np.int32)
    a.count, a.arrive, a.delivery = np.array([HAND_JOBS], np.int32), np.array([0], np.int32), np.array([20], np.int32)
    return a


def instance_set(specs):
    """A solved InstanceSet of shops given as (Jr, p, jobs per kind), one order at 0."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    s = fi.InstanceSet(len(specs))
    for i, (Jr, p, jobs) in enumerate(specs):
        p = np.asarray(p)
        elig_list = np.zeros(p.shape, np.int32)
        for k in range(len(p)):
            e = np.flatnonzero(p[k])
            elig_list[k, :len(e)] = e
        s.set_raw(i, Jr, p, (p > 0).sum(1), elig_list, [jobs], [0], [int(p.max()) * 3])
    return s.solve_fluid()


def table(rows, cap=CAP):
    out = np.full((cap, 6), -1, np.int32)
    if len(rows):
        out[:len(rows)] = rows
    return out


# name -> (rows (r, stage, n, m, begin, end), the answers)
HAND = {
    # two rows end at C: the first in table order starts the path; type 0 has no other machine
    "two ends at C": ([(0, 0, 0, 0, 0, 3), (1, 0, 0, 1, 0, 3)],
                      dict(makespan=3, tail=[0, 0], flags=[3, 1], path=[0], moves=[], skipped=0)),
    # row 2's job predecessor (row 0) and machine predecessor (row 1) are both tight: the later row wins, a machine arc
    "both tight, machine later": ([(0, 0, 0, 1, 0, 4), (1, 0, 0, 0, 1, 4), (0, 1, 0, 0, 4, 6)],
                                  dict(makespan=6, tail=[2, 2, 0], flags=[1, 7, 3], path=[2, 1],
                                       moves=[(4, 1, 1), (1, 2, 1), (1, 1, 1)], skipped=0)),
    # ... and with the two in the other order, a job arc
    "both tight, job later": ([(1, 0, 0, 0, 1, 4), (0, 0, 0, 1, 0, 4), (0, 1, 0, 0, 4, 6)],
                              dict(makespan=6, tail=[2, 2, 0], flags=[1, 3, 3], path=[2, 1], moves=[(1, 2, 1), (1, 1, 0)],
                                   skipped=0)),
    # row 0 is both the job and the machine predecessor of row 1: a job arc, no pair move
    "both predecessors": ([(0, 0, 0, 0, 0, 2), (0, 1, 0, 0, 2, 5)],
                          dict(makespan=5, tail=[3, 0], flags=[3, 3], path=[1, 0], moves=[(1, 1, 1)], skipped=0)),
    # the arc row 0 -> row 3 with a row of a's job in front of a row of b's job between them: no pair move expresses it
    # (a foreign table: machine 1's rows stand against their times, so the tails follow the table's order alone)
    "skipped arc": ([(1, 0, 0, 0, 0, 2), (1, 1, 0, 1, 2, 3), (2, 0, 0, 1, 0, 1), (2, 1, 0, 0, 2, 4)],
                    dict(makespan=4, tail=[4, 3, 2, 0], flags=[6, 0, 0, 3], path=[3, 0], moves=[(1, 3, 1), (1, 0, 1)], skipped=1)),
    # idle time in front of the last row: no tight predecessor, the path is that row
    "idle": ([(0, 0, 0, 0, 0, 3), (0, 1, 0, 0, 4, 6)],
             dict(makespan=6, tail=[2, 0], flags=[0, 3], path=[1], moves=[(1, 1, 1)], skipped=0)),
}


def hand_answer(name, max_moves, cap=CAP):
    """The written answer of HAND[name] in the shape of critical_reference.critical_one."""
    rows, ans = HAND[name]
    L, path, moves = len(rows), ans["path"], ans["moves"]
    out = dict(tail=np.full(cap, -1, np.int32), flags=np.zeros(cap, np.uint8), path=np.full(cap, -1, np.int32), path_len=len(path),
               moves=np.zeros((max_moves, 3), np.int32), n_moves=len(moves), skipped=ans["skipped"], status=0, makespan=ans["makespan"])
    out["tail"][:L], out["flags"][:L], out["path"][:len(path)] = ans["tail"], ans["flags"], path
    for i, mv in enumerate(moves[:max_moves]):
        out["moves"][i] = mv
    return out


VALID = [(0, 0, 0, 0, 0, 3), (1, 0, 0, 1, 0, 2), (0, 1, 0, 1, 3, 5)]
# name -> (row index, column, value) that makes VALID fail one range check
BAD_ROWS = {
    "r negative": (1, 0, -2), "r = R": (1, 0, 3), "r = -1 in a row that is no end": (0, 0, -1),
    "n negative": (1, 2, -1), "n = jobs": (1, 2, 1), "m negative": (2, 3, -1), "m = M": (2, 3, 2),
    "stage negative": (0, 1, -1), "stage = stages": (2, 1, 2), "begin negative": (0, 4, -1), "begin = end": (1, 4, 2),
    "begin > end": (1, 4, 7),
}


def bad_table(name, cap=CAP):
    rows = np.array(VALID, np.int32)
    t, c, v = BAD_ROWS[name]
    rows[t, c] = v
    return table(rows, cap)
