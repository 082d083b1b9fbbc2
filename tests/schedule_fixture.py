"""Reader of tests/golden/schedule.npz (written by tests/golden/make_schedule_golden.py): the reference's dispatched
schedules, (r, j, n, m, time_begin, time_end) per operation in dispatch order, with the episodes that produced them."""
import os

import numpy as np

from tests import helpers as H

PATH = os.path.join(H.GOLDEN, "schedule.npz")


def load():
    """{suite: (variant, [episode dict: inst, source, rng_seed, actions, mo (or None), table])}."""
    z = np.load(PATH, allow_pickle=False)
    out = {}
    for suite in [str(s) for s in z["suites"]]:
        eps = []
        for i in range(int(z[suite + "_n_episodes"])):
            p = "%s_e%d_" % (suite, i)
            a = H.Arrays()
            for key in ("Jr", "p", "elig_n", "elig_list", "count", "arrive", "delivery", "x", "power", "idle_power", "bk_n", "bk"):
                if p + "inst_" + key in z.files:
                    setattr(a, key, z[p + "inst_" + key])
            a.ddt = float(z[p + "inst_ddt"])
            a.name = str(z[p + "inst_name"])
            a.R, a.S = len(a.Jr), len(a.arrive)
            a.K, a.M = a.p.shape
            eps.append(dict(inst=a, source=int(z[p + "source"]), rng_seed=int(z[p + "rng_seed"]), actions=z[p + "actions"],
                            mo=z[p + "mo"] if p + "mo" in z.files else None, table=z[p + "table"]))
        out[suite] = (int(z[suite + "_variant"]), eps)
    return out
