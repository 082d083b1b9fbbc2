"""Reference-held fixture of the dispatched schedule: tests/golden/schedule.npz.

For every suite it replays stored episodes of the existing fixtures (same instances, actions, random.choice stream and
reward arguments) on the REFERENCE environment, imported the way make_golden.py imports it (under oracle/ref_shim,
the build's own fluid LP supplying x), and reads the reference's task objects after the episode
(SO_FJSSP.py:182-184, MO_DFJSP_breakdown.py:233-235): (kind, task, job number, machine, time_begin, time_end) of every
dispatched operation, in dispatch order.  Only arrays enter the file.

    python tests/golden/make_schedule_golden.py              # (re)write schedule.npz
    python tests/golden/make_schedule_golden.py --compare    # regenerate and check the file is byte-identical

Layout of schedule.npz (prefix <suite>_e<i>_ per stored episode):
    inst_<key>  the instance arrays (as make_golden.py stores them) and inst_name
    source      index of the episode in tests/golden/<suite>.npz
    rng_seed, actions u8[T][2], mo f64[4] (variants with reward arguments)
    table       i32[T][6] = (r, j, n, m, time_begin, time_end) in dispatch order
and suites (the suite names), <suite>_variant, <suite>_n_episodes.
"""
import argparse
import io
import os
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
import make_golden as mg  # noqa: E402  (puts the reference under oracle/ref_shim on sys.path)
from tests import helpers as H  # noqa: E402

OUT = os.path.join(HERE, "schedule.npz")
# suite -> (variant, reference environment, stored episodes at most); one episode per instance first
SUITES = [("mk01", 0, "so", 3), ("synth10x5", 0, "so", 4), ("multijob", 0, "so", 4), ("multiorder", 0, "so", 3),
          ("so_sfjsp", 1, "sf", 4), ("so_dfjsp", 5, "sod", 4), ("mo_discretes", 2, "mo", 4), ("mo_dfjsp", 4, "dyn", 9)]


def _env_class(kind):
    from environments.SO_FJSSP import SO_FJSSP_Environment
    from environments.MO_FJSSP_discretes import MO_FJSSP_Environment
    from environments.SO_SFJSP import SO_SFJSP_Environment
    from environments.MO_DFJSP_breakdown import MO_DFJSP_Environment
    from environments.SO_DFJSP import SO_DFJSP_Environment
    return {"so": SO_FJSSP_Environment, "mo": MO_FJSSP_Environment, "sf": SO_SFJSP_Environment,
            "dyn": MO_DFJSP_Environment, "sod": SO_DFJSP_Environment}[kind]


def _mo_arg(kind, ep):
    """The reward arguments of run_reference from the fixture's stored mo vector (-1 = None)."""
    none = lambda v: None if v < 0 else float(v)
    if kind in ("sf", "sod"):
        return kind
    if kind == "dyn":
        m = ep["mo"]
        return ("dyn", int(m[0]), none(m[1]), none(m[2]), none(m[3]))
    if kind == "mo":
        m = ep["mo"]
        return (float(m[0]), float(m[1]), none(m[2]), none(m[3]))
    return None


def reference_table(env, ep, koff):
    """(r, j, n, m, time_begin, time_end) per step, from the reference's task objects (machine.task_list)."""
    tasks = {}
    for m in env.machine_tuple:
        for task in env.machine_dict[m].task_list:
            tasks[(task.kind, task.task, task.number)] = (task.machine, task.time_begin, task.time_end)
    T = ep["T"]
    out = np.zeros((T, 6), np.int32)
    for t in range(T):
        k, n = int(ep["k"][t]), int(ep["job_n"][t])
        r = int(np.searchsorted(koff, k, side="right") - 1)
        j = k - int(koff[r])
        m, b, e = tasks.pop((r, j, n))
        assert m == int(ep["m"][t])
        out[t] = (r, j, n, m, b, e)
    assert not tasks, "the reference holds dispatched tasks the trace does not"
    return out


def _windows(a):
    """Start times of the breakdown windows of every machine."""
    off = np.concatenate(([0], np.cumsum(a.bk_n)))
    bk = np.asarray(a.bk).reshape(-1, 2)
    return [set(int(x) for x in bk[off[m]:off[m + 1], 0]) for m in range(len(a.bk_n))]


def build():
    store = {}
    tmp = tempfile.mkdtemp(prefix="fjsp_schedule_golden_")
    store["suites"] = np.array([s for s, _, _, _ in SUITES])
    for suite, variant, kind, n_max in SUITES:
        insts, eps, _ = H.load_suite(suite)
        picked, seen = [], set()
        for e, ep in enumerate(eps):                      # one episode per instance, in file order
            if ep["inst"] not in seen and len(picked) < n_max:
                picked.append(e); seen.add(ep["inst"])
        for e, ep in enumerate(eps):                      # then fill up
            if e not in picked and len(picked) < n_max:
                picked.append(e)
        shifted = at_end = 0
        for i, e in enumerate(sorted(picked)):
            ep = eps[e]
            a = insts[ep["inst"]]
            a.koff = np.concatenate(([0], np.cumsum(a.Jr))).astype(np.int32)
            folder = os.path.basename(a.name) or "inst"
            parent = os.path.join(tmp, "%s_%d" % (suite, i))
            mg.write_csv_folder(a, os.path.join(parent, folder))
            ref, env = mg.run_reference(_env_class(kind), a, parent, folder, ep["actions"], ep["rng_seed"], check_lp=False,
                                        mo=_mo_arg(kind, ep))
            assert ref["T"] == ep["T"] and np.array_equal(ref["k"], ep["k"]) and np.array_equal(ref["m"], ep["m"]), \
                "%s episode %d replays differently on the reference" % (suite, e)
            table = reference_table(env, ep, a.koff)
            clock = np.concatenate(([0], ep["step_time"][:-1]))
            shifted += int(np.sum(table[:, 4] != clock))
            if hasattr(a, "bk_n"):
                w = _windows(a)
                at_end += int(sum(1 for row in table if int(row[5]) in w[int(row[3])]))
            p = "%s_e%d_" % (suite, i)
            mg.store_instance(store, p + "inst_", a, a.name)
            store[p + "source"] = np.int32(e)
            store[p + "rng_seed"] = np.uint64(ep["rng_seed"])
            store[p + "actions"] = np.ascontiguousarray(ep["actions"][:ep["T"]], np.uint8)
            if "mo" in ep:
                store[p + "mo"] = np.asarray(ep["mo"], np.float64)
            store[p + "table"] = table
        store[suite + "_variant"] = np.int32(variant)
        store[suite + "_n_episodes"] = np.int32(len(picked))
        print("%-13s episodes %d  operations started after their dispatch clock (breakdown shift) %d, ending where a window "
              "opens %d" % (suite, len(picked), shifted, at_end))
    return store


def serialise(store):
    """npz bytes with fixed member timestamps and order (np.savez stamps the current time: not reproducible)."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(store):
            arr = io.BytesIO()
            np.lib.format.write_array(arr, np.asanyarray(store[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, arr.getvalue())
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", action="store_true", help="regenerate and check that schedule.npz is byte-identical")
    args = ap.parse_args()
    data = serialise(build())
    if args.compare:
        old = open(OUT, "rb").read()
        if old != data:
            print("schedule.npz DIFFERS from the regenerated fixture (%d vs %d bytes)" % (len(old), len(data)))
            sys.exit(1)
        print("schedule.npz is byte-identical to the regenerated fixture (%d bytes)" % len(data))
        return
    with open(OUT, "wb") as f:
        f.write(data)
    print("wrote %s (%d bytes)" % (OUT, len(data)))


if __name__ == "__main__":
    main()
