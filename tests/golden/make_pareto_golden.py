#!/usr/bin/env python3
"""tests/golden/pareto_reference.npz from the REFERENCE'S OWN DataProcess (build container only: needs /root/reference).

Imports utilities/Utility_Class.py itself and records, on a few hundred small point sets,

    filter_pareto_front   :132-146   the front of the set, and of the set joined with a second one (the "true" front)
    calculate_gd          :184-198   gd(true front, front)
    calculate_igd         :168-182   igd(true front, front)
    calculate_spread      :200-227   spread(front, true front)
    normalized_data       :124-130   front / the per-objective maximum of the true front

The sets: C in {1, 2, 3, 17, 64, 65, 130} points of D in 1..4 objectives, integer-valued coordinates drawn from
ranges of {2, 4, 9, 40} values, so ties, duplicates and dominated points all occur; three seeds each.  What keeps the
module from importing in this image is supplied as in make_agent_fixtures_ref.py: `openpyxl` / `docplex` from
oracle/ref_shim, matplotlib on the Agg backend, and any other plotting / spreadsheet module that is missing as an empty
stub in sys.modules.  Nothing of the reference travels: only the arrays in the .npz do (points as int16, results f64).

    python tests/golden/make_pareto_golden.py
"""
import importlib
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
OUT = os.path.join(HERE, "pareto_reference.npz")

SIZES, DIMS, RANGES, SEEDS = (1, 2, 3, 17, 64, 65, 130), (1, 2, 3, 4), (2, 4, 9, 40), (0, 1, 2)


class _Anything(object):
    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        return _Anything()

    def __call__(self, *a, **k):
        return _Anything()

    def __setitem__(self, k, v):
        pass


def bootstrap_reference():
    """The reference's DataProcess class."""
    if not os.path.isdir(REF):
        raise SystemExit("needs %s (build container only)" % REF)
    for p in (os.path.join(REPO, "oracle", "ref_shim"), REF):
        if p not in sys.path:
            sys.path.insert(0, p)
    try:
        import matplotlib
        matplotlib.use("Agg")
    except ImportError:
        pass
    for name in ("matplotlib", "matplotlib.pyplot", "matplotlib.ticker", "matplotlib.font_manager", "matplotlib.patches",
                 "mpl_toolkits", "mpl_toolkits.mplot3d", "mpl_toolkits.mplot3d.axes3d", "openpyxl", "openpyxl.styles", "pandas",
                 "scipy", "scipy.spatial", "scipy.spatial.distance"):
        try:
            importlib.import_module(name)
        except ImportError:                       # plotting / spreadsheet only: DataProcess uses none of them
            stub = types.ModuleType(name)
            stub.__getattr__ = lambda attr: _Anything()
            stub.__path__ = []
            sys.modules[name] = stub
    import utilities.Utility_Class as UC
    return UC.DataProcess


def main():
    dp = bootstrap_reference()()
    points, other, front, true_front, normal = [], [], [], [], []
    meta, metrics = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")           # (the NaN cases: a mean of infinities, 0 / 0)
        for C in SIZES:
            for D in DIMS:
                for R in RANGES:
                    for seed in SEEDS:
                        rs = np.random.RandomState(100000 * seed + 1000 * C + 10 * D + R)
                        a = rs.randint(0, R, (C, D)).astype(np.float64)
                        b = rs.randint(0, R, (max(C // 2, 1), D)).astype(np.float64)
                        f = dp.filter_pareto_front(a)
                        t = dp.filter_pareto_front(np.concatenate([a, b]))
                        with np.errstate(all="ignore"):
                            m = [dp.calculate_gd(t, f), dp.calculate_igd(t, f), dp.calculate_spread(f, t)]
                            nm = dp.normalized_data(f, t.max(axis=0))
                        meta.append([C, D, R, seed, len(b), len(f), len(t)])
                        metrics.append(m)
                        points.append(a.reshape(-1)); other.append(b.reshape(-1)); front.append(f.reshape(-1))
                        true_front.append(t.reshape(-1)); normal.append(np.asarray(nm, np.float64).reshape(-1))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt)
    np.savez_compressed(OUT, meta=np.asarray(meta, np.int32), metrics=np.asarray(metrics, np.float64), points=cat(points, np.int16),
                        other=cat(other, np.int16), front=cat(front, np.float64), true_front=cat(true_front, np.float64),
                        normalised=cat(normal, np.float64))
    print("%s: %d sets, %d bytes" % (OUT, len(meta), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
