"""Recorded instances of the HOST generator: tests/golden/generator_streams.npz.

The host generator (csrc/fjsp_instance.cpp) and the device generator (csrc/fjsp_generate.hip) compile one statement of the
draw stream and of the shop, csrc/fjsp_gen_stream.h.  This file pins what the host generator made of a seed at commit
00686ef, the last one at which fjsp_instance.cpp walked a sequential stream of its own: for every parameter set of
param_sets() and 64 consecutive seeds the return code, a digest of the shop, the bits of the due-date tightness and, for
MO_DFJSP sets, the seed the instance was made of and its machine data.  tests/test_generator_golden_host.py records the
same from the library under test and compares.  Needs no GPU.

    FJSP_AMD_LIB=<library of the commit> python tests/golden/make_generator_golden.py --commit <hash>     # (re)write the file
    python tests/golden/make_generator_golden.py --compare         # record from the tree's library and check against the file

Layout of generator_streams.npz: commit, sets (their names) and per set, with N = 64 seeds
    <set>_seed       u64[N]   the seeds
    <set>_rc         i32[N]   what the generate call returned (0 or a negative FJSP_E_* code; the rest is 0 where it failed)
    <set>_digest     u64[N]   BLAKE2b-64 over R, M, K, S and the int32 arrays Jr, p, elig_n, elig_list, count, arrive, delivery
    <set>_ddt        u64[N]   the bit pattern of ddt
    <set>_seed_used  u64[N]   MO_DFJSP sets: fjsp_gen_dynamic_seed
    <set>_machine    i32[..]  MO_DFJSP sets: power, idle_power, bk_n, bk of every instance, flattened, one behind the other
    <set>_machine_at i64[N+1] where instance i's lie in <set>_machine

The sets: the three of tests/test_generate_host.py, the reference's training distributions (reference_training_ranges,
reference_order_ranges, reference_dynamic_ranges), and edge sets at which each shared function meets a boundary:
    one_machine        M = 1: every shuffle draw is randint(0, 0), every list has one entry
    machines_32        M = 32, the most a record holds
    types_beyond_64    R_max x J_max = 80 operation types: more than one chunk of a wave's lanes
    orders_16_tied     S = 16 orders all arriving at 0 (t_si = 0), one or two jobs of two kinds: the sort meets ties
    ddt_signed         DDT_min < 0 < DDT_max: delivery times of either sign, truncated towards zero
    one_job            N_min = N_max = 1
    dynamic_no_windows MO_DFJSP with W_max = 0
    dynamic_windows    MO_DFJSP with up to three breakdown windows per machine
    dynamic_redraw     one kind of 2..4 operations on four machines, redraws = 16: instances are drawn again
    dynamic_refused    the same with redraws = 0: instances are refused (FJSP_E_UNSUPPORTED)
build() asserts that dynamic_redraw holds a seed that was drawn again, that dynamic_refused holds a refused one, and that no
other set holds a failing seed: otherwise nothing would pin those branches.
"""
import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests.golden.make_ppo_round_golden import differences, serialise      # noqa: E402

OUT = os.path.join(HERE, "generator_streams.npz")
N_SEEDS = 64
SHOP_KEYS = ("Jr", "p", "elig_n", "elig_list", "count", "arrive", "delivery")
MACHINE_KEYS = ("power", "idle_power", "bk_n", "bk")


def param_sets():
    """name -> GenParams / GenRanges / GenOrders / GenDynamic, in the file's order."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd._capi import GenDynamic, GenMachine, GenOrders, GenParams, GenRanges
    from tests.test_generate_host import PARAM_SETS

    def base(**kw):
        d = dict(R_min=2, R_max=3, J_min=1, J_max=3, M=4, p_min=1, p_max=9, N_min=1, N_max=2, S=1, DDT=1.0, t_si_min=100.0, t_si_max=200.0)
        d.update(kw)
        return GenParams(**d)

    def few_types(redraws):
        return GenDynamic(GenOrders(GenRanges(base(R_min=1, R_max=1, J_min=2, J_max=4), 4, 4, 0.5, 1.5), 1, 2),
                          GenMachine(10, 200, 1, 9, 2, 1, 60, 1, 30), redraws)

    sets = {name: PARAM_SETS[name] for name in sorted(PARAM_SETS)}
    sets["training_mpppo"] = fi.reference_training_ranges("mpppo")
    sets["training_ddqn"] = fi.reference_training_ranges("ddqn")
    sets["orders_da3c"] = fi.reference_order_ranges("da3c")
    sets["orders_hmpsac"] = fi.reference_order_ranges("hmpsac")
    sets["dynamic_hmpsac"] = fi.reference_dynamic_ranges("hmpsac")
    sets["one_machine"] = base(M=1)
    sets["machines_32"] = base(M=32, J_min=2)
    sets["types_beyond_64"] = base(R_min=14, R_max=16, J_min=4, J_max=5)
    sets["orders_16_tied"] = GenOrders(GenRanges(base(R_min=2, R_max=2, J_max=2, t_si_min=0.0, t_si_max=0.0), 3, 5, 0.5, 1.5), 16, 16)
    sets["ddt_signed"] = GenRanges(base(), 3, 6, -1.0, 1.5)
    sets["one_job"] = GenOrders(GenRanges(base(N_max=1), 3, 6, 0.5, 1.5), 1, 3)
    sets["dynamic_no_windows"] = GenDynamic(GenOrders(GenRanges(base(R_min=3, J_min=2), 3, 6, 0.5, 1.5), 1, 3), GenMachine(10, 200, 1, 9, 0, 1, 60, 1, 30), 8)
    sets["dynamic_windows"] = GenDynamic(GenOrders(GenRanges(base(R_min=3, J_min=2), 3, 6, 0.5, 1.5), 1, 3), GenMachine(10, 200, 1, 9, 3, 1, 60, 1, 30), 8)
    sets["dynamic_redraw"] = few_types(16)
    sets["dynamic_refused"] = few_types(0)
    return sets


def seed_base(index):
    return 31000 + 1000 * index


def record(name, index, q):
    """The file's arrays of one set, from the library the binding loads."""
    from deep_reinforcement_learning_for_fjsp_amd import _capi, instances as fi
    from deep_reinforcement_learning_for_fjsp_amd._capi import GenDynamic, GenOrders, GenRanges
    lib = _capi.lib()
    dynamic = isinstance(q, GenDynamic)
    call = (lib.fjsp_instances_generate_dynamic if dynamic else lib.fjsp_instances_generate_orders if isinstance(q, GenOrders) else
            lib.fjsp_instances_generate_drawn if isinstance(q, GenRanges) else lib.fjsp_instances_generate)
    seeds = np.arange(seed_base(index), seed_base(index) + N_SEEDS, dtype=np.uint64)
    rc, digest, ddt = np.zeros(N_SEEDS, np.int32), np.zeros(N_SEEDS, np.uint64), np.zeros(N_SEEDS, np.uint64)
    used, machine, at = np.zeros(N_SEEDS, np.uint64), [], [0]
    s = fi.InstanceSet(N_SEEDS)
    for i, seed in enumerate(seeds.tolist()):
        rc[i] = call(s.handle, i, seed, C.byref(q))
        if rc[i] == 0:
            a = s.arrays(i)
            h = hashlib.blake2b(np.array([a.R, a.M, a.K, a.S], np.int32).tobytes(), digest_size=8)
            for key in SHOP_KEYS:
                v = getattr(a, key)
                assert v.dtype == np.int32, key
                h.update(np.ascontiguousarray(v).tobytes())
            digest[i] = int.from_bytes(h.digest(), "little")
            ddt[i] = np.array([a.ddt], np.float64).view(np.uint64)[0]
            if dynamic:
                used[i] = fi.dynamic_seed(q, seed)
                machine += [np.ascontiguousarray(getattr(a, key), dtype=np.int32).ravel() for key in MACHINE_KEYS]
        at.append(sum(len(m) for m in machine))
    out = {"seed": seeds, "rc": rc, "digest": digest, "ddt": ddt}
    if dynamic:
        out.update(seed_used=used, machine=np.concatenate(machine) if machine else np.zeros(0, np.int32), machine_at=np.array(at, np.int64))
    return {"%s_%s" % (name, k): v for k, v in out.items()}


def build(commit):
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    sets = param_sets()
    store = {"commit": np.array(commit), "sets": np.array(list(sets))}
    for index, (name, q) in enumerate(sets.items()):
        got = record(name, index, q)
        rc = got[name + "_rc"]
        redrawn = int((got[name + "_seed_used"][rc == 0] != got[name + "_seed"][rc == 0]).sum()) if name + "_seed_used" in got else 0
        print("%-19s failed %2d  drawn again %2d" % (name, int((rc != 0).sum()), redrawn))
        if name == "dynamic_refused":
            assert (rc == _capi.FJSP_E_UNSUPPORTED).any() and np.isin(rc, (0, _capi.FJSP_E_UNSUPPORTED)).all(), rc
        else:
            assert not rc.any(), (name, rc)
        if name == "dynamic_redraw":
            assert redrawn > 0
        store.update(got)
    return store


def _head():
    try:
        return subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=REPO, stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit the library was built at (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--compare", action="store_true", help="record from the tree's library and check against generator_streams.npz")
    args = ap.parse_args()
    if args.compare:
        old = np.load(OUT, allow_pickle=False)
        bad = differences(old, build(str(old["commit"])))
        if bad:
            print("generator_streams.npz DIFFERS from this library's instances: %s" % ", ".join(bad))
            sys.exit(1)
        print("generator_streams.npz (written at %s) holds this library's instances" % str(old["commit"]))
        return
    commit = args.commit or _head()
    if not commit:
        sys.exit("--commit is needed: this tree is no git checkout")
    store = build(commit)
    with open(args.out, "wb") as f:
        f.write(serialise(store))
    print("wrote %s at %s (%d bytes)" % (args.out, commit, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
