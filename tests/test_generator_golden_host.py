"""The host generator against its recorded instances (tests/golden/generator_streams.npz, written by
tests/golden/make_generator_golden.py at the last commit whose fjsp_instance.cpp walked a sequential stream of its own):
every parameter set, 64 seeds each -- return code, digest of the shop, bits of the due-date tightness, and for MO_DFJSP sets
the seed the instance was made of and its machine data.  The device generator compiles the same statement of the stream
(csrc/fjsp_gen_stream.h) and is compared with the host bit for bit by the test_gpu_generate*.py files."""
import os

import numpy as np
import pytest

from deep_reinforcement_learning_for_fjsp_amd import _capi
from tests.golden import make_generator_golden as G

GOLDEN = np.load(G.OUT, allow_pickle=False)
SETS = G.param_sets()


def test_the_file_holds_every_set_and_the_branches_it_is_there_for():
    assert list(GOLDEN["sets"]) == list(SETS) and os.path.getsize(G.OUT) < (1 << 20)
    for name in SETS:
        rc = GOLDEN[name + "_rc"]
        assert rc.shape == (G.N_SEEDS,)
        if name == "dynamic_refused":
            assert (rc == _capi.FJSP_E_UNSUPPORTED).any() and np.isin(rc, (0, _capi.FJSP_E_UNSUPPORTED)).all()
        else:
            assert not rc.any(), name
    assert (GOLDEN["dynamic_redraw_seed_used"] != GOLDEN["dynamic_redraw_seed"]).any()


@pytest.mark.parametrize("name", list(SETS))
def test_the_host_generator_makes_the_recorded_instances(name):
    got = G.record(name, list(SETS).index(name), SETS[name])
    assert sorted(got) == sorted(k for k in GOLDEN.files if k.startswith(name + "_") and k[len(name) + 1:] in
                                 ("seed", "rc", "digest", "ddt", "seed_used", "machine", "machine_at"))
    for key in ("seed", "rc", "seed_used", "ddt", "digest", "machine_at"):
        k = "%s_%s" % (name, key)
        if k in got:
            bad = np.flatnonzero(got[k] != GOLDEN[k]) if got[k].shape == GOLDEN[k].shape else "shape"
            assert got[k].dtype == GOLDEN[k].dtype and not len(bad), (k, "seeds / entries that differ", bad)
    if name + "_machine" in got:
        at, a, b = GOLDEN[name + "_machine_at"], got[name + "_machine"], GOLDEN[name + "_machine"]
        bad = [i for i in range(G.N_SEEDS) if not np.array_equal(a[at[i]:at[i + 1]], b[at[i]:at[i + 1]])]
        assert a.dtype == b.dtype and a.shape == b.shape and not bad, (name, "machine data differ at seeds", bad)
