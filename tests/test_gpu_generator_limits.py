"""GPU: the device instance generator (csrc/fjsp_generate.hip: generate_pack_kernel, generate_pack_dynamic_kernel,
generate_machine_kernel, generate_finish_kernel, the list and clear kernels of the masked refill) at the size limits
check_worst_case accepts -- the cases of tests/generator_limit_cases.py.

The reference is the host path on the same seeds, as in tests/test_gpu_generate.py: InstanceSet.generate_range + solve_fluid +
EnvBatch with the same variant, rng_seed and kernel family; tests/test_generator_limit_cases_host.py pins that host path to
the Python restatement of the stream on the same cases and proves the edge each case exists for.  Everything is compared bit
for bit: instance arrays (and the machine data of MO_DFJSP), instance_dims, the fluid tables of every env, the reset state,
every state / reward / done of the episode (the whole episode, or its first 64 steps where the case says so) and read().
No tolerance enters.  4 instances = 4 envs per case (8 for redraw_deep, 5 for the refills).

Wall time of every test on an MI355X (pytest --durations=0, the call phase; the whole module: 19 tests in 3.9 s):
    test_refills[kinds_256] 0.35 s          test_limit_case[kinds_256-v0] 0.25 s      test_refills[machines_32_p_max] 0.20 s
    test_limit_case[kinds_256_orders-v0] 0.20 s   [jobs_many-v0] 0.09 s   [stages_255-v0] 0.06 s   [two_by_128-v0] 0.06 s
    [kinds_255-v0] 0.05 s   [orders_16-v0] 0.04 s   [kinds_spread-v0] 0.04 s   [windows_max-v4] 0.03 s
    [machines_32_p_max-v0] 0.03 s   [machines_32_p_max-v5] 0.03 s   [rows_15_kinds-v0] 0.02 s   [rows_64_types-v0] 0.02 s
    [redraw_deep-v4] 0.01 s   [machines_32-v0] 0.01 s   test_job_count_at_the_lds_rule 0.02 s
    test_redraw_exhausted_is_named_and_the_next_create_succeeds 0.01 s

What the module sees that tests/test_gpu_generate.py does not, checked on builds of fjsp_generate.hip with one stored value
changed each (test_gpu_generate.py passes on all four):
    kind byte (r & 0x7F) in kB                    kinds_255, kinds_256_orders fail (kinds_256 alone does not: a batch that is
                                                  not single_job and has one order never reads the byte)
    machine bit 1u << (m & 15) in elig            machines_32, machines_32_p_max (both variants), windows_max, its refill fail
    processing time stored through a u8           machines_32_p_max (both variants), orders_16, windows_max, its refill fail
    job count of kind r stored at (r % 64)        kinds_256, kinds_spread, the kinds_256 refill fail
"""
import numpy as np
import pytest

from tests import generator_limit_cases as LC
from tests import helpers as H
from tests import test_gpu_generate_dynamic as TD
from tests import test_gpu_regenerate_masked as TM
from tests.test_gpu_generate import acts_for, episode, ops_of, pair, same_episode, same_instance, torch_gpu  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

RNG_SEED = 5


def run_id(run):
    return "%s-v%d" % run


def make_pair(c, variant, n=None, seed=None):
    n = c["n_inst"] if n is None else n
    return pair(c["params"], n, c["seed"] if seed is None else seed, variant=variant, family=c["family"], rng_seed=RNG_SEED)


def play(torch, b, T):
    """reset, T steps, read() (MO_DFJSP: its own action space, reward policy 1)."""
    return TD.episode(torch, b, T) if b.variant == LC.VARIANT_MO_DFJSP else episode(torch, b, T)


def same_batches(G, Hb, what):
    """Instances (with the machine data of a dynamic handle), their dims, the fluid tables of every env."""
    assert (G.kernel_family, G.state_size, G.n_inst, G.N) == (Hb.kernel_family, Hb.state_size, Hb.n_inst, Hb.N), what
    for i in range(G.n_inst):
        a, h = G.instance_arrays(i), Hb.instances.arrays(i)
        same_instance(a, h, "%s instance %d" % (what, i))
        assert G.instance_dims(i) == Hb.instance_dims(i), (what, i)
        if hasattr(h, "power"):
            TD.same_machine_data(a, h, "%s instance %d" % (what, i))
    for q in range(G.N):
        H.same(G.fluid_tables(q), Hb.fluid_tables(q), "%s fluid tables of env %d" % (what, q))


def routes(G):
    st = G.generated_stats()
    return st, (st["lp_device"], st["lp_global"], st["lp_host"])


@pytest.mark.parametrize("run", LC.GPU_RUNS, ids=run_id)
def test_limit_case(torch_gpu, run):
    torch = torch_gpu
    name, variant = run
    c = LC.CASES[name]
    what = run_id(run)
    G, Hb = make_pair(c, variant)
    if c["family"] is not None:
        assert G.kernel_family == c["family"] and G.row_build() == Hb.row_build(), what
    same_batches(G, Hb, what)
    arrs = [G.instance_arrays(i) for i in range(G.n_inst)]
    assert c["reaches"](arrs), what                  # the edge, on what the device made
    # ---- the LP routes: every instance on one list, the one the tableau rule says
    st, (n_lds, n_glob, n_host) = routes(G)
    n_fit = sum(1 for a in arrs if LC.tableau_fits(a))
    assert st["instances"] == G.n_inst and (n_lds, n_glob, n_host) == (n_fit, 0, G.n_inst - n_fit), (what, st)
    if c["route"]:
        assert (n_lds if c["route"] == "lds" else n_host) == G.n_inst, (what, st)
    if name == "redraw_deep":
        from deep_reinforcement_learning_for_fjsp_amd import instances as fi
        assert [a.seed_used for a in arrs] == [fi.dynamic_seed(c["params"], c["seed"] + i) for i in range(G.n_inst)], what
        assert sum(1 for i, a in enumerate(arrs) if a.seed_used != c["seed"] + i) == sum(1 for t in LC.REDRAW_ATTEMPTS if t > 0)
    # ---- the episode
    ops = ops_of(Hb)
    T = ops if c["steps"] is None else min(ops, c["steps"])
    eg, eh = play(torch, G, T), play(torch, Hb, T)
    if c["steps"] is None:
        assert np.all(eh[1]["done"] == 1), what
    same_episode(eg, eh, what=what)
    if Hb.instances.arrays(0).S > 1:                 # through every arrival, their LPs solved alike
        assert G.lp_solves == Hb.lp_solves > 0, what
    for q in range(G.N):
        H.same(G.fluid_tables(q), Hb.fluid_tables(q), "%s fluid tables of env %d after the episode" % (what, q))
    # ---- the row kernels: the fused rollout as well
    if c["family"] == 1:
        outs = []
        for b in (G, Hb):
            acts, mo = acts_for(torch, b, T, seed=32)
            b.reset()
            tr, rw, s = b.rollout(acts, mo=mo)
            outs.append(((H.host(tr), H.host(rw), H.host(s)), H.read(b)))
        H.same(outs[0], outs[1], what + " fused rollout")
        assert np.all(outs[0][1]["done"] == 1), what


@pytest.mark.parametrize("name", ["kinds_256", "machines_32_p_max"])
def test_refills(torch_gpu, name):
    """After an episode a whole refill, then a masked one of the first, the last and a middle instance of five: the new
    instances against the host on their seeds, the untouched ones keep their bytes and their envs play on as a twin's do
    (generate_clear_kernel at the largest record and env strides)."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    c = LC.CASES[name]
    prm, n = c["params"], 5
    A, B, D = c["seed"], c["seed"] + 1000, c["seed"] + 2000
    G = TM.generated(prm, n, A)
    play(torch, G, c["steps"] or ops_of(G))
    G.regenerate(B)
    assert bool(G.done.all()) and np.all(H.read(G)["done"] == 1)
    Hb = EnvBatch(LC.host_set(dict(c, seed=B, n_inst=n)), n, rng_seed=RNG_SEED)
    same_batches(G, Hb, name + " regenerated")
    H.same(H.host(G.reset()), H.host(Hb.reset()), name + " reset state after the regenerate")
    # ---- the masked refill, ten steps into the next episode
    twin = TM.generated(prm, n, B)
    t0, T = 10, prm.R_max * prm.J_max * prm.N_max
    acts, mo = acts_for(torch, G, t0 + T)
    TM.warm_up(G, twin, acts, t0)
    before = [G.instance_arrays(i) for i in range(n)]
    picked = [0, 2, 4]
    applied = H.host(G.regenerate_masked(D, TM.as_mask(torch, G, picked)))
    assert np.flatnonzero(applied).tolist() == picked
    assert [G.instance_seed(i) for i in range(n)] == [(D if i in picked else B) + i for i in range(n)]
    assert G.generated_stats()["instances"] == len(picked)
    for i in range(n):
        if i not in picked:
            same_instance(G.instance_arrays(i), before[i], "%s untouched instance %d" % (name, i))
        else:
            assert not np.array_equal(G.instance_arrays(i).p, before[i].p), i
    Ho = TM.oracle(G, prm, rng_seed=RNG_SEED)
    TM.same_made(G, Ho, applied, name)
    TM.play_on(torch, G, twin, Ho, applied, acts, mo, t0, name)


def test_redraw_exhausted_is_named_and_the_next_create_succeeds(torch_gpu):
    from deep_reinforcement_learning_for_fjsp_amd._capi import FJSP_E_UNSUPPORTED, FjspError
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    c = LC.CASES["redraw_exhausted"]
    with pytest.raises(FjspError) as host_err:
        LC.host_set(c, solve=False)
    with pytest.raises(FjspError) as err:
        EnvBatch.generated(c["params"], c["n_inst"], c["seed"], variant=LC.VARIANT_MO_DFJSP, rng_seed=RNG_SEED)
    named = "instance %d (seed %d)" % (LC.EXHAUSTED_INSTANCE, c["seed"] + LC.EXHAUSTED_INSTANCE)
    tail = "in each of 17 attempts (redraws = 16)"
    assert err.value.code == host_err.value.code == FJSP_E_UNSUPPORTED
    assert named in str(err.value) and named in str(host_err.value) and tail in str(err.value) and tail in str(host_err.value)
    d = LC.CASES["redraw_deep"]
    G = EnvBatch.generated(d["params"], d["n_inst"], d["seed"], variant=LC.VARIANT_MO_DFJSP, rng_seed=RNG_SEED)
    assert np.all(H.read(G)["done"] == 1) and G.instance_arrays(1).seed_used != d["seed"] + 1


def test_job_count_at_the_lds_rule(torch_gpu):
    """plan_layout's rule at KP = 64: four envs of a workgroup keep 1776 + 8 JP bytes (padded) each in 160 KiB of LDS, so
    JP = 4864 jobs is the last multiple of 64 that fits and 4928 the first that does not.  The rule is applied after the device
    is found (plan_batch), so this pair lives here and not in the host tests' REFUSED tables."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd._capi import FJSP_E_UNSUPPORTED, FjspError
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    at = lambda jobs: LC.gp(R_min=2, R_max=2, J_min=1, J_max=1, M=2, N_min=jobs // 2, N_max=jobs // 2)
    G, Hb = pair(at(4864), 2, LC.SEED, rng_seed=RNG_SEED)
    assert G.instance_dims(0)["jobs"] == 4864
    same_batches(G, Hb, "4864 jobs")
    same_episode(episode(torch, G, 16), episode(torch, Hb, 16), what="4864 jobs")
    with pytest.raises(FjspError) as err:
        EnvBatch.generated(at(4928), 2, LC.SEED)
    assert err.value.code == FJSP_E_UNSUPPORTED and "LDS staging: 4928 jobs" in str(err.value)
