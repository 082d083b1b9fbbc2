"""GPU: batches generated on the device from parameter RANGES (EnvBatch.generated with a GenRanges: every instance draws
its own machine count and due-date tightness) against the host path -- InstanceSet.generate_range(seed, ranges) +
solve_fluid + EnvBatch -- on the same seeds: the same instances, fluid tables and episodes, bit for bit.  Both handles run
the same kernels, so the one tolerance is the one tests/test_gpu_generate.py has: columns 4 and 6 of the
MO_FJSSP_discretes static state (host pow(d, 2.0), device d * d), within helpers.POW_RTOL.

Seeds are chosen on the CPU (the host generator and fjsp_gen_draw) so that a batch holds what its case is about: the
largest machine count of the range (the host handle is sized from its instances, the device handle from M_max: with it
both have the same padded width and the same builds), more than one M, both LP routes, a machine without operation.

Case 2 of the issue (M 10-20, R 3-4, J 3-4, 2-3 jobs per kind) asks for both LP routes in one call.  At those shapes no
tableau can miss the device: the largest (K = 16, R = 4, M = 20, every pair eligible) has 48 rows x 370 columns =
147 664 bytes of LDS against the limit of 159 744, and 370 columns against 512.  The case is kept at its shapes with
every other assertion (its LP counts are those computed on the CPU: all on the device), and the two routes in one call
are asserted by test_wave_both_lp_routes_in_one_call on R 3-6, J 3-5, where the tableaus of the larger instances (from
about 70 rows x 290 columns) pass that limit."""
import numpy as np
import pytest

from tests import helpers as H
from tests.test_gpu_generate import acts_for, episode, ops_of, pair, same_episode, same_instance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def rg(M_min, M_max, DDT_min=0.5, DDT_max=1.5, **kw):
    from deep_reinforcement_learning_for_fjsp_amd._capi import GenParams, GenRanges
    d = dict(M=0, p_min=1, p_max=20, N_min=1, N_max=1, S=1, DDT=0.0, t_si_min=100.0, t_si_max=200.0)
    d.update(kw)
    return GenRanges(GenParams(**d), M_min, M_max, DDT_min, DDT_max)


def rows_ranges():
    """One job per kind, at most 50 operation types and 10 jobs on 3 to 8 machines: the row kernels' batch."""
    return rg(3, 8, R_min=10, R_max=10, J_min=3, J_max=5)


def drawn(q, seed, n):
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    return [fi.draw_params(q, seed + i) for i in range(n)]


def seed_with_m_max(q, n, start=1000, also=lambda ps: True):
    """The first seed from `start` whose n instances include one of M_max machines (and whatever `also` asks of the draws)."""
    return next(s for s in range(start, start + 4000) if max(p.M for p in drawn(q, s, n)) == q.M_max and also(drawn(q, s, n)))


def tableau_fits(a, MP):
    """choose_lp_service's rule on the order-0 LP of instance arrays a in a batch padded to MP machines."""
    K, M, R, nx = a.K, a.M, a.R, int((np.asarray(a.p) > 0).sum())
    nr = K + M + (K - R)
    nc = nx + 1 + nr + 1
    lds = nr * nc * 8 + nc * 8 + 2 * nr * 8 + nr * 4 + K * M * 2 + K * 2 + nr * 2 + K * MP * 2 + K * 8 + 128
    return ((lds + 15) & ~15) <= 156 * 1024 and nc <= 512


def fits_on_cpu(q, seed, n):
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    s = fi.InstanceSet(n).generate_range(seed, q)
    return sum(1 if tableau_fits(s.arrays(i), q.M_max) else 0 for i in range(n))


def check_pair(torch, G, Hb, q, what, mo_static=False):
    """tests/test_gpu_generate.check_pair, with every instance's own M and DDT against fjsp_gen_draw."""
    assert (G.kernel_family, G.state_size) == (Hb.kernel_family, Hb.state_size), what
    n_fit = 0
    ps = drawn(q, G.seed_base + G.first_env, G.n_inst)
    for i in range(G.n_inst):
        a = G.instance_arrays(i)
        same_instance(a, Hb.instances.arrays(i), "%s instance %d" % (what, i))
        assert (a.M, a.ddt) == (ps[i].M, ps[i].DDT) and G.instance_dims(i)["M"] == ps[i].M, (what, i)
        n_fit += 1 if tableau_fits(a, q.M_max) else 0
    for i in range(G.N):
        H.same(G.fluid_tables(i), Hb.fluid_tables(i), "%s fluid tables of env %d" % (what, i))
    T = ops_of(G)
    assert T <= 200, (what, T)
    same_episode(episode(torch, G, T), episode(torch, Hb, T), mo_static, what)
    st = G.generated_stats()
    assert st["instances"] == G.n_inst and (st["lp_device"], st["lp_host"]) == (n_fit, G.n_inst - n_fit), (what, st, n_fit)
    return st, n_fit


def machines(G):
    return [G.instance_dims(i)["M"] for i in range(G.n_inst)]


# ---- 1. the row family ------------------------------------------------------------------------------------------------------
def test_rows(torch_gpu):
    q = rows_ranges()
    seed = seed_with_m_max(q, 32)
    G, Hb = pair(q, 32, seed)
    assert G.kernel_family == 1 and G.row_build() == Hb.row_build()
    assert len(set(machines(G))) > 1 and max(machines(G)) == 8
    check_pair(torch_gpu, G, Hb, q, "rows")
    # ... and the fused rollout
    T = ops_of(G)
    outs = []
    for b in (G, Hb):
        acts, mo = acts_for(torch_gpu, b, T, seed=32)
        b.reset()
        tr, rw, s = b.rollout(acts, mo=mo)
        outs.append(((H.host(tr), H.host(rw), H.host(s)), H.read(b)))
    H.same(outs[0], outs[1], "fused rollout")
    assert np.all(outs[0][1]["done"] == 1)


def test_rows_lean_build(torch_gpu):
    """A count that is no multiple of 4, the large-batch build: it reads kenv, which the device writes."""
    q = rows_ranges()
    seed = seed_with_m_max(q, 37)
    with H.env_var("FJSP_GROUP_EARLY", "0"):
        G, Hb = pair(q, 37, seed)
    assert G.kernel_family == 1 and G.row_build()["early"] == 0 and G.row_build() == Hb.row_build()
    assert len(set(machines(G))) > 1
    check_pair(torch_gpu, G, Hb, q, "lean rows")


def test_rows_need_m_max_of_at_most_eight(torch_gpu):
    from deep_reinforcement_learning_for_fjsp_amd._capi import FJSP_E_UNSUPPORTED, FjspError
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    q = rg(3, 9, R_min=10, R_max=10, J_min=3, J_max=5)
    with pytest.raises(FjspError) as err:
        EnvBatch.generated(q, 8, 7, family=1)
    assert err.value.code == FJSP_E_UNSUPPORTED and "does not fit the row kernels" in str(err.value)
    assert EnvBatch.generated(q, 8, 7).kernel_family == 0


# ---- 2. the wave family, more than eight machines, several jobs per kind ----------------------------------------------------
def test_wave_more_than_eight_machines_multi_job(torch_gpu):
    q = rg(10, 20, R_min=3, R_max=4, J_min=3, J_max=4, N_min=2, N_max=3)
    seed = seed_with_m_max(q, 32)
    n_fit_cpu = fits_on_cpu(q, seed, 32)
    G, Hb = pair(q, 32, seed)
    assert G.kernel_family == 0 and len(set(machines(G))) > 1
    assert any(int(G.instance_arrays(i).elig_n.max()) > 4 for i in range(32))       # beyond first4: the set-order path
    st, n_fit = check_pair(torch_gpu, G, Hb, q, "M 10-20, multi-job")
    assert n_fit == n_fit_cpu and (st["lp_device"], st["lp_host"]) == (n_fit_cpu, 32 - n_fit_cpu)
    assert st["device_pivots"] > 0


def test_wave_both_lp_routes_in_one_call(torch_gpu):
    q = rg(10, 20, R_min=3, R_max=6, J_min=3, J_max=5, N_min=2, N_max=3)
    seed = next(s for s in range(1000, 5000) if max(p.M for p in drawn(q, s, 32)) == 20 and 0 < fits_on_cpu(q, s, 32) < 32)
    n_fit_cpu = fits_on_cpu(q, seed, 32)
    G, Hb = pair(q, 32, seed)
    st, n_fit = check_pair(torch_gpu, G, Hb, q, "M 10-20, both LP routes")
    assert 0 < n_fit_cpu < 32 and n_fit == n_fit_cpu
    assert (st["lp_device"], st["lp_host"]) == (n_fit_cpu, 32 - n_fit_cpu) and st["device_pivots"] > 0


# ---- 3. a range that crosses 8 ---------------------------------------------------------------------------------------------
def test_range_across_eight_machines(torch_gpu):
    q = rg(6, 12, R_min=4, R_max=6, J_min=3, J_max=4)
    seed = seed_with_m_max(q, 32, also=lambda ps: min(p.M for p in ps) <= 8)
    G, Hb = pair(q, 32, seed)
    ms = machines(G)
    assert G.kernel_family == 0 and min(ms) <= 8 < max(ms) == 12        # M <= 8 instances in a batch whose MP > 8
    check_pair(torch_gpu, G, Hb, q, "M 6-12")


# ---- 4. degenerate ends ----------------------------------------------------------------------------------------------------
def test_one_or_two_machines(torch_gpu):
    q = rg(1, 2, R_min=1, R_max=1, J_min=1, J_max=1, p_max=2)
    seed = seed_with_m_max(q, 8, also=lambda ps: min(p.M for p in ps) == 1)
    G, Hb = pair(q, 8, seed)
    assert sorted(set(machines(G))) == [1, 2]
    a = G.instance_arrays(machines(G).index(1))
    assert (a.R, a.K, a.M) == (1, 1, 1)
    check_pair(torch_gpu, G, Hb, q, "M 1-2, 1 x 1")


def test_point_range_is_the_fixed_parameter_batch(torch_gpu):
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    from tests.test_gpu_generate import gp
    base = dict(R_min=3, R_max=5, J_min=2, J_max=3, N_min=1, N_max=2)
    q = rg(6, 6, 1.25, 1.25, **base)
    G, Hb = pair(q, 16, 40)
    check_pair(torch_gpu, G, Hb, q, "point range")
    # two fresh handles: an env's random stream runs on across episodes, and G has played one
    P, F = EnvBatch.generated(q, 16, 40, rng_seed=5), EnvBatch.generated(gp(M=6, DDT=1.25, **base), 16, 40, rng_seed=5)
    assert (F.kernel_family, F.step_bytes) == (P.kernel_family, P.step_bytes)
    for i in range(16):
        same_instance(P.instance_arrays(i), F.instance_arrays(i), "instance %d" % i)
    T = ops_of(P)
    H.same(episode(torch_gpu, P, T), episode(torch_gpu, F, T), "point range against fixed parameters")
    assert P.generated_stats()["lp_device"] == F.generated_stats()["lp_device"]


# ---- 5. each variant the generator supports --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["SO_DFJSP", "SO_SFJSP", "MO_FJSSP_discretes"])
def test_each_variant(torch_gpu, name):
    from deep_reinforcement_learning_for_fjsp_amd import batch as B, instances as fi
    variant = {"SO_DFJSP": B.VARIANT_SO_DFJSP, "SO_SFJSP": B.VARIANT_SO_SFJSP, "MO_FJSSP_discretes": B.VARIANT_MO_FJSSP_DISCRETES}[name]
    q = rows_ranges()

    def playable(s):            # SO_DFJSP: every machine of every instance has an operation
        hs = fi.InstanceSet(16).generate_range(s, q)
        return all(np.all((hs.arrays(i).p > 0).sum(0) > 0) for i in range(16))
    seed = next(s for s in range(1000, 5000) if max(p.M for p in drawn(q, s, 16)) == 8 and playable(s))
    G, Hb = pair(q, 16, seed, variant=variant)
    assert len(set(machines(G))) > 1
    check_pair(torch_gpu, G, Hb, q, name, mo_static=name == "MO_FJSSP_discretes")
    if name == "MO_FJSSP_discretes":
        st, ps = H.host(G.reset()), drawn(q, seed, 16)
        assert np.array_equal(H.bits(st[:, 0]), H.bits(np.array([p.DDT for p in ps])))
        assert np.array_equal(st[:, 1], np.array([float(p.M) for p in ps]))


def test_failing_instance_is_named_and_the_handle_recovers(torch_gpu):
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd._capi import FJSP_E_STATE, FJSP_E_UNSUPPORTED, FjspError
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, VARIANT_SO_DFJSP
    q = rg(2, 3, R_min=1, R_max=1, J_min=1, J_max=1)
    # one operation type with n ~ U{1..M} eligible machines: SO_DFJSP cannot play n < M (a machine divides by zero)

    def empty(s):
        return bool(np.any((fi.InstanceSet(1).generate(0, s, q).arrays(0).p > 0).sum(0) == 0))
    bad = next(s for s in range(1000, 3000) if not empty(s) and empty(s + 1))
    good = next(s for s in range(1000, 3000) if not empty(s) and not empty(s + 1)
                and {fi.draw_params(q, s).M, fi.draw_params(q, s + 1).M} == {2, 3})
    with pytest.raises(FjspError) as err:
        EnvBatch.generated(q, 2, bad, variant=VARIANT_SO_DFJSP)
    assert err.value.code == FJSP_E_UNSUPPORTED and "instance 1 (seed %d)" % (bad + 1) in str(err.value)
    G = EnvBatch.generated(q, 2, good, variant=VARIANT_SO_DFJSP)
    with pytest.raises(FjspError) as err:
        G.regenerate(bad)
    assert err.value.code == FJSP_E_UNSUPPORTED and "instance 1 (seed %d)" % (bad + 1) in str(err.value)
    for refused in (G.reset, G.read, lambda: G.fluid_tables(0), lambda: G.instance_arrays(0)):
        with pytest.raises(FjspError) as err:
            refused()
        assert err.value.code == FJSP_E_STATE
    G.regenerate(good)
    G.reset()
    assert np.all(H.read(G)["done"] == 0)


# ---- 6. regenerate in place ------------------------------------------------------------------------------------------------
def test_regenerate_in_place(torch_gpu):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    q = rg(6, 12, R_min=4, R_max=6, J_min=3, J_max=4)
    A, Bs, n = 7, 5000, 32
    G = EnvBatch.generated(q, n, A, rng_seed=3)
    acts, _ = acts_for(torch, G, 5)
    G.reset()
    for t in range(5):
        G.step(acts[t])
    under_a = [G.instance_arrays(i) for i in range(n)]
    G.regenerate(Bs)
    assert bool(G.done.all()) and np.all(H.read(G)["done"] == 1)
    assert [G.instance_dims(i)["M"] for i in range(n)] == [p.M for p in drawn(q, Bs, n)] != [a.M for a in under_a]
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    G.regenerate(A)
    for k in range(8):
        G.regenerate(Bs + k)
    G.regenerate(A)
    torch.cuda.synchronize()
    assert abs(torch.cuda.mem_get_info()[0] - free0) <= 2 << 20, "device memory moved across ten regenerates"
    for i in range(n):
        same_instance(G.instance_arrays(i), under_a[i], "instance %d after A, B, A" % i)
    T = ops_of(G)
    H.same(episode(torch, G, T), episode(torch, EnvBatch.generated(q, n, A, rng_seed=3), T), "episode after A, B, A")


# ---- 7. shards -------------------------------------------------------------------------------------------------------------
def test_shards_are_slices_of_the_whole_batch(torch_gpu):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    q = rg(6, 12, R_min=4, R_max=6, J_min=3, J_max=4)
    whole = EnvBatch.generated(q, 32, 7, rng_seed=9)
    shards = [EnvBatch.generated(q, 16, 7, rng_seed=9, first_env=f) for f in (0, 16)]
    for i in range(32):
        same_instance(whole.instance_arrays(i), shards[i // 16].instance_arrays(i % 16), "instance %d" % i)
    assert len(set(machines(shards[1]))) > 1
    T = ops_of(whole)
    (sw, rw), parts = episode(torch, whole, T), [episode(torch, s, T) for s in shards]
    cat = lambda xs: np.concatenate(xs, 0)
    H.same(sw[0], cat([p[0][0] for p in parts]), "reset state")
    for t in range(1, T + 1):
        H.same(list(sw[t]), [cat([p[0][t][k] for p in parts]) for k in range(3)], "step %d" % t)
    H.same(rw, {k: cat([p[1][k] for p in parts]) for k in rw}, "read()")
    shards[1].regenerate(8)
    whole.regenerate(8)
    for i in range(16):
        same_instance(whole.instance_arrays(16 + i), shards[1].instance_arrays(i), "instance %d after a regenerate" % (16 + i))


# ---- 8. snapshots and recording --------------------------------------------------------------------------------------------
def test_snapshot_follows_the_seeds_and_the_ranges(torch_gpu):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd._capi import FjspError
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    from tests.test_gpu_generate import gp
    q = rows_ranges()
    G, G2 = EnvBatch.generated(q, 16, 7, rng_seed=3), EnvBatch.generated(q, 16, 7, rng_seed=3)
    acts, _ = acts_for(torch, G, 4)
    G.reset()
    for t in range(4):
        G.step(acts[t])
    snap = G.snapshot()
    G2.restore(snap, check=True)
    assert snap.errors() == 0
    H.same(H.read(G), H.read(G2), "restored into a handle generated alike")
    G2.regenerate(8)
    with pytest.raises(FjspError) as err:
        G2.restore(snap)
    assert "not compatible with the snapshot" in str(err.value)
    # other ranges over the same base, same seeds
    with pytest.raises(FjspError) as err:
        EnvBatch.generated(rg(3, 8, 0.5, 1.25, R_min=10, R_max=10, J_min=3, J_max=5), 16, 7, rng_seed=3).restore(snap)
    assert "not compatible with the snapshot" in str(err.value)
    # a point range makes the instances of the fixed parameter set, record for record: the fingerprints still differ
    base = dict(R_min=10, R_max=10, J_min=3, J_max=5)
    P, F = EnvBatch.generated(rg(5, 5, 1.0, 1.0, **base), 16, 7, rng_seed=3), EnvBatch.generated(gp(M=5, DDT=1.0, **base), 16, 7, rng_seed=3)
    assert (P.kernel_family, P.row_build()) == (F.kernel_family, F.row_build())
    P.reset()
    snap_p = P.snapshot()
    with pytest.raises(FjspError) as err:
        F.restore(snap_p)
    assert "not compatible with the snapshot" in str(err.value)
    F.reset()
    with pytest.raises(FjspError) as err:
        P.restore(F.snapshot())
    assert "not compatible with the snapshot" in str(err.value)


def test_recording_survives_a_regenerate(torch_gpu):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import schedule as S
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    q = rg(6, 12, R_min=4, R_max=6, J_min=3, J_max=4, N_min=1, N_max=2)
    G = EnvBatch.generated(q, 16, 7)
    cap = G.record_schedule()
    assert cap == 48                      # the ranges' worst case: 6 kinds x 4 operations x 2 jobs
    G.regenerate(8)
    assert G.record_schedule() == cap
    T = ops_of(G)
    episode(torch, G, T)
    table, length = [H.host(x) for x in G.schedule()]
    for i in range(16):
        a = G.instance_arrays(i)
        assert length[i] == int((a.count.reshape(1, a.R) * a.Jr[None, :]).sum())
        assert S.validate(a, table[i, :length[i]].astype(np.int64), 0) == [], i


# ---- 9. the Batched* classes -----------------------------------------------------------------------------------------------
def test_batched_classes_take_ranges(torch_gpu):
    from deep_reinforcement_learning_for_fjsp_amd import environments as E, instances as fi
    from deep_reinforcement_learning_for_fjsp_amd._capi import FJSP_E_UNSUPPORTED, FjspError
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    q = rows_ranges()

    def playable(s):            # BatchedSODFJSP: every machine of every instance has an operation
        hs = fi.InstanceSet(8).generate_range(s, q)
        return all(np.all((hs.arrays(i).p > 0).sum(0) > 0) for i in range(8))
    s0, s1 = [s for s in range(1000, 5000) if playable(s)][:2]
    for cls in (E.BatchedSOFJSSP, E.BatchedSODFJSP, E.BatchedSOSFJSP, E.BatchedMOFJSSP):
        env = cls(q, 8, seed_base=s0, rng_seed=2)
        twin = EnvBatch.generated(q, 8, s0, variant=cls.variant, rng_seed=2)
        assert env.batch.variant == cls.variant and env.N == 8 and len(set(machines(env.batch))) > 1
        H.same(H.host(env.reset()), H.host(twin.reset()), cls.__name__)
        env.batch.regenerate(s1)
        assert not np.array_equal(env.batch.instance_arrays(0).p, twin.instance_arrays(0).p)
    with pytest.raises(FjspError) as err:
        E.BatchedMODFJSP(q, 8, seed_base=s0)
    assert err.value.code == FJSP_E_UNSUPPORTED and "MO_DFJSP needs machine data" in str(err.value)
    with pytest.raises(ValueError):
        E.BatchedSOFJSSP(q)


def test_decoders_take_a_ranges_batch(torch_gpu):
    from deep_reinforcement_learning_for_fjsp_amd import lookahead as L
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    G = EnvBatch.generated(rows_ranges(), 16, 7)
    G.reset()
    L.rollout_dispatch(G, H.DET_SO[:3], "makespan")
    r = H.read(G)
    assert np.all(r["done"] == 1) and np.all(r["status"] == 0)
    assert G.machine_time_end().shape == (16, 8)
