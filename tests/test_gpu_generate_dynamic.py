"""GPU: MO_DFJSP batches generated on the device (EnvBatch.generated with a GenDynamic, fjsp_env_create_generated_dynamic)
against the host path -- InstanceSet.generate_range + solve_fluid + EnvBatch(variant=MO_DFJSP) -- on the same seeds and
rng_seed: the same instances with their machine data, per-env fluid tables and episodes (30 state columns, reward, done)
through every order arrival and breakdown window, and the same read() with its energy, bit for bit.  Both handles run the
same kernels and pivot-identical LP services, so no tolerance applies.  Every case: 8 instances shared by 16 envs, R = 3,
J 2..3, p 5..30, N 2..3, t_si 100..200, window gaps 1..60 and lengths 1..30, every episode played to its end."""
import numpy as np
import pytest

from tests import helpers as H
from tests.test_generate_dynamic_host import DYN_KEYS, REDRAW_BASE, dyn, idle_in_attempt_0, machine, redraw_shape
from tests.test_gpu_generate import ops_of, same_instance, torch_gpu  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

N_INST, N_ENVS = 8, 16
FIXED = dict(S_min=2, S_max=2, M_min=4, M_max=4, DDT_min=1.0, DDT_max=1.0)
DRAWN = dict(S_min=1, S_max=3, M_min=3, M_max=6, DDT_min=0.5, DDT_max=1.5)


def host_batch(q, seed, rng_seed=5):
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, VARIANT_MO_DFJSP
    return EnvBatch(fi.InstanceSet(N_INST).generate_range(seed, q).solve_fluid(), N_ENVS, variant=VARIANT_MO_DFJSP, rng_seed=rng_seed)


def generated(q, seed, rng_seed=5):
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, VARIANT_MO_DFJSP
    return EnvBatch.generated(q, N_ENVS, seed, n_inst=N_INST, variant=VARIANT_MO_DFJSP, rng_seed=rng_seed)


def acts_for(torch, b, T, seed=31):
    from deep_reinforcement_learning_for_fjsp_amd.batch import global_actions
    return torch.from_numpy(global_actions(seed, b.first_env, b.N, T, 12, 10)).cuda()         # MO_DFJSP: 12 task rules x 10 machine rules


def mo_rows(torch, b, policy, norm=(0.0, 0.0, 0.0)):
    return torch.tensor([[float(policy)] + list(norm)], dtype=torch.float64, device="cuda").repeat(b.N, 1)


def episode(torch, b, T, mo=None, seed=31):
    """reset, T per-step steps, read(): everything a caller sees (mo None: reward policy 1)."""
    acts = acts_for(torch, b, T, seed)
    out = [H.host(b.reset())]
    for t in range(T):
        st, rw, dn = b.step(acts[t], mo=mo)
        out.append((H.host(st), H.host(rw), H.host(dn)))
    return out, H.read(b)


def same_machine_data(a, b, what):
    for key in DYN_KEYS:
        x, y = getattr(a, key), getattr(b, key)
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), (what, key)


def same_instances(G, Hb, what):
    for i in range(G.n_inst):
        a, h = G.instance_arrays(i), Hb.instances.arrays(i)
        same_instance(a, h, "%s instance %d" % (what, i))
        same_machine_data(a, h, "%s instance %d" % (what, i))
        assert G.instance_dims(i) == Hb.instance_dims(i), (what, i)


def check_pair(torch, G, Hb, what, mo=None):
    """Instances with their machine data, the fluid tables of every env, every state / reward / done of whole episodes, read()."""
    assert (G.kernel_family, G.state_size, G.n_inst, G.N) == (Hb.kernel_family, Hb.state_size, Hb.n_inst, Hb.N) == (0, 30, N_INST, N_ENVS), what
    same_instances(G, Hb, what)
    for i in range(G.N):
        H.same(G.fluid_tables(i), Hb.fluid_tables(i), "%s fluid tables of env %d" % (what, i))
    T = ops_of(Hb)
    eg, eh = episode(torch, G, T, mo), episode(torch, Hb, T, mo)
    assert np.all(eh[1]["done"] == 1) and eh[0][1][0].shape == (N_ENVS, 30), what
    assert "energy_consumption" in eh[1] and np.all(eh[1]["energy_consumption"] > 0), what
    H.same(eg, eh, what)
    for i in range(G.N):
        H.same(G.fluid_tables(i), Hb.fluid_tables(i), "%s fluid tables of env %d after the episode" % (what, i))
    st = G.generated_stats()
    assert st["instances"] == G.n_inst and st["lp_device"] + st["lp_host"] + st["lp_global"] == G.n_inst, st
    return eg


# ---- 1, 2: the generator ------------------------------------------------------------------------------------------------------
def test_fixed(torch_gpu):
    q = dyn(**FIXED)
    G, Hb = generated(q, 40), host_batch(q, 40)
    assert G.lp_on_device == Hb.lp_on_device == 0            # 16 envs: the host service on both
    check_pair(torch_gpu, G, Hb, "M = 4, S = 2, W_max = 3")
    assert G.lp_solves > 0 and G.lp_solves == Hb.lp_solves
    a = G.instance_arrays(0)
    assert (a.M, a.S) == (4, 2) and a.power.shape == (a.K, 4) and a.seed_used == 40
    assert sum(int(G.instance_arrays(i).bk_n.sum()) for i in range(N_INST)) > 0


def test_drawn(torch_gpu):
    q = dyn(**DRAWN)
    Hb = host_batch(q, 60)
    arrs = [Hb.instances.arrays(i) for i in range(N_INST)]
    assert len({a.M for a in arrs}) > 1 and len({a.S for a in arrs}) > 1
    assert any(0 in a.bk_n for a in arrs) and any(a.bk_n.max() == 3 for a in arrs)
    check_pair(torch_gpu, generated(q, 60), Hb, "M 3..6, S 1..3")


# ---- 3: the windows take effect -------------------------------------------------------------------------------------------------
def test_windows_change_the_episode(torch_gpu):
    q0, q3 = dyn(mc=machine(0), **DRAWN), dyn(mc=machine(3), **DRAWN)
    G0, G3 = generated(q0, 60), generated(q3, 60)
    for i in range(N_INST):
        a, b = G0.instance_arrays(i), G3.instance_arrays(i)
        same_instance(a, b, "instance %d" % i)
        assert np.array_equal(a.power, b.power) and np.array_equal(a.idle_power, b.idle_power), i
        assert a.bk.shape == (0, 2) and not a.bk_n.any(), i
    e0 = check_pair(torch_gpu, G0, host_batch(q0, 60), "W_max = 0")
    e3 = check_pair(torch_gpu, G3, host_batch(q3, 60), "W_max = 3")
    states = lambda e: np.stack([x[0] for x in e[0][1:]])
    assert not np.array_equal(states(e0), states(e3))
    assert not np.array_equal(e0[1]["energy_consumption"], e3[1]["energy_consumption"])


# ---- 4: reward policy 3 -----------------------------------------------------------------------------------------------------------
def test_reward_policy_3(torch_gpu):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import environments as E
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    q = dyn(**DRAWN)
    g = E.BatchedMODFJSP(q, N_ENVS, n_inst=N_INST, seed_base=60, rng_seed=5)
    h = E.BatchedMODFJSP(fi.InstanceSet(N_INST).generate_range(60, q).solve_fluid(), N_ENVS, rng_seed=5)
    for env in (g, h):
        env.set_objective(3, completion=900.0, tardiness=400.0, energy_consumption=250000.0)
    T = ops_of(h.batch)
    acts = acts_for(torch, g.batch, T)
    H.same(H.host(g.reset()), H.host(h.reset()), "reset")
    rewards = []
    for t in range(T):
        og, oh = g.step(acts[t]), h.step(acts[t])
        H.same([H.host(x) for x in og], [H.host(x) for x in oh], "step %d" % t)
        rewards.append(H.host(og[1]))
    H.same(H.read(g.batch), H.read(h.batch), "read()")
    # ... and policy 3 is not policy 1: the same actions earn other rewards
    p1 = episode(torch, generated(q, 60), T)
    assert not np.array_equal(np.stack(rewards), np.stack([x[1] for x in p1[0][1:]]))


# ---- 5: redraw on the device ------------------------------------------------------------------------------------------------------
def test_redraw_on_the_device(torch_gpu):
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd._capi import FJSP_E_UNSUPPORTED, FjspError
    q = redraw_shape()
    idle = [i for i in range(N_INST) if idle_in_attempt_0(q, REDRAW_BASE + i)]
    assert len(idle) >= 2
    G, Hb = generated(q, REDRAW_BASE), host_batch(q, REDRAW_BASE)
    for i in range(N_INST):
        used = G.instance_arrays(i).seed_used
        assert used == fi.dynamic_seed(q, REDRAW_BASE + i) and (used != REDRAW_BASE + i) == (i in idle), i
    check_pair(torch_gpu, G, Hb, "redrawn instances")
    with pytest.raises(FjspError) as host_err:
        host_batch(redraw_shape(redraws=0), REDRAW_BASE)
    with pytest.raises(FjspError) as err:
        generated(redraw_shape(redraws=0), REDRAW_BASE)
    assert err.value.code == host_err.value.code == FJSP_E_UNSUPPORTED
    named = "instance %d (seed %d)" % (idle[0], REDRAW_BASE + idle[0])
    assert named in str(err.value) and named in str(host_err.value) and "redraws = 0" in str(err.value)


# ---- 6: regenerate ------------------------------------------------------------------------------------------------------------------
def test_regenerate(torch_gpu):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd._capi import FJSP_E_STATE, FjspError
    s1, s2 = 60, 9000
    q = dyn(t_si_min=1.0, t_si_max=3.0, **DRAWN)             # arrivals closer than any operation is long: envs park early
    G = generated(q, s1)
    H1, H2 = host_batch(q, s1), host_batch(q, s2)
    T = max(ops_of(H1), ops_of(H2))
    first = episode(torch, G, T)
    H.same(first, episode(torch, H1, T), "seeds 1")
    G.regenerate(s2)
    assert bool(G.done.all()) and np.all(H.read(G)["done"] == 1)
    same_instances(G, H2, "regenerated")
    second = episode(torch, G, T)
    H.same(second, episode(torch, H2, T), "seeds 2 after a regenerate")
    H.same(second, episode(torch, generated(q, s2), T), "seeds 2 on a fresh handle")
    G.regenerate(s1)
    H.same(episode(torch, G, T), first, "seeds 1 again")
    # refused while envs are parked in the asynchronous service
    acts = acts_for(torch, G, 8)
    mo = mo_rows(torch, G, 1)
    G.reset()
    for t in range(8):
        G.step_async(acts[t], mo=mo)
    assert G.async_stats[0] > 0
    with pytest.raises(FjspError) as err:
        G.regenerate(s2)
    assert err.value.code == FJSP_E_STATE and "fjsp_env_arrivals_flush" in str(err.value)
    G.flush_arrivals(mo=mo)
    assert G.parked == 0
    G.regenerate(s2)
    H.same(episode(torch, G, T), second, "after flush and regenerate")


# ---- 7: every LP service ----------------------------------------------------------------------------------------------------------
# The handle chooses its arrival service from the parameters' worst tableau by fjsp_env_create's rule.  FIXED's worst tableau
# (9 operation types x 4 machines) fits the LDS, so FJSP_LP_IMPL=global serves it with the LDS simplex; GLOBAL_SHAPE's (30 x 12:
# 66 rows x 428 columns) does not, and goes to the global-memory simplex.
GLOBAL_SHAPE = dict(S_min=2, S_max=2, M_min=12, M_max=12, DDT_min=1.0, DDT_max=1.0, R_min=5, R_max=6, J_min=4, J_max=5, N_min=1, N_max=2)
_REF = {}


def reference_episode(torch, name, q):
    """The host twin's episode of a shape, played once and shared by the cases that need it."""
    if name not in _REF:
        Hb = host_batch(q, 40)
        T = ops_of(Hb)
        _REF[name] = (Hb, T, episode(torch, Hb, T))
    return _REF[name]


@pytest.mark.parametrize("impl,shape,on_device", [("host", "fixed", 0), ("device", "fixed", 1), ("global", "fixed", 1), ("global", "beyond the LDS", 2)])
def test_lp_services(torch_gpu, impl, shape, on_device):
    q = dyn(**(FIXED if shape == "fixed" else GLOBAL_SHAPE))
    Hb, T, ref = reference_episode(torch_gpu, shape, q)
    with H.env_var("FJSP_LP_IMPL", impl):
        G = generated(q, 40)
    assert G.lp_on_device == on_device, impl
    st = G.generated_stats()
    assert (st["lp_host"] == N_INST) if impl == "host" else (st["lp_host"] == 0), (impl, st)
    same_instances(G, Hb, impl)
    H.same(episode(torch_gpu, G, T), ref, impl)
    assert G.lp_solves == Hb.lp_solves > 0, impl
    assert (G.lp_device_pivots > 0) == (impl != "host"), impl


# ---- 8: schedule and snapshot -----------------------------------------------------------------------------------------------------
def test_schedule_and_snapshot(torch_gpu):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd._capi import FjspError
    q = dyn(**DRAWN)
    G, G2, Hb = generated(q, 60), generated(q, 60), host_batch(q, 60)
    cap = G.record_schedule()
    assert cap == 3 * 3 * 3 * 3                            # the parameters' worst case over three orders
    Hb.record_schedule()
    T = ops_of(Hb)
    acts = acts_for(torch, G, T)
    G.reset(); Hb.reset()
    half = T // 2
    for t in range(half):
        G.step(acts[t]); Hb.step(acts[t])
    snap = G.snapshot()
    G2.restore(snap, check=True)
    assert snap.errors() == 0
    H.same(H.read(G), H.read(G2), "restored into a handle generated alike")
    rest = []
    for t in range(half, T):
        rest.append([H.host(x) for x in G.step(acts[t])])
        Hb.step(acts[t])
    H.same(H.read(G), H.read(Hb), "read()")
    (tg, lg), (th, lh) = [[H.host(x) for x in b.schedule()] for b in (G, Hb)]
    assert np.array_equal(lg, lh) and np.all(lg > 0)
    for i in range(N_ENVS):
        assert np.array_equal(tg[i, :lg[i]], th[i, :lh[i]]), i
    # the snapshot replays: the restored handle, and the first one restored onto itself
    G.restore(snap)
    for b in (G2, G):
        for t in range(half, T):
            H.same([H.host(x) for x in b.step(acts[t])], rest[t - half], "replay step %d" % t)
        H.same(H.read(b), H.read(Hb), "read() of the replay")
    # another machine range over the same seeds: another fingerprint
    with pytest.raises(FjspError) as err:
        generated(dyn(mc=machine(2), **DRAWN), 60).restore(snap)
    assert "not compatible with the snapshot" in str(err.value)
    G2.regenerate(61)
    with pytest.raises(FjspError) as err:
        G2.restore(snap)
    assert "not compatible with the snapshot" in str(err.value)


# ---- 9: the wrapper and the messages --------------------------------------------------------------------------------------------------
def test_wrapper_and_messages(torch_gpu):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import environments as E
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, ST_STEP_AFTER_DONE, VARIANT_MO_DFJSP
    from deep_reinforcement_learning_for_fjsp_amd._capi import FJSP_E_UNSUPPORTED, FjspError, GenParams
    q = dyn(**DRAWN)
    env = E.BatchedMODFJSP(q, n_envs=N_ENVS, n_inst=N_INST, seed_base=60, rng_seed=5)
    twin = host_batch(q, 60)
    T = ops_of(twin)
    acts = acts_for(torch, env.batch, T)
    H.same(H.host(env.reset()), H.host(twin.reset()), "reset")
    for t in range(T):
        out = env.step(acts[t])
        H.same([H.host(x) for x in out], [H.host(x) for x in twin.step(acts[t], mo=env.mo)], "step %d" % t)
    assert bool(out[2].all())
    H.same(H.read(env.batch), H.read(twin), "read()")
    # (T is the longest instance's episode: the shorter ones were stepped after their end, which is the one flag allowed)
    assert not np.any(H.read(env.batch)["status"] & ~ST_STEP_AFTER_DONE)
    # a GenDynamic makes MO_DFJSP batches only, and the three older creates still refuse MO_DFJSP
    with pytest.raises(FjspError) as err:
        EnvBatch.generated(q, N_ENVS, 60, n_inst=N_INST)
    assert err.value.code == FJSP_E_UNSUPPORTED
    with pytest.raises(FjspError):
        E.BatchedSODFJSP(q, N_ENVS, n_inst=N_INST, seed_base=60)
    prm = GenParams.from_buffer_copy(q.o.r.base)
    prm.M, prm.S, prm.DDT = 4, 1, 1.0
    for params in (prm, q.o.r, q.o):
        with pytest.raises(FjspError) as err:
            EnvBatch.generated(params, N_ENVS, 60, n_inst=N_INST, variant=VARIANT_MO_DFJSP)
        assert err.value.code == FJSP_E_UNSUPPORTED
        assert "MO_DFJSP needs machine data" in str(err.value) and "fjsp_env_create_generated_dynamic" in str(err.value)
