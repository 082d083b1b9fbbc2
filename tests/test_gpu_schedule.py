"""GPU: the dispatched-schedule table (fjsp_env_record_schedule / fjsp_env_schedule) of both kernel families against
the reference-held fixtures and the C oracle, through every path that dispatches, and without perturbing the env."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

# suite -> kernel family the batch must run on (None: not asserted)
FAMILY = {"mk01": 1, "synth10x5": 1, "multijob": 0, "mo_dfjsp": 0}


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _table(b):
    t, n = b.schedule()
    return t.cpu().numpy(), n.cpu().numpy()


@pytest.mark.parametrize("suite", ["mk01", "synth10x5", "multijob", "multiorder", "so_sfjsp", "so_dfjsp", "mo_discretes",
                                   "mo_dfjsp"])
def test_schedule_equals_the_reference_tables(torch_gpu, suite):
    """tests/golden/schedule.npz: the reference's task objects (kind, task, job, machine, time_begin, time_end) after
    each stored episode -- breakdown-shifted starts and ends included -- against the device table, exactly, through the
    per-step and the fused path."""
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    from tests import schedule_fixture as F
    torch = torch_gpu
    variant, eps = F.load()[suite]
    for ep in eps:
        a, want = ep["inst"], ep["table"]
        T = len(want)
        actions = torch.from_numpy(np.ascontiguousarray(ep["actions"][:, None, :])).cuda()
        mo = None
        if ep["mo"] is not None:
            mo = torch.from_numpy(np.maximum(ep["mo"], 0.0)[None, :] if variant == 4 else ep["mo"][None, :].copy()).cuda()
        for mode in ("step", "rollout"):
            b = EnvBatch(H.instance_set_from([a]), 1, rng_seed=ep["rng_seed"], variant=variant)
            assert b.env_seed(0) == ep["rng_seed"]
            if suite in FAMILY:
                assert b.kernel_family == FAMILY[suite]
            assert b.record_schedule() == int((np.asarray(a.count) * np.asarray(a.Jr)[None, :]).sum())
            b.reset()
            if mode == "step":
                for t in range(T):
                    b.step(actions[t], mo=mo)
            else:
                b.rollout(actions, mo=mo)
            table, length = _table(b)
            assert length[0] == T, (suite, ep["source"], mode)
            assert np.array_equal(table[0, :T], want), (suite, ep["source"], mode)
            assert np.all(table[0, T:] == -1)


def _random_episode(torch, b, T, seed, n_task=6, n_machine=5):
    from deep_reinforcement_learning_for_fjsp_amd.batch import global_actions
    acts = torch.from_numpy(global_actions(seed, 0, b.N, T, n_task, n_machine)).cuda()
    b.reset()
    for t in range(T):
        b.step(acts[t])
    return acts.cpu().numpy()


@pytest.mark.parametrize("N", [4096, 8192])
def test_large_synth_batches_against_the_oracle(torch_gpu, N):
    """4096 envs: the small-batch row build; 8192: the large-batch build (gstep_kernel<..., false>)."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    torch = torch_gpu
    NI = 128
    s = fi.InstanceSet(NI).generate_range(4000, fi.bench_10x5_params()).solve_fluid()
    T = max(s.dims(i)["K"] for i in range(NI))
    b = EnvBatch(s, N, rng_seed=11)
    assert b.kernel_family == 1
    b.record_schedule()
    acts = _random_episode(torch, b, T, 5)
    table, length = _table(b)
    fin = {k: v.cpu().numpy() for k, v in b.read().items()}
    assert np.all(fin["done"] == 1) and np.all((fin["status"] & ~4) == 0)      # (4: stepped again after done, K < T)
    arrs = [s.arrays(i) for i in range(NI)]
    for e in range(N):
        a = arrs[e % NI]
        rows = table[e, :length[e]].astype(np.int64)
        assert sch.validate(a, rows, 0) == [], e
        obj = sch.objectives(a, rows, 0)
        assert obj["makespan"] == fin["makespan"][e] and obj["delay_time_sum"] == fin["delay_time_sum"][e], e
    for e in np.random.RandomState(N).choice(N, 64, replace=False).tolist():
        a = arrs[e % NI]
        want = H.play_oracle(a, a.x, acts[:, e], b.env_seed(e))
        rows = sch.from_trace(a, want["k"], want["m"], want["job_n"], want["step_time"])
        assert length[e] == want["T"] and np.array_equal(table[e, :want["T"]], rows), e


def test_training_distribution_batch_is_feasible(torch_gpu):
    """The training distribution of tools/bench_training_dist.py (Instance_generate.py:42-54, M = 15, one order): 4096
    wave-family envs played to the end, every schedule feasible and consistent with read()."""
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, global_actions
    torch = torch_gpu
    NI, N = 64, 4096
    s = fi.InstanceSet(NI)
    for i in range(NI):
        s.generate(i, 5000 + i, fi.reference_generator_params(1.0, 15, 1))
    s.solve_fluid()
    b = EnvBatch(s, N, rng_seed=3)
    assert b.kernel_family == 0
    b.record_schedule()
    acts = torch.from_numpy(global_actions(9, 0, N, 64, 6, 5)).cuda()
    b.reset()
    t = 0
    while not bool((b.done != 0).all()):
        for _ in range(50):
            b.step(acts[t % 64], state=False)
            t += 1
        assert t < 20000
    table, length = _table(b)
    fin = {k: v.cpu().numpy() for k, v in b.read().items()}
    arrs = [s.arrays(i) for i in range(NI)]
    for e in range(N):
        a = arrs[e % NI]
        rows = table[e, :length[e]].astype(np.int64)
        assert sch.validate(a, rows, 0) == [], e
        obj = sch.objectives(a, rows, 0)
        assert obj["delay_time_sum"] == fin["delay_time_sum"][e] and obj["makespan"] == fin["makespan"][e], e


@pytest.mark.parametrize("impl", ["rows", "wave"])
def test_every_path_gives_the_same_table_and_recording_does_not_perturb(torch_gpu, impl):
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, global_actions
    from deep_reinforcement_learning_for_fjsp_amd._capi import FjspError
    torch = torch_gpu
    N = 300
    s = fi.InstanceSet(16).generate_range(77, fi.bench_10x5_params()).solve_fluid()
    T = max(s.dims(i)["K"] for i in range(16))
    acts = torch.from_numpy(global_actions(3, 0, N, T, 6, 5)).cuda()
    with H.env_var("FJSP_STEP_IMPL", "wave" if impl == "wave" else None):
        mk = lambda: EnvBatch(s, N, rng_seed=4)
        plain, rec = mk(), mk()
        assert plain.kernel_family == (0 if impl == "wave" else 1)
        rec.record_schedule()
        outs = []
        for b in (plain, rec):
            b.reset()
            o = []
            for t in range(T):
                tr = torch.empty(N, 2, dtype=torch.int16, device="cuda")
                st, r, d = b.step(acts[t], trace_out=tr)
                o.append((H.bits(st.cpu().numpy()), H.bits(r.cpu().numpy()), d.cpu().numpy(), tr.cpu().numpy()))
            outs.append(o)
        for x, y in zip(*outs):
            for u, v in zip(x, y):
                assert np.array_equal(u, v)
        ref_table, ref_len = _table(rec)
        # step without a state
        b = mk(); b.record_schedule(); b.reset()
        for t in range(T):
            b.step(acts[t], state=False)
        assert np.array_equal(_table(b)[0], ref_table)
        # fused rollout, with and without the final state
        for state in (True, False):
            b = mk(); b.record_schedule(); b.reset()
            tr_r, _, _ = b.rollout(acts, state=state)
            assert np.array_equal(_table(b)[0], ref_table)
        # mid-episode switch refused; autoreset keeps the finished episode readable after its done step
        b = mk(); b.record_schedule(); b.reset()
        b.step(acts[0])
        with pytest.raises(FjspError):
            b.record_schedule(False)
        for t in range(1, T):
            b.step(acts[t])
        assert bool((b.done != 0).all())
        assert np.array_equal(_table(b)[0], ref_table)     # the finished episodes stay readable ...
        b.step(acts[0], autoreset=True)                    # ... until autoreset restarts them: one dispatch of the new episode
        t1, n1 = _table(b)
        assert np.all(n1 == 1) and np.all(t1[:, 0] >= 0) and np.all(t1[:, 1:] == -1)
        # off again between episodes: the plain kernels run and schedule() refuses
        b2 = mk(); b2.record_schedule(); b2.record_schedule(False)
        with pytest.raises(RuntimeError):
            b2.schedule()


def test_fused_policy_rollout_records_what_the_per_step_loop_records(torch_gpu):
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    torch = torch_gpu
    N = 64
    s = fi.InstanceSet(8).generate_range(5, fi.bench_10x5_params()).solve_fluid()
    T = max(s.dims(i)["K"] for i in range(8))
    # a wave-family batch with the fused policy rollout vs the per-step loop over the SAME actions
    with H.env_var("FJSP_STEP_IMPL", "wave"):
        b = EnvBatch(s, N, rng_seed=8)
        b.record_schedule()
        from deep_reinforcement_learning_for_fjsp_amd._capi import ActorParams, check
        import ctypes as C
        torch.manual_seed(0)
        S, A = b.state_size, 30
        w = [torch.randn(128, S, device="cuda") * 0.1, torch.zeros(128, device="cuda"), torch.randn(128, 128, device="cuda") * 0.1,
             torch.zeros(128, device="cuda"), torch.randn(A, 128, device="cuda") * 0.1, torch.zeros(A, device="cuda")]
        ap = ActorParams(*[C.c_void_p(x.data_ptr()) for x in w], S, 128, A)
        from deep_reinforcement_learning_for_fjsp_amd import _capi
        lib = _capi.lib()
        buf = C.c_void_p()
        check(lib.fjsp_rollout_create(T, N, S, 0, C.byref(buf)))
        try:
            st0 = b.reset().clone()
            eps = torch.zeros(1, dtype=torch.float32, device="cuda")
            seed = torch.tensor([123], dtype=torch.int64, device="cuda")
            flat = torch.zeros(T, N, dtype=torch.float32, device="cuda")
            logp = torch.zeros(T, N, dtype=torch.float32, device="cuda")
            last = torch.zeros(N, S, dtype=torch.float64, device="cuda")
            check(lib.fjsp_env_rollout_policy(b._h, buf, C.byref(ap), C.c_void_p(eps.data_ptr()), C.c_void_p(seed.data_ptr()), 5, T, None,
                                              C.c_void_p(st0.data_ptr()), C.c_void_p(flat.data_ptr()), C.c_void_p(logp.data_ptr()),
                                              C.c_void_p(last.data_ptr()), b._stream()))
            fused, fused_len = _table(b)
        finally:
            lib.fjsp_rollout_destroy(buf)
        f = flat.cpu().numpy().astype(np.int64)
        pair = np.stack([f // 5, f % 5], 2).astype(np.uint8)
        b2 = EnvBatch(s, N, rng_seed=8)
        b2.record_schedule(); b2.reset()
        for t in range(T):
            b2.step(torch.from_numpy(np.ascontiguousarray(pair[t])).cuda())
        step_t, step_len = _table(b2)
        assert np.array_equal(fused_len, step_len) and np.array_equal(fused, step_t)


def test_async_arrivals_record_each_step_once(torch_gpu):
    """fjsp_env_step_async on an order-arrival batch: the parking call writes the record, arrival_kernel adds none;
    after flush_arrivals the tables equal the blocking step's."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, VARIANT_MO_DFJSP, global_actions
    torch = torch_gpu
    insts, _, _ = H.load_suite("mo_dfjsp")
    s = H.instance_set_from(insts)
    N = 48
    acts = torch.from_numpy(global_actions(21, 0, N, 1400, 12, 10)).cuda()
    mo = torch.zeros(N, 4, dtype=torch.float64, device="cuda"); mo[:, 0] = 1.0
    a = EnvBatch(s, N, variant=VARIANT_MO_DFJSP, rng_seed=5)
    a.record_schedule(); a.reset()
    t = 0
    while not bool((a.done != 0).all()):
        a.step(acts[t], mo=mo)
        t += 1
        assert t < 1400
    want, want_len = _table(a)
    b = EnvBatch(s, N, variant=VARIANT_MO_DFJSP, rng_seed=5)
    b.record_schedule(); b.reset()
    cursor = torch.zeros(N, dtype=torch.int64, device="cuda")
    idx = torch.arange(N, device="cuda")
    for _ in range(4000):
        if bool((b.done != 0).all()) and b.parked == 0:
            break
        act = acts[cursor.clamp(max=1399), idx].contiguous()
        live = b.done == 0
        _, _, _, ready = b.step_async(act, mo=mo)
        cursor += (live & (ready != 0)).long()
    b.flush_arrivals()
    got, got_len = _table(b)
    assert np.array_equal(got_len, want_len) and np.array_equal(got, want)
    for e in range(N):
        rows = got[e, :got_len[e]].astype(np.int64)
        assert sch.validate(insts[e % len(insts)], rows, 4) == [], e
