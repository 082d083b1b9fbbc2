"""GPU: saved environment states (fjsp_snapshot_*, EnvBatch.snapshot / restore), the drop-in classes' copies that carry
the episode, and the rollout lookahead built on them (lookahead.rollout_dispatch)."""
import copy
import ctypes as C
import pickle

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _training_dist(n, seed):
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    s = fi.InstanceSet(n)
    for i in range(n):
        s.generate(i, seed + i, fi.reference_generator_params(1.0, 15, 1))
    return s.solve_fluid()


def _play_steps(torch, b, acts, mo):
    """Per-step path: every step's (state, reward, done, trace), then read() and schedule()."""
    out = []
    tr = torch.zeros(b.N, 2, dtype=torch.int16, device=b.device)
    for t in range(acts.shape[0]):
        st, rw, dn = b.step(acts[t], mo=mo, trace_out=tr)
        out.append((H.host(st), H.host(rw), H.host(dn), H.host(tr)))
    return out, H.read(b), [H.host(x) for x in b.schedule()]


def _play_rollout(torch, b, acts, mo):
    tr, rw, st = b.rollout(acts, mo=mo)
    return (H.host(tr), H.host(rw), H.host(st)), H.read(b), [H.host(x) for x in b.schedule()]


def _rewind_case(torch, b, acts, t1, mo=None):
    """reset, t1 steps, snapshot, play to the end (per step); restore and replay: everything bit-identical.  Then the
    fused rollout from the restored state twice, and against the per-step trajectory where the envs stepped."""
    b.record_schedule()
    b.reset()
    for t in range(t1):
        b.step(acts[t], mo=mo)
    snap = b.snapshot()
    assert snap.capacity == b.schedule_capacity
    rest = acts[t1:]
    first = _play_steps(torch, b, rest, mo)
    b.restore(snap, check=True)
    again = _play_steps(torch, b, rest, mo)
    H.same(first, again, "per-step replay")
    b.restore(snap)
    fused = _play_rollout(torch, b, rest, mo)
    b.restore(snap)
    fused2 = _play_rollout(torch, b, rest, mo)
    H.same(fused, fused2, "fused replay")
    # fused vs per-step: same choices, rewards where an env stepped, same end state, read() and schedule table
    (tr, rw, st), rd, sched = fused
    steps, rd_s, sched_s = first
    tr_s = np.stack([x[3] for x in steps])
    rw_s = np.stack([x[1] for x in steps])
    assert np.array_equal(tr, tr_s)
    live = tr[..., 0] >= 0
    assert np.array_equal(H.bits(rw[live]), H.bits(rw_s[live]))
    for k in rd:
        if k == "status":
            assert np.array_equal(rd[k] & ~4, rd_s[k] & ~4)
        else:
            assert np.array_equal(rd[k], rd_s[k]), k
    H.same(sched, sched_s, "schedule fused vs per-step")
    assert np.all(rd["done"] == 1)
    return snap


def _random_acts(torch, N, T, n_task, n_machine, seed):
    from deep_reinforcement_learning_for_fjsp_amd.batch import global_actions
    return torch.from_numpy(global_actions(seed, 0, N, T, n_task, n_machine)).cuda()


@pytest.mark.parametrize("case", ["rows", "wave", "so_sfjsp", "mo_discretes", "multijob"])
def test_rewind_is_exact(torch_gpu, case):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, VARIANT_MO_FJSSP_DISCRETES, VARIANT_SO_SFJSP
    N = 256
    if case == "multijob":
        s, variant, n_task, n_machine, NI = _training_dist(16, 700), 0, 6, 5, 16
    else:
        s, NI = H.gen_10x5(32, 600), 32
        variant, n_task, n_machine = {"rows": (0, 6, 5), "wave": (0, 6, 5), "so_sfjsp": (VARIANT_SO_SFJSP, 20, 1),
                                      "mo_discretes": (VARIANT_MO_FJSSP_DISCRETES, 18, 1)}[case]
    with H.env_var("FJSP_STEP_IMPL", "wave" if case == "wave" else None):
        b = EnvBatch(s, N, variant=variant, rng_seed=77)
    assert b.kernel_family == (0 if case in ("wave", "multijob", "so_sfjsp") else 1)
    T = int(H.ops(s, NI, N).max())
    acts = _random_acts(torch, N, T, n_task, n_machine, 31)
    mo = None
    if variant == VARIANT_MO_FJSSP_DISCRETES:
        mo = torch.tensor([[0.5, 0.5, 800.0, 300.0]], dtype=torch.float64, device="cuda").repeat(N, 1)
    _rewind_case(torch, b, acts, T // 3, mo)


@pytest.mark.parametrize("lp", ["host", "device"])
def test_rewind_is_exact_with_arrivals_and_breakdowns(torch_gpu, lp):
    """MO_DFJSP with order arrivals (fluid LPs solved on the host or on the device) and machine breakdowns."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, VARIANT_MO_DFJSP
    insts, _, _ = H.load_suite("mo_dfjsp")
    if lp == "device":           # the device LP service takes batches whose every tableau fits a CU's LDS
        insts = [a for a in insts if not a.name.startswith("HMPSAC")]
    s = H.instance_set_from(insts)
    N = 2 * len(insts)
    with H.env_var("FJSP_LP_IMPL", lp):
        b = EnvBatch(s, N, variant=VARIANT_MO_DFJSP, rng_seed=5)
    assert b.lp_on_device == (1 if lp == "device" else 0)
    T = int(H.ops(s, len(insts), N).max())
    acts = _random_acts(torch, N, T, 12, 10, 17)
    mo = torch.zeros(N, 4, dtype=torch.float64, device="cuda"); mo[:, 0] = 1.0
    assert any(a.S > 1 for a in insts) and any(int(np.sum(a.bk_n)) > 0 for a in insts)
    _rewind_case(torch, b, acts, T // 4, mo)


@pytest.mark.parametrize("family", ["rows", "wave"])
def test_rewind_fused_policy_rollout(torch_gpu, family):
    """fjsp_env_rollout_policy (actor inside the environment kernel) from a restored state, twice: same actions, same
    schedule, same last state."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import _capi
    from deep_reinforcement_learning_for_fjsp_amd._capi import ActorParams, check
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    N = 128
    s = H.gen_10x5(8, 90)
    T = int(H.ops(s, 8, N).max())
    with H.env_var("FJSP_STEP_IMPL", "wave" if family == "wave" else None):
        b = EnvBatch(s, N, rng_seed=8)
    b.record_schedule()
    torch.manual_seed(0)
    S, A = b.state_size, 30
    w = [torch.randn(128, S, device="cuda") * 0.1, torch.zeros(128, device="cuda"), torch.randn(128, 128, device="cuda") * 0.1,
         torch.zeros(128, device="cuda"), torch.randn(A, 128, device="cuda") * 0.1, torch.zeros(A, device="cuda")]
    ap = ActorParams(*[C.c_void_p(x.data_ptr()) for x in w], S, 128, A)
    lib = _capi.lib()
    b.reset()
    acts = _random_acts(torch, N, 4, 6, 5, 3)
    for t in range(4):
        b.step(acts[t])
    snap = b.snapshot()
    outs = []
    for _ in range(2):
        b.restore(snap, check=True)
        buf = C.c_void_p()
        check(lib.fjsp_rollout_create(T, N, S, 0, C.byref(buf)))
        try:
            eps = torch.zeros(1, dtype=torch.float32, device="cuda")
            seed = torch.tensor([123], dtype=torch.int64, device="cuda")
            flat = torch.zeros(T, N, dtype=torch.float32, device="cuda")
            logp = torch.zeros(T, N, dtype=torch.float32, device="cuda")
            last = torch.zeros(N, S, dtype=torch.float64, device="cuda")
            st0 = b.state.clone()
            check(lib.fjsp_env_rollout_policy(b._h, buf, C.byref(ap), C.c_void_p(eps.data_ptr()), C.c_void_p(seed.data_ptr()), 5, T,
                                              None, C.c_void_p(st0.data_ptr()), C.c_void_p(flat.data_ptr()),
                                              C.c_void_p(logp.data_ptr()), C.c_void_p(last.data_ptr()), b._stream()))
            outs.append((H.host(flat), H.host(logp), H.host(last), H.read(b), [H.host(x) for x in b.schedule()]))
        finally:
            lib.fjsp_rollout_destroy(buf)
    H.same(outs[0], outs[1], "fused policy replay")


def test_branch_across_batches(torch_gpu):
    """512-env source saved into a 512 x 20 branch batch (above the row kernels' 5120-env switch to the large build):
    every branch block continues exactly as a twin of the source stepped with that block's deterministic pair."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    NI, N, P = 64, 512, len(H.DET_SO)
    s = H.gen_10x5(NI, 1234)
    T = int(H.ops(s, NI, N).max())
    src = EnvBatch(s, N, rng_seed=9)
    twin = EnvBatch(s, N, rng_seed=9)
    br = EnvBatch(s, P * N, rng_seed=9)
    assert src.kernel_family == br.kernel_family == 1 and P * N > 5120 >= N
    for x in (src, twin, br):
        x.record_schedule()
    pre = torch.from_numpy(np.tile(np.array(H.DET_SO, np.uint8)[np.arange(N) % P][None], (5, 1, 1))).cuda()
    src.reset(); twin.reset()
    for t in range(5):
        src.step(pre[t]); twin.step(pre[t])
    snap = src.snapshot()
    twin_snap = twin.snapshot()
    br.restore(snap, np.tile(np.arange(N), P))
    pairs = torch.tensor(H.DET_SO, dtype=torch.uint8, device="cuda")
    act_b = pairs[:, None, :].expand(P, N, 2).reshape(P * N, 2).contiguous()
    st_b, rw_b = [], []
    for t in range(T - 5):
        st, rw, _ = br.step(act_b)
        st_b.append(H.host(st)); rw_b.append(H.host(rw))
    tab_b, len_b = [H.host(x) for x in br.schedule()]
    for p in (0, 7, 19):
        twin.restore(twin_snap)
        a = pairs[p][None].expand(N, 2).contiguous()
        for t in range(T - 5):
            st, rw, _ = twin.step(a)
            assert np.array_equal(H.bits(st_b[t][p * N:(p + 1) * N]), H.bits(H.host(st))), (p, t)
            assert np.array_equal(H.bits(rw_b[t][p * N:(p + 1) * N]), H.bits(H.host(rw))), (p, t)
        tab, ln = [H.host(x) for x in twin.schedule()]
        assert np.array_equal(tab_b[p * N:(p + 1) * N], tab) and np.array_equal(len_b[p * N:(p + 1) * N], ln), p


def test_same_slot_in_another_batch_replays_random_rules(torch_gpu):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, EnvSnapshot
    NI, N = 16, 64
    s = H.gen_10x5(NI, 55)
    T = int(H.ops(s, NI, N).max())
    acts = torch.full((T, N, 2), 0, dtype=torch.uint8, device="cuda")
    acts[..., 0], acts[..., 1] = 5, 4                               # both random.choice rules
    a = EnvBatch(s, N, rng_seed=123, first_env=256)
    bb = EnvBatch(s, N, rng_seed=123, first_env=256)
    a.reset()
    for t in range(6):
        a.step(acts[t])
    snap = EnvSnapshot.from_bytes(bb, a.snapshot().to_bytes())
    bb.restore(snap)
    for t in range(6, T):
        sa, ra, _ = a.step(acts[t])
        sb, rb, _ = bb.step(acts[t])
        assert np.array_equal(H.bits(H.host(sa)), H.bits(H.host(sb))) and np.array_equal(H.bits(H.host(ra)), H.bits(H.host(rb))), t
    H.same(H.read(a), H.read(bb), "read")


def test_errors(torch_gpu):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd._capi import FjspError
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, VARIANT_MO_DFJSP, VARIANT_SO_SFJSP
    s = H.gen_10x5(4, 10)
    b = EnvBatch(s, 8, rng_seed=1)
    b.reset()
    b.step(torch.zeros(8, 2, dtype=torch.uint8, device="cuda"))
    snap = b.snapshot()
    # instance mismatch, host src: ValueError before any launch
    bad = np.full(8, -1); bad[0] = 1
    with pytest.raises(ValueError):
        b.restore(snap, bad)
    # instance mismatch, device src: env untouched, counted
    b2 = EnvBatch(s, 8, rng_seed=1)
    b2.reset()
    before = H.read(b2)
    b2.restore(snap, torch.tensor(bad, dtype=torch.int32, device="cuda"))
    assert snap.errors() > 0
    H.same(before, H.read(b2), "untouched env")
    with pytest.raises(ValueError):
        b2.restore(snap, torch.tensor(bad, dtype=torch.int32, device="cuda"), check=True)
    # other instance set, other variant: FJSP_E_ARG
    for other in (EnvBatch(H.gen_10x5(4, 11), 8), EnvBatch(s, 8, variant=VARIANT_SO_SFJSP)):
        with pytest.raises(FjspError) as ei:
            other.restore(snap)
        assert ei.value.code == -1
        with pytest.raises(FjspError) as ei:
            other.snapshot(out=snap)
        assert ei.value.code == -1
    # a recording batch and a snapshot without records: FJSP_E_STATE
    rec = EnvBatch(s, 8, rng_seed=1)
    rec.record_schedule()
    with pytest.raises(FjspError) as ei:
        rec.restore(snap)
    assert ei.value.code == -7
    # parked asynchronous envs: FJSP_E_STATE
    insts, _, _ = H.load_suite("mo_dfjsp")
    ds = H.instance_set_from(insts)
    N = 96
    d = EnvBatch(ds, N, variant=VARIANT_MO_DFJSP, rng_seed=5)
    mo = torch.zeros(N, 4, dtype=torch.float64, device="cuda"); mo[:, 0] = 1.0
    d.reset()
    dsnap = d.snapshot()
    acts = _random_acts(torch, N, 400, 12, 10, 3)
    parked = False
    for t in range(400):
        d.step_async(acts[t], mo=mo)
        if d.parked > 0:
            parked = True
            break
    assert parked
    for call in (lambda: d.snapshot(), lambda: d.restore(dsnap)):
        with pytest.raises(FjspError) as ei:
            call()
        assert ei.value.code == -7
    d.flush_arrivals()
    d.snapshot(out=dsnap)


def _dropin_cases():
    from deep_reinforcement_learning_for_fjsp_amd.environments import (MO_DFJSP_Environment, MO_FJSSP_Environment,
                                                                       SO_FJSSP_Environment, SO_SFJSP_Environment)
    return [
        ("so_fjssp", lambda: SO_FJSSP_Environment(use_instance=True, DDT=1.0, M=6, S=1, seed=3, rng_seed=41),
         lambda e, t: e.step([t % 6, (t * 7) % 5])),
        ("so_sfjsp", lambda: SO_SFJSP_Environment(use_instance=True, DDT=1.0, M=6, S=1, seed=4, rng_seed=42),
         lambda e, t: e.step((t * 3) % 20)),
        ("mo_fjssp", lambda: MO_FJSSP_Environment(use_instance=True, DDT=1.0, M=6, S=1, seed=5, rng_seed=43),
         lambda e, t: e.step((t * 5) % 18, weight_vector=(0.5, 0.5), completion=900.0, tardiness=400.0)),
        ("mo_dfjsp", lambda: MO_DFJSP_Environment(use_instance=True, DDT=1.0, M=6, S=3, seed=6, rng_seed=44),
         lambda e, t: e.step([t % 12, (t * 3) % 10], reward_policy=1)),
    ]


def _play_out(env, step, t0):
    out, t = [], t0
    while not env.done:
        s, r, d = step(env, t)
        out.append((np.asarray(s).copy(), r, d, env.step_time, env.delay_time_sum))
        t += 1
    return out


@pytest.mark.parametrize("k", range(4))
def test_dropin_copies_carry_the_episode(torch_gpu, k):
    name, make, step = _dropin_cases()[k]
    orig, twin = make(), make()
    orig.reset(); twin.reset()
    for t in range(7):
        step(orig, t); step(twin, t)
    c1 = copy.deepcopy(orig)
    c2 = pickle.loads(pickle.dumps(orig))
    assert c1._batch is not orig._batch and c2._batch is not orig._batch
    assert c1.step_count == orig.step_count == 7 and np.array_equal(H.bits(c2.state), H.bits(orig.state))
    want = _play_out(twin, step, 7)
    for env in (c1, orig, c2):          # the copies and the original go on independently, each as the uncopied twin
        got = _play_out(env, step, 7)
        assert len(got) == len(want), name
        for g, w in zip(got, want):
            assert np.array_equal(H.bits(g[0]), H.bits(w[0])) and g[1:] == w[1:], name
        assert env.reward_sum == twin.reward_sum


def test_old_state_dict_still_loads(torch_gpu):
    from deep_reinforcement_learning_for_fjsp_amd.environments import SO_FJSSP_Environment
    ref = SO_FJSSP_Environment(use_instance=True, DDT=1.0, M=6, S=1, seed=11, rng_seed=5)
    a = ref._set.arrays(0)
    old = dict(arrays=(a.Jr, a.p, a.elig_n, a.elig_list, a.count, a.arrive, a.delivery, a.ddt, a.x),
               file_name="DDT1.0_M6_S1", device=0, rng_seed=5)
    env = SO_FJSSP_Environment.__new__(SO_FJSSP_Environment)
    env.__setstate__(old)
    assert env.step_count == 0 and env.state is None and env.file_name == "DDT1.0_M6_S1"
    assert np.array_equal(H.bits(env.reset()), H.bits(ref.reset()))


def test_lookahead_beats_every_fixed_pair_so_fjssp(torch_gpu):
    """256 generated 10x5 instances, the 20 deterministic pairs: the lookahead's makespan is <= the best fixed pair's
    for every env, and the CPU oracle replaying the chosen actions reaches the same makespan."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    from deep_reinforcement_learning_for_fjsp_amd.lookahead import rollout_dispatch
    NI = N = 256
    s = H.gen_10x5(NI, 9000)
    T = int(H.ops(s, NI, N).max())
    fixed = []
    ev = EnvBatch(s, len(H.DET_SO) * N, rng_seed=2)
    ev.reset()
    pairs = torch.tensor(H.DET_SO, dtype=torch.uint8, device="cuda")
    ev.rollout(pairs[:, None, :].expand(len(H.DET_SO), N, 2).reshape(1, -1, 2).expand(T, -1, 2).contiguous(), trace=False,
               rewards=False, state=False)
    fixed = ev.read()["makespan"].cpu().numpy().reshape(len(H.DET_SO), N)
    b = EnvBatch(s, N, rng_seed=2)
    b.reset()
    res = rollout_dispatch(b, H.DET_SO, "makespan")
    got = res["objective"].cpu().numpy()
    assert np.all(got <= fixed.min(0))
    ops = H.ops(s, NI, N)
    assert np.array_equal(res["steps"], ops)
    for e in np.random.RandomState(1).choice(N, 24, replace=False).tolist():
        a = s.arrays(e)
        want = H.play_oracle(a, a.x, res["actions"][:ops[e], e], b.env_seed(e))
        assert want["makespan"] == got[e], e


def test_lookahead_beats_every_fixed_pair_mo_dfjsp(torch_gpu):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, VARIANT_MO_DFJSP
    from deep_reinforcement_learning_for_fjsp_amd.lookahead import rollout_dispatch
    insts, _, _ = H.load_suite("mo_dfjsp")
    insts = [a for a in insts if a.name.startswith("gen")]         # small instances with arrivals and breakdowns
    assert any(a.S > 1 for a in insts) and any(int(np.sum(a.bk_n)) > 0 for a in insts)
    s = H.instance_set_from(insts)
    NI = len(insts)
    N = 4 * NI
    cands = [(a, m) for a in range(4) for m in range(3)]            # deterministic task / machine rules
    T = int(H.ops(s, NI, N).max())
    ev = EnvBatch(s, len(cands) * N, variant=VARIANT_MO_DFJSP, rng_seed=2)
    mo = torch.zeros(len(cands) * N, 4, dtype=torch.float64, device="cuda"); mo[:, 0] = 1.0
    ev.reset()
    pairs = torch.tensor(cands, dtype=torch.uint8, device="cuda")
    ev.rollout(pairs[:, None, :].expand(len(cands), N, 2).reshape(1, -1, 2).expand(T, -1, 2).contiguous(), trace=False,
               rewards=False, state=False, mo=mo)
    fixed = ev.read()["delay_time_sum"].cpu().numpy().reshape(len(cands), N)
    b = EnvBatch(s, N, variant=VARIANT_MO_DFJSP, rng_seed=2)
    b.reset()
    res = rollout_dispatch(b, cands, "tardiness", mo=mo[:N])
    got = res["objective"].cpu().numpy()
    assert np.all(got <= fixed.min(0))


def test_bad_device_save_index_leaves_an_entry_no_restore_takes(torch_gpu):
    """A device index outside [0, N): the kernel counts it, the entry's instance is -1 and its rows are zero, and a
    restore from it leaves the env and its rows as they were."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    s = H.gen_10x5(4, 12)
    b = EnvBatch(s, 8, rng_seed=1)
    b.reset()
    b.step(torch.zeros(8, 2, dtype=torch.uint8, device="cuda"))
    snap = b.snapshot(torch.tensor([0, 1, 8, -1], dtype=torch.int32, device="cuda"))
    assert snap.errors() == 2
    assert snap.instance.cpu().tolist() == [0, 1, -1, -1]
    assert not bool(snap.state[2:].any()) and not bool(snap.done[2:].any())
    before, st = H.read(b), H.host(b.state)
    b.restore(snap, torch.tensor([-1, -1, 2, -1, -1, -1, -1, -1], dtype=torch.int32, device="cuda"))
    assert snap.errors() == 1
    H.same(before, H.read(b), "untouched env")
    assert np.array_equal(H.bits(st), H.bits(H.host(b.state)))


def test_kernel_family_is_a_create_argument(torch_gpu):
    from deep_reinforcement_learning_for_fjsp_amd._capi import FjspError
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    from deep_reinforcement_learning_for_fjsp_amd.lookahead import make_branch
    s = H.gen_10x5(4, 13)
    with H.env_var("FJSP_STEP_IMPL", "wave"):
        assert EnvBatch(s, 8).kernel_family == 0
        rows = EnvBatch(s, 8, kernel_family=1)           # the argument, not the environment variable, decides
        assert rows.kernel_family == 1
        assert make_branch(rows, 3).kernel_family == 1
    assert EnvBatch(s, 8, kernel_family=0).kernel_family == 0
    with pytest.raises(FjspError) as ei:
        EnvBatch(_training_dist(2, 40), 4, kernel_family=1)    # several jobs per kind: no row kernels
    assert ei.value.code == -5
    with pytest.raises(ValueError):
        EnvBatch(s, 8, kernel_family=2)


def test_lookahead_stops_on_an_env_that_cannot_finish(torch_gpu):
    """A source env with an error bit (an undefined rule) is never done: rollout_dispatch raises instead of looping."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    from deep_reinforcement_learning_for_fjsp_amd.lookahead import rollout_dispatch
    s = H.gen_10x5(4, 14)
    b = EnvBatch(s, 8, rng_seed=1)
    b.reset()
    a = torch.zeros(8, 2, dtype=torch.uint8, device="cuda")
    a[3, 0] = 6                                                  # task rule index 6 does not exist
    b.step(a)
    assert int(b.read()["status"][3].item()) & 1
    with pytest.raises(RuntimeError):
        rollout_dispatch(b, H.DET_SO[:4], "makespan")
    with pytest.raises(ValueError):
        rollout_dispatch(b, [(6, 5)], "makespan")                # refused before anything is created
