"""GPU: the one-wave-per-environment kernels (csrc/fjsp_kernels.hip: step / rollout / reset / arrival, 1, 2 and 4 chunks
of 64 operation types) against the C oracle at their size limits.

The cases are tests/wave_limit_cases.py's (tests/test_wave_limit_cases_host.py proves on the CPU that each reaches the
condition it exists for): K = 64 | 65, 128 | 129, 255 | 256; R = 255 | 256 kinds; a kind of 254 | 255 stages; M = 8 | 9,
31 | 32; job tables of 16 | 17, 64 | 65, 128 | 129 and 131 jobs; 64 orders; tardiness next to 2^31; K = 65, 128 | 129 with
three orders (the two- and four-chunk builds of the kernels with order arrivals).  Every batch is created
with kernel_family=0 (the wave kernels also where the row kernels would fit), instances at offset 2, 6 environments.

Per case: per-step launches against the oracle's replay of every environment -- chosen (operation type, machine),
reward (bit-equal) and done at every step, the reset state and every state (tests.helpers.assert_state_close), the totals
and the machines' end times; then, bit for bit against those per-step results on fresh batches, the fused rollout with
and without a final state, and one autoreset step against reset + step.  K = 256, M = 32 and S = 64 also record the
schedule through the per-step and the fused kernels and compare it with the oracle's dispatches.
"""
import numpy as np
import pytest

from tests import helpers as H
from tests import wave_limit_cases as WC

pytestmark = pytest.mark.gpu

TOTALS = ("delay_time_sum", "makespan", "step_time", "step_count", "completion_time")


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _steps(torch, b, acts, mo):
    """reset(), then every step of acts (device u8[T, N, 2]) through the per-step launch, traced."""
    T, N = acts.shape[0], b.N
    st = torch.zeros(T, N, b.state_size, dtype=torch.float64, device=b.device)
    rw = torch.zeros(T, N, dtype=torch.float64, device=b.device)
    dn = torch.zeros(T, N, dtype=torch.uint8, device=b.device)
    tr = torch.zeros(T, N, 2, dtype=torch.int16, device=b.device)
    st0 = b.reset().cpu().numpy()
    for t in range(T):
        b.step(acts[t], mo=mo, state_out=st[t], reward_out=rw[t], done_out=dn[t], trace_out=tr[t])
    fin = H.read(b)
    fin["tend"] = b.machine_time_end().cpu().numpy()
    return dict(state=st.cpu().numpy(), reward=rw.cpu().numpy(), done=dn.cpu().numpy(), trace=tr.cpu().numpy(), state0=st0, fin=fin)


def _expected_rows(a, w):
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    if hasattr(a, "bk_n"):                      # breakdown windows move starts and ends
        return WC.dispatch_rows(a, w)[0]
    return sch.from_trace(a, w["k"], w["m"], w["job_n"], w["step_time"])


def _check_schedule(b, c, arrs, want, path):
    table, length = [x.cpu().numpy() for x in b.schedule()]
    for e, w in enumerate(want):
        rows = _expected_rows(arrs[e % c.n_inst], w)
        assert length[e] == w["T"] and np.array_equal(table[e, :w["T"]], rows), "%s recorded %s env %d" % (c.name, path, e)
        assert (table[e, w["T"]:] == -1).all(), "%s recorded %s env %d: rows after the episode" % (c.name, path, e)
    assert (H.read(b)["status"] & 16 == 0).all(), "%s recorded %s: schedule overflow" % (c.name, path)


@pytest.mark.parametrize("cid", WC.case_ids(), ids=WC.case_name)
def test_wave_kernels_at_their_limits(torch_gpu, cid):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    c = WC.case(cid)
    v, N, kw = c.variant, WC.N_ENVS, WC.STATE_KW[c.variant]
    s = WC.instance_set(c)
    arrs = WC.set_arrays(c, s)
    acts_h = WC.actions(c)
    acts = torch.from_numpy(acts_h).cuda()
    rows = WC.mo_rows(c)
    mo = None if rows is None else torch.tensor(rows, dtype=torch.float64).cuda()

    def batch():
        b = EnvBatch(s, N, first=WC.FIRST, n_inst=c.n_inst, variant=v, rng_seed=WC.RNG_SEED, kernel_family=0)
        assert b.kernel_family == 0
        return b
    b = batch()
    assert [b.env_seed(e) for e in range(N)] == [WC.env_seed(e) for e in range(N)]
    want = WC.replay(c, arrs, acts_h)
    run = _steps(torch, b, acts, mo)
    fin = run["fin"]

    # ---- per-step launches against the oracle
    if c.finite:
        assert np.isfinite(run["state0"]).all(), c.name + ": a reset state entry is NaN or infinite"
        for e, w in enumerate(want):
            bad = np.argwhere(~np.isfinite(run["state"][:w["T"], e]))
            assert len(bad) == 0, "%s env %d: state entry %d is %r at step %d (oracle: %r)" % (
                c.name, e, bad[0][1], run["state"][bad[0][0], e, bad[0][1]], bad[0][0], w["states"][bad[0][0], bad[0][1]])
    assert (fin["done"] == 1).all() and (fin["status"] & ~4 == 0).all(), c.name
    for e, w in enumerate(want):
        a = arrs[e % c.n_inst]
        Te, te = w["T"], "%s env %d (K=%d M=%d S=%d)" % (c.name, e, a.K, a.M, a.S)
        tr = run["trace"][:, e]
        for t in np.nonzero((tr[:Te, 0] != w["k"]) | (tr[:Te, 1] != w["m"]))[0][:1]:
            raise AssertionError("%s: step %d chose (k, m) = %s, the oracle (%d, %d)" % (te, t, tuple(tr[t]), w["k"][t], w["m"][t]))
        assert (tr[Te:] == -1).all(), te + " choices after the episode"
        assert np.array_equal(H.bits(run["reward"][:Te, e]), H.bits(w["reward"])), te + " rewards"
        assert np.array_equal(run["done"][:Te, e], w["done"]) and (run["done"][Te:, e] == 1).all(), te + " done"
        H.assert_state_close(run["state0"][e], w["state0"], te + " reset", **kw)
        H.assert_state_close(run["state"][:Te, e], w["states"], te, **kw)
        assert fin["step_count"][e] == Te and fin["step_time"][e] == w["step_time"][-1], te
        assert fin["makespan"][e] == w["makespan"], te
        assert fin["delay_time_sum"][e] == w["delay_time_sum"], "%s delay_time_sum %d, the oracle %d" % (te, fin["delay_time_sum"][e], w["delay_time_sum"])
        assert fin["completion_time"][e] == w["completion_time"], te
        if v == 4:
            assert fin["energy_consumption"][e] == w["energy"], te
        assert np.array_equal(fin["tend"][e, :a.M], w["tend"]), te + " machine_time_end"

    # ---- the fused rollout, with and without a final state, against the per-step results
    Ks = fin["step_count"]
    for state in (True, False):
        b2 = batch()
        b2.reset()
        tr2, rw2, st_last = b2.rollout(acts, mo=mo, state=state)
        fin2 = H.read(b2)
        tag = "%s rollout(state=%s)" % (c.name, state)
        assert np.array_equal(tr2.cpu().numpy(), run["trace"]), tag + " traces"
        assert np.array_equal(H.bits(rw2.cpu().numpy()), H.bits(run["reward"])), tag + " rewards"
        for key in TOTALS + ("done",):
            assert np.array_equal(fin2[key], fin[key]), (tag, key)
        if state:
            assert np.array_equal(H.bits(st_last.cpu().numpy()), H.bits(run["state"][Ks - 1, np.arange(N)])), tag + " final state"
        else:
            assert st_last is None

    # ---- autoreset on the finished batch = reset() + step() of a fresh one (a deterministic pair: the random.choice
    # stream goes on across resets)
    det = torch.tensor(WC.DET_PAIR[v], dtype=torch.uint8).repeat(N, 1).cuda()
    fresh = batch()
    fresh.reset()
    st_f, r_f, d_f = [x.clone() for x in fresh.step(det, mo=mo)]
    st_a, r_a, d_a = b.step(det, autoreset=True, mo=mo)
    assert torch.equal(st_a, st_f) and torch.equal(r_a, r_f) and torch.equal(d_a, d_f), c.name + " autoreset"
    fa, ff = H.read(b), H.read(fresh)
    for key in TOTALS:
        assert np.array_equal(fa[key], ff[key]), (c.name, "autoreset", key)
    assert (fa["status"] == 0).all(), c.name + " autoreset: sticky status bits"

    # ---- recording through the per-step and the fused kernels
    if c.record:
        b3 = batch()
        b3.record_schedule()
        rec = _steps(torch, b3, acts, mo)
        assert np.array_equal(rec["trace"], run["trace"]) and np.array_equal(H.bits(rec["state"]), H.bits(run["state"])), c.name + " recorded steps"
        _check_schedule(b3, c, arrs, want, "steps")
        b4 = batch()
        b4.record_schedule()
        b4.reset()
        tr4, rw4, _ = b4.rollout(acts, mo=mo)
        assert np.array_equal(tr4.cpu().numpy(), run["trace"]) and np.array_equal(H.bits(rw4.cpu().numpy()), H.bits(run["reward"])), c.name + " recorded rollout"
        _check_schedule(b4, c, arrs, want, "rollout")
