"""GPU: fjsp_schedule_decode and fjsp_schedule_critical (csrc/fjsp_decode.hip) at the limits fjsp_env_create accepts -- the
cases of tests/decode_limit_cases.py, whose conditions tests/test_decode_limit_cases_host.py proves on the CPU -- and on
handles whose instances the device generated.

The references are tests/decode_reference.py and tests/critical_reference.py, which work in Python integers; no kernel
output is a reference.  Everything is compared bit for bit: objective, status, table and length of every candidate; every key
of critical_reference.KEYS of every table; and every move critical writes (in the long cases the first of each table) is
decoded again -- as a move, and as the plan schedule.apply_moves makes of it -- and must equal the reference's decode of the
materialised plan.  Each batch decodes one candidate more than a workgroup takes; lane 0 and lane 37 carry the edge candidate.

Wall time on an MI355X (pytest --durations=0, the call phase): 35 tests in about 13 s, nearly all of it the references' Python
loops over the long tables -- long-65535 3.3 s, long-32767 | 32768 | 32769 2.3 | 1.6 | 1.6 s, far 2.1 s, kinds 0.5 s, improve
0.4 s, every other test below 0.2 s.  In the same run tests/test_gpu_decode.py took 3.4 s (40 tests) and
tests/test_gpu_critical.py 2.9 s.

What the module sees that the feature tests do not, checked on builds of fjsp_decode.hip with one value changed each and
every index still in range (test_gpu_decode.py, test_gpu_critical.py and both test_gpu_improve modules pass on the first four):
    tard accumulated in 32 bits                   clock-one, clock-two, late fail
    kind index & 0x7F                             kinds, late fail
    stage byte & 0x7F                             long-65535, far, stages-so, stages-two fail
    w - u <= 32767 reverted to v - u <= 65535     far fails (critical emits a move decode refuses)
    machine index & 15                            far, kinds and five group cases fail (three feature tests fail too)"""
import numpy as np
import pytest

from tests import critical_reference as R
from tests import decode_limit_cases as DL
from tests import decode_reference as D
from tests import generator_limit_cases as LC
from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _same(got, want, keys, what):
    for key in keys:
        g = got[key].cpu().numpy()
        w = np.asarray(want[key])
        assert g.shape == w.shape, (what, key, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError("%s: %s differs at %d places, first at %s: got %s, want %s" %
                                 (what, key, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def _emitted_again(torch, b, c, ref, what):
    """The emitted moves that reference(c) chose, decoded as moves and as materialised plans."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    em = ref["emitted"]
    E = em["d"].shape[1]
    parents = torch.from_numpy(np.stack([np.stack([c.plans[i][d] for d in em["d"][i]]) for i in range(c.N)]))
    moves = torch.from_numpy(em["moves"])
    got = b.decode(parents, moves, E, want_table=True)
    _same(got, em["decode"], DL.DKEYS, what + ", emitted moves")
    made = sch.apply_moves(parents.cuda(), moves.cuda())
    again = b.decode(made, None, E, want_table=True)
    _same(again, em["decode"], DL.DKEYS, what + ", emitted moves materialised")


@pytest.mark.parametrize("name", DL.NAMES)
def test_limit_case(torch_gpu, name):
    from deep_reinforcement_learning_for_fjsp_amd._capi import FJSP_E_UNSUPPORTED, FjspError
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    torch = torch_gpu
    c = DL.case(name)
    b = EnvBatch(DL.set_of(c), c.N, variant=c.variant)
    assert b.decode_capacity() == c.cap and b.decode_group() == c.group, (name, b.decode_capacity(), b.decode_group())
    if c.group == 0:                                             # refused on the host, before any launch
        for call in (lambda: b.decode(torch.full((1, c.cap, 3), -1, dtype=torch.int32)),
                     lambda: b.critical(torch.full((1, c.cap, 6), -1, dtype=torch.int32))):
            with pytest.raises(FjspError) as err:
                call()
            assert err.value.code == FJSP_E_UNSUPPORTED and "exceeds 5120 bytes" in str(err.value), name
        return
    ref = DL.reference(c)
    plan, moves = torch.from_numpy(c.plan_array()), torch.from_numpy(c.move_array())
    got = b.decode(plan, moves, c.Q, want_table=True)
    _same(got, ref["decode"], DL.DKEYS, name + ", decode")
    lean = b.decode(plan, moves, c.Q)
    assert lean["table"] is None
    _same(lean, ref["decode"], ("objective", "status", "length"), name + ", decode without a table")
    crit = b.critical(torch.from_numpy(ref["tables"]), c.Q, c.max_moves)
    for key in R.KEYS:
        assert crit[key].cpu().numpy().dtype == ref["critical"][key].dtype, (name, key)
    _same(crit, ref["critical"], R.KEYS, name + ", critical")
    _emitted_again(torch, b, c, ref, name)
    if c.N > 1:                                                  # ... and one shared parent per env, q_plans = 1
        shared = torch.from_numpy(np.stack([c.plans[i][0] for i in range(c.N)]))
        mv = np.array([[(0, 0, 0) if c.combos[i][k][1] is None or c.combos[i][k][0] != 0 else c.combos[i][k][1] for k in c.pick] for i in range(c.N)], np.int32)
        want = D.decode([c.inst(i) for i in range(c.N)], c.variant, shared.numpy(), mv[:, :8], 8)
        _same(b.decode(shared, torch.from_numpy(np.ascontiguousarray(mv[:, :8])), 8, want_table=True), want, DL.DKEYS, name + ", shared parents")


def test_critical_at_the_last_int32(torch_gpu):
    """An extra beside clock-one, whose tables a decode wrote: the two-order clock case's tables 2^30 later (foreign tables
    with idle time in front): end + tail = C = 2^31 - 1."""
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    c = DL.case("clock-two")
    a, tabs = DL.shifted_clock_tables()
    b = EnvBatch(DL.set_of(c), 2, variant=0)
    both = np.stack([tabs, tabs])                                # env 1 plays the filler: every row fails its range check
    want = R.critical(c.arrs, both, len(tabs), 8)
    assert want["makespan"][0, 0] == DL.INT_MAX and np.all(want["makespan"][0] > 2 ** 31 - 2 ** 21)
    assert np.all(want["status"][0] == 0) and np.all(want["status"][1] == 1)
    _same(b.critical(torch_gpu.from_numpy(both), len(tabs), 8), want, R.KEYS, "shifted clock tables")


# ---- handles whose instances the device generated ------------------------------------------------------------------------
N_INST, N_ENVS, Q_GEN = DL.GEN_INST, DL.GEN_ENVS, DL.GEN_CANDIDATES
GEN = DL.gen_params()
SEED_A, SEED_B, SEED_C = DL.GEN_SEEDS
PLAYABLE = DL.PLAYABLE           # (tests/test_decode_limit_cases_host.py holds what these seeds make)


def _host_arrays(prm, seeds):
    from deep_reinforcement_learning_for_fjsp_amd import instances as fi
    s = fi.InstanceSet(len(seeds))
    for i, seed in enumerate(seeds):
        s.generate(i, seed, prm)
    return s, [s.arrays(i) for i in range(len(seeds))]


def _check_generated(torch, G, arrs, rs, what, old_plans=None, worst=True):
    """Fresh random plans of every env's instance (and, given, the plans of the instances the handle held before) through
    decode, their tables through critical, against the references on the host generator's arrays."""
    cap = G.decode_capacity()
    insts = [arrs[q % G.n_inst] for q in range(G.N)]
    plans = np.stack([[D.random_plan(a, rs, cap) for _ in range(Q_GEN)] for a in insts])
    mv = np.zeros((G.N, Q_GEN, 3), np.int32)
    mv[:, 1] = (DL.MOVE_MACHINE, 0, 1)
    mv[:, 2] = (DL.MOVE_SWAP, 0, 0)
    want = D.decode(insts, G.variant, plans, mv, Q_GEN, cap)
    _same(G.decode(torch.from_numpy(plans), torch.from_numpy(mv), Q_GEN, want_table=True), want, DL.DKEYS, what + ", decode")
    assert np.all(want["status"][:, 0] == 0) and (not worst or np.all(want["length"][:, 0] < cap)), what        # cap is the worst case
    tables = D.decode(insts, G.variant, plans, None, Q_GEN, cap)["table"]
    _same(G.critical(torch.from_numpy(tables), Q_GEN, 12), R.critical(insts, tables, Q_GEN, 12), R.KEYS, what + ", critical")
    if old_plans is not None:
        want_old = D.decode(insts, G.variant, old_plans, None, Q_GEN, cap)
        _same(G.decode(torch.from_numpy(old_plans), None, Q_GEN, want_table=True), want_old, DL.DKEYS, what + ", the old plans")
    return plans, want


@pytest.mark.parametrize("kind", list(GEN))
def test_generated_handles_decode_what_their_instances_are(torch_gpu, kind):
    """decode_kinds_kernel reads the record generate_pack_kernel wrote: after create, after a whole regenerate and after a
    masked one the plans decode exactly as the references say for the instances the handle holds now."""
    from deep_reinforcement_learning_for_fjsp_amd import schedule as sch
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch, global_actions
    torch = torch_gpu
    prm = GEN[kind]
    rs = np.random.RandomState(len(kind))
    G = EnvBatch.generated(prm, N_ENVS, SEED_A, n_inst=N_INST, rng_seed=5)
    _, arrs = _host_arrays(prm, [SEED_A + i for i in range(N_INST)])
    ops = [DL.ops_total(a) for a in arrs]
    base = prm if kind == "single" else prm.r.base
    cap = G.decode_capacity()
    assert cap == base.R_max * base.J_max * base.N_max * (1 if kind == "single" else 3) and cap > max(ops), (kind, cap, ops)
    assert (kind == "orders") == any(a.S > 1 for a in arrs)
    plans_a, want_a = _check_generated(torch, G, arrs, rs, kind + " created")
    # ---- a recorded episode decodes to its own table
    assert G.record_schedule() == cap
    T = max(ops)
    acts = torch.from_numpy(global_actions(17, 0, G.N, T, 6, 5)).cuda()
    G.reset()
    table, length = torch.full((G.N, cap, 6), -1, dtype=torch.int32, device="cuda"), torch.zeros(G.N, dtype=torch.int32, device="cuda")
    for t in range(T):                                           # (an env that is done starts over at its next step: keep its table)
        _, _, done = G.step(acts[t])
        new = (done != 0) & (length == 0)
        if bool(new.any()):
            tab, ln = G.schedule()
            table[new], length[new] = tab[new], ln[new]
    assert length.cpu().tolist() == [ops[q % N_INST] for q in range(G.N)]
    got = G.decode(sch.plan_of(table), want_table=True)
    assert bool((got["status"] == 0).all()) and torch.equal(got["length"][:, 0], length)
    if kind == "single":                                         # the environments' schedules are semi-active
        assert torch.equal(got["table"][:, 0], table)
    else:           # with arrivals a dispatch waits for the event clock (tests/test_gpu_decode.py: the golden order suites): never earlier
        assert torch.equal(got["table"][:, 0, :, :4], table[..., :4]) and bool((got["table"][:, 0, :, 4:] <= table[..., 4:]).all())
    insts = [arrs[q % N_INST] for q in range(G.N)]
    _same(got, D.decode(insts, 0, sch.plan_of(table).cpu().numpy(), None, 1, cap), DL.DKEYS, kind + " recorded")
    # ---- a whole regenerate: the old plans fail or decode differently exactly as the references say
    G.regenerate(SEED_B)
    _, arrs_b = _host_arrays(prm, [SEED_B + i for i in range(N_INST)])
    plans_b, want_b = _check_generated(torch, G, arrs_b, rs, kind + " regenerated", old_plans=plans_a)
    stale = D.decode([arrs_b[q % N_INST] for q in range(G.N)], 0, plans_a, None, Q_GEN, cap)
    assert any(not np.array_equal(stale[key], D.decode(insts, 0, plans_a, None, Q_GEN, cap)[key]) for key in DL.DKEYS), "the new instances decode the old plans alike"
    # ---- a masked regenerate: instances 0, 2 and 4 refreshed, 1 and 3 untouched
    mask = torch.tensor([1, 0, 1, 0, 1], dtype=torch.uint8, device="cuda")
    assert G.regenerate_masked(SEED_C, mask).cpu().tolist() == [1, 0, 1, 0, 1]
    seeds = [(SEED_C if i % 2 == 0 else SEED_B) + i for i in range(N_INST)]
    assert [G.instance_seed(i) for i in range(N_INST)] == seeds
    _, arrs_c = _host_arrays(prm, seeds)
    _check_generated(torch, G, arrs_c, rs, kind + " masked", old_plans=plans_b)


def test_a_failed_regenerate_refuses_both_entry_points_until_one_succeeds(torch_gpu):
    from deep_reinforcement_learning_for_fjsp_amd._capi import FJSP_E_STATE, FJSP_E_UNSUPPORTED, FjspError
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    torch = torch_gpu
    bad, good = LC.CASES["redraw_exhausted"], LC.CASES["redraw_deep"]
    # a generated MO_DFJSP handle is not decoded
    Gd = EnvBatch.generated(good["params"], good["n_inst"], good["seed"], variant=LC.VARIANT_MO_DFJSP, rng_seed=5)
    assert Gd.decode_group() == 0 and Gd.decode_capacity() > 0
    calls = lambda b: (lambda: b.decode(torch.full((b.N, b.decode_capacity(), 3), -1, dtype=torch.int32)),
                       lambda: b.critical(torch.full((b.N, b.decode_capacity(), 6), -1, dtype=torch.int32)))
    for call in calls(Gd):
        with pytest.raises(FjspError) as err:
            call()
        assert err.value.code == FJSP_E_UNSUPPORTED
    # The all-attempts-fail seed as the decoder can meet it: MO_DFJSP is refused before the handle's state is looked at, so
    # the same shop (one operation type, 32 machines) is generated as SO_DFJSP, which takes no shop with an idle machine
    # either and does not draw again.  One instance: only every 32nd seed plays.
    prm = bad["params"].o
    seed_bad = bad["seed"] + LC.EXHAUSTED_INSTANCE
    G = EnvBatch.generated(prm, 2, PLAYABLE[0], n_inst=1, variant=LC.VARIANT_SO_DFJSP, rng_seed=5)
    rs = np.random.RandomState(3)
    _check_generated(torch, G, _host_arrays(prm, PLAYABLE[:1])[1], rs, "before the failure", worst=False)
    with pytest.raises(FjspError) as err:
        G.regenerate(seed_bad)
    assert err.value.code == FJSP_E_UNSUPPORTED and "seed %d" % seed_bad in str(err.value)
    for call in calls(G):
        with pytest.raises(FjspError) as err:
            call()
        assert err.value.code == FJSP_E_STATE and "regenerate of this handle failed" in str(err.value)
    G.regenerate(PLAYABLE[1])
    _check_generated(torch, G, _host_arrays(prm, PLAYABLE[1:])[1], rs, "after the next regenerate", worst=False)


def test_improve_on_a_generated_handle_equals_the_host_made_batch(torch_gpu):
    """One round of improve(neighbourhood="critical") -- begin_order, critical, decode, apply_moves -- on a generated handle and
    on the equal batch made on the host: the same plans, objectives, history and tables."""
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as ps
    from deep_reinforcement_learning_for_fjsp_amd.batch import EnvBatch
    torch = torch_gpu
    prm = GEN["single"]
    G = EnvBatch.generated(prm, N_ENVS, SEED_A, n_inst=N_INST, rng_seed=5)
    s, arrs = _host_arrays(prm, [SEED_A + i for i in range(N_INST)])
    Hb = EnvBatch(s.solve_fluid(), N_ENVS, rng_seed=5)
    capg, caph = G.decode_capacity(), Hb.decode_capacity()
    assert capg > caph
    rs = np.random.RandomState(8)
    plan = np.stack([D.random_plan(arrs[q % N_INST], rs, capg) for q in range(N_ENVS)])
    og = ps.improve(G, torch.from_numpy(plan).cuda(), 1, neighbours=16, seed=4, neighbourhood="critical")
    oh = ps.improve(Hb, torch.from_numpy(plan[:, :caph]).cuda(), 1, neighbours=16, seed=4, neighbourhood="critical")
    for key in ("objective", "history", "accepted", "length"):
        assert torch.equal(og[key], oh[key]), key
    assert torch.equal(og["plan"][:, :caph], oh["plan"]) and torch.equal(og["table"][:, :caph], oh["table"])
    assert bool((og["plan"][:, caph:] == -1).all()) and int(og["accepted"].sum()) > 0
    want = D.decode([arrs[q % N_INST] for q in range(N_ENVS)], 0, og["plan"].cpu().numpy(), None, 1, capg)
    assert np.array_equal(og["objective"].cpu().numpy(), want["objective"][:, 0]) and np.array_equal(og["table"].cpu().numpy(), want["table"][:, 0])
