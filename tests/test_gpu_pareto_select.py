"""GPU: fjsp_pareto_select (csrc/fjsp_pareto.hip) against its numpy restatement (tests/pareto_reference.py): index, count
and mask bit for bit on every shape class (one candidate, fewer / exactly / more than one wavefront's 64, exactly / more
than the workgroup's 256, the limit of 1024; 1..4 objectives), fill (ties, duplicates, signed zeros, NaN, infinities, an
anti-chain, a chain, all equal, invalid candidates, a source with no candidate) and cap; and pareto.gd / igd / spread
against what the reference's DataProcess computed (tests/golden/pareto_reference.npz)."""
import numpy as np
import pytest

from tests import pareto_reference as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 2), (63, 2), (64, 2), (65, 2), (64, 4), (256, 3), (257, 4), (1024, 3), (1024, 1)]       # (C, D)
N_SRC = (1, 5, 257)
FILLS = ("random", "ties", "zeros", "antichain", "chain", "equal", "nan", "inf", "valid", "empty_source")


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _fill(kind, C, N, D, rs):
    """(obj f64[C, N, D], valid u8[C, N] or None)"""
    obj, valid = rs.standard_normal((C, N, D)) * 100.0, None
    order = np.argsort(rs.rand(C, N), axis=0).astype(np.float64)        # a permutation of 0..C-1 per source env
    if kind == "ties":
        obj = rs.randint(0, 4, (C, N, D)).astype(np.float64)
    elif kind == "zeros":
        obj = rs.randint(-1, 2, (C, N, D)).astype(np.float64)
        obj = np.where(obj == 0.0, np.where(rs.rand(C, N, D) < 0.5, 0.0, -0.0), obj)
    elif kind == "antichain":                # (i, C-1-i, i, C-1-i): every candidate on the front when D >= 2
        obj = np.stack([order if d % 2 == 0 else C - 1 - order for d in range(D)], axis=2)
    elif kind == "chain":
        obj = np.stack([order] * D, axis=2)
    elif kind == "equal":
        obj = np.full((C, N, D), 7.0)
    elif kind == "nan":
        obj = rs.randint(0, 6, (C, N, D)).astype(np.float64)
        obj[rs.rand(C, N, D) < 0.2] = np.nan
        obj[rs.rand(C, N, D) < 0.05] = -np.nan
    elif kind == "inf":
        obj = rs.randint(0, 3, (C, N, D)).astype(np.float64)
        obj[rs.rand(C, N, D) < 0.2] = np.inf
        obj[rs.rand(C, N, D) < 0.2] = -np.inf
    elif kind == "valid":
        obj = rs.randint(0, 5, (C, N, D)).astype(np.float64)
        valid = (rs.rand(C, N) < 0.6).astype(np.uint8) * rs.randint(1, 256, (C, N)).astype(np.uint8)
    elif kind == "empty_source":
        obj = np.stack([order if d % 2 == 0 else C - 1 - order for d in range(D)], axis=2)
        valid = np.ones((C, N), np.uint8)
        valid[:, 0] = 0                       # source 0: no valid candidate; the last source: every vector has a NaN
        obj[np.arange(C), N - 1, rs.randint(0, D, C)] = np.nan
    return np.ascontiguousarray(obj, np.float64), valid


def _run(torch, obj, valid, cap):
    from deep_reinforcement_learning_for_fjsp_amd import pareto
    got = pareto.select(torch.from_numpy(obj).cuda(), None if valid is None else torch.from_numpy(valid).cuda(), cap)
    return [x.cpu().numpy() for x in got]


def _same(got, want, what):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.uint8, what
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), what + ": index"
    assert np.array_equal(got[1], want[1]), what + ": count"
    assert np.array_equal(got[2], want[2]), what + ": mask"


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_kernel_equals_reference(torch_gpu, shape, fill):
    C, D = shape
    for N in N_SRC:
        rs = np.random.RandomState(1000 * C + 10 * D + N + 7 * FILLS.index(fill))
        obj, valid = _fill(fill, C, N, D, rs)
        full = R.select(obj, valid)
        what = "%s %s n_src %d" % (shape, fill, N)
        if fill == "antichain" and D >= 2:
            assert np.all(full[1] == C), what
        if fill in ("chain", "equal"):
            assert np.all(full[1] == 1), what
            assert fill == "chain" or np.all(full[0][:, 0] == 0), what
        if fill == "empty_source":
            assert full[1][0] == 0 and full[1][N - 1] == 0 and np.all(full[0][0] == -1), what
        below = max(1, min(C, int(full[1].max()) - 1))                    # a cap below the largest front, when there is room
        for cap in sorted({1, C, below}):
            _same(_run(torch_gpu, obj, valid, cap), R.capped(full, cap), what + " cap %d" % cap)


def test_two_runs_are_bitwise_equal_and_front_points(torch_gpu):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import pareto
    rs = np.random.RandomState(11)
    for C, D in ((64, 2), (300, 3)):
        obj, _ = _fill("ties", C, 129, D, rs)
        obj[rs.rand(C, 129) < 0.1, 0] = np.nan
        d_obj = torch.from_numpy(obj).cuda()
        a, b = pareto.select(d_obj, cap=9), pareto.select(d_obj, cap=9)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        pts = pareto.front_points(d_obj, a[0]).cpu().numpy()
        assert np.array_equal(pts.view(np.uint64), R.front_points(obj, a[0].cpu().numpy()).view(np.uint64))


def test_graph_capture_replays_on_new_values(torch_gpu):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import pareto
    rs = np.random.RandomState(5)
    for C, D in ((40, 2), (130, 3)):
        obj, valid = _fill("valid", C, 65, D, rs)
        d_obj, d_valid = torch.from_numpy(obj).cuda(), torch.from_numpy(valid).cuda()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            pareto.select(d_obj, d_valid, 6)                        # (warm-up outside the capture)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="relaxed"):
            out = pareto.select(d_obj, d_valid, 6)
        obj2, valid2 = _fill("valid", C, 65, D, rs)
        d_obj.copy_(torch.from_numpy(obj2)); d_valid.copy_(torch.from_numpy(valid2))
        graph.replay()
        torch.cuda.synchronize()
        assert not np.array_equal(R.select(obj, valid, 6)[0], R.select(obj2, valid2, 6)[0])
        _same([x.cpu().numpy() for x in out], R.select(obj2, valid2, 6), "replay %d x %d" % (C, D))


def test_argument_errors(torch_gpu):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import _capi, pareto
    lib, p = _capi.lib(), _capi.ptr
    obj = torch.zeros(4, 3, 2, dtype=torch.float64, device="cuda")
    index = torch.full((3, 4), 99, dtype=torch.int32, device="cuda")
    count = torch.full((3,), 99, dtype=torch.int32, device="cuda")
    mask = torch.full((4, 3), 99, dtype=torch.uint8, device="cuda")
    call = lambda o, n_src, n_cand, n_obj, cap, ix, ct: lib.fjsp_pareto_select(o, None, n_src, n_cand, n_obj, cap, ix, ct, p(mask), None)
    bad = [(None, 3, 4, 2, 4, p(index), p(count)), (p(obj), 3, 4, 2, 4, None, p(count)), (p(obj), 3, 4, 2, 4, p(index), None),
           (p(obj), 0, 4, 2, 4, p(index), p(count)), (p(obj), -1, 4, 2, 4, p(index), p(count)),
           (p(obj), 3, 0, 2, 1, p(index), p(count)), (p(obj), 3, 1025, 2, 4, p(index), p(count)),
           (p(obj), 3, 4, 0, 4, p(index), p(count)), (p(obj), 3, 4, 5, 4, p(index), p(count)),
           (p(obj), 3, 4, 2, 0, p(index), p(count)), (p(obj), 3, 4, 2, 5, p(index), p(count))]
    for args in bad:
        assert call(*args) == _capi.FJSP_E_ARG, args[1:5]
        assert b"fjsp_pareto_select" in lib.fjsp_last_error()
    torch.cuda.synchronize()
    assert bool((index == 99).all()) and bool((count == 99).all()) and bool((mask == 99).all())      # nothing was launched
    assert call(p(obj), 3, 4, 2, 4, p(index), p(count)) == 0
    torch.cuda.synchronize()
    assert count.tolist() == [1, 1, 1] and index[:, 0].tolist() == [0, 0, 0] and bool((index[:, 1:] == -1).all())
    with pytest.raises(_capi.FjspError):
        pareto.select(obj, cap=5)
    with pytest.raises(ValueError):
        pareto.select(obj.float())
    with pytest.raises(ValueError):
        pareto.select(obj.cpu())


def test_select_and_metrics_equal_the_reference_results(torch_gpu):
    """Grouped by shape, the golden point sets as source envs of one batch: the kernel's fronts are filter_pareto_front's
    arrays, and the device metrics are within the host test's bounds of calculate_gd / _igd / _spread."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import pareto
    sets = R.golden_sets()
    for D in (1, 2, 3, 4):
        group = [s for s in sets if s["D"] == D]
        N, F, T = len(group), max(len(s["front"]) for s in group), max(len(s["true_front"]) for s in group)
        front, true = np.full((N, F, D), np.nan), np.full((N, T, D), np.nan)
        for C in sorted({s["C"] for s in group}):
            sub = [(i, s) for i, s in enumerate(group) if s["C"] == C]
            obj = torch.from_numpy(np.stack([s["points"] for _, s in sub], axis=1)).cuda()            # [C, n, D]
            index, count, _ = pareto.select(obj)
            pts = pareto.front_points(obj, index).cpu().numpy()
            for k, (i, s) in enumerate(sub):
                n = int(count[k])
                assert n == len(s["front"]) and np.array_equal(pts[k, :n], s["front"]) and np.all(np.isnan(pts[k, n:])), (C, D, k)
                front[i, :n] = pts[k, :n]
        for i, s in enumerate(group):
            true[i, :len(s["true_front"])] = s["true_front"]
        fc = torch.tensor([len(s["front"]) for s in group], dtype=torch.int32, device="cuda")
        tc = torch.tensor([len(s["true_front"]) for s in group], dtype=torch.int32, device="cuda")
        d_front, d_true = torch.from_numpy(front).cuda(), torch.from_numpy(true).cuda()
        got = dict(gd=pareto.gd(d_front, fc, d_true, tc), igd=pareto.igd(d_front, fc, d_true, tc), spread=pareto.spread(d_front, fc, d_true, tc))
        got = {k: v.cpu().numpy() for k, v in got.items()}
        mx = np.array([s["true_front"].max(axis=0) for s in group])
        with np.errstate(all="ignore"):
            norm = pareto.normalise(d_front, torch.from_numpy(mx).cuda()).cpu().numpy()
        for i, s in enumerate(group):
            bounds = dict(gd=R.gd(s["true_front"], s["front"])[1], igd=R.igd(s["true_front"], s["front"])[1],
                          spread=R.spread(s["front"], s["true_front"])[1])
            for name in ("gd", "igd", "spread"):
                what = (name, s["C"], D, s["range"], s["seed"], got[name][i], s[name], bounds[name])
                if np.isnan(s[name]):
                    assert np.isnan(got[name][i]), what
                else:
                    assert abs(got[name][i] - s[name]) <= bounds[name], what
            assert np.array_equal(norm[i, :len(s["front"])], s["normalised"], equal_nan=True), (s["C"], D)
