"""GPU: fjsp_beam_select (csrc/fjsp_beam.hip) against its numpy restatement (tests/beam_reference.py): parent, action and
cost of every rank, bit for bit, on every shape class (one candidate, fewer / exactly / more than 64 candidates, the
limits) and cost fill (ties, signed zeros, +inf beams, NaN, empty sources, done beams)."""
import numpy as np
import pytest

from tests import beam_reference as R

pytestmark = pytest.mark.gpu

# (width_in, n_actions, width_out): the last six have 63, 64, 65 candidates as a product and in one beam
SHAPES = [(1, 1, 1), (1, 30, 4), (4, 30, 4), (3, 18, 5), (2, 120, 8), (64, 128, 64),
          (7, 9, 7), (8, 8, 8), (5, 13, 5), (1, 63, 3), (1, 64, 3), (1, 65, 3)]
N_SRC = (1, 5, 257)
FILLS = ("random", "ties", "zeros", "inf_beams", "nan", "empty_sources", "done", "done_null")


@pytest.fixture(scope="module")
def torch_gpu(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _fill(kind, W, N, A, rs):
    """(cost f64[W, N, A], done u8[W, N] or None)"""
    cost, done = rs.standard_normal((W, N, A)) * 100.0, None
    if kind == "ties":
        cost = rs.randint(0, 3, (W, N, A)).astype(np.float64)
    elif kind == "zeros":
        cost = np.where(rs.rand(W, N, A) < 0.5, 0.0, -0.0) * np.where(rs.rand(W, N, A) < 0.7, 1.0, 0.0) + rs.randint(-1, 2, (W, N, A))
        cost = np.where(cost == 0.0, np.where(rs.rand(W, N, A) < 0.5, 0.0, -0.0), cost)
    elif kind == "inf_beams":
        cost[rs.rand(W, N) < 0.5] = np.inf
        cost[rs.rand(W, N, A) < 0.05] = -np.inf
    elif kind == "nan":
        cost = rs.randint(0, 4, (W, N, A)).astype(np.float64)
        cost[rs.rand(W, N, A) < 0.2] = np.nan
        cost[rs.rand(W, N, A) < 0.05] = -np.nan
    elif kind == "empty_sources":
        cost[:, rs.rand(N) < 0.5, :] = np.inf
        cost[:, 0, :] = np.nan                    # (at least one source with no candidate at all)
    elif kind in ("done", "done_null"):
        cost = rs.randint(0, 5, (W, N, A)).astype(np.float64)           # finite values in the entries a done beam ignores
        cost[rs.rand(W, N, A) < 0.1] = np.inf
        done = (rs.rand(W, N) < 0.5).astype(np.uint8) if kind == "done" else None
    return np.ascontiguousarray(cost, np.float64), done


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%d" % s)
def test_kernel_equals_reference(torch_gpu, shape, fill):
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    W, A, Wo = shape
    for N in N_SRC:
        rs = np.random.RandomState(1000 * W + 10 * A + N + 7 * FILLS.index(fill))
        cost, done = _fill(fill, W, N, A, rs)
        want = R.beam_select(cost, done, Wo)
        got = PS.beam_select(torch.from_numpy(cost).cuda(), None if done is None else torch.from_numpy(done).cuda(), Wo)
        got = [x.cpu().numpy() for x in got]
        what = "%s %s n_src %d" % (shape, fill, N)
        assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float64, what
        assert np.array_equal(got[0], want[0]), what + ": parent"
        assert np.array_equal(got[1], want[1]), what + ": action"
        assert np.array_equal(got[2].view(np.uint64), want[2].view(np.uint64)), what + ": cost"
        if fill == "empty_sources":
            assert np.all(want[0][:, 0] == -1) and np.all(np.isinf(want[2][:, 0]))
        if fill == "done":
            assert W * N < 8 or np.any(want[1] == -1)


def test_width_out_differs_from_width_in_and_graph_capture(torch_gpu):
    """More ranks asked for than candidates exist, fewer than beams exist, and the launch replayed from a captured graph
    (stream-ordered, no host synchronisation)."""
    torch = torch_gpu
    from deep_reinforcement_learning_for_fjsp_amd import policy_search as PS
    rs = np.random.RandomState(5)
    for W, A, Wo in ((2, 3, 64), (64, 2, 1), (16, 30, 3)):
        cost, _ = _fill("ties", W, 33, A, rs)
        want = R.beam_select(cost, None, Wo)
        got = [x.cpu().numpy() for x in PS.beam_select(torch.from_numpy(cost).cuda(), None, Wo)]
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (W, A, Wo)
    cost, done = _fill("done", 4, 65, 30, rs)
    d_cost, d_done = torch.from_numpy(cost).cuda(), torch.from_numpy(done).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        PS.beam_select(d_cost, d_done, 4)                      # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="relaxed"):
        out = PS.beam_select(d_cost, d_done, 4)
    cost2, done2 = _fill("done", 4, 65, 30, rs)
    d_cost.copy_(torch.from_numpy(cost2)); d_done.copy_(torch.from_numpy(done2))
    graph.replay()
    torch.cuda.synchronize()
    want = R.beam_select(cost2, done2, 4)
    for g, w in zip(out, want):
        assert np.array_equal(g.cpu().numpy(), w)
