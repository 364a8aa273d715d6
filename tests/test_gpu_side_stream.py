"""Every device entry point on a caller's stream that is not ordered with the null stream.

PyTorch's side streams are non-blocking, so in a real pipeline a hipMemsetAsync, rocPRIM call or launch that
the library put on the null stream instead of the caller's stream reads stale inputs, or runs ahead of the
launches it depends on. Each case (tests/contract_cases.py, one Arena, the same raw C calls as
test_gpu_memory_contract.py) makes that deterministic:
  1. the input views hold a decoy: another valid input of the same shape (a canonical graph of the same n and
     m with other edges and weights, its own flags, parents and weighted depths where those are inputs);
  2. on a fresh torch.cuda.Stream() a delay of ordinary queued device work is enqueued (a run of large fills),
  3. then the copies of the real inputs into the views;
  4. the delay must still be running (`not side.query()`: a condition, not a measurement; if it fires,
     lengthen the delay), and the entry is called with the side stream's handle;
  5. after side.synchronize() the outputs equal the CPU reference for the real inputs and the red zones are
     intact.
Handle-based calls build their index on the side stream the same way and issue their queries there, each
behind a delay of its own. G1 and G2 only, one fill."""
import pytest

import contract_cases as C

pytestmark = pytest.mark.gpu

GRAPHS = ("G1", "G2")
FILL = 0xA5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert C.native().device_count() > 0
    return torch


def side_run(torch, entry, *args, capacity=24 << 20):
    """Twice, on two streams created one after the other. The runtime spreads streams over a few hardware
    queues in turn; a side stream that shares its queue with the null stream is ordered with it by the queue
    itself, and a misplaced operation could not fail there. Two consecutive streams do not both share it."""
    for _ in range(2):
        ctx = C.Ctx(torch, FILL, side=torch.cuda.Stream(), capacity=capacity)
        got, want = entry(ctx, *args)
        ctx.sync()
        assert not ctx.real, ("inputs never delivered", list(ctx.real))
        bad = ctx.A.check()
        assert not bad, ("red zone", ctx.A.describe(bad))
        assert not ctx.problems, ctx.problems
        C.assert_matches(got, want, "side stream")


@pytest.mark.parametrize("form", ["coo", "csr_u", "csr"])
@pytest.mark.parametrize("options", ["default", "no_tail", "bucketed"])
@pytest.mark.parametrize("g", GRAPHS)
def test_mst_device(torch_cuda, g, options, form):
    N = C.native()
    opt = {"default": 0, "no_tail": N.OPT_NO_TAIL, "bucketed": N.OPT_BUCKETED}[options]
    side_run(torch_cuda, C.entry_solver, C.graph(g), form, opt, capacity=96 << 20)


@pytest.mark.parametrize("g", GRAPHS)
def test_csr_offsets(torch_cuda, g):
    side_run(torch_cuda, C.entry_csr_offsets, C.graph(g))


@pytest.mark.parametrize("broken", [False, True])
@pytest.mark.parametrize("g", GRAPHS)
def test_check_canonical(torch_cuda, g, broken):
    side_run(torch_cuda, C.entry_check_canonical, C.graph(g), broken)


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("g", GRAPHS)
def test_flags_to_eids(torch_cuda, g, exact):
    side_run(torch_cuda, C.entry_flags_to_eids, C.graph(g), 3, 2, exact)


def test_mst_batch_device(torch_cuda):
    side_run(torch_cuda, C.entry_batch)


@pytest.mark.parametrize("with_src", [True, False])
def test_canonicalize_device(torch_cuda, with_src):
    side_run(torch_cuda, C.entry_canonicalize, with_src)


@pytest.mark.parametrize("t", list(C.WEIGHT_TYPES))
def test_weight_ranks_device(torch_cuda, t):
    side_run(torch_cuda, C.entry_weight_ranks, t)


def test_generators(torch_cuda):
    """no device input to go stale: the delay still puts every launch behind queued work, so one that took
    the null stream would run ahead of the launches it depends on"""
    side_run(torch_cuda, C.entry_rmat, 12, 16, 1, 2)
    side_run(torch_cuda, C.entry_grid, 33, 0, 2)


@pytest.mark.parametrize("g", GRAPHS)
def test_verify_msf_device(torch_cuda, g):
    side_run(torch_cuda, C.entry_verify, C.graph(g), "msf")


@pytest.mark.parametrize("kind", ["none", "max_weight", "num_clusters"])
@pytest.mark.parametrize("g", GRAPHS)
def test_forest_labels_device(torch_cuda, g, kind):
    side_run(torch_cuda, C.entry_labels, C.graph(g), "msf", kind)


@pytest.mark.parametrize("order", [True, False])
@pytest.mark.parametrize("g", GRAPHS)
def test_forest_root_device(torch_cuda, g, order):
    side_run(torch_cuda, C.entry_root, C.graph(g), "msf", order)


@pytest.mark.parametrize("g", GRAPHS)
def test_forest_paths_create_and_query(torch_cuda, g):
    side_run(torch_cuda, C.entry_paths, C.graph(g), ("key", "lca", "hops"))


@pytest.mark.parametrize("by_edge", [True, False])
@pytest.mark.parametrize("g", GRAPHS)
def test_forest_replace_device(torch_cuda, g, by_edge):
    side_run(torch_cuda, C.entry_replace, C.graph(g), by_edge)


@pytest.mark.parametrize("hops", [False, True])
@pytest.mark.parametrize("g", GRAPHS)
def test_forest_wdepth_device(torch_cuda, g, hops):
    side_run(torch_cuda, C.entry_wdepth, C.graph(g), hops)


@pytest.mark.parametrize("hops", [False, True])
@pytest.mark.parametrize("g", GRAPHS)
def test_forest_dist_query(torch_cuda, g, hops):
    side_run(torch_cuda, C.entry_dist_query, C.graph(g), hops, True)


@pytest.mark.parametrize("by_edge", [True, False])
@pytest.mark.parametrize("g", GRAPHS)
def test_forest_edge_dist_device(torch_cuda, g, by_edge):
    side_run(torch_cuda, C.entry_edge_dist, C.graph(g), False, by_edge)


@pytest.mark.parametrize("hops,with_ecc", [(False, True), (True, False)])
@pytest.mark.parametrize("g", GRAPHS)
def test_forest_diameter_device(torch_cuda, g, hops, with_ecc):
    side_run(torch_cuda, C.entry_diameter, C.graph(g), hops, with_ecc)


@pytest.mark.parametrize("children,sizes", [(True, True), (False, False)])
@pytest.mark.parametrize("g", GRAPHS)
def test_forest_dendro_device(torch_cuda, g, children, sizes):
    side_run(torch_cuda, C.entry_dendro, C.graph(g), "msf", children, sizes)


@pytest.mark.parametrize("method,probabilities", [("eom", True), ("leaf", False)])
@pytest.mark.parametrize("g", GRAPHS)
def test_forest_cluster_device(torch_cuda, g, method, probabilities):
    side_run(torch_cuda, C.entry_cluster, C.graph(g), method, probabilities)


@pytest.mark.parametrize("mode", ["out", "inplace", "null"])
@pytest.mark.parametrize("g", GRAPHS)
def test_mutual_reach_device(torch_cuda, g, mode):
    side_run(torch_cuda, C.entry_mreach, C.graph(g), mode)
