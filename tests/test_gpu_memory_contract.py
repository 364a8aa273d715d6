"""The other half of the C ABI in include/ghs_mst.h, for every device entry point: a call writes only the
outputs and the workspace it was given, and its result does not depend on what those buffers held before.

Every case calls the C entry itself (tests/contract_cases.py) with all its device pointers carved out of one
Arena (tests/arena.py): 64 KiB of red zone on both sides of every buffer, every pointer aligned as the header
asks and no more, the workspace exactly as long as the library's own *_bytes function says. Each case runs
once per fill (0x00 and 0xA5: a stray store of any constant changes a byte under one of them), and after the
call and a sync:
  (a) no red-zone byte changed;
  (b) the inputs are byte-identical (w under the in-place form of ghs_mutual_reach_device excepted);
  (c) the defined part of every output equals the CPU reference of the per-module tests;
  (d) the defined part of every output and every result struct (without its ms_* fields) is byte-identical
      across the fills: nothing depends on what an output, a workspace or a flag array held before;
  (e) with one byte less than the declared size the call returns GHS_E_NOMEM and the whole arena is unchanged.
Nothing about timing is asserted, and no number here comes from the code under test."""
import pytest

import contract_cases as C
from arena import FILLS

pytestmark = pytest.mark.gpu

BIG = 96 << 20     # the solver's workspace is 35 MiB at any size


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert C.native().device_count() > 0
    return torch


def contract(torch, entry, *args, capacity=24 << 20, sized=True, ws_unused=False):
    """sized: the entry declares a workspace / temp / index size, so (e) applies. ws_unused: the header lets
    the workspace pointer be NULL for this input (labels, root, dendro, verify and mreach at m == 0: "only the
    output pointers are needed"), so its size cannot matter: the short call may also succeed, and must then
    still satisfy (a) and (c)."""
    N = C.native()
    runs = []
    for fill in FILLS:
        ctx = C.Ctx(torch, fill, capacity=capacity)
        got, want = entry(ctx, *args)
        ctx.sync()
        bad = ctx.A.check()
        assert not bad, ("(a) red zone", hex(fill), ctx.A.describe(bad))
        ctx.check_inputs()
        assert not ctx.problems, ("(b)", hex(fill), ctx.problems)
        C.assert_matches(got, want, ("(c)", hex(fill)))
        runs.append(C.frozen(got))
        del ctx
    assert runs[0].keys() == runs[1].keys()
    for k in runs[0]:
        assert runs[0][k] == runs[1][k], ("(d) differs between the fills", k)
    if not sized:
        return
    ctx = C.Ctx(torch, FILLS[1], short=1, capacity=capacity)
    try:
        got, want = entry(ctx, *args)
        rc = N.GHS_OK
    except C.Stop as e:
        rc = e.rc
    ctx.sync()
    if rc == N.GHS_OK and (ctx.sized_bytes == 0 or ws_unused):   # a declared size of 0 bytes leaves nothing to cut
        bad = ctx.A.check()
        assert not bad, ("(a) red zone, short workspace", ctx.A.describe(bad))
        C.assert_matches(got, want, "(c) short workspace")
        return
    assert rc == N.GHS_E_NOMEM, ("(e)", rc)
    assert ctx.A.unchanged(ctx.snap), "(e) the refused call wrote something"


SOLVER_GRAPHS = ("G0", "G1", "G1w", "G2", "G3", "G4")
FOREST_GRAPHS = ("G0", "G1", "G1w", "G2")


def _options(name):
    N = C.native()
    return {"default": 0, "no_tail": N.OPT_NO_TAIL, "bucketed": N.OPT_BUCKETED}[name]


# ---- the solver and what goes with it ---------------------------------------------------------------------------
@pytest.mark.parametrize("options", ["default", "no_tail", "bucketed"])
@pytest.mark.parametrize("form", ["coo", "csr_u", "csr"])
@pytest.mark.parametrize("g", SOLVER_GRAPHS)
def test_mst_device(torch_cuda, g, form, options):
    contract(torch_cuda, C.entry_solver, C.graph(g), form, _options(options), capacity=BIG)


@pytest.mark.parametrize("g", SOLVER_GRAPHS[:5])
def test_csr_offsets(torch_cuda, g):
    contract(torch_cuda, C.entry_csr_offsets, C.graph(g), sized=False)


@pytest.mark.parametrize("g,broken", [("G0", False)] + [(g, b) for g in ("G1", "G2", "G3") for b in (False, True)])
def test_check_canonical(torch_cuda, g, broken):
    contract(torch_cuda, C.entry_check_canonical, C.graph(g), broken, sized=False)


@pytest.mark.parametrize("lo,hi,exact", [(0, 0, False), (0, 0, True), (3, 2, False), (5, 1, True)])
@pytest.mark.parametrize("g", ("G0", "G1", "G2", "G4"))
def test_flags_to_eids(torch_cuda, g, lo, hi, exact):
    contract(torch_cuda, C.entry_flags_to_eids, C.graph(g), lo, hi, exact, sized=False)


def test_mst_batch_device(torch_cuda):
    contract(torch_cuda, C.entry_batch)


@pytest.mark.parametrize("with_src", [True, False])
def test_canonicalize_device(torch_cuda, with_src):
    contract(torch_cuda, C.entry_canonicalize, with_src)


@pytest.mark.parametrize("empty", [False, True])
@pytest.mark.parametrize("t", list(C.WEIGHT_TYPES))
def test_weight_ranks_device(torch_cuda, t, empty):
    contract(torch_cuda, C.entry_weight_ranks, t, empty)


@pytest.mark.parametrize("scale,ef,seed,wseed", [(12, 16, 1, 2), (5, 3, 7, 9)])
def test_rmat_generate(torch_cuda, scale, ef, seed, wseed):
    contract(torch_cuda, C.entry_rmat, scale, ef, seed, wseed)


@pytest.mark.parametrize("k,mode,wseed", [(33, 0, 2), (34, 1, 5)])
def test_grid_generate(torch_cuda, k, mode, wseed):
    contract(torch_cuda, C.entry_grid, k, mode, wseed, sized=False)


@pytest.mark.parametrize("g,which", [(g, "msf") for g in ("G0", "G1", "G1w", "G2", "G4")] + [("G1", "cycle"), ("G1w", "cycle")])
def test_verify_msf_device(torch_cuda, g, which):
    contract(torch_cuda, C.entry_verify, C.graph(g), which, ws_unused=C.graph(g).m == 0)


# ---- labels and the rooted forest -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["none", "max_weight", "num_clusters"])
@pytest.mark.parametrize("g,which", [(g, "msf") for g in FOREST_GRAPHS + ("G3",)] + [("G1", "cycle")])
def test_forest_labels_device(torch_cuda, g, which, kind):
    contract(torch_cuda, C.entry_labels, C.graph(g), which, kind, ws_unused=C.graph(g).m == 0)


@pytest.mark.parametrize("order", [True, False])
@pytest.mark.parametrize("g,which", [(g, "msf") for g in FOREST_GRAPHS + ("G3",)] + [("G1", "cycle")])
def test_forest_root_device(torch_cuda, g, which, order):
    contract(torch_cuda, C.entry_root, C.graph(g), which, order, ws_unused=C.graph(g).m == 0)


@pytest.mark.parametrize("outputs", [("key", "lca", "hops"), ("key",), ("lca", "hops")])
@pytest.mark.parametrize("g", FOREST_GRAPHS)
def test_forest_paths_create_and_query(torch_cuda, g, outputs):
    contract(torch_cuda, C.entry_paths, C.graph(g), outputs)


@pytest.mark.parametrize("by_edge", [True, False])
@pytest.mark.parametrize("g", FOREST_GRAPHS)
def test_forest_replace_device(torch_cuda, g, by_edge):
    contract(torch_cuda, C.entry_replace, C.graph(g), by_edge)


@pytest.mark.parametrize("hops", [False, True])
@pytest.mark.parametrize("g", FOREST_GRAPHS)
def test_forest_wdepth_device(torch_cuda, g, hops):
    contract(torch_cuda, C.entry_wdepth, C.graph(g), hops)


@pytest.mark.parametrize("with_lca", [True, False])
@pytest.mark.parametrize("hops", [False, True])
@pytest.mark.parametrize("g", FOREST_GRAPHS)
def test_forest_dist_query(torch_cuda, g, hops, with_lca):
    contract(torch_cuda, C.entry_dist_query, C.graph(g), hops, with_lca, sized=False)


@pytest.mark.parametrize("by_edge", [True, False])
@pytest.mark.parametrize("hops", [False, True])
@pytest.mark.parametrize("g", FOREST_GRAPHS)
def test_forest_edge_dist_device(torch_cuda, g, hops, by_edge):
    contract(torch_cuda, C.entry_edge_dist, C.graph(g), hops, by_edge, sized=False)


@pytest.mark.parametrize("with_ecc", [True, False])
@pytest.mark.parametrize("hops", [False, True])
@pytest.mark.parametrize("g", FOREST_GRAPHS)
def test_forest_diameter_device(torch_cuda, g, hops, with_ecc):
    contract(torch_cuda, C.entry_diameter, C.graph(g), hops, with_ecc)


# ---- dendrogram, clusters, mutual reachability ------------------------------------------------------------------
@pytest.mark.parametrize("children,sizes", [(True, True), (False, True), (True, False), (False, False)])
@pytest.mark.parametrize("g,which", [(g, "msf") for g in FOREST_GRAPHS] + [("G1", "cycle")])
def test_forest_dendro_device(torch_cuda, g, which, children, sizes):
    contract(torch_cuda, C.entry_dendro, C.graph(g), which, children, sizes, ws_unused=C.graph(g).m == 0)


@pytest.mark.parametrize("probabilities", [True, False])
@pytest.mark.parametrize("method", ["eom", "leaf"])
@pytest.mark.parametrize("g", FOREST_GRAPHS)
def test_forest_cluster_device(torch_cuda, g, method, probabilities):
    contract(torch_cuda, C.entry_cluster, C.graph(g), method, probabilities)


@pytest.mark.parametrize("mode", ["out", "inplace", "null"])
@pytest.mark.parametrize("g", FOREST_GRAPHS + ("G3",))
def test_mutual_reach_device(torch_cuda, g, mode):
    contract(torch_cuda, C.entry_mreach, C.graph(g), mode, ws_unused=C.graph(g).m == 0)
