"""GPU: the batched solve (csrc/batch.hip, one workgroup per graph) against oracle Kruskal.

Every graph of every batch is compared with oracle.kruskal_c on its own canonical arrays: flags
bit-exact, weight and count equal. The batches sit on the size-class boundaries
(_native.BATCH_CLASS_LIMITS), on the loop caps' worst shapes and on the batch caps."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import fixture_names, load_fixture

pytestmark = pytest.mark.gpu

README = [(0, 1, 1), (0, 2, 4), (1, 2, 2), (1, 3, 5), (2, 3, 3), (2, 4, 7), (3, 4, 6), (3, 5, 8), (4, 5, 9)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from distributed_ghs_implementation_amd import _native
    assert _native.device_count() > 0
    return torch


def _native_mod():
    from distributed_ghs_implementation_amd import _native
    return _native


def _canon(n, u, v, w):
    from distributed_ghs_implementation_amd import canonicalize
    return canonicalize(n, u=np.asarray(u), v=np.asarray(v), w=np.asarray(w))


def _raw(n, u, v, w):
    from distributed_ghs_implementation_amd import CanonicalGraph
    return CanonicalGraph(n, u, v, w)


def _random(rng, n, m, wmax):
    return _canon(n, rng.integers(0, n, m), rng.integers(0, n, m), rng.integers(0, wmax + 1, m, dtype=np.int64))


def _device_solve(graphs):
    """batch_mst over the graphs -> (flags as a host uint8 array, results, offsets)."""
    from distributed_ghs_implementation_amd.device import DeviceBatch, batch_mst
    b = DeviceBatch.from_graphs(graphs)
    in_mst, res = batch_mst(b)
    return in_mst.cpu().numpy(), res, b.eoff.cpu().numpy().view("uint32").astype(np.int64)


def _check_graph(g, flags, r, what=""):
    from oracle import oracle
    ref_in, ref_tw, ref_k = oracle.kruskal_c(g.n, g.u, g.v, g.w)
    assert int(r["status"]) == 0, (what, int(r["status"]))
    assert np.array_equal(flags, ref_in), (what, g.n, g.m)
    assert int(r["total_weight"]) == ref_tw and int(r["num_mst_edges"]) == ref_k, (what, g.n, g.m)


def _check_all(graphs, flags, res, eoff, skip=()):
    assert len(res) == len(graphs) and len(flags) == int(eoff[-1])
    for k, g in enumerate(graphs):
        if k not in skip:
            _check_graph(g, flags[eoff[k]:eoff[k + 1]], res[k], what=k)


def test_golden_fixtures_in_one_batch(torch_cuda):
    from distributed_ghs_implementation_amd import canonicalize, minimum_spanning_forest_batch
    fxs = [load_fixture(n) for n in fixture_names()]
    graphs = [canonicalize(fx["num_nodes"], edges=[tuple(e) for e in fx["edges"]]) for fx in fxs]
    out = minimum_spanning_forest_batch(graphs)
    assert len(out) == len(fxs)
    for fx, r in zip(fxs, out):
        assert [list(t) for t in r.triples()] == fx["expected_mst_edges"], fx["name"]
        assert r.total_weight == fx["expected_total_weight"], fx["name"]
        assert r.stats == [] and r.ms_total > 0
    flags, res, eoff = _device_solve(graphs)
    _check_all(graphs, flags, res, eoff)


def test_class_boundaries_and_ties(torch_cuda):
    N = _native_mod()
    ns = {1, 2, 3, 63, 64, 65, 4095, 4096}
    for lim in N.BATCH_CLASS_LIMITS:
        ns |= {lim - 1, lim, lim + 1}
    ns = sorted(n for n in ns if 1 <= n <= N.BATCH_MAX_VERTICES)
    rng = np.random.default_rng(11)
    graphs = []
    for n in ns:
        for wmax in (0, 1, 3, (1 << 32) - 1):
            for m in (0, 1, n // 2, n, 2 * n, 5 * n, 10 * n):
                graphs.append(_random(rng, n, m, wmax))
    graphs.append(_canon(1, [], [], []))  # a lone vertex
    assert 250 <= len(graphs) <= 400
    order = rng.permutation(len(graphs))  # the classes interleave
    graphs = [graphs[i] for i in order]
    flags, res, eoff = _device_solve(graphs)
    _check_all(graphs, flags, res, eoff)
    assert int(res["rounds"].max()) <= 13


def _path(n, w):
    return _raw(n, np.arange(n - 1), np.arange(1, n), w)


def _grid(k, w):
    idx = np.arange(k * k).reshape(k, k)
    u = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    v = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    return _canon(k * k, u, v, np.full(len(u), w))


def test_worst_shapes_for_the_loops(torch_cuda):
    n = 4096
    a, b = np.triu_indices(64, 1)
    x = np.arange(1, n)
    graphs = [
        _path(n, np.arange(n - 1)),              # every vertex hooks its predecessor: one 4096-chain
        _path(n, np.arange(n - 1)[::-1].copy()),
        _raw(n, np.zeros(n - 1), np.arange(1, n), np.arange(n - 1) % 7),  # a star
        _grid(64, 5),                            # ties only
        _raw(64, a, b, np.full(len(a), 9)),      # K_64, ties only
        _path(n, np.full(n - 1, 3)),             # a path of ties
        _path(n, np.log2(x & -x).astype(np.int64)),  # w = ctz(eid + 1): fragments pair up, log2 n rounds
    ]
    flags, res, eoff = _device_solve(graphs)
    _check_all(graphs, flags, res, eoff)
    assert (res["status"] == 0).all()
    assert int(res["rounds"].max()) <= 13, res["rounds"]
    assert (res["num_mst_edges"] == np.array([g.n - 1 for g in graphs])).all()


def test_u64_totals(torch_cuda):
    n = 4096
    g = _path(n, np.full(n - 1, 0xFFFFFFFF, dtype=np.uint32))
    flags, res, eoff = _device_solve([g, g])
    _check_all([g, g], flags, res, eoff)
    assert int(res["total_weight"][0]) == 4095 * ((1 << 32) - 1) == int(res["total_weight"][1])


def test_forests(torch_cuda):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    rng = np.random.default_rng(3)
    graphs = []
    for n in (5, 64, 65, 300, 513, 2000, 4096):
        for frac in (0.0, 0.3, 0.6):
            graphs.append(_random(rng, n, int(frac * n), 4))  # sparse: isolated vertices, several components
    # two cliques and three isolated vertices
    a, b = np.triu_indices(5, 1)
    graphs.append(_canon(13, np.concatenate([a, a + 5]), np.concatenate([b, b + 5]), np.arange(2 * len(a))))
    flags, res, eoff = _device_solve(graphs)
    _check_all(graphs, flags, res, eoff)
    for g, r in zip(graphs, res):
        mat = coo_matrix((np.ones(g.m, np.int8), (g.u.astype(np.int64), g.v.astype(np.int64))), shape=(g.n, g.n))
        comps = int(connected_components(mat, directed=False, return_labels=False))
        assert int(r["num_mst_edges"]) == g.n - comps
    assert int(res["num_mst_edges"][-1]) == 13 - 5


def test_many_more_graphs_than_blocks(torch_cuda):
    from distributed_ghs_implementation_amd import canonicalize
    B = 20000
    base = canonicalize(6, edges=README)
    rng = np.random.default_rng(42)
    w = rng.permuted(np.tile(base.w, (B, 1)), axis=1)  # graph i: the nine README weights, permuted
    graphs = [_raw(6, base.u, base.v, w[i]) for i in range(B)]
    flags, res, eoff = _device_solve(graphs)
    assert (res["status"] == 0).all() and (res["num_mst_edges"] == 5).all()
    _check_all(graphs, flags, res, eoff)


BAD_FORMS = [([1, 0], [2, 3]), ([0, 0], [1, 9]), ([2], [1]), ([0, 0], [1, 1])]  # test_noncanonical_device_input_rejected


@pytest.mark.parametrize("form", range(len(BAD_FORMS)))
def test_bad_graph_in_the_middle(form, torch_cuda):
    from distributed_ghs_implementation_amd.mst import pack_batch
    N = _native_mod()
    rng = np.random.default_rng(100 + form)
    B = 40
    graphs = [_random(rng, int(n), int(3 * n), 5) for n in rng.choice([4, 30, 64, 65, 200, 600], B)]
    u, v = BAD_FORMS[form]
    graphs[B // 2] = _raw(4, u, v, [1] * len(u))
    flags, res, eoff = _device_solve(graphs)
    assert int(res["status"][B // 2]) == 1
    assert (np.delete(res["status"], B // 2) == 0).all()
    assert not flags[eoff[B // 2]:eoff[B // 2 + 1]].any()
    assert int(res["num_mst_edges"][B // 2]) == 0 and int(res["total_weight"][B // 2]) == 0
    _check_all(graphs, flags, res, eoff, skip={B // 2})
    # the host entry: GHS_E_NONCANON naming the graph, the healthy graphs still filled in
    L = N.load()
    nvert, eo, pu, pv, pw = pack_batch(graphs)
    hflags = np.full(int(eo[-1]), 7, np.uint8)
    hres = (N.BatchResult * B)()
    rc = L.ghs_mst_batch_host(B, nvert.ctypes.data, eo.ctypes.data, pu.ctypes.data, pv.ctypes.data, pw.ctypes.data,
                              hflags.ctypes.data, hres)
    assert rc == N.GHS_E_NONCANON
    assert f"graph {B // 2}:".encode() in L.ghs_last_error()
    assert np.array_equal(hflags, flags)
    assert np.array_equal(np.frombuffer(hres, dtype=N.BATCH_RESULT_DTYPE), res)
    from distributed_ghs_implementation_amd import minimum_spanning_forest_batch
    with pytest.raises(N.GHSError) as ei:
        minimum_spanning_forest_batch(graphs)
    assert ei.value.code == N.GHS_E_NONCANON and f"graph {B // 2}:" in str(ei.value)


def test_offsets_not_monotone(torch_cuda):
    """Graphs whose offsets run backwards or past eoff[B] get status 1 and are never touched."""
    import torch
    from distributed_ghs_implementation_amd.device import DeviceBatch, batch_mst
    from distributed_ghs_implementation_amd import canonicalize
    g = canonicalize(6, edges=README)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.uint32).view("int32"), device="cuda")
    pad = np.zeros(3, np.uint32)
    b = DeviceBatch(t([6, 6, 6]), t([0, 9, 12, 10]), t(np.concatenate([g.u, pad])), t(np.concatenate([g.v, pad])),
                    t(np.concatenate([g.w, pad])))
    in_mst, res = batch_mst(b)
    assert res["status"].tolist() == [0, 1, 1]
    _check_graph(g, in_mst.cpu().numpy()[:9], res[0])


def test_over_the_caps(torch_cuda):
    from distributed_ghs_implementation_amd import minimum_spanning_forest, minimum_spanning_forest_batch
    N = _native_mod()
    rng = np.random.default_rng(8)
    big = _random(rng, N.BATCH_MAX_VERTICES + 1, 20000, 50)
    a, b = np.triu_indices(1500, 1)
    dense = _raw(1500, a, b, rng.integers(0, 1000, len(a)))  # K_1500: over the edge cap
    assert dense.m > N.BATCH_MAX_EDGES
    small = _random(rng, 50, 200, 9)
    graphs = [small, big, small, dense, small]
    flags, res, eoff = _device_solve(graphs)
    assert res["status"].tolist() == [0, 3, 0, 3, 0]
    assert not flags[eoff[1]:eoff[2]].any() and not flags[eoff[3]:eoff[4]].any()
    _check_all(graphs, flags, res, eoff, skip={1, 3})
    out = minimum_spanning_forest_batch(graphs)  # oversized graphs go through the level engine, transparently
    for g, r in zip(graphs, out):
        single = minimum_spanning_forest(g)
        assert np.array_equal(r.in_mst, single.in_mst) and r.total_weight == single.total_weight
    assert out[0].stats == [] and len(out[1].stats) > 0
    # the host entry itself reports an oversized graph as an argument error, by index
    from distributed_ghs_implementation_amd.mst import pack_batch
    L = N.load()
    nvert, eo, pu, pv, pw = pack_batch(graphs[:3])
    hflags = np.zeros(int(eo[-1]), np.uint8)
    hres = (N.BatchResult * 3)()
    assert L.ghs_mst_batch_host(3, nvert.ctypes.data, eo.ctypes.data, pu.ctypes.data, pv.ctypes.data, pw.ctypes.data,
                                hflags.ctypes.data, hres) == N.GHS_E_ARG
    assert b"graph 1:" in L.ghs_last_error()


def test_batch_equals_single_and_is_deterministic(torch_cuda):
    from distributed_ghs_implementation_amd import minimum_spanning_forest, minimum_spanning_forest_batch
    rng = np.random.default_rng(21)
    graphs = [_random(rng, int(n), int(rng.integers(0, 6 * n)), int(wmax))
              for n, wmax in zip(rng.choice([2, 7, 64, 100, 512, 513, 1000, 4096], 20), rng.choice([0, 2, 1000], 20))]
    out = minimum_spanning_forest_batch(graphs)
    for g, r in zip(graphs, out):
        single = minimum_spanning_forest(g)
        assert np.array_equal(r.in_mst, single.in_mst)
        assert r.total_weight == single.total_weight and r.num_edges == single.num_edges
    f1, r1, _ = _device_solve(graphs)
    f2, r2, _ = _device_solve(graphs)
    assert f1.tobytes() == f2.tobytes() and r1.tobytes() == r2.tobytes()


def test_single_graph_and_side_stream(torch_cuda):
    import torch
    from distributed_ghs_implementation_amd import canonicalize
    from distributed_ghs_implementation_amd.device import DeviceBatch, batch_mst
    g = canonicalize(6, edges=README)
    flags, res, eoff = _device_solve([g])  # B = 1
    _check_all([g], flags, res, eoff)
    assert int(res["total_weight"][0]) == 20
    empty_in, empty_res = batch_mst(DeviceBatch.from_graphs([]))
    assert empty_in.numel() == 0 and len(empty_res) == 0
    rng = np.random.default_rng(2)
    graphs = [_random(rng, int(n), int(4 * n), 9) for n in rng.choice([5, 64, 70, 600], 200)]
    b = DeviceBatch.from_graphs(graphs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        in_mst, res = batch_mst(b)  # enqueued on `side`, read after that stream's sync
        side.synchronize()
        host = in_mst.cpu().numpy()
    torch.cuda.current_stream().wait_stream(side)
    _check_all(graphs, host, res, b.eoff.cpu().numpy().view("uint32").astype(np.int64))


def test_rank_mapped_weights(torch_cuda):
    from distributed_ghs_implementation_amd import canonicalize, minimum_spanning_forest_batch
    from oracle import oracle
    rng = np.random.default_rng(9)
    graphs = []
    for n in (6, 40, 65, 700):
        m = 4 * n
        u, v = rng.integers(0, n, m), rng.integers(0, n, m)
        graphs.append(canonicalize(n, u=u, v=v, w=rng.choice([0.5, -1.25, 3.0, 2.75, 1e9, -1e-3], m)))
        graphs.append(canonicalize(n, u=u, v=v, w=rng.integers(-5, 6, m)))
    assert all(g.weights is not None for g in graphs)
    out = minimum_spanning_forest_batch(graphs)
    for g, r in zip(graphs, out):
        ref_in, _, ref_k = oracle.kruskal_c(g.n, g.u, g.v, g.w)  # on the ranks: the same order, ties kept
        assert np.array_equal(r.in_mst, ref_in.astype(bool)) and r.num_edges == ref_k
        mine = [c for _, _, c in r.triples()]
        assert mine == g.weights[ref_in.astype(bool)].tolist()  # the caller's values, not the ranks
        assert r.total_weight == pytest.approx(sum(mine))


def test_cli_batch_dir(tmp_path, torch_cuda):
    from distributed_ghs_implementation_amd import __main__ as cli
    from distributed_ghs_implementation_amd import graph as G
    names = ["cgf_n6.json", "readme6.json", "ties_0.json", "thread_cfg1.json", "simple3.json"]
    exp = {}
    for i, name in enumerate(names):
        fx = load_fixture(name)
        g = G.canonicalize(fx["num_nodes"], edges=[tuple(e) for e in fx["edges"]])
        key = f"g{i}_{name.split('.')[0]}"
        if i == 4:
            key += ".mstbin"
            G.write_mstbin(str(tmp_path / key), g)
        else:
            G.write_graph_dir(g, str(tmp_path / key))
        exp[key] = fx
    assert cli.main(["--batch-dir", str(tmp_path), "--check", "--quiet"]) == 0
    outs = [str(tmp_path / k / "ghs_mst.json") for k in sorted(exp) if not k.endswith(".mstbin")]
    outs.append(str(tmp_path / "g4_simple3.ghs_mst.json"))
    assert len(outs) == 5
    for path, key in zip(outs, sorted(exp)):
        got = json.load(open(path))
        assert got["mst_edges"] == exp[key]["expected_mst_edges"], key
        assert got["total_weight"] == exp[key]["expected_total_weight"]
    records = json.load(open(tmp_path / "ghs_experiments.json"))
    assert [r["experiment"] for r in records] == sorted(exp)
    for r in records:
        assert r["is_correct"] is True
        assert r["mst_weight"] == exp[r["experiment"]]["expected_total_weight"]
        assert r["edges_found"] == r["edges_expected"]
    assert len([f for f in os.listdir(tmp_path) if f == "ghs_experiments.json"]) == 1
