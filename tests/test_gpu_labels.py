"""GPU: vertex labels and forest cuts (ghs_forest_labels_device, csrc/labels.hip) against a union-find.

The expected answer is computed here, on the host: K = the flagged edges after the cut (numpy; for a
count cut the flagged edges sorted by (w, eid) minus the last d), a union-find whose root is the
smallest vertex, clusters ranked by smallest vertex. Label arrays are compared whole and byte for
byte, together with every field of the result (flagged / kept / dropped edges, clusters, cut key,
is_forest)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, fixture_names, load_fixture

pytestmark = pytest.mark.gpu

U64_MAX = (1 << 64) - 1
INFO_FIELDS = ("flagged_edges", "kept_edges", "dropped_edges", "num_clusters", "cut_key", "is_forest")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from distributed_ghs_implementation_amd import _native
    assert _native.device_count() > 0
    return torch


def _oracle():
    from oracle import oracle
    return oracle


def _t(a, dtype=np.uint32):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.view("int32").copy() if dtype == np.uint32 else a.copy()).cuda()


def _edges(n, u, v, w):
    from distributed_ghs_implementation_amd.device import DeviceEdges
    return DeviceEdges(n, _t(u), _t(v), _t(w))


def _kruskal(n, u, v, w):
    return _oracle().kruskal_c(n, u, v, w)[0][: len(u)]


# ---- the expected answer ---------------------------------------------------------------------------
def uf_labels(n, u, v, kept):
    """Labels of the components of (V, kept edges): union-find rooted at the smallest vertex, clusters
    ranked by their smallest vertex."""
    par = list(range(n))

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x
    uu, vv = np.asarray(u)[kept].tolist(), np.asarray(v)[kept].tolist()
    for a, b in zip(uu, vv):
        ra, rb = find(a), find(b)
        if ra < rb:
            par[rb] = ra
        elif rb < ra:
            par[ra] = rb
    root = np.array([find(x) for x in range(n)], dtype=np.int64)
    roots = np.unique(root)
    assert np.array_equal(roots, np.flatnonzero(root == np.arange(n)))  # a root is its cluster's smallest vertex
    return np.searchsorted(roots, root).astype(np.uint32), len(roots)


def expected(n, u, v, w, flags, max_weight=None, num_clusters=None, values=None):
    """(labels, info) on the host. values: the weights the threshold is compared with (default w)."""
    u, v, w = (np.asarray(a, dtype=np.int64) for a in (u, v, w))
    T = np.flatnonzero(np.asarray(flags) != 0)
    cut_key = U64_MAX
    if max_weight is not None:
        vals = w if values is None else np.asarray(values)
        K = T[vals[T] <= max_weight]
    elif num_clusters is not None:
        order = T[np.lexsort((T, w[T]))]  # by (w, eid)
        d = min(max(num_clusters - (n - len(T)), 0), len(T))
        K = order[: len(T) - d]
        if d:
            e = int(order[len(T) - d])
            cut_key = (int(w[e]) << 32) | e
    else:
        K = T
    labels, clusters = uf_labels(n, u, v, K)
    info = {"flagged_edges": len(T), "kept_edges": len(K), "dropped_edges": len(T) - len(K),
            "num_clusters": clusters, "cut_key": cut_key, "is_forest": clusters == n - len(K)}
    return labels, info


def _labels(edges, flags_t, **cut):
    import torch

    from distributed_ghs_implementation_amd.device import forest_labels
    lab, info = forest_labels(edges, flags_t, **cut)
    assert lab.dtype == torch.int32 and lab.is_cuda and lab.numel() == edges.n
    return lab.cpu().numpy().view(np.uint32), info


def _check(n, u, v, w, flags, edges=None, flags_t=None, values=None, **cut):
    """Run the device call and compare labels and every result field with the host's; returns info."""
    e = _edges(n, u, v, w) if edges is None else edges
    ft = _t(np.asarray(flags) != 0, np.uint8) if flags_t is None else flags_t
    got, info = _labels(e, ft, **cut)
    want, winfo = expected(n, u, v, w, flags, values=values, **cut)
    assert np.array_equal(got, want), (cut, np.flatnonzero(got != want)[:8])
    assert {k: info[k] for k in INFO_FIELDS} == winfo, (cut, info, winfo)
    assert n == 0 or got[0] == 0
    return info


def _canon(n, u, v, w):
    from distributed_ghs_implementation_amd import canonicalize
    g = canonicalize(n, u=np.asarray(u), v=np.asarray(v), w=np.asarray(w))
    assert g.weights is None
    return g


def _random_canon(seed, n, m_raw, wmax, m_exact=None):
    rng = np.random.default_rng(seed)
    g = _canon(n, rng.integers(0, n, m_raw), rng.integers(0, n, m_raw), rng.integers(0, wmax + 1, m_raw))
    u, v, w = g.u, g.v, g.w
    if m_exact is not None:  # a prefix of a canonical list is canonical
        assert g.m >= m_exact
        u, v, w = u[:m_exact], v[:m_exact], w[:m_exact]
    return n, u, v, w


def _round_bound(n):
    return 2 * max(1, int(np.ceil(np.log2(max(n, 2))))) + 2


# ---- exhaustive: every flag vector of a small tie-heavy graph -------------------------------------
EX_N = 7  # vertex 6 is isolated
EX_EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (2, 4), (3, 4), (4, 5)]
EX_W = [1, 1, 2, 1, 2, 1, 1, 2, 1]


def test_exhaustive_all_flag_vectors_all_cuts(torch_cuda):
    """All 466 flag vectors with at most 6 flags (cyclic ones included: is_forest = 0, labels still
    exact) under no cut, every distinct weight and its neighbours as threshold, and k in
    {1, 2, 3, 7, 8}; the 46 vectors with 7 or more flags cannot be forests of 7 vertices: GHS_E_ARG.
    The vectors are rows of one 9-byte-pitch tensor, so the flag pointer takes every alignment."""
    from distributed_ghs_implementation_amd import _native
    from distributed_ghs_implementation_amd.device import forest_labels
    u = np.array([a for a, _ in EX_EDGES], np.uint32)
    v = np.array([b for _, b in EX_EDGES], np.uint32)
    w = np.array(EX_W, np.uint32)
    e = _edges(EX_N, u, v, w)
    allflags = np.array([[(bits >> k) & 1 for k in range(9)] for bits in range(512)], np.uint8)
    dev = _t(allflags.ravel(), np.uint8)
    thresholds = sorted({t for x in set(EX_W) for t in (x - 1, x, x + 1)})
    assert thresholds == [0, 1, 2, 3]
    cyclic = overfull = 0
    for bits in range(512):
        flags, ft = allflags[bits], dev[9 * bits: 9 * bits + 9]
        if int(flags.sum()) >= 7:
            overfull += 1
            for cut in ({}, {"max_weight": 1}, {"num_clusters": 2}):
                with pytest.raises(_native.GHSError) as ei:
                    forest_labels(e, ft, **cut)
                assert ei.value.code == _native.GHS_E_ARG and "more flags" in str(ei.value)
            continue
        info = _check(EX_N, u, v, w, flags, edges=e, flags_t=ft)
        cyclic += not info["is_forest"]
        for t in thresholds:
            _check(EX_N, u, v, w, flags, edges=e, flags_t=ft, max_weight=t)
        for k in (1, 2, 3, 7, 8):
            _check(EX_N, u, v, w, flags, edges=e, flags_t=ft, num_clusters=k)
    assert overfull == 46 and cyclic > 0


# ---- every golden fixture ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", fixture_names())
def test_golden_fixtures_components_of_the_graph(name, torch_cuda):
    """The oracle's flags, no cut: the labels are the connected components of the whole graph."""
    from distributed_ghs_implementation_amd import canonicalize
    fx = load_fixture(name)
    g = canonicalize(fx["num_nodes"], edges=[tuple(e) for e in fx["edges"]])
    ref = _kruskal(g.n, g.u, g.v, g.w)
    e = _edges(g.n, g.u, g.v, g.w)
    got, info = _labels(e, _t(ref, np.uint8))
    want, clusters = uf_labels(g.n, g.u, g.v, np.arange(g.m))
    assert np.array_equal(got, want)
    assert (info["num_clusters"], info["flagged_edges"], info["kept_edges"]) == (clusters, int(ref.sum()), int(ref.sum()))
    assert info["is_forest"] is True and info["cut_key"] == U64_MAX
    _check(g.n, g.u, g.v, g.w, ref, edges=e)


# ---- single linkage ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_single_linkage_property(seed, torch_cuda):
    """Cutting the MSF at t labels exactly the components of ALL edges with w <= t, for every t; a
    count cut into k gives exactly max(k, components) clusters and the host's cut key."""
    n, u, v, w = _random_canon(seed, 300, 1700, 7)
    assert 1300 <= len(u) <= 1700
    ref = _kruskal(n, u, v, w)
    e, ft = _edges(n, u, v, w), _t(ref, np.uint8)
    comps = n - int(ref.sum())
    for t in range(8):
        got, info = _labels(e, ft, max_weight=t)
        want, clusters = uf_labels(n, u, v, np.flatnonzero(w <= t))
        assert np.array_equal(got, want), t
        assert info["num_clusters"] == clusters and info["is_forest"] is True
        _check(n, u, v, w, ref, edges=e, flags_t=ft, max_weight=t)
    for k in (1, 2, 3, comps, comps + 1, 17, 150, n - 1, n, n + 5):
        info = _check(n, u, v, w, ref, edges=e, flags_t=ft, num_clusters=k)
        assert info["num_clusters"] == max(min(k, n), comps), k


# ---- shapes that stress the rounds and the jump ------------------------------------------------------
def _bitrev(i, bits):
    r = 0
    for _ in range(bits):
        r, i = (r << 1) | (i & 1), i >> 1
    return r


def _shape(kind):
    """(n, raw u, raw v, raw w): forests (or, for the grid, a graph whose MSF is taken)."""
    if kind == "path-id":
        n = 5000
        return n, np.arange(n - 1), np.arange(1, n), np.arange(n - 1) % 5
    if kind == "path-bitrev":  # the 5000-path over bit-reversed 13-bit ids; the other ids stay isolated
        p = np.array([_bitrev(i, 13) for i in range(5000)])
        return 8192, p[:-1], p[1:], np.arange(4999) % 5
    if kind == "path-interleaved":  # ids 0, k, 1, k + 1, ...
        k = 2500
        p = np.empty(5000, np.int64)
        p[0::2], p[1::2] = np.arange(k), k + np.arange(k)
        return 5000, p[:-1], p[1:], np.arange(4999) % 5
    if kind == "star-last":
        n = 4096
        return n, np.full(n - 1, n - 1), np.arange(n - 1), np.arange(n - 1) % 3
    if kind == "star-0":
        n = 4096
        return n, np.zeros(n - 1, np.int64), np.arange(1, n), np.arange(n - 1) % 3
    if kind == "caterpillar":  # a 1000-spine (ids 3i) with two legs per spine vertex
        s = 3 * np.arange(1000)
        return 3000, np.concatenate([s[:-1], s, s]), np.concatenate([s[1:], s + 1, s + 2]), np.arange(2999) % 4
    if kind == "grid-equal":
        k = 32
        ids = np.arange(k * k).reshape(k, k)
        u = np.concatenate([ids[:, :-1].ravel(), ids[:-1, :].ravel()])
        v = np.concatenate([ids[:, 1:].ravel(), ids[1:, :].ravel()])
        return k * k, u, v, np.full(len(u), 4)
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["path-id", "path-bitrev", "path-interleaved", "star-last", "star-0", "caterpillar",
                                  "grid-equal"])
def test_shapes_rounds_and_jump(kind, torch_cuda):
    n, ru, rv, rw = _shape(kind)
    g = _canon(n, ru, rv, rw)
    u, v, w = g.u, g.v, g.w
    flags = _kruskal(n, u, v, w)
    if kind != "grid-equal":
        assert flags.all()  # the shape is a forest
    e, ft = _edges(n, u, v, w), _t(flags, np.uint8)
    info = _check(n, u, v, w, flags, edges=e, flags_t=ft)
    assert info["is_forest"] is True and 1 <= info["rounds"] <= _round_bound(n)
    if kind == "path-id":
        assert info["rounds"] == 1  # every vertex hooks onto its predecessor: one chain 5000 long
    if kind in ("path-bitrev", "path-interleaved"):
        assert info["rounds"] >= 2
    for t in (0, 1, 3):
        assert _check(n, u, v, w, flags, edges=e, flags_t=ft, max_weight=t)["rounds"] <= _round_bound(n)
    for k in (2, 3, 1000):
        assert _check(n, u, v, w, flags, edges=e, flags_t=ft, num_clusters=k)["rounds"] <= _round_bound(n)


# ---- sizes at which a kernel takes another path ----------------------------------------------------
@pytest.mark.parametrize("m,flagged", [(4095, 1023), (4096, 1024), (4097, 1025), (4081, 2047), (4097, 2048),
                                       (8193, 2049), (4080, 255), (4112, 257)])
def test_tile_boundaries_of_the_flag_pass(m, flagged, torch_cuda):
    """A block of the flag pass covers 4096 flag bytes; a block iteration of the select's histogram and
    of the appending list passes 2048 entries (8 per thread), of the other list passes 256. Any
    `flagged` edges of the list are flagged (cycles allowed)."""
    n, u, v, w = _random_canon(m, 3000, 3 * m, 2, m_exact=m)
    rng = np.random.default_rng(flagged)
    flags = np.zeros(m, np.uint8)
    flags[1 + rng.choice(m - 2, size=flagged - 2, replace=False)] = 1
    flags[[0, m - 1]] = 1  # the first and the last edge among them
    assert int(flags.sum()) == flagged
    e, ft = _edges(n, u, v, w), _t(flags, np.uint8)
    _check(n, u, v, w, flags, edges=e, flags_t=ft)
    for t in (0, 1):
        _check(n, u, v, w, flags, edges=e, flags_t=ft, max_weight=t)
    c = expected(n, u, v, w, flags)[1]["num_clusters"]
    for k in (c + 1, c + int(flags.sum()) // 2, n):
        _check(n, u, v, w, flags, edges=e, flags_t=ft, num_clusters=k)


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2047, 2049, 4097])
def test_tile_boundaries_of_the_vertex_passes(n, torch_cuda):
    """A block of the root scan covers 1024 vertices; 4 vertices per lane with a scalar tail."""
    n, u, v, w = _random_canon(n, n, n + n // 2, 3)
    flags = _kruskal(n, u, v, w)
    e, ft = _edges(n, u, v, w), _t(flags, np.uint8)
    _check(n, u, v, w, flags, edges=e, flags_t=ft)
    _check(n, u, v, w, flags, edges=e, flags_t=ft, max_weight=1)
    _check(n, u, v, w, flags, edges=e, flags_t=ft, num_clusters=n // 3)


def test_unaligned_flags_and_labels_view(torch_cuda):
    """The flags may start at any byte (a slice): scalar head and tail around the 16-byte body."""
    m = 4099
    n, u, v, w = _random_canon(9, 3000, 3 * m, 2, m_exact=m)
    flags = np.zeros(m, np.uint8)
    flags[np.random.default_rng(5).choice(m, size=1500, replace=False)] = 1
    flags[[0, 1, m - 2, m - 1]] = 1
    e = _edges(n, u, v, w)
    for off in (1, 2, 3, 7, 8, 15, 17):
        buf = _t(np.concatenate([np.ones(off, np.uint8), flags, np.ones(21, np.uint8)]), np.uint8)
        view = buf[off: off + m]
        assert view.data_ptr() % 16 == off % 16
        _check(n, u, v, w, flags, edges=e, flags_t=view)
        _check(n, u, v, w, flags, edges=e, flags_t=view, max_weight=1)
        _check(n, u, v, w, flags, edges=e, flags_t=view, num_clusters=2000)
    # bool flags, a longer tensor than m, and a strided view made contiguous
    import torch
    ft = _t(flags, np.uint8)
    _check(n, u, v, w, flags, edges=e, flags_t=ft.to(torch.bool))
    _check(n, u, v, w, flags, edges=e, flags_t=torch.cat([ft, torch.ones(7, dtype=torch.uint8, device=ft.device)]))
    _check(n, u, v, w, flags, edges=e, flags_t=torch.stack([ft, ft], dim=1)[:, 0])


# ---- degenerate cases ------------------------------------------------------------------------------
def test_degenerate_cases(torch_cuda):
    z = np.zeros(0, np.uint32)
    for n in (1, 5):  # no edges: identity labels
        for cut in ({}, {"max_weight": 3}, {"num_clusters": 2}):
            info = _check(n, z, z, z, np.zeros(0, np.uint8), **cut)
            assert (info["num_clusters"], info["rounds"], info["is_forest"]) == (n, 0, True)
    # n = 2 with and without its edge
    assert _check(2, [0], [1], [5], [1])["num_clusters"] == 1
    assert _check(2, [0], [1], [5], [0])["num_clusters"] == 2
    assert _check(2, [0], [1], [5], [1], max_weight=4)["num_clusters"] == 2
    assert _check(2, [0], [1], [5], [1], max_weight=5)["num_clusters"] == 1
    assert _check(2, [0], [1], [5], [1], num_clusters=2)["cut_key"] == (5 << 32)
    # one edge among isolated vertices
    info = _check(1000, [3], [700], [9], [1])
    assert (info["num_clusters"], info["rounds"]) == (999, 1)
    # all-zero flags, k = 1 / n / > n, threshold 0 and 2^32 - 1
    n, u, v, w = _random_canon(21, 200, 900, 2)
    w = w.copy()
    w[::7] = 0xFFFFFFFF
    ref = _kruskal(n, u, v, w)
    e, ft = _edges(n, u, v, w), _t(ref, np.uint8)
    info = _check(n, u, v, w, np.zeros(len(u), np.uint8), edges=e)
    assert (info["num_clusters"], info["rounds"], info["flagged_edges"]) == (n, 0, 0)
    _check(n, u, v, w, np.zeros(len(u), np.uint8), edges=e, num_clusters=3)
    for k in (1, n, n + 1, 10 * n, (1 << 64) - 1):
        _check(n, u, v, w, ref, edges=e, flags_t=ft, num_clusters=k)
    assert _check(n, u, v, w, ref, edges=e, flags_t=ft, num_clusters=n)["num_clusters"] == n
    for t in (0, 0xFFFFFFFE, 0xFFFFFFFF):
        _check(n, u, v, w, ref, edges=e, flags_t=ft, max_weight=t)
    assert _check(n, u, v, w, ref, edges=e, flags_t=ft, max_weight=0xFFFFFFFF)["dropped_edges"] == 0


# ---- the engine's own output --------------------------------------------------------------------------
def _graph_components(g):
    return uf_labels(g.n, g.u, g.v, np.arange(g.m))


@pytest.mark.parametrize("graph", ["rmat12", "rmat14", "grid64-0", "grid64-1"])
def test_engine_output_labels_are_the_graph_components(graph, torch_cuda):
    from distributed_ghs_implementation_amd.device import DeviceMST, generate_grid, generate_rmat
    e = {"rmat12": lambda: generate_rmat(12), "rmat14": lambda: generate_rmat(14),
         "grid64-0": lambda: generate_grid(64, 0), "grid64-1": lambda: generate_grid(64, 1)}[graph]()
    eng = DeviceMST(e)
    res, _ = eng.run()
    before = eng.in_mst.clone()
    lab, info = eng.labels()
    g = e.to_host()
    want, clusters = _graph_components(g)
    assert np.array_equal(lab.cpu().numpy().view(np.uint32), want)
    assert info["num_clusters"] == clusters == g.n - res.num_mst_edges
    assert (info["flagged_edges"], info["kept_edges"], info["is_forest"]) == (res.num_mst_edges, res.num_mst_edges, True)
    assert info["rounds"] <= _round_bound(g.n)
    # the flags are only read: unchanged, and the verifier still accepts them
    assert bool((eng.in_mst == before).all())
    assert eng.verify()["ok"] is True
    flags = eng.in_mst_host()
    wmed = int(np.median(g.w[flags])) if flags.any() else 0
    _check(g.n, g.u, g.v, g.w, flags, edges=e, flags_t=eng.in_mst, max_weight=wmed)
    _check(g.n, g.u, g.v, g.w, flags, edges=e, flags_t=eng.in_mst, num_clusters=clusters + 100)
    lab2, info2 = eng.labels(num_clusters=clusters + 100)
    assert info2["num_clusters"] == clusters + 100


def test_engine_csr_and_emulated_ranks(torch_cuda):
    from distributed_ghs_implementation_amd.device import DeviceMST, emulated_mst, forest_labels, generate_rmat
    e = generate_rmat(12).with_csr()
    eng = DeviceMST(e)
    assert eng.csr
    eng.run()
    g = e.to_host()
    want, clusters = _graph_components(g)
    lab, info = forest_labels(e, eng.in_mst)  # the CSR engine's flags with the COO list
    assert np.array_equal(lab.cpu().numpy().view(np.uint32), want) and info["num_clusters"] == clusters
    _, _, in3 = emulated_mst(e, 3)
    lab3, info3 = forest_labels(e, in3)
    assert np.array_equal(lab3.cpu().numpy().view(np.uint32), want) and info3["num_clusters"] == clusters
    with pytest.raises(ValueError, match="CSR"):
        forest_labels(e.csr_only(), eng.in_mst)


# ---- rank-mapped weights ---------------------------------------------------------------------------
def test_rank_mapped_weights_threshold_in_caller_units(torch_cuda):
    from distributed_ghs_implementation_amd.device import DeviceEdges, DeviceMST
    rng = np.random.default_rng(77)
    n, m_raw = 400, 2500
    pool = np.array([-7.5, -2.25, -2.25, 0.0, 0.125, 1.0, 1.0, 3.5, 1e9, -1e-9])
    ru, rv = rng.integers(0, n, m_raw), rng.integers(0, n, m_raw)
    rw = pool[rng.integers(0, len(pool), m_raw)].astype(np.float64)
    e = DeviceEdges.from_raw(n, ru, rv, rw, rank_weights=True)
    assert e.weights is not None
    eng = DeviceMST(e)
    eng.run()
    g = e.to_host()
    flags = eng.in_mst_host()
    assert np.array_equal(flags, _kruskal(g.n, g.u, g.v, g.w).astype(bool))
    # below every weight, exactly a weight, between two, above all, infinities
    for t in (-8.0, -7.5, -2.25, -2.0, -1e-9, 0.0, 0.0625, 0.125, 1.0, 3.5, 5e8, 1e9, 2e9, float("inf"), float("-inf")):
        info = _check(g.n, g.u, g.v, g.w, flags, edges=e, flags_t=eng.in_mst, values=g.weights, max_weight=t)
        if t < -7.5:
            assert info["kept_edges"] == 0 and info["num_clusters"] == n
    lab, info = eng.labels(max_weight=1.0)
    want, _ = expected(g.n, g.u, g.v, g.w, flags, max_weight=1.0, values=g.weights)
    assert np.array_equal(lab.cpu().numpy().view(np.uint32), want)
    # int64 weights beyond 2^53: compared as integers
    big = (1 << 60) + rng.integers(-3, 4, m_raw).astype(np.int64)
    e2 = DeviceEdges.from_raw(n, ru, rv, big, rank_weights=True)
    eng2 = DeviceMST(e2)
    eng2.run()
    g2 = e2.to_host()
    for t in ((1 << 60) - 4, (1 << 60) - 3, (1 << 60), (1 << 60) + 1, (1 << 60) + 3, 1 << 62):
        _check(g2.n, g2.u, g2.v, g2.w, eng2.in_mst_host(), edges=e2, flags_t=eng2.in_mst, values=g2.weights, max_weight=t)


# ---- the host path ---------------------------------------------------------------------------------
def test_host_path_mstresult_labels(torch_cuda):
    from distributed_ghs_implementation_amd import canonicalize, minimum_spanning_forest
    fx = load_fixture("cgf_n1000_p001.json")
    g = canonicalize(fx["num_nodes"], edges=[tuple(e) for e in fx["edges"]])
    r = minimum_spanning_forest(g)
    lab = r.labels()
    assert lab.dtype == np.uint32 and np.array_equal(lab, _graph_components(g)[0])
    for cut in ({"max_weight": int(np.median(g.w))}, {"num_clusters": 40}):
        got, info = r.labels(return_info=True, **cut)
        want, winfo = expected(g.n, g.u, g.v, g.w, r.in_mst, **cut)
        assert np.array_equal(got, want) and {k: info[k] for k in INFO_FIELDS} == winfo
    # float weights, rank-mapped by canonicalize: the threshold is in the caller's units
    rng = np.random.default_rng(3)
    raw = [(int(a), int(b), float(c)) for a, b, c in zip(rng.integers(0, 150, 700), rng.integers(0, 150, 700),
                                                         rng.integers(-4, 5, 700) * 0.5)]
    gf = canonicalize(150, edges=raw)
    assert gf.weights is not None
    rf = minimum_spanning_forest(gf)
    assert np.array_equal(rf.labels(), _graph_components(gf)[0])
    for t in (-3.0, -2.0, -0.25, 0.0, 1.5, 2.0, 99.0):
        got, info = rf.labels(max_weight=t, return_info=True)
        want, winfo = expected(gf.n, gf.u, gf.v, gf.w, rf.in_mst, max_weight=t, values=gf.weights)
        assert np.array_equal(got, want) and {k: info[k] for k in INFO_FIELDS} == winfo, t
    got, info = rf.labels(num_clusters=10, return_info=True)
    want, winfo = expected(gf.n, gf.u, gf.v, gf.w, rf.in_mst, num_clusters=10)
    assert np.array_equal(got, want) and {k: info[k] for k in INFO_FIELDS} == winfo


def test_noncanonical_list_rejected(torch_cuda):
    from distributed_ghs_implementation_amd import _native
    from distributed_ghs_implementation_amd.device import forest_labels
    n, u, v, w = _random_canon(3, 50, 200, 3)
    ref = _kruskal(n, u, v, w)
    L = _native.load()
    for mutate in ("swap", "loop", "range"):
        bu, bv = u.copy(), v.copy()
        if mutate == "swap":
            bu[[3, 4]], bv[[3, 4]] = bu[[4, 3]], bv[[4, 3]]
        elif mutate == "loop":
            bv[5] = bu[5]
        else:
            bv[len(bv) - 1] = n
        with pytest.raises(_native.GHSError) as ei:
            forest_labels(_edges(n, bu, bv, w), _t(ref, np.uint8))
        assert ei.value.code == _native.GHS_E_NONCANON, mutate
        out = np.zeros(n, np.uint32)
        res = _native.LabelsResult()
        rc = L.ghs_forest_labels_host(n, len(bu), bu.ctypes.data, bv.ctypes.data, w.ctypes.data, ref.ctypes.data, 0, 0,
                                      out.ctypes.data, ctypes.byref(res))
        assert rc == _native.GHS_E_NONCANON, mutate


def test_cli_labels_with_clusters(tmp_path, torch_cuda):
    """--labels OUT.npy --clusters 3 end to end, in a fresh process."""
    import shutil

    from distributed_ghs_implementation_amd import read_graph_dir
    d = tmp_path / "graph_data"
    shutil.copytree(os.path.join(GOLDEN, "graph_data_n6"), d)
    out = tmp_path / "labels.npy"
    p = subprocess.run([sys.executable, "-m", "distributed_ghs_implementation_amd", "--graph-dir", str(d),
                        "--labels", str(out), "--clusters", "3"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    g = read_graph_dir(str(d))
    flags = _kruskal(g.n, g.u, g.v, g.w)
    want, winfo = expected(g.n, g.u, g.v, g.w, flags, num_clusters=3)
    got = np.load(out)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    line = f"Clusters: {winfo['num_clusters']} (kept {winfo['kept_edges']} of {winfo['flagged_edges']} forest edges)"
    assert line in p.stdout, p.stdout[-2000:]
    assert winfo["num_clusters"] == 3
