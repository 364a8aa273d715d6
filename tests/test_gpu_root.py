"""GPU: the rooted forest (ghs_forest_root_device, csrc/root.hip) against an iterative DFS.

The expected answer is computed here, on the host: adjacency sorted by neighbour id, every tree
rooted at its smallest vertex, trees numbered in root order, a vertex entered from parent p visiting
its children in ascending id cyclically, starting after p. parent, parent_eid, depth, pre and size are
compared whole, together with flagged_edges, num_trees, max_depth and is_forest; a union-find says
which flag vectors are forests."""
import ctypes
import os
import subprocess
import sys
from bisect import bisect_left

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, fixture_names, load_fixture

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
ARRAYS = ("parent", "parent_eid", "depth", "pre", "size")


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


def _edges(n, u, v):
    from distributed_ghs_implementation_amd.device import DeviceEdges
    return DeviceEdges(n, _t(u), _t(v), _t(np.zeros(len(u), np.uint32)))


def _kruskal(n, u, v, w):
    return _oracle().kruskal_c(n, u, v, w)[0][: len(u)]


def _canon(n, u, v, w=None):
    from distributed_ghs_implementation_amd import canonicalize
    w = np.zeros(len(u), np.int64) if w is None else np.asarray(w)
    return canonicalize(n, u=np.asarray(u), v=np.asarray(v), w=w)


# ---- the expected answer ---------------------------------------------------------------------------
def is_forest(n, u, v, flags):
    par = list(range(n))

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x
    T = np.flatnonzero(np.asarray(flags) != 0)
    for a, b in zip(np.asarray(u)[T].tolist(), np.asarray(v)[T].tolist()):
        ra, rb = find(a), find(b)
        if ra == rb:
            return False
        par[ra] = rb
    return True


def host_rooted(n, u, v, flags):
    """The five arrays (uint32) and {flagged_edges, num_trees, max_depth, is_forest} of a forest."""
    T = np.flatnonzero(np.asarray(flags) != 0)
    tu, tv = np.asarray(u, np.int64)[T], np.asarray(v, np.int64)[T]
    src, dst, eid = np.concatenate([tu, tv]), np.concatenate([tv, tu]), np.concatenate([T, T])
    order = np.lexsort((dst, src))  # every adjacency in ascending neighbour id
    src, dst, eid = src[order], dst[order].tolist(), eid[order].tolist()
    off = np.searchsorted(src, np.arange(n + 1)).tolist()
    parent, peid, depth, pre, size = [NONE] * n, [NONE] * n, [0] * n, [-1] * n, [1] * n
    cnt = trees = 0
    for r in range(n):
        if pre[r] >= 0:
            continue
        trees += 1
        pre[r] = cnt
        cnt += 1
        stack = [[r, off[r], off[r + 1] - off[r]]]  # vertex, next adjacency slot, children left
        while stack:
            top = stack[-1]
            x = top[0]
            if top[2] == 0:
                stack.pop()
                if stack:
                    size[stack[-1][0]] += size[x]
                continue
            if top[1] == off[x + 1]:
                top[1] = off[x]  # cyclically
            y, e = dst[top[1]], eid[top[1]]
            top[1] += 1
            top[2] -= 1
            assert pre[y] < 0, "not a forest"
            parent[y], peid[y], depth[y], pre[y] = x, e, depth[x] + 1, cnt
            cnt += 1
            j = bisect_left(dst, x, off[y], off[y + 1])  # start after the parent
            stack.append([y, j + 1, off[y + 1] - off[y] - 1])
    arrays = {k: np.array(a, dtype=np.uint32) for k, a in zip(ARRAYS, (parent, peid, depth, pre, size))}
    info = {"flagged_edges": len(T), "num_trees": trees, "max_depth": max(depth) if n else 0, "is_forest": True}
    return arrays, info


def round_bound(T):
    """include/ghs_mst.h: rounds <= 2 ceil(log2(2 |T|)) + 2."""
    return 2 * int(np.ceil(np.log2(2 * T))) + 2 if T else 0


def _rooted(edges, flags_t, order=True):
    import torch

    from distributed_ghs_implementation_amd.device import forest_root
    r, info = forest_root(edges, flags_t, order=order)
    out = {}
    for k in ARRAYS:
        t = getattr(r, k)
        if t is None:
            assert not order and k in ("pre", "size")
            continue
        assert t.dtype == torch.int32 and t.is_cuda and t.numel() == edges.n
        out[k] = t.cpu().numpy().view(np.uint32)
    return out, info, r


def check_properties(n, u, v, flags, got):
    """What holds for any correct rooting, with no oracle."""
    par, peid, dep, pre, size = (got[k].astype(np.int64) for k in ARRAYS)
    nonroot = np.flatnonzero(par != NONE)
    e = peid[nonroot]
    assert (np.asarray(flags)[e] != 0).all()
    uu, vv = np.asarray(u, np.int64)[e], np.asarray(v, np.int64)[e]
    assert (((uu == nonroot) & (vv == par[nonroot])) | ((vv == nonroot) & (uu == par[nonroot]))).all()
    assert (dep[nonroot] == dep[par[nonroot]] + 1).all()
    assert np.array_equal(np.sort(pre), np.arange(n))
    assert (pre[par[nonroot]] < pre[nonroot]).all()
    kids = np.zeros(n, np.int64)
    np.add.at(kids, par[nonroot], size[nonroot])
    assert np.array_equal(size, 1 + kids)
    roots = np.flatnonzero(par == NONE)
    assert (peid[roots] == NONE).all() and (dep[roots] == 0).all()


def _check(n, u, v, flags, edges=None, flags_t=None, want=None):
    """Run the device call and compare all five arrays and the result fields with the host's."""
    e = _edges(n, u, v) if edges is None else edges
    ft = _t(np.asarray(flags) != 0, np.uint8) if flags_t is None else flags_t
    got, info, r = _rooted(e, ft)
    warr, winfo = host_rooted(n, u, v, flags) if want is None else want
    for k in ARRAYS:
        assert np.array_equal(got[k], warr[k]), (k, np.flatnonzero(got[k] != warr[k])[:8])
    assert {k: info[k] for k in winfo} == winfo, (info, winfo)
    assert info["rounds"] <= round_bound(winfo["flagged_edges"]), info
    check_properties(n, u, v, flags, got)
    return info, r


def random_forest(n, T, seed, m=None):
    """A canonical list of m >= T edges over n vertices whose flagged edges are a random forest of T
    edges: T of the vertices 1 .. n - 1 (1 and n - 1 among them) hang from a random smaller vertex,
    n - 1 from n - 2, so (0, 1) and (n - 2, n - 1) — the first and the last edge of any canonical list
    over these vertices — are flagged. Returns (u, v, flags)."""
    rng = np.random.default_rng(seed)
    assert 2 <= T <= n - 1 and n >= 3
    kids = np.concatenate([[1, n - 1], 2 + rng.choice(n - 3, size=T - 2, replace=False)]) if T > 2 else np.array([1, n - 1])
    par = (rng.random(len(kids)) * kids).astype(np.int64)
    par[1] = n - 2
    pairs = {(int(a), int(b)) for a, b in zip(par, kids)}
    forest = set(pairs)
    while m is not None and len(pairs) < m:
        a, b = sorted(rng.integers(0, n, 2).tolist())
        if a != b:
            pairs.add((a, b))
    lst = sorted(pairs)
    u = np.array([a for a, _ in lst], np.uint32)
    v = np.array([b for _, b in lst], np.uint32)
    flags = np.array([p in forest for p in lst], np.uint8)
    assert flags[0] and flags[-1] and int(flags.sum()) == T
    return u, v, flags


# ---- exhaustive: every flag vector of a small graph -------------------------------------------------
EX_N = 7  # vertex 6 is isolated
EX_EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (2, 4), (3, 4), (4, 5)]


def test_exhaustive_all_flag_vectors(torch_cuda):
    """All 512 flag vectors of the 9-edge graph as rows of one 9-byte-pitch tensor, so the flag pointer
    takes every alignment. Forests: all five arrays and every result field; cyclic vectors with at most
    6 flags: is_forest False and flagged_edges exact; 7 or more flags: GHS_E_ARG."""
    from distributed_ghs_implementation_amd import _native
    from distributed_ghs_implementation_amd.device import forest_root
    u = np.array([a for a, _ in EX_EDGES], np.uint32)
    v = np.array([b for _, b in EX_EDGES], np.uint32)
    e = _edges(EX_N, u, v)
    allflags = np.array([[(bits >> k) & 1 for k in range(9)] for bits in range(512)], np.uint8)
    dev = _t(allflags.ravel(), np.uint8)
    forests = cyclic = overfull = 0
    for bits in range(512):
        flags, ft = allflags[bits], dev[9 * bits: 9 * bits + 9]
        if int(flags.sum()) >= 7:
            overfull += 1
            with pytest.raises(_native.GHSError) as ei:
                forest_root(e, ft)
            assert ei.value.code == _native.GHS_E_ARG and "more flags" in str(ei.value)
        elif is_forest(EX_N, u, v, flags):
            forests += 1
            _check(EX_N, u, v, flags, edges=e, flags_t=ft)
        else:
            cyclic += 1
            _, info = forest_root(e, ft)
            assert info["is_forest"] is False and info["flagged_edges"] == int(flags.sum()), (bits, info)
    assert overfull == 46 and forests > 0 and cyclic > 0 and forests + cyclic == 466


# ---- every golden fixture ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", fixture_names())
def test_golden_fixtures(name, torch_cuda):
    from distributed_ghs_implementation_amd import canonicalize
    from distributed_ghs_implementation_amd.device import DeviceEdges, forest_labels
    fx = load_fixture(name)
    g = canonicalize(fx["num_nodes"], edges=[tuple(e) for e in fx["edges"]])
    ref = _kruskal(g.n, g.u, g.v, g.w)
    e = DeviceEdges(g.n, _t(g.u), _t(g.v), _t(g.w))
    ft = _t(ref, np.uint8)
    info, r = _check(g.n, g.u, g.v, ref, edges=e, flags_t=ft)
    lab, linfo = forest_labels(e, ft)
    lab = lab.cpu().numpy().view(np.uint32)
    par = r.parent.cpu().numpy().view(np.uint32)
    nonroot = par != NONE
    assert np.array_equal(lab[nonroot], lab[par[nonroot]])
    assert info["num_trees"] == linfo["num_clusters"] and info["is_forest"] is True


# ---- shapes ---------------------------------------------------------------------------------------------
def _bitrev(i, bits):
    r = 0
    for _ in range(bits):
        r, i = (r << 1) | (i & 1), i >> 1
    return r


def _shape(kind):
    """(n, raw u, raw v) of a forest."""
    if kind == "path-id":
        n = 5000
        return n, np.arange(n - 1), np.arange(1, n)
    if kind == "path-bitrev":  # the 5000-path over bit-reversed 13-bit ids; the other ids stay isolated
        p = np.array([_bitrev(i, 13) for i in range(5000)])
        return 8192, p[:-1], p[1:]
    if kind == "path-interleaved":  # ids 0, k, 1, k + 1, ...
        k = 2500
        p = np.empty(5000, np.int64)
        p[0::2], p[1::2] = np.arange(k), k + np.arange(k)
        return 5000, p[:-1], p[1:]
    if kind == "star-0":
        n = 4096
        return n, np.zeros(n - 1, np.int64), np.arange(1, n)
    if kind == "star-last":
        n = 4096
        return n, np.full(n - 1, n - 1), np.arange(n - 1)
    if kind == "caterpillar":  # a 1000-spine (ids 3i) with two legs per spine vertex
        s = 3 * np.arange(1000)
        return 3000, np.concatenate([s[:-1], s, s]), np.concatenate([s[1:], s + 1, s + 2])
    if kind.startswith("heap-"):  # a complete binary tree in heap order
        n = int(kind[5:])
        c = np.arange(1, n)
        return n, (c - 1) // 2, c
    if kind == "broom":  # a path of 3000, then 3000 leaves at its far end
        return 6000, np.concatenate([np.arange(2999), np.full(3000, 2999)]), np.concatenate([np.arange(1, 3000), np.arange(3000, 6000)])
    if kind == "small-tours":  # per block of 6 ids: an edge, an isolated vertex, a 3-vertex path
        b = 6 * np.arange(10000)
        return 60000, np.concatenate([b, b + 3, b + 4]), np.concatenate([b + 1, b + 4, b + 5])
    if kind == "long-path":
        n = (1 << 17) + 1
        return n, np.arange(n - 1), np.arange(1, n)
    if kind == "long-path-permuted":
        n = (1 << 17) + 1
        p = np.random.default_rng(17).permutation(n)
        return n, p[:-1], p[1:]
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["path-id", "path-bitrev", "path-interleaved", "star-0", "star-last", "caterpillar",
                                  "heap-4095", "heap-4096", "heap-4097", "broom", "small-tours", "long-path",
                                  "long-path-permuted"])
def test_shapes(kind, torch_cuda):
    n, ru, rv = _shape(kind)
    g = _canon(n, ru, rv)
    assert g.m == len(ru)
    flags = np.ones(g.m, np.uint8)
    info, r = _check(n, g.u, g.v, flags)
    assert info["is_forest"] is True and 1 <= info["rounds"] <= round_bound(g.m)
    dep = r.depth.cpu().numpy().view(np.uint32)
    if kind == "path-id":
        assert info["max_depth"] == 4999 and np.array_equal(dep, np.arange(5000))
    if kind == "long-path":
        assert info["max_depth"] == 1 << 17
    if kind == "star-last":  # root 0 is a leaf, the centre at depth 1, the rest at depth 2
        assert dep[0] == 0 and dep[n - 1] == 1 and (dep[1: n - 1] == 2).all()
    if kind == "small-tours":
        assert info["num_trees"] == 30000 and info["max_depth"] == 2


# ---- sizes at which a kernel takes another path ----------------------------------------------------
@pytest.mark.parametrize("T", [31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 32767, 32768,
                               32769])
def test_tile_boundaries_of_the_arc_and_edge_passes(T, torch_cuda):
    """Per block: 4096 flag bytes (the flag pass), 1024 items of a scan (over the 2|T| arcs' marks, the
    n vertices and the splitter words), 256 items of the other passes (tree edges, arcs, splitters,
    vertices); a splitter word covers 64 arcs and a scan block 1024 words = 65536 arcs. |T| at one below,
    at and one above 32 (64 arcs), 128 and 256 (256 arcs / edges), 512 (1024 arcs), 1024 and 32768
    (65536 arcs); every edge of the list is flagged, n = |T| + 1 and |T| + 40."""
    for n in (T + 1, T + 40):
        u, v, flags = random_forest(n, T, seed=T)
        _check(n, u, v, flags)


@pytest.mark.parametrize("n", [255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097])
def test_tile_boundaries_of_the_vertex_passes(n, torch_cuda):
    """n at the 256-vertex block and the 1024-vertex scan tile (and at 4096), with a third of the
    vertices isolated."""
    u, v, flags = random_forest(n, (2 * n) // 3, seed=n)
    _check(n, u, v, flags)


@pytest.mark.parametrize("m,T", [(4095, 1023), (4096, 1024), (4097, 1025), (4081, 2047), (4097, 2048), (8193, 2049),
                                 (4080, 255), (4112, 257)])
def test_tile_boundaries_of_the_flag_pass(m, T, torch_cuda):
    """m flag bytes around the 4096-byte block of the flag pass, |T| of them set; the first and the last
    edge of the list are among the flagged."""
    u, v, flags = random_forest(3000, T, seed=m, m=m)
    assert len(u) == m
    _check(3000, u, v, flags)


def test_unaligned_flags(torch_cuda):
    """The flags may start at any byte (a slice): scalar head and tail around the 16-byte body."""
    import torch
    m, n = 4099, 3000
    u, v, flags = random_forest(n, 1500, seed=5, m=m)
    e = _edges(n, u, v)
    want = host_rooted(n, u, v, flags)
    for off in (1, 2, 3, 7, 8, 15, 17):
        buf = _t(np.concatenate([np.ones(off, np.uint8), flags, np.ones(21, np.uint8)]), np.uint8)
        view = buf[off: off + m]
        assert view.data_ptr() % 16 == off % 16
        _check(n, u, v, flags, edges=e, flags_t=view, want=want)
    ft = _t(flags, np.uint8)
    _check(n, u, v, flags, edges=e, flags_t=ft.to(torch.bool), want=want)
    _check(n, u, v, flags, edges=e, flags_t=torch.cat([ft, torch.ones(7, dtype=torch.uint8, device=ft.device)]), want=want)


def test_order_false_and_determinism(torch_cuda):
    n = 5000
    u, v, flags = random_forest(n, 4000, seed=8, m=9000)
    e, ft = _edges(n, u, v), _t(flags, np.uint8)
    a, ia, _ = _rooted(e, ft)
    b, ib, _ = _rooted(e, ft)
    for k in ARRAYS:
        assert a[k].tobytes() == b[k].tobytes(), k  # two calls: identical bytes
    assert {k: ia[k] for k in ia if k != "ms_total"} == {k: ib[k] for k in ib if k != "ms_total"}
    c, ic, r = _rooted(e, ft, order=False)
    assert r.pre is None and r.size is None and set(c) == {"parent", "parent_eid", "depth"}
    for k in c:
        assert np.array_equal(c[k], a[k]), k
    assert (ic["num_trees"], ic["max_depth"], ic["is_forest"]) == (ia["num_trees"], ia["max_depth"], True)
    with pytest.raises(ValueError):
        r.is_ancestor(0, 1)


def test_degenerate_cases(torch_cuda):
    z = np.zeros(0, np.uint32)
    for n in (1, 5):  # no edges: every vertex is a root
        info, r = _check(n, z, z, np.zeros(0, np.uint8))
        assert (info["num_trees"], info["rounds"], info["max_depth"], info["is_forest"]) == (n, 0, 0, True)
        assert np.array_equal(r.pre.cpu().numpy().view(np.uint32), np.arange(n))
        assert (r.parent.cpu().numpy().view(np.uint32) == NONE).all()
    assert _check(2, [0], [1], [1])[0]["num_trees"] == 1
    assert _check(2, [0], [1], [0])[0]["num_trees"] == 2
    info, r = _check(1000, [3], [700], [1])  # one edge among isolated vertices
    assert (info["num_trees"], info["max_depth"]) == (999, 1)
    assert int(r.parent[700]) == 3 and int(r.pre[700]) == 4 and int(r.pre[4]) == 5
    u, v, flags = random_forest(200, 150, seed=21, m=900)
    info, _ = _check(200, u, v, np.zeros(900, np.uint8))  # all-zero flags
    assert (info["num_trees"], info["rounds"], info["flagged_edges"]) == (200, 0, 0)


def test_noncanonical_list_rejected(torch_cuda):
    from distributed_ghs_implementation_amd import _native
    from distributed_ghs_implementation_amd.device import forest_root
    n = 50
    u, v, flags = random_forest(n, 30, seed=3, m=200)
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
            forest_root(_edges(n, bu, bv), _t(flags, np.uint8))
        assert ei.value.code == _native.GHS_E_NONCANON, mutate
        out = [np.zeros(n, np.uint32) for _ in range(5)]
        res = _native.RootResult()
        rc = L.ghs_forest_root_host(n, len(bu), bu.ctypes.data, bv.ctypes.data, flags.ctypes.data,
                                    *[o.ctypes.data for o in out], ctypes.byref(res))
        assert rc == _native.GHS_E_NONCANON, mutate


# ---- the engine's own output --------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["rmat12", "rmat14", "grid64-0", "grid64-1"])
def test_engine_output_rooted(graph, torch_cuda):
    import torch

    from distributed_ghs_implementation_amd.device import DeviceMST, generate_grid, generate_rmat
    e = {"rmat12": lambda: generate_rmat(12), "rmat14": lambda: generate_rmat(14),
         "grid64-0": lambda: generate_grid(64, 0), "grid64-1": lambda: generate_grid(64, 1)}[graph]()
    eng = DeviceMST(e)
    res, _ = eng.run()
    before = eng.in_mst.clone()
    r, info = eng.rooted()
    g = e.to_host()
    flags = eng.in_mst_host()
    want, winfo = host_rooted(g.n, g.u, g.v, flags)
    got = {k: getattr(r, k).cpu().numpy().view(np.uint32) for k in ARRAYS}
    for k in ARRAYS:
        assert np.array_equal(got[k], want[k]), k
    assert {k: info[k] for k in winfo} == winfo
    assert info["num_trees"] == g.n - res.num_mst_edges and info["rounds"] <= round_bound(res.num_mst_edges)
    check_properties(g.n, g.u, g.v, flags, got)
    assert bool((eng.in_mst == before).all())  # the flags are only read
    # is_ancestor against walks up the parent pointers
    rng = np.random.default_rng(4)
    b = rng.integers(0, g.n, 64)
    a = b.copy()
    for i in range(64):  # an ancestor some steps up, or an unrelated vertex
        for _ in range(int(rng.integers(0, 6))):
            if want["parent"][a[i]] != NONE:
                a[i] = want["parent"][a[i]]
    assert bool(r.is_ancestor(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()).all())
    c = rng.integers(0, g.n, 64)
    expect = []
    for x, y in zip(c, b):
        while y != x and want["parent"][y] != NONE:
            y = want["parent"][y]
        expect.append(bool(x == y))
    assert r.is_ancestor(torch.from_numpy(c).cuda(), torch.from_numpy(b).cuda()).cpu().tolist() == expect


def test_engine_csr_and_emulated_ranks(torch_cuda):
    from distributed_ghs_implementation_amd.device import DeviceMST, emulated_mst, forest_root, generate_rmat
    e = generate_rmat(12).with_csr()
    eng = DeviceMST(e)
    assert eng.csr
    eng.run()
    g = e.to_host()
    want = host_rooted(g.n, g.u, g.v, eng.in_mst_host())
    _check(g.n, g.u, g.v, eng.in_mst_host(), edges=e, flags_t=eng.in_mst, want=want)  # CSR engine's flags, COO list
    _, _, in3 = emulated_mst(e, 3)
    _check(g.n, g.u, g.v, eng.in_mst_host(), edges=e, flags_t=in3, want=want)
    with pytest.raises(ValueError, match="CSR"):
        forest_root(e.csr_only(), eng.in_mst)


# ---- the host path ---------------------------------------------------------------------------------
def test_host_path_mstresult_rooted(torch_cuda):
    from distributed_ghs_implementation_amd import canonicalize, minimum_spanning_forest
    fx = load_fixture("cgf_n1000_p001.json")
    g = canonicalize(fx["num_nodes"], edges=[tuple(e) for e in fx["edges"]])
    r = minimum_spanning_forest(g)
    got, info = r.rooted(return_info=True)
    want, winfo = host_rooted(g.n, g.u, g.v, r.in_mst)
    for k in ARRAYS:
        assert got[k].dtype == np.uint32 and np.array_equal(got[k], want[k]), k
    assert {k: info[k] for k in winfo} == winfo
    rng = np.random.default_rng(3)  # float weights, rank-mapped by canonicalize
    raw = [(int(a), int(b), float(c)) for a, b, c in zip(rng.integers(0, 150, 700), rng.integers(0, 150, 700),
                                                         rng.integers(-4, 5, 700) * 0.5)]
    gf = canonicalize(150, edges=raw)
    assert gf.weights is not None
    rf = minimum_spanning_forest(gf)
    got = rf.rooted()
    want, _ = host_rooted(gf.n, gf.u, gf.v, rf.in_mst)
    for k in ARRAYS:
        assert np.array_equal(got[k], want[k]), k


def test_cli_rooted(tmp_path, torch_cuda):
    """--rooted OUT.npz end to end, in a fresh process."""
    import shutil

    from distributed_ghs_implementation_amd import read_graph_dir
    d = tmp_path / "graph_data"
    shutil.copytree(os.path.join(GOLDEN, "graph_data_n6"), d)
    out = tmp_path / "rooted.npz"
    p = subprocess.run([sys.executable, "-m", "distributed_ghs_implementation_amd", "--graph-dir", str(d),
                        "--rooted", str(out)], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    g = read_graph_dir(str(d))
    flags = _kruskal(g.n, g.u, g.v, g.w)
    want, winfo = host_rooted(g.n, g.u, g.v, flags)
    got = np.load(out)
    assert sorted(got.files) == sorted(ARRAYS)
    for k in ARRAYS:
        assert got[k].dtype == np.uint32 and np.array_equal(got[k], want[k]), k
    assert f"Rooted forest: {winfo['num_trees']} trees, max depth {winfo['max_depth']}" in p.stdout, p.stdout[-2000:]
