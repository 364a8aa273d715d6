"""GPU: path queries on the rooted forest (ghs_forest_paths_*, csrc/paths.hip) against a plain walk.

The expected answer is computed here, on the host: every tree rooted at its smallest vertex by a
breadth-first pass, then for a pair (a, b) a walk up the parent pointers, the deeper end first, that
collects the largest key w << 32 | eid, the meeting vertex and the number of steps. a == b and pairs in
different trees have no edge: key = UINT64_MAX."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_fixture

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
NOKEY = (1 << 64) - 1
QPL_TILE = 4 * 256  # queries per lane x block size of k_pa_query


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from distributed_ghs_implementation_amd import _native
    assert _native.device_count() > 0
    return torch


def _t(a, dtype=np.uint32):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.view("int32").copy() if dtype == np.uint32 else a.copy()).cuda()


def _edges(n, u, v, w):
    from distributed_ghs_implementation_amd.device import DeviceEdges
    return DeviceEdges(n, _t(u), _t(v), _t(w))


def canonical(n, pairs, w):
    """Undirected pairs + weights -> canonical arrays (u < v, sorted by (u, v)); pairs are distinct."""
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    lo, hi = p.min(axis=1), p.max(axis=1)
    order = np.lexsort((hi, lo))
    return lo[order].astype(np.uint32), hi[order].astype(np.uint32), np.asarray(w, np.uint32)[order]


# ---- the expected answer ---------------------------------------------------------------------------
def is_forest(n, u, v, flags):
    par = list(range(n))

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x
    for e in np.flatnonzero(np.asarray(flags) != 0).tolist():
        ra, rb = find(int(u[e])), find(int(v[e]))
        if ra == rb:
            return False
        par[ra] = rb
    return True


def host_rooted(n, u, v, flags):
    """parent, parent_eid, depth (python lists) of a forest, every tree rooted at its smallest vertex."""
    adj = [[] for _ in range(n)]
    for e in np.flatnonzero(np.asarray(flags) != 0).tolist():
        a, b = int(u[e]), int(v[e])
        adj[a].append((b, e))
        adj[b].append((a, e))
    parent, peid, depth, seen = [NONE] * n, [NONE] * n, [0] * n, [False] * n
    trees = 0
    for r in range(n):
        if seen[r]:
            continue
        trees += 1
        seen[r] = True
        frontier = [r]
        while frontier:
            nxt = []
            for x in frontier:
                for y, e in adj[x]:
                    if not seen[y]:
                        seen[y] = True
                        parent[y], peid[y], depth[y] = x, e, depth[x] + 1
                        nxt.append(y)
            frontier = nxt
    return parent, peid, depth, trees


def walk(a, b, parent, peid, depth, w):
    """(key, lca, hops) of one pair by walking up the parent pointers."""
    if a == b:
        return NOKEY, a, 0
    key, hops, x, y = -1, 0, a, b
    while depth[x] > depth[y]:
        key, x, hops = max(key, (int(w[peid[x]]) << 32) | peid[x]), parent[x], hops + 1
    while depth[y] > depth[x]:
        key, y, hops = max(key, (int(w[peid[y]]) << 32) | peid[y]), parent[y], hops + 1
    while x != y:
        if parent[x] == NONE:  # two roots
            return NOKEY, NONE, NONE
        key = max(key, (int(w[peid[x]]) << 32) | peid[x], (int(w[peid[y]]) << 32) | peid[y])
        x, y, hops = parent[x], parent[y], hops + 2
    return key, x, hops


def expected(rooting, w, a, b):
    parent, peid, depth, _ = rooting
    out = [walk(int(x), int(y), parent, peid, depth, w) for x, y in zip(a, b)]
    return (np.array([o[0] for o in out], np.uint64), np.array([o[1] for o in out], np.uint32),
            np.array([o[2] for o in out], np.uint32))


def _ask(index, a, b, **kw):
    ans = index.query(_t(a), _t(b), **kw)
    return ans, tuple(None if t is None else t.cpu().numpy().view(d) for t, d in
                      ((ans.key, np.uint64), (ans.lca, np.uint32), (ans.hops, np.uint32)))


def _check_pairs(index, rooting, w, a, b):
    ans, (key, lca, hops) = _ask(index, a, b)
    wkey, wlca, whops = expected(rooting, w, a, b)
    assert np.array_equal(key, wkey), np.flatnonzero(key != wkey)[:8]
    assert np.array_equal(lca, wlca), np.flatnonzero(lca != wlca)[:8]
    assert np.array_equal(hops, whops), np.flatnonzero(hops != whops)[:8]
    assert ans.info["queries"] == len(a) and ans.info["connected"] == int((wlca != NONE).sum())
    assert ans.connected.cpu().numpy().tolist() == (wlca != NONE).tolist()
    assert ans.has_edge.cpu().numpy().tolist() == (wkey != NOKEY).tolist()
    assert np.array_equal(ans.eid.cpu().numpy().view(np.uint32), (wkey & 0xFFFFFFFF).astype(np.uint32))
    assert np.array_equal(ans.w.cpu().numpy().view(np.uint32), (wkey >> 32).astype(np.uint32))
    return ans


def _tree_case(n, u, v, w, flags=None, seed=0, extra=()):
    """Index a flagged forest (default: every edge) and check random pairs + `extra` against the walk."""
    from distributed_ghs_implementation_amd.device import forest_paths
    flags = np.ones(len(u), np.uint8) if flags is None else flags
    e = _edges(n, u, v, w)
    index, info = forest_paths(e, _t(flags, np.uint8))
    rooting = host_rooted(n, u, v, flags)
    maxd = max(rooting[2]) if n else 0
    assert info["levels"] == max(1, int(maxd).bit_length()) and info["max_depth"] == maxd
    assert info["num_trees"] == rooting[3]
    rng = np.random.default_rng(seed)
    a = np.concatenate([rng.integers(0, n, 300), [p[0] for p in extra]]).astype(np.int64)
    b = np.concatenate([rng.integers(0, n, 300), [p[1] for p in extra]]).astype(np.int64)
    _check_pairs(index, rooting, w, a, b)
    return index, info, rooting


# ---- exhaustive: every forest of a small graph, every ordered pair ---------------------------------
EX_N = 7  # vertex 6 is isolated
EX_EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (2, 4), (3, 4), (4, 5)]
EX_W = [0, 3, 3, 1, 0, 3, 1, 2, 0]  # ties, and w = 0 on edge 0: its key is 0


def test_exhaustive_all_forests_all_pairs(torch_cuda):
    from distributed_ghs_implementation_amd import _native
    from distributed_ghs_implementation_amd.device import forest_paths
    u = np.array([a for a, _ in EX_EDGES], np.uint32)
    v = np.array([b for _, b in EX_EDGES], np.uint32)
    w = np.array(EX_W, np.uint32)
    e = _edges(EX_N, u, v, w)
    a, b = (np.array(x) for x in zip(*itertools.product(range(EX_N), repeat=2)))
    forests = cyclic = 0
    for bits in range(1 << len(EX_EDGES)):
        flags = np.array([(bits >> k) & 1 for k in range(len(EX_EDGES))], np.uint8)
        if not is_forest(EX_N, u, v, flags):
            cyclic += 1
            if cyclic % 16 == 1:  # a sample of the cyclic vectors: they raise
                with pytest.raises((ValueError, _native.GHSError)):
                    forest_paths(e, _t(flags, np.uint8))
            continue
        forests += 1
        index, info = forest_paths(e, _t(flags, np.uint8))
        rooting = host_rooted(EX_N, u, v, flags)
        assert info["num_trees"] == EX_N - int(flags.sum())
        _check_pairs(index, rooting, w, a, b)
        index.close()
    assert forests > 100 and cyclic > 100
    # the key-0 edge as the only edge of a path: key 0 is an answer, not "no edge"
    flags = np.zeros(len(EX_EDGES), np.uint8)
    flags[0] = 1
    index, _ = forest_paths(e, _t(flags, np.uint8))
    _, (key, lca, hops) = _ask(index, [0, 1, 0, 1, 0], [1, 0, 0, 1, 2])
    assert key.tolist() == [0, 0, NOKEY, NOKEY, NOKEY]
    assert lca.tolist() == [0, 0, 0, 1, NONE] and hops.tolist() == [1, 1, 0, 0, NONE]


def test_ties_all_weights_equal(torch_cuda):
    """All weights equal: the bottleneck is the largest eid on the path."""
    rng = np.random.default_rng(11)
    n = 3000
    kids = np.arange(1, n)
    par = (rng.random(n - 1) * kids).astype(np.int64)
    u, v, w = canonical(n, np.stack([par, kids], 1), np.full(n - 1, 7))
    index, _, rooting = _tree_case(n, u, v, w, seed=12)
    a, b = rng.integers(0, n, 200), rng.integers(0, n, 200)
    _, (key, _, _) = _ask(index, a, b)
    parent, peid, _, _ = rooting
    for x, y, k in zip(a.tolist(), b.tolist(), key.tolist()):
        if x == y:
            continue
        up = lambda z: [z] + (up(parent[z]) if parent[z] != NONE else [])  # noqa: E731
        px, py = up(x), up(y)
        common = set(px) & set(py)
        on_path = [peid[z] for z in px + py if z not in common]
        assert k == (7 << 32) | max(on_path)


# ---- depth boundaries: K changes between neighbours ---------------------------------------------------
@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("max_depth", [1, 2, 3, 4, 7, 8, 9, 255, 256, 257, 65535, 65536, 65537])
def test_depth_boundaries_on_paths(max_depth, permuted, torch_cuda):
    n = max_depth + 1
    rng = np.random.default_rng(max_depth * 2 + permuted)
    ids = np.arange(n)
    if permuted:
        ids = np.concatenate([[0], 1 + rng.permutation(n - 1)])  # vertex 0 stays the root end
    w = rng.integers(0, 1 << 32, n - 1, dtype=np.uint64)
    u, v, w = canonical(n, np.stack([ids[:-1], ids[1:]], 1), w)
    extra = [(int(ids[0]), int(ids[-1])), (int(ids[-1]), int(ids[0]))]  # both ends of the path
    for k in range(0, max(1, int(max_depth).bit_length()) + 1):
        for d in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            if d <= max_depth:
                lo = int(rng.integers(0, max_depth - d + 1))
                extra += [(int(ids[lo]), int(ids[lo + d])), (int(ids[lo + d]), int(ids[lo]))]
    from distributed_ghs_implementation_amd.device import forest_paths
    flags = np.ones(n - 1, np.uint8)
    index, info = forest_paths(_edges(n, u, v, w), _t(flags, np.uint8))
    assert info["levels"] == max(1, int(max_depth).bit_length()) and info["max_depth"] == max_depth
    assert info["num_trees"] == 1 and info["index_bytes"] >= 16 * info["levels"] * n
    # on a path the walk is a slice: depth = position along ids
    pos = np.empty(n, np.int64)
    pos[ids] = np.arange(n)
    eid_of = {}
    for e_, (x, y) in enumerate(zip(u.tolist(), v.tolist())):
        eid_of[min(pos[x], pos[y])] = e_
    step_key = np.array([(int(w[eid_of[i]]) << 32) | eid_of[i] for i in range(n - 1)], np.uint64)
    a = np.array([p[0] for p in extra])
    b = np.array([p[1] for p in extra])
    _, (key, lca, hops) = _ask(index, a, b)
    for x, y, k, l, h in zip(a.tolist(), b.tolist(), key.tolist(), lca.tolist(), hops.tolist()):
        lo, hi = sorted((int(pos[x]), int(pos[y])))
        assert h == hi - lo and l == int(ids[lo])
        assert k == (NOKEY if lo == hi else int(step_key[lo:hi].max())), (x, y)


# ---- shapes -----------------------------------------------------------------------------------------
def _shape(kind, rng):
    if kind == "star-0":
        n = 5000
        pairs = [(0, i) for i in range(1, n)]
    elif kind == "star-last":
        n = 5000
        pairs = [(i, n - 1) for i in range(n - 1)]
    elif kind == "caterpillar":
        spine = 2000
        n = 3 * spine
        pairs = [(i, i + 1) for i in range(spine - 1)] + [(i, spine + 2 * i + k) for i in range(spine) for k in (0, 1)]
    elif kind.startswith("heap-"):
        n = int(kind[5:])
        pairs = [((i - 1) // 2, i) for i in range(1, n)]
    elif kind == "broom":
        handle, n = 3000, 6000
        pairs = [(i, i + 1) for i in range(handle)] + [(handle, i) for i in range(handle + 1, n)]
    elif kind == "small-tours":
        trees = 30000
        n = 3 * trees
        perm = rng.permutation(n)
        pairs = [(perm[3 * t], perm[3 * t + 1]) for t in range(trees)] + [(perm[3 * t + 1], perm[3 * t + 2]) for t in range(trees)]
    else:
        raise KeyError(kind)
    w = rng.integers(0, 16, len(pairs))  # repeated weights
    return (n,) + canonical(n, pairs, w)


@pytest.mark.parametrize("kind", ["star-0", "star-last", "caterpillar", "heap-4095", "heap-4096", "heap-4097", "broom",
                                  "small-tours"])
def test_shapes(kind, torch_cuda):
    rng = np.random.default_rng(len(kind))
    n, u, v, w = _shape(kind, rng)
    extra = [(0, n - 1), (n - 1, 0), (0, 0), (n - 1, n - 1)]
    # pairs within one block of 1024 queries and across blocks, neighbours in id
    extra += [(i, i + 1) for i in range(0, n - 1, max(1, n // 600))]
    if kind == "small-tours":  # pairs inside one tree: the ends of tree edges and of two-edge paths
        extra += [(int(u[e]), int(v[e])) for e in range(0, len(u), 97)]
    index, info, rooting = _tree_case(n, u, v, w, seed=5, extra=extra)
    if kind == "small-tours":
        assert info["num_trees"] == 30000 and info["levels"] <= 2


# ---- query tiling, slices, NULL outputs -------------------------------------------------------------
@pytest.fixture(scope="module")
def heap_index(torch_cuda):
    from distributed_ghs_implementation_amd.device import forest_paths
    rng = np.random.default_rng(77)
    n = 4097
    u, v, w = canonical(n, [((i - 1) // 2, i) for i in range(1, n)], rng.integers(0, 50, n - 1))
    flags = np.ones(n - 1, np.uint8)
    edges = _edges(n, u, v, w)
    index, _ = forest_paths(edges, _t(flags, np.uint8))
    rooting = host_rooted(n, u, v, flags)
    a, b = rng.integers(0, n, QPL_TILE + 2), rng.integers(0, n, QPL_TILE + 2)
    a[:3], b[:3] = [0, n - 1, 5], [n - 1, n - 1, 2]
    return index, rooting, w, a, b, expected(rooting, w, a, b)


@pytest.mark.parametrize("Q", [1, 255, 256, 257, QPL_TILE - 1, QPL_TILE, QPL_TILE + 1])
def test_query_tiling(Q, heap_index):
    index, rooting, w, a, b, (wkey, wlca, whops) = heap_index
    _, (key, lca, hops) = _ask(index, a[:Q], b[:Q])
    assert np.array_equal(key, wkey[:Q]) and np.array_equal(lca, wlca[:Q]) and np.array_equal(hops, whops[:Q])


def test_sliced_arrays_and_null_outputs(heap_index):
    import torch

    from distributed_ghs_implementation_amd import _native
    index, rooting, w, a, b, (wkey, wlca, whops) = heap_index
    Q = 300
    # each output left out in turn
    for drop in ("key", "lca", "hops"):
        ans, got = _ask(index, a[:Q], b[:Q], **{drop: False})
        for name, g_, want in zip(("key", "lca", "hops"), got, (wkey, wlca, whops)):
            if name == drop:
                assert g_ is None and getattr(ans, name) is None
            else:
                assert np.array_equal(g_, want[:Q]), (drop, name)
    # a / b / lca / hops as slices at a 4-byte offset (key needs 8 bytes: offset 8)
    L = _native.load()
    ta, tb = _t(np.concatenate([[NONE], a[:Q]])), _t(np.concatenate([[NONE], b[:Q]]))
    olca = torch.full((Q + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ohops = torch.full((Q + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    okey = torch.full((Q + 2,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    sa, sb, sl, sh, sk = ta[1:], tb[1:], olca[1:Q + 1], ohops[1:Q + 1], okey[1:Q + 1]
    assert sa.data_ptr() % 8 == 4 and sl.data_ptr() % 8 == 4 and sk.data_ptr() % 16 == 8
    res = _native.PathsQueryResult()
    vp = ctypes.c_void_p
    _native.check(L.ghs_forest_paths_query(index._h, Q, vp(sa.data_ptr()), vp(sb.data_ptr()), vp(sk.data_ptr()),
                                           vp(sl.data_ptr()), vp(sh.data_ptr()),
                                           vp(torch.cuda.current_stream().cuda_stream), ctypes.byref(res)))
    assert np.array_equal(sk.cpu().numpy().view(np.uint64), wkey[:Q])
    assert np.array_equal(sl.cpu().numpy().view(np.uint32), wlca[:Q])
    assert np.array_equal(sh.cpu().numpy().view(np.uint32), whops[:Q])
    for t in (olca, ohops, okey):  # nothing written outside the slices
        assert int(t[0]) == 0x5A5A5A5A and int(t[Q + 1]) == 0x5A5A5A5A
    assert res.queries == Q and res.connected == Q
    # ints instead of tensors
    one = index.query(0, 4096)
    assert int(one.lca[0]) == 0 and int(one.hops[0]) == int(whops[0])


# ---- the engine's own output: the cycle property, no oracle -----------------------------------------
@pytest.mark.parametrize("graph", ["rmat12", "rmat14", "grid64-0", "grid64-1"])
def test_engine_output_cycle_property(graph, torch_cuda):
    from distributed_ghs_implementation_amd.device import DeviceMST, generate_grid, generate_rmat
    e = {"rmat12": lambda: generate_rmat(12), "rmat14": lambda: generate_rmat(14),
         "grid64-0": lambda: generate_grid(64, 0), "grid64-1": lambda: generate_grid(64, 1)}[graph]()
    eng = DeviceMST(e)
    eng.run()
    before = eng.in_mst.clone()
    assert eng.verify()["unspanned_edges"] == 0
    index, info = eng.paths()
    ans = index.query(e.u, e.v)  # all m edges of the graph as pairs
    assert bool((eng.in_mst == before).all())  # the flags are only read
    g = e.to_host()
    flags = eng.in_mst_host()
    key = ans.key.cpu().numpy().view(np.uint64)
    lca = ans.lca.cpu().numpy().view(np.uint32)
    hops = ans.hops.cpu().numpy().view(np.uint32)
    own = (g.w.astype(np.uint64) << np.uint64(32)) | np.arange(g.m, dtype=np.uint64)
    assert np.array_equal(key[flags], own[flags])            # a tree edge is its own path
    assert ((lca[flags] == g.u[flags]) | (lca[flags] == g.v[flags])).all() and (hops[flags] == 1).all()
    assert (key[~flags] < own[~flags]).all()                 # a non-tree edge closes a cycle of smaller keys
    assert (lca != NONE).all() and ans.info["connected"] == g.m  # no edge joins two trees of the MSF
    assert (hops[~flags] >= 2).all()
    rooting = host_rooted(g.n, g.u, g.v, flags)
    assert info["num_trees"] == rooting[3] and info["max_depth"] == max(rooting[2])
    rng = np.random.default_rng(8)
    _check_pairs(index, rooting, g.w, rng.integers(0, g.n, 2000), rng.integers(0, g.n, 2000))


# ---- minimax ------------------------------------------------------------------------------------------
def test_minimax_distance_of_the_graph(torch_cuda):
    """The bottleneck weight on the MSF equals the min over all paths of the largest edge weight."""
    from distributed_ghs_implementation_amd.device import DeviceMST
    rng = np.random.default_rng(21)
    n = 48
    pairs = {(i, i + 1) for i in range(n - 1)}  # connected
    while len(pairs) < 200:
        x, y = sorted(rng.integers(0, n, 2).tolist())
        if x != y:
            pairs.add((x, y))
    pairs = sorted(pairs)
    u, v, w = canonical(n, pairs, rng.integers(1, 12, len(pairs)))  # repeated weights
    INF = 1 << 40
    D = np.full((n, n), INF, np.int64)
    D[u, v] = D[v, u] = w
    np.fill_diagonal(D, 0)
    for k in range(n):  # the minimax closure
        D = np.minimum(D, np.maximum(D[:, k:k + 1], D[k:k + 1, :]))
    e = _edges(n, u, v, w)
    eng = DeviceMST(e)
    eng.run()
    index, _ = eng.paths()
    a, b = (np.array(x) for x in zip(*itertools.product(range(n), repeat=2)))
    ans = index.query(_t(a), _t(b))
    vals, has = ans.weights(e)
    vals, has = vals.cpu().numpy(), has.cpu().numpy()
    assert has.tolist() == (a != b).tolist()
    assert np.array_equal(vals[has], D[a, b][has])


# ---- rejections: untrusted arrays, and the process stays healthy ------------------------------------
def test_rejections_leave_the_process_healthy(torch_cuda):
    import torch

    from distributed_ghs_implementation_amd import _native
    from distributed_ghs_implementation_amd.device import RootedForest, forest_paths, forest_root
    n = 12
    u, v, w = canonical(n, [(i, i + 1) for i in range(n - 1)], np.arange(n - 1) + 5)  # a path, depth 11
    e = _edges(n, u, v, w)
    flags = _t(np.ones(n - 1), np.uint8)
    good, rinfo = forest_root(e, flags, order=False)
    assert rinfo["max_depth"] == n - 1
    rooting = host_rooted(n, u, v, np.ones(n - 1))

    def healthy():
        index, info = forest_paths(e, rooted=good, max_depth=n - 1)
        assert info["levels"] == 4 and info["num_trees"] == 1
        _check_pairs(index, rooting, w, np.arange(n), np.arange(n)[::-1].copy())
        return index

    def tampered(**changes):
        arrs = {k: getattr(good, k).clone() for k in ("parent", "parent_eid", "depth")}
        for k, (pos, val) in changes.items():
            arrs[k][pos] = val
        return RootedForest(arrs["parent"], arrs["parent_eid"], arrs["depth"], None, None)

    healthy()
    cases = {
        "parent out of range": (tampered(parent=(5, n)), n - 1),
        "parent far out of range": (tampered(parent=(5, -2)), n - 1),
        "parent_eid out of range": (tampered(parent_eid=(5, n - 1)), n - 1),
        "parent_eid joins other vertices": (tampered(parent_eid=(5, 0)), n - 1),
        "root with a depth": (tampered(depth=(0, 1)), n - 1),
        "depth off": (tampered(depth=(5, 7)), n - 1),
        "depth above max_depth": (good, n - 2),
    }
    # a 2-cycle whose depths look consistent from one side: 3 -> 4 -> 3, depth[4] = depth[3] + 1
    cyc = tampered(parent=(3, 4), parent_eid=(3, 3))
    cases["2-cycle"] = (cyc, n - 1)
    for name, (rooted, md) in cases.items():
        with pytest.raises(_native.GHSError) as ei:
            forest_paths(e, rooted=rooted, max_depth=md)
        assert ei.value.code == _native.GHS_E_ARG and "not a rooted forest" in str(ei.value), name
        healthy()
    # m == 0: every vertex must be a root
    e0 = _edges(4, [], [], [])
    roots = _t(np.full(4, NONE))
    zero = _t(np.zeros(4))
    index, info = forest_paths(e0, rooted=RootedForest(roots, roots, zero, None, None), max_depth=0)
    assert info["num_trees"] == 4 and info["levels"] == 1
    _, (key, lca, hops) = _ask(index, [0, 1, 2], [0, 2, 2])
    assert key.tolist() == [NOKEY] * 3 and lca.tolist() == [0, NONE, 2] and hops.tolist() == [0, NONE, 0]
    with pytest.raises(_native.GHSError):
        forest_paths(e0, rooted=RootedForest(_t([NONE, 0, NONE, NONE]), _t([NONE, 0, NONE, NONE]), _t([0, 1, 0, 0]),
                                             None, None), max_depth=1)
    # a query id >= n
    index = healthy()
    for a, b in (([0, n], [1, 1]), ([0, 1], [1, NONE]), ([n + 5], [n + 5])):
        with pytest.raises(_native.GHSError) as ei:
            index.query(torch.tensor(a, dtype=torch.int64, device="cuda"), torch.tensor(b, dtype=torch.int64, device="cuda"))
        assert ei.value.code == _native.GHS_E_ARG and "out of range" in str(ei.value)
        _check_pairs(index, rooting, w, np.arange(n), np.arange(n)[::-1].copy())
    with pytest.raises(ValueError):
        index.query(torch.tensor([-1], device="cuda"), torch.tensor([0], device="cuda"))
    # cyclic flags through the flag form
    tri_u, tri_v, tri_w = canonical(4, [(0, 1), (0, 2), (1, 2)], [1, 2, 3])  # n - 1 flags, one cycle
    with pytest.raises(ValueError, match="forest"):
        forest_paths(_edges(4, tri_u, tri_v, tri_w), _t(np.ones(3), np.uint8))
    index.close()
    with pytest.raises(ValueError, match="closed"):
        index.query(0, 1)


# ---- other ---------------------------------------------------------------------------------------------
def test_determinism_and_index_reuse(torch_cuda):
    from distributed_ghs_implementation_amd.device import DeviceMST, generate_rmat
    e = generate_rmat(12)
    eng = DeviceMST(e)
    eng.run()
    rng = np.random.default_rng(2)
    a, b = _t(rng.integers(0, e.n, 5000)), _t(rng.integers(0, e.n, 5000))
    i1, info1 = eng.paths()
    i2, info2 = eng.paths()
    assert {k: info1[k] for k in info1 if k != "ms_total"} == {k: info2[k] for k in info2 if k != "ms_total"}
    nb = 16 * info1["levels"] * e.n
    assert bool((i1._index[:nb] == i2._index[:nb]).all())  # the levels, byte for byte
    r1, r2, r3 = i1.query(a, b), i2.query(a, b), i1.query(a, b)
    for x in (r2, r3):
        assert bool((r1.key == x.key).all()) and bool((r1.lca == x.lca).all()) and bool((r1.hops == x.hops).all())


def test_rank_mapped_float_weights_in_the_callers_units(torch_cuda):
    from distributed_ghs_implementation_amd.device import DeviceEdges, DeviceMST
    rng = np.random.default_rng(31)
    n, m = 400, 3000
    ru, rv = rng.integers(0, n, m), rng.integers(0, n, m)
    rw = np.round(rng.normal(size=m), 1)  # floats, negative values, ties
    e = DeviceEdges.from_raw(n, ru, rv, rw, rank_weights=True)
    assert e.weights is not None
    eng = DeviceMST(e)
    eng.run()
    index, _ = eng.paths()
    g = e.to_host()
    rooting = host_rooted(g.n, g.u, g.v, eng.in_mst_host())
    a, b = rng.integers(0, n, 1500), rng.integers(0, n, 1500)
    b[0] = a[0]  # a pair without an edge
    ans = _check_pairs(index, rooting, g.w, a, b)
    wkey, _, _ = expected(rooting, g.w, a, b)
    vals, has = ans.weights(e)
    vals, has = vals.cpu().numpy(), has.cpu().numpy()
    assert vals.dtype == g.weights.dtype and has.tolist() == (wkey != NOKEY).tolist()
    assert np.array_equal(vals[has], g.weights[(wkey[has] & 0xFFFFFFFF).astype(np.int64)])
    assert np.isnan(vals[~has]).all() and (~has).any()


def test_host_path_mstresult_paths(torch_cuda):
    from distributed_ghs_implementation_amd import canonicalize, minimum_spanning_forest
    fx = load_fixture("cgf_n1000_p001.json")
    g = canonicalize(fx["num_nodes"], edges=[tuple(e) for e in fx["edges"]])
    r = minimum_spanning_forest(g)
    rooting = host_rooted(g.n, g.u, g.v, r.in_mst)
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, g.n, 1500), rng.integers(0, g.n, 1500)
    a[:2], b[:2] = [0, 7], [0, 7]
    got, info = r.paths(a, b, return_info=True)
    wkey, wlca, whops = expected(rooting, g.w, a, b)
    has = wkey != NOKEY
    assert np.array_equal(got["lca"], wlca) and np.array_equal(got["hops"], whops)
    assert got["lca"].dtype == np.uint32 and got["eid"].dtype == np.uint32
    assert np.array_equal(got["has_edge"], has) and np.array_equal(got["connected"], wlca != NONE)
    assert np.array_equal(got["eid"][has], (wkey[has] & 0xFFFFFFFF).astype(np.uint32)) and (got["eid"][~has] == NONE).all()
    own = g.w if g.weights is None else g.weights
    assert np.array_equal(got["weight"][has], own[(wkey[has] & 0xFFFFFFFF).astype(np.int64)])
    assert info["queries"] == 1500 and info["connected"] == int((wlca != NONE).sum())
    single = r.paths(int(a[5]), int(b[5]))
    assert single["hops"].tolist() == [int(whops[5])]
    # flags that are not a forest
    from distributed_ghs_implementation_amd import _native
    from distributed_ghs_implementation_amd.mst import MSTResult
    tri = canonicalize(4, edges=[(0, 1, 1), (0, 2, 2), (1, 2, 3)])  # n - 1 flags, one cycle
    with pytest.raises(_native.GHSError) as ei:
        MSTResult(tri, np.ones(3, bool), 6, 1, [], 0.0).paths([0], [1])
    assert ei.value.code == _native.GHS_E_ARG and "not a forest" in str(ei.value)


def test_cli_paths(tmp_path, torch_cuda):
    """--paths OUT.npz --pairs PAIRS.npy end to end, in a fresh process."""
    import shutil

    from distributed_ghs_implementation_amd import read_graph_dir
    from oracle import oracle
    d = tmp_path / "graph_data"
    shutil.copytree(os.path.join(GOLDEN, "graph_data_n6"), d)
    g = read_graph_dir(str(d))
    pairs = np.array(list(itertools.product(range(g.n), repeat=2)), np.int64)
    np.save(tmp_path / "pairs.npy", pairs)
    out = tmp_path / "paths.npz"
    p = subprocess.run([sys.executable, "-m", "distributed_ghs_implementation_amd", "--graph-dir", str(d),
                        "--paths", str(out), "--pairs", str(tmp_path / "pairs.npy")],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    flags = oracle.kruskal_c(g.n, g.u, g.v, g.w)[0][: g.m]
    rooting = host_rooted(g.n, g.u, g.v, flags)
    wkey, wlca, whops = expected(rooting, g.w, pairs[:, 0], pairs[:, 1])
    has = wkey != NOKEY
    got = np.load(out)
    assert sorted(got.files) == ["a", "b", "eid", "hops", "lca", "weight"]
    assert np.array_equal(got["a"], pairs[:, 0]) and np.array_equal(got["b"], pairs[:, 1])
    assert np.array_equal(got["lca"], wlca) and np.array_equal(got["hops"], whops)
    assert np.array_equal(got["eid"][has], (wkey[has] & 0xFFFFFFFF).astype(np.uint32))
    own = g.w if g.weights is None else g.weights
    assert np.array_equal(got["weight"][has], own[(wkey[has] & 0xFFFFFFFF).astype(np.int64)])
    line = f"Path queries: {len(pairs)} pairs, {int((wlca != NONE).sum())} connected, max bottleneck {got['weight'][has].max()}"
    assert line in p.stdout, p.stdout[-2000:]
