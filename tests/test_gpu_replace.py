"""GPU: replacement edges, bridges and the best swap of the rooted forest (ghs_forest_replace_*,
csrc/replace.hip) against a plain walk.

The expected answer is computed here, on the host: every tree rooted at its smallest vertex by a
breadth-first pass, then every non-forest edge's two ends walked up the parent pointers, one step at a
time, to their meeting point, and its key w << 32 | eid min-ed into every vertex passed. That shares
nothing with the power-of-two ranges of the kernels. tests/test_replace_abi.py checks this walk against
the definition itself (delete the edge, split the tree, take the smallest crossing key)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_fixture

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
NOKEY = (1 << 64) - 1
TILE = 4 * 256  # edges per lane x block size of k_rp_cover


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


def canonical(pairs, w):
    """Undirected distinct pairs + weights -> canonical arrays (u < v, sorted by (u, v)) and the order used."""
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    lo, hi = p.min(axis=1), p.max(axis=1)
    assert (lo != hi).all() and len({(int(a), int(b)) for a, b in zip(lo, hi)}) == len(p)
    order = np.lexsort((hi, lo))
    return lo[order].astype(np.uint32), hi[order].astype(np.uint32), np.asarray(w, np.uint32)[order], order


# ---- the expected answer ---------------------------------------------------------------------------
def host_rooted(n, u, v, flags):
    """parent, parent_eid, depth (python lists) of a forest, every tree rooted at its smallest vertex."""
    adj = [[] for _ in range(n)]
    for e in np.flatnonzero(np.asarray(flags) != 0).tolist():
        a, b = int(u[e]), int(v[e])
        adj[a].append((b, e))
        adj[b].append((a, e))
    parent, peid, depth, seen = [NONE] * n, [NONE] * n, [0] * n, [False] * n
    for r in range(n):
        if seen[r]:
            continue
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
    return parent, peid, depth


def walk_oracle(n, u, v, w, flags):
    """(repl per vertex as uint64, eid per edge as uint32, counts) by walking every non-forest edge's
    ends up the parent pointers to their meeting point."""
    parent, peid, depth = host_rooted(n, u, v, flags)
    m = len(u)
    forest = {peid[x] for x in range(n) if parent[x] != NONE}
    repl = [NOKEY] * n
    covering = cross = 0
    for e in range(m):
        if e in forest:
            continue
        key = (int(w[e]) << 32) | e
        x, y, passed = int(u[e]), int(v[e]), []
        while depth[x] > depth[y]:
            passed.append(x)
            x = parent[x]
        while depth[y] > depth[x]:
            passed.append(y)
            y = parent[y]
        while x != y and parent[x] != NONE:
            passed += [x, y]
            x, y = parent[x], parent[y]
        if x != y:  # two roots
            cross += 1
            continue
        covering += 1
        for z in passed:
            if key < repl[z]:
                repl[z] = key
    by_edge = np.full(m, NONE, np.uint32)
    bridges = improving = 0
    best = None
    for x in range(n):
        if parent[x] == NONE:
            continue
        e = peid[x]
        if repl[x] == NOKEY:
            bridges += 1
            continue
        by_edge[e] = repl[x] & 0xFFFFFFFF
        improving += repl[x] < ((int(w[e]) << 32) | e)
        cand = ((repl[x] >> 32) - int(w[e]), e, repl[x] & 0xFFFFFFFF)
        best = cand if best is None or cand[:2] < best[:2] else best
    counts = {"tree_edges": len(forest), "covering_edges": covering, "cross_edges": cross, "bridges": bridges,
              "improving": improving, "best_delta": best[0] if best else 0,
              "best_out_eid": best[1] if best else NONE, "best_in_eid": best[2] if best else NONE}
    return np.array(repl, np.uint64), by_edge, counts


def kruskal_flags(n, u, v, w, heaviest=False):
    """The MSF's flags by (w, eid) order (heaviest=True: the maximum spanning forest instead)."""
    keys = (np.asarray(w, np.uint64) << np.uint64(32)) | np.arange(len(u), dtype=np.uint64)
    order = np.argsort(keys)[::-1] if heaviest else np.argsort(keys)
    par = list(range(n))

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x
    flags = np.zeros(len(u), np.uint8)
    for e in order.tolist():
        ra, rb = find(int(u[e])), find(int(v[e]))
        if ra != rb:
            par[ra] = rb
            flags[e] = 1
    return flags


def _run(n, u, v, w, flags, levels=None):
    """Index the flagged forest, replace, and compare everything with the walk. Returns (Replacements, info)."""
    from distributed_ghs_implementation_amd.device import forest_paths
    e = _edges(n, u, v, w)
    index, pinfo = forest_paths(e, _t(flags, np.uint8))
    if levels is not None:
        assert pinfo["levels"] == levels, pinfo
    rep, info = index.replacements(e)
    wkey, wby, counts = walk_oracle(n, u, v, w, flags)
    key = rep.key.cpu().numpy().view(np.uint64)
    assert np.array_equal(key, wkey), np.flatnonzero(key != wkey)[:8]
    assert np.array_equal(rep.eid_by_edge.cpu().numpy().view(np.uint32), wby)
    got = {k: info[k] for k in counts}
    assert got == counts, (got, counts)
    assert rep.has_replacement.cpu().numpy().tolist() == (wkey != NOKEY).tolist()
    assert np.array_equal(rep.eid.cpu().numpy().view(np.uint32), (wkey & 0xFFFFFFFF).astype(np.uint32))
    assert np.array_equal(rep.w.cpu().numpy().view(np.uint32), (wkey >> 32).astype(np.uint32))
    assert info["tree_edges"] + info["covering_edges"] + info["cross_edges"] == len(u)
    # a second run on the same index: the same bytes; without the per-edge array: the same keys
    rep2, info2 = index.replacements(e)
    assert bytes(rep2.key.cpu().numpy().data) == bytes(rep.key.cpu().numpy().data)
    assert bytes(rep2.eid_by_edge.cpu().numpy().data) == bytes(rep.eid_by_edge.cpu().numpy().data)
    assert {k: info2[k] for k in counts} == counts
    rep3, _ = index.replacements(e, by_edge=False)
    assert rep3.eid_by_edge is None and np.array_equal(rep3.key.cpu().numpy().view(np.uint64), wkey)
    index.close()
    return rep, info


def _random_tree(n, rng):
    return [(int(rng.integers(0, i)), i) for i in range(1, n)]


def _extra_pairs(n, have, count, rng):
    have = {(min(a, b), max(a, b)) for a, b in have}
    out = []
    while len(out) < count:
        a, b = (int(x) for x in rng.integers(0, n, 2))
        p = (min(a, b), max(a, b))
        if a != b and p not in have:
            have.add(p)
            out.append(p)
    return out


def _tree_plus(n, tree, extra, rng, equal=None):
    """Tree edges with weights below every other edge's, so the tree is the MSF. -> n, u, v, w, flags"""
    pairs = list(tree) + list(extra)
    if equal is None:
        w = np.concatenate([rng.integers(0, 50, len(tree)), rng.integers(50, 120, len(extra))])
    else:
        w = np.full(len(pairs), equal)
    u, v, w, order = canonical(pairs, w)
    flags = np.zeros(len(pairs), np.uint8)
    flags[np.flatnonzero(order < len(tree))] = 1
    return n, u, v, w, flags


# ---- empty and trivial -------------------------------------------------------------------------------
def test_trivial_inputs(torch_cuda):
    z = np.zeros(0, np.uint32)
    for n in (1, 5):  # no edges: every vertex a root, every slot unset
        rep, info = _run(n, z, z, z, np.zeros(0, np.uint8), levels=1)
        assert info["tree_edges"] == 0 and info["best_out_eid"] == NONE and info["best_in_eid"] == NONE
    rng = np.random.default_rng(1)
    n, u, v, w, flags = _tree_plus(20, _random_tree(20, rng), [], rng)  # a tree: every edge a bridge
    rep, info = _run(n, u, v, w, flags)
    assert info["bridges"] == 19 == info["tree_edges"] and info["best_delta"] == 0 and info["best_out_eid"] == NONE
    assert not rep.has_replacement.any()


def test_star_one_level(torch_cuda):
    rng = np.random.default_rng(2)
    tree = [(0, i) for i in range(1, 9)]
    n, u, v, w, flags = _tree_plus(9, tree, [(1, 2), (2, 3), (5, 7), (1, 7)], rng)
    rep, info = _run(n, u, v, w, flags, levels=1)
    assert info["bridges"] == 3 and info["covering_edges"] == 4  # leaves 4, 6, 8 hang on bridges


def test_path_with_all_chords(torch_cuda):
    rng = np.random.default_rng(3)
    tree = [(i, i + 1) for i in range(9)]
    chords = [(a, b) for a in range(10) for b in range(a + 2, 10)]
    assert len(chords) == 36
    n, u, v, w, flags = _tree_plus(10, tree, chords, rng)
    _, info = _run(n, u, v, w, flags, levels=4)
    assert info["bridges"] == 0 and info["improving"] == 0 and info["covering_edges"] == 36
    # the same path hung at its middle: both sides of a chord are non-zero (the smallest vertex is the root)
    relabel = [5, 4, 6, 3, 7, 2, 8, 1, 9, 0]  # path position -> vertex id: position 9 is vertex 0
    tree2 = [(relabel[a], relabel[b]) for a, b in tree]
    chords2 = [(relabel[a], relabel[b]) for a, b in chords]
    n, u, v, w, flags = _tree_plus(10, tree2, chords2, rng)
    _run(n, u, v, w, flags)


def test_balanced_binary_tree(torch_cuda):
    rng = np.random.default_rng(4)
    tree = [((i - 1) // 2, i) for i in range(1, 63)]
    n, u, v, w, flags = _tree_plus(63, tree, _extra_pairs(63, tree, 40, rng), rng)
    _, info = _run(n, u, v, w, flags, levels=3)
    assert info["covering_edges"] == 40 and info["improving"] == 0


def test_deep_path_with_chords(torch_cuda):
    rng = np.random.default_rng(5)
    tree = [(i, i + 1) for i in range(1099)]
    n, u, v, w, flags = _tree_plus(1100, tree, _extra_pairs(1100, tree, 1500, rng), rng)
    _, info = _run(n, u, v, w, flags, levels=11)
    assert info["improving"] == 0 and info["best_delta"] >= 0


def test_three_trees_and_cross_edges(torch_cuda):
    rng = np.random.default_rng(6)
    sizes, base, tree, inside, between = (12, 17, 9), 0, [], [], []
    blocks = []
    for s in sizes:
        ids = list(range(base, base + s))
        blocks.append(ids)
        t = [(ids[a], ids[b]) for a, b in _random_tree(s, rng)]
        tree += t
        inside += [(ids[a], ids[b]) for a, b in _extra_pairs(s, [(ids.index(p), ids.index(q)) for p, q in t], 6, rng)]
        base += s
    between = [(blocks[0][3], blocks[1][5]), (blocks[1][0], blocks[2][8]), (blocks[0][11], blocks[2][0]),
               (blocks[0][0], blocks[1][0]), (blocks[1][16], blocks[2][4])]
    n, u, v, w, flags = _tree_plus(base, tree, inside + between, rng)
    _, info = _run(n, u, v, w, flags)
    assert info["cross_edges"] == 5 and info["covering_edges"] == 18 and info["tree_edges"] == base - 3


def test_equal_weights_ties_by_eid(torch_cuda):
    rng = np.random.default_rng(7)
    tree = _random_tree(40, rng)
    n, u, v, w, flags = _tree_plus(40, tree, _extra_pairs(40, tree, 60, rng), rng, equal=7)
    rep, info = _run(n, u, v, w, flags)
    assert info["best_delta"] == 0 and info["bridges"] < info["tree_edges"]  # the counts: against the walk in _run
    keys = rep.key.cpu().numpy().view(np.uint64)
    assert ((keys[keys != NOKEY] >> np.uint64(32)) == 7).all()


@pytest.mark.parametrize("m", [TILE - 1, TILE, TILE + 1, 4 * TILE + 1])
def test_tile_edges_of_the_cover_kernel(torch_cuda, m):
    rng = np.random.default_rng(8)
    n = 300
    tree = _random_tree(n, rng)
    n, u, v, w, flags = _tree_plus(n, tree, _extra_pairs(n, tree, m - len(tree), rng), rng)
    assert len(u) == m
    _run(n, u, v, w, flags)


def test_slices_at_a_16_byte_offset(torch_cuda):
    from distributed_ghs_implementation_amd.device import DeviceEdges, forest_paths
    rng = np.random.default_rng(9)
    tree = _random_tree(100, rng)
    n, u, v, w, flags = _tree_plus(100, tree, _extra_pairs(100, tree, 1200, rng), rng)
    pad = np.full(4, 0xDEADBEEF, np.uint32)
    tu, tv, tw = (_t(np.concatenate([pad, a, pad]))[4:4 + len(a)] for a in (u, v, w))
    assert tu.data_ptr() % 256 == 16
    e = DeviceEdges(n, tu, tv, tw)
    index, _ = forest_paths(e, _t(flags, np.uint8))
    rep, info = index.replacements(e)
    wkey, wby, counts = walk_oracle(n, u, v, w, flags)
    assert np.array_equal(rep.key.cpu().numpy().view(np.uint64), wkey)
    assert np.array_equal(rep.eid_by_edge.cpu().numpy().view(np.uint32), wby)
    assert {k: info[k] for k in counts} == counts
    index.close()


def test_flags_that_are_not_the_msf(torch_cuda):
    rng = np.random.default_rng(10)
    tree = _random_tree(80, rng)
    n, u, v, w, _ = _tree_plus(80, tree, _extra_pairs(80, tree, 200, rng), rng)
    heavy = kruskal_flags(n, u, v, w, heaviest=True)
    _, info = _run(n, u, v, w, heavy)
    assert info["improving"] > 0 and info["best_delta"] < 0
    _, info = _run(n, u, v, w, kruskal_flags(n, u, v, w))
    assert info["improving"] == 0 and info["best_delta"] >= 0


def test_device_argument_errors_on_a_live_index(torch_cuda):
    """The checks that need an index over n > 0: NULL d_repl, a short workspace, an endpoint >= n."""
    import ctypes

    from distributed_ghs_implementation_amd import _native
    from distributed_ghs_implementation_amd.device import forest_paths
    torch = torch_cuda
    rng = np.random.default_rng(11)
    tree = [(i, i + 1) for i in range(19)]
    n, u, v, w, flags = _tree_plus(20, tree, _extra_pairs(20, tree, 30, rng), rng)
    e = _edges(n, u, v, w)
    index, pinfo = forest_paths(e, _t(flags, np.uint8))
    L = _native.load()
    wb = L.ghs_forest_replace_workspace_bytes(n, pinfo["max_depth"])
    assert wb == 8 * 4 * n + (-8 * 4 * n) % 256 + 256
    key = torch.empty(n, dtype=torch.int64, device="cuda")
    ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
    res = _native.ReplaceResult()

    def call(m=len(u), tu=e.u, repl=key.data_ptr(), wbytes=wb):
        return L.ghs_forest_replace_device(index._h, m, tu.data_ptr(), e.v.data_ptr(), e.w.data_ptr(), repl, None,
                                           ws.data_ptr(), wbytes, None, ctypes.byref(res))
    assert call(repl=None) == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error()
    assert call(wbytes=wb - 1) == _native.GHS_E_NOMEM
    bad = e.u.clone()
    bad[len(u) - 1] = n  # one endpoint out of range, at the last position
    assert call(tu=bad) == _native.GHS_E_ARG and b"out of range" in L.ghs_last_error()
    assert call() == _native.GHS_OK
    assert np.array_equal(key.cpu().numpy().view(np.uint64), walk_oracle(n, u, v, w, flags)[0])
    index.close()


# ---- a golden fixture with the engine's own flags -------------------------------------------------------
def _host_bridges(n, u, v):
    """The number of bridges of the graph by an iterative DFS (low-link)."""
    adj = [[] for _ in range(n)]
    for e in range(len(u)):
        adj[int(u[e])].append((int(v[e]), e))
        adj[int(v[e])].append((int(u[e]), e))
    disc, low, t, bridges = [-1] * n, [0] * n, 0, 0
    for r in range(n):
        if disc[r] >= 0:
            continue
        disc[r] = low[r] = t
        t += 1
        stack = [(r, -1, iter(adj[r]))]
        while stack:
            x, pe, it = stack[-1]
            for y, e in it:
                if e == pe:
                    continue
                if disc[y] < 0:
                    disc[y] = low[y] = t
                    t += 1
                    stack.append((y, e, iter(adj[y])))
                    break
                low[x] = min(low[x], disc[y])
            else:
                stack.pop()
                if stack:
                    px = stack[-1][0]
                    low[px] = min(low[px], low[x])
                    bridges += low[x] > disc[px]
    return bridges


def test_golden_fixture_with_the_engines_flags(torch_cuda):
    from distributed_ghs_implementation_amd import canonicalize, minimum_spanning_forest
    fx = load_fixture("cgf_n1000_p001.json")
    raw = [tuple(e) for e in fx["edges"]]
    g = canonicalize(fx["num_nodes"], edges=raw)
    r = minimum_spanning_forest(g)
    out, info = r.replacements(return_info=True, per_vertex=True)
    wkey, wby, counts = walk_oracle(g.n, g.u, g.v, g.w, r.in_mst)
    assert np.array_equal(out["eid"], wby) and np.array_equal(out["key"], wkey)
    assert {k: info[k] for k in counts} == counts
    assert info["improving"] == 0 and info["tree_edges"] == r.num_edges
    assert info["bridges"] == _host_bridges(g.n, g.u, g.v) == int(out["is_bridge"].sum())
    assert np.array_equal(out["has_replacement"], wby != NONE)
    own = g.w if g.weights is None else g.weights
    assert np.array_equal(out["weight"][out["has_replacement"]], own[wby[wby != NONE].astype(np.int64)])
    assert out["second_best_weight"] == r.total_weight + info["best_delta"]
    # take a forest edge out of the graph: the replacement is flagged instead
    forest = np.flatnonzero(r.in_mst)
    picks = [int(info["best_out_eid"]), int(forest[len(forest) // 2])]
    picks.append(int(np.flatnonzero(out["is_bridge"])[0]) if out["is_bridge"].any() else int(forest[-1]))
    trees = g.n - r.num_edges
    for e in picks:
        keep = np.ones(g.m, bool)
        keep[e] = False
        g2 = canonicalize(g.n, u=g.u[keep], v=g.v[keep], w=g.w[keep])
        r2 = minimum_spanning_forest(g2)
        was = {(int(a), int(b)) for a, b in zip(g.u[r.in_mst], g.v[r.in_mst])}
        now = {(int(a), int(b)) for a, b in zip(g2.u[r2.in_mst], g2.v[r2.in_mst])}
        gone = (int(g.u[e]), int(g.v[e]))
        if out["is_bridge"][e]:
            assert now == was - {gone} and g2.n - r2.num_edges == trees + 1
            assert r2.total_weight == r.total_weight - int(g.w[e])
        else:
            f = int(out["eid"][e])
            assert now == (was - {gone}) | {(int(g.u[f]), int(g.v[f]))} and g2.n - r2.num_edges == trees
            assert r2.total_weight == r.total_weight + int(g.w[f]) - int(g.w[e])
    assert r.total_weight + info["best_delta"] == out["second_best_weight"]


def test_float_weights_report_the_callers_values(torch_cuda):
    from distributed_ghs_implementation_amd import canonicalize, minimum_spanning_forest
    rng = np.random.default_rng(12)
    tree = _random_tree(30, rng)
    pairs = tree + _extra_pairs(30, tree, 50, rng)
    vals = np.round(rng.uniform(-3.0, 9.0, len(pairs)), 2)
    g = canonicalize(30, edges=[(a, b, float(x)) for (a, b), x in zip(pairs, vals)])
    assert g.weights is not None and g.weights.dtype.kind == "f"
    r = minimum_spanning_forest(g)
    out, info = r.replacements(return_info=True)
    _, wby, counts = walk_oracle(g.n, g.u, g.v, g.w, r.in_mst)
    assert np.array_equal(out["eid"], wby) and {k: info[k] for k in counts} == counts
    has = wby != NONE
    assert out["weight"].dtype == g.weights.dtype
    assert np.array_equal(out["weight"][has], g.weights[wby[has].astype(np.int64)]) and np.isnan(out["weight"][~has]).all()
    deltas = g.weights[wby[has].astype(np.int64)] - g.weights[has]
    assert (deltas >= 0).all() and out["second_best_weight"] == r.total_weight + float(deltas.min())


def test_cli_writes_the_npz(torch_cuda, tmp_path):
    from distributed_ghs_implementation_amd import minimum_spanning_forest
    from distributed_ghs_implementation_amd.graph import read_graph_dir
    d = tmp_path / "graph_data"
    shutil.copytree(os.path.join(GOLDEN, "graph_data_n6"), d)
    g = read_graph_dir(str(d))
    out = tmp_path / "replacements.npz"
    p = subprocess.run([sys.executable, "-m", "distributed_ghs_implementation_amd", "--graph-dir", str(d),
                        "--replacements", str(out)], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    wkey, wby, counts = walk_oracle(g.n, g.u, g.v, g.w, minimum_spanning_forest(g).in_mst)
    got = np.load(out)
    assert sorted(got.files) == sorted(["eid_by_edge", "key"] + list(counts))
    assert np.array_equal(got["eid_by_edge"], wby) and np.array_equal(got["key"], wkey)
    assert {k: int(got[k]) for k in counts} == counts
    assert f"Replacements: {counts['tree_edges']} forest edges, {counts['bridges']} bridges" in p.stdout, p.stdout[-2000:]
