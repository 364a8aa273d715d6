"""GPU: tree distances, edge stretch and tree diameters on the rooted forest (ghs_forest_wdepth_* /
ghs_forest_dist_* / ghs_forest_edge_dist_* / ghs_forest_diameter_*, csrc/dist.hip) against plain walks.

The expected answers are computed here, on the host: every tree rooted at its smallest vertex by a
breadth-first pass that adds the weights up (the weighted depth); for a pair (a, b) a climb up the
parent pointers, the deeper end first, that adds up the weights it passes and ends at the meeting
vertex; for a tree the far ends by exhaustive search (a breadth-first pass over the whole tree from
the root, then from p), ties to the smallest id, and on the smaller inputs every eccentricity from
the full matrix of pairwise distances. All comparisons are exact equality."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
INF = (1 << 64) - 1
WMAX = (1 << 32) - 1


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


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def canonical(n, pairs, w):
    """Undirected pairs + weights -> canonical arrays (u < v, sorted by (u, v)); pairs are distinct."""
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    lo, hi = p.min(axis=1), p.max(axis=1)
    order = np.lexsort((hi, lo))
    return lo[order].astype(np.uint32), hi[order].astype(np.uint32), np.asarray(w, np.uint32)[order]


def msf_flags(n, u, v, w):
    from oracle import oracle
    return oracle.kruskal_c(n, u, v, w)[0][: len(u)]


# ---- the expected answers -----------------------------------------------------------------------------
class Reference:
    """A flagged forest on the host: every tree rooted at its smallest vertex by a breadth-first pass.
    hops=True gives every edge the weight 1. Built once per input and only read afterwards."""

    def __init__(self, n, u, v, w, flags, hops=False):
        self.n = n
        self.adj = [[] for _ in range(n)]
        for e in np.flatnonzero(np.asarray(flags) != 0).tolist():
            a, b, c = int(u[e]), int(v[e]), 1 if hops else int(w[e])
            self.adj[a].append((b, c))
            self.adj[b].append((a, c))
        self.parent = np.full(n, -1, np.int64)
        self.pw = np.zeros(n, np.int64)  # the weight of the edge to the parent
        self.depth = np.zeros(n, np.int64)
        self.root_of = np.zeros(n, np.int64)
        self.wdepth = np.zeros(n, np.uint64)
        self.trees = []  # per tree: its vertices in breadth-first order, the root first
        seen = [False] * n
        for r in range(n):
            if seen[r]:
                continue
            seen[r] = True
            order, wd = [r], {r: 0}
            for x in order:  # grows while it is walked
                for y, c in self.adj[x]:
                    if not seen[y]:
                        seen[y] = True
                        self.parent[y], self.pw[y], self.depth[y] = x, c, self.depth[x] + 1
                        wd[y] = wd[x] + c
                        order.append(y)
            for x in order:
                self.root_of[x], self.wdepth[x] = r, wd[x]
            self.trees.append(order)

    STRIDE = 256

    def _strides(self):
        """up[v] = the vertex STRIDE parent steps above v (the root when there are fewer), ws[v] = the
        weights of those steps added up: STRIDE plain passes of one step each."""
        if not hasattr(self, "_up"):
            up, ws = np.arange(self.n, dtype=np.int64), np.zeros(self.n, np.uint64)
            for _ in range(self.STRIDE):
                ws += self.pw[up].astype(np.uint64)  # 0 at a root
                up = np.where(self.parent[up] >= 0, self.parent[up], up)
            self._up, self._ws = up, ws
        return self._up, self._ws

    def climb(self, a, b):
        """(dist, lca) per pair by climbing the parent pointers, all pairs side by side: the deeper end
        climbs, at equal depths both do, until they meet. Where the ends are STRIDE or more levels apart,
        or level and with different vertices STRIDE steps up, the climb takes STRIDE steps at once."""
        up, ws = self._strides()
        S = self.STRIDE
        x, y = np.array(a, np.int64), np.array(b, np.int64)
        dist = np.zeros(len(x), np.uint64)
        apart = self.root_of[x] != self.root_of[y]
        live = ~apart & (x != y)
        while live.any():
            dx, dy = self.depth[x], self.depth[y]
            both = live & (dx == dy) & (up[x] != up[y])
            jx, jy = both | (live & (dx - dy >= S)), both | (live & (dy - dx >= S))
            dist[jx] += ws[x[jx]]
            dist[jy] += ws[y[jy]]
            x[jx], y[jy] = up[x[jx]], up[y[jy]]
            one = live & ~jx & ~jy
            mx, my = one & (dx >= dy), one & (dy >= dx)  # equal depths and still apart: both climb
            dist[mx] += self.pw[x[mx]].astype(np.uint64)
            dist[my] += self.pw[y[my]].astype(np.uint64)
            x[mx], y[my] = self.parent[x[mx]], self.parent[y[my]]
            live &= x != y
        dist[apart] = INF
        return dist, np.where(apart, NONE, x).astype(np.uint32)

    def from_vertex(self, s):
        """{vertex: distance from s} over the whole tree of s, by a breadth-first pass."""
        d, order = {s: 0}, [s]
        for x in order:
            for y, c in self.adj[x]:
                if y not in d:
                    d[y] = d[x] + c
                    order.append(y)
        return d

    @staticmethod
    def farthest(d):
        far = max(d.values())
        return min(x for x, dx in d.items() if dx == far), far

    def diameters(self):
        """Per root: (diameter, p, q) by exhaustive search, ties to the smallest id."""
        out = {}
        for order in self.trees:
            p, _ = self.farthest(self.from_vertex(order[0]))
            q, diam = self.farthest(self.from_vertex(p))
            out[order[0]] = (diam, p, q)
        return out

    def all_pairs(self, order):
        """The full distance matrix of one tree, rows and columns in `order` (breadth-first)."""
        pos = {x: i for i, x in enumerate(order)}
        D = np.zeros((len(order), len(order)), np.uint64)
        for i, x in enumerate(order[1:], 1):
            row = D[pos[int(self.parent[x])], :i] + np.uint64(self.pw[x])
            D[i, :i] = row
            D[:i, i] = row
        return D

    def eccentricities(self):
        ecc = np.zeros(self.n, np.uint64)
        true_diam = {}
        for order in self.trees:
            D = self.all_pairs(order)
            ecc[order] = D.max(axis=1)
            true_diam[order[0]] = int(D.max())
        return ecc, true_diam


def _index(n, u, v, w, flags):
    from distributed_ghs_implementation_amd.device import forest_paths
    e = _edges(n, u, v, w)
    index, info = forest_paths(e, _t(flags, np.uint8))
    return e, index, info


def _check_wdepth(index, ref):
    wd = _u64(index.wdepth())
    assert np.array_equal(wd, ref.wdepth), np.flatnonzero(wd != ref.wdepth)[:8]
    assert index.wdepth() is index.wdepth()  # cached on the index
    assert np.array_equal(_u64(index.wdepth(hops=True)), ref.depth.astype(np.uint64))


def _check_pairs(index, ref, a, b, hops=False):
    dist, lca = index.distances(_t(a), _t(b), hops=hops, lca=True)
    wdist, wlca = ref.climb(a, b)
    dist, lca = _u64(dist), _u32(lca)
    assert np.array_equal(dist, wdist), np.flatnonzero(dist != wdist)[:8]
    assert np.array_equal(lca, wlca), np.flatnonzero(lca != wlca)[:8]
    info = index.last_distance_info
    conn = wdist != INF
    assert info["queries"] == len(a) and info["connected"] == int(conn.sum())
    assert info["disconnected"] == int((~conn).sum())
    assert info["max_dist"] == (int(wdist[conn].max()) if conn.any() else 0)
    only = index.distances(_t(a), _t(b), hops=hops)  # without the lca output
    assert np.array_equal(_u64(only), wdist)


def _check_diameters(tm, ref, ecc=None, true_diam=None):
    """root_of, and per root the diameter and both ends; ecc (the full array) where the caller has it."""
    n = ref.n
    want = ref.diameters()
    assert np.array_equal(_u32(tm.root_of), ref.root_of.astype(np.uint32))
    wdiam, wa, wb = np.zeros(n, np.uint64), np.full(n, NONE, np.uint32), np.full(n, NONE, np.uint32)
    for r, (d, p, q) in want.items():
        wdiam[r], wa[r], wb[r] = d, p, q
    diam, ea, eb = _u64(tm.diameter), _u32(tm.end_a), _u32(tm.end_b)
    assert np.array_equal(diam, wdiam), np.flatnonzero(diam != wdiam)[:8]
    assert np.array_equal(ea, wa), np.flatnonzero(ea != wa)[:8]
    assert np.array_equal(eb, wb), np.flatnonzero(eb != wb)[:8]
    assert tm.roots().cpu().numpy().tolist() == sorted(want)
    info = tm.info
    far = max(d for d, _, _ in want.values())
    widest = min(r for r, (d, _, _) in want.items() if d == far)
    assert (info["num_trees"], info["max_diameter"], info["max_root"]) == (len(want), far, widest)
    if true_diam is not None:  # two sweeps find the true diameter
        assert {r: d for r, (d, _, _) in want.items()} == true_diam
    if ecc is not None:
        got = _u64(tm.ecc)
        assert np.array_equal(got, ecc), np.flatnonzero(got != ecc)[:8]
        inside = np.flatnonzero(ref.root_of == widest)
        least = int(ecc[inside].min())
        centre = int(inside[ecc[inside] == least].min())
        assert (info["min_ecc"], info["center"]) == (least, centre) and tm.center() == (centre, least)


# ---- trivial sizes -------------------------------------------------------------------------------------
def test_trivial_sizes(torch_cuda):
    # n = 1
    e, index, _ = _index(1, [], [], [], [])
    assert _u64(index.wdepth()).tolist() == [0]
    d, lca = index.distances(0, 0, lca=True)
    assert _u64(d).tolist() == [0] and _u32(lca).tolist() == [0]
    tm = index.diameters()
    assert (_u32(tm.root_of).tolist(), _u64(tm.diameter).tolist(), _u32(tm.end_a).tolist(), _u32(tm.end_b).tolist(),
            _u64(tm.ecc).tolist()) == ([0], [0], [0], [0], [0])
    assert tm.info["num_trees"] == 1 and tm.center() == (0, 0)
    ed = index.edge_distances(e)
    assert ed.dist.numel() == 0 and ed.info["edges"] == 0 and ed.info["sum_dist"] == 0 and ed.info["max_eid"] == NONE
    assert index.distances(_t([]), _t([])).numel() == 0  # q == 0
    # n = 2, one edge
    e, index, _ = _index(2, [0], [1], [7], [1])
    assert _u64(index.wdepth()).tolist() == [0, 7]
    assert _u64(index.distances(_t([0, 1, 1, 0]), _t([1, 0, 1, 0]))).tolist() == [7, 7, 0, 0]
    tm = index.diameters()
    assert (_u32(tm.root_of).tolist(), _u64(tm.diameter).tolist(), _u32(tm.end_a).tolist(), _u32(tm.end_b).tolist(),
            _u64(tm.ecc).tolist()) == ([0, 0], [7, 0], [1, NONE], [0, NONE], [7, 7])
    assert tm.info["max_diameter"] == 7 and tm.center() == (0, 7)
    ed = index.edge_distances(e)
    assert _u64(ed.dist).tolist() == [7] and ed.stretch().cpu().numpy().tolist() == [1.0]
    assert (ed.info["sum_dist"], ed.info["sum_w"], ed.info["max_dist"], ed.info["max_eid"], ed.info["tight_edges"],
            ed.info["cross_edges"]) == (7, 7, 7, 0, 1, 0)
    # three isolated vertices, m = 0
    e, index, _ = _index(3, [], [], [], [])
    assert _u64(index.wdepth()).tolist() == [0, 0, 0]
    assert _u64(index.distances(_t([0, 1, 2]), _t([0, 2, 1]))).tolist() == [0, INF, INF]
    tm = index.diameters()
    assert (_u32(tm.root_of).tolist(), _u64(tm.diameter).tolist(), _u32(tm.end_a).tolist(), _u32(tm.end_b).tolist(),
            _u64(tm.ecc).tolist()) == ([0, 1, 2], [0, 0, 0], [0, 1, 2], [0, 1, 2], [0, 0, 0])
    assert tm.info["num_trees"] == 3 and tm.info["max_root"] == 0 and tm.center() == (0, 0)


def test_stretch_of_weightless_edges(torch_cuda):
    """A forest that is not the MSF: a weightless graph edge beside a path of weight 10 (inf), a weightless
    forest edge (0 / 0 = 1), an edge between two trees (inf)."""
    u, v, w = canonical(6, [(0, 1), (1, 2), (0, 2), (2, 3), (3, 4), (4, 5)], [5, 5, 0, 0, 2, 1])
    flags = np.array([1, 0, 1, 1, 0, 1], np.uint8)  # canonical order: (0,1) (0,2) (1,2) (2,3) (3,4) (4,5)
    e, index, _ = _index(6, u, v, w, flags)
    ed = index.edge_distances(e)
    assert _u64(ed.dist).tolist() == [5, 10, 5, 0, INF, 1]
    assert ed.stretch().cpu().numpy().tolist() == [1.0, float("inf"), 1.0, 1.0, float("inf"), 1.0]
    assert (ed.info["sum_dist"], ed.info["sum_w"], ed.info["max_dist"], ed.info["max_eid"], ed.info["cross_edges"],
            ed.info["tight_edges"]) == (21, 11, 10, 1, 1, 4)
    assert ed.average_stretch() == 21 / 11


# ---- a path of 70 000 vertices: K = 17, sums far above 2^32 -----------------------------------------------
def test_path_70000_scrambled_heaviest_weights(torch_cuda):
    n = 70000
    rng = np.random.default_rng(70)
    perm = rng.permutation(n)
    at = int(np.flatnonzero(perm == 0)[0])
    perm[at], perm[1000] = perm[1000], 0  # the root (the smallest id) 1000 steps from one end: two arms
    u, v, w = canonical(n, np.stack([perm[:-1], perm[1:]], axis=1), np.full(n - 1, WMAX))
    flags = np.ones(n - 1, np.uint8)
    e, index, info = _index(n, u, v, w, flags)
    ref = Reference(n, u, v, w, flags)
    assert int(ref.depth.max()) == n - 1001 >= 1 << 16 and info["levels"] == 17  # every doubling level is used
    assert int(ref.wdepth.max()) > 1 << 48
    _check_wdepth(index, ref)
    a, b = rng.integers(0, n, 4096), rng.integers(0, n, 4096)
    a[:3], b[:3] = [perm[0], perm[0], 5], [perm[-1], perm[0], 5]  # end to end, and a == b twice
    _check_pairs(index, ref, a, b)
    tm = index.diameters()
    _check_diameters(tm, ref)
    assert tm.info["max_diameter"] == (n - 1) * WMAX and tm.info["num_trees"] == 1
    r = int(ref.root_of[0])
    assert {int(_u32(tm.end_a)[r]), int(_u32(tm.end_b)[r])} == {int(perm[0]), int(perm[-1])}
    # on a path every eccentricity is the distance to the farther end
    da, db = ref.from_vertex(int(perm[0])), ref.from_vertex(int(perm[-1]))
    assert _u64(tm.ecc).tolist() == [max(da[x], db[x]) for x in range(n)]
    ed = index.edge_distances(e)  # all forest edges: dist == w
    assert np.array_equal(_u64(ed.dist), w.astype(np.uint64))
    assert (ed.info["sum_dist"], ed.info["tight_edges"], ed.info["max_dist"], ed.info["max_eid"]) == ((n - 1) * WMAX, n - 1, WMAX, 0)


# ---- a star with ties ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("hub", [0, 517, 1000])
def test_star_of_1000_leaves_with_ties(hub, torch_cuda):
    n = 1001
    leaves = [x for x in range(n) if x != hub]
    u, v, w = canonical(n, [(hub, x) for x in leaves], np.full(n - 1, 9))
    flags = np.ones(n - 1, np.uint8)
    e, index, _ = _index(n, u, v, w, flags)
    ref = Reference(n, u, v, w, flags)
    _check_wdepth(index, ref)
    ecc, true_diam = ref.eccentricities()
    tm = index.diameters()
    _check_diameters(tm, ref, ecc, true_diam)
    # the tie rule picks the smallest ids: p the smallest vertex at the largest distance from the root 0, q
    # the smallest leaf other than p; the centre is the hub
    p, q = int(_u32(tm.end_a)[0]), int(_u32(tm.end_b)[0])
    assert p == min(x for x in leaves if x != 0)  # the root 0 is the hub or a leaf at distance 0 from itself
    assert q == min(x for x in leaves if x != p) and int(_u64(tm.diameter)[0]) == 18
    assert tm.center() == (hub, 9)
    rng = np.random.default_rng(hub)
    _check_pairs(index, ref, rng.integers(0, n, 3000), rng.integers(0, n, 3000))


# ---- grid 64 x 64, weights in [0, 8): zero weights and many ties ------------------------------------------
@pytest.fixture(scope="module")
def grid_case():
    k = 64
    n = k * k
    rng = np.random.default_rng(64)
    idx = np.arange(n).reshape(k, k)
    pairs = np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], axis=1),
                            np.stack([idx[:-1, :].ravel(), idx[1:, :].ravel()], axis=1)])
    u, v, w = canonical(n, pairs, rng.integers(0, 8, len(pairs)))
    flags = msf_flags(n, u, v, w)
    ref = Reference(n, u, v, w, flags)
    ecc, true_diam = ref.eccentricities()
    edge_dist, _ = ref.climb(u, v)
    return n, u, v, w, flags, ref, ecc, true_diam, edge_dist


def test_grid_edges_and_eccentricities(grid_case, torch_cuda):
    n, u, v, w, flags, ref, ecc, true_diam, wdist = grid_case
    assert (w == 0).sum() > 100 and len(ref.trees) == 1
    e, index, _ = _index(n, u, v, w, flags)
    _check_wdepth(index, ref)
    w64 = w.astype(np.uint64)
    far = int(wdist.max())
    for by_edge in (True, False):
        ed = index.edge_distances(e, by_edge=by_edge)
        if by_edge:
            dist = _u64(ed.dist)
            assert np.array_equal(dist, wdist), np.flatnonzero(dist != wdist)[:8]
            s = ed.stretch().cpu().numpy()
            with np.errstate(divide="ignore", invalid="ignore"):
                want = wdist.astype(np.float64) / w.astype(np.float64)
            want[(wdist == 0) & (w == 0)] = 1.0
            # on an MSF a weightless edge closes a weightless cycle: 0 / 0, defined as 1
            assert np.array_equal(s, want) and (s[flags != 0] == 1.0).all() and (s[w == 0] == 1.0).all()
            assert ed.average_stretch() == sum(int(x) for x in wdist) / int(w64.sum())
        else:
            assert ed.dist is None
            with pytest.raises(ValueError):
                ed.stretch()
        info = ed.info
        assert info["edges"] == len(u) and info["cross_edges"] == 0
        assert info["sum_dist"] == sum(int(x) for x in wdist) and info["sum_w"] == int(w64.sum())
        assert info["max_dist"] == far and info["max_eid"] == int(np.flatnonzero(wdist == far)[0])
        assert info["tight_edges"] == int((wdist == w64).sum()) >= int((flags != 0).sum())
    tm = index.diameters()
    _check_diameters(tm, ref, ecc, true_diam)
    assert index.diameters(ecc=False).ecc is None
    rng = np.random.default_rng(5)
    _check_pairs(index, ref, rng.integers(0, n, 5000), rng.integers(0, n, 5000))


def test_determinism_grid_twice(grid_case, torch_cuda):
    n, u, v, w, flags = grid_case[:5]
    rng = np.random.default_rng(6)
    a, b = _t(rng.integers(0, n, 5000)), _t(rng.integers(0, n, 5000))
    runs = []
    for _ in range(2):
        e, index, _ = _index(n, u, v, w, flags)
        tm = index.diameters()
        ed = index.edge_distances(e)
        runs.append([index.wdepth(), index.wdepth(hops=True), index.distances(a, b), ed.dist, tm.root_of, tm.diameter,
                     tm.end_a, tm.end_b, tm.ecc,
                     {k: x for k, x in ed.info.items() if k != "ms_total"}, {k: x for k, x in tm.info.items() if k != "ms_total"}])
    for x, y in zip(*runs):
        if isinstance(x, dict):
            assert x == y
        else:
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


# ---- R-MAT scale 12, edge factor 4: thousands of trees, most of them single vertices ---------------------------
def test_rmat12_many_trees(torch_cuda):
    from distributed_ghs_implementation_amd.device import DeviceMST, generate_rmat
    e = generate_rmat(12, 4)
    g = e.to_host()
    flags = msf_flags(g.n, g.u, g.v, g.w)
    eng = DeviceMST(e)
    eng.run()
    assert np.array_equal(eng.in_mst_host(), flags != 0)
    ref = Reference(g.n, g.u, g.v, g.w, flags)
    sizes = [len(t) for t in ref.trees]
    print(f"rmat12 ef4: {len(sizes)} trees, {sizes.count(1)} single vertices, the largest of {max(sizes)}")
    assert len(sizes) > 100 and sizes.count(1) >= 50 and max(sizes) > 100
    index, _ = eng.paths()
    _check_wdepth(index, ref)
    rng = np.random.default_rng(12)
    a, b = rng.integers(0, g.n, 6000), rng.integers(0, g.n, 6000)
    lone = [t[0] for t in ref.trees if len(t) == 1][:50]
    big = max(ref.trees, key=len)
    a[:50], b[:50] = lone, big[:50]            # across trees
    a[50:100], b[50:100] = lone, lone          # a == b on single vertices
    a[100:150], b[100:150] = big[:50], big[:50]
    _check_pairs(index, ref, a, b)
    assert (ref.climb(a, b)[0] == INF).sum() >= 50
    # hops: the same distances as the path query's hop counts
    hop_ref = Reference(g.n, g.u, g.v, g.w, flags, hops=True)
    _check_pairs(index, hop_ref, a, b, hops=True)
    hq = _u32(index.query(_t(a), _t(b)).hops)
    hd = _u64(index.distances(_t(a), _t(b), hops=True))
    assert np.array_equal(np.where(hq == NONE, np.uint64(INF), hq.astype(np.uint64)), hd)
    ecc, true_diam = ref.eccentricities()
    _check_diameters(index.diameters(), ref, ecc, true_diam)
    hecc, htrue = hop_ref.eccentricities()
    _check_diameters(index.diameters(hops=True), hop_ref, hecc, htrue)
    # the graph's own edges: none crosses two trees of its MSF
    wdist, _ = ref.climb(g.u, g.v)
    ed = index.edge_distances(e)
    assert np.array_equal(_u64(ed.dist), wdist) and ed.info["cross_edges"] == 0
    assert ed.info["sum_dist"] == sum(int(x) for x in wdist) and ed.info["tight_edges"] == int((wdist == g.w).sum())
    # the engine's shortcuts
    assert np.array_equal(_u64(eng.distances(_t(a), _t(b))), ref.climb(a, b)[0])
    assert eng.diameters(ecc=False).info["max_diameter"] == max(true_diam.values())
    assert eng.edge_distances(by_edge=False).info["sum_dist"] == ed.info["sum_dist"]
    # a forest that does not span: every other edge of the MSF; graph edges now cross trees
    half = flags.copy()
    half[np.flatnonzero(flags)[::2]] = 0
    from distributed_ghs_implementation_amd.device import forest_paths
    hindex, _ = forest_paths(e, _t(half, np.uint8))
    href = Reference(g.n, g.u, g.v, g.w, half)
    hwant, _ = href.climb(g.u, g.v)
    hed = hindex.edge_distances(e)
    inside = hwant != INF
    assert np.array_equal(_u64(hed.dist), hwant) and hed.info["cross_edges"] == int((~inside).sum()) > 0
    assert hed.info["sum_dist"] == sum(int(x) for x in hwant[inside]) and hed.info["sum_w"] == int(g.w[inside].sum(dtype=np.uint64))
    assert np.isinf(hed.stretch().cpu().numpy()[~inside]).all()


# ---- rejections ----------------------------------------------------------------------------------------------
def test_out_of_range_id_and_closed_index(torch_cuda):
    import torch

    from distributed_ghs_implementation_amd import _native
    n = 12
    u, v, w = canonical(n, [(i, i + 1) for i in range(n - 1)], np.arange(n - 1) + 5)
    flags = np.ones(n - 1, np.uint8)
    e, index, _ = _index(n, u, v, w, flags)
    ref = Reference(n, u, v, w, flags)
    for a, b in (([0, n], [1, 1]), ([0, 1], [1, NONE]), ([n + 5], [n + 5])):
        with pytest.raises(_native.GHSError) as ei:
            index.distances(torch.tensor(a, dtype=torch.int64, device="cuda"), torch.tensor(b, dtype=torch.int64, device="cuda"))
        assert ei.value.code == _native.GHS_E_ARG and "vertex id out of range" in str(ei.value)
        _check_pairs(index, ref, np.arange(n), np.arange(n)[::-1].copy())  # the index stays healthy
    with pytest.raises(ValueError):
        index.distances(torch.tensor([-1], device="cuda"), torch.tensor([0], device="cuda"))
    with pytest.raises(ValueError):
        index.distances(_t([0, 1]), _t([0]))
    index.close()
    for call in (lambda: index.distances(0, 1), lambda: index.wdepth(), lambda: index.diameters(),
                 lambda: index.edge_distances(e)):
        with pytest.raises(ValueError, match="closed"):
            call()


def test_cyclic_flags_host_forms(torch_cuda):
    from distributed_ghs_implementation_amd import _native, canonicalize
    from distributed_ghs_implementation_amd.mst import MSTResult
    tri = canonicalize(4, edges=[(0, 1, 1), (0, 2, 2), (1, 2, 3)])  # n - 1 flags, one cycle
    r = MSTResult(tri, np.ones(3, bool), 6, 1, [], 0.0)
    for call in (lambda: r.distances([0], [1]), lambda: r.diameters(), lambda: r.edge_distances()):
        with pytest.raises(_native.GHSError) as ei:
            call()
        assert ei.value.code == _native.GHS_E_ARG and "flags are not a forest" in str(ei.value)


def test_rank_mapped_weights_need_hops(torch_cuda):
    from distributed_ghs_implementation_amd.device import DeviceEdges, DeviceMST
    rng = np.random.default_rng(31)
    n, m = 400, 3000
    ru, rv = rng.integers(0, n, m), rng.integers(0, n, m)
    e = DeviceEdges.from_raw(n, ru, rv, np.round(rng.normal(size=m), 1), rank_weights=True)
    assert e.weights is not None
    eng = DeviceMST(e)
    eng.run()
    index, _ = eng.paths()
    a, b = rng.integers(0, n, 1500), rng.integers(0, n, 1500)
    for call in (lambda: index.wdepth(), lambda: index.distances(_t(a), _t(b)), lambda: index.diameters(),
                 lambda: index.edge_distances(e), lambda: eng.distances(_t(a), _t(b)), lambda: eng.edge_distances(),
                 lambda: eng.diameters()):
        with pytest.raises(ValueError, match="hops=True"):
            call()
    g = e.to_host()
    ref = Reference(g.n, g.u, g.v, g.w, eng.in_mst_host(), hops=True)
    _check_pairs(index, ref, a, b, hops=True)
    _check_diameters(index.diameters(hops=True), ref, *ref.eccentricities())
    assert np.array_equal(_u64(eng.distances(_t(a), _t(b), hops=True)), ref.climb(a, b)[0])


# ---- the host forms and the command line ---------------------------------------------------------------------
def test_host_forms_mstresult(grid_case, torch_cuda):
    from distributed_ghs_implementation_amd.graph import CanonicalGraph
    from distributed_ghs_implementation_amd.mst import MSTResult
    n, u, v, w, flags, ref, ecc, true_diam, wdist = grid_case
    r = MSTResult(CanonicalGraph(n, u, v, w), flags != 0, 0, 1, [], 0.0)
    rng = np.random.default_rng(9)
    a, b = rng.integers(0, n, 2000), rng.integers(0, n, 2000)
    dist, lca, info = r.distances(a, b, return_lca=True, return_info=True)
    want, wlca = ref.climb(a, b)
    assert dist.dtype == np.uint64 and np.array_equal(dist, want) and np.array_equal(lca, wlca)
    assert info["queries"] == 2000 and info["connected"] == 2000 and info["max_dist"] == int(want.max())
    assert r.distances(int(a[3]), int(b[3])).tolist() == [int(want[3])]
    assert np.array_equal(r.distances(a, b, hops=True), Reference(n, u, v, w, flags, hops=True).climb(a, b)[0])
    sd = r.edge_distances()
    assert np.array_equal(sd["dist"], wdist) and sd["sum_dist"] == sum(int(x) for x in wdist)
    assert sd["max_eid"] == int(np.flatnonzero(wdist == wdist.max())[0]) and sd["cross_edges"] == 0
    tm, tinfo = r.diameters(return_info=True)
    want_d = ref.diameters()
    assert np.array_equal(tm["ecc"], ecc) and np.array_equal(tm["root_of"], ref.root_of.astype(np.uint32))
    assert tm["roots"].tolist() == sorted(want_d)
    for root, (d, p, q) in want_d.items():
        assert (int(tm["diameter"][root]), int(tm["end_a"][root]), int(tm["end_b"][root])) == (d, p, q)
    assert tinfo["max_diameter"] == max(true_diam.values()) and tinfo["min_ecc"] == int(ecc.min())


def test_cli_distances_diameters_stretch(tmp_path, torch_cuda):
    """--distances OUT.npz --pairs PAIRS.npy, --diameters OUT.npz and --stretch OUT.npz end to end, in a
    fresh process."""
    import shutil

    from distributed_ghs_implementation_amd import read_graph_dir
    d = tmp_path / "graph_data"
    shutil.copytree(os.path.join(GOLDEN, "graph_data_n6"), d)
    g = read_graph_dir(str(d))
    assert g.weights is None
    pairs = np.array(list(itertools.product(range(g.n), repeat=2)), np.int64)
    np.save(tmp_path / "pairs.npy", pairs)
    outs = {k: tmp_path / f"{k}.npz" for k in ("distances", "diameters", "stretch")}
    p = subprocess.run([sys.executable, "-m", "distributed_ghs_implementation_amd", "--graph-dir", str(d),
                        "--distances", str(outs["distances"]), "--pairs", str(tmp_path / "pairs.npy"),
                        "--diameters", str(outs["diameters"]), "--stretch", str(outs["stretch"])],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    flags = msf_flags(g.n, g.u, g.v, g.w)
    ref = Reference(g.n, g.u, g.v, g.w, flags)
    want, wlca = ref.climb(pairs[:, 0], pairs[:, 1])
    got = np.load(outs["distances"])
    assert sorted(got.files) == ["a", "b", "dist", "lca"]
    assert np.array_equal(got["a"], pairs[:, 0]) and np.array_equal(got["b"], pairs[:, 1])
    assert got["dist"].dtype == np.uint64 and np.array_equal(got["dist"], want) and np.array_equal(got["lca"], wlca)
    conn = want != INF
    assert f"Distances: {len(pairs)} pairs, {int(conn.sum())} connected, max distance {int(want[conn].max())}" in p.stdout
    got = np.load(outs["diameters"])
    ecc, true_diam = ref.eccentricities()
    want_d = ref.diameters()
    assert np.array_equal(got["root_of"], ref.root_of.astype(np.uint32)) and np.array_equal(got["ecc"], ecc)
    assert got["roots"].tolist() == sorted(want_d) and int(got["num_trees"]) == len(want_d)
    for root, (dm, pp, qq) in want_d.items():
        assert (int(got["diameter"][root]), int(got["end_a"][root]), int(got["end_b"][root])) == (dm, pp, qq)
    assert int(got["max_diameter"]) == max(true_diam.values())
    got = np.load(outs["stretch"])
    wdist, _ = ref.climb(g.u, g.v)
    inside = wdist != INF
    assert np.array_equal(got["dist"], wdist) and int(str(got["sum_dist"])) == sum(int(x) for x in wdist[inside])
    assert int(got["sum_w"]) == int(g.w[inside].sum(dtype=np.uint64)) and int(got["tight_edges"]) == int((wdist == g.w).sum())
    # --pairs alone still goes with nothing
    p = subprocess.run([sys.executable, "-m", "distributed_ghs_implementation_amd", "--graph-dir", str(d),
                        "--distances", str(outs["distances"])], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 2 and "--pairs" in p.stderr
