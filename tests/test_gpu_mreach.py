"""Core distances and mutual reachability on the GPU (device.mutual_reachability / ghs_mutual_reach_device)
and HDBSCAN end to end (device.hdbscan), against numpy: the symmetric CSR built by scipy and one
np.partition per row. core and w_out are compared exactly, on the smallest graphs at which each path of
csrc/mreach.hip can go wrong: degenerate inputs, the short-row rule, stars whose hub row is all forward, all
reverse or mixed, hub degrees at both class boundaries (the result says which class ran), ties, the ends of
the weight range, small and large k, rank-mapped floats, scikit-learn's own mutual-reachability graph, and
scipy's minimum spanning tree and connected components of the reference graph for the end-to-end call."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32_MAX = (1 << 32) - 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from distributed_ghs_implementation_amd import _native
    assert _native.device_count() > 0
    return torch


def _classes():
    from distributed_ghs_implementation_amd import _native
    return _native.GHS_MREACH_BLOCK_ROW_MIN, _native.GHS_MREACH_GRID_ROW_MIN


# ---- the reference ------------------------------------------------------------------------------------------
def ref_rows(n, u, v):
    """indptr and, per entry, the canonical edge it is: the symmetric CSR of the list, built by scipy"""
    import scipy.sparse as sp
    m = len(u)
    eid = np.arange(1, m + 1, dtype=np.int64)                    # + 1: no explicit zeros
    A = sp.csr_matrix((np.concatenate([eid, eid]), (np.concatenate([u, v]), np.concatenate([v, u]))), shape=(n, n))
    return A.indptr.astype(np.int64), A.data - 1


def ref_mreach(n, u, v, w, k):
    """core (of w's dtype; 0 for an isolated vertex, the row's maximum for a short row), w_out, degrees"""
    u, v, w = np.asarray(u, np.int64), np.asarray(v, np.int64), np.asarray(w)
    indptr, eid = ref_rows(n, u, v)
    core = np.zeros(n, dtype=w.dtype)
    deg = np.diff(indptr)
    one = np.nonzero(deg == 1)[0]
    core[one] = w[eid[indptr[one]]]                              # a row of one entry is its own k-th smallest
    for x in np.nonzero(deg > 1)[0]:
        row = w[eid[indptr[x]:indptr[x + 1]]]
        kk = min(k, len(row))
        core[x] = np.partition(row, kk - 1)[kk - 1]
    w_out = np.maximum(np.maximum(core[u], core[v]), w) if len(u) else w.copy()
    return core, w_out, deg


def canonical(n, a, b, w):
    """any pairs -> the canonical list: u < v, (u, v) strictly ascending, the first weight of a pair kept"""
    a, b, w = np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(w)
    keep = a != b
    a, b, w = a[keep], b[keep], w[keep]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    _, first = np.unique(lo * n + hi, return_index=True)
    return lo[first].astype(np.uint32), hi[first].astype(np.uint32), w[first]


def star(hub, deg):
    """hub joined to deg leaves: n = deg + 1"""
    n = deg + 1
    leaves = np.delete(np.arange(n, dtype=np.int64), hub)
    return n, np.minimum(leaves, hub).astype(np.uint32), np.maximum(leaves, hub).astype(np.uint32)


def path(n):
    return np.arange(n - 1, dtype=np.uint32), np.arange(1, n, dtype=np.uint32)


def weights(rng, m, mode):
    if mode == "ties":
        return rng.integers(1, 8, m).astype(np.uint32)
    if mode == "equal":
        return np.full(m, 77, np.uint32)
    return rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def skewed_graph():
    """1500 vertices, degrees from 0 to several hundred: every class below the grid rows in one list"""
    rng = np.random.default_rng(11)
    n, t = 1500, 20000
    a = ((n - 20) * rng.random(t) ** 3).astype(np.int64)
    b = rng.integers(0, n - 20, t)                               # the last 20 vertices stay isolated
    u, v, w = canonical(n, a, b, rng.integers(0, 1 << 32, t, dtype=np.uint64).astype(np.uint32))
    return n, u, v, w


@functools.lru_cache(maxsize=None)
def skewed_ref(k):
    n, u, v, w = skewed_graph()
    return ref_mreach(n, u, v, w, k)


# ---- the device ----------------------------------------------------------------------------------------------
def dev_edges(torch, n, u, v, w, csr=False):
    from distributed_ghs_implementation_amd.device import DeviceEdges

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).cuda()
    e = DeviceEdges(n, dev(u), dev(v), dev(w))
    return e.with_csr() if csr else e


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def run(torch, n, u, v, w, k, **kw):
    from distributed_ghs_implementation_amd.device import mutual_reachability
    kw.setdefault("short_rows", "clamp")
    mr = mutual_reachability(dev_edges(torch, n, u, v, w), min_samples=k, **kw)
    return u32(mr.core), u32(mr.edges.w), mr.info


def check(torch, n, u, v, w, k, block_rows=None, grid_rows=None):
    core, w_out, info = run(torch, n, u, v, w, k)
    rc, rw, deg = ref_mreach(n, u, v, w, k)
    assert np.array_equal(core, rc), (n, k, np.nonzero(core != rc)[0][:8])
    assert np.array_equal(w_out, rw), (n, k, np.nonzero(w_out != rw)[0][:8])
    B, G = _classes()
    assert info["short_rows"] == int(((deg > 0) & (deg < k)).sum())
    assert info["isolated"] == int((deg == 0).sum())
    assert info["raised_edges"] == int((rw > np.asarray(w)).sum())
    assert info["max_degree"] == (int(deg.max()) if n else 0)
    assert info["block_rows"] == int(((deg >= B) & (deg < G)).sum())
    assert info["grid_rows"] == int((deg >= G).sum())
    if block_rows is not None:
        assert (info["block_rows"], info["grid_rows"]) == (block_rows, grid_rows), info
    return info


def raw_call(torch, n, u, v, w, k, mode):
    """the C entry itself: mode "out" (w_out its own buffer), "inplace" (w_out == w) or "null" (no w_out)"""
    from distributed_ghs_implementation_amd import _native
    from distributed_ghs_implementation_amd.device import _ptr, _stream
    L = _native.load()
    e = dev_edges(torch, n, u, v, w)
    m = len(u)
    core = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    out = torch.full((max(m, 1),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ws_bytes = int(L.ghs_mutual_reach_workspace_bytes(n, m))
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device="cuda")
    res = _native.MreachResult()
    w_out = {"out": _ptr(out), "inplace": _ptr(e.w), "null": None}[mode]
    _native.check(L.ghs_mutual_reach_device(n, m, _ptr(e.u), _ptr(e.v), _ptr(e.w), k, _ptr(core), w_out, _ptr(ws), ws_bytes,
                                            _stream(), ctypes.byref(res)))
    torch.cuda.synchronize()
    return u32(core), u32(out)[:m], u32(e.w), res.as_dict()


# ---- degenerate inputs and the short-row rule ---------------------------------------------------------------------
def test_one_vertex_no_edges_single_edge(torch_cuda):
    none = np.zeros(0, np.uint32)
    for n in (1, 5):
        info = check(torch_cuda, n, none, none, none, 3)
        assert info["isolated"] == n and info["short_rows"] == 0
    one = np.array([9], np.uint32)
    for k in (1, 2):
        info = check(torch_cuda, 2, np.array([0], np.uint32), np.array([1], np.uint32), one, k)
        assert info["short_rows"] == (2 if k == 2 else 0)
    check(torch_cuda, 7, np.array([2], np.uint32), np.array([5], np.uint32), one, 1)   # isolated vertices around it
    core, w_out, _ = run(torch_cuda, 2, np.array([0], np.uint32), np.array([1], np.uint32), one, 1)
    assert core.tolist() == [9, 9] and w_out.tolist() == [9]


@pytest.mark.parametrize("k", [1, 2, 3])
def test_path_crosses_the_short_row_rule(torch_cuda, k):
    n = 9
    u, v = path(n)
    w = np.array([5, 1, 7, 3, 3, 8, 2, 6], np.uint32)
    info = check(torch_cuda, n, u, v, w, k)
    assert info["short_rows"] == {1: 0, 2: 2, 3: n}[k]           # the ends have one edge, the others two
    core, w_out, _ = run(torch_cuda, n, u, v, w, k)
    if k == 1:
        assert core.tolist() == [5, 1, 1, 3, 3, 3, 2, 2, 6] and w_out.tolist() == [5, 1, 7, 3, 3, 8, 2, 6]
    if k == 3:                                                   # clamped: the larger of the two edges
        assert core.tolist() == [5, 5, 7, 7, 3, 8, 8, 6, 6] and w_out.tolist() == [5, 7, 7, 7, 8, 8, 8, 6]


def test_short_rows_policy(torch_cuda):
    from distributed_ghs_implementation_amd.device import mutual_reachability
    n = 9
    u, v = path(n)
    w = np.array([5, 1, 7, 3, 3, 8, 2, 6], np.uint32)
    e = dev_edges(torch_cuda, n, u, v, w)
    with pytest.raises(ValueError, match=r"9 vertices.*min_samples = 3"):
        mutual_reachability(e, min_samples=3)                    # short_rows="error" is the default
    with pytest.raises(ValueError, match=r"2 vertices.*min_samples = 2"):
        e.mutual_reachability(min_samples=2, short_rows="error")
    assert np.array_equal(u32(e.w), w)                           # the input is untouched
    mr = mutual_reachability(e, min_samples=3, short_rows="clamp")
    assert u32(mr.core).tolist() == [5, 5, 7, 7, 3, 8, 8, 6, 6] and mr.info["short_rows"] == 9
    # isolated vertices are no error
    mr = mutual_reachability(dev_edges(torch_cuda, 12, u, v, w), min_samples=1)
    assert mr.info["isolated"] == 3 and u32(mr.core)[9:].tolist() == [0, 0, 0]


@pytest.mark.parametrize("k", [4, 33, 257])
def test_degrees_just_below_at_and_above_k(torch_cuda, k):
    """three hubs of degree k - 1, k and k + 1 over shared leaves: the first is a short row"""
    rng = np.random.default_rng(k)
    n = 3 + k + 1
    a = np.concatenate([np.full(d, h) for h, d in enumerate((k - 1, k, k + 1))])
    b = np.concatenate([3 + np.arange(d) for d in (k - 1, k, k + 1)])
    u, v, w = canonical(n, a, b, weights(rng, len(a), "wide"))
    core, _, _ = run(torch_cuda, n, u, v, w, k)
    _, _, deg = ref_mreach(n, u, v, w, k)
    assert deg[:3].tolist() == [k - 1, k, k + 1]
    for h in range(3):
        row = np.sort(w[u == h])
        assert core[h] == row[min(k, len(row)) - 1]              # the maximum, the maximum, the second largest
    check(torch_cuda, n, u, v, w, k)


# ---- stars: one long row, forward, reverse or mixed, at the class boundaries ------------------------------
def _hub(where, deg):
    return {"first": 0, "last": deg, "middle": deg // 2 + 1}[where]


def _star_degrees():
    B, G = _classes()
    return [5, 32, 33, 64, B - 1, B, B + 1, 4099, G - 1, G, G + 1]


@pytest.mark.parametrize("where", ["first", "last", "middle"])
@pytest.mark.parametrize("deg", _star_degrees())
def test_star_hub_classes(torch_cuda, where, deg):
    B, G = _classes()
    rng = np.random.default_rng(deg)
    n, u, v = star(_hub(where, deg), deg)
    if where == "first":
        assert (u == 0).all()                                    # the hub's row is all forward
    if where == "last":
        assert (v == deg).all()                                  # all reverse
    if where == "middle":
        assert 0 < int((u == _hub(where, deg)).sum()) < deg      # mixed
    block, grid = int(B <= deg < G), int(deg >= G)
    for mode in ("wide", "ties"):
        w = weights(rng, deg, mode)
        for k in sorted({1, 2, deg // 3 + 1, deg - 1, deg, deg + 7}):
            if k >= 1:
                check(torch_cuda, n, u, v, w, k, block_rows=block, grid_rows=grid)


def test_two_grid_rows_share_the_grid(torch_cuda):
    """both hubs of a double star are grid rows: one all forward, one all reverse, histogrammed together"""
    B, G = _classes()
    rng = np.random.default_rng(5)
    n = G + 300
    mid = np.arange(1, n - 1)
    u = np.concatenate([np.zeros(n - 2, np.int64), mid])
    v = np.concatenate([mid, np.full(n - 2, n - 1)])
    u, v, w = canonical(n, u, v, weights(rng, len(u), "wide"))
    for k in (1, 2, 1000, G):
        check(torch_cuda, n, u, v, w, k, block_rows=0, grid_rows=2)
    check(torch_cuda, n, u, v, weights(rng, len(u), "ties"), 3, block_rows=0, grid_rows=2)


# ---- weights: ties, the ends of the range, duplicates around the k-th ------------------------------------
@pytest.mark.parametrize("deg", [6, 40, 300])
def test_equal_weights_and_range_ends_and_duplicate_runs(torch_cuda, deg):
    rng = np.random.default_rng(deg)
    n, u, v = star(deg // 2, deg)
    check(torch_cuda, n, u, v, weights(rng, deg, "equal"), 3)
    w = weights(rng, deg, "wide")
    w[0], w[-1] = 0, U32_MAX                                     # both ends of the range in the hub's row
    w[1], w[2] = 0, U32_MAX
    for k in (1, 2, 3, deg - 2, deg - 1, deg):
        check(torch_cuda, n, u, v, w, k)
    assert run(torch_cuda, n, u, v, w, 1)[0][deg // 2] == 0 and run(torch_cuda, n, u, v, w, deg)[0][deg // 2] == U32_MAX
    # the k-th value inside a run of duplicates: 2 below, a run of deg - 4 equal values, 2 above
    w = np.full(deg, 1 << 31, np.uint32)
    w[:2], w[-2:] = (5, 6), ((1 << 31) + 1, U32_MAX)
    w = rng.permutation(w)
    for k in (2, 3, deg // 2, deg - 2, deg - 1):
        core, _, _ = run(torch_cuda, n, u, v, w, k)
        assert core[deg // 2] == ((1 << 31) if 3 <= k <= deg - 2 else np.sort(w)[k - 1])
        check(torch_cuda, n, u, v, w, k)


@pytest.mark.parametrize("k", [1, 64, 1000])
def test_small_and_large_k_on_a_skewed_graph(torch_cuda, k):
    n, u, v, w = skewed_graph()
    rc, rw, deg = skewed_ref(k)
    B, G = _classes()
    assert deg.min() == 0 and ((deg > 0) & (deg <= 32)).any() and ((deg > 32) & (deg < B)).any() and (deg >= B).any()
    core, w_out, info = run(torch_cuda, n, u, v, w, k)
    assert np.array_equal(core, rc) and np.array_equal(w_out, rw)
    assert info["block_rows"] == int((deg >= B).sum()) > 1 and info["grid_rows"] == 0
    assert info["short_rows"] == int(((deg > 0) & (deg < k)).sum()) and info["isolated"] == int((deg == 0).sum())


@pytest.mark.parametrize("seed,n,t,k", [(1, 2000, 9000, 3), (2, 1999, 30000, 5), (3, 257, 4000, 15), (4, 64, 2016, 40)])
def test_random_sparse_graphs_with_heavy_ties(torch_cuda, seed, n, t, k):
    rng = np.random.default_rng(seed)
    u, v, w = canonical(n, rng.integers(0, n, t), rng.integers(0, n, t), weights(rng, t, "ties"))
    check(torch_cuda, n, u, v, w, k)
    check(torch_cuda, n, u, v, weights(rng, len(u), "wide"), k)


# ---- outputs and policies ---------------------------------------------------------------------------------------
def test_in_place_null_output_and_determinism(torch_cuda):
    n, u, v, w = skewed_graph()
    rc, rw, _ = skewed_ref(5)
    core_o, out_o, w_o, info_o = raw_call(torch_cuda, n, u, v, w, 5, "out")
    assert np.array_equal(core_o, rc) and np.array_equal(out_o, rw) and np.array_equal(w_o, w)   # w only read
    core_i, out_i, w_i, info_i = raw_call(torch_cuda, n, u, v, w, 5, "inplace")
    assert core_i.tobytes() == core_o.tobytes() and w_i.tobytes() == out_o.tobytes()
    assert (out_i == 0x5A5A5A5A).all()                           # the spare buffer was not touched
    core_n, out_n, w_n, info_n = raw_call(torch_cuda, n, u, v, w, 5, "null")
    assert core_n.tobytes() == core_o.tobytes() and (out_n == 0x5A5A5A5A).all() and np.array_equal(w_n, w)
    assert info_n["raised_edges"] == 0 and info_o["raised_edges"] == info_i["raised_edges"] == int((rw > w).sum())
    core_2, out_2, _, info_2 = raw_call(torch_cuda, n, u, v, w, 5, "out")
    assert core_2.tobytes() == core_o.tobytes() and out_2.tobytes() == out_o.tobytes()
    strip = {k: x for k, x in info_o.items() if k != "ms_total"}
    assert strip == {k: x for k, x in info_2.items() if k != "ms_total"}


def test_python_in_place_shares_and_copies(torch_cuda):
    from distributed_ghs_implementation_amd.device import mutual_reachability
    n, u, v, w = skewed_graph()
    _, rw, _ = skewed_ref(5)
    e = dev_edges(torch_cuda, n, u, v, w, csr=True)
    mr = mutual_reachability(e, min_samples=5, short_rows="clamp")
    assert mr.edges is not e and mr.edges.u is e.u and mr.edges.v is e.v and mr.edges.off is e.off
    assert np.array_equal(u32(e.w), w) and np.array_equal(u32(mr.edges.w), rw)
    mr2 = e.mutual_reachability(min_samples=5, short_rows="clamp", in_place=True)
    assert mr2.edges is e and np.array_equal(u32(e.w), rw) and np.array_equal(u32(mr2.core), u32(mr.core))


def test_include_self(torch_cuda):
    from distributed_ghs_implementation_amd.device import mutual_reachability
    n, u, v, w = skewed_graph()
    e = dev_edges(torch_cuda, n, u, v, w)
    mr = mutual_reachability(e, min_samples=6, short_rows="clamp", include_self=True)
    rc, rw, _ = skewed_ref(5)                                    # the point itself is the first neighbour
    assert mr.info["k"] == 5 and np.array_equal(u32(mr.core), rc) and np.array_equal(u32(mr.edges.w), rw)
    mr = mutual_reachability(e, min_samples=1, include_self=True)   # nothing left to select: no library call
    assert mr.info["k"] == 0 and not u32(mr.core).any() and np.array_equal(u32(mr.edges.w), w)
    assert mr.edges.w.data_ptr() != e.w.data_ptr()


def test_coo_and_csr_lists_agree(torch_cuda):
    from distributed_ghs_implementation_amd.device import mutual_reachability
    n, u, v, w = skewed_graph()
    a = mutual_reachability(dev_edges(torch_cuda, n, u, v, w), min_samples=4, short_rows="clamp")
    b = mutual_reachability(dev_edges(torch_cuda, n, u, v, w, csr=True), min_samples=4, short_rows="clamp")
    assert b.edges.off is not None and a.edges.off is None
    assert u32(a.core).tobytes() == u32(b.core).tobytes() and u32(a.edges.w).tobytes() == u32(b.edges.w).tobytes()
    with pytest.raises(ValueError, match="COO"):
        mutual_reachability(dev_edges(torch_cuda, n, u, v, w).csr_only(), min_samples=4)


def test_noncanonical_list_is_refused(torch_cuda):
    from distributed_ghs_implementation_amd import _native
    from distributed_ghs_implementation_amd.device import mutual_reachability
    u, v = np.array([0, 0, 1], np.uint32), np.array([2, 1, 2], np.uint32)      # (0, 2) before (0, 1)
    with pytest.raises(_native.GHSError) as ei:
        mutual_reachability(dev_edges(torch_cuda, 3, u, v, np.ones(3, np.uint32)), min_samples=1)
    assert ei.value.code == _native.GHS_E_NONCANON


# ---- rank-mapped float weights ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_rank_mapped_floats_report_the_callers_values(torch_cuda, dtype):
    from distributed_ghs_implementation_amd.device import DeviceEdges, mutual_reachability
    rng = np.random.default_rng(21)
    n, t, k = 400, 3000, 4
    a, b = rng.integers(0, n - 5, t), rng.integers(0, n - 5, t)                # five isolated vertices
    wf = np.round(rng.random(t) * 50 - 10, 1).astype(dtype)                    # ties, negative values
    e = DeviceEdges.from_raw(n, a, b, wf, rank_weights=True)
    g = e.to_host()
    assert g.weights is not None and g.weights.dtype == dtype
    rc, rw, deg = ref_mreach(n, g.u, g.v, g.weights, k)
    assert (deg == 0).sum() >= 5
    mr = mutual_reachability(e, min_samples=k, short_rows="clamp")
    assert mr.edges.weights.dtype == e.weights.dtype
    assert np.array_equal(mr.edges.weights.cpu().numpy(), rw)
    assert np.array_equal(mr.core_values().cpu().numpy(), rc)
    # the new ranks are the ranks of the new values
    assert np.array_equal(u32(mr.edges.w), np.searchsorted(np.unique(wf), rw).astype(np.uint32))   # ranks among all raw weights
    assert np.array_equal(g.weights, e.weights.cpu().numpy())                  # the input is untouched


# ---- scikit-learn ---------------------------------------------------------------------------------------------------
def test_against_scikit_learn_on_every_edge(torch_cuda):
    reach = pytest.importorskip("sklearn.cluster._hdbscan._reachability")
    import scipy.sparse as sp
    rng = np.random.default_rng(7)
    n, k = 300, 5
    # a ring of +-5 neighbours (degree >= 10) plus random edges: no short rows, so scikit-learn drops nothing
    ring = np.arange(n)
    a = np.concatenate([np.tile(ring, 5), rng.integers(0, n, 1500)])
    b = np.concatenate([(ring[None, :] + np.arange(1, 6)[:, None]).ravel() % n, rng.integers(0, n, 1500)])
    u, v, w = canonical(n, a, b, rng.integers(1, 50, len(a)).astype(np.uint32))
    m = len(u)
    deg = np.bincount(np.concatenate([u, v]), minlength=n)
    assert deg.min() >= 10 >= k and m >= 2500
    wf = w.astype(np.float64)
    A = sp.csr_matrix((np.concatenate([wf, wf]), (np.concatenate([u, v]), np.concatenate([v, u]))), shape=(n, n))
    R = reach.mutual_reachability_graph(A.copy(), min_samples=k).tocsr()
    assert R.nnz == 2 * m                                        # every edge is there, in both directions
    theirs = np.asarray(R[u.astype(np.int64), v.astype(np.int64)]).ravel()
    assert np.array_equal(theirs, np.asarray(R[v.astype(np.int64), u.astype(np.int64)]).ravel())
    core, w_out, info = run(torch_cuda, n, u, v, w, k, short_rows="error")
    assert info["short_rows"] == 0
    assert np.array_equal(w_out.astype(np.float64), theirs)      # no edge left out
    assert np.array_equal(w_out, ref_mreach(n, u, v, w, k)[1])


# ---- end to end ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def knn_like_graph():
    rng = np.random.default_rng(33)
    n = 600
    ring = np.arange(n)
    a = np.concatenate([np.tile(ring, 4), rng.integers(0, n, 2500)])
    b = np.concatenate([(ring[None, :] + np.arange(1, 5)[:, None]).ravel() % n, rng.integers(0, n, 2500)])
    return (n,) + canonical(n, a, b, rng.integers(1, 40, len(a)).astype(np.uint32))


def test_hdbscan_equals_the_four_calls_and_scipy(torch_cuda):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components, minimum_spanning_tree

    from distributed_ghs_implementation_amd.device import DeviceMST, forest_labels, hdbscan, mutual_reachability
    n, u, v, w = knn_like_graph()
    k, mcs = 4, 6
    e = dev_edges(torch_cuda, n, u, v, w)
    h = hdbscan(e, min_cluster_size=mcs, min_samples=k)
    assert np.array_equal(u32(e.w), w)                           # the input list is left as it is
    # the four calls by hand, byte for byte
    mr = mutual_reachability(e, min_samples=k)
    eng = DeviceMST(mr.edges)
    res, _ = eng.run()
    dg = eng.dendrogram()
    cl = dg.clusters(mr.edges, min_cluster_size=mcs)
    assert u32(h.reach.core).tobytes() == u32(mr.core).tobytes() and u32(h.reach.edges.w).tobytes() == u32(mr.edges.w).tobytes()
    assert h.mst.in_mst.cpu().numpy().tobytes() == eng.in_mst.cpu().numpy().tobytes()
    for name in ("leaf_parent", "merge_eid", "merge_parent", "child_a", "child_b", "size"):
        assert getattr(h.dendrogram, name).cpu().numpy().tobytes() == getattr(dg, name).cpu().numpy().tobytes(), name
    for name in ("label", "probability", "point_cluster", "point_lambda", "cluster_head", "cluster_parent", "cluster_size",
                 "cluster_birth", "cluster_stability", "cluster_selected"):
        assert getattr(h.clusters, name).cpu().numpy().tobytes() == getattr(cl, name).cpu().numpy().tobytes(), name
    assert h.labels is h.clusters.label and int(h.labels.max()) >= 0
    # the reference mutual-reachability graph
    _, rw, deg = ref_mreach(n, u, v, w, k)
    assert deg.min() >= k and np.array_equal(u32(mr.edges.w), rw)
    assert eng.verify()["ok"]                                    # THE minimum spanning forest of the new weights
    A = sp.csr_matrix((rw.astype(np.float64), (u.astype(np.int64), v.astype(np.int64))), shape=(n, n))
    assert rw.min() >= 1                                         # no explicit zeros: scipy sees every edge
    assert int(res.total_weight) == int(round(minimum_spanning_tree(A).sum()))
    for t in (int(np.percentile(rw, 20)), int(np.median(rw)), int(rw.max())):
        keep = rw <= t
        _, theirs = connected_components(sp.csr_matrix((np.ones(keep.sum()), (u[keep].astype(np.int64),
                                                                                v[keep].astype(np.int64))), shape=(n, n)),
                                         directed=False)
        ours = u32(forest_labels(mr.edges, eng.in_mst, max_weight=t)[0]).astype(np.int64)
        # the same partition: the pairs (ours, theirs) are a bijection
        pairs = np.unique(np.stack([ours, theirs]), axis=1)
        assert pairs.shape[1] == len(np.unique(ours)) == len(np.unique(theirs)), t


def test_hdbscan_edges_from_raw_arrays(torch_cuda):
    from distributed_ghs_implementation_amd import hdbscan_edges
    from distributed_ghs_implementation_amd.device import hdbscan
    n, u, v, w = knn_like_graph()
    rng = np.random.default_rng(3)
    p = rng.permutation(len(u))                                  # any order, either orientation
    flip = rng.random(len(u)) < 0.5
    ru, rv = np.where(flip, v, u)[p].astype(np.int64), np.where(flip, u, v)[p].astype(np.int64)
    out, info = hdbscan_edges(n, ru, rv, w[p].astype(np.int64), min_cluster_size=6, min_samples=4, return_info=True)
    h = hdbscan(dev_edges(torch_cuda, n, u, v, w), min_cluster_size=6, min_samples=4)
    assert np.array_equal(out["label"], h.labels.cpu().numpy()) and out["label"].dtype == np.int32
    assert np.array_equal(out["core"], ref_mreach(n, u, v, w, 4)[0].astype(np.int64))
    assert np.array_equal(out["probability"], h.clusters.probability.cpu().numpy())
    ids = out["mst_raw_ids"]
    assert len(ids) == int(h.mst.in_mst.sum()) and len(np.unique(ids)) == len(ids)
    back = {(min(a, b), max(a, b)) for a, b in zip(ru[ids].tolist(), rv[ids].tolist())}
    flags = h.mst.in_mst_host()
    assert back == set(zip(u[flags].tolist(), v[flags].tolist()))
    assert info["reach"]["short_rows"] == 0 and info["cluster"]["num_selected"] == int(out["label"].max()) + 1
    # float weights, rank-mapped on the device: the same clustering in the caller's units
    outf = hdbscan_edges(n, ru, rv, w[p].astype(np.float64) * 0.5, rank_weights=True, min_cluster_size=6, min_samples=4)
    assert outf["core"].dtype == np.float64 and np.array_equal(outf["core"], out["core"] * 0.5)
    assert np.array_equal(outf["label"], out["label"])
