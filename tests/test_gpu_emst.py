"""device.emst, EMST.edges() and hdbscan_points(exact=True) on the GPU against references written here.

The reference shares nothing with the device code: the dense matrix of weight bits, every pair u < v sorted by
(bits(w2), u, v), union-find Kruskal. u, v and w are compared for byte equality, in both metrics and for every
slice count.
Exact cases: small-integer lattice coordinates with dim * max|a - b|^2 < 2^24, so every float32 step of the
device's chain is exact in any order and an int64 numpy matrix is the truth; integer core distances (the k-th
smallest of a row) likewise. General floats: the truth's d2 is the device's own, from device.knn(k = n - 1), a
different kernel; what is tested is the tree built on those bits. dim == 1 needs neither: float32 numpy computes
fmaf(s, s, 0) = s * s exactly as the device must."""
import functools
import math

import numpy as np
import pytest

from distributed_ghs_implementation_amd import _native

pytestmark = pytest.mark.gpu

SLICES = (0, 1, 2, 3, 64)      # 64: more slices than candidate tiles at every n below
METRICS = ("sqeuclidean", "euclidean")
NS = (2, 3, 63, 64, 65, 129, 257, 600)
DIMS = (1, 3, 4, 31, 32, 33, 70)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert _native.device_count() > 0
    return torch


# ---- the reference ------------------------------------------------------------------------------------------
def kruskal(W, reverse_ties=False):
    """W: (n, n) symmetric matrix of non-negative weights that order as the float32 bits do (uint32 bits or
    integers). The tree canonical Kruskal builds over all pairs u < v in (W, u, v) order, as (u, v, W[u, v]) in
    ascending (u, v). reverse_ties: the order (W, -u, -v) instead, to show that ties decide."""
    n = len(W)
    iu, iv = np.triu_indices(n, 1)
    w = W[iu, iv]
    order = np.lexsort((-iv, -iu, w)) if reverse_ties else np.lexsort((iv, iu, w))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    tree = []
    for e in order.tolist():
        a, b = find(int(iu[e])), find(int(iv[e]))
        if a != b:
            parent[a] = b
            tree.append(e)
            if len(tree) == n - 1:
                break
    assert len(tree) == n - 1
    tree = np.sort(np.asarray(tree, np.int64))       # triu order is ascending (u, v)
    return iu[tree].astype(np.uint32), iv[tree].astype(np.uint32), w[tree]


def with_cores(D, core):
    """max(D[i, j], core[i], core[j]) off the diagonal"""
    if core is None:
        return D
    return np.maximum(D, np.maximum(core[:, None], core[None, :]))


def kth_smallest(D, k):
    """per row, the k-th smallest entry off the diagonal (k >= 1)"""
    n = len(D)
    off = D[~np.eye(n, dtype=bool)].reshape(n, n - 1)
    return np.sort(off, axis=1)[:, min(k, n - 1) - 1]


def want_w(w2_f32, metric):
    return np.sqrt(w2_f32) if metric == "euclidean" else w2_f32      # np.sqrt on float32 is correctly rounded


@functools.lru_cache(maxsize=None)
def lattice(n, dim, seed=0):
    X = np.random.default_rng(1000 * seed + 7 * n + dim).integers(0, 12, (n, dim))
    X.setflags(write=False)
    return X


def int_d2(X):
    X = np.asarray(X, np.int64)
    D = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    assert D.max() < (1 << 24)
    return D


def run(torch, x, core2=None, metric="euclidean", slices=0):
    from distributed_ghs_implementation_amd import device
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    c = None if core2 is None else torch.from_numpy(np.ascontiguousarray(core2, np.float32)).cuda()
    t = device.emst(x, core2=c, metric=metric, slices=slices)
    return t.u.cpu().numpy().view(np.uint32), t.v.cpu().numpy().view(np.uint32), t.w.cpu().numpy(), t.info


def check(torch, x, core2, ref, slices=SLICES, metrics=METRICS):
    """ref = (u, v, w2 as float32): byte equality in both metrics and for every slice count, the result's
    fields, rounds <= ceil(log2 n), the same bytes on a second call"""
    ru, rv, rw2 = ref
    n = len(ru) + 1
    for metric in metrics:
        want = want_w(rw2, metric)
        first = None
        for s in slices:
            u, v, w, info = run(torch, x, core2, metric, s)
            assert np.array_equal(u, ru) and np.array_equal(v, rv), (metric, s, np.flatnonzero((u != ru) | (v != rv))[:4].tolist())
            assert np.array_equal(w.view(np.uint32), want.view(np.uint32)), (metric, s)
            assert info["num_edges"] == n - 1 and info["zero_edges"] == int((rw2 == 0).sum()), info
            assert 1 <= info["rounds"] <= max(1, math.ceil(math.log2(n))), info
            assert info["pairs"] == info["rounds"] * n * (n - 1) and info["query_tiles"] == -(-n // 64), info
            assert 1 <= info["slices"] <= 64 and (s == 0 or info["slices"] == s), info
            assert 1 <= info["components_after_first_round"] <= n // 2, info
            assert (info["rounds"] == 1) == (info["components_after_first_round"] == 1), info
            got = (u.tobytes(), v.tobytes(), w.tobytes())
            first = first or got
            assert got == first                                  # every slice count: identical bytes
        u, v, w, _ = run(torch, x, core2, metric, 0)
        assert (u.tobytes(), v.tobytes(), w.tobytes()) == first      # and from call to call


# ---- exact arithmetic ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n", NS)
def test_lattice_points_give_canonical_kruskals_tree(torch_cuda, n, dim):
    X = lattice(n, dim)
    D = int_d2(X)
    for k in (None, 1, 4):
        core = None if k is None else kth_smallest(D, k)
        ru, rv, rw = kruskal(with_cores(D, core))
        check(torch_cuda, np.asarray(X, np.float32), core, (ru, rv, rw.astype(np.float32)))


def test_the_lattice_has_ties_that_decide_tree_edges():
    """no GPU work: with the ties broken the other way round Kruskal picks other edges, on the plain weights and
    on the mutual-reachability ones, so the cases above do exercise the (u, v) part of the key"""
    for n, dim in ((257, 3), (600, 4), (129, 1)):
        D = int_d2(lattice(n, dim))
        for k in (None, 4):
            W = with_cores(D, None if k is None else kth_smallest(D, k))
            a, b = kruskal(W), kruskal(W, reverse_ties=True)
            assert not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])), (n, dim, k)
            assert np.array_equal(np.sort(a[2]), np.sort(b[2]))      # the same weights: the MST's multiset is unique


# ---- general floats: the tree on the device's own d2 bits -----------------------------------------------------
@pytest.mark.parametrize("n,dim", [(2, 3), (65, 5), (128, 64), (129, 33)])
def test_general_floats_against_kruskal_on_the_knn_distances(torch_cuda, n, dim):
    from distributed_ghs_implementation_amd import device
    torch = torch_cuda
    X = np.random.default_rng(n + dim).normal(size=(n, dim)).astype(np.float32) * np.float32(3.7)
    nn = device.knn(torch.from_numpy(X).cuda(), n - 1, metric="sqeuclidean")
    idx, d2 = nn.idx.cpu().numpy().view(np.uint32).astype(np.int64), nn.dist.cpu().numpy()
    B = np.zeros((n, n), np.uint32)
    B[np.arange(n)[:, None], idx] = d2.view(np.uint32)
    assert np.array_equal(B, B.T)                                # symmetric bit for bit
    for k in (None, 1, 5):
        core = None if k is None else d2[:, min(k, n - 1) - 1]    # rows are ascending: the k-th nearest
        W = with_cores(B, None if core is None else core.view(np.uint32))
        ru, rv, rb = kruskal(W)
        check(torch, X, core, (ru, rv, rb.astype(np.uint32).view(np.float32)))


# ---- special shapes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 65, 300])
def test_all_points_equal_give_the_star_at_vertex_0(torch_cuda, n):
    X = np.full((n, 5), 2.5, np.float32)
    ref = (np.zeros(n - 1, np.uint32), np.arange(1, n, dtype=np.uint32), np.zeros(n - 1, np.float32))
    check(torch_cuda, X, None, ref)
    u, v, w, info = run(torch_cuda, X)
    assert info["zero_edges"] == n - 1 and info["rounds"] == 1 and not w.any()


def test_points_on_a_line_in_shuffled_order(torch_cuda):
    """dim == 1: s * s in float32 numpy is the device's chain; the tree is the path along the line, duplicates joined
    at 0"""
    rng = np.random.default_rng(5)
    x = rng.permutation(np.repeat(np.arange(0, 700, 3), 2)[:401]).astype(np.float32)
    s = x[:, None] - x[None, :]
    D = (s * s).astype(np.float32)
    ru, rv, rb = kruskal(D.view(np.uint32))
    check(torch_cuda, x[:, None], None, (ru, rv, rb.view(np.float32)))
    assert sorted(np.unique(rb.view(np.float32)).tolist()) == [0.0, 9.0]


def test_two_far_clusters_of_duplicates(torch_cuda):
    """two points, each repeated: two stars of weight 0 and the one bridge (0, first point of the other cluster)"""
    n = 150
    side = np.random.default_rng(9).integers(0, 2, n)
    side[:2] = (1, 0)
    X = np.where(side[:, None] == 1, np.float32(1000.0), np.float32(-1000.0)) * np.ones((1, 3), np.float32)
    D = int_d2(X.astype(np.int64) // 1000) * 1000000
    ru, rv, rw = kruskal(D)
    assert int((rw > 0).sum()) == 1 and (int(ru[rw > 0][0]), int(rv[rw > 0][0])) == (0, 1)
    check(torch_cuda, X, None, (ru, rv, rw.astype(np.float32)))
    core = np.full(n, 7.0, np.float32)                           # a core above the zero distances lifts them
    ru, rv, rw = kruskal(with_cores(D, core.astype(np.int64)))
    check(torch_cuda, X, core, (ru, rv, rw.astype(np.float32)))


def test_a_d2_that_overflows_to_inf_is_an_ordinary_value(torch_cuda):
    x = np.array([3e19, -3e19, 3.0000002e19, -2.9999998e19, 1e19, 0.0, -3e19, 2e19], np.float32)
    with np.errstate(over="ignore"):
        s = x[:, None] - x[None, :]
        D = (s * s).astype(np.float32)
    assert np.isinf(D).any() and np.isfinite(D).sum() > len(x)
    ru, rv, rb = kruskal(D.view(np.uint32))
    check(torch_cuda, x[:, None], None, (ru, rv, rb.view(np.float32)))
    far = np.array([[3e19], [-3e19], [-3e19]], np.float32)       # every edge but one is +inf
    with np.errstate(over="ignore"):
        s = far[:, 0][:, None] - far[:, 0][None, :]
        D = (s * s).astype(np.float32)
    ru, rv, rb = kruskal(D.view(np.uint32))
    assert np.isinf(rb.view(np.float32)).sum() == 1
    check(torch_cuda, far, None, (ru, rv, rb.view(np.float32)))


@pytest.mark.parametrize("dim", [1, 3, 33])
def test_misaligned_row_views(torch_cuda, dim):
    """dim % 4 != 0: rows are only 4-byte aligned; a view that starts off a 16-byte boundary, and a strided one"""
    torch = torch_cuda
    n = 130
    X = lattice(n, dim, seed=3)
    D = int_d2(X)
    ru, rv, rw = kruskal(D)
    ref = (ru, rv, rw.astype(np.float32))
    flat = torch.zeros(n * dim + 3, dtype=torch.float32, device="cuda")
    for off in (1, 2, 3):
        view = flat[off:off + n * dim].view(n, dim)
        view.copy_(torch.from_numpy(np.asarray(X, np.float32)))
        assert view.data_ptr() % 16 != 0
        check(torch, view, None, ref, slices=(0, 3))
    wide = torch.zeros((n, dim + 5), dtype=torch.float32, device="cuda")
    wide[:, 2:2 + dim] = torch.from_numpy(np.asarray(X, np.float32))
    check(torch, wide[:, 2:2 + dim], None, ref, slices=(0,))
    for dtype in (torch.float16, torch.int32, torch.uint8):      # widened exactly
        check(torch, torch.from_numpy(np.asarray(X, np.int32)).cuda().to(dtype), None, ref, slices=(0,), metrics=("euclidean",))


# ---- error returns ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_coordinates_are_refused(torch_cuda, bad):
    n, dim = 200, 7
    for pos in (0, (n * dim) // 2, n * dim - 1):
        X = np.asarray(lattice(n, dim, seed=4), np.float32).copy()
        X.reshape(-1)[pos] = bad
        for s in (0, 1, 64):
            with pytest.raises(_native.GHSError, match="non-finite coordinate") as ei:
                run(torch_cuda, X, None, "euclidean", s)
            assert ei.value.code == _native.GHS_E_ARG
    u, v, w, info = run(torch_cuda, np.asarray(lattice(n, dim, seed=4), np.float32))     # the next call is fine
    assert info["num_edges"] == n - 1


@pytest.mark.parametrize("bad", [-1.0, np.nan, np.inf, -np.inf, -1e-45])
def test_bad_core_distances_are_refused(torch_cuda, bad):
    n, dim = 200, 3
    X = np.asarray(lattice(n, dim, seed=4), np.float32)
    for pos in (0, n // 2, n - 1):
        core = np.ones(n, np.float32)
        core[pos] = bad
        with pytest.raises(_native.GHSError, match="bad core distance") as ei:
            run(torch_cuda, X, core)
        assert ei.value.code == _native.GHS_E_ARG
    core = np.zeros(n, np.float32)
    core[::2] = -0.0                                             # -0.0 is zero
    a, b = run(torch_cuda, X, core), run(torch_cuda, X, None)
    assert all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3]))


def test_round_diagnostic(torch_cuda):
    """ghs_emst_rounds: the components left after every round of this thread's last call, strictly falling to 1 and at
    least halving; sweep times only when asked for"""
    import ctypes
    L = _native.load()
    X = np.asarray(lattice(600, 5, seed=2), np.float32)
    for enable in (1, 0):
        assert L.ghs_emst_rounds(enable, 0, None, None, None) == _native.GHS_OK
        info = run(torch_cuda, X)[3]
        rounds, comps, ms = ctypes.c_uint32(0), (ctypes.c_uint32 * 32)(), (ctypes.c_double * 32)()
        assert L.ghs_emst_rounds(0, 32, comps, ms, ctypes.byref(rounds)) == _native.GHS_OK
        r = rounds.value
        assert r == info["rounds"] and comps[0] == info["components_after_first_round"] and comps[r - 1] == 1
        assert all(2 * comps[k] <= (comps[k - 1] if k else 600) for k in range(r))
        assert all((ms[k] > 0) == bool(enable) for k in range(r))


def test_one_point_and_no_points(torch_cuda):
    torch = torch_cuda
    for n in (0, 1):
        u, v, w, info = run(torch, np.zeros((n, 3), np.float32))
        assert len(u) == len(v) == len(w) == 0 and info["num_edges"] == 0 and info["rounds"] == 0


# ---- EMST.edges() -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim,k", [(2, 3, None), (257, 5, 4), (600, 33, None)])
def test_edges_are_canonical_and_the_solver_flags_every_one(torch_cuda, n, dim, k):
    from distributed_ghs_implementation_amd import device
    torch = torch_cuda
    X = lattice(n, dim, seed=6)
    D = int_d2(X)
    core = None if k is None else kth_smallest(D, k).astype(np.float32)
    t = device.emst(torch.from_numpy(np.asarray(X, np.float32)).cuda(),
                    core2=None if core is None else torch.from_numpy(core).cuda())
    e = t.edges()
    assert e.n == n and e.m == n - 1 and t.edges() is e
    assert torch.equal(e.u, t.u) and torch.equal(e.v, t.v) and torch.equal(e.weights, t.w)
    assert np.array_equal(e.src.cpu().numpy().view(np.uint32), np.arange(n - 1, dtype=np.uint32))     # already canonical
    ok = _native.load().ghs_check_canonical
    import ctypes
    flag = ctypes.c_int(0)
    _native.check(ok(n, n - 1, ctypes.c_void_p(e.u.data_ptr()), ctypes.c_void_p(e.v.data_ptr()), None, ctypes.byref(flag)))
    assert flag.value == 1
    w, r = t.w.cpu().numpy(), e.w.cpu().numpy().view(np.uint32)
    assert np.array_equal(np.argsort(w, kind="stable"), np.argsort(r, kind="stable")) and len(np.unique(w)) == len(np.unique(r))
    mst = device.DeviceMST(e)
    res, _ = mst.run()
    assert res.num_mst_edges == n - 1 and mst.in_mst_host().all()
    assert mst.verify()["ok"]


# ---- hdbscan_points(exact=True) -----------------------------------------------------------------------------
def two_blobs():
    """40 + 40 distinct lattice points, the blobs 1000 apart: integer coordinates, exact in float32"""
    rng = np.random.default_rng(17)
    cells = np.stack(np.unravel_index(rng.permutation(20 ** 3)[:80], (20, 20, 20)), 1).astype(np.int64)
    cells[40:, 0] += 1000
    return cells


def test_two_far_blobs_become_one_tree(torch_cuda):
    from distributed_ghs_implementation_amd import device
    torch = torch_cuda
    Q = two_blobs()
    n, ms = len(Q), 3
    x = torch.from_numpy(Q.astype(np.float32)).cuda()
    approx = device.hdbscan_points(x, min_cluster_size=5, min_samples=ms, k=3)
    assert approx.dendrogram.info["num_trees"] >= 2 and approx.dendrogram.t < n - 1     # the k-NN forest: the case means something
    got = device.hdbscan_points(x, min_cluster_size=5, min_samples=ms, exact=True, k="ignored")
    assert got.reach is None and got.dendrogram.info["num_trees"] == 1 and got.dendrogram.t == n - 1
    assert got.emst.info["num_edges"] == n - 1 and got.emst.info["zero_edges"] == 0
    # the dense definition in exact integers: core2 = the (ms - 1)-th smallest off the diagonal
    D = int_d2(Q)
    core2 = kth_smallest(D, ms - 1)
    MR = with_cores(D, core2)
    gap2 = MR[:40, 40:].min()
    heights = got.dendrogram.heights(got.emst.edges()).cpu().numpy()
    assert heights.dtype == np.float32 and heights.max() == np.sqrt(np.float32(gap2)) and gap2 > 900 ** 2
    assert np.array_equal(got.core.cpu().numpy(), np.sqrt(core2.astype(np.float32)))
    ru, rv, rw = kruskal(MR)
    assert np.array_equal(got.emst.u.cpu().numpy().view(np.uint32), ru) and np.array_equal(got.emst.v.cpu().numpy().view(np.uint32), rv)
    assert np.array_equal(np.sort(heights), np.sort(np.sqrt(rw.astype(np.float32))))
    lab = got.labels.cpu().numpy()
    assert (lab >= 0).all() and len(set(lab[:40])) == 1 and len(set(lab[40:])) == 1 and lab[0] != lab[40]
    sq = device.hdbscan_points(x, min_cluster_size=5, min_samples=1, metric="sqeuclidean", exact=True)
    assert not sq.core.any() and sq.dendrogram.t == n - 1
    assert np.array_equal(sq.emst.w.cpu().numpy(), kruskal(D)[2].astype(np.float32))


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("d", [2, 16])
def test_merge_heights_against_scipy_single_linkage(torch_cuda, d, seed):
    """mr64 from the definition in float64; the sorted merge heights agree within rtol 2 * ((d + 3) * 2^-24 + 2^-24):
    the header's d2 bound halved by the square root, plus the root's rounding, with a factor 2 of margin for the
    cores entering through the same chain"""
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    from distributed_ghs_implementation_amd import device
    n, ms = 300, 5
    X = np.random.default_rng(100 * d + seed).normal(size=(n, d)).astype(np.float32)
    X64 = X.astype(np.float64)
    D = np.sqrt(((X64[:, None, :] - X64[None, :, :]) ** 2).sum(-1))
    core = np.sort(D, axis=1)[:, ms - 1]                         # the point is its own first neighbour
    mr64 = with_cores(D, core)
    np.fill_diagonal(mr64, 0.0)
    want = np.sort(hierarchy.linkage(squareform(mr64, checks=False), "single")[:, 2])
    got = device.hdbscan_points(torch_cuda.from_numpy(X).cuda(), min_cluster_size=5, min_samples=ms, exact=True)
    assert got.dendrogram.t == n - 1
    heights = np.sort(got.dendrogram.heights(got.emst.edges()).cpu().numpy().astype(np.float64))
    rtol = 2 * ((d + 3) * 2.0 ** -24 + 2.0 ** -24)
    err = np.abs(heights - want) / want
    print(f"d={d} seed={seed}: max relative height error {err.max():.3e}, bound {rtol:.3e}")
    assert (err <= rtol).all(), (err.max(), rtol)


# The blob seeds and the (min_cluster_size, min_samples) grid of test_gpu_knn.SK_CASES. scikit-learn 1.7.2's
# HDBSCAN(algorithm="brute") alone separates every one of the 18 cases into the three true blobs without noise
# (confirmed on the CPU before these assertions were written): none is dropped.
SK_DROPPED = ()


def sk_cases():
    from test_gpu_knn import SK_CASES
    return [c for c in SK_CASES if c not in SK_DROPPED]


@pytest.mark.parametrize("seed,mcs,ms", sk_cases())
def test_partition_and_noise_equal_scikit_learns_brute_hdbscan(torch_cuda, seed, mcs, ms):
    cluster = pytest.importorskip("sklearn.cluster")
    from test_gpu_knn import sk_blobs
    from distributed_ghs_implementation_amd import device
    X = sk_blobs(seed)
    truth = np.repeat(np.arange(3), 40)
    sk = cluster.HDBSCAN(min_cluster_size=mcs, min_samples=ms, algorithm="brute").fit(X.astype(np.float64)).labels_
    assert (sk >= 0).all() and len(set(zip(truth.tolist(), sk.tolist()))) == 3      # scikit-learn finds the blobs
    got = device.hdbscan_points(torch_cuda.from_numpy(X).cuda(), min_cluster_size=mcs, min_samples=ms, exact=True)
    lab = got.labels.cpu().numpy()
    assert np.array_equal(lab < 0, sk < 0)                       # the same noise set
    pairs = set(zip(sk[sk >= 0].tolist(), lab[lab >= 0].tolist()))
    assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})       # the same partition


def test_exact_equals_the_complete_knn_graph(torch_cuda):
    """n = 100, k = n - 1: the k-NN graph is complete, so the forest path computes the same tree"""
    from distributed_ghs_implementation_amd import device, hdbscan_points
    torch = torch_cuda
    rng = np.random.default_rng(3)
    X = np.concatenate([c + rng.normal(size=(n, 4)) for c, n in ((0.0, 40), (8.0, 35), (-9.0, 25))]).astype(np.float32)
    x = torch.from_numpy(X).cuda()
    a = device.hdbscan_points(x, exact=True)
    b = device.hdbscan_points(x, exact=False, k=99)
    assert torch.equal(a.labels, b.labels) and int(a.labels.max()) >= 1
    assert a.dendrogram.t == b.dendrogram.t == 99
    ha, hb = (np.sort(r.dendrogram.heights(e).cpu().numpy()) for r, e in ((a, a.emst.edges()), (b, b.reach.edges)))
    assert np.array_equal(ha, hb)
    assert np.array_equal(a.core.cpu().numpy(), b.reach.core_values().cpu().numpy())
    # the numpy layer: the same labels, the tree as rows (a, b, distance)
    out, info = hdbscan_points(X, exact=True, return_info=True)
    assert np.array_equal(out["label"], a.labels.cpu().numpy()) and set(info) == {"emst", "cluster"}
    T = out["mst_edges"]
    assert T.shape == (99, 3) and T.dtype == np.float64 and (T[:, 0] < T[:, 1]).all()
    assert np.array_equal(T[:, 2].astype(np.float32), a.emst.w.cpu().numpy()) and np.array_equal(out["core"], a.core.cpu().numpy())


def test_emst_points_on_numpy_input(torch_cuda):
    from distributed_ghs_implementation_amd.mst import emst_points
    X = lattice(257, 5, seed=6)
    D = int_d2(X)
    out, info = emst_points(np.asarray(X, np.float32), return_info=True)
    ru, rv, rw = kruskal(D)
    assert out["core"] is None and info["num_edges"] == 256
    assert np.array_equal(out["u"], ru) and np.array_equal(out["v"], rv) and np.array_equal(out["w"], np.sqrt(rw.astype(np.float32)))
    out = emst_points(np.asarray(X, np.int32), min_samples=5, metric="sqeuclidean")
    core2 = kth_smallest(D, 4)
    ru, rv, rw = kruskal(with_cores(D, core2))
    assert np.array_equal(out["u"], ru) and np.array_equal(out["v"], rv) and np.array_equal(out["w"], rw.astype(np.float32))
    assert np.array_equal(out["core"], core2.astype(np.float32))


def test_duplicates_name_the_zero_edges(torch_cuda):
    from distributed_ghs_implementation_amd import device
    X = np.repeat(np.asarray(lattice(40, 3, seed=8)), 6, axis=0).astype(np.float32)
    with pytest.raises(_native.GHSError, match="zero_edges") as ei:
        device.hdbscan_points(torch_cuda.from_numpy(X).cuda(), min_cluster_size=5, min_samples=3, exact=True)
    assert ei.value.code == _native.GHS_E_ARG
