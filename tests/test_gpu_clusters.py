"""HDBSCAN cluster extraction on the GPU (forest_clusters / ghs_forest_cluster_device) against a reference
written here that restates the semantics of include/ghs_mst.h with fractions.Fraction: every array and
every result field, on degenerate inputs, a chain dendrogram, block boundaries, forests, a condensed tree
as high as a caterpillar is long, a first frontier wider than one workgroup, both selection methods, the
engine's own forests, rank-mapped weights, the host and CLI layers, malformed dendrograms, and scikit-learn.

What is compared, and how:
  exactly          label, point_cluster, cluster_head, cluster_parent, cluster_size, cluster_selected,
                   num_clusters, num_selected, num_noise, num_top, cluster_height;
  bit for bit      point_lambda and cluster_birth against numpy's 1.0 / h, probability against numpy's
                   np.minimum(l, M) / M;
  cluster_stability against the exact rational value with the tolerance (rows(C) + 4) 2^-52 sum(lambda)
                   over the rows of C (its own vertices, and its child clusters as size(D) birth(D)): the
                   forward error bound of a float64 sum of that many rounded differences.
Before the GPU call every case asserts, on the CPU, that the smallest relative margin of any EOM
comparison |s - stability| / max(s, stability) in the exact reference is >= 1e-6: a condition on the
inputs (the seeds below were chosen to satisfy it), so a rounding in the last bits cannot flip a choice."""
import ctypes
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
MARGIN = 1e-6
EXACT = ("label", "point_cluster", "cluster_head", "cluster_parent", "cluster_size", "cluster_selected")
FIELDS = ("num_clusters", "num_selected", "num_noise", "num_top", "cluster_height")
DENDRO = ("leaf_parent", "merge_parent", "child_a", "child_b", "size")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from distributed_ghs_implementation_amd import _native
    assert _native.device_count() > 0
    return torch


def clog2(x):
    return max(int(x) - 1, 0).bit_length()


# ---- the dendrogram of a weighted forest: Kruskal's union-find ---------------------------------------------
def host_dendro(n, u, v, w):
    """leaf_parent, merge_parent, child_a, child_b, size (uint32) and the heights, in merge order, of the
    forest with edges (u, v) and weights w: merge j is the j-th lightest edge under (w, position)."""
    order = np.lexsort((np.arange(len(w)), np.asarray(w)))
    t = len(order)
    uf, top = list(range(n)), list(range(n))

    def find(x):
        while uf[x] != x:
            uf[x] = uf[uf[x]]
            x = uf[x]
        return x
    d = {"leaf_parent": np.full(n, NONE, np.uint32), "merge_parent": np.full(t, NONE, np.uint32),
         "child_a": np.zeros(t, np.uint32), "child_b": np.zeros(t, np.uint32), "size": np.zeros(t, np.uint32)}
    csize = [1] * n + [0] * t
    for j, e in enumerate(order.tolist()):
        ra, rb = find(int(u[e])), find(int(v[e]))
        assert ra != rb
        ca, cb = sorted((top[ra], top[rb]))
        for c in (ca, cb):
            if c < n:
                d["leaf_parent"][c] = j
            else:
                d["merge_parent"][c - n] = j
        d["child_a"][j], d["child_b"][j] = ca, cb
        csize[n + j] = csize[ca] + csize[cb]
        d["size"][j] = csize[n + j]
        uf[ra] = rb
        top[rb] = n + j
    d["height"] = np.asarray(w)[order]
    return d


# ---- the expected answer ---------------------------------------------------------------------------------------
def ref_clusters(n, d, mcs, method="eom", allow_single=False):
    """The semantics of include/ghs_mst.h, exactly: lambdas, stabilities and the EOM comparisons are
    rationals (Fraction(h) is exact for a float h too). Returns a dict of the expected arrays, the
    fields, the stabilities' tolerances and the smallest relative margin of an EOM comparison."""
    lp, mp, ca, cb, sz = (d[k].astype(np.int64) for k in DENDRO)
    t = len(mp)
    h = d["height"]
    hf = np.asarray(h, dtype=np.float64)
    lam_f = 1.0 / hf if t else np.zeros(0)
    lam_x = [1 / Fraction(x.item() if hasattr(x, "item") else x) for x in h]
    size = (lambda c: 1 if c < n else int(sz[c - n]))
    split = [size(ca[j]) >= mcs and size(cb[j]) >= mcs for j in range(t)]
    head = [bool(sz[j] >= mcs and (mp[j] == NONE or split[mp[j]])) for j in range(t)]
    heads = [j for j in range(t - 1, -1, -1) if head[j]]   # by merge index descending
    cid = {j: k for k, j in enumerate(heads)}
    K = len(heads)
    hd = [-1] * t                                          # the nearest ancestor-or-self head of a big merge
    for j in range(t - 1, -1, -1):
        if sz[j] >= mcs:
            hd[j] = j if head[j] else hd[mp[j]]
    ntop = sum(1 for j in heads if mp[j] == NONE)
    cpar = np.full(K, NONE, np.int64)
    birth_x, birth_f = [Fraction(0)] * K, np.zeros(K)
    csize = np.array([sz[j] for j in heads], np.int64).reshape(K)
    kids = [[] for _ in range(K)]
    for k, j in enumerate(heads):
        if mp[j] != NONE:
            cpar[k] = cid[hd[mp[j]]]
            birth_x[k], birth_f[k] = lam_x[mp[j]], lam_f[mp[j]]
            kids[cpar[k]].append(k)
    pc = np.full(n, NONE, np.int64)
    pl_f = np.zeros(n)
    anchor = np.full(n, -1, np.int64)
    for v in range(n):
        a = lp[v]
        while a != NONE and sz[a] < mcs:
            a = mp[a]
        if a != NONE:
            pc[v], pl_f[v], anchor[v] = cid[hd[a]], lam_f[a], a
    # stabilities: the own vertices grouped by anchor (one lambda each), then the child rows
    stab = [Fraction(0)] * K
    lamsum = [Fraction(0)] * K
    rows = [0] * K
    groups = {}
    for v in np.flatnonzero(pc != NONE):
        key = (int(pc[v]), int(anchor[v]))
        groups[key] = groups.get(key, 0) + 1
    for (k, a), cnt in groups.items():
        stab[k] += cnt * (lam_x[a] - birth_x[k])
        lamsum[k] += cnt * lam_x[a]
        rows[k] += cnt
    for k in range(K):
        for c in kids[k]:
            stab[k] += int(csize[c]) * (birth_x[c] - birth_x[k])
            lamsum[k] += int(csize[c]) * birth_x[c]
            rows[k] += 1
    tol = [(rows[k] + 4) * 2.0 ** -52 * float(lamsum[k]) for k in range(K)]
    # selection
    best, chosen, margin = list(stab), [False] * K, None
    height = [1] * K
    for k in range(K - 1, -1, -1):                         # children have larger ids
        s = sum((best[c] for c in kids[k]), Fraction(0))
        if kids[k]:
            height[k] = 1 + max(height[c] for c in kids[k])
        if cpar[k] == NONE and ntop == 1 and not allow_single:
            best[k] = s
        elif not kids[k]:
            chosen[k] = True
        elif method == "leaf":
            best[k] = s
        else:
            den = max(abs(s), abs(stab[k]))
            if den > 0:
                mg = float(abs(s - stab[k]) / den)
                margin = mg if margin is None else min(margin, mg)
            if s > stab[k]:
                best[k] = s
            else:
                chosen[k] = True
    sel_anc = [-1] * K                                     # the topmost chosen ancestor-or-self
    for k in range(K):
        up = sel_anc[cpar[k]] if cpar[k] != NONE else -1
        sel_anc[k] = up if up >= 0 else (k if chosen[k] else -1)
    selected = np.array([sel_anc[k] == k for k in range(K)], np.uint8).reshape(K)
    selid = np.cumsum(selected) - 1
    label = np.full(n, -1, np.int64)
    M = np.zeros(K)
    for k in range(K):
        if cpar[k] != NONE:
            M[cpar[k]] = max(M[cpar[k]], birth_f[k])
    for v in np.flatnonzero(pc != NONE):
        M[pc[v]] = max(M[pc[v]], pl_f[v])
        if sel_anc[pc[v]] >= 0:
            label[v] = selid[sel_anc[pc[v]]]
    prob = np.zeros(n)
    lab = np.flatnonzero(label >= 0)
    if len(lab):
        Mv = M[[sel_anc[pc[v]] for v in lab]]
        with np.errstate(invalid="ignore", divide="ignore"):
            prob[lab] = np.where(Mv == 0, 1.0, np.minimum(pl_f[lab], Mv) / Mv)
    out = {"label": label.astype(np.int32), "point_cluster": pc.astype(np.uint32), "point_lambda": pl_f,
           "probability": prob, "cluster_head": np.array(heads, np.uint32).reshape(K), "cluster_parent": cpar.astype(np.uint32),
           "cluster_size": csize.astype(np.uint32), "cluster_birth": birth_f, "cluster_selected": selected,
           "stability_exact": stab, "stability_tol": tol}
    fields = {"num_clusters": K, "num_selected": int(selected.sum()), "num_noise": int((label < 0).sum()), "num_top": ntop,
              "cluster_height": max(height) if K else 0}
    return out, fields, margin


# ---- the device side ---------------------------------------------------------------------------------------------
def _t(a, dtype=np.uint32):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.view("int32").copy() if dtype == np.uint32 else a.copy()).cuda()


def _dendrogram(n, d):
    from distributed_ghs_implementation_amd.device import Dendrogram
    t = len(d["merge_parent"])
    return Dendrogram(n, _t(d["leaf_parent"]), _t(np.zeros(t, np.uint32)), _t(d["merge_parent"]), _t(d["child_a"]),
                      _t(d["child_b"]), _t(d["size"]), info={"is_forest": True})


def _got(c):
    out = {}
    for k in EXACT + ("point_lambda", "probability", "cluster_birth", "cluster_stability"):
        a = getattr(c, k).cpu().numpy()
        out[k] = a.view(np.uint32) if a.dtype == np.int32 and k != "label" else a
    return out


def launch_bound(info):
    """select_launches <= min(H_c, ceil(K / 2048)) + 2 (include/ghs_mst.h)."""
    K = info["num_clusters"]
    return min(info["cluster_height"], -(-K // 2048)) + 2


def round_bound(t, K):
    """the fused head / anchor doubling <= ceil(log2 t) + 1, the selected ancestors <= ceil(log2 K) + 1"""
    return (clog2(t) + 1 if K or t else 0) + (clog2(K) + 1 if K else 0)


def _compare(got, info, want, fields, n, t):
    for k in EXACT:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert {k: info[k] for k in FIELDS} == fields
    for k in ("point_lambda", "cluster_birth", "probability"):
        assert got[k].dtype == np.float64 and np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), k
    for k, (x, tol) in enumerate(zip(want["stability_exact"], want["stability_tol"])):
        err = abs(Fraction(float(got["cluster_stability"][k])) - x)
        assert err <= tol, (k, float(err), tol)
    assert info["select_launches"] <= launch_bound(info), info
    assert info["rounds"] <= round_bound(t, fields["num_clusters"]), info


def _check(n, d, mcs, method="eom", allow_single=False, want=None):
    from distributed_ghs_implementation_amd.device import forest_clusters
    want, fields, margin = want if want is not None else ref_clusters(n, d, mcs, method, allow_single)
    assert margin is None or margin >= MARGIN, margin        # a condition on the inputs
    c = forest_clusters(_dendrogram(n, d), heights=np.asarray(d["height"], np.float64), min_cluster_size=mcs,
                        method=method, allow_single_cluster=allow_single)
    _compare(_got(c), c.info, want, fields, n, len(d["merge_parent"]))
    return c, want, fields


# ---- shapes --------------------------------------------------------------------------------------------------------
def random_tree(n, seed, window=6):
    """vertex i hangs under one of the `window` vertices in front of it; distinct weights 7 k + 3"""
    rng = np.random.default_rng(seed)
    u = np.array([int(rng.integers(max(0, i - window), i)) for i in range(1, n)], np.int64)
    v = np.arange(1, n, dtype=np.int64)
    w = (rng.permutation(n - 1) + 1).astype(np.int64) * 7 + 3
    return u, v, w


def blobs(count, seed, spine):
    """`count` blobs of four vertices (three light edges each, weights 1 .. 3 count, shuffled), joined by
    the count - 1 edges `spine(i)` = (blob a, blob b), the i-th of them the i-th lightest of the heavy ones."""
    rng = np.random.default_rng(seed)
    u, v = [], []
    for b in range(count):
        for k in range(1, 4):
            u.append(4 * b + int(rng.integers(0, k)))
            v.append(4 * b + k)
    w = list((rng.permutation(3 * count) + 1) * 2 + 1)
    gaps = np.cumsum(rng.integers(1, 50, count - 1)) + 8 * count
    for i in range(count - 1):
        a, b = spine(i)
        u.append(4 * a + int(rng.integers(0, 4)))
        v.append(4 * b + int(rng.integers(0, 4)))
        w.append(int(gaps[i]))
    return 4 * count, np.array(u, np.int64), np.array(v, np.int64), np.array(w, np.int64)


def balanced_spine(count):
    """joins blocks of blobs pairwise, level by level: edge i -> the first blobs of the two blocks"""
    pairs, step = [], 1
    while step < count:
        for a in range(0, count - step, 2 * step):
            pairs.append((a, a + step))
        step *= 2
    return lambda i: pairs[i]


def test_degenerate_cases(torch_cuda):
    z = np.zeros(0, np.int64)
    # t = 0: every vertex is noise
    c, _, f = _check(5, host_dendro(5, z, z, z), 2)
    assert f["num_clusters"] == 0 and c.info["num_noise"] == 5 and c.num_clusters == 0
    assert c.info["select_launches"] == 0 and c.info["rounds"] == 0
    # one edge
    one = host_dendro(2, [0], [1], [9])
    _, _, f = _check(2, one, 2)
    assert f == {"num_clusters": 1, "num_selected": 0, "num_noise": 2, "num_top": 1, "cluster_height": 1}
    _, want, f = _check(2, one, 2, allow_single=True)
    assert f["num_selected"] == 1 and list(want["label"]) == [0, 0]
    # mcs > n: all noise, K = 0
    u, v, w = random_tree(40, 1)
    _, _, f = _check(40, host_dendro(40, u, v, w), 41)
    assert f["num_clusters"] == 0 and f["num_noise"] == 40
    _, _, f = _check(40, host_dendro(40, u, v, w), 1000)       # capacity 0
    assert f["num_clusters"] == 0
    # a single tree that never splits: a star, K = 1
    star = host_dendro(30, np.zeros(29, np.int64), np.arange(1, 30), np.arange(1, 30) * 3)
    _, want, f = _check(30, star, 5)
    assert f["num_clusters"] == 1 and f["num_noise"] == 30 and f["num_selected"] == 0
    _, want, f = _check(30, star, 5, allow_single=True)
    assert f["num_selected"] == 1 and f["num_noise"] == 0 and (want["label"] == 0).all()
    _, want, f = _check(30, star, 5, method="leaf", allow_single=True)
    assert f["num_selected"] == 1 and f["num_noise"] == 0


def test_monotone_path(torch_cuda):
    """The path 0 - 1 - ... - 4999 with ascending weights: a chain dendrogram 4999 merges high; a vertex's
    anchor is mcs merges above its leaf and every big merge's head is thousands of merges up."""
    n = 5000
    d = host_dendro(n, np.arange(n - 1), np.arange(1, n), np.arange(1, n) * 2 + 1)
    for mcs in (2, 64):
        c, _, f = _check(n, d, mcs, allow_single=True)
        assert f["num_clusters"] == 1 and f["num_selected"] == 1
        assert c.info["rounds"] >= clog2(n - 1)               # nothing walked the chain


@pytest.mark.parametrize("mcs", [2, 3, 5, 64])
@pytest.mark.parametrize("n", [255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097])
def test_random_trees(n, mcs, torch_cuda):
    u, v, w = random_tree(n, n)
    _, _, f = _check(n, host_dendro(n, u, v, w), mcs)
    assert f["num_top"] == 1 and (f["num_clusters"] >= 3 or mcs == 64)


def forest_case(seed=5):
    """trees of 300, 120, 64, 9, 4, 3 and 2 vertices and three isolated vertices, ids interleaved"""
    rng = np.random.default_rng(seed)
    sizes = [300, 120, 64, 9, 4, 3, 2, 1, 1, 1]
    n = sum(sizes)
    perm = rng.permutation(n)
    us, vs, off = [], [], 0
    for k in sizes:
        for i in range(1, k):
            us.append(perm[off + int(rng.integers(max(0, i - 5), i))])
            vs.append(perm[off + i])
        off += k
    w = (rng.permutation(len(us)) + 1).astype(np.int64) * 5 + 2
    return n, np.array(us, np.int64), np.array(vs, np.int64), w


@pytest.mark.parametrize("mcs", [2, 5, 10])
def test_forest_with_small_trees_and_isolated_vertices(mcs, torch_cuda):
    n, u, v, w = forest_case()
    d = host_dendro(n, u, v, w)
    _, want, f = _check(n, d, mcs)
    assert f["num_top"] == {2: 7, 5: 4, 10: 3}[mcs] and f["num_top"] >= 2
    tops = want["cluster_parent"] == NONE
    assert (want["cluster_selected"][tops] == 1).any()         # a tree top is selectable in a forest
    assert f["num_noise"] >= 3 + (0 if mcs == 2 else 2 + 3 + 4)
    _check(n, d, mcs, allow_single=True)                       # no difference with several tops
    _check(n, d, mcs, method="leaf")


def test_caterpillar_of_blobs(torch_cuda):
    """600 blobs on a spine whose edges grow along it: the condensed tree is 600 levels high and never
    wider than 2 clusters, so one single-workgroup launch sweeps all of it."""
    n, u, v, w = blobs(600, 11, lambda i: (i, i + 1))
    c, _, f = _check(n, host_dendro(n, u, v, w), 4)
    assert f["num_clusters"] == 2 * 600 - 1 and f["cluster_height"] == 600
    assert c.info["select_launches"] == 2                      # the first frontier, then the fused sweep


def test_balanced_tree_of_blobs(torch_cuda):
    """3000 blobs joined as a balanced tree: the first frontiers (3000, 1500 leaves and finished pairs)
    are wider than one workgroup, then the single workgroup takes over."""
    n, u, v, w = blobs(3000, 12, balanced_spine(3000))
    c, _, f = _check(n, host_dendro(n, u, v, w), 4)
    assert f["num_clusters"] == 2 * 3000 - 1 and f["cluster_height"] == 13
    assert c.info["select_launches"] >= 3                      # the leaves, a wide frontier at least, the fused sweep
    _check(n, host_dendro(n, u, v, w), 4, method="leaf")


def test_leaf_against_eom(torch_cuda):
    n = 1500
    u, v, w = random_tree(n, 77)
    d = host_dendro(n, u, v, w)
    _, eom, fe = _check(n, d, 5)
    _, leaf, fl = _check(n, d, 5, method="leaf")
    assert fl["num_selected"] > fe["num_selected"]
    kids = np.bincount(leaf["cluster_parent"][leaf["cluster_parent"] != NONE].astype(np.int64), minlength=fl["num_clusters"])
    assert np.array_equal(leaf["cluster_selected"] == 1, kids == 0)
    for k in EXACT[1:5]:
        assert np.array_equal(eom[k], leaf[k]), k              # the condensed tree is the same


def test_float_heights_and_optional_probabilities(torch_cuda):
    from distributed_ghs_implementation_amd.device import forest_clusters
    n = 700
    u, v, w = random_tree(n, 21)
    d = host_dendro(n, u, v, np.sort(np.random.default_rng(2).random(n - 1) * 3 + 1e-3)[np.argsort(np.argsort(w))])
    c, want, f = _check(n, d, 4)
    c2 = forest_clusters(_dendrogram(n, d), heights=d["height"], min_cluster_size=4, probabilities=False)
    assert c2.probability is None and np.array_equal(c2.label.cpu().numpy(), want["label"])
    tree = c.condensed_tree()
    assert tree.dtype.names == ("parent", "child", "lambda_val", "child_size")
    assert len(tree) == (f["num_clusters"] - f["num_top"]) + int((want["point_cluster"] != NONE).sum())
    assert tree["parent"].min() >= n and int(tree["child_size"][tree["child"] >= n].max()) <= n


def test_two_calls_are_byte_identical(torch_cuda):
    from distributed_ghs_implementation_amd.device import forest_clusters
    n, u, v, w = blobs(3000, 12, balanced_spine(3000))
    d = host_dendro(n, u, v, w)
    dg = _dendrogram(n, d)
    runs = [_got(forest_clusters(dg, heights=d["height"].astype(np.float64), min_cluster_size=4)) for _ in range(2)]
    u2, v2, w2 = random_tree(4097, 4097)
    d2 = host_dendro(4097, u2, v2, w2)
    dg2 = _dendrogram(4097, d2)
    runs2 = [_got(forest_clusters(dg2, heights=d2["height"].astype(np.float64), min_cluster_size=2)) for _ in range(2)]
    for a, b in (runs, runs2):
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k


# ---- the engine's own forests, weights, Python layers ---------------------------------------------------------
def _from_device_dendrogram(dg, heights):
    d = {k: getattr(dg, k).cpu().numpy().view(np.uint32) for k in DENDRO}
    d["height"] = heights
    return d


def test_engine_rmat_forest(torch_cuda):
    """DeviceMST.clusters() on the engine's own MSF of R-MAT scale 10 (a forest: isolated vertices and
    small components beside the giant one), heights the uint32 weights. The generator's weights are a
    bijection of eid ^ wseed that maps 0 to 0: with wseed >= m no edge has the weight 0."""
    from distributed_ghs_implementation_amd.device import DeviceMST, generate_rmat
    e = generate_rmat(10, wseed=1 << 30)
    eng = DeviceMST(e)
    eng.run()
    dg = eng.dendrogram()
    h = dg.heights(e).cpu().numpy()
    assert h.min() > 0
    d = _from_device_dendrogram(dg, h)
    for mcs in (3, 8):
        want, fields, margin = ref_clusters(e.n, d, mcs)
        assert margin is None or margin >= MARGIN
        c = eng.clusters(min_cluster_size=mcs)
        _compare(_got(c), c.info, want, fields, e.n, dg.t)
        assert fields["num_noise"] > 0 and fields["num_clusters"] > 1


def test_zero_weight_is_an_error(torch_cuda):
    """An integer weight 0 in the forest is GHS_E_ARG, not an infinite lambda (R-MAT's edge `wseed`)."""
    from distributed_ghs_implementation_amd import _native
    from distributed_ghs_implementation_amd.device import DeviceMST, generate_rmat
    eng = DeviceMST(generate_rmat(10, wseed=2))
    eng.run()
    assert int(eng.dendrogram().heights(eng.edges).min()) == 0
    with pytest.raises(_native.GHSError) as ei:
        eng.clusters(min_cluster_size=5)
    assert ei.value.code == _native.GHS_E_ARG


def test_rank_mapped_float_weights(torch_cuda):
    """Float weights through from_raw(rank_weights=True): the heights are the caller's float64 values."""
    from distributed_ghs_implementation_amd.device import DeviceEdges, DeviceMST
    rng = np.random.default_rng(3)
    e = DeviceEdges.from_raw(300, rng.integers(0, 300, 1500), rng.integers(0, 300, 1500), rng.random(1500) + 0.25,
                             rank_weights=True)
    eng = DeviceMST(e)
    eng.run()
    dg = eng.dendrogram()
    h = dg.heights(e).cpu().numpy()
    assert h.dtype == np.float64 and h.min() >= 0.25
    want, fields, margin = ref_clusters(e.n, _from_device_dendrogram(dg, h), 5)
    assert margin is None or margin >= MARGIN
    c = dg.clusters(e, min_cluster_size=5)
    _compare(_got(c), c.info, want, fields, e.n, dg.t)


def _small_graph():
    rng = np.random.default_rng(8)
    n = 60
    pairs = sorted({(min(a, b), max(a, b)) for a, b in rng.integers(0, n, (260, 2)) if a != b})
    w = rng.permutation(len(pairs)) + 1
    return n, [(int(a), int(b), int(c)) for (a, b), c in zip(pairs, w)]


def test_host_path_mstresult_clusters(torch_cuda):
    from distributed_ghs_implementation_amd import canonicalize, minimum_spanning_forest
    n, triples = _small_graph()
    g = canonicalize(n, edges=triples)
    r = minimum_spanning_forest(g)
    dg = r.dendrogram()
    d = {k: dg[k] for k in DENDRO}
    d["height"] = dg["height"]
    for method, single in (("eom", False), ("leaf", True)):
        want, fields, margin = ref_clusters(n, d, 3, method, single)
        assert margin is None or margin >= MARGIN
        got, info = r.clusters(min_cluster_size=3, method=method, allow_single_cluster=single, return_info=True)
        _compare(got, info, want, fields, n, len(d["merge_parent"]))


def test_cli_clusters(tmp_path, torch_cuda):
    """--clusters OUT.npz --min-cluster-size K end to end, in a fresh process."""
    import shutil

    from distributed_ghs_implementation_amd import minimum_spanning_forest, read_graph_dir
    gd = tmp_path / "graph_data"
    shutil.copytree(os.path.join(GOLDEN, "graph_data_n6"), gd)
    out = tmp_path / "clusters.npz"
    p = subprocess.run([sys.executable, "-m", "distributed_ghs_implementation_amd", "--graph-dir", str(gd),
                        "--clusters", str(out), "--min-cluster-size", "2", "--allow-single-cluster"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    g = read_graph_dir(str(gd))
    dg = minimum_spanning_forest(g).dendrogram()
    d = {k: dg[k] for k in DENDRO}
    d["height"] = dg["height"]
    want, fields, margin = ref_clusters(g.n, d, 2, "eom", True)
    assert margin is None or margin >= MARGIN
    got = np.load(out)
    for k in EXACT:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["probability"], want["probability"])
    assert {k: int(got[k]) for k in FIELDS} == fields
    assert f"Clusters: {fields['num_selected']} selected of {fields['num_clusters']}" in p.stdout, p.stdout[-2000:]
    assert f"Clusters saved to: {out}" in p.stdout


# ---- malformed dendrograms ------------------------------------------------------------------------------------
def _corruptions(n, d):
    """(name, a corrupted copy) for every class of the header's validation list; d: two trees"""
    t = len(d["merge_parent"])
    tops = np.flatnonzero(d["merge_parent"] == NONE)
    assert len(tops) == 2
    inner = int(np.flatnonzero(d["child_b"] >= n)[0])           # a merge with a merge below it
    leafy = int(np.flatnonzero(d["child_a"] < n)[-1])           # a merge with a vertex below it

    def edit(key, idx, value):
        c = {k: a.copy() for k, a in d.items()}
        c["height"] = c["height"].astype(np.float64)
        c[key][idx] = value
        return c
    yield "leaf_parent >= t", edit("leaf_parent", 3, t)
    yield "leaf_parent far", edit("leaf_parent", 0, 0xFFFFFFFE)
    yield "merge_parent == j", edit("merge_parent", 5, 5)
    yield "merge_parent < j", edit("merge_parent", t - 2, 0)
    yield "merge_parent >= t", edit("merge_parent", 5, t)
    yield "child_a == child_b", edit("child_a", 7, d["child_b"][7])
    yield "child_b >= n + j", edit("child_b", 7, n + 7)
    yield "child_b far", edit("child_b", 0, 0xFFFFFFF0)
    yield "child_a > child_b", edit("child_a", inner, d["child_b"][inner] + 1)
    other = (int(d["leaf_parent"][d["child_a"][leafy]]) + 1) % t
    yield "a vertex's parent is not its merge", edit("leaf_parent", int(d["child_a"][leafy]), other)
    below = int(d["child_b"][inner]) - n
    yield "a merge's parent is not its merge", edit("merge_parent", below, t - 1 if inner != t - 1 else NONE)
    yield "size", edit("size", inner, int(d["size"][inner]) + 1)
    yield "a parent without being a child", edit("merge_parent", int(tops[0]), t - 1)
    yield "height 0", edit("height", 0, 0.0)
    yield "height < 0", edit("height", 0, -1.0)
    yield "height inf", edit("height", t - 1, np.inf)
    yield "height nan", edit("height", 4, np.nan)
    yield "heights descending", edit("height", 10, float(d["height"][9]) / 2)


def test_malformed_dendrograms_are_rejected(torch_cuda):
    """Corrupted copies of a valid dendrogram: GHS_E_ARG, no output byte written, and the next valid call
    is right."""
    import torch

    from distributed_ghs_implementation_amd import _native
    L = _native.load()
    rng = np.random.default_rng(6)                            # two trees, of 300 and 120 vertices
    us, vs, off = [], [], 0
    for k in (300, 120):
        for i in range(1, k):
            us.append(off + int(rng.integers(max(0, i - 5), i)))
            vs.append(off + i)
        off += k
    n2 = off
    d = host_dendro(n2, np.array(us), np.array(vs), (rng.permutation(len(us)) + 1) * 5 + 2)
    t = len(d["merge_parent"])
    assert t == n2 - 2
    mcs = 5
    cap = int(L.ghs_forest_cluster_capacity(n2, t, mcs))
    ws_bytes = int(L.ghs_forest_cluster_workspace_bytes(n2, t, mcs))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    outs = [torch.full((n2,), 0x5A, dtype=torch.uint8, device="cuda").repeat_interleave(8) for _ in range(4)]
    outs += [torch.full((cap * 8,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(6)]
    count = 0
    for name, bad in _corruptions(n2, d):
        ins = [_t(bad[k]) for k in DENDRO] + [_t(bad["height"], np.float64)]
        res = _native.ClusterResult()
        rc = L.ghs_forest_cluster_device(n2, t, *[ctypes.c_void_p(x.data_ptr()) for x in ins], mcs, 0,
                                         *[ctypes.c_void_p(x.data_ptr()) for x in outs], ctypes.c_void_p(ws.data_ptr()),
                                         ws_bytes, None, ctypes.byref(res))
        torch.cuda.synchronize()
        assert rc == _native.GHS_E_ARG, name
        assert b"malformed dendrogram" in L.ghs_last_error(), name
        for x in outs:
            assert bool((x == 0x5A).all()), name
        count += 1
    assert count == 18
    _check(n2, d, mcs)


# ---- scikit-learn --------------------------------------------------------------------------------------------------
def _same_partition(a, b):
    if not np.array_equal(a < 0, b < 0):
        return False
    m = {}
    for x, y in zip(a.tolist(), b.tolist()):
        if x >= 0 and m.setdefault(x, y) != y:
            return False
    return len(set(m.values())) == len(m)


def sklearn_labels(n, d, mcs):
    """tree_to_labels on the linkage of d; the tops of a forest joined at infinite distance in a comb"""
    tree = pytest.importorskip("sklearn.cluster._hdbscan._tree")
    t = len(d["merge_parent"])
    sz = d["size"].astype(np.int64)
    size = (lambda c: 1 if c < n else int(SZ[c - n]))
    CA, CB, H, SZ = list(d["child_a"]), list(d["child_b"]), list(np.asarray(d["height"], np.float64)), list(sz)
    tops = [n + j for j in range(t) if d["merge_parent"][j] == NONE] + [x for x in range(n) if d["leaf_parent"][x] == NONE]
    cur = tops[0]
    for x in tops[1:]:
        CA.append(cur)
        CB.append(x)
        H.append(np.inf)
        SZ.append(size(cur) + size(x))
        cur = n + len(H) - 1
    Z = np.zeros(len(H), dtype=tree.HIERARCHY_dtype)
    Z["left_node"], Z["right_node"], Z["value"], Z["cluster_size"] = CA, CB, H, SZ
    return tree.tree_to_labels(Z, mcs)


def sklearn_cases():
    for n, seed in ((257, 1), (1025, 2), (4097, 3)):
        u, v, w = random_tree(n, seed)
        yield n, u, v, w
    n, u, v, w = blobs(300, 4, balanced_spine(300))
    yield n, u, v, w
    # a forest whose trees all have >= mcs vertices
    rng = np.random.default_rng(9)
    us, vs, off = [], [], 0
    for k in (200, 90, 31, 12):
        for i in range(1, k):
            us.append(off + int(rng.integers(max(0, i - 5), i)))
            vs.append(off + i)
        off += k
    yield off, np.array(us), np.array(vs), (rng.permutation(len(us)) + 1) * 3 + 1


def test_cross_check_with_scikit_learn(torch_cuda):
    """The same partition up to a renaming of the labels, the same noise set, probabilities at rtol 1e-12."""
    pytest.importorskip("sklearn.cluster._hdbscan._tree")
    from distributed_ghs_implementation_amd.device import forest_clusters
    for n, u, v, w in sklearn_cases():
        d = host_dendro(n, u, v, w)
        for mcs in (2, 5, 10):
            _, _, margin = ref_clusters(n, d, mcs)
            assert margin is None or margin >= MARGIN
            lab, prob = sklearn_labels(n, d, mcs)
            c = forest_clusters(_dendrogram(n, d), heights=d["height"].astype(np.float64), min_cluster_size=mcs)
            assert _same_partition(c.label.cpu().numpy().astype(np.int64), np.asarray(lab, np.int64)), (n, mcs)
            np.testing.assert_allclose(c.probability.cpu().numpy(), prob, rtol=1e-12, atol=0)
