"""The memory contract of the eleven host-array forms (ghs_mst_host, ghs_mst_batch_host, ghs_forest_*_host,
ghs_mutual_reach_host): a call writes only the defined part of the host arrays it was given.

test_gpu_memory_contract.py checks the device entries; the host forms stage their arrays through device memory
and copy out by hand-written counts, and a wrong count writes past a caller's host array. Here every HOST
pointer of a call, the result struct included, is a view of one Arena (tests/arena.py) on a CPU tensor: exactly
as long as include/ghs_mst.h says, aligned as its element type and no more, 64 KiB of red zone on both sides.
Graphs and expected values are those of tests/contract_cases.py. Every case runs under both fills, once with
every optional output present and once with every optional output NULL, and after each call:
  (a) no red-zone byte changed;
  (b) every input view is byte-identical (w under the in-place form of ghs_mutual_reach_host excepted);
  (c) the defined part of every output equals the CPU reference, and so does the result struct without ms_*;
  (d) the bytes of an output view past its defined part still hold the fill (the per-merge arrays past
      flagged_edges, the per-cluster arrays past num_clusters, the round stats past num_stats, everything but
      leaf_parent of a dendrogram with is_forest = 0);
  (e) the mandatory outputs and the result are the same with and without the optional outputs;
  (f) q == 0, num_graphs == 0 and the empty graph G0 (for the clusters: t == 0) return GHS_OK and change
      nothing but what the header defines;
  (g) flags that close a cycle: GHS_E_ARG "flags are not a forest" from the paths, replace, dist and diameter
      forms, and no output view is written.
One call per run; nothing about timing is asserted, and no number here comes from the code under test."""
import ctypes

import numpy as np
import pytest

import contract_cases as C
from arena import FILLS, Arena

pytestmark = pytest.mark.gpu

CAPACITY = 4 << 20      # the largest case (G4: 3 x 4 m + m bytes, m <= 70000) and its red zones: under 2 MiB
FOREST_GRAPHS = ("G0", "G1", "G1w", "G2")
u32, u64, f64 = np.uint32, np.uint64, np.float64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert C.native().device_count() > 0
    return torch


class Host:
    """the host pointers of one call"""

    def __init__(self, torch, fill):
        self.A = Arena(torch, "cpu", fill, CAPACITY)
        self.inputs, self.outputs = [], {}
        self.snap = None

    def p(self, name):
        return ctypes.c_void_p(self.A.ptr(name))

    def inp(self, name, array):
        a = np.ascontiguousarray(array)
        self.A.put(name, a, a.dtype.alignment)
        self.inputs.append(name)
        return self.p(name)

    def edges(self, g, names="uvw"):
        return [self.inp(k, getattr(g, k)) for k in names]

    def out(self, name, count, dtype, wanted=True):
        """an output of `count` elements; not wanted: the optional output is NULL"""
        if not wanted:
            return None
        dt = np.dtype(dtype)
        self.A.take(count * dt.itemsize, dt.alignment, name)
        self.outputs[name] = dt
        return self.p(name)

    def struct(self, name, cls, count=1):
        self.A.take(count * ctypes.sizeof(cls), ctypes.alignment(cls), name)
        self.outputs[name] = np.dtype(np.uint8)
        return ctypes.cast(self.p(name), ctypes.POINTER(cls))

    def call(self, fn, *args):
        self.snap = self.A.snapshot()
        return fn(*args)

    def read(self, name, count=None):
        return self.A.read(name, self.outputs[name], count)

    def result(self, cls, name="result"):
        return C.fields(cls.from_buffer_copy(self.A.read(name).tobytes()))

    def outside(self, allowed):
        """the offsets of the bytes the call changed outside the views in `allowed`"""
        changed = self.A.buf != self.snap
        for name in allowed:
            off, nb = self.A.views[name]
            changed[off:off + nb] = False
        return self.where(changed.nonzero().reshape(-1).tolist())

    def where(self, offsets):
        """for messages: the views the offsets lie in, and "red zone" for those in none"""
        names = set()
        for o in offsets[:64]:
            inside = [k for k, (off, nb) in self.A.views.items() if off <= o < off + nb]
            names.add(inside[0] if inside else "red zone near " + self.A.nearest(o)[0])
        return sorted(names)


class Run:
    """what a form's call left: its code, the defined outputs, the reference, and per output view the number
    of defined elements (a view not named is defined as a whole)"""

    def __init__(self, rc, got, want, defined=(), optional=()):
        self.rc, self.got, self.want, self.defined, self.optional = rc, got, want, dict(defined), set(optional)


def host_contract(torch, form, *args, optional=True, rc_want=None, same_result=None):
    """optional: the form has optional outputs, so (e) applies. same_result: the result fields that (e)
    compares (default: all)."""
    N = C.native()
    for fill in FILLS:
        runs = []
        for opt in ((True, False) if optional else (True,)):
            h = Host(torch, fill)
            r = form(h, opt, *args)
            what = (form.__name__, hex(fill), "all outputs" if opt else "optional outputs NULL")
            assert r.rc == (N.GHS_OK if rc_want is None else rc_want), (what, r.rc, C.lib().ghs_last_error())
            bad = h.A.check()
            assert not bad, ("(a) red zone", what, h.A.describe(bad))
            changed = [k for k in h.inputs if not h.A.unchanged(h.snap, k)]
            assert not changed, ("(b) inputs changed", what, changed)
            C.assert_matches(r.got, r.want, ("(c)", what))
            for name, dt in h.outputs.items():
                off, nb = h.A.views[name]
                d = r.defined.get(name, nb // dt.itemsize) * dt.itemsize
                assert d <= nb, (what, name, d, nb)
                assert torch.equal(h.A.buf[off + d:off + nb], h.A.pristine[off + d:off + nb]), \
                    ("(d) written past the defined part", what, name, d, nb)
            runs.append(r)
        if optional:
            a, b = (C.frozen({k: x for k, x in r.got.items() if k not in r.optional}) for r in runs)
            assert runs[1].optional.isdisjoint(runs[1].got), runs[1].got.keys()
            if same_result is not None:
                a["result"], b["result"] = ({k: x["result"][k] for k in same_result} for x in (a, b))
            assert a.keys() == b.keys()
            for k in a:
                assert a[k] == b[k], ("(e) differs without the optional outputs", form.__name__, hex(fill), k)


def refused(torch, form, *args):
    """(g): GHS_E_ARG "flags are not a forest", and nothing but the result struct is written"""
    N = C.native()
    for fill in FILLS:
        for opt in (True, False):
            h = Host(torch, fill)
            rc = form(h, opt, *args, cycle=True)
            assert rc == N.GHS_E_ARG, (form.__name__, rc)
            assert b"flags are not a forest" in C.lib().ghs_last_error(), C.lib().ghs_last_error()
            bad = h.outside(["result"])
            assert not bad, ("(g) the refused call wrote", form.__name__, hex(fill), bad)


def untouched(torch, form, *args):
    """(f): GHS_OK, a result struct of zeros, and nothing else written"""
    N = C.native()
    for fill in FILLS:
        for opt in (True, False):
            h = Host(torch, fill)
            rc = form(h, opt, *args, q0=True)
            assert rc == N.GHS_OK, (form.__name__, rc, C.lib().ghs_last_error())
            bad = h.outside(["result"] if "result" in h.A.views else [])
            assert not bad, ("(f) the empty call wrote", form.__name__, hex(fill), bad)
            if "result" in h.A.views:
                assert not h.A.read("result").any(), (form.__name__, "result is not zero")


def flags_of(g, which):
    return C.flag_vector(g, which)


# ---- the solver and the batch ---------------------------------------------------------------------------------
def form_mst(h, opt, g):
    L, N = C.lib(), C.native()
    pu, pv, pw = h.edges(g)
    f = h.out("in_mst", g.m, np.uint8)
    res = h.struct("result", N.Result)
    stats = h.struct("stats", N.RoundStats, N.GHS_MAX_ROUND_STATS) if opt else None
    rc = h.call(L.ghs_mst_host, g.n, g.m, pu, pv, pw, f, res, stats)
    r = h.result(N.Result)
    got = {"in_mst": h.read("in_mst"), "result": r}
    want = {"in_mst": g.flags, "result": {"num_mst_edges": g.kruskal[2], "total_weight": g.kruskal[1]}}
    return Run(rc, got, want, {"stats": r["num_stats"] * ctypes.sizeof(N.RoundStats)})


@pytest.mark.parametrize("g", ("G0", "G1", "G1w", "G2", "G3", "G4"))
def test_mst_host(torch_cuda, g):
    host_contract(torch_cuda, form_mst, C.graph(g))


def form_batch(h, opt, q0=False):
    L, N = C.lib(), C.native()
    nvert, eoff, (u, v, w), want_flags, want_res, bad = C.batch()
    if q0:
        nvert, eoff, u, v, w = nvert[:0], eoff[:1], u[:0], v[:0], w[:0]
    B, M = len(nvert), int(eoff[-1])
    ins = [h.inp(k, x) for k, x in (("nvert", nvert), ("eoff", eoff), ("u", u), ("v", v), ("w", w))]
    f = h.out("in_mst", M, np.uint8)
    res = h.out("results", B, np.dtype(N.BATCH_RESULT_DTYPE, align=True))
    rc = h.call(L.ghs_mst_batch_host, B, *ins, f, res)
    if q0:
        return rc
    got_res = h.read("results")
    ok = np.array([r is not None for r in want_res])
    got = {"in_mst": h.read("in_mst"), "status": got_res["status"].copy(),
           "totals": [(int(r["total_weight"]), int(r["num_mst_edges"])) for r in got_res[ok]]}
    want = {"in_mst": want_flags, "status": np.where(ok, 0, 1).astype(u32), "totals": [r for r in want_res if r]}
    return Run(rc, got, want)


def test_mst_batch_host(torch_cuda):
    """the batch holds one graph that is not canonical: its neighbours are solved, the call says which one"""
    host_contract(torch_cuda, form_batch, optional=False, rc_want=C.native().GHS_E_NONCANON)
    assert b"batch graph 11" in C.lib().ghs_last_error()


def test_mst_batch_host_no_graphs(torch_cuda):
    untouched(torch_cuda, form_batch)


# ---- labels and the rooted forest -----------------------------------------------------------------------------
def form_labels(h, opt, g, which, kind):
    L, N = C.lib(), C.native()
    cut = C.label_cut(g, kind)
    mode = {"none": N.GHS_CUT_NONE, "max_weight": N.GHS_CUT_WEIGHT, "num_clusters": N.GHS_CUT_COUNT}[kind]
    param = cut[0][1] if cut else (g.n + 7 if kind == "num_clusters" else 0)
    ins = h.edges(g) + [h.inp("in_mst", flags_of(g, which))]
    lab = h.out("labels", g.n, u32)
    res = h.struct("result", N.LabelsResult)
    rc = h.call(L.ghs_forest_labels_host, g.n, g.m, *ins, mode, param, lab, res)
    want_lab, info = C.labels_want(g.name, which, cut)
    return Run(rc, {"labels": h.read("labels"), "result": h.result(N.LabelsResult)}, {"labels": want_lab, "result": info})


@pytest.mark.parametrize("kind", ["none", "max_weight", "num_clusters"])
@pytest.mark.parametrize("g,which", [(g, "msf") for g in FOREST_GRAPHS + ("G3",)] + [("G1", "cycle")])
def test_forest_labels_host(torch_cuda, g, which, kind):
    host_contract(torch_cuda, form_labels, C.graph(g), which, kind, optional=False)


def form_root(h, opt, g, which):
    L, N = C.lib(), C.native()
    ins = h.edges(g, "uv") + [h.inp("in_mst", flags_of(g, which))]
    names = ("parent", "parent_eid", "depth", "pre", "size")
    outs = [h.out(k, g.n, u32, wanted=opt or k not in ("pre", "size")) for k in names]
    res = h.struct("result", N.RootResult)
    rc = h.call(L.ghs_forest_root_host, g.n, g.m, *ins, *outs, res)
    r = h.result(N.RootResult)
    if which == "cycle":      # a result, not an error: only these two fields are specified
        f = {k: r[k] for k in ("flagged_edges", "is_forest")}
        return Run(rc, {"result": f}, {"result": {"flagged_edges": int(g.cycle_flags.sum()), "is_forest": 0}})
    arrays, info = C.root_want(g.name)
    got = {k: h.read(k) for k in names if k in h.outputs}
    got["result"] = r
    want = {k: arrays[k] for k in names if k in h.outputs}
    want["result"] = info
    return Run(rc, got, want, optional=("pre", "size"))


@pytest.mark.parametrize("g,which", [(g, "msf") for g in FOREST_GRAPHS + ("G3",)] + [("G1", "cycle")])
def test_forest_root_host(torch_cuda, g, which):
    host_contract(torch_cuda, form_root, C.graph(g), which)


# ---- the forms that root the flags themselves -----------------------------------------------------------------
def rooted_inputs(h, g, cycle):
    return h.edges(g) + [h.inp("in_mst", g.cycle_flags if cycle else g.flags)]


def pair_inputs(h, a, b, q0):
    if q0:
        a, b = a[:0], b[:0]
    return len(a), h.inp("a", a), h.inp("b", b)


def form_paths(h, opt, g, cycle=False, q0=False):
    L, N = C.lib(), C.native()
    ins = rooted_inputs(h, g, cycle)
    q, pa, pb = pair_inputs(h, *g.pairs(), q0)
    outs = [h.out(k, q, dt, wanted=opt) for k, dt in (("key", u64), ("lca", u32), ("hops", u32))]
    res = h.struct("result", N.PathsQueryResult)
    rc = h.call(L.ghs_forest_paths_host, g.n, g.m, *ins, q, pa, pb, *outs, res)
    if cycle or q0:
        return rc
    key, lca, hops = C.paths_want(g.name)
    got = {"result": h.result(N.PathsQueryResult)}
    want = {"result": {"queries": q, "connected": int((lca != C.NONE).sum())}}
    if opt:
        got.update(key=h.read("key"), lca=h.read("lca"), hops=h.read("hops"))
        want.update(key=key, lca=lca, hops=hops)
    return Run(rc, got, want, optional=("key", "lca", "hops"))


def form_replace(h, opt, g, cycle=False):
    L, N = C.lib(), C.native()
    ins = rooted_inputs(h, g, cycle)
    outs = [h.out("repl", g.n, u64, wanted=opt), h.out("repl_eid_by_edge", g.m, u32, wanted=opt)]
    res = h.struct("result", N.ReplaceResult)
    rc = h.call(L.ghs_forest_replace_host, g.n, g.m, *ins, *outs, res)
    if cycle:
        return rc
    repl, eid_by_edge, counts = C.replace_want(g.name)
    got, want = {"result": h.result(N.ReplaceResult)}, {"result": counts}
    if opt:
        got.update(repl=h.read("repl"), repl_eid_by_edge=h.read("repl_eid_by_edge"))
        want.update(repl=repl, repl_eid_by_edge=eid_by_edge)
    return Run(rc, got, want, optional=("repl", "repl_eid_by_edge"))


def form_dist(h, opt, g, hops, cycle=False, q0=False):
    L, N = C.lib(), C.native()
    ins = rooted_inputs(h, g, cycle)
    q, pa, pb = pair_inputs(h, *g.pairs(1), q0)
    outs = [h.out("dist", q, u64, wanted=opt), h.out("lca", q, u32, wanted=opt)]
    res = h.struct("result", N.DistQueryResult)
    rc = h.call(L.ghs_forest_dist_host, g.n, g.m, *ins, N.GHS_DIST_HOPS if hops else N.GHS_DIST_WEIGHT, q, pa, pb, *outs,
                res)
    if cycle or q0:
        return rc
    dist, lca = C.dist_query_want(g.name, hops)
    conn = dist != C.U64_MAX
    got = {"result": h.result(N.DistQueryResult)}
    want = {"result": {"queries": q, "connected": int(conn.sum()), "disconnected": int((~conn).sum()),
                       "max_dist": int(dist[conn].max()) if conn.any() else 0}}
    if opt:
        got.update(dist=h.read("dist"), lca=h.read("lca"))
        want.update(dist=dist, lca=lca)
    return Run(rc, got, want, optional=("dist", "lca"))


DIAMETER_ARRAYS = (("root_of", u32), ("diam", u64), ("end_a", u32), ("end_b", u32), ("ecc", u64))


def form_diameter(h, opt, g, hops, cycle=False):
    L, N = C.lib(), C.native()
    ins = rooted_inputs(h, g, cycle)
    outs = [h.out(k, g.n, dt, wanted=opt) for k, dt in DIAMETER_ARRAYS]
    res = h.struct("result", N.DiameterResult)
    rc = h.call(L.ghs_forest_diameter_host, g.n, g.m, *ins, N.GHS_DIST_HOPS if hops else N.GHS_DIST_WEIGHT, *outs, res)
    if cycle:
        return rc
    arrays, want_res = C.diameter_want(g.name, hops)
    got, want = {"result": h.result(N.DiameterResult)}, {"result": want_res}
    if opt:
        got.update({k: h.read(k) for k, _ in DIAMETER_ARRAYS})
        want.update({k: arrays[k] for k, _ in DIAMETER_ARRAYS})
    return Run(rc, got, want, optional=[k for k, _ in DIAMETER_ARRAYS])


@pytest.mark.parametrize("g", FOREST_GRAPHS)
def test_forest_paths_host(torch_cuda, g):
    host_contract(torch_cuda, form_paths, C.graph(g))


@pytest.mark.parametrize("g", FOREST_GRAPHS)
def test_forest_replace_host(torch_cuda, g):
    host_contract(torch_cuda, form_replace, C.graph(g))


@pytest.mark.parametrize("hops", [False, True])
@pytest.mark.parametrize("g", FOREST_GRAPHS)
def test_forest_dist_host(torch_cuda, g, hops):
    host_contract(torch_cuda, form_dist, C.graph(g), hops)


@pytest.mark.parametrize("hops", [False, True])
@pytest.mark.parametrize("g", FOREST_GRAPHS)
def test_forest_diameter_host(torch_cuda, g, hops):
    host_contract(torch_cuda, form_diameter, C.graph(g), hops)


@pytest.mark.parametrize("form,args", [(form_paths, ()), (form_replace, ()), (form_dist, (False,)), (form_diameter, (True,))],
                         ids=["paths", "replace", "dist", "diameter"])
@pytest.mark.parametrize("g", ("G1", "G1w"))
def test_cycle_is_refused(torch_cuda, g, form, args):
    refused(torch_cuda, form, C.graph(g), *args)


@pytest.mark.parametrize("form,args", [(form_paths, ()), (form_dist, (False,))], ids=["paths", "dist"])
@pytest.mark.parametrize("g", ("G0", "G1"))
def test_no_queries(torch_cuda, g, form, args):
    untouched(torch_cuda, form, C.graph(g), *args)


# ---- dendrogram, clusters, mutual reachability ----------------------------------------------------------------
def form_dendro(h, opt, g, which):
    L, N = C.lib(), C.native()
    cap = min(g.m, g.n - 1)
    ins = h.edges(g) + [h.inp("in_mst", flags_of(g, which))]
    names = ("merge_eid", "merge_parent", "child_a", "child_b", "size")
    optional = names[2:]
    leaf = h.out("leaf_parent", g.n, u32)
    outs = [h.out(k, cap, u32, wanted=opt or k not in optional) for k in names]
    res = h.struct("result", N.DendroResult)
    rc = h.call(L.ghs_forest_dendro_host, g.n, g.m, *ins, leaf, *outs, res)
    r = h.result(N.DendroResult)
    here = [k for k in names if k in h.outputs]
    if which == "cycle":      # a result, not an error: leaf_parent is unspecified, nothing else is copied out
        f = {k: r[k] for k in ("flagged_edges", "is_forest")}
        return Run(rc, {"result": f}, {"result": {"flagged_edges": int(g.cycle_flags.sum()), "is_forest": 0}},
                   {k: 0 for k in here})
    arrays, info = C.dendro_want(g.name)
    t = info["flagged_edges"]
    assert t <= cap
    got = {k: h.read(k, t) for k in here}
    got.update(leaf_parent=h.read("leaf_parent"), result=r)
    want = {k: arrays[k] for k in here}
    want.update(leaf_parent=arrays["leaf_parent"], result=info)
    return Run(rc, got, want, {k: t for k in here}, optional)


@pytest.mark.parametrize("g,which", [(g, "msf") for g in FOREST_GRAPHS] + [("G1", "cycle"), ("G1w", "cycle")])
def test_forest_dendro_host(torch_cuda, g, which):
    host_contract(torch_cuda, form_dendro, C.graph(g), which)


def form_cluster(h, opt, g, method):
    """t == 0 (G0): the six inputs are NULL, as the header allows"""
    L, N = C.lib(), C.native()
    d = g.forest_dendrogram
    n, t = g.n, len(d["merge_parent"])
    cap = int(L.ghs_forest_cluster_capacity(n, t, C.MCS))
    ins = [h.inp(k, d[k]) if t else None for k in ("leaf_parent", "merge_parent", "child_a", "child_b", "size", "height")]
    per_vertex = (("label", np.int32), ("probability", f64), ("point_cluster", u32), ("point_lambda", f64))
    per_cluster = (("cluster_head", u32), ("cluster_parent", u32), ("cluster_size", u32), ("cluster_birth", f64),
                   ("cluster_stability", f64), ("cluster_selected", np.uint8))
    optional = ("probability", "point_lambda")
    outs = [h.out(k, n, dt, wanted=opt or k not in optional) for k, dt in per_vertex]
    outs += [h.out(k, cap, dt) for k, dt in per_cluster]
    res = h.struct("result", N.ClusterResult)
    rc = h.call(L.ghs_forest_cluster_host, n, t, *ins, C.MCS, N.GHS_CLUSTER_LEAF if method == "leaf" else 0, *outs, res)
    r = h.result(N.ClusterResult)
    out, info = C.cluster_want(g.name, method)
    K = info["num_clusters"]
    assert K <= cap
    got = {k: h.read(k) for k, _ in per_vertex if k in h.outputs}
    got.update({k: h.read(k, K) for k, _ in per_cluster}, result=r)
    want = {k: out[k] for k in got if k not in ("result", "cluster_stability")}
    want.update(result=info, cluster_stability=(out["stability_exact"], out["stability_tol"]))
    return Run(rc, got, want, {k: K for k, _ in per_cluster}, optional)


@pytest.mark.parametrize("method", ["eom", "leaf"])
@pytest.mark.parametrize("g", FOREST_GRAPHS)
def test_forest_cluster_host(torch_cuda, g, method):
    host_contract(torch_cuda, form_cluster, C.graph(g), method)


def form_mreach(h, opt, g, inplace=False, k=3):
    """with its optional output: w_out a buffer of its own, or exactly w (in place); without: core only"""
    L, N = C.lib(), C.native()
    pu, pv, pw = h.edges(g)
    core = h.out("core", g.n, u32)
    w_out = None
    if opt and inplace:
        h.inputs.remove("w")
        h.outputs["w"] = np.dtype(u32)
        w_out = pw
    elif opt:
        w_out = h.out("w_out", g.m, u32)
    res = h.struct("result", N.MreachResult)
    rc = h.call(L.ghs_mutual_reach_host, g.n, g.m, pu, pv, pw, k, core, w_out, res)
    want_core, rw, info = C.mreach_want(g.name, k)
    info = dict(info, raised_edges=int((rw > g.w).sum()) if opt else 0)
    got, want = {"core": h.read("core"), "result": h.result(N.MreachResult)}, {"core": want_core, "result": info}
    if opt:
        got["w_out"], want["w_out"] = h.read("w" if inplace else "w_out"), rw
    return Run(rc, got, want, optional=("w_out",))


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("g", FOREST_GRAPHS + ("G3",))
def test_mutual_reach_host(torch_cuda, g, inplace):
    """raised_edges counts what w_out raised: 0 by definition without w_out, so (e) leaves it out"""
    same = [k for k, _ in C.native().MreachResult._fields_ if not k.startswith("ms_") and k != "raised_edges"]
    host_contract(torch_cuda, form_mreach, C.graph(g), inplace, same_result=same)
