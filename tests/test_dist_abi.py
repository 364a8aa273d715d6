"""The tree-distance entry points' C-ABI boundary without a GPU (ghs_forest_dist_workspace_bytes,
ghs_forest_wdepth_device, ghs_forest_dist_query, ghs_forest_edge_dist_device, ghs_forest_diameter_device
and the two host forms): the structs' layouts, every argument check that comes before any device work
(never GHS_E_NODEVICE on a host without a GPU), the workspace size, the q == 0 / m == 0 / n == 0
answers, the Python layer's ValueErrors and the independence of csrc/dist.hip from every other
translation unit."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from distributed_ghs_implementation_amd import _native

# host addresses standing in for device pointers: every check below fails before anything is read
BASE = 1 << 20
U, V, W, WD, A, B, DIST, LCA, WS, ROOTOF, DIAM, ENDA, ENDB, ECC = (BASE + (k << 16) for k in range(14))
CSRC = os.path.join(ROOT, "distributed_ghs_implementation_amd", "csrc")
SYMBOLS = {"ghs_forest_dist_workspace_bytes", "ghs_forest_wdepth_device", "ghs_forest_dist_query",
           "ghs_forest_edge_dist_device", "ghs_forest_diameter_device", "ghs_forest_dist_host",
           "ghs_forest_diameter_host"}
NONE = 0xFFFFFFFF
ARG, NOMEM, OK = _native.GHS_E_ARG, _native.GHS_E_NOMEM, _native.GHS_OK


@pytest.fixture()
def lib_and_handle():
    L = _native.load()
    r = _native.PathsResult()
    h = ctypes.c_void_p(0)
    rc = L.ghs_forest_paths_create(0, 0, None, None, None, None, None, None, 0, None, 0, None, ctypes.byref(r), ctypes.byref(h))
    assert rc == OK and h.value
    yield L, h
    assert L.ghs_forest_paths_destroy(h) == OK


def _wdepth(L, h, metric=0, wd=WD, ws=WS, wbytes=256):
    return L.ghs_forest_wdepth_device(h, metric, wd, ws, wbytes, None)


def _query(L, h, wd=WD, q=3, a=A, b=B, dist=DIST, lca=LCA, res=True):
    r = _native.DistQueryResult()
    return L.ghs_forest_dist_query(h, wd, q, a, b, dist, lca, ctypes.byref(r) if res else None, None), r


def _edges(L, h, wd=WD, m=3, u=U, v=V, w=W, dist=DIST, res=True):
    r = _native.EdgeDistResult()
    return L.ghs_forest_edge_dist_device(h, wd, m, u, v, w, dist, ctypes.byref(r) if res else None, None), r


def _diam(L, h, wd=WD, root_of=ROOTOF, diam=DIAM, end_a=ENDA, end_b=ENDB, ecc=ECC, ws=WS, wbytes=256, res=True):
    r = _native.DiameterResult()
    return L.ghs_forest_diameter_device(h, wd, root_of, diam, end_a, end_b, ecc, ws, wbytes,
                                        ctypes.byref(r) if res else None, None), r


def test_struct_layouts_symbols_and_header():
    Q, E, D = _native.DistQueryResult, _native.EdgeDistResult, _native.DiameterResult
    assert (ctypes.sizeof(Q), ctypes.sizeof(E), ctypes.sizeof(D)) == (48, 80, 48)
    assert [f for f, _ in Q._fields_] == ["queries", "connected", "disconnected", "max_dist", "ms_total", "reserved"]
    assert [getattr(Q, f).offset for f, _ in Q._fields_] == [0, 8, 16, 24, 32, 40]
    assert [f for f, _ in E._fields_] == ["edges", "sum_dist_lo", "sum_dist_hi", "sum_w", "max_dist", "cross_edges",
                                          "tight_edges", "max_eid", "reserved32", "ms_total", "reserved"]
    assert [getattr(E, f).offset for f, _ in E._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 72]
    assert [f for f, _ in D._fields_] == ["num_trees", "max_diameter", "min_ecc", "max_root", "center", "ms_total", "reserved"]
    assert [getattr(D, f).offset for f, _ in D._fields_] == [0, 8, 16, 24, 28, 32, 40]
    e = E(sum_dist_lo=5, sum_dist_hi=3)
    assert e.as_dict()["sum_dist"] == (3 << 64) + 5 and "sum_dist_lo" not in e.as_dict()
    assert (_native.GHS_DIST_WEIGHT, _native.GHS_DIST_HOPS) == (0, 1)
    assert SYMBOLS <= set(_native.EXPORTED_SYMBOLS)
    L = _native.load()
    for s in SYMBOLS:
        assert getattr(L, s) is not None
    assert L.ghs_abi_version() == 10 and _native.ABI_VERSION == 10  # additions only
    header = open(os.path.join(ROOT, "include", "ghs_mst.h")).read()
    assert re.search(r"#define\s+GHS_MST_ABI_VERSION\s+10\b", header)
    for s in SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", header), s
    assert re.search(r"#define\s+GHS_DIST_WEIGHT\s+0u", header) and re.search(r"#define\s+GHS_DIST_HOPS\s+1u", header)
    for name, size in (("ghs_dist_query_result", 48), ("ghs_edge_dist_result", 80), ("ghs_diameter_result", 48)):
        assert f"typedef struct {name} {{   /* {size} bytes */" in header
    assert header.index("ghs_forest_replace_host(") < header.index("typedef struct ghs_dist_query_result")
    assert "2^63" in header  # the exactness bound is stated
    nm = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    exported = {ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip()}
    assert SYMBOLS <= exported, SYMBOLS - exported


def test_workspace_bytes_without_a_gpu():
    L = _native.load()
    ns = (0, 1, 2, 31, 32, 33, 1000, 1 << 20, (1 << 32) - 1)
    depths = (0, 1, 2, 3, 4, 255, 256, 32767, 32768, 65535, 65536, (1 << 32) - 2)  # K = 1 .. 32
    table = [[L.ghs_forest_dist_workspace_bytes(n, d) for d in depths] for n in ns]
    for i, n in enumerate(ns):
        for j, d in enumerate(depths):
            assert table[i][j] % 256 == 0 and table[i][j] >= 8 * n + 256, (n, d)
            assert table[i][j] == (8 * n + 255) // 256 * 256 + 256, (n, d)
            assert i == 0 or table[i][j] >= table[i - 1][j], (n, d)   # monotone in n
            assert j == 0 or table[i][j] >= table[i][j - 1], (n, d)   # monotone in K
    assert L.ghs_forest_dist_workspace_bytes(0, 0) == 256
    assert L.ghs_forest_dist_workspace_bytes(4096 * 4096, 39854) == 8 * 4096 * 4096 + 256


def test_wdepth_argument_checks_in_order(lib_and_handle):
    L, h = lib_and_handle
    # the handle first, then the metric, then the pointers, then the workspace size
    assert _wdepth(L, None, metric=7, ws=None, wbytes=0) == ARG and b"handle" in L.ghs_last_error()
    for metric in (2, 7, NONE):
        assert _wdepth(L, h, metric=metric, ws=None, wbytes=0) == ARG and b"metric" in L.ghs_last_error()
    for metric in (_native.GHS_DIST_WEIGHT, _native.GHS_DIST_HOPS):
        assert _wdepth(L, h, metric=metric, ws=None, wbytes=0) == ARG and b"NULL" in L.ghs_last_error()
        for off in (1, 2, 4, 6):  # d_wdepth: 8 bytes
            assert _wdepth(L, h, metric=metric, wd=WD + off, wbytes=0) == ARG and b"aligned" in L.ghs_last_error(), off
        for off in (1, 4, 8, 12):  # the workspace: 16 bytes
            assert _wdepth(L, h, metric=metric, ws=WS + off, wbytes=0) == ARG and b"aligned" in L.ghs_last_error(), off
        for short in (0, 1, 255):
            assert _wdepth(L, h, metric=metric, wbytes=short) == NOMEM and b"workspace" in L.ghs_last_error()
        assert _wdepth(L, h, metric=metric, wd=WD + 8, ws=WS + 16, wbytes=255) == NOMEM
        # an index over no vertices: nothing to write
        assert _wdepth(L, h, metric=metric) == OK
        assert _wdepth(L, h, metric=metric, wd=None) == OK


def test_query_argument_checks_and_q0(lib_and_handle):
    L, h = lib_and_handle
    rc, _ = _query(L, None, res=False)
    assert rc == ARG and b"result" in L.ghs_last_error()
    rc, _ = _query(L, None)
    assert rc == ARG and b"handle" in L.ghs_last_error()
    for q in (1 << 32, 1 << 40):
        rc, _ = _query(L, h, q=q, a=None)
        assert rc == ARG and b"2^32" in L.ghs_last_error()
    for name in ("a", "b", "dist"):
        rc, _ = _query(L, h, **{name: None})
        assert rc == ARG and b"NULL" in L.ghs_last_error(), name
    for name, base in (("a", A), ("b", B), ("lca", LCA)):  # 4 bytes
        for off in (1, 2, 3):
            rc, _ = _query(L, h, **{name: base + off})
            assert rc == ARG and b"aligned" in L.ghs_last_error(), (name, off)
    for name, base in (("wd", WD), ("dist", DIST)):  # 8 bytes
        for off in (1, 2, 4, 6):
            rc, _ = _query(L, h, **{name: base + off})
            assert rc == ARG and b"aligned" in L.ghs_last_error(), (name, off)
    # q == 0: GHS_OK with no device work, whatever the pointers
    rc, r = _query(L, h, q=0, wd=None, a=None, b=None, dist=None, lca=None)
    assert rc == OK and (r.queries, r.connected, r.disconnected, r.max_dist, r.reserved) == (0, 0, 0, 0, 0)
    rc, _ = _query(L, h, q=0, a=A + 1)
    assert rc == OK
    # an index over no vertices: every id is out of range; a NULL lca is fine
    for kw in ({}, {"lca": None}, {"a": A + 4, "dist": DIST + 8}):
        rc, r = _query(L, h, **kw)
        assert rc == ARG and b"out of range" in L.ghs_last_error() and r.queries == 3, kw


def test_edge_dist_argument_checks_and_m0(lib_and_handle):
    L, h = lib_and_handle
    rc, _ = _edges(L, None, res=False)
    assert rc == ARG and b"result" in L.ghs_last_error()
    rc, _ = _edges(L, None)
    assert rc == ARG and b"handle" in L.ghs_last_error()
    for m in (1 << 31, 1 << 40):
        rc, _ = _edges(L, h, m=m, u=None)
        assert rc == ARG and b"2^31" in L.ghs_last_error()
    for name in ("u", "v", "w"):
        rc, _ = _edges(L, h, **{name: None})
        assert rc == ARG and b"NULL" in L.ghs_last_error(), name
    for name, base in (("u", U), ("v", V), ("w", W)):  # 16 bytes
        for off in (1, 4, 8, 12):
            rc, _ = _edges(L, h, **{name: base + off})
            assert rc == ARG and b"aligned" in L.ghs_last_error(), (name, off)
    for name, base in (("wd", WD), ("dist", DIST)):  # 8 bytes
        for off in (1, 2, 4, 6):
            rc, _ = _edges(L, h, **{name: base + off})
            assert rc == ARG and b"aligned" in L.ghs_last_error(), (name, off)
    rc, r = _edges(L, h, m=0, wd=None, u=None, v=None, w=None, dist=None)
    assert rc == OK
    assert (r.edges, r.sum_dist_lo, r.sum_dist_hi, r.sum_w, r.max_dist, r.cross_edges, r.tight_edges) == (0,) * 7
    assert (r.max_eid, r.reserved32, r.reserved) == (NONE, 0, 0)
    for kw in ({}, {"dist": None}):  # edges over no vertices: every endpoint is out of range
        rc, r = _edges(L, h, **kw)
        assert rc == ARG and b"out of range" in L.ghs_last_error() and r.edges == 3, kw


def test_diameter_argument_checks_and_n0(lib_and_handle):
    L, h = lib_and_handle
    rc, _ = _diam(L, None, res=False)
    assert rc == ARG and b"result" in L.ghs_last_error()
    rc, _ = _diam(L, None)
    assert rc == ARG and b"handle" in L.ghs_last_error()
    rc, _ = _diam(L, h, ws=None, wbytes=0)
    assert rc == ARG and b"NULL" in L.ghs_last_error()
    for name, base in (("root_of", ROOTOF), ("end_a", ENDA), ("end_b", ENDB)):  # 4 bytes
        for off in (1, 2, 3):
            rc, _ = _diam(L, h, wbytes=0, **{name: base + off})
            assert rc == ARG and b"aligned" in L.ghs_last_error(), (name, off)
    for name, base in (("wd", WD), ("diam", DIAM), ("ecc", ECC)):  # 8 bytes
        for off in (1, 2, 4, 6):
            rc, _ = _diam(L, h, wbytes=0, **{name: base + off})
            assert rc == ARG and b"aligned" in L.ghs_last_error(), (name, off)
    for off in (1, 4, 8, 12):  # the workspace: 16 bytes
        rc, _ = _diam(L, h, wbytes=0, ws=WS + off)
        assert rc == ARG and b"aligned" in L.ghs_last_error(), off
    for short in (0, 1, 255):
        for kw in ({}, {"ecc": None}, {"root_of": ROOTOF + 4, "diam": DIAM + 8}):
            rc, _ = _diam(L, h, wbytes=short, **kw)
            assert rc == NOMEM and b"workspace" in L.ghs_last_error(), (short, kw)
    # an index over no vertices: nothing to write, no tree
    rc, r = _diam(L, h, wd=None, root_of=None, diam=None, end_a=None, end_b=None, ecc=None)
    assert rc == OK and (r.num_trees, r.max_diameter, r.min_ecc, r.reserved) == (0, 0, 0, 0)
    assert (r.max_root, r.center) == (NONE, NONE)


def test_host_entry_argument_checks():
    L = _native.load()
    z = np.zeros(8, np.uint32)
    f = np.zeros(8, np.uint8)
    k8 = np.zeros(8, np.uint64)
    p, fp, kp = z.ctypes.data, f.ctypes.data, k8.ctypes.data

    def dist(n=5, m=3, u=p, v=p, w=p, fl=fp, metric=0, q=2, a=p, b=p, d=kp, lca=p, r=True):
        res = _native.DistQueryResult()
        return L.ghs_forest_dist_host(n, m, u, v, w, fl, metric, q, a, b, d, lca, ctypes.byref(res) if r else None), res

    def diam(n=5, m=3, u=p, v=p, w=p, fl=fp, metric=0, outs=(p, kp, p, p, kp), r=True):
        res = _native.DiameterResult()
        return L.ghs_forest_diameter_host(n, m, u, v, w, fl, metric, *outs, ctypes.byref(res) if r else None), res

    assert dist(r=False)[0] == ARG and b"result" in L.ghs_last_error()
    assert diam(r=False)[0] == ARG and b"result" in L.ghs_last_error()
    for call in (dist, diam):
        assert call(metric=2)[0] == ARG and b"metric" in L.ghs_last_error()
        assert call(m=1 << 31)[0] == ARG and b"2^31" in L.ghs_last_error()
        for name in ("u", "v", "w", "fl"):
            assert call(**{name: None})[0] == ARG and b"NULL" in L.ghs_last_error(), name
    assert dist(q=1 << 32)[0] == ARG and b"2^32" in L.ghs_last_error()
    for name in ("a", "b"):
        assert dist(**{name: None})[0] == ARG and b"NULL" in L.ghs_last_error(), name
    # q == 0 and n == 0: GHS_OK with no device work
    rc, r = dist(q=0, a=None, b=None, d=None, lca=None)
    assert rc == OK and (r.queries, r.connected, r.disconnected, r.max_dist) == (0, 0, 0, 0)
    rc, r = dist(n=0, m=0, u=None, v=None, w=None, fl=None)
    assert rc == ARG and b"out of range" in L.ghs_last_error()
    rc, r = diam(n=0, m=0, u=None, v=None, w=None, fl=None, outs=(None,) * 5)
    assert rc == OK and (r.num_trees, r.max_root, r.center) == (0, NONE, NONE)
    if _native.device_count() == 0:  # past the argument checks: there is no CPU fallback
        for metric in (0, 1):
            assert dist(metric=metric)[0] == _native.GHS_E_NODEVICE
            assert dist(metric=metric, d=None, lca=None)[0] == _native.GHS_E_NODEVICE
            assert diam(metric=metric)[0] == _native.GHS_E_NODEVICE
            assert diam(metric=metric, outs=(None,) * 5)[0] == _native.GHS_E_NODEVICE


def test_python_layer_value_errors_without_a_gpu():
    """What the Python layer refuses before any native call."""
    from distributed_ghs_implementation_amd import canonicalize
    from distributed_ghs_implementation_amd.device import (PathIndex, forest_diameters, forest_distances,
                                                           forest_edge_distances)
    from distributed_ghs_implementation_amd.mst import MSTResult
    closed = PathIndex(None, None, 4, "cpu")
    for call in (lambda: closed.wdepth(), lambda: forest_distances(closed, 0, 1), lambda: forest_diameters(closed),
                 lambda: forest_edge_distances(None, closed), lambda: forest_distances(None, 0, 1)):
        with pytest.raises(ValueError, match="closed"):
            call()
    ranked = PathIndex(ctypes.c_void_p(1), None, 4, "cpu", ranked=True)
    try:
        for call in (lambda: ranked.wdepth(), lambda: ranked.distances(0, 1), lambda: ranked.diameters()):
            with pytest.raises(ValueError, match="hops=True"):
                call()
    finally:
        ranked._h = None  # never a real handle: nothing to destroy
    g = canonicalize(3, edges=[(0, 1, 0.5), (1, 2, 0.25)])
    if g.weights is not None:  # float weights are rank-mapped
        r = MSTResult(g, np.ones(2, bool), 0, 1, [], 0.0)
        for call in (lambda: r.distances([0], [1]), lambda: r.edge_distances(), lambda: r.diameters()):
            with pytest.raises(ValueError, match="hops=True"):
                call()
    gi = canonicalize(3, edges=[(0, 1, 5), (1, 2, 7)])
    r = MSTResult(gi, np.ones(2, bool), 12, 1, [], 0.0)
    with pytest.raises(ValueError):
        r.distances([0], [3])
    with pytest.raises(ValueError):
        r.distances([0, 1], [1])
    assert r.distances(np.zeros(0, np.int64), np.zeros(0, np.int64)).tolist() == []  # q == 0: no device work


def test_dist_hip_stands_alone():
    """csrc/dist.hip includes common.h only, defines and launches only its own kernels, reaches the index
    through ghs_forest_paths_info alone; the host forms live in host.hip and launch no kernel."""
    src = open(os.path.join(CSRC, "dist.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    local = re.findall(r'#include\s+"([^"]+)"', code)
    assert local == ["common.h"], local
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", code))
    launched = set(re.findall(r"\b(k_\w+)\s*(?:<[^<>]*>)?\s*<<<", code))
    assert defined and launched <= defined, launched - defined
    assert all(k.startswith("k_ds_") for k in defined), defined
    for other in os.listdir(CSRC):
        if other.endswith((".hip", ".h")) and other != "dist.hip":
            text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, other)).read())
            assert not re.search(r"\bk_ds_\w+", text), other
    assert "ghs_forest_paths_info(" in code and "struct ghs_paths {" not in code
    assert "asm" not in code and "__builtin_amdgcn" not in code  # plain C++ stores throughout
    host = open(os.path.join(CSRC, "host.hip")).read()
    for s in ("ghs_forest_dist_host", "ghs_forest_diameter_host"):
        assert s in host and s not in src
    assert not re.search(r"\bk_\w+\s*<<<", host[host.index("Host-buffer forms of the tree distances"):])
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert makefile.count("$(OUTDIR)/dist.o") == 3  # the library and both link lines of the stub build
