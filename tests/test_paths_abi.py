"""The path-query entry points' C-ABI boundary without a GPU (ghs_forest_paths_index_bytes / _create /
_query / _destroy / _host): the results' layouts, every argument check that comes before any device
work, the index size, the n == 0 and q == 0 answers, the Python layers' ValueErrors, and the
independence of csrc/paths.hip from every other translation unit."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from distributed_ghs_implementation_amd import _native

# host addresses standing in for device pointers: every check below fails before anything is read
BASE = 1 << 20
NAMES = ("u", "v", "w", "parent", "parent_eid", "depth", "index")
GOOD = tuple(BASE + (k << 16) for k in range(len(NAMES)))
CSRC = os.path.join(ROOT, "distributed_ghs_implementation_amd", "csrc")
PATHS_HIP = os.path.join(CSRC, "paths.hip")
SYMBOLS = {"ghs_forest_paths_index_bytes", "ghs_forest_paths_create", "ghs_forest_paths_query",
           "ghs_forest_paths_destroy", "ghs_forest_paths_host"}


def _create(L, n, m, ptrs, max_depth, index_bytes, res=True, out=True):
    u, v, w, par, peid, dep, idx = ptrs
    r = _native.PathsResult()
    h = ctypes.c_void_p(0)
    rc = L.ghs_forest_paths_create(n, m, u, v, w, par, peid, dep, max_depth, idx, index_bytes, None,
                                   ctypes.byref(r) if res else None, ctypes.byref(h) if out else None)
    return rc, r, h


def _empty_handle(L):
    rc, r, h = _create(L, 0, 0, (None,) * 7, 0, 0)
    assert rc == _native.GHS_OK and h.value
    return h


def _query(L, h, q, a, b, key, lca, hops, res=True):
    r = _native.PathsQueryResult()
    rc = L.ghs_forest_paths_query(h, q, a, b, key, lca, hops, None, ctypes.byref(r) if res else None)
    return rc, r


def test_result_layouts_symbols_and_header():
    R, Q = _native.PathsResult, _native.PathsQueryResult
    assert ctypes.sizeof(R) == 48 and ctypes.sizeof(Q) == 32
    assert [f for f, _ in R._fields_] == ["levels", "max_depth", "num_trees", "index_bytes", "ms_total", "reserved"]
    assert [getattr(R, f).offset for f, _ in R._fields_] == [0, 8, 16, 24, 32, 40]
    assert [f for f, _ in Q._fields_] == ["queries", "connected", "ms_total", "reserved"]
    assert [getattr(Q, f).offset for f, _ in Q._fields_] == [0, 8, 16, 24]
    assert SYMBOLS <= set(_native.EXPORTED_SYMBOLS)
    L = _native.load()
    for s in SYMBOLS:
        assert getattr(L, s) is not None
    assert L.ghs_abi_version() == 10 and _native.ABI_VERSION == 10
    header = open(os.path.join(ROOT, "include", "ghs_mst.h")).read()
    assert re.search(r"#define\s+GHS_MST_ABI_VERSION\s+10\b", header)
    for s in SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", header), s
    assert header.index("ghs_forest_root_host(") < header.index("typedef struct ghs_paths_result")
    assert "ghs_implementation.py:235-387" in header  # the reference's convergecast walk
    assert "one query at a time per" in header        # the concurrency rule
    assert set(R().as_dict()) == {f for f, _ in R._fields_} - {"reserved"}
    assert set(Q().as_dict()) == {f for f, _ in Q._fields_} - {"reserved"}


def test_index_bytes_without_a_gpu():
    L = _native.load()
    ns = (0, 1, 2, 7, 15, 16, 17, 1023, 1024, 1025, 100000, 1 << 20, 1 << 24, (1 << 32) - 1)
    depths = (0, 1, 2, 3, 4, 7, 8, 255, 256, 65535, 65536, (1 << 31) - 1, 1 << 31, (1 << 32) - 2)

    def levels(d):
        return max(1, int(d).bit_length())
    table = [[L.ghs_forest_paths_index_bytes(n, d) for d in depths] for n in ns]
    for i, n in enumerate(ns):
        assert table[i] == sorted(table[i]), n                      # nondecreasing in K
        for j, d in enumerate(depths):
            extra = table[i][j] - 16 * levels(d) * n
            assert 256 <= extra < 512, (n, d, extra)                # 16 K n + a bounded constant (the status block)
            assert table[i][j] % 256 == 0
    for j, d in enumerate(depths):
        col = [table[i][j] for i in range(len(ns))]
        assert col == sorted(col), d                                # nondecreasing in n
    # K changes exactly at the powers of two (n = 1024: a level is a multiple of the 256-byte rounding)
    n = 1024
    for k in range(1, 20):
        below, at = L.ghs_forest_paths_index_bytes(n, (1 << k) - 1), L.ghs_forest_paths_index_bytes(n, 1 << k)
        assert at - below == 16 * n, k
    # the 4096^2 random-weight grid, 39 854 deep, K = 16: 4.3 GB
    assert L.ghs_forest_paths_index_bytes(4096 * 4096, 39854) == 16 * 16 * 4096 * 4096 + 256


def test_create_null_and_misaligned_pointers():
    L = _native.load()
    ib = L.ghs_forest_paths_index_bytes(5, 2)
    for k, name in enumerate(NAMES):
        args = list(GOOD)
        args[k] = None
        rc, _, h = _create(L, 5, 3, args, 2, ib)
        assert rc == _native.GHS_E_ARG and not h.value, name   # not GHS_E_NODEVICE: the check comes first
        assert b"NULL" in L.ghs_last_error()
    assert _create(L, 5, 3, GOOD, 2, ib, res=False)[0] == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error()
    assert _create(L, 5, 3, GOOD, 2, ib, out=False)[0] == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error()
    for k in (0, 1, 2, 6):  # u, v, w, index: 16 bytes
        for off in (1, 4, 8, 12):
            args = list(GOOD)
            args[k] += off
            rc, _, _ = _create(L, 5, 3, args, 2, ib)
            assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), (k, off)
    for k in (3, 4, 5):  # parent, parent_eid, depth: 4 bytes; a 4-byte offset passes on to the next check
        for off in (1, 2, 3):
            args = list(GOOD)
            args[k] += off
            rc, _, _ = _create(L, 5, 3, args, 2, ib)
            assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), (k, off)
        args = list(GOOD)
        args[k] += 4
        assert _create(L, 5, 3, args, 2, 0)[0] == _native.GHS_E_NOMEM
    # m == 0: the edge pointers may be NULL (the next check, a short index, answers)
    u, v, w, par, peid, dep, idx = GOOD
    assert _create(L, 5, 0, (None, None, None, par, peid, dep, idx), 0, 0)[0] == _native.GHS_E_NOMEM


def test_create_ranges_and_short_index():
    L = _native.load()
    for m in (1 << 31, 1 << 40):
        rc, _, _ = _create(L, 5, m, GOOD, 2, 1 << 50)
        assert rc == _native.GHS_E_ARG and b"2^31" in L.ghs_last_error()
    for n, d in ((5, 5), (5, 6), (1, 1), (1000, 1 << 40)):
        rc, _, _ = _create(L, n, 3, GOOD, d, 1 << 50)
        assert rc == _native.GHS_E_ARG and b"max_depth" in L.ghs_last_error(), (n, d)
    ib = L.ghs_forest_paths_index_bytes(5000, 4999)
    for short in (0, 1, ib - 1):
        assert _create(L, 5000, 20000, GOOD, 4999, short)[0] == _native.GHS_E_NOMEM, short


def test_no_vertices_and_no_queries():
    L = _native.load()
    rc, r, h = _create(L, 0, 0, (None,) * 7, 0, 0)
    assert rc == _native.GHS_OK and h.value
    assert (r.levels, r.max_depth, r.num_trees) == (0, 0, 0)
    # q == 0: GHS_OK, no device work, whatever the pointers
    rc, qr = _query(L, h, 0, None, None, None, None, None)
    assert rc == _native.GHS_OK and (qr.queries, qr.connected) == (0, 0)
    # an index over no vertices: every id is out of range
    rc, _ = _query(L, h, 3, BASE, BASE, None, None, None)
    assert rc == _native.GHS_E_ARG and b"out of range" in L.ghs_last_error()
    assert L.ghs_forest_paths_destroy(h) == _native.GHS_OK
    assert L.ghs_forest_paths_destroy(None) == _native.GHS_OK


def test_query_argument_errors():
    L = _native.load()
    h = _empty_handle(L)
    a, b, key, lca, hops = (BASE + (k << 16) for k in range(5))
    assert _query(L, None, 3, a, b, key, lca, hops)[0] == _native.GHS_E_ARG and b"handle" in L.ghs_last_error()
    assert _query(L, h, 3, a, b, key, lca, hops, res=False)[0] == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error()
    for q in (1 << 32, 1 << 40):
        assert _query(L, h, q, a, b, key, lca, hops)[0] == _native.GHS_E_ARG and b"2^32" in L.ghs_last_error()
    assert _query(L, h, 3, None, b, key, lca, hops)[0] == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error()
    assert _query(L, h, 3, a, None, key, lca, hops)[0] == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error()
    for k in (0, 1, 3, 4):  # a, b, lca, hops: 4 bytes
        for off in (1, 2, 3):
            args = [a, b, key, lca, hops]
            args[k] += off
            assert _query(L, h, 3, *args)[0] == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), (k, off)
    for off in (1, 2, 4, 6):  # key: 8 bytes
        assert _query(L, h, 3, a, b, key + off, lca, hops)[0] == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error()
    # 4-byte-offset slices of a / b / lca / hops and NULL outputs pass the pointer checks
    rc, _ = _query(L, h, 3, a + 4, b + 4, None, lca + 4, hops + 4)
    assert rc == _native.GHS_E_ARG and b"out of range" in L.ghs_last_error()
    rc, _ = _query(L, h, 3, a, b, None, None, None)
    assert rc == _native.GHS_E_ARG and b"out of range" in L.ghs_last_error()
    assert L.ghs_forest_paths_destroy(h) == _native.GHS_OK


def test_host_entry_argument_errors():
    L = _native.load()
    res = _native.PathsQueryResult()
    z = np.zeros(8, np.uint32)
    f = np.zeros(8, np.uint8)
    k8 = np.zeros(8, np.uint64)
    p, fp, kp = z.ctypes.data, f.ctypes.data, k8.ctypes.data

    def host(n, m, u, v, w, fl, q, a, b, key, lca, hops, r=res):
        return L.ghs_forest_paths_host(n, m, u, v, w, fl, q, a, b, key, lca, hops, ctypes.byref(r) if r is not None else None)
    assert host(5, 3, p, p, p, fp, 2, p, p, kp, p, p, r=None) == _native.GHS_E_ARG
    assert host(5, 1 << 31, p, p, p, fp, 2, p, p, kp, p, p) == _native.GHS_E_ARG and b"2^31" in L.ghs_last_error()
    assert host(5, 3, p, p, p, fp, 1 << 32, p, p, kp, p, p) == _native.GHS_E_ARG and b"2^32" in L.ghs_last_error()
    for k in range(4):  # u, v, w, flags
        args = [p, p, p, fp]
        args[k] = None
        assert host(5, 3, *args, 2, p, p, kp, p, p) == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error(), k
    assert host(5, 3, p, p, p, fp, 2, None, p, kp, p, p) == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error()
    assert host(5, 3, p, p, p, fp, 2, p, None, kp, p, p) == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error()
    # q == 0: GHS_OK with no device work; no vertices: every id is out of range
    assert host(5, 3, p, p, p, fp, 0, None, None, None, None, None) == _native.GHS_OK
    assert (res.queries, res.connected) == (0, 0)
    assert host(0, 0, None, None, None, None, 2, p, p, kp, p, p) == _native.GHS_E_ARG
    assert b"out of range" in L.ghs_last_error()


@pytest.mark.skipif(_native.device_count() > 0, reason="CPU-only behaviour")
def test_nodevice_only_after_the_argument_checks():
    L = _native.load()
    res = _native.PathsQueryResult()
    z = np.zeros(8, np.uint32)
    f = np.zeros(8, np.uint8)
    k8 = np.zeros(8, np.uint64)
    p, fp, kp = z.ctypes.data, f.ctypes.data, k8.ctypes.data
    # every argument is fine: only now the missing device is reported
    assert L.ghs_forest_paths_host(5, 3, p, p, p, fp, 2, p, p, kp, p, p, ctypes.byref(res)) == _native.GHS_E_NODEVICE
    assert L.ghs_forest_paths_host(5, 3, p, p, p, fp, 2, p, p, None, None, None, ctypes.byref(res)) == _native.GHS_E_NODEVICE
    # and a bad argument still wins over it
    assert L.ghs_forest_paths_host(5, 3, None, p, p, fp, 2, p, p, kp, p, p, ctypes.byref(res)) == _native.GHS_E_ARG
    ib = L.ghs_forest_paths_index_bytes(5, 2)
    assert _create(L, 5, 3, GOOD, 2, ib)[0] == _native.GHS_E_NODEVICE
    assert _create(L, 5, 3, GOOD, 2, ib - 1)[0] == _native.GHS_E_NOMEM
    from distributed_ghs_implementation_amd import canonicalize
    from distributed_ghs_implementation_amd.mst import MSTResult
    g = canonicalize(3, edges=[(0, 1, 1), (1, 2, 2)])
    with pytest.raises(_native.GHSError) as ei:
        MSTResult(g, np.ones(2, bool), 3, 1, [], 0.0).paths([0], [2])
    assert ei.value.code == _native.GHS_E_NODEVICE


def test_python_value_errors_without_a_gpu():
    import torch

    from distributed_ghs_implementation_amd import canonicalize
    from distributed_ghs_implementation_amd.device import DeviceEdges, RootedForest, forest_paths
    from distributed_ghs_implementation_amd.mst import MSTResult
    z = torch.zeros(3, dtype=torch.int32)
    flags = torch.zeros(3, dtype=torch.uint8)
    csr_only = DeviceEdges(3, None, z, z, off=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="CSR"):
        forest_paths(csr_only, flags)
    coo = DeviceEdges(3, z, z, z)
    rooted = RootedForest(z, z, z, None, None)
    with pytest.raises(ValueError):
        forest_paths(coo)                                   # neither flags nor a rooted forest
    with pytest.raises(ValueError):
        forest_paths(coo, flags, rooted=rooted, max_depth=0)  # both
    with pytest.raises(ValueError, match="max_depth"):
        forest_paths(coo, rooted=rooted)                    # a rooted forest without its depth bound
    with pytest.raises(ValueError):
        forest_paths(coo, rooted=RootedForest(z[:2], z, z, None, None), max_depth=0)  # fewer than n entries
    with pytest.raises(ValueError):
        forest_paths(coo, torch.zeros(2, dtype=torch.uint8))  # fewer flags than edges
    g = canonicalize(3, edges=[(0, 1, 1), (1, 2, 2)])
    r = MSTResult(g, np.ones(2, bool), 3, 1, [], 0.0)
    for a, b in (([0], [3]), ([-1], [0]), ([0, 1], [1]), ([0.5], [1])):
        with pytest.raises(ValueError):
            r.paths(a, b)
    out, info = r.paths(np.zeros(0, np.int64), np.zeros(0, np.int64), return_info=True)  # q == 0 needs no GPU
    assert all(len(out[k]) == 0 for k in ("eid", "weight", "lca", "hops", "connected")) and info["queries"] == 0


def test_cli_paths_needs_pairs():
    from distributed_ghs_implementation_amd.__main__ import main
    for argv in (["--paths", "out.npz"], ["--pairs", "pairs.npy"]):
        with pytest.raises(SystemExit) as ei:
            main(argv)
        assert ei.value.code == 2  # an argparse error


def test_paths_hip_stands_alone():
    """csrc/paths.hip includes no project source but common.h, launches only kernels it defines (all
    named k_pa_*), and shares no kernel name with any other file of csrc/."""
    src = open(PATHS_HIP).read()
    assert re.findall(r'^\s*#\s*include\s+"([^"]+)"', src, re.M) == ["common.h"]
    for inc in re.findall(r"^\s*#\s*include\s+<([^>]+)>", src, re.M):
        assert inc.startswith("hip/") or "/" not in inc, inc  # HIP and the C++ library
    launched = set(re.findall(r"\b(k_\w+)\s*(?:<[^<>]*>)?\s*<<<", src))
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src, re.S))
    assert launched and launched <= defined, launched - defined
    assert defined == {"k_pa_level0", "k_pa_level", "k_pa_query"}
    other = ""
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")) and name != "paths.hip":
            other += open(os.path.join(CSRC, name)).read()
    for part in sorted(os.listdir(os.path.join(CSRC, "boruvka"))):
        other += open(os.path.join(CSRC, "boruvka", part)).read()
    other_kernels = set(re.findall(r"\bvoid\s+(k_\w+)\s*\(", other))
    assert other_kernels and not (defined & other_kernels)
    assert not re.search(r"\bk_pa_\w+", other)
    # the host form lives in host.hip and goes through the public calls only
    host = open(os.path.join(CSRC, "host.hip")).read()
    assert "ghs_forest_paths_host" in host and "ghs_forest_paths_host" not in src


def test_makefile_links_paths_everywhere():
    lines = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ").split("\n")
    objs = [ln for ln in lines if re.match(r"OBJS\s*:=", ln)]
    assert len(objs) == 1 and "$(OUTDIR)/paths.o" in objs[0] and "$(OUTDIR)/root.o" in objs[0]
    prereq = [ln for ln in lines if ln.startswith("rcclstub:")]
    assert len(prereq) == 1 and "$(OUTDIR)/paths.o" in prereq[0]     # the target's prerequisites
    link = [ln for ln in lines if ln.startswith("\t") and "-o $(STUB)/libghs_mst_rcclstub.so" in ln]
    assert len(link) == 1 and "$(OUTDIR)/paths.o" in link[0]         # and its link line
