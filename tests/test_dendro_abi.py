"""The dendrogram entry points' C-ABI boundary without a GPU (ghs_forest_dendro_workspace_bytes /
ghs_forest_dendro_device / ghs_forest_dendro_host): the result's layout, every argument check that
comes before any device work, the workspace size, the n == 0 answer, the Python layers' ValueErrors,
and the independence of csrc/dendro.hip from every other translation unit."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from distributed_ghs_implementation_amd import _native

# host addresses standing in for device pointers: every check below fails before anything is read
BASE = 1 << 20
NAMES = ("u", "v", "w", "flags", "leaf_parent", "merge_eid", "merge_parent", "child_a", "child_b", "size", "ws")
GOOD = tuple(BASE + (k << 16) for k in range(len(NAMES)))
OPTIONAL = ("child_a", "child_b", "size")
CSRC = os.path.join(ROOT, "distributed_ghs_implementation_amd", "csrc")
DENDRO_HIP = os.path.join(CSRC, "dendro.hip")
SYMBOLS = {"ghs_forest_dendro_workspace_bytes", "ghs_forest_dendro_device", "ghs_forest_dendro_host"}


def _call(L, n, m, ptrs, ws_bytes):
    res = _native.DendroResult()
    rc = L.ghs_forest_dendro_device(n, m, *ptrs[:10], ptrs[10], ws_bytes, None, ctypes.byref(res))
    return rc, res


def test_result_layout_symbols_and_header():
    R = _native.DendroResult
    assert ctypes.sizeof(R) == 48
    assert [f for f, _ in R._fields_] == ["flagged_edges", "num_trees", "max_height", "levels", "rounds", "is_forest",
                                          "reserved", "ms_total"]
    assert [getattr(R, f).offset for f, _ in R._fields_] == [0, 8, 16, 24, 28, 32, 36, 40]
    assert SYMBOLS <= set(_native.EXPORTED_SYMBOLS)
    L = _native.load()
    for s in SYMBOLS:
        assert getattr(L, s) is not None
    assert L.ghs_abi_version() == 10 and _native.ABI_VERSION == 10
    header = open(os.path.join(ROOT, "include", "ghs_mst.h")).read()
    assert re.search(r"#define\s+GHS_MST_ABI_VERSION\s+10\b", header)
    for s in SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", header), s
    assert header.index("ghs_forest_diameter_host(") < header.index("typedef struct ghs_dendro_result")  # after distances
    body = header[header.index("typedef struct ghs_dendro_result"): header.index("} ghs_dendro_result_t;")]
    order = [body.index(f) for f, _ in R._fields_]
    assert order == sorted(order)  # the header declares the fields in the same order
    for name in ("d_leaf_parent", "d_merge_eid", "d_merge_parent", "d_child_a", "d_child_b", "d_size"):
        assert name in header, name
    d = R().as_dict()
    assert set(d) == {f for f, _ in R._fields_} - {"reserved"} and d["is_forest"] is False


def test_workspace_bytes_without_a_gpu():
    L = _native.load()
    ns = (0, 1, 2, 7, 1023, 1024, 1025, 4095, 4096, 4097, 100000, 1 << 20, 1 << 24, (1 << 32) - 1)
    ms = (0, 1, 2, 1023, 1024, 1025, 4081, 4096, 4097, 1 << 20, 1 << 28, (1 << 31) - 1)
    table = [[L.ghs_forest_dendro_workspace_bytes(n, m) for m in ms] for n in ns]
    for i, n in enumerate(ns):
        assert table[i] == sorted(table[i]), n          # nondecreasing in m
    for j, m in enumerate(ms):
        col = [table[i][j] for i in range(len(ns))]
        assert col == sorted(col), m                    # nondecreasing in n
        for i, n in enumerate(ns):
            if m and n > 1:
                assert table[i][j] >= 28 * n, (n, m)    # a level's per-vertex scratch
    # sized by min(m, n - 1) possible merges (20 B kept at level 0 + the 16 B of the key sort), not by m
    W = L.ghs_forest_dendro_workspace_bytes
    assert W(1000, 1 << 20) >= 28 * 1000 + 36 * 999
    assert W(1000, 1 << 20) < W(1000, 999) + (1 << 16)
    assert W(1 << 20, 10) < W(1 << 20, 1 << 20)
    # the kept levels and the lifting tables stay within a constant + 2 log2(C) bytes per possible merge
    C = (1 << 24) - 1
    assert W(1 << 24, 1 << 28) < 28 * ((1 << 24) + 1) + (56 + 12 + 2 * 26 + 16) * C + (1 << 22)


def test_null_pointers_rejected_before_device_work():
    L = _native.load()
    tb = L.ghs_forest_dendro_workspace_bytes(5, 3)
    for k, name in enumerate(NAMES):
        if name in OPTIONAL:
            continue
        args = list(GOOD)
        args[k] = None
        rc, _ = _call(L, 5, 3, args, tb)
        assert rc == _native.GHS_E_ARG, name  # not GHS_E_NODEVICE: the check comes first
        assert b"NULL" in L.ghs_last_error()
    assert L.ghs_forest_dendro_device(5, 3, *GOOD[:10], GOOD[10], tb, None, None) == _native.GHS_E_ARG
    assert b"NULL" in L.ghs_last_error()
    # m == 0 needs leaf_parent only
    rc, _ = _call(L, 5, 0, [None] * 11, 0)
    assert rc == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error()
    only_leaf = [None] * 11
    only_leaf[4] = GOOD[4] + 2
    rc, _ = _call(L, 5, 0, only_leaf, 0)
    assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error()
    if _native.device_count() == 0:
        only_leaf[4] = GOOD[4]
        rc, _ = _call(L, 5, 0, only_leaf, 0)
        assert rc == _native.GHS_E_NODEVICE  # every pointer check passed with leaf_parent alone


def test_children_and_size_may_be_null():
    """NULL d_child_a / d_child_b / d_size pass the pointer checks: the next check (a short workspace) answers."""
    L = _native.load()
    for drop in ((7,), (8,), (9,), (7, 8), (7, 9), (8, 9), (7, 8, 9)):
        args = list(GOOD)
        for k in drop:
            args[k] = None
        rc, _ = _call(L, 5, 3, args, 0)
        assert rc == _native.GHS_E_NOMEM, drop


def test_misaligned_pointers_rejected():
    L = _native.load()
    tb = L.ghs_forest_dendro_workspace_bytes(5, 3)
    for k in (0, 1, 2, 10):  # u, v, w, workspace: 16 bytes
        for off in (1, 4, 8, 12):
            args = list(GOOD)
            args[k] += off
            rc, _ = _call(L, 5, 3, args, tb)
            assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), (k, off)
    for k in (4, 5, 6, 7, 8, 9):  # the six outputs: 4 bytes
        for off in (1, 2, 3):
            args = list(GOOD)
            args[k] += off
            rc, _ = _call(L, 5, 3, args, tb)
            assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), (k, off)
    for off in (1, 2, 3, 5, 9):  # the flags: any byte alignment passes the pointer checks
        args = list(GOOD)
        args[3] += off
        rc, _ = _call(L, 5, 3, args, 0)
        assert rc == _native.GHS_E_NOMEM, off


def test_edge_count_cap_and_short_workspace():
    L = _native.load()
    for m in (1 << 31, 1 << 40):
        rc, _ = _call(L, 5, m, GOOD, 1 << 50)
        assert rc == _native.GHS_E_ARG and b"2^31" in L.ghs_last_error()
    tb = L.ghs_forest_dendro_workspace_bytes(5000, 20000)
    for short in (0, 1, tb - 1):
        rc, _ = _call(L, 5000, 20000, GOOD, short)
        assert rc == _native.GHS_E_NOMEM, short


def test_no_vertices_is_ok_with_null_pointers():
    L = _native.load()
    rc, res = _call(L, 0, 0, (None,) * 11, 0)
    assert rc == _native.GHS_OK
    assert (res.flagged_edges, res.num_trees, res.max_height, res.levels, res.rounds, res.is_forest) == (0, 0, 0, 0, 0, 1)


def test_host_entry_argument_errors():
    L = _native.load()
    res = _native.DendroResult()
    a = np.zeros(8, np.uint32)
    f = np.zeros(8, np.uint8)
    p, fp = a.ctypes.data, f.ctypes.data

    def host(n, m, *ptrs, r=res):
        return L.ghs_forest_dendro_host(n, m, *ptrs, ctypes.byref(r) if r is not None else None)
    full = [p, p, p, fp, p, p, p, p, p, p]
    assert host(5, 1 << 31, *full) == _native.GHS_E_ARG and b"2^31" in L.ghs_last_error()
    for k in range(7):  # u, v, w, flags, leaf_parent, merge_eid, merge_parent
        args = list(full)
        args[k] = None
        assert host(5, 3, *args) == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error(), k
    assert host(5, 0, *([None] * 10)) == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error()
    assert host(5, 3, *full, r=None) == _native.GHS_E_ARG
    assert host(0, 0, *([None] * 10)) == _native.GHS_OK
    assert (res.num_trees, res.is_forest) == (0, 1)
    if _native.device_count() == 0:  # the optional three may be NULL: the next answer is the missing device
        assert host(5, 3, *full[:7], None, None, None) == _native.GHS_E_NODEVICE


def test_python_value_errors_without_a_gpu():
    import torch

    from distributed_ghs_implementation_amd.device import Dendrogram, DeviceEdges, forest_dendrogram
    z = torch.zeros(3, dtype=torch.int32)
    flags = torch.zeros(3, dtype=torch.uint8)
    csr_only = DeviceEdges(3, None, z, z, off=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="CSR"):
        forest_dendrogram(csr_only, flags)
    coo = DeviceEdges(3, z, z, z)
    with pytest.raises(ValueError):
        forest_dendrogram(coo, torch.zeros(2, dtype=torch.uint8))   # fewer flags than edges
    with pytest.raises(ValueError):
        forest_dendrogram(coo, torch.zeros(3, dtype=torch.int32))   # not flags
    with pytest.raises(ValueError):
        forest_dendrogram(coo, torch.zeros((3, 1), dtype=torch.uint8))
    # linkage: one tree only, and only with the children and the sizes
    one = torch.zeros(1, dtype=torch.int32)
    two = Dendrogram(3, z, one, one, one, one, one, info={"is_forest": True})   # 1 merge on 3 vertices
    with pytest.raises(ValueError, match="one tree"):
        two.linkage(coo)
    with pytest.raises(ValueError, match="children"):
        Dendrogram(2, z[:2], one, one, None, None, one).linkage(coo)
    with pytest.raises(ValueError, match="cycle"):
        Dendrogram(2, z[:2], one, one, one, one, one, info={"is_forest": False}).linkage(coo)


@pytest.mark.skipif(_native.device_count() > 0, reason="CPU-only behaviour")
def test_no_cpu_fallback_without_gpu():
    from distributed_ghs_implementation_amd import canonicalize
    from distributed_ghs_implementation_amd.mst import MSTResult
    g = canonicalize(3, edges=[(0, 1, 1), (1, 2, 2)])
    with pytest.raises(_native.GHSError) as ei:
        MSTResult(g, np.ones(2, bool), 3, 1, [], 0.0).dendrogram()
    assert ei.value.code == _native.GHS_E_NODEVICE


def test_dendro_hip_stands_alone():
    """csrc/dendro.hip includes no project source but common.h, launches only kernels it defines (all
    named k_dg_*), and shares no kernel name with any other file of csrc/."""
    src = open(DENDRO_HIP).read()
    assert re.findall(r'^\s*#\s*include\s+"([^"]+)"', src, re.M) == ["common.h"]
    for inc in re.findall(r"^\s*#\s*include\s+<([^>]+)>", src, re.M):
        assert inc.startswith(("hip/", "rocprim/")) or "/" not in inc, inc  # HIP, rocPRIM, the C++ library
    launched = set(re.findall(r"\b(k_\w+)\s*(?:<[^<>]*>)?\s*<<<", src))
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src, re.S))
    assert launched and launched <= defined, launched - defined
    assert all(k.startswith("k_dg_") for k in defined), defined
    assert "ghs_check_canonical(" in src
    assert src.index("ghs_check_canonical(n, m") < src.index("const Layout l = layout(n, m);")  # before any index
    other = ""
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")) and name != "dendro.hip":
            other += open(os.path.join(CSRC, name)).read()
    for part in sorted(os.listdir(os.path.join(CSRC, "boruvka"))):
        other += open(os.path.join(CSRC, "boruvka", part)).read()
    other_kernels = set(re.findall(r"\bvoid\s+(k_\w+)\s*\(", other))
    assert other_kernels and not (defined & other_kernels)
    assert not re.search(r"\bk_dg_\w*", other)


def test_makefile_links_dendro_everywhere():
    lines = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ").split("\n")
    objs = [ln for ln in lines if re.match(r"OBJS\s*:=", ln)]
    assert len(objs) == 1 and "$(OUTDIR)/dendro.o" in objs[0] and "$(OUTDIR)/root.o" in objs[0]
    prereq = [ln for ln in lines if ln.startswith("rcclstub:")]
    assert len(prereq) == 1 and "$(OUTDIR)/dendro.o" in prereq[0]     # the target's prerequisites
    link = [ln for ln in lines if ln.startswith("\t") and "-o $(STUB)/libghs_mst_rcclstub.so" in ln]
    assert len(link) == 1 and "$(OUTDIR)/dendro.o" in link[0]         # and its link line
