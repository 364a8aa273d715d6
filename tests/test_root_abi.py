"""The rooted-forest entry points' C-ABI boundary without a GPU (ghs_forest_root_workspace_bytes /
ghs_forest_root_device / ghs_forest_root_host): the result's layout, every argument check that comes
before any device work, the workspace size, the n == 0 answer, the Python layers' ValueErrors, and the
independence of csrc/root.hip from every other translation unit."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from distributed_ghs_implementation_amd import _native

# host addresses standing in for device pointers: every check below fails before anything is read
BASE = 1 << 20
NAMES = ("u", "v", "flags", "parent", "parent_eid", "depth", "pre", "size", "ws")
GOOD = tuple(BASE + (k << 16) for k in range(len(NAMES)))
CSRC = os.path.join(ROOT, "distributed_ghs_implementation_amd", "csrc")
ROOT_HIP = os.path.join(CSRC, "root.hip")
SYMBOLS = {"ghs_forest_root_workspace_bytes", "ghs_forest_root_device", "ghs_forest_root_host"}


def _call(L, n, m, ptrs, ws_bytes):
    u, v, f, par, peid, dep, pre, size, ws = ptrs
    res = _native.RootResult()
    rc = L.ghs_forest_root_device(n, m, u, v, f, par, peid, dep, pre, size, ws, ws_bytes, None, ctypes.byref(res))
    return rc, res


def test_result_layout_symbols_and_header():
    R = _native.RootResult
    assert ctypes.sizeof(R) == 48
    assert [f for f, _ in R._fields_] == ["flagged_edges", "num_trees", "max_depth", "rounds", "is_forest", "ms_total",
                                          "reserved"]
    assert [getattr(R, f).offset for f, _ in R._fields_] == [0, 8, 16, 24, 28, 32, 40]
    assert SYMBOLS <= set(_native.EXPORTED_SYMBOLS)
    L = _native.load()
    for s in SYMBOLS:
        assert getattr(L, s) is not None
    assert L.ghs_abi_version() == 10 and _native.ABI_VERSION == 10
    header = open(os.path.join(ROOT, "include", "ghs_mst.h")).read()
    assert re.search(r"#define\s+GHS_MST_ABI_VERSION\s+10\b", header)
    for s in SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", header), s
    assert header.index("ghs_forest_labels_host(") < header.index("typedef struct ghs_root_result")
    for ref in ("ghs_implementation.py:63,212", "ghs_implementation_mpi.py:57,309"):
        assert ref in header  # the reference's in_branch lines
    assert "cyclically, starting after p" in header  # the child rule, stated exactly
    d = R().as_dict()
    assert set(d) == {f for f, _ in R._fields_} - {"reserved"} and d["is_forest"] is False


def test_workspace_bytes_without_a_gpu():
    L = _native.load()
    ns = (0, 1, 2, 7, 1023, 1024, 1025, 4095, 4096, 4097, 100000, 1 << 20, 1 << 24, (1 << 32) - 1)
    ms = (0, 1, 2, 1023, 1024, 1025, 4081, 4096, 4097, 1 << 20, 1 << 28, (1 << 31) - 1)
    table = [[L.ghs_forest_root_workspace_bytes(n, m) for m in ms] for n in ns]
    for i, n in enumerate(ns):
        assert table[i] == sorted(table[i]), n          # nondecreasing in m
        assert all(b >= 28 * n for b in table[i]), n    # adjacency ranges, tree sizes, root prefixes
    for j, m in enumerate(ms):
        col = [table[i][j] for i in range(len(ns))]
        assert col == sorted(col), m                    # nondecreasing in n
    # sized by min(m, n - 1) possible tree edges (24 B each + 84 B per arc), not by m
    assert L.ghs_forest_root_workspace_bytes(1000, 1 << 20) >= 28 * 1000 + (24 + 2 * 84) * 999
    assert L.ghs_forest_root_workspace_bytes(1000, 1 << 20) < L.ghs_forest_root_workspace_bytes(1000, 999) + (1 << 16)
    assert L.ghs_forest_root_workspace_bytes(1 << 20, 10) < L.ghs_forest_root_workspace_bytes(1 << 20, 1 << 20)


def test_null_pointers_rejected_before_device_work():
    L = _native.load()
    tb = L.ghs_forest_root_workspace_bytes(5, 3)
    for k, name in enumerate(NAMES):
        if name in ("pre", "size"):
            continue
        args = list(GOOD)
        args[k] = None
        rc, _ = _call(L, 5, 3, args, tb)
        assert rc == _native.GHS_E_ARG, name  # not GHS_E_NODEVICE: the check comes first
        assert b"NULL" in L.ghs_last_error()
    u, v, f, par, peid, dep, pre, size, ws = GOOD
    assert L.ghs_forest_root_device(5, 3, u, v, f, par, peid, dep, pre, size, ws, tb, None, None) == _native.GHS_E_ARG
    assert b"NULL" in L.ghs_last_error()
    # m == 0 needs the three mandatory outputs
    for k in (3, 4, 5):
        args = [None, None, None, par, peid, dep, None, None, None]
        args[k] = None
        rc, _ = _call(L, 5, 0, args, 0)
        assert rc == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error()


def test_pre_and_size_may_be_null():
    """NULL d_pre / d_size pass the pointer checks: the next check (a short workspace) answers."""
    L = _native.load()
    for drop in ((6,), (7,), (6, 7)):
        args = list(GOOD)
        for k in drop:
            args[k] = None
        rc, _ = _call(L, 5, 3, args, 0)
        assert rc == _native.GHS_E_NOMEM, drop


def test_misaligned_pointers_rejected():
    L = _native.load()
    tb = L.ghs_forest_root_workspace_bytes(5, 3)
    for k in (0, 1, 8):  # u, v, workspace: 16 bytes
        for off in (1, 4, 8, 12):
            args = list(GOOD)
            args[k] += off
            rc, _ = _call(L, 5, 3, args, tb)
            assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), (k, off)
    for k in (3, 4, 5, 6, 7):  # the five outputs: 4 bytes
        for off in (1, 2, 3):
            args = list(GOOD)
            args[k] += off
            rc, _ = _call(L, 5, 3, args, tb)
            assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), (k, off)
    for off in (1, 2, 3, 5, 9):  # the flags: any byte alignment passes the pointer checks
        args = list(GOOD)
        args[2] += off
        rc, _ = _call(L, 5, 3, args, 0)
        assert rc == _native.GHS_E_NOMEM, off


def test_edge_count_cap_and_short_workspace():
    L = _native.load()
    for m in (1 << 31, 1 << 40):
        rc, _ = _call(L, 5, m, GOOD, 1 << 50)
        assert rc == _native.GHS_E_ARG and b"2^31" in L.ghs_last_error()
    tb = L.ghs_forest_root_workspace_bytes(5000, 20000)
    for short in (0, 1, tb - 1):
        rc, _ = _call(L, 5000, 20000, GOOD, short)
        assert rc == _native.GHS_E_NOMEM, short


def test_no_vertices_is_ok_with_null_pointers():
    L = _native.load()
    rc, res = _call(L, 0, 0, (None,) * 9, 0)
    assert rc == _native.GHS_OK
    assert (res.flagged_edges, res.num_trees, res.max_depth, res.rounds, res.is_forest) == (0, 0, 0, 0, 1)


def test_host_entry_argument_errors():
    L = _native.load()
    res = _native.RootResult()
    a = np.zeros(8, np.uint32)
    f = np.zeros(8, np.uint8)
    p, fp = a.ctypes.data, f.ctypes.data

    def host(n, m, u, v, fl, par, peid, dep, pre, size, r=res):
        return L.ghs_forest_root_host(n, m, u, v, fl, par, peid, dep, pre, size, ctypes.byref(r) if r is not None else None)
    assert host(5, 1 << 31, p, p, fp, p, p, p, p, p) == _native.GHS_E_ARG and b"2^31" in L.ghs_last_error()
    for k in range(6):  # u, v, flags, parent, parent_eid, depth
        args = [p, p, fp, p, p, p, p, p]
        args[k] = None
        assert host(5, 3, *args) == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error(), k
    assert host(5, 0, None, None, None, p, p, None, p, p) == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error()
    assert host(5, 3, p, p, fp, p, p, p, p, p, r=None) == _native.GHS_E_ARG
    assert host(0, 0, None, None, None, None, None, None, None, None) == _native.GHS_OK
    assert (res.num_trees, res.is_forest) == (0, 1)


def test_python_value_errors_without_a_gpu():
    import torch

    from distributed_ghs_implementation_amd.device import DeviceEdges, forest_root
    z = torch.zeros(3, dtype=torch.int32)
    flags = torch.zeros(3, dtype=torch.uint8)
    csr_only = DeviceEdges(3, None, z, z, off=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="CSR"):
        forest_root(csr_only, flags)
    coo = DeviceEdges(3, z, z, z)
    with pytest.raises(ValueError):
        forest_root(coo, torch.zeros(2, dtype=torch.uint8))   # fewer flags than edges
    with pytest.raises(ValueError):
        forest_root(coo, torch.zeros(3, dtype=torch.int32))   # not flags
    with pytest.raises(ValueError):
        forest_root(coo, torch.zeros((3, 1), dtype=torch.uint8))


@pytest.mark.skipif(_native.device_count() > 0, reason="CPU-only behaviour")
def test_no_cpu_fallback_without_gpu():
    from distributed_ghs_implementation_amd import canonicalize
    from distributed_ghs_implementation_amd.mst import MSTResult
    g = canonicalize(3, edges=[(0, 1, 1), (1, 2, 2)])
    with pytest.raises(_native.GHSError) as ei:
        MSTResult(g, np.ones(2, bool), 3, 1, [], 0.0).rooted()
    assert ei.value.code == _native.GHS_E_NODEVICE


def test_root_hip_stands_alone():
    """csrc/root.hip includes no project source but common.h, launches only kernels it defines (all
    named k_rt_*), and shares no kernel name with any other file of csrc/."""
    src = open(ROOT_HIP).read()
    assert re.findall(r'^\s*#\s*include\s+"([^"]+)"', src, re.M) == ["common.h"]
    for inc in re.findall(r"^\s*#\s*include\s+<([^>]+)>", src, re.M):
        assert inc.startswith(("hip/", "rocprim/")) or "/" not in inc, inc  # HIP, rocPRIM, the C++ library
    launched = set(re.findall(r"\b(k_\w+)\s*(?:<[^<>]*>)?\s*<<<", src))
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src, re.S))
    assert launched and launched <= defined, launched - defined
    assert all(k.startswith("k_rt_") for k in defined), defined
    assert "ghs_check_canonical(" in src
    other = ""
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")) and name != "root.hip":
            other += open(os.path.join(CSRC, name)).read()
    for part in sorted(os.listdir(os.path.join(CSRC, "boruvka"))):
        other += open(os.path.join(CSRC, "boruvka", part)).read()
    other_kernels = set(re.findall(r"\bvoid\s+(k_\w+)\s*\(", other))
    assert other_kernels and not (defined & other_kernels)
    assert not re.search(r"\bk_rt_\w+", other)


def test_makefile_links_root_everywhere():
    lines = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ").split("\n")
    objs = [ln for ln in lines if re.match(r"OBJS\s*:=", ln)]
    assert len(objs) == 1 and "$(OUTDIR)/root.o" in objs[0] and "$(OUTDIR)/labels.o" in objs[0]
    prereq = [ln for ln in lines if ln.startswith("rcclstub:")]
    assert len(prereq) == 1 and "$(OUTDIR)/root.o" in prereq[0]     # the target's prerequisites
    link = [ln for ln in lines if ln.startswith("\t") and "-o $(STUB)/libghs_mst_rcclstub.so" in ln]
    assert len(link) == 1 and "$(OUTDIR)/root.o" in link[0]         # and its link line
