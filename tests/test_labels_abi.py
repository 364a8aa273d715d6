"""The vertex-label entry points' C-ABI boundary without a GPU (ghs_forest_labels_workspace_bytes /
ghs_forest_labels_device / ghs_forest_labels_host): the result's layout, every argument check that
comes before any device work, the workspace size, the n == 0 answer, the Python layers' ValueErrors,
and the independence of csrc/labels.hip from the solver and the verifier."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from distributed_ghs_implementation_amd import _native

U64_MAX = (1 << 64) - 1
# host addresses standing in for device pointers: every check below fails before anything is read
BASE = 1 << 20
U_PTR, V_PTR, W_PTR, F_PTR, L_PTR, WS_PTR = (BASE + (k << 16) for k in range(6))
GOOD = (U_PTR, V_PTR, W_PTR, F_PTR, L_PTR, WS_PTR)
CSRC = os.path.join(ROOT, "distributed_ghs_implementation_amd", "csrc")
LABELS_HIP = os.path.join(CSRC, "labels.hip")


def _call(L, n, m, ptrs, ws_bytes, mode=0, param=0):
    u, v, w, f, lab, ws = ptrs
    res = _native.LabelsResult()
    rc = L.ghs_forest_labels_device(n, m, u, v, w, f, mode, param, lab, ws, ws_bytes, None, ctypes.byref(res))
    return rc, res


def test_result_layout_symbols_and_constants():
    R = _native.LabelsResult
    assert ctypes.sizeof(R) == 64
    assert [f for f, _ in R._fields_] == ["flagged_edges", "kept_edges", "dropped_edges", "num_clusters", "cut_key",
                                          "rounds", "is_forest", "ms_total", "reserved"]
    assert (R.cut_key.offset, R.rounds.offset, R.is_forest.offset, R.ms_total.offset) == (32, 40, 44, 48)
    names = {"ghs_forest_labels_workspace_bytes", "ghs_forest_labels_device", "ghs_forest_labels_host"}
    assert names <= set(_native.EXPORTED_SYMBOLS)
    L = _native.load()
    for s in names:
        assert getattr(L, s) is not None
    assert L.ghs_abi_version() == 10
    assert (_native.GHS_CUT_NONE, _native.GHS_CUT_WEIGHT, _native.GHS_CUT_COUNT) == (0, 1, 2)
    header = open(os.path.join(ROOT, "include", "ghs_mst.h")).read()
    for name, val in (("GHS_CUT_NONE", 0), ("GHS_CUT_WEIGHT", 1), ("GHS_CUT_COUNT", 2)):
        assert re.search(rf"#define\s+{name}\s+{val}u\b", header), name
    d = R().as_dict()
    assert set(d) == {f for f, _ in R._fields_} - {"reserved"} and d["is_forest"] is False


def test_workspace_bytes_without_a_gpu():
    L = _native.load()
    ns = (0, 1, 2, 7, 1023, 1024, 1025, 4095, 4096, 4097, 100000, 1 << 20, 1 << 24, (1 << 32) - 1)
    ms = (0, 1, 2, 1023, 1024, 1025, 4081, 4096, 4097, 1 << 20, 1 << 28, (1 << 31) - 1)
    table = [[L.ghs_forest_labels_workspace_bytes(n, m) for m in ms] for n in ns]
    for i, n in enumerate(ns):
        assert table[i] == sorted(table[i]), n          # nondecreasing in m
        assert all(b >= 8 * n for b in table[i]), n     # par + ranks
    for j, m in enumerate(ms):
        col = [table[i][j] for i in range(len(ns))]
        assert col == sorted(col), m                    # nondecreasing in n
    # room for min(m, n - 1) kept edges, twice (the live list and its successor), and their keys
    assert L.ghs_forest_labels_workspace_bytes(1000, 1 << 20) >= 8 * 1000 + 3 * 8 * 999
    assert L.ghs_forest_labels_workspace_bytes(1 << 20, 10) < L.ghs_forest_labels_workspace_bytes(1 << 20, 1 << 20)


def test_null_pointers_rejected_before_device_work():
    L = _native.load()
    tb = L.ghs_forest_labels_workspace_bytes(5, 3)
    for k in range(6):
        args = list(GOOD)
        args[k] = None
        rc, _ = _call(L, 5, 3, args, tb)
        assert rc == _native.GHS_E_ARG, k  # not GHS_E_NODEVICE: the check comes first
        assert b"NULL" in L.ghs_last_error()
    u, v, w, f, lab, ws = GOOD
    assert L.ghs_forest_labels_device(5, 3, u, v, w, f, 0, 0, lab, ws, tb, None, None) == _native.GHS_E_ARG
    assert b"NULL" in L.ghs_last_error()
    # m == 0 needs the labels only
    rc, _ = _call(L, 5, 0, (None, None, None, None, None, None), 0)
    assert rc == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error()


def test_misaligned_pointers_rejected():
    L = _native.load()
    tb = L.ghs_forest_labels_workspace_bytes(5, 3)
    for k in (0, 1, 2, 5):  # u, v, w, workspace: 16 bytes
        for off in (1, 4, 8, 12):
            args = list(GOOD)
            args[k] += off
            rc, _ = _call(L, 5, 3, args, tb)
            assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), (k, off)
    for off in (1, 2, 3):  # labels: 4 bytes
        args = list(GOOD)
        args[4] += off
        rc, _ = _call(L, 5, 3, args, tb)
        assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), off


def test_edge_count_cap_mode_param_and_short_workspace():
    L = _native.load()
    for m in (1 << 31, 1 << 40):
        rc, _ = _call(L, 5, m, GOOD, 1 << 50)
        assert rc == _native.GHS_E_ARG and b"2^31" in L.ghs_last_error()
    tb = L.ghs_forest_labels_workspace_bytes(5000, 20000)
    for mode in (3, 7, 0xFFFFFFFF):
        rc, _ = _call(L, 5000, 20000, GOOD, tb, mode=mode, param=1)
        assert rc == _native.GHS_E_ARG and b"mode" in L.ghs_last_error(), mode
    for param in (1 << 32, (1 << 32) + 5, U64_MAX):
        rc, _ = _call(L, 5000, 20000, GOOD, tb, mode=_native.GHS_CUT_WEIGHT, param=param)
        assert rc == _native.GHS_E_ARG and b"2^32" in L.ghs_last_error(), param
    rc, _ = _call(L, 5000, 20000, GOOD, tb, mode=_native.GHS_CUT_COUNT, param=0)
    assert rc == _native.GHS_E_ARG and b">= 1" in L.ghs_last_error()
    for short in (0, 1, tb - 1):
        rc, _ = _call(L, 5000, 20000, GOOD, short)
        assert rc == _native.GHS_E_NOMEM, short


def test_host_entry_argument_errors():
    L = _native.load()
    res = _native.LabelsResult()
    a = np.zeros(4, np.uint32)
    f = np.zeros(4, np.uint8)
    p = a.ctypes.data

    def host(n, m, u, v, w, fl, mode, param, lab, r=res):
        return L.ghs_forest_labels_host(n, m, u, v, w, fl, mode, param, lab, ctypes.byref(r) if r is not None else None)
    assert host(5, 3, p, p, p, f.ctypes.data, 9, 0, p) == _native.GHS_E_ARG and b"mode" in L.ghs_last_error()
    assert host(5, 3, p, p, p, f.ctypes.data, 1, 1 << 32, p) == _native.GHS_E_ARG and b"2^32" in L.ghs_last_error()
    assert host(5, 3, p, p, p, f.ctypes.data, 2, 0, p) == _native.GHS_E_ARG and b">= 1" in L.ghs_last_error()
    assert host(5, 1 << 31, p, p, p, f.ctypes.data, 0, 0, p) == _native.GHS_E_ARG and b"2^31" in L.ghs_last_error()
    assert host(5, 3, None, p, p, f.ctypes.data, 0, 0, p) == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error()
    assert host(5, 3, p, p, p, f.ctypes.data, 0, 0, None) == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error()
    assert host(5, 3, p, p, p, f.ctypes.data, 0, 0, p, r=None) == _native.GHS_E_ARG
    assert host(0, 0, None, None, None, None, 0, 0, None) == _native.GHS_OK
    assert (res.num_clusters, res.cut_key, res.is_forest) == (0, U64_MAX, 1)


@pytest.mark.parametrize("mode,param", [(0, 0), (1, 7), (2, 3)])
def test_no_vertices_is_ok_with_null_pointers(mode, param):
    L = _native.load()
    rc, res = _call(L, 0, 0, (None,) * 6, 0, mode=mode, param=param)
    assert rc == _native.GHS_OK
    assert (res.flagged_edges, res.kept_edges, res.dropped_edges, res.num_clusters, res.rounds) == (0, 0, 0, 0, 0)
    assert res.cut_key == U64_MAX and res.is_forest == 1


def test_python_value_errors_without_a_gpu():
    import torch

    from distributed_ghs_implementation_amd import canonicalize
    from distributed_ghs_implementation_amd.device import DeviceEdges, forest_labels
    from distributed_ghs_implementation_amd.mst import MSTResult
    z = torch.zeros(3, dtype=torch.int32)
    flags = torch.zeros(3, dtype=torch.uint8)
    csr_only = DeviceEdges(3, None, z, z, off=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="CSR"):
        forest_labels(csr_only, flags)
    coo = DeviceEdges(3, z, z, z)
    with pytest.raises(ValueError):
        forest_labels(coo, torch.zeros(2, dtype=torch.uint8))   # fewer flags than edges
    with pytest.raises(ValueError):
        forest_labels(coo, torch.zeros(3, dtype=torch.int32))   # not flags
    with pytest.raises(ValueError, match="not both"):
        forest_labels(coo, flags, max_weight=1, num_clusters=2)
    with pytest.raises(ValueError):
        forest_labels(coo, flags, num_clusters=0)
    with pytest.raises(ValueError):
        forest_labels(coo, flags, max_weight=1 << 32)
    g = canonicalize(3, edges=[(0, 1, 1), (1, 2, 2)])
    r = MSTResult(g, np.ones(2, bool), 3, 1, [], 0.0)
    with pytest.raises(ValueError, match="not both"):
        r.labels(max_weight=1, num_clusters=2)
    with pytest.raises(ValueError):
        r.labels(num_clusters=0)
    with pytest.raises(ValueError):
        r.labels(max_weight=-1)


@pytest.mark.skipif(_native.device_count() > 0, reason="CPU-only behaviour")
def test_no_cpu_fallback_without_gpu():
    from distributed_ghs_implementation_amd import canonicalize
    from distributed_ghs_implementation_amd.mst import MSTResult
    g = canonicalize(3, edges=[(0, 1, 1), (1, 2, 2)])
    with pytest.raises(_native.GHSError) as ei:
        MSTResult(g, np.ones(2, bool), 3, 1, [], 0.0).labels()
    assert ei.value.code == _native.GHS_E_NODEVICE


def test_labels_hip_stands_alone():
    """csrc/labels.hip includes no project source but common.h, launches only kernels it defines, and
    shares no kernel name with the solver or the verifier."""
    src = open(LABELS_HIP).read()
    assert re.findall(r'^\s*#\s*include\s+"([^"]+)"', src, re.M) == ["common.h"]
    for inc in re.findall(r"^\s*#\s*include\s+<([^>]+)>", src, re.M):
        assert inc.startswith(("hip/", "rocprim/")) or "/" not in inc, inc  # HIP, rocPRIM, the C++ library
    launched = set(re.findall(r"\b(k_\w+)\s*(?:<[^<>]*>)?\s*<<<", src))
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src, re.S))
    assert launched and launched <= defined, launched - defined
    other = ""
    for name in ("boruvka.hip", "batch.hip", "verify.hip", "ingest.hip", "multi.hip", "host.hip"):
        other += open(os.path.join(CSRC, name)).read()
    for part in sorted(os.listdir(os.path.join(CSRC, "boruvka"))):
        other += open(os.path.join(CSRC, "boruvka", part)).read()
    other_kernels = set(re.findall(r"\bvoid\s+(k_\w+)\s*\(", other))
    assert other_kernels and not (defined & other_kernels)


def test_makefile_links_labels_everywhere():
    lines = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ").split("\n")
    objs = [ln for ln in lines if re.match(r"OBJS\s*:=", ln)]
    assert len(objs) == 1 and "$(OUTDIR)/labels.o" in objs[0]
    prereq = [ln for ln in lines if ln.startswith("rcclstub:")]
    assert len(prereq) == 1 and "$(OUTDIR)/labels.o" in prereq[0]   # the target's prerequisites
    link = [ln for ln in lines if ln.startswith("\t") and "-o $(STUB)/libghs_mst_rcclstub.so" in ln]
    assert len(link) == 1 and "$(OUTDIR)/labels.o" in link[0]       # and its link line
