"""The device verifier's C-ABI boundary without a GPU (ghs_verify_workspace_bytes /
ghs_verify_msf_device): the result's layout, every argument check that comes before any device work,
the workspace size, the m == 0 verdict, and the independence of csrc/verify.hip from the solver."""
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
U_PTR, V_PTR, W_PTR, F_PTR, WS_PTR = (BASE + (k << 16) for k in range(5))
VERIFY_HIP = os.path.join(ROOT, "distributed_ghs_implementation_amd", "csrc", "verify.hip")


def _call(L, n, m, u, v, w, f, ws, ws_bytes):
    res = _native.VerifyResult()
    return L.ghs_verify_msf_device(n, m, u, v, w, f, ws, ws_bytes, None, ctypes.byref(res)), res


def test_result_layout_and_symbols():
    assert ctypes.sizeof(_native.VerifyResult) == 80
    assert [f for f, _ in _native.VerifyResult._fields_] == [
        "ok", "rounds", "overfull", "reserved", "tree_edges", "components", "total_weight",
        "cyclic_edges", "unspanned_edges", "lighter_edges", "first_bad_eid", "ms_total"]
    assert _native.VerifyResult.tree_edges.offset == 16 and _native.VerifyResult.ms_total.offset == 72
    assert {"ghs_verify_workspace_bytes", "ghs_verify_msf_device"} <= set(_native.EXPORTED_SYMBOLS)
    assert _native.load().ghs_abi_version() == 10


def test_workspace_bytes_without_a_gpu():
    L = _native.load()
    ns = (0, 1, 2, 7, 4095, 4096, 4097, 100000, 1 << 20, 1 << 24, (1 << 32) - 1)
    ms = (0, 1, 2, 1023, 1024, 1025, 4096, 4097, 1 << 20, 1 << 28, (1 << 31) - 1)
    table = [[L.ghs_verify_workspace_bytes(n, m) for m in ms] for n in ns]
    for i, n in enumerate(ns):
        assert table[i] == sorted(table[i]), n          # nondecreasing in m
        assert all(b >= 32 * n for b in table[i]), n    # the <= 2n nodes of 16 bytes
    for j, m in enumerate(ms):
        col = [table[i][j] for i in range(len(ns))]
        assert col == sorted(col), m                    # nondecreasing in n
    # room for min(m, n - 1) tree edges, twice (the live list and its successor)
    assert L.ghs_verify_workspace_bytes(1000, 1 << 20) >= 32 * 1000 + 2 * 16 * 999
    assert L.ghs_verify_workspace_bytes(1 << 20, 10) < L.ghs_verify_workspace_bytes(1 << 20, 1 << 20)


def test_null_pointers_rejected_before_device_work():
    L = _native.load()
    tb = L.ghs_verify_workspace_bytes(5, 3)
    good = [U_PTR, V_PTR, W_PTR, F_PTR, WS_PTR]
    for k in range(5):
        args = list(good)
        args[k] = None
        rc, _ = _call(L, 5, 3, *args, tb)
        assert rc == _native.GHS_E_ARG  # not GHS_E_NODEVICE: the check comes first
        assert b"NULL" in L.ghs_last_error()
    assert L.ghs_verify_msf_device(5, 3, U_PTR, V_PTR, W_PTR, F_PTR, WS_PTR, tb, None, None) == _native.GHS_E_ARG
    assert b"NULL" in L.ghs_last_error()


def test_misaligned_pointers_rejected():
    L = _native.load()
    tb = L.ghs_verify_workspace_bytes(5, 3)
    for k in (0, 1, 2, 4):  # u, v, w, workspace: 16 bytes
        for off in (1, 4, 8, 12):
            args = [U_PTR, V_PTR, W_PTR, F_PTR, WS_PTR]
            args[k] += off
            rc, _ = _call(L, 5, 3, *args, tb)
            assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), (k, off)


def test_edge_count_cap_and_short_workspace():
    L = _native.load()
    for m in (1 << 31, 1 << 40):
        rc, _ = _call(L, 5, m, U_PTR, V_PTR, W_PTR, F_PTR, WS_PTR, 1 << 50)
        assert rc == _native.GHS_E_ARG and b"2^31" in L.ghs_last_error()
    tb = L.ghs_verify_workspace_bytes(5000, 20000)
    for short in (0, 1, tb - 1):
        rc, _ = _call(L, 5000, 20000, U_PTR, V_PTR, W_PTR, F_PTR, WS_PTR, short)
        assert rc == _native.GHS_E_NOMEM, short


@pytest.mark.parametrize("n", [0, 1, 6, (1 << 32) - 1])
def test_empty_edge_list_is_ok_with_null_pointers(n):
    L = _native.load()
    rc, res = _call(L, n, 0, None, None, None, None, None, 0)
    assert rc == _native.GHS_OK
    assert (res.ok, res.overfull, res.rounds) == (1, 0, 0)
    assert (res.tree_edges, res.components, res.total_weight) == (0, n, 0)
    assert (res.cyclic_edges, res.unspanned_edges, res.lighter_edges) == (0, 0, 0)
    assert res.first_bad_eid == U64_MAX


def test_python_entry_points_without_a_gpu():
    """The m == 0 verdict through the Python layers (no device work), and the argument checks of
    device.verify_msf that need no GPU."""
    import torch

    from distributed_ghs_implementation_amd import canonicalize
    from distributed_ghs_implementation_amd.device import DeviceEdges, verify_msf
    from distributed_ghs_implementation_amd.verify import format_device_report, verify_forest_device
    g = canonicalize(4, edges=[])
    rep = verify_forest_device(g, np.zeros(0, bool))
    assert rep["ok"] is True and rep["components"] == 4 and rep["first_bad_eid"] == U64_MAX
    assert "CORRECT" in format_device_report(rep) and "INCORRECT" not in format_device_report(rep)
    with pytest.raises(ValueError):
        verify_forest_device(g, np.zeros(3, bool))
    z = torch.zeros(3, dtype=torch.int32)
    csr_only = DeviceEdges(3, None, z, z, off=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="CSR"):
        verify_msf(csr_only, torch.zeros(3, dtype=torch.uint8))
    coo = DeviceEdges(3, z, z, z)
    with pytest.raises(ValueError):
        verify_msf(coo, torch.zeros(2, dtype=torch.uint8))   # fewer flags than edges
    with pytest.raises(ValueError):
        verify_msf(coo, torch.zeros(3, dtype=torch.int32))   # not flags


@pytest.mark.skipif(_native.device_count() > 0, reason="CPU-only behaviour")
def test_no_cpu_fallback_without_gpu():
    from distributed_ghs_implementation_amd import canonicalize
    from distributed_ghs_implementation_amd.verify import verify_forest_device
    g = canonicalize(3, edges=[(0, 1, 1), (1, 2, 2)])
    with pytest.raises(_native.GHSError) as ei:
        verify_forest_device(g, np.ones(2, bool))
    assert ei.value.code == _native.GHS_E_NODEVICE


def test_verify_hip_is_independent_of_the_solver():
    """csrc/verify.hip includes no project source except common.h, and names no solver kernel."""
    src = open(VERIFY_HIP).read()
    project_includes = re.findall(r'^\s*#\s*include\s+"([^"]+)"', src, re.M)
    assert project_includes == ["common.h"]
    for inc in re.findall(r"^\s*#\s*include\s+<([^>]+)>", src, re.M):
        assert inc.startswith(("hip/", "rocprim/")) or "/" not in inc, inc  # HIP, rocPRIM, the C++ library
    launched = set(re.findall(r"\b(k_\w+)\s*<<<", src))
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src, re.S))
    assert launched and launched <= defined, launched - defined
    csrc = os.path.dirname(VERIFY_HIP)
    solver_src = open(os.path.join(csrc, "boruvka.hip")).read() + open(os.path.join(csrc, "batch.hip")).read()
    for part in sorted(os.listdir(os.path.join(csrc, "boruvka"))):
        solver_src += open(os.path.join(csrc, "boruvka", part)).read()
    solver_kernels = set(re.findall(r"\bvoid\s+(k_\w+)\s*\(", solver_src))
    assert solver_kernels and not (defined & solver_kernels)
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert makefile.count("$(OUTDIR)/verify.o") >= 3  # OBJS and both lines of the rcclstub target
