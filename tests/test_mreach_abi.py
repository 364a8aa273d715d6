"""The mutual-reachability entry points' C-ABI boundary without a GPU (ghs_mutual_reach_workspace_bytes /
ghs_mutual_reach_device / ghs_mutual_reach_host): the result's layout, the section's place in the header,
every argument check that comes before any device work, the workspace table, the n == 0 answer, the
Python layers' ValueErrors, and the independence of csrc/mreach.hip from every other translation unit."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from distributed_ghs_implementation_amd import _native

# host addresses standing in for device pointers: every check below fails before anything is read
BASE = 1 << 24
NAMES = ("u", "v", "w", "core", "w_out", "ws")
GOOD = tuple(BASE + (k << 20) for k in range(len(NAMES)))   # 1 MiB apart: nothing overlaps at n, m <= 2^16
CSRC = os.path.join(ROOT, "distributed_ghs_implementation_amd", "csrc")
MREACH_HIP = os.path.join(CSRC, "mreach.hip")
SYMBOLS = {"ghs_mutual_reach_workspace_bytes", "ghs_mutual_reach_device", "ghs_mutual_reach_host"}
N, M = 50, 200


def _call(L, n, m, ptrs, ws_bytes, k=5, res=True):
    r = _native.MreachResult()
    u, v, w, core, w_out, ws = ptrs
    rc = L.ghs_mutual_reach_device(n, m, u, v, w, k, core, w_out, ws, ws_bytes, None, ctypes.byref(r) if res else None)
    return rc, r


def test_result_layout_symbols_and_header():
    R = _native.MreachResult
    assert ctypes.sizeof(R) == 48
    assert [f for f, _ in R._fields_] == ["short_rows", "isolated", "raised_edges", "max_degree", "block_rows",
                                          "grid_rows", "reserved", "ms_total"]
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
    assert "/* 48 bytes */" in header[header.index("typedef struct ghs_mreach_result"):][:80]
    # directly after the cluster section, before ghs_check_canonical
    assert header.index("ghs_forest_cluster_host(") < header.index("typedef struct ghs_mreach_result")
    assert header.index("ghs_mutual_reach_host(") < header.index("int ghs_check_canonical(")
    between = header[header.index("ghs_forest_cluster_host("): header.index("typedef struct ghs_mreach_result")]
    assert "typedef struct" not in between                       # no other section in between
    body = header[header.index("typedef struct ghs_mreach_result"): header.index("} ghs_mreach_result_t;")]
    order = [body.index(f) for f, _ in R._fields_]
    assert order == sorted(order)  # the header declares the fields in the same order
    for name in ("d_u", "d_v", "d_w", "d_core", "d_w_out", "d_workspace"):
        assert name in header[header.index("int ghs_mutual_reach_device("):][:700], name
    for name in ("GHS_MREACH_BLOCK_ROW_MIN", "GHS_MREACH_GRID_ROW_MIN"):
        mt = re.search(rf"#define\s+{name}\s+(\d+)u", header)
        assert mt and int(mt.group(1)) == getattr(_native, name), name
    assert 4 * 64 >= _native.GHS_MREACH_BLOCK_ROW_MIN < _native.GHS_MREACH_GRID_ROW_MIN
    d = R().as_dict()
    assert set(d) == {f for f, _ in R._fields_} - {"reserved"}


def test_workspace_table_without_a_gpu():
    W = _native.load().ghs_mutual_reach_workspace_bytes
    ns = (1, 2, 7, 1023, 1024, 1025, 100000, 1 << 20, 1 << 24, (1 << 32) - 1)
    ms = (1, 2, 255, 256, 257, 4096, 32767, 32768, 32769, 1 << 20, (1 << 24) + 3, 1 << 28, (1 << 31) - 1)
    table = [[W(n, m) for m in ms] for n in ns]
    for i, n in enumerate(ns):
        assert table[i] == sorted(table[i]), n                   # nondecreasing in m
        for j, m in enumerate(ms):
            assert table[i][j] % 256 == 0 and table[i][j] >= 8 * n + 8 * m + 1024, (n, m)
    for j, m in enumerate(ms):
        col = [table[i][j] for i in range(len(ns))]
        assert col == sorted(col), m                             # nondecreasing in n
    # 8 B per vertex + 8 B per edge + the sort's storage (its own copy of the pairs) + the lists, not more
    n, m = 1 << 24, 1 << 28
    assert W(n, m) < 8 * n + 8 * m + 8 * m + m // 2 + (1 << 24)
    assert W(0, 5) == 0 and W(5, 0) == 0 and W(5, 1 << 31) == 0


def test_argument_errors_come_before_device_work():
    L = _native.load()
    tb = L.ghs_mutual_reach_workspace_bytes(N, M)
    assert tb > 0
    rc, _ = _call(L, N, M, GOOD, tb, res=False)
    assert rc == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error()
    rc, _ = _call(L, N, M, GOOD, tb, k=0)
    assert rc == _native.GHS_E_ARG and b"k" in L.ghs_last_error()
    for m in (1 << 31, (1 << 31) + 1, 1 << 40):
        rc, _ = _call(L, N, m, GOOD, 1 << 62)
        assert rc == _native.GHS_E_ARG and b"2^31" in L.ghs_last_error(), m
    if _native.device_count() == 0:                              # every check passes: only the device is missing
        rc, _ = _call(L, N, M, GOOD, tb)
        assert rc == _native.GHS_E_NODEVICE
        rc, _ = _call(L, N, M, GOOD, tb, k=(1 << 32) - 1)        # any k >= 1
        assert rc == _native.GHS_E_NODEVICE


def test_null_pointers_rejected_before_device_work():
    L = _native.load()
    tb = L.ghs_mutual_reach_workspace_bytes(N, M)
    for k, name in enumerate(NAMES):
        args = list(GOOD)
        args[k] = None
        if name == "w_out":                                      # optional: the core distances alone
            if _native.device_count() == 0:                      # (with a GPU the call would go on to run)
                rc, _ = _call(L, N, M, args, tb)
                assert rc == _native.GHS_E_NODEVICE
            continue
        rc, _ = _call(L, N, M, args, tb if name != "ws" else 0)
        assert rc == _native.GHS_E_ARG, name                     # not GHS_E_NODEVICE: the check comes first
        assert b"NULL" in L.ghs_last_error()
    # m == 0 needs core only
    rc, _ = _call(L, 5, 0, (None,) * 6, 0)
    assert rc == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error()
    if _native.device_count() == 0:
        rc, _ = _call(L, 5, 0, (None, None, None, GOOD[3], None, None), 0)
        assert rc == _native.GHS_E_NODEVICE


def test_misaligned_pointers_rejected():
    L = _native.load()
    tb = L.ghs_mutual_reach_workspace_bytes(N, M)
    for name in ("u", "v", "w", "w_out", "ws"):
        for off in (1, 2, 4, 8, 12):
            args = list(GOOD)
            args[NAMES.index(name)] += off
            rc, _ = _call(L, N, M, args, tb)
            assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), (name, off)
    for off in (1, 2, 3):
        args = list(GOOD)
        args[NAMES.index("core")] += off
        rc, _ = _call(L, N, M, args, tb)
        assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), off
    for off in (4, 8, 12):                                       # core is 32-bit words: 4 bytes are enough
        args = list(GOOD)
        args[NAMES.index("core")] += off
        rc, _ = _call(L, N, M, args, 0)
        assert rc == _native.GHS_E_NOMEM, off


def test_overlapping_pointers_rejected():
    L = _native.load()
    tb = L.ghs_mutual_reach_workspace_bytes(N, M)
    u, v, w, core, w_out, ws = GOOD
    for shift in (16, 4 * M - 16, -16, -(4 * M - 16)):           # w_out inside w's range, not equal to it
        rc, _ = _call(L, N, M, (u, v, w, core, w + shift, ws), tb)
        assert rc == _native.GHS_E_ARG and b"overlap" in L.ghs_last_error(), shift
    for shift in (4 * M, -4 * M):                                # adjacent is fine
        rc, _ = _call(L, N, M, (u, v, w, core, w + shift, ws), 0)
        assert rc == _native.GHS_E_NOMEM, shift
    rc, _ = _call(L, N, M, (u, v, w, core, w, ws), 0)            # exactly w: in place
    assert rc == _native.GHS_E_NOMEM
    for k, name in enumerate(("u", "v", "w")):                   # core over any input
        for shift in (0, 4, 4 * M - 4, -(4 * N - 4)):
            rc, _ = _call(L, N, M, (u, v, w, GOOD[k] + shift, w_out, ws), tb)
            assert rc == _native.GHS_E_ARG and b"overlap" in L.ghs_last_error(), (name, shift)
        for shift in (4 * M, -4 * N):
            rc, _ = _call(L, N, M, (u, v, w, GOOD[k] + shift, w_out, ws), 0)
            assert rc == _native.GHS_E_NOMEM, (name, shift)
    for other in (u, v, core):                                   # w_out over u, v or core
        rc, _ = _call(L, N, M, (u, v, w, core, other, ws), tb)
        assert rc == _native.GHS_E_ARG and b"overlap" in L.ghs_last_error()


def test_short_workspace():
    L = _native.load()
    tb = L.ghs_mutual_reach_workspace_bytes(5000, 40000)
    for short in (0, 1, tb - 1):
        rc, _ = _call(L, 5000, 40000, GOOD, short)
        assert rc == _native.GHS_E_NOMEM, short


def test_no_vertices_is_ok_with_null_pointers():
    L = _native.load()
    rc, res = _call(L, 0, 0, (None,) * 6, 0)
    assert rc == _native.GHS_OK
    assert all(v == 0 for v in res.as_dict().values())
    rc, _ = _call(L, 0, 0, (None,) * 6, 0, k=0)
    assert rc == _native.GHS_E_ARG                               # still an argument error
    rc, _ = _call(L, 0, 0, (None,) * 6, 0, res=False)
    assert rc == _native.GHS_E_ARG


def test_host_entry_argument_errors():
    L = _native.load()
    res = _native.MreachResult()
    a = [np.zeros(64, np.uint32) for _ in range(5)]
    u, v, w, core, w_out = (x.ctypes.data for x in a)

    def host(n, m, ptrs, k=2, r=res):
        return L.ghs_mutual_reach_host(n, m, *ptrs[:3], k, *ptrs[3:], ctypes.byref(r) if r is not None else None)
    full = [u, v, w, core, w_out]
    assert host(8, 7, full, k=0) == _native.GHS_E_ARG and b"k" in L.ghs_last_error()
    assert host(8, 1 << 31, full) == _native.GHS_E_ARG and b"2^31" in L.ghs_last_error()
    assert host(8, 7, full, r=None) == _native.GHS_E_ARG
    for k, name in enumerate(("u", "v", "w", "core")):
        args = list(full)
        args[k] = None
        assert host(8, 7, args) == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error(), name
    assert host(8, 7, [u, v, w, core, w + 4]) == _native.GHS_E_ARG and b"overlap" in L.ghs_last_error()
    assert host(8, 7, [u, v, w, w + 8, w_out]) == _native.GHS_E_ARG and b"overlap" in L.ghs_last_error()
    assert host(0, 0, [None] * 5) == _native.GHS_OK and res.isolated == 0
    if _native.device_count() == 0:
        assert host(8, 7, full) == _native.GHS_E_NODEVICE
        assert host(8, 7, [u, v, w, core, None]) == _native.GHS_E_NODEVICE
        assert host(8, 7, [u, v, w, core, w]) == _native.GHS_E_NODEVICE     # in place


def test_python_value_errors_without_a_gpu():
    import torch

    from distributed_ghs_implementation_amd import hdbscan_edges
    from distributed_ghs_implementation_amd.device import DeviceEdges, hdbscan, mutual_reachability
    z = torch.zeros(3, dtype=torch.int32)
    coo = DeviceEdges(3, z, z, z)
    for bad in (0, -1, 2.5, "5", None, 1 << 32):
        with pytest.raises(ValueError, match="min_samples"):
            mutual_reachability(coo, min_samples=bad)
        with pytest.raises(ValueError, match="min_samples"):
            coo.mutual_reachability(min_samples=bad)
    with pytest.raises(ValueError, match="short_rows"):
        mutual_reachability(coo, short_rows="drop")
    with pytest.raises(ValueError, match="short_rows"):
        hdbscan(coo, short_rows="infinite")
    with pytest.raises(ValueError, match="min_samples"):
        hdbscan(coo, min_samples=0)
    with pytest.raises(ValueError, match="min_cluster_size"):
        hdbscan(coo, min_cluster_size=1)
    with pytest.raises(ValueError, match="method"):
        coo.hdbscan(method="dbscan")
    with pytest.raises(ValueError, match="COO"):
        mutual_reachability(DeviceEdges(3, None, z, z, off=torch.zeros(4, dtype=torch.int32)))
    e = np.zeros(2, np.int64)
    with pytest.raises(ValueError, match="min_samples"):
        hdbscan_edges(3, e, e, e, min_samples=0)
    with pytest.raises(ValueError, match="short_rows"):
        hdbscan_edges(3, e, e, e, short_rows="no")
    with pytest.raises(ValueError, match="min_cluster_size"):
        hdbscan_edges(3, e, e, e, min_cluster_size=1)
    assert _native.mreach_args(5, "error") == 5 and _native.mreach_args(5, "clamp", include_self=True) == 4
    assert _native.mreach_args(1, "error", include_self=True) == 0
    assert _native.mreach_args(np.int64(7), "clamp") == 7


@pytest.mark.skipif(_native.device_count() > 0, reason="CPU-only behaviour")
def test_no_cpu_fallback_without_gpu():
    import torch

    from distributed_ghs_implementation_amd.device import DeviceEdges, hdbscan, mutual_reachability
    u = torch.tensor([0, 1], dtype=torch.int32)
    v = torch.tensor([1, 2], dtype=torch.int32)
    w = torch.tensor([3, 4], dtype=torch.int32)
    for call in (lambda: mutual_reachability(DeviceEdges(3, u, v, w), min_samples=1),
                 lambda: mutual_reachability(DeviceEdges(3, u, v, w), min_samples=1, include_self=True),
                 lambda: hdbscan(DeviceEdges(3, u, v, w), min_cluster_size=2)):
        with pytest.raises(_native.GHSError) as ei:
            call()
        assert ei.value.code == _native.GHS_E_NODEVICE


def test_cli_options_without_a_gpu(capsys, tmp_path):
    from distributed_ghs_implementation_amd.__main__ import main
    cases = ((["--min-samples", "5"], "--min-samples needs --hdbscan OUT.npz or --mutual-reachability OUT.npz"),
             (["--hdbscan", "o.npz", "--min-samples", "0"], "--min-samples K needs K >= 1"),
             (["--hdbscan", "o.npz", "--min-cluster-size", "1"], "--min-cluster-size K with K >= 2"),
             (["--hdbscan", "o.npz", "--short-rows", "drop"], "invalid choice"),
             (["--min-cluster-size", "5"], "--min-cluster-size needs --clusters OUT.npz"))     # as before
    for argv, text in cases:
        with pytest.raises(SystemExit) as ei:
            main(["--graph-dir", "nowhere"] + argv)
        assert ei.value.code == 2, argv
        assert text in capsys.readouterr().err, argv
    # these pass the option checks: the next failure is the missing graph directory, not argparse's exit
    for argv in (["--hdbscan", str(tmp_path / "h.npz")],
                 ["--hdbscan", str(tmp_path / "h.npz"), "--min-samples", "3", "--min-cluster-size", "5", "--cluster-method",
                  "leaf", "--allow-single-cluster", "--short-rows", "clamp"],
                 ["--mutual-reachability", str(tmp_path / "m.npz"), "--min-samples", "7"]):
        with pytest.raises(Exception) as ei:
            main(["--graph-dir", str(tmp_path / "nowhere")] + argv)
        assert not isinstance(ei.value, SystemExit), argv
        capsys.readouterr()


def test_mreach_hip_stands_alone():
    """csrc/mreach.hip includes no project source but common.h, launches only kernels it defines (all named
    k_mr_*), shares no kernel name with any other file of csrc/, checks canonicity before its first launch,
    selects without a loop over k, and is compiled without fast-math."""
    src = open(MREACH_HIP).read()
    assert re.findall(r'^\s*#\s*include\s+"([^"]+)"', src, re.M) == ["common.h"]
    for inc in re.findall(r"^\s*#\s*include\s+<([^>]+)>", src, re.M):
        assert inc.startswith(("hip/", "rocprim/")) or "/" not in inc, inc  # HIP, rocPRIM, the C++ library
    launched = set(re.findall(r"\b(k_\w+)\s*(?:<[^<>]*>)?\s*<<<", src))
    defined = set(re.findall(r"(?:__global__|GHS_STREAM_KERNEL)[^;{]*?\bvoid\s+(k_\w+)\s*\(", src, re.S))
    assert launched and launched == defined, launched ^ defined
    assert all(k.startswith("k_mr_") for k in defined), defined
    first = min(src.index(k + "<<<") for k in launched)
    assert src.index("ghs_check_canonical(n, m64") < first       # no index is formed from an unchecked list
    assert "GHS_STREAM_KERNEL void k_mr_reweight" in src         # the project's streaming shape
    assert "__ballot" in src and "__popcll" in src               # the register select counts, it does not extract
    other = ""
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")) and name != "mreach.hip":
            other += open(os.path.join(CSRC, name)).read()
    for part in sorted(os.listdir(os.path.join(CSRC, "boruvka"))):
        other += open(os.path.join(CSRC, "boruvka", part)).read()
    other_kernels = set(re.findall(r"\bvoid\s+(k_\w+)\s*\(", other))
    assert other_kernels and not (defined & other_kernels)
    assert not re.search(r"\bk_mr_\w*", other)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "fast-math" not in mk and "-Ofast" not in mk


def test_makefile_links_mreach_everywhere():
    lines = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ").split("\n")
    objs = [ln for ln in lines if re.match(r"OBJS\s*:=", ln)]
    assert len(objs) == 1 and "$(OUTDIR)/mreach.o" in objs[0] and "$(OUTDIR)/cluster.o" in objs[0]
    prereq = [ln for ln in lines if ln.startswith("rcclstub:")]
    assert len(prereq) == 1 and "$(OUTDIR)/mreach.o" in prereq[0]     # the target's prerequisites
    link = [ln for ln in lines if ln.startswith("\t") and "-o $(STUB)/libghs_mst_rcclstub.so" in ln]
    assert len(link) == 1 and "$(OUTDIR)/mreach.o" in link[0]         # and its link line
