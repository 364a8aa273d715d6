"""The cluster-extraction entry points' C-ABI boundary without a GPU (ghs_forest_cluster_workspace_bytes /
ghs_forest_cluster_capacity / ghs_forest_cluster_device / ghs_forest_cluster_host): the result's layout,
every argument check that comes before any device work, the workspace and capacity tables, the n == 0
answer, the Python layers' ValueErrors, and the independence of csrc/cluster.hip from every other
translation unit."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from distributed_ghs_implementation_amd import _native

# host addresses standing in for device pointers: every check below fails before anything is read
BASE = 1 << 20
INS = ("leaf_parent", "merge_parent", "child_a", "child_b", "size", "height")
OUTS = ("label", "probability", "point_cluster", "point_lambda", "cluster_head", "cluster_parent", "cluster_size",
        "cluster_birth", "cluster_stability", "cluster_selected")
NAMES = INS + OUTS + ("ws",)
GOOD = tuple(BASE + (k << 16) for k in range(len(NAMES)))
OPTIONAL = ("probability", "point_lambda")
WORDS = ("leaf_parent", "merge_parent", "child_a", "child_b", "size", "label", "point_cluster", "cluster_head",
         "cluster_parent", "cluster_size")
DOUBLES = ("height", "probability", "point_lambda", "cluster_birth", "cluster_stability")
CSRC = os.path.join(ROOT, "distributed_ghs_implementation_amd", "csrc")
CLUSTER_HIP = os.path.join(CSRC, "cluster.hip")
SYMBOLS = {"ghs_forest_cluster_workspace_bytes", "ghs_forest_cluster_capacity", "ghs_forest_cluster_device",
           "ghs_forest_cluster_host"}


def _call(L, n, t, ptrs, ws_bytes, mcs=5, flags=0):
    res = _native.ClusterResult()
    rc = L.ghs_forest_cluster_device(n, t, *ptrs[:6], mcs, flags, *ptrs[6:16], ptrs[16], ws_bytes, None, ctypes.byref(res))
    return rc, res


def test_result_layout_symbols_and_header():
    R = _native.ClusterResult
    assert ctypes.sizeof(R) == 40
    assert [f for f, _ in R._fields_] == ["num_clusters", "num_selected", "num_noise", "num_top", "cluster_height",
                                          "rounds", "select_launches", "reserved", "ms_total"]
    assert [getattr(R, f).offset for f, _ in R._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32]
    assert SYMBOLS <= set(_native.EXPORTED_SYMBOLS)
    L = _native.load()
    for s in SYMBOLS:
        assert getattr(L, s) is not None
    assert L.ghs_abi_version() == 10 and _native.ABI_VERSION == 10
    header = open(os.path.join(ROOT, "include", "ghs_mst.h")).read()
    assert re.search(r"#define\s+GHS_MST_ABI_VERSION\s+10\b", header)
    for s in SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", header), s
    assert "/* 40 bytes */" in header[header.index("typedef struct ghs_cluster_result"):][:80]
    assert header.index("ghs_forest_dendro_host(") < header.index("typedef struct ghs_cluster_result")  # after the dendrogram
    assert header.index("} ghs_cluster_result_t;") < header.index("int ghs_check_canonical(")
    body = header[header.index("typedef struct ghs_cluster_result"): header.index("} ghs_cluster_result_t;")]
    order = [body.index(f) for f, _ in R._fields_]
    assert order == sorted(order)  # the header declares the fields in the same order
    for name in ("d_" + k for k in NAMES[:-1]):
        assert name in header, name
    assert re.search(r"#define\s+GHS_CLUSTER_ALLOW_SINGLE\s+1u", header) and _native.GHS_CLUSTER_ALLOW_SINGLE == 1
    assert re.search(r"#define\s+GHS_CLUSTER_LEAF\s+2u", header) and _native.GHS_CLUSTER_LEAF == 2
    assert "zero" in header[header.index("HDBSCAN cluster extraction"):header.index("typedef struct ghs_cluster_result")]
    d = R().as_dict()
    assert set(d) == {f for f, _ in R._fields_} - {"reserved"}


def test_capacity_and_workspace_tables_without_a_gpu():
    L = _native.load()
    C, W = L.ghs_forest_cluster_capacity, L.ghs_forest_cluster_workspace_bytes
    ns = (1, 2, 7, 1023, 1024, 1025, 4095, 4096, 4097, 100000, 1 << 20, 1 << 24, 1 << 31)
    ts = (0, 1, 2, 1023, 1024, 1025, 4096, 1 << 20, (1 << 24) - 1, 1 << 31)
    for mcs in (2, 3, 5, 64, 100):
        for n in ns:
            for t in ts:
                assert C(n, t, mcs) == min(t, 2 * (n // mcs)), (n, t, mcs)
        table = [[W(n, t, mcs) for t in ts] for n in ns]
        for i, n in enumerate(ns):
            assert table[i] == sorted(table[i]), (n, mcs)        # nondecreasing in t
        for j, t in enumerate(ts):
            col = [table[i][j] for i in range(len(ns))]
            assert col == sorted(col), (t, mcs)                  # nondecreasing in n
            for i, n in enumerate(ns):
                assert table[i][j] >= 24 * n + 16 * t + 84 * C(n, t, mcs) + 1024, (n, t, mcs)
    # 16 B per merge + 24 B per vertex + 84 B per cluster of capacity + the sort's storage, not more
    n, t = 1 << 24, (1 << 24) - 1
    assert W(n, t, 5) < 16 * t + 24 * n + 84 * C(n, t, 5) + 12 * n + (1 << 22)
    assert W(n, t, 100) < W(n, t, 5) < W(n, t, 2)
    assert C(10, 9, 1) == 0 and C(10, 9, 0) == 0                 # no such min_cluster_size
    assert W(0, 0, 5) == 0 and W(10, 9, 1) == 0 and W(1 << 31, (1 << 31) + 1, 5) == 0


def test_argument_errors_come_before_device_work():
    L = _native.load()
    tb = L.ghs_forest_cluster_workspace_bytes(50, 40, 5)
    for mcs in (0, 1):
        rc, _ = _call(L, 50, 40, GOOD, tb, mcs=mcs)
        assert rc == _native.GHS_E_ARG and b"min_cluster_size" in L.ghs_last_error()
    rc, _ = _call(L, 50, 40, GOOD, tb, flags=4)
    assert rc == _native.GHS_E_ARG and b"flags" in L.ghs_last_error()
    for n, t in ((1 << 31, (1 << 31) + 1), ((1 << 32) - 1, 2), (5, 1 << 40)):
        rc, _ = _call(L, n, t, GOOD, 1 << 60)
        assert rc == _native.GHS_E_ARG and b"32 bits" in L.ghs_last_error(), (n, t)
    assert L.ghs_forest_cluster_device(50, 40, *GOOD[:6], 5, 0, *GOOD[6:16], GOOD[16], tb, None, None) == _native.GHS_E_ARG
    assert b"NULL" in L.ghs_last_error()


def test_null_pointers_rejected_before_device_work():
    L = _native.load()
    tb = L.ghs_forest_cluster_workspace_bytes(50, 40, 5)
    for k, name in enumerate(NAMES):
        args = list(GOOD)
        args[k] = None
        rc, _ = _call(L, 50, 40, args, tb if name != "ws" else 0)
        if name in OPTIONAL:
            if _native.device_count() == 0:
                assert rc == _native.GHS_E_NODEVICE, name     # every check passed without it
            continue
        assert rc == _native.GHS_E_ARG, name                  # not GHS_E_NODEVICE: the check comes first
        assert b"NULL" in L.ghs_last_error()
    # t == 0 needs label, point_cluster and the workspace only
    few = [None] * 17
    rc, _ = _call(L, 5, 0, few, 0)
    assert rc == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error()
    few[NAMES.index("label")], few[NAMES.index("point_cluster")], few[16] = GOOD[6], GOOD[8], GOOD[16]
    tb0 = L.ghs_forest_cluster_workspace_bytes(5, 0, 5)
    rc, _ = _call(L, 5, 0, few, tb0 - 1)
    assert rc == _native.GHS_E_NOMEM
    if _native.device_count() == 0:
        rc, _ = _call(L, 5, 0, few, tb0)
        assert rc == _native.GHS_E_NODEVICE


def test_misaligned_pointers_rejected():
    L = _native.load()
    tb = L.ghs_forest_cluster_workspace_bytes(50, 40, 5)
    for name in WORDS:
        for off in (1, 2, 3):
            args = list(GOOD)
            args[NAMES.index(name)] += off
            rc, _ = _call(L, 50, 40, args, tb)
            assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), (name, off)
    for name in DOUBLES:
        for off in (1, 2, 4, 6):
            args = list(GOOD)
            args[NAMES.index(name)] += off
            rc, _ = _call(L, 50, 40, args, tb)
            assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), (name, off)
    for off in (1, 4, 8, 12):
        args = list(GOOD)
        args[16] += off
        rc, _ = _call(L, 50, 40, args, tb)
        assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), off
    for off in (1, 3, 7):  # cluster_selected is bytes: any alignment passes the pointer checks
        args = list(GOOD)
        args[NAMES.index("cluster_selected")] += off
        rc, _ = _call(L, 50, 40, args, 0)
        assert rc == _native.GHS_E_NOMEM, off


def test_short_workspace():
    L = _native.load()
    tb = L.ghs_forest_cluster_workspace_bytes(5000, 4999, 5)
    for short in (0, 1, tb - 1):
        rc, _ = _call(L, 5000, 4999, GOOD, short)
        assert rc == _native.GHS_E_NOMEM, short


def test_no_vertices_is_ok_with_null_pointers():
    L = _native.load()
    rc, res = _call(L, 0, 0, (None,) * 17, 0)
    assert rc == _native.GHS_OK
    assert all(v == 0 for k, v in res.as_dict().items())
    rc, _ = _call(L, 0, 0, (None,) * 17, 0, mcs=1)
    assert rc == _native.GHS_E_ARG                               # still an argument error


def test_host_entry_argument_errors():
    L = _native.load()
    res = _native.ClusterResult()
    a = np.zeros(64, np.uint32)
    f = np.zeros(64, np.float64)
    b = np.zeros(64, np.uint8)
    p, fp, bp = a.ctypes.data, f.ctypes.data, b.ctypes.data
    full = [p, p, p, p, p, fp, p, fp, p, fp, p, p, p, fp, fp, bp]

    def host(n, t, ptrs, mcs=2, flags=0, r=res):
        return L.ghs_forest_cluster_host(n, t, *ptrs[:6], mcs, flags, *ptrs[6:], ctypes.byref(r) if r is not None else None)
    assert host(8, 7, full, mcs=1) == _native.GHS_E_ARG and b"min_cluster_size" in L.ghs_last_error()
    assert host(8, 7, full, flags=8) == _native.GHS_E_ARG and b"flags" in L.ghs_last_error()
    assert host(1 << 31, (1 << 31) + 1, full) == _native.GHS_E_ARG and b"32 bits" in L.ghs_last_error()
    for k, name in enumerate(NAMES[:-1]):
        args = list(full)
        args[k] = None
        rc = host(8, 7, args)
        if name in OPTIONAL:
            if _native.device_count() == 0:
                assert rc == _native.GHS_E_NODEVICE, name
            continue
        assert rc == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error(), name
    assert host(8, 7, full, r=None) == _native.GHS_E_ARG
    assert host(0, 0, [None] * 16) == _native.GHS_OK and res.num_clusters == 0
    if _native.device_count() == 0:
        assert host(8, 7, full) == _native.GHS_E_NODEVICE


def test_python_value_errors_without_a_gpu():
    import torch

    from distributed_ghs_implementation_amd.device import Dendrogram, DeviceEdges, forest_clusters
    z = torch.zeros(3, dtype=torch.int32)
    one = torch.zeros(1, dtype=torch.int32)
    h = torch.ones(1, dtype=torch.float64)
    coo = DeviceEdges(3, z, z, z)
    good = Dendrogram(2, z[:2], one, one, one, one, one, info={"is_forest": True})
    with pytest.raises(ValueError, match="exactly one"):
        forest_clusters(good)
    with pytest.raises(ValueError, match="exactly one"):
        forest_clusters(good, edges=coo, heights=h)
    with pytest.raises(ValueError, match="children"):
        forest_clusters(Dendrogram(2, z[:2], one, one, None, None, one), heights=h)
    with pytest.raises(ValueError, match="children"):
        forest_clusters(Dendrogram(2, z[:2], one, one, one, one, None), heights=h)
    with pytest.raises(ValueError, match="cycle"):
        forest_clusters(Dendrogram(2, z[:2], one, one, one, one, one, info={"is_forest": False}), heights=h)
    with pytest.raises(ValueError, match="min_cluster_size"):
        forest_clusters(good, heights=h, min_cluster_size=1)
    with pytest.raises(ValueError, match="method"):
        forest_clusters(good, heights=h, method="dbscan")
    with pytest.raises(ValueError, match="exactly one"):
        good.clusters(None)
    assert _native.cluster_args(5, "eom", False) == (5, 0)
    assert _native.cluster_args(2, "leaf", True) == (2, _native.GHS_CLUSTER_LEAF | _native.GHS_CLUSTER_ALLOW_SINGLE)


@pytest.mark.skipif(_native.device_count() > 0, reason="CPU-only behaviour")
def test_no_cpu_fallback_without_gpu():
    import torch

    from distributed_ghs_implementation_amd import canonicalize
    from distributed_ghs_implementation_amd.device import Dendrogram, forest_clusters
    from distributed_ghs_implementation_amd.mst import MSTResult
    z = torch.zeros(2, dtype=torch.int32)
    one = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_native.GHSError) as ei:
        forest_clusters(Dendrogram(2, z, one, one, one, one, one), heights=torch.ones(1, dtype=torch.float64),
                        min_cluster_size=2)
    assert ei.value.code == _native.GHS_E_NODEVICE
    g = canonicalize(3, edges=[(0, 1, 1), (1, 2, 2)])
    with pytest.raises(_native.GHSError) as ei:
        MSTResult(g, np.ones(2, bool), 3, 1, [], 0.0).clusters(min_cluster_size=2)
    assert ei.value.code == _native.GHS_E_NODEVICE
    with pytest.raises(ValueError, match="min_cluster_size"):
        MSTResult(g, np.ones(2, bool), 3, 1, [], 0.0).clusters(min_cluster_size=1)


def test_cli_options_without_a_gpu(capsys, tmp_path):
    """--clusters keeps its integer meaning with --labels; a file name asks for --min-cluster-size."""
    from distributed_ghs_implementation_amd.__main__ import main
    cases = ((["--clusters", "out.npz"], "--clusters OUT.npz needs --min-cluster-size"),
             (["--clusters", "out.npz", "--min-cluster-size", "1"], "--clusters OUT.npz needs --min-cluster-size"),
             (["--clusters", "3x"], "--clusters OUT.npz needs --min-cluster-size"),       # a mistyped K is a file name
             (["--min-cluster-size", "5"], "--min-cluster-size needs --clusters OUT.npz"),
             (["--clusters", "3", "--min-cluster-size", "5", "--labels", "x.npy"], "--min-cluster-size needs --clusters OUT.npz"),
             (["--clusters", "3"], "need --labels"),                                      # the integer form, as before
             (["--clusters", "3", "--max-weight", "2", "--labels", "x.npy"], "exclude each other"))
    for argv, text in cases:
        with pytest.raises(SystemExit) as ei:
            main(["--graph-dir", "nowhere"] + argv)
        assert ei.value.code == 2, argv
        assert text in capsys.readouterr().err, argv
    # both forms pass the option checks: the next failure is the missing graph directory, not argparse's exit
    for argv in (["--clusters", "3", "--labels", str(tmp_path / "x.npy")],
                 ["--clusters", str(tmp_path / "c.npz"), "--min-cluster-size", "5", "--cluster-method", "leaf",
                  "--allow-single-cluster"]):
        with pytest.raises(Exception) as ei:
            main(["--graph-dir", str(tmp_path / "nowhere")] + argv)
        assert not isinstance(ei.value, SystemExit), argv
        capsys.readouterr()


def test_cluster_hip_stands_alone():
    """csrc/cluster.hip includes no project source but common.h, launches only kernels it defines (all
    named k_cl_*), shares no kernel name with any other file of csrc/, validates before anything else
    runs, and is compiled without fast-math."""
    src = open(CLUSTER_HIP).read()
    assert re.findall(r'^\s*#\s*include\s+"([^"]+)"', src, re.M) == ["common.h"]
    for inc in re.findall(r"^\s*#\s*include\s+<([^>]+)>", src, re.M):
        assert inc.startswith(("hip/", "rocprim/")) or "/" not in inc, inc  # HIP, rocPRIM, the C++ library
    launched = set(re.findall(r"\b(k_\w+)\s*(?:<[^<>]*>)?\s*<<<", src))
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src, re.S))
    assert launched and launched <= defined, launched - defined
    assert all(k.startswith("k_cl_") for k in defined), defined
    first = min(src.index(k + "<<<") for k in launched)
    assert first == src.index("k_cl_validate<<<")                # nothing follows a pointer before it
    assert "atomicAdd(double" not in src and not re.search(r"atomicAdd\(\s*&?\s*c_stab", src)
    other = ""
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")) and name != "cluster.hip":
            other += open(os.path.join(CSRC, name)).read()
    for part in sorted(os.listdir(os.path.join(CSRC, "boruvka"))):
        other += open(os.path.join(CSRC, "boruvka", part)).read()
    other_kernels = set(re.findall(r"\bvoid\s+(k_\w+)\s*\(", other))
    assert other_kernels and not (defined & other_kernels)
    assert not re.search(r"\bk_cl_\w*", other)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "fast-math" not in mk and "-Ofast" not in mk


def test_makefile_links_cluster_everywhere():
    lines = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ").split("\n")
    objs = [ln for ln in lines if re.match(r"OBJS\s*:=", ln)]
    assert len(objs) == 1 and "$(OUTDIR)/cluster.o" in objs[0] and "$(OUTDIR)/dendro.o" in objs[0]
    prereq = [ln for ln in lines if ln.startswith("rcclstub:")]
    assert len(prereq) == 1 and "$(OUTDIR)/cluster.o" in prereq[0]    # the target's prerequisites
    link = [ln for ln in lines if ln.startswith("\t") and "-o $(STUB)/libghs_mst_rcclstub.so" in ln]
    assert len(link) == 1 and "$(OUTDIR)/cluster.o" in link[0]        # and its link line
