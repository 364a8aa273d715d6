"""The replacement-edge entry points' C-ABI boundary without a GPU (ghs_forest_paths_info,
ghs_forest_replace_workspace_bytes / _device / _host): the structs' layouts, every argument check that
comes before any device work, the workspace size, the n == 0 answers, the Python layer's ValueErrors,
the independence of csrc/replace.hip from every other translation unit, and the GPU tests' walk oracle
against the definition itself."""
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
U, V, W, REPL, BYEDGE, WS = (BASE + (k << 16) for k in range(6))
CSRC = os.path.join(ROOT, "distributed_ghs_implementation_amd", "csrc")
REPLACE_HIP = os.path.join(CSRC, "replace.hip")
SYMBOLS = {"ghs_forest_paths_info", "ghs_forest_replace_workspace_bytes", "ghs_forest_replace_device",
           "ghs_forest_replace_host", "ghs_forest_replace_phases"}
NONE = 0xFFFFFFFF


def _empty_handle(L):
    r = _native.PathsResult()
    h = ctypes.c_void_p(0)
    rc = L.ghs_forest_paths_create(0, 0, None, None, None, None, None, None, 0, None, 0, None, ctypes.byref(r), ctypes.byref(h))
    assert rc == _native.GHS_OK and h.value
    return h


def _replace(L, h, m=3, u=U, v=V, w=W, repl=REPL, by_edge=BYEDGE, ws=WS, wbytes=256, res=True):
    r = _native.ReplaceResult()
    rc = L.ghs_forest_replace_device(h, m, u, v, w, repl, by_edge, ws, wbytes, None, ctypes.byref(r) if res else None)
    return rc, r


def test_struct_layouts_symbols_and_header():
    R, I = _native.ReplaceResult, _native.PathsInfo
    assert ctypes.sizeof(R) == 64 and ctypes.sizeof(I) == 32
    assert [f for f, _ in R._fields_] == ["tree_edges", "covering_edges", "cross_edges", "bridges", "improving",
                                          "best_delta", "best_out_eid", "best_in_eid", "ms_total", "reserved"]
    assert [getattr(R, f).offset for f, _ in R._fields_] == [0, 8, 16, 24, 28, 32, 40, 44, 48, 56]
    assert R._fields_[5][1] is ctypes.c_int64
    assert [f for f, _ in I._fields_] == ["n", "levels", "max_depth", "d_index"]
    assert [getattr(I, f).offset for f, _ in I._fields_] == [0, 8, 16, 24]
    assert set(R().as_dict()) == {f for f, _ in R._fields_} - {"reserved"}
    assert SYMBOLS <= set(_native.EXPORTED_SYMBOLS)
    L = _native.load()
    for s in SYMBOLS:
        assert getattr(L, s) is not None
    assert L.ghs_abi_version() == 10 and _native.ABI_VERSION == 10  # additions only
    header = open(os.path.join(ROOT, "include", "ghs_mst.h")).read()
    assert re.search(r"#define\s+GHS_MST_ABI_VERSION\s+10\b", header)
    for s in SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", header), s
    assert "typedef struct ghs_replace_result {   /* 64 bytes */" in header
    assert header.index("ghs_forest_paths_host(") < header.index("typedef struct ghs_paths_info")
    assert header.index("typedef struct ghs_paths_info") < header.index("typedef struct ghs_replace_result")
    nm = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    exported = {ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip()}
    assert SYMBOLS <= exported, SYMBOLS - exported


def test_workspace_bytes_without_a_gpu():
    L = _native.load()

    def want(n, d):
        k = max(1, int(d).bit_length())
        return (8 * (k - 1) * n + 255) // 256 * 256 + 256
    for n in (0, 1, 2, 31, 32, 33, 1000, 1 << 20, (1 << 32) - 1):
        for d in (0, 1, 2, 3, 4, 255, 256, 32767, 32768, 65535, (1 << 32) - 2):
            assert L.ghs_forest_replace_workspace_bytes(n, d) == want(n, d), (n, d)
    # K = 1: the status block alone; K = 2: one level; K = 16 (the 4096^2 grid, 39 854 deep): 15 levels
    assert L.ghs_forest_replace_workspace_bytes(1000, 1) == 256
    assert L.ghs_forest_replace_workspace_bytes(1000, 0) == 256
    assert L.ghs_forest_replace_workspace_bytes(1000, 2) == 8 * 1000 + 192 + 256
    assert L.ghs_forest_replace_workspace_bytes(1000, 3) == 8 * 1000 + 192 + 256
    assert L.ghs_forest_replace_workspace_bytes(4096 * 4096, 39854) == 8 * 15 * 4096 * 4096 + 256


def test_paths_info_on_the_empty_handle():
    L = _native.load()
    h = _empty_handle(L)
    pi = _native.PathsInfo(n=7, levels=7, max_depth=7, d_index=7)
    assert L.ghs_forest_paths_info(h, ctypes.byref(pi)) == _native.GHS_OK
    assert pi.as_dict() == {"n": 0, "levels": 0, "max_depth": 0, "d_index": 0}
    assert L.ghs_forest_paths_info(h, None) == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error()
    assert L.ghs_forest_paths_info(None, ctypes.byref(pi)) == _native.GHS_E_ARG and b"handle" in L.ghs_last_error()
    assert L.ghs_forest_paths_destroy(h) == _native.GHS_OK


def test_phase_times_are_opt_in_and_need_no_gpu():
    L = _native.load()
    ms = (ctypes.c_double * 4)(7, 7, 7, 7)
    assert L.ghs_forest_replace_phases(0, ms) == _native.GHS_OK and list(ms) == [0.0] * 4  # nothing recorded yet
    assert L.ghs_forest_replace_phases(1, None) == _native.GHS_OK
    h = _empty_handle(L)
    assert _replace(L, h, m=0, u=None, v=None, w=None)[0] == _native.GHS_OK   # no device work: nothing to time
    assert L.ghs_forest_replace_phases(0, ms) == _native.GHS_OK and list(ms) == [0.0] * 4
    assert L.ghs_forest_paths_destroy(h) == _native.GHS_OK


def test_device_entry_argument_checks_in_order():
    L = _native.load()
    h = _empty_handle(L)
    # the handle first, then the result, then m, then the pointers, then the workspace size
    rc, _ = _replace(L, None, m=1 << 31, u=None, wbytes=0)
    assert rc == _native.GHS_E_ARG and b"handle" in L.ghs_last_error()
    rc, _ = _replace(L, h, m=1 << 31, u=None, wbytes=0, res=False)
    assert rc == _native.GHS_E_ARG and b"result" in L.ghs_last_error()
    for m in (1 << 31, 1 << 40):
        rc, _ = _replace(L, h, m=m, u=None, wbytes=0)
        assert rc == _native.GHS_E_ARG and b"2^31" in L.ghs_last_error()
    for name in ("u", "v", "w", "ws"):
        rc, _ = _replace(L, h, wbytes=0, **{name: None})
        assert rc == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error(), name
    for name, base in (("u", U), ("v", V), ("w", W), ("ws", WS)):  # 16 bytes
        for off in (1, 4, 8, 12):
            rc, _ = _replace(L, h, wbytes=0, **{name: base + off})
            assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), (name, off)
    for off in (1, 2, 4, 6):  # d_repl: 8 bytes
        rc, _ = _replace(L, h, wbytes=0, repl=REPL + off)
        assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), off
    for off in (1, 2, 3):  # the per-edge array: 4 bytes
        rc, _ = _replace(L, h, wbytes=0, by_edge=BYEDGE + off)
        assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), off
    # offsets that keep the alignment, and a NULL per-edge array, pass on to the next check: the size
    for kw in ({"repl": REPL + 8}, {"by_edge": BYEDGE + 4}, {"by_edge": None}, {"u": U + 16}):
        assert _replace(L, h, wbytes=255, **kw)[0] == _native.GHS_E_NOMEM, kw
    for short in (0, 1, 255):
        rc, _ = _replace(L, h, wbytes=short)
        assert rc == _native.GHS_E_NOMEM and b"workspace" in L.ghs_last_error()
    # m == 0: the edge pointers may be NULL; an index over no vertices: nothing to write, GHS_OK
    rc, r = _replace(L, h, m=0, u=None, v=None, w=None, repl=None, by_edge=None)
    assert rc == _native.GHS_OK
    assert (r.tree_edges, r.covering_edges, r.cross_edges, r.bridges, r.improving, r.best_delta) == (0,) * 6
    assert (r.best_out_eid, r.best_in_eid, r.reserved) == (NONE, NONE, 0)
    # edges over no vertices: every endpoint is out of range
    rc, _ = _replace(L, h)
    assert rc == _native.GHS_E_ARG and b"out of range" in L.ghs_last_error()
    # a second live handle is independent of the first one's destruction
    h2 = _empty_handle(L)
    assert L.ghs_forest_paths_destroy(h) == _native.GHS_OK
    assert _replace(L, h2, m=0, u=None, v=None, w=None)[0] == _native.GHS_OK
    assert L.ghs_forest_paths_destroy(h2) == _native.GHS_OK


def test_host_entry_argument_checks():
    L = _native.load()
    res = _native.ReplaceResult()
    z = np.zeros(8, np.uint32)
    f = np.zeros(8, np.uint8)
    k8 = np.zeros(8, np.uint64)
    p, fp, kp = z.ctypes.data, f.ctypes.data, k8.ctypes.data

    def host(n, m, u, v, w, fl, repl, by_edge, r=res):
        return L.ghs_forest_replace_host(n, m, u, v, w, fl, repl, by_edge, ctypes.byref(r) if r is not None else None)
    assert host(5, 3, p, p, p, fp, kp, p, r=None) == _native.GHS_E_ARG and b"result" in L.ghs_last_error()
    assert host(5, 1 << 31, p, p, p, fp, kp, p) == _native.GHS_E_ARG and b"2^31" in L.ghs_last_error()
    for k in range(4):  # u, v, w, flags
        args = [p, p, p, fp]
        args[k] = None
        assert host(5, 3, *args, kp, p) == _native.GHS_E_ARG and b"NULL" in L.ghs_last_error(), k
    # no vertices: GHS_OK with no device work
    assert host(0, 0, None, None, None, None, None, None) == _native.GHS_OK
    assert (res.tree_edges, res.bridges, res.best_out_eid, res.best_in_eid) == (0, 0, NONE, NONE)
    if _native.device_count() == 0:  # every argument is fine: only now the missing device is reported
        assert host(5, 3, p, p, p, fp, kp, p) == _native.GHS_E_NODEVICE
        assert host(5, 3, p, p, p, fp, None, None) == _native.GHS_E_NODEVICE
        assert host(5, 3, None, p, p, fp, kp, p) == _native.GHS_E_ARG  # and a bad argument still wins over it


def test_python_value_errors_without_a_gpu():
    import torch

    from distributed_ghs_implementation_amd.device import DeviceEdges, PathIndex, forest_replacements
    L = _native.load()
    z = torch.zeros(3, dtype=torch.int32)
    coo = DeviceEdges(3, z, z, z)
    index = PathIndex(_empty_handle(L), None, 3, torch.device("cuda", 0))
    with pytest.raises(ValueError, match="device"):
        forest_replacements(coo, index)            # the edges are on the CPU, the index on a GPU
    with pytest.raises(ValueError, match="device"):
        index.replacements(coo)
    with pytest.raises(ValueError, match="CSR"):
        forest_replacements(DeviceEdges(3, None, z, z, off=torch.zeros(4, dtype=torch.int32)), index)
    index.close()
    with pytest.raises(ValueError, match="closed"):
        forest_replacements(coo, index)
    with pytest.raises(ValueError, match="closed"):
        index.replacements(coo)
    other = PathIndex(_empty_handle(L), None, 4, torch.device("cpu"))
    with pytest.raises(ValueError, match="vertices"):
        forest_replacements(coo, other)            # an index over another vertex count
    other.close()


def test_cli_lists_the_option():
    from distributed_ghs_implementation_amd import __main__ as cli
    assert "--replacements OUT.npz" in cli.__doc__
    with pytest.raises(SystemExit) as ei:
        cli.main(["--replacements"])               # the option takes a file name
    assert ei.value.code == 2


def test_replace_hip_stands_alone():
    """csrc/replace.hip includes no project source but common.h, launches only kernels it defines (all
    named k_rp_*), shares no kernel name with any other file of csrc/, and reaches the index through
    ghs_forest_paths_info alone."""
    src = open(REPLACE_HIP).read()
    assert re.findall(r'^\s*#\s*include\s+"([^"]+)"', src, re.M) == ["common.h"]
    for inc in re.findall(r"^\s*#\s*include\s+<([^>]+)>", src, re.M):
        assert inc.startswith("hip/") or "/" not in inc, inc  # HIP and the C++ library
    launched = set(re.findall(r"\b(k_\w+)\s*(?:<[^<>]*>)?\s*<<<", src))
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src, re.S))
    assert launched and launched == defined, launched ^ defined
    assert all(k.startswith("k_rp_") for k in defined), defined
    other = ""
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")) and name != "replace.hip":
            other += open(os.path.join(CSRC, name)).read()
    for part in sorted(os.listdir(os.path.join(CSRC, "boruvka"))):
        other += open(os.path.join(CSRC, "boruvka", part)).read()
    other_kernels = set(re.findall(r"\bvoid\s+(k_\w+)\s*\(", other))
    assert other_kernels and not (defined & other_kernels)
    assert not re.search(r"\bk_rp_\w+", other)
    assert not (set(re.findall(r"\bk_\w+", src)) - defined)   # and names no other file's kernel
    assert "ghs_forest_paths_info(" in src and "struct ghs_paths {" not in src
    # paths.hip gained the info call and nothing else that launches: still its three kernels
    paths = open(os.path.join(CSRC, "paths.hip")).read()
    assert "ghs_forest_paths_info" in paths
    assert set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", paths, re.S)) == {"k_pa_level0", "k_pa_level", "k_pa_query"}
    # the host form lives in host.hip and goes through the public calls only
    host = open(os.path.join(CSRC, "host.hip")).read()
    assert "ghs_forest_replace_host" in host and "ghs_forest_replace_host" not in src
    assert not re.search(r"\bk_\w+\s*<<<", host[host.index("ghs_forest_replace_host"):])


def test_makefile_links_replace_everywhere():
    lines = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ").split("\n")
    objs = [ln for ln in lines if re.match(r"OBJS\s*:=", ln)]
    assert len(objs) == 1 and "$(OUTDIR)/replace.o" in objs[0] and "$(OUTDIR)/paths.o" in objs[0]
    prereq = [ln for ln in lines if ln.startswith("rcclstub:")]
    assert len(prereq) == 1 and "$(OUTDIR)/replace.o" in prereq[0]     # the target's prerequisites
    link = [ln for ln in lines if ln.startswith("\t") and "-o $(STUB)/libghs_mst_rcclstub.so" in ln]
    assert len(link) == 1 and "$(OUTDIR)/replace.o" in link[0]         # and its link line


# ---- the GPU tests' oracle against the definition ---------------------------------------------------------
def _brute_force(n, u, v, w, flags):
    """repl per forest edge by the definition: delete the edge, split its tree, take the smallest key
    among the non-forest edges that cross the split. -> {eid: key or None}"""
    m = len(u)
    forest = [e for e in range(m) if flags[e]]
    out = {}
    for e in forest:
        adj = {x: [] for x in range(n)}
        for f in forest:
            if f != e:
                adj[int(u[f])].append(int(v[f]))
                adj[int(v[f])].append(int(u[f]))

        def side(r):
            seen, todo = {r}, [r]
            while todo:
                for y in adj[todo.pop()]:
                    if y not in seen:
                        seen.add(y)
                        todo.append(y)
            return seen
        sa, sb = side(int(u[e])), side(int(v[e]))
        assert not (sa & sb)
        keys = [(int(w[f]) << 32) | f for f in range(m) if not flags[f]
                and ((int(u[f]) in sa and int(v[f]) in sb) or (int(u[f]) in sb and int(v[f]) in sa))]
        out[e] = min(keys) if keys else None
    return out


def test_walk_oracle_equals_the_definition():
    from test_gpu_replace import NOKEY, canonical, host_rooted, kruskal_flags, walk_oracle
    rng = np.random.default_rng(2024)
    seen_bridge = seen_cross = seen_improving = 0
    for trial in range(50):
        n = int(rng.integers(2, 31))
        every = [(a, b) for a in range(n) for b in range(a + 1, n)]
        m = int(rng.integers(1, min(len(every), 3 * n) + 1))
        pairs = [every[i] for i in rng.choice(len(every), m, replace=False)]
        u, v, w, _ = canonical(pairs, rng.integers(0, 6 if trial % 2 else 1000, m))
        flags = kruskal_flags(n, u, v, w, heaviest=trial % 5 == 4)   # some forests are not the MSF
        if trial % 3 == 2:                                           # some are not spanning: drop two forest edges
            flags[np.flatnonzero(flags)[:2]] = 0
        repl, by_edge, counts = walk_oracle(n, u, v, w, flags)
        want = _brute_force(n, u, v, w, flags)
        parent, peid, _ = host_rooted(n, u, v, flags)
        assert sorted(want) == sorted(peid[x] for x in range(n) if parent[x] != NONE)
        for x in range(n):
            if parent[x] == NONE:
                assert int(repl[x]) == NOKEY
                continue
            key = want[peid[x]]
            assert int(repl[x]) == (NOKEY if key is None else key), (trial, x)
            assert int(by_edge[peid[x]]) == (NONE if key is None else key & NONE)
        assert (by_edge[flags == 0] == NONE).all()
        have = {e: k for e, k in want.items() if k is not None}
        assert counts["tree_edges"] == len(want) and counts["bridges"] == len(want) - len(have)
        assert counts["improving"] == sum(k < ((int(w[e]) << 32) | e) for e, k in have.items())
        assert counts["tree_edges"] + counts["covering_edges"] + counts["cross_edges"] == m
        if have:
            delta, out = min(((k >> 32) - int(w[e]), e) for e, k in have.items())
            assert (counts["best_delta"], counts["best_out_eid"], counts["best_in_eid"]) == (delta, out, have[out] & NONE)
        else:
            assert (counts["best_delta"], counts["best_out_eid"], counts["best_in_eid"]) == (0, NONE, NONE)
        seen_bridge += counts["bridges"] > 0
        seen_cross += counts["cross_edges"] > 0
        seen_improving += counts["improving"] > 0
    assert seen_bridge and seen_cross and seen_improving   # the trials reach every kind of answer
