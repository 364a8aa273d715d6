"""The exact-MST entry points' C-ABI boundary without a GPU (ghs_emst_workspace_bytes / ghs_emst_device /
ghs_emst_host): the result's layout, the section's place in the header and the semantics it states, every
argument check that comes before any device work, the workspace table, the n == 0 and n == 1 answers, the
Python layers' ValueErrors, the CLI's option errors, and the independence of csrc/emst.hip from every other
translation unit."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from distributed_ghs_implementation_amd import _native

# host addresses standing in for device pointers: every check below fails before anything is read
BASE = 1 << 30
NAMES = ("x", "core2", "u", "v", "w", "ws")
GOOD = tuple(BASE + (k << 26) for k in range(len(NAMES)))   # 64 MiB apart: nothing overlaps at the sizes below
CSRC = os.path.join(ROOT, "distributed_ghs_implementation_amd", "csrc")
EMST_HIP = os.path.join(CSRC, "emst.hip")
SYMBOLS = {"ghs_emst_workspace_bytes", "ghs_emst_device", "ghs_emst_host", "ghs_emst_rounds"}
N, DIM = 300, 7
SQ, EU = _native.GHS_KNN_SQEUCLIDEAN, _native.GHS_KNN_EUCLIDEAN


def _call(L, n=N, dim=DIM, metric=EU, slices=0, ptrs=GOOD, ws_bytes=None, res=True):
    r = _native.EmstResult()
    x, core2, u, v, w, ws = ptrs
    if ws_bytes is None:
        ws_bytes = L.ghs_emst_workspace_bytes(n, dim, slices)
    rc = L.ghs_emst_device(n, dim, x, core2, metric, slices, u, v, w, ws, ws_bytes, None, ctypes.byref(r) if res else None)
    return rc, r


def test_result_layout_symbols_and_header():
    R = _native.EmstResult
    assert ctypes.sizeof(R) == 64
    names = [f for f, _ in R._fields_]
    assert names == ["num_edges", "pairs", "zero_edges", "rounds", "slices", "query_tiles", "reserved0",
                     "components_after_first_round", "ms_total", "reserved"]
    assert [getattr(R, f).offset for f in names] == [0, 8, 16, 24, 28, 32, 36, 40, 48, 56]
    assert SYMBOLS <= set(_native.EXPORTED_SYMBOLS)
    L = _native.load()
    for s in SYMBOLS:
        assert getattr(L, s) is not None
    assert L.ghs_abi_version() == 10 and _native.ABI_VERSION == 10
    header = open(os.path.join(ROOT, "include", "ghs_mst.h")).read()
    assert re.search(r"#define\s+GHS_MST_ABI_VERSION\s+10\b", header)
    for s in SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", header), s
    assert "/* 64 bytes */" in header[header.index("typedef struct ghs_emst_result"):][:80]
    # a section of its own directly after ghs_check_canonical, before the stepwise solver
    assert header.index("int ghs_check_canonical(") < header.index("typedef struct ghs_emst_result")
    assert header.index("int ghs_emst_host(") < header.index("typedef struct ghs_solver ghs_solver_t;")
    between = header[header.index("int ghs_check_canonical("): header.index("typedef struct ghs_emst_result")]
    assert "typedef struct" not in between and "ABI 10 addition" in between and "int ghs_" not in between[10:]
    body = header[header.index("typedef struct ghs_emst_result"): header.index("} ghs_emst_result_t;")]
    order = [re.search(rf"\b{f}(\[\d+\])?;", body).start() for f in names]      # the declarations, not the comments
    assert order == sorted(order)  # the header declares the fields in the same order
    for name in ("d_x", "d_core2", "d_u", "d_v", "d_w", "d_workspace", "metric", "slices", "may be NULL"):
        assert name in header[header.index("int ghs_emst_device("):][:700], name
    d = R().as_dict()
    assert set(d) == set(names) - {"reserved", "reserved0"}
    # the semantics the tests hold the code to are stated in the header
    section = header[header.index("exact MST from points"): header.index("typedef struct ghs_emst_result")]
    for phrase in ("max(d2(i, j), core2[i], core2[j])", "fmaf(s, s, acc)", "bit for bit the", "(float_bits(w2), u, v)",
                   "lexicographically", "Keys are distinct", "canonical Kruskal", "overflows to +inf", "d_u[e] < d_v[e]",
                   "strictly ascending", "correctly rounded sqrt(w2)", "same bytes for every `slices`", "ceil(log2 n)",
                   "GHS_E_ROUNDCAP", "non-finite coordinate", "bad core distance", "One host sync", "n - 1 >= 2^31",
                   "NULL means all zero"):
        assert phrase in section, phrase


def test_workspace_table_without_a_gpu():
    """256-aligned, nondecreasing in n and in (explicit) slices, linear in n up to the sort's scratch: the
    status block, 28 bytes per point and 24 per edge, each array rounded up to 256. dim does not enter."""
    W = _native.load().ghs_emst_workspace_bytes
    ns = (2, 3, 63, 64, 65, 257, 1000, 4096, 100000, 1 << 20)
    ss = (0, 1, 2, 3, 7, 64)
    for dim in (1, 16, 4096):
        table = {(n, s): W(n, dim, s) for n in ns for s in ss}
        for (n, s), b in table.items():
            assert b % 256 == 0 and b >= 256 + 28 * n + 24 * (n - 1), (n, s)
            assert b < 2 * (28 * n + 24 * (n - 1)) + (1 << 20), (n, s)
        for s in ss:
            col = [table[n, s] for n in ns]
            assert col == sorted(col), s
        for n in ns:
            col = [table[n, s] for s in ss[1:]]
            assert col == sorted(col), n
            assert table[n, 1] <= table[n, 0] <= table[n, 64]
    assert W(5, 3, 0) == W(5, 4096, 0)                              # dim does not enter
    for bad in ((0, 3, 0), (1, 3, 0), (5, 0, 0), (5, 4097, 0), (5, 3, 65), ((1 << 31) + 1, 3, 1), ((1 << 32) - 1, 3, 1)):
        assert W(*bad) == 0, bad
    assert W(1 << 31, 1, 1) > 0                                    # n - 1 == 2^31 - 1 is the largest


def test_argument_errors_come_before_device_work():
    L = _native.load()
    E = _native.GHS_E_ARG
    rc, _ = _call(L, res=False)
    assert rc == E and b"NULL" in L.ghs_last_error()
    for dim in (0, 4097, 1 << 31):
        rc, _ = _call(L, dim=dim, ws_bytes=1 << 40)
        assert rc == E and b"dim" in L.ghs_last_error(), dim
    for metric in (2, 7, (1 << 32) - 1):
        rc, _ = _call(L, metric=metric)
        assert rc == E and b"metric" in L.ghs_last_error(), metric
    for slices in (65, 1000):
        rc, _ = _call(L, slices=slices, ws_bytes=1 << 40)
        assert rc == E and b"slices" in L.ghs_last_error(), slices
    for n in ((1 << 31) + 1, (1 << 32) - 1):                     # n - 1 == 2^31 and above
        rc, _ = _call(L, n=n, dim=1, ws_bytes=1 << 62)
        assert rc == E and b"2^31" in L.ghs_last_error(), n
    if _native.device_count() == 0:                              # every check passes: only the device is missing
        for kw in ({}, {"n": 2}, {"dim": 4096, "n": 200}, {"metric": SQ}, {"slices": 64}, {"slices": 1},
                   {"ptrs": (GOOD[0], None) + GOOD[2:]}):
            rc, _ = _call(L, **kw)
            assert rc == _native.GHS_E_NODEVICE, kw


def test_null_pointers_rejected_before_device_work():
    L = _native.load()
    for k, name in enumerate(NAMES):
        if name == "core2":
            continue                                             # optional
        args = list(GOOD)
        args[k] = None
        rc, _ = _call(L, ptrs=args)
        assert rc == _native.GHS_E_ARG, name                     # not GHS_E_NODEVICE: the check comes first
        assert b"NULL" in L.ghs_last_error()


def test_misaligned_pointers_rejected():
    L = _native.load()
    for name in ("x", "ws"):
        for off in (1, 2, 4, 8, 12):
            args = list(GOOD)
            args[NAMES.index(name)] += off
            rc, _ = _call(L, ptrs=args)
            assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), (name, off)
    for name in ("core2", "u", "v", "w"):
        for off in (1, 2, 3):
            args = list(GOOD)
            args[NAMES.index(name)] += off
            rc, _ = _call(L, ptrs=args)
            assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), (name, off)
        for off in (4, 8, 12):                                   # 32-bit words: 4 bytes are enough
            args = list(GOOD)
            args[NAMES.index(name)] += off
            rc, _ = _call(L, ptrs=args, ws_bytes=0)
            assert rc == _native.GHS_E_NOMEM, (name, off)


def test_overlapping_pointers_rejected():
    L = _native.load()
    x, c, u, v, w, ws = GOOD
    xb, cb, ob = 4 * N * DIM, 4 * N, 4 * (N - 1)
    assert xb % 16 == 0
    wb = L.ghs_emst_workspace_bytes(N, DIM, 0)

    def call(ptrs, ws_bytes=wb):
        return _call(L, ptrs=ptrs, ws_bytes=ws_bytes)[0]
    for ptrs in ((x, c, u, u, w, ws), (x, c, u, u + ob - 4, w, ws), (x, c, u, v, v - ob + 4, ws),       # outputs over outputs
                 (x, c, x, v, w, ws), (x, c, u, x + xb - 4, w, ws), (x, c, u, v, x - ob + 4, ws),       # outputs over x
                 (x, c, c, v, w, ws), (x, c, u, c + cb - 4, w, ws), (x, c, u, v, c - ob + 4, ws),       # outputs over core2
                 (x, c, u, v, w, x + 16), (x, c, u, v, w, x + xb - 16), (x, c, u, v, w, x - wb + 16),   # ws over x
                 (x, c, u, v, w, c), (x, c, u, v, w, u), (x, c, u, v, w, v + ob - 12), (x, c, u, v, w, w)):
        assert call(ptrs) == _native.GHS_E_ARG and b"overlap" in L.ghs_last_error(), ptrs
    for ptrs in ((x, c, u, u + ob, w, ws), (x, c, u, u - ob, w, ws), (x, c, x + xb, v, w, ws), (x, c, u, v, w, x + xb),
                 (x, None, c, v, w, ws)):
        assert call(ptrs, ws_bytes=0) == _native.GHS_E_NOMEM, ptrs    # adjacent is fine


def test_short_workspace():
    L = _native.load()
    for n, slices in ((2, 0), (5000, 0), (5000, 1), (300, 3), (1 << 20, 0)):
        tb = L.ghs_emst_workspace_bytes(n, 16, slices)
        for short in (0, 1, tb - 1):
            rc, _ = _call(L, n=n, dim=16, slices=slices, ws_bytes=short)
            assert rc == _native.GHS_E_NOMEM, (n, slices, short)


def test_no_points_and_one_point_are_ok_with_null_pointers():
    L = _native.load()
    for n in (0, 1):
        rc, res = _call(L, n=n, ptrs=(None,) * 6, ws_bytes=0)
        assert rc == _native.GHS_OK, n
        assert all(v == 0 for v in res.as_dict().values()) and list(res.reserved) == [0] and res.reserved0 == 0
        for kw in ({"dim": 0}, {"dim": 4097}, {"metric": 2}, {"slices": 65}, {"res": False}):
            rc, _ = _call(L, n=n, ptrs=(None,) * 6, ws_bytes=0, **kw)
            assert rc == _native.GHS_E_ARG, (n, kw)              # still an argument error
    rc, res = _call(L, n=1, ptrs=(GOOD[0], None, None, None, None, None), ws_bytes=0)   # one point: no outputs needed
    assert rc == _native.GHS_OK and res.num_edges == 0


def test_round_diagnostic_without_a_gpu():
    """ghs_emst_rounds: nothing ran on this thread's last call (n <= 1 does no device work), any pointer may be
    NULL, and no more than `capacity` entries are written"""
    L = _native.load()
    rc, _ = _call(L, n=1, ptrs=(None,) * 6, ws_bytes=0)
    assert rc == _native.GHS_OK
    rounds = ctypes.c_uint32(77)
    comps, ms = (ctypes.c_uint32 * 4)(9, 9, 9, 9), (ctypes.c_double * 4)(9, 9, 9, 9)
    assert L.ghs_emst_rounds(0, 4, comps, ms, ctypes.byref(rounds)) == _native.GHS_OK
    assert L.ghs_emst_rounds(0, 0, None, None, None) == _native.GHS_OK
    assert rounds.value <= 32 and list(comps)[min(rounds.value, 4):] == [9] * (4 - min(rounds.value, 4))


def test_host_entry_argument_errors():
    L = _native.load()
    res = _native.EmstResult()
    xa, ca = np.zeros((8, 3), np.float32), np.zeros(8, np.float32)
    ua, va, wa = np.zeros(8, np.uint32), np.zeros(8, np.uint32), np.zeros(8, np.float32)
    x, c, u, v, w = (a.ctypes.data for a in (xa, ca, ua, va, wa))

    def host(n=8, dim=3, ptrs=(x, c, u, v, w), metric=EU, r=res):
        return L.ghs_emst_host(n, dim, ptrs[0], ptrs[1], metric, ptrs[2], ptrs[3], ptrs[4],
                               ctypes.byref(r) if r is not None else None)
    E = _native.GHS_E_ARG
    assert host(dim=0) == E and host(dim=4097) == E and host(metric=2) == E and host(r=None) == E
    assert host(n=(1 << 31) + 1, dim=1) == E and b"2^31" in L.ghs_last_error()
    for k in (0, 2, 3, 4):
        args = [x, c, u, v, w]
        args[k] = None
        assert host(ptrs=args) == E and b"NULL" in L.ghs_last_error(), k
    assert host(ptrs=(x, c, u, u + 4, w)) == E and b"overlap" in L.ghs_last_error()
    assert host(ptrs=(x, c, x + 8, v, w)) == E and b"overlap" in L.ghs_last_error()
    assert host(ptrs=(x, c, u, v, c + 4)) == E and b"overlap" in L.ghs_last_error()
    assert host(ptrs=(x, c, u + 1, v, w)) == E and b"aligned" in L.ghs_last_error()
    assert host(ptrs=(x, c + 2, u, v, w)) == E and b"aligned" in L.ghs_last_error()
    assert host(n=0, ptrs=(None,) * 5) == _native.GHS_OK and res.pairs == 0
    assert host(n=1, ptrs=(x, None, None, None, None)) == _native.GHS_OK and res.num_edges == 0
    if _native.device_count() == 0:
        assert host() == _native.GHS_E_NODEVICE
        assert host(ptrs=(x, None, u, v, w), metric=SQ) == _native.GHS_E_NODEVICE


def test_python_value_errors_without_a_gpu():
    import torch

    from distributed_ghs_implementation_amd import hdbscan_points
    from distributed_ghs_implementation_amd import device as D
    from distributed_ghs_implementation_amd.mst import emst_points
    x = torch.zeros((10, 3), dtype=torch.float32)
    with pytest.raises(ValueError, match="float64"):
        D.emst(x.double())
    with pytest.raises(ValueError, match="two-dimensional"):
        D.emst(x[0])
    with pytest.raises(ValueError, match="two-dimensional"):
        D.emst(np.zeros((10, 3), np.float32))
    with pytest.raises(ValueError, match="metric"):
        D.emst(x, metric="cosine")
    with pytest.raises(ValueError, match="columns"):
        D.emst(torch.zeros((10, 4097)))
    with pytest.raises(ValueError, match="columns"):
        D.emst(torch.zeros((10, 0)))
    with pytest.raises(ValueError, match="expected, got"):
        D.emst(torch.zeros((10, 3), dtype=torch.complex64))
    for bad in (-1, 65, 1.5, "2"):
        with pytest.raises(ValueError, match="slices"):
            D.emst(x, slices=bad)
    for bad in (torch.zeros(10, dtype=torch.float64), torch.zeros((10, 1)), np.zeros(10, np.float32), [0.0] * 10):
        with pytest.raises(ValueError, match="core2"):
            D.emst(x, core2=bad)
    with pytest.raises(ValueError, match="core2: 10 entries"):
        D.emst(x, core2=torch.zeros(9))
    # hdbscan_points(exact=True): the same value errors as before, k ignored
    with pytest.raises(ValueError, match="float64"):
        D.hdbscan_points(x.double(), exact=True)
    with pytest.raises(ValueError, match="min_cluster_size"):
        D.hdbscan_points(x, min_cluster_size=1, exact=True)
    with pytest.raises(ValueError, match="min_samples"):
        D.hdbscan_points(x, min_samples=0, exact=True)
    with pytest.raises(ValueError, match="method"):
        D.hdbscan_points(x, method="dbscan", exact=True)
    with pytest.raises(ValueError, match="metric"):
        D.hdbscan_points(x, metric="manhattan", exact=True)
    with pytest.raises(ValueError, match="k \\+ 1 points"):
        D.hdbscan_points(x, min_samples=12, exact=True)          # the core needs min_samples - 1 <= n - 1 neighbours
    with pytest.raises(ValueError, match="at least 2 points"):
        D.hdbscan_points(x[:1], min_samples=1, exact=True)
    X = np.zeros((10, 3), np.float32)
    for call in (lambda a, **kw: hdbscan_points(a, exact=True, **kw), emst_points):
        with pytest.raises(ValueError, match="float64"):
            call(X.astype(np.float64))
        with pytest.raises(ValueError, match="two-dimensional"):
            call(X[0])
        with pytest.raises(ValueError, match="2\\^24"):
            call(np.full((10, 3), 1 << 24, np.uint32), min_samples=3)
        with pytest.raises(ValueError, match="expected, got"):
            call(X.astype(np.complex64))
        with pytest.raises(ValueError, match="metric"):
            call(X, metric="cosine")
        with pytest.raises(ValueError, match="min_samples"):
            call(X, min_samples=0)
        with pytest.raises(ValueError, match="k \\+ 1 points"):
            call(X, min_samples=12)
    assert _native.emst_args("euclidean") == (EU, 0)
    assert _native.emst_args("sqeuclidean", np.int64(64), n=1 << 31, dim=4096) == (SQ, 64)
    with pytest.raises(ValueError, match="2\\^31"):
        _native.emst_args("euclidean", 0, n=(1 << 31) + 1, dim=1)


@pytest.mark.skipif(_native.device_count() > 0, reason="CPU-only behaviour")
def test_no_cpu_fallback_without_gpu():
    import torch

    from distributed_ghs_implementation_amd import hdbscan_points
    from distributed_ghs_implementation_amd import device as D
    from distributed_ghs_implementation_amd.mst import emst_points
    x = torch.arange(60, dtype=torch.float32).reshape(20, 3)
    for call in (lambda: D.emst(x), lambda: D.emst(x, core2=torch.ones(20)),
                 lambda: D.hdbscan_points(x, min_cluster_size=3, exact=True),
                 lambda: hdbscan_points(x.numpy(), min_cluster_size=3, exact=True),
                 lambda: emst_points(x.numpy()), lambda: emst_points(x.numpy(), min_samples=3)):
        with pytest.raises(_native.GHSError) as ei:
            call()
        assert ei.value.code == _native.GHS_E_NODEVICE


def test_cli_options_without_a_gpu(capsys, tmp_path):
    from distributed_ghs_implementation_amd.__main__ import main
    p = str(tmp_path / "nowhere.npy")                            # never read: the option errors come first
    cases = ((["--emst", "o.npz"], "--emst / --exact need --points X.npy"),
             (["--exact"], "--emst / --exact need --points X.npy"),
             (["--hdbscan", "o.npz", "--exact"], "--emst / --exact need --points X.npy"),
             (["--points", p, "--emst", "o.npz", "--graph", "g.mstbin"], "--points excludes --graph"),
             (["--points", p, "--emst", "o.npz", "--generator", "rmat"], "--points excludes --graph"),
             (["--points", p], "or --emst OUT.npz"),
             (["--points", p, "--exact"], "or --emst OUT.npz"),
             (["--points", p, "--emst", "o.npz", "--exact"], "--exact needs --hdbscan OUT.npz"),
             (["--points", p, "--emst", "o.npz", "--metric", "cosine"], "invalid choice"),
             (["--points", p, "--emst", "o.npz", "--min-samples", "0"], "--min-samples K needs K >= 1"),
             (["--points", p, "--emst", "o.npz", "--labels", "l.npy"], "--points takes --knn-graph OUT.npz and --hdbscan"),
             (["--points", p, "--emst", "o.npz", "--min-cluster-size", "5"], "--min-cluster-size needs --clusters OUT.npz"),
             (["--min-samples", "3"], "--min-samples needs --hdbscan OUT.npz or --mutual-reachability OUT.npz"))
    for argv, text in cases:
        with pytest.raises(SystemExit) as ei:
            main(argv)
        assert ei.value.code == 2, argv
        assert text in capsys.readouterr().err, argv
    # these pass the option checks: the next failure is the missing file, not argparse's exit
    for argv in (["--points", p, "--emst", str(tmp_path / "t.npz")],
                 ["--points", p, "--emst", str(tmp_path / "t.npz"), "--min-samples", "5", "--metric", "sqeuclidean"],
                 ["--points", p, "--hdbscan", str(tmp_path / "h.npz"), "--exact"],
                 ["--points", p, "--hdbscan", str(tmp_path / "h.npz"), "--exact", "--emst", str(tmp_path / "t.npz"),
                  "--min-samples", "3", "--min-cluster-size", "5", "--cluster-method", "leaf", "--knn", "15"]):
        with pytest.raises(FileNotFoundError):
            main(argv)
        capsys.readouterr()


def test_emst_hip_stands_alone():
    """csrc/emst.hip includes no project source but common.h, launches only kernels it defines (all named
    k_emst_*), shares no kernel name with any other file of csrc/, restates the distance chain with an explicit
    fmaf (never the |a|^2 + |b|^2 - 2ab form), has no floating-point atomic, syncs once per round, and is
    compiled without fast-math."""
    src = open(EMST_HIP).read()
    assert re.findall(r'^\s*#\s*include\s+"([^"]+)"', src, re.M) == ["common.h"]
    for inc in re.findall(r"^\s*#\s*include\s+<([^>]+)>", src, re.M):
        assert inc.startswith(("hip/", "rocprim/")) or "/" not in inc, inc      # HIP, rocPRIM and the C++ library
    launched = set(re.findall(r"\b(k_\w+)\s*(?:<[^<>]*>)?\s*<<<", src))
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src, re.S))
    assert launched and launched == defined, launched ^ defined
    assert all(k.startswith("k_emst_") for k in defined), defined
    assert {"k_emst_scan", "k_emst_cmin", "k_emst_cmax", "k_emst_hook", "k_emst_jump"} <= defined
    code = re.sub(r"//[^\n]*", "", src)
    assert "fmaf(" in code and "__fsub_rn(" in code               # the chain as the header states it, no contraction
    assert "sqrtf(" in code and "radix_sort_pairs" in code
    assert "mfma" not in code.lower() and "dot(" not in code      # no |a|^2 + |b|^2 - 2ab
    # atomics: integer only, never on a float
    atomics = re.findall(r"atomic\w+\s*\(([^;]*);", code)
    assert atomics and all("float" not in a and "acc" not in a for a in atomics), atomics
    assert {m for m in re.findall(r"\b(atomic\w+)\s*\(", code)} <= {"atomicMin", "atomicAdd"}
    assert not re.search(r"unsafeAtomic|atomicAdd_f|__hip_atomic_fetch_add\s*\(\s*\(?float", code)
    # one sync inside the round loop, one after the last pass; nothing on the null stream
    loop = code[code.index("while (edges < t)"): code.index("rocprim::radix_sort_pairs(base")]
    assert loop.count("hipStreamSynchronize(") == 1 and code.count("hipStreamSynchronize(") == 2
    assert "hipDeviceSynchronize" not in code and "<<<grid, EM_BLOCK, 0, st>>>" in code
    for launch in re.findall(r"<<<([^>]*)>>>", code):
        assert launch.rstrip().endswith(", st"), launch
    assert "GHS_E_ROUNDCAP" in code
    other = ""
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")) and name != "emst.hip":
            other += open(os.path.join(CSRC, name)).read()
    for part in sorted(os.listdir(os.path.join(CSRC, "boruvka"))):
        other += open(os.path.join(CSRC, "boruvka", part)).read()
    other_kernels = set(re.findall(r"\bvoid\s+(k_\w+)\s*\(", other))
    assert other_kernels and not (defined & other_kernels)
    assert not re.search(r"\bk_emst_\w*", other) and "emst" not in other
    for prefix in ("k_knn_", "k_mr_", "k_cl_", "k_dg_", "k_ds_", "k_rp_", "k_rt_", "k_pa_", "k_lb_"):   # the other modules' own names
        assert prefix not in src, prefix
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "fast-math" not in mk and "-Ofast" not in mk


def test_makefile_links_emst_everywhere():
    lines = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ").split("\n")
    objs = [ln for ln in lines if re.match(r"OBJS\s*:=", ln)]
    assert len(objs) == 1 and "$(OUTDIR)/emst.o" in objs[0] and "$(OUTDIR)/knn.o" in objs[0]
    prereq = [ln for ln in lines if ln.startswith("rcclstub:")]
    assert len(prereq) == 1 and "$(OUTDIR)/emst.o" in prereq[0]       # the target's prerequisites
    link = [ln for ln in lines if ln.startswith("\t") and "-o $(STUB)/libghs_mst_rcclstub.so" in ln]
    assert len(link) == 1 and "$(OUTDIR)/emst.o" in link[0]           # and its link line
