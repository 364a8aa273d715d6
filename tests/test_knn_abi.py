"""The k-NN entry points' C-ABI boundary without a GPU (ghs_knn_workspace_bytes / ghs_knn_device /
ghs_knn_host): the result's layout, the section's place in the header, every argument check that comes
before any device work, the workspace table, the n == 0 answer, the Python layers' ValueErrors, the CLI's
option errors, and the independence of csrc/knn.hip from every other translation unit."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from distributed_ghs_implementation_amd import _native

# host addresses standing in for device pointers: every check below fails before anything is read
BASE = 1 << 30
NAMES = ("x", "idx", "dist", "ws")
GOOD = tuple(BASE + (k << 26) for k in range(len(NAMES)))   # 64 MiB apart: nothing overlaps at the sizes below
CSRC = os.path.join(ROOT, "distributed_ghs_implementation_amd", "csrc")
KNN_HIP = os.path.join(CSRC, "knn.hip")
SYMBOLS = {"ghs_knn_workspace_bytes", "ghs_knn_device", "ghs_knn_host"}
N, DIM, K = 300, 7, 9
SQ, EU = _native.GHS_KNN_SQEUCLIDEAN, _native.GHS_KNN_EUCLIDEAN


def _call(L, n=N, dim=DIM, k=K, metric=EU, slices=0, ptrs=GOOD, ws_bytes=None, res=True):
    r = _native.KnnResult()
    x, idx, dist, ws = ptrs
    if ws_bytes is None:
        ws_bytes = L.ghs_knn_workspace_bytes(n, dim, k, slices)
    rc = L.ghs_knn_device(n, dim, x, k, metric, slices, idx, dist, ws, ws_bytes, None, ctypes.byref(r) if res else None)
    return rc, r


def test_result_layout_symbols_and_header():
    R = _native.KnnResult
    assert ctypes.sizeof(R) == 48
    assert [f for f, _ in R._fields_] == ["pairs", "zero_neighbours", "slices", "query_tiles", "ms_total", "reserved"]
    assert [getattr(R, f).offset for f, _ in R._fields_] == [0, 8, 16, 20, 24, 32]
    assert SYMBOLS <= set(_native.EXPORTED_SYMBOLS)
    L = _native.load()
    for s in SYMBOLS:
        assert getattr(L, s) is not None
    assert L.ghs_abi_version() == 10 and _native.ABI_VERSION == 10
    header = open(os.path.join(ROOT, "include", "ghs_mst.h")).read()
    assert re.search(r"#define\s+GHS_MST_ABI_VERSION\s+10\b", header)
    for s in SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", header), s
    assert "/* 48 bytes */" in header[header.index("typedef struct ghs_knn_result"):][:80]
    # a section of its own between ghs_mutual_reach_phases and ghs_check_canonical
    assert header.index("int ghs_mutual_reach_phases(") < header.index("typedef struct ghs_knn_result")
    assert header.index("int ghs_knn_host(") < header.index("int ghs_check_canonical(")
    between = header[header.index("int ghs_mutual_reach_phases("): header.index("typedef struct ghs_knn_result")]
    assert "typedef struct" not in between and "ABI 10 addition" in between
    after = header[header.index("int ghs_knn_host("): header.index("int ghs_check_canonical(")]
    assert "typedef struct" not in after
    body = header[header.index("typedef struct ghs_knn_result"): header.index("} ghs_knn_result_t;")]
    order = [body.index(f) for f, _ in R._fields_]
    assert order == sorted(order)  # the header declares the fields in the same order
    for name in ("d_x", "d_idx", "d_dist", "d_workspace", "metric", "slices"):
        assert name in header[header.index("int ghs_knn_device("):][:500], name
    for name in ("GHS_KNN_MAX_K", "GHS_KNN_MAX_DIM", "GHS_KNN_MAX_SLICES", "GHS_KNN_SQEUCLIDEAN", "GHS_KNN_EUCLIDEAN",
                 "GHS_KNN_TILE_Q", "GHS_KNN_TILE_C", "GHS_KNN_DIM_CHUNK"):
        mt = re.search(rf"#define\s+{name}\s+(\d+)u", header)
        assert mt and int(mt.group(1)) == getattr(_native, name), name
    assert (_native.GHS_KNN_MAX_K, _native.GHS_KNN_MAX_DIM, _native.GHS_KNN_MAX_SLICES) == (128, 4096, 64)
    assert _native.KNN_METRICS == {"sqeuclidean": SQ, "euclidean": EU} and (SQ, EU) == (0, 1)
    d = R().as_dict()
    assert set(d) == {f for f, _ in R._fields_} - {"reserved"}
    # the semantics the tests hold the code to are stated in the header
    section = header[header.index("k-NN graph"): header.index("#define GHS_KNN_MAX_K")]
    for phrase in ("fmaf(s, s, acc)", "(dim + 3) * 2^-23", "ties go to the", "never by distance", "non-finite coordinate",
                   "one host sync"):
        assert phrase in section, phrase


def test_workspace_table_without_a_gpu():
    """256-aligned, nondecreasing in n, k and (explicit) slices, and never more than the S * n * k keys of 8
    bytes, rounded up to 256, plus the 256-byte status block: below 2 * 8 * S * n * k + 512. slices == 0 is
    the size for the count the library chooses from n, and no more than that of GHS_KNN_MAX_SLICES."""
    W = _native.load().ghs_knn_workspace_bytes
    ns = (2, 3, 63, 64, 65, 257, 1000, 4096, 100000, 1 << 20)
    ks = (1, 2, 15, 16, 17, 64, 128)
    ss = (1, 2, 3, 7, 64)
    for dim in (1, 16, 4096):
        table = {(n, k, s): W(n, dim, k, s) for n in ns for k in ks for s in ss}
        for (n, k, s), b in table.items():
            assert b % 256 == 0 and b >= 256, (n, k, s)
            assert b >= 8 * s * n * k * (s > 1), (n, k, s)
            assert b < 2 * 8 * s * n * k + 512, (n, k, s)
        for k in ks:
            for s in ss:
                col = [table[n, k, s] for n in ns]
                assert col == sorted(col), (k, s)
        for n in ns:
            for s in ss:
                col = [table[n, k, s] for k in ks]
                assert col == sorted(col), (n, s)
            for k in ks:
                col = [table[n, k, s] for s in ss]
                assert col == sorted(col), (n, k)
                assert 256 <= W(n, dim, k, 0) <= table[n, k, 64]
    assert W(1 << 20, 16, 15, 0) == 256                          # enough query tiles: one slice, no keys
    assert W(5, 3, 2, 0) == W(5, 4096, 2, 0)                     # dim does not enter
    for bad in ((0, 3, 2, 0), (5, 0, 2, 0), (5, 4097, 2, 0), (5, 3, 0, 0), (5, 3, 129, 0), (5, 3, 2, 65),
                (1 << 25, 3, 128, 1)):
        assert W(*bad) == 0, bad


def test_argument_errors_come_before_device_work():
    L = _native.load()
    E = _native.GHS_E_ARG
    rc, _ = _call(L, res=False)
    assert rc == E and b"NULL" in L.ghs_last_error()
    for k in (0, 129, 1 << 31):
        rc, _ = _call(L, k=k, ws_bytes=1 << 40)
        assert rc == E and b"k" in L.ghs_last_error(), k
    for k, n in ((K, K), (K + 1, K), (1, 1), (128, 128), (2, 2), (100, 3)):   # k == n and above: at most n - 1 neighbours
        rc, _ = _call(L, n=n, k=k, ws_bytes=1 << 40)
        assert rc == E and b"n - 1" in L.ghs_last_error(), (k, n)
    for dim in (0, 4097, 1 << 31):
        rc, _ = _call(L, dim=dim, ws_bytes=1 << 40)
        assert rc == E and b"dim" in L.ghs_last_error(), dim
    for metric in (2, 7, (1 << 32) - 1):
        rc, _ = _call(L, metric=metric)
        assert rc == E and b"metric" in L.ghs_last_error(), metric
    for slices in (65, 1000):
        rc, _ = _call(L, slices=slices, ws_bytes=1 << 40)
        assert rc == E and b"slices" in L.ghs_last_error(), slices
    for n, k in ((1 << 25, 128), (1 << 31, 2), ((1 << 32) - 1, 1 << 6)):   # n * k == 2^32 and above
        rc, _ = _call(L, n=n, k=k, dim=1, ws_bytes=1 << 62)
        assert rc == E and b"2^32" in L.ghs_last_error(), (n, k)
    if _native.device_count() == 0:                              # every check passes: only the device is missing
        for kw in ({}, {"n": 129, "k": 128}, {"k": 128}, {"dim": 4096, "n": 200}, {"metric": SQ}, {"slices": 64}, {"slices": 1}):
            rc, _ = _call(L, **kw)
            assert rc == _native.GHS_E_NODEVICE, kw


def test_null_pointers_rejected_before_device_work():
    L = _native.load()
    for k, name in enumerate(NAMES):
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
    for name in ("idx", "dist"):
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
    x, idx, dist, ws = GOOD
    xb, ob = 4 * N * DIM, 4 * N * K
    assert xb % 16 == 0
    wb = L.ghs_knn_workspace_bytes(N, DIM, K, 3)
    assert wb > 256

    def call(ptrs, ws_bytes=wb):
        return _call(L, slices=3, ptrs=ptrs, ws_bytes=ws_bytes)[0]
    for ptrs in ((x, idx, idx, ws), (x, idx, idx + ob - 4, ws), (x, idx, idx - ob + 4, ws),       # dist over idx
                 (x, x, dist, ws), (x, x + xb - 4, dist, ws), (x, x - ob + 4, dist, ws),          # idx over x
                 (x, idx, x + 16, ws), (x, idx, x - ob + 4, ws),                                  # dist over x
                 (x, idx, dist, x + 16), (x, idx, dist, x + xb - 16), (x, idx, dist, x - wb + 16),    # ws over x
                 (x, idx, dist, idx), (x, idx, dist, dist + ob - 16)):                            # ws over the outputs
        assert call(ptrs) == _native.GHS_E_ARG and b"overlap" in L.ghs_last_error(), ptrs
    for ptrs in ((x, idx, idx + ob, ws), (x, idx, idx - ob, ws), (x, x + xb, dist, ws), (x, idx, dist, x + xb)):
        assert call(ptrs, ws_bytes=0) == _native.GHS_E_NOMEM, ptrs    # adjacent is fine


def test_short_workspace():
    L = _native.load()
    for n, k, slices in ((5000, 15, 0), (5000, 15, 1), (300, 128, 3), (1 << 20, 15, 0)):
        tb = L.ghs_knn_workspace_bytes(n, 16, k, slices)
        for short in (0, 1, tb - 1):
            rc, _ = _call(L, n=n, dim=16, k=k, slices=slices, ws_bytes=short)
            assert rc == _native.GHS_E_NOMEM, (n, k, slices, short)


def test_no_points_is_ok_with_null_pointers():
    L = _native.load()
    rc, res = _call(L, n=0, ptrs=(None,) * 4, ws_bytes=0)
    assert rc == _native.GHS_OK
    assert all(v == 0 for v in res.as_dict().values()) and list(res.reserved) == [0, 0]
    for kw in ({"k": 0}, {"k": 129}, {"dim": 0}, {"metric": 2}, {"slices": 65}, {"res": False}):
        rc, _ = _call(L, n=0, ptrs=(None,) * 4, ws_bytes=0, **kw)
        assert rc == _native.GHS_E_ARG, kw                       # still an argument error


def test_host_entry_argument_errors():
    L = _native.load()
    res = _native.KnnResult()
    xa = np.zeros((8, 3), np.float32)
    ia, da = np.zeros((8, 8), np.uint32), np.zeros((8, 8), np.float32)      # room for every k below
    x, idx, dist = xa.ctypes.data, ia.ctypes.data, da.ctypes.data

    def host(n=8, dim=3, ptrs=(x, idx, dist), k=4, metric=EU, r=res):
        return L.ghs_knn_host(n, dim, ptrs[0], k, metric, ptrs[1], ptrs[2], ctypes.byref(r) if r is not None else None)
    E = _native.GHS_E_ARG
    assert host(k=0) == E and host(k=129) == E and host(k=8) == E and b"n - 1" in L.ghs_last_error()
    assert host(dim=0) == E and host(dim=4097) == E and host(metric=2) == E and host(r=None) == E
    assert host(n=1 << 25, k=128, dim=1) == E and b"2^32" in L.ghs_last_error()
    for k in range(3):
        args = [x, idx, dist]
        args[k] = None
        assert host(ptrs=args) == E and b"NULL" in L.ghs_last_error(), k
    assert host(ptrs=(x, idx, idx + 4)) == E and b"overlap" in L.ghs_last_error()
    assert host(ptrs=(x, x + 8, dist)) == E and b"overlap" in L.ghs_last_error()
    assert host(ptrs=(x, idx + 1, dist)) == E and b"aligned" in L.ghs_last_error()
    assert host(n=0, ptrs=(None, None, None)) == _native.GHS_OK and res.pairs == 0
    if _native.device_count() == 0:
        assert host() == _native.GHS_E_NODEVICE
        assert host(k=7, metric=SQ) == _native.GHS_E_NODEVICE


def test_python_value_errors_without_a_gpu():
    import torch

    from distributed_ghs_implementation_amd import hdbscan_points
    from distributed_ghs_implementation_amd import device as D
    x = torch.zeros((10, 3), dtype=torch.float32)
    for call in (D.knn, D.knn_graph):
        with pytest.raises(ValueError, match="float64"):
            call(x.double(), 3)
        with pytest.raises(ValueError, match="two-dimensional"):
            call(x[0], 3)
        with pytest.raises(ValueError, match="two-dimensional"):
            call(np.zeros((10, 3), np.float32), 3)
        for bad in (0, -1, 129, 2.5, "3", None, 10, 11):
            with pytest.raises(ValueError, match="k"):
                call(x, bad)
        with pytest.raises(ValueError, match="metric"):
            call(x, 3, metric="cosine")
        with pytest.raises(ValueError, match="columns"):
            call(torch.zeros((10, 4097)), 3)
        with pytest.raises(ValueError, match="columns"):
            call(torch.zeros((10, 0)), 3)
        with pytest.raises(ValueError, match="expected, got"):
            call(torch.zeros((10, 3), dtype=torch.complex64), 3)
    for bad in (-1, 65, 1.5, "2"):
        with pytest.raises(ValueError, match="slices"):
            D.knn(x, 3, slices=bad)
    with pytest.raises(ValueError, match="float64"):
        D.hdbscan_points(x.double())
    with pytest.raises(ValueError, match="min_samples - 1"):
        D.hdbscan_points(x, min_samples=5, k=3)                  # k < min_samples - 1
    with pytest.raises(ValueError, match="k \\+ 1 points"):
        D.hdbscan_points(x, min_samples=5, k=10)                 # k > n - 1
    with pytest.raises(ValueError, match="k \\+ 1 points"):
        D.hdbscan_points(x, min_cluster_size=20)                 # k = min_samples = 20 by default
    with pytest.raises(ValueError, match="min_cluster_size"):
        D.hdbscan_points(x, min_cluster_size=1)
    with pytest.raises(ValueError, match="min_samples"):
        D.hdbscan_points(x, min_samples=0)
    with pytest.raises(ValueError, match="method"):
        D.hdbscan_points(x, method="dbscan")
    with pytest.raises(ValueError, match="metric"):
        D.hdbscan_points(x, metric="manhattan")
    X = np.zeros((10, 3), np.float32)
    with pytest.raises(ValueError, match="float64"):
        hdbscan_points(X.astype(np.float64))
    with pytest.raises(ValueError, match="two-dimensional"):
        hdbscan_points(X[0])
    with pytest.raises(ValueError, match="min_samples - 1"):
        hdbscan_points(X, min_samples=6, k=4)
    with pytest.raises(ValueError, match="k \\+ 1 points"):
        hdbscan_points(X, min_samples=3, k=10)
    with pytest.raises(ValueError, match="2\\^24"):
        hdbscan_points(np.full((10, 3), 1 << 24, np.uint32), min_samples=3)
    with pytest.raises(ValueError, match="expected, got"):
        hdbscan_points(X.astype(np.complex64))
    assert _native.knn_args(5, "euclidean") == (5, EU, 0)
    assert _native.knn_args(np.int64(128), "sqeuclidean", 64, n=129, dim=4096) == (128, SQ, 64)
    with pytest.raises(ValueError, match="2\\^32"):
        _native.knn_args(128, "euclidean", 0, n=1 << 25, dim=1)


@pytest.mark.skipif(_native.device_count() > 0, reason="CPU-only behaviour")
def test_no_cpu_fallback_without_gpu():
    import torch

    from distributed_ghs_implementation_amd import hdbscan_points
    from distributed_ghs_implementation_amd import device as D
    x = torch.arange(60, dtype=torch.float32).reshape(20, 3)
    for call in (lambda: D.knn(x, 3), lambda: D.knn_graph(x, 3), lambda: D.hdbscan_points(x, min_cluster_size=3),
                 lambda: hdbscan_points(x.numpy(), min_cluster_size=3)):
        with pytest.raises(_native.GHSError) as ei:
            call()
        assert ei.value.code == _native.GHS_E_NODEVICE


def test_cli_options_without_a_gpu(capsys, tmp_path):
    from distributed_ghs_implementation_amd.__main__ import main
    p = str(tmp_path / "nowhere.npy")                            # never read: the option errors come first
    cases = ((["--knn", "5"], "--knn / --metric / --knn-graph need --points X.npy"),
             (["--metric", "euclidean"], "--knn / --metric / --knn-graph need --points X.npy"),
             (["--knn-graph", "o.npz"], "--knn / --metric / --knn-graph need --points X.npy"),
             (["--points", p, "--knn-graph", "o.npz", "--knn", "5", "--graph", "g.mstbin"], "--points excludes --graph"),
             (["--points", p, "--knn-graph", "o.npz", "--knn", "5", "--generator", "rmat"], "--points excludes --graph"),
             (["--points", p, "--knn-graph", "o.npz", "--knn", "5", "--batch-dir", "d"], "--points excludes --graph"),
             (["--points", p], "--points X.npy needs --knn-graph OUT.npz or --hdbscan OUT.npz"),
             (["--points", p, "--knn-graph", "o.npz"], "--knn-graph OUT.npz needs --knn K"),
             (["--points", p, "--knn-graph", "o.npz", "--knn", "0"], "--knn K needs 1 <= K <= 128"),
             (["--points", p, "--hdbscan", "o.npz", "--knn", "129"], "--knn K needs 1 <= K <= 128"),
             (["--points", p, "--hdbscan", "o.npz", "--metric", "cosine"], "invalid choice"),
             (["--points", p, "--hdbscan", "o.npz", "--labels", "l.npy"], "--points takes --knn-graph OUT.npz and --hdbscan"),
             (["--points", p, "--hdbscan", "o.npz", "--min-samples", "0"], "--min-samples K needs K >= 1"),
             (["--points", p, "--hdbscan", "o.npz", "--min-cluster-size", "1"], "--min-cluster-size K with K >= 2"))
    for argv, text in cases:
        with pytest.raises(SystemExit) as ei:
            main(argv)
        assert ei.value.code == 2, argv
        assert text in capsys.readouterr().err, argv
    # these pass the option checks: the next failure is the missing file, not argparse's exit
    for argv in (["--points", p, "--knn-graph", str(tmp_path / "g.npz"), "--knn", "5"],
                 ["--points", p, "--hdbscan", str(tmp_path / "h.npz")],
                 ["--points", p, "--hdbscan", str(tmp_path / "h.npz"), "--knn", "15", "--metric", "sqeuclidean",
                  "--min-samples", "3", "--min-cluster-size", "5", "--cluster-method", "leaf", "--allow-single-cluster"]):
        with pytest.raises(FileNotFoundError):
            main(argv)
        capsys.readouterr()


def test_knn_hip_stands_alone():
    """csrc/knn.hip includes no project source but common.h, launches only kernels it defines (all named
    k_knn_*), shares no kernel name with any other file of csrc/, writes the distance chain with an explicit
    fmaf, has no floating-point atomic, and is compiled without fast-math."""
    src = open(KNN_HIP).read()
    assert re.findall(r'^\s*#\s*include\s+"([^"]+)"', src, re.M) == ["common.h"]
    for inc in re.findall(r"^\s*#\s*include\s+<([^>]+)>", src, re.M):
        assert inc.startswith("hip/") or "/" not in inc, inc      # HIP and the C++ library
    launched = set(re.findall(r"\b(k_\w+)\s*(?:<[^<>]*>)?\s*<<<", src))
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src, re.S))
    assert launched and launched == defined, launched ^ defined
    assert all(k.startswith("k_knn_") for k in defined), defined
    assert {"k_knn_scan", "k_knn_merge"} <= defined
    code = re.sub(r"//[^\n]*", "", src)
    assert "fmaf(" in code and "__fsub_rn(" in code               # the chain as the header states it, no contraction
    assert "sqrtf(" in code
    # atomics: on the LDS queue counters and the uint64 count of zeros only, never on a float
    atomics = re.findall(r"atomic\w+\s*\(([^;]*);", code)
    assert atomics and all("float" not in a and "dist" not in a for a in atomics), atomics
    assert not re.search(r"atomic\w*\s*\(\s*(&\s*)?\(?\s*(float|dist|acc)", code)
    assert not re.search(r"unsafeAtomic|atomicAdd_f|__hip_atomic_fetch_add\s*\(\s*\(?float", code)
    assert "hipStreamSynchronize" in code and code.count("hipStreamSynchronize(") == 1      # one host sync per call
    assert "hipDeviceSynchronize" not in code and "<<<grid, KN_BLOCK, 0, st>>>" in code     # nothing on the null stream
    for launch in re.findall(r"<<<([^>]*)>>>", code):
        assert launch.rstrip().endswith(", st"), launch
    other = ""
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")) and name != "knn.hip":
            other += open(os.path.join(CSRC, name)).read()
    for part in sorted(os.listdir(os.path.join(CSRC, "boruvka"))):
        other += open(os.path.join(CSRC, "boruvka", part)).read()
    other_kernels = set(re.findall(r"\bvoid\s+(k_\w+)\s*\(", other))
    assert other_kernels and not (defined & other_kernels)
    assert not re.search(r"\bk_knn_\w*", other)
    for prefix in ("k_mr_", "k_cl_", "k_dg_", "k_ds_", "k_rp_", "k_rt_", "k_pa_"):      # the other modules' own names
        assert prefix not in src, prefix
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "fast-math" not in mk and "-Ofast" not in mk


def test_makefile_links_knn_everywhere():
    lines = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ").split("\n")
    objs = [ln for ln in lines if re.match(r"OBJS\s*:=", ln)]
    assert len(objs) == 1 and "$(OUTDIR)/knn.o" in objs[0] and "$(OUTDIR)/mreach.o" in objs[0]
    prereq = [ln for ln in lines if ln.startswith("rcclstub:")]
    assert len(prereq) == 1 and "$(OUTDIR)/knn.o" in prereq[0]        # the target's prerequisites
    link = [ln for ln in lines if ln.startswith("\t") and "-o $(STUB)/libghs_mst_rcclstub.so" in ln]
    assert len(link) == 1 and "$(OUTDIR)/knn.o" in link[0]            # and its link line
