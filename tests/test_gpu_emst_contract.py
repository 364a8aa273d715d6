"""ghs_emst_device under the memory contract and on a side stream, and ghs_emst_host on CPU arenas.

entry_emst_device makes the call the way the entries of tests/contract_cases.py do: every device pointer is a
view of one Arena (64 KiB red zones, each pointer aligned as the header asks and no more: 16 bytes for d_x and the
workspace, 4 for d_core2 / d_u / d_v / d_w), the workspace exactly ghs_emst_workspace_bytes long. The three modes
are those of test_gpu_memory_contract.py and test_gpu_side_stream.py, whose runners are used as they are:
  contract   nothing outside the declared outputs and the workspace is written, the inputs are unchanged, the
             answer equals the Kruskal reference and does not depend on what the buffers held before (fills 0x00
             and 0xA5);
  short      one byte less than the declared size: GHS_E_NOMEM, nothing written;
  side       decoy points and cores in the input views, the real ones copied on a side stream behind a delay: the
             answer is still right, so nothing ran on the null stream.
The host form runs through test_gpu_host_forms.host_contract: every host pointer a view of a CPU arena."""
import ctypes

import numpy as np
import pytest

import contract_cases as C
from test_gpu_emst import int_d2, kruskal, kth_smallest, lattice, want_w, with_cores
from test_gpu_host_forms import Run, host_contract
from test_gpu_memory_contract import contract
from test_gpu_side_stream import side_run

pytestmark = pytest.mark.gpu

SHAPES = [(257, 5, 4, 0), (129, 17, None, 3), (600, 33, 1, 64), (2, 1, None, 0)]      # n, dim, core k, slices


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert C.native().device_count() > 0
    return torch


def case(n, dim, k, metric):
    """the points, the cores and what the call must write"""
    X = lattice(n, dim, seed=21)
    D = int_d2(X)
    core = None if k is None else kth_smallest(D, k).astype(np.float32)
    ru, rv, rw = kruskal(with_cores(D, None if core is None else core.astype(np.int64)))
    rw = rw.astype(np.float32)
    want = {"u": ru, "v": rv, "w": want_w(rw, metric).view(np.uint32)}
    info = {"num_edges": n - 1, "zero_edges": int((rw == 0).sum()), "query_tiles": -(-n // 64), "reserved0": 0}
    return np.asarray(X, np.float32), core, want, info


def entry_emst_device(ctx, n, dim, k, slices, metric="euclidean"):
    L, N = C.lib(), C.native()
    X, core, want, info = case(n, dim, k, metric)
    decoy = np.asarray(lattice(n, dim, seed=22), np.float32)
    ctx.inp("d_x", X, 16, lambda: decoy)
    if core is not None:
        ctx.inp("d_core2", core, 4, lambda: core[::-1] + np.float32(3))
    ctx.out("d_u", 4 * (n - 1), 4)
    ctx.out("d_v", 4 * (n - 1), 4)
    ctx.out("d_w", 4 * (n - 1), 4)
    ws, wsz = ctx.sized("d_workspace", int(L.ghs_emst_workspace_bytes(n, dim, slices)))
    res = N.EmstResult()
    ctx.go()
    ctx.call(L.ghs_emst_device, n, dim, ctx.p("d_x"), ctx.p("d_core2") if core is not None else None, N.KNN_METRICS[metric],
             slices, ctx.p("d_u"), ctx.p("d_v"), ctx.p("d_w"), ws, wsz, ctx.stream, ctypes.byref(res))
    ctx.sync()
    if slices:
        info["slices"] = slices
    result = {f: getattr(res, f) for f in ("num_edges", "zero_edges", "slices", "query_tiles", "reserved0", "rounds", "pairs",
                                           "components_after_first_round")}
    assert result["pairs"] == result["rounds"] * n * (n - 1) and 1 <= result["rounds"] <= max(1, int(np.ceil(np.log2(n))))
    result["reserved"] = tuple(res.reserved)
    got = {"u": ctx.read("d_u", np.uint32), "v": ctx.read("d_v", np.uint32), "w": ctx.read("d_w", np.uint32), "result": result}
    return got, dict(want, result=dict(info, reserved=(0,)))


@pytest.mark.parametrize("n,dim,k,slices", SHAPES)
def test_emst_device_contract_and_short_workspace(torch_cuda, n, dim, k, slices):
    contract(torch_cuda, entry_emst_device, n, dim, k, slices)


@pytest.mark.parametrize("n,dim,k,slices", SHAPES[:3])
def test_emst_device_side_stream(torch_cuda, n, dim, k, slices):
    side_run(torch_cuda, entry_emst_device, n, dim, k, slices)


def test_emst_device_contract_squared(torch_cuda):
    contract(torch_cuda, entry_emst_device, 257, 5, 4, 1, "sqeuclidean")


def form_emst(h, opt, n, dim, k, metric):
    L, N = C.lib(), C.native()
    X, core, want, info = case(n, dim, k, metric)
    px = h.inp("x", X)
    pc = h.inp("core2", core) if core is not None else None
    pu, pv, pw = h.out("u", n - 1, np.uint32), h.out("v", n - 1, np.uint32), h.out("w", n - 1, np.uint32)
    res = h.struct("result", N.EmstResult)
    rc = h.call(L.ghs_emst_host, n, dim, px, pc, N.KNN_METRICS[metric], pu, pv, pw, res)
    got = {"u": h.read("u"), "v": h.read("v"), "w": h.read("w"), "result": h.result(N.EmstResult)}
    return Run(rc, got, dict(want, result=info))


@pytest.mark.parametrize("metric", ["euclidean", "sqeuclidean"])
@pytest.mark.parametrize("n,dim,k", [(257, 5, 4), (129, 17, None), (2, 1, None)])
def test_emst_host_on_cpu_arenas(torch_cuda, n, dim, k, metric):
    host_contract(torch_cuda, form_emst, n, dim, k, metric, optional=False)


def test_emst_host_without_points_and_with_bad_ones(torch_cuda):
    L, N = C.lib(), C.native()
    res = N.EmstResult()
    assert L.ghs_emst_host(0, 3, None, None, N.GHS_KNN_EUCLIDEAN, None, None, None, ctypes.byref(res)) == N.GHS_OK
    assert res.num_edges == 0 and res.rounds == 0 and res.slices == 0
    X = np.zeros((4, 3), np.float32)
    X[2, 1] = np.inf
    u, v, w = np.zeros(3, np.uint32), np.zeros(3, np.uint32), np.zeros(3, np.float32)
    rc = L.ghs_emst_host(4, 3, X.ctypes.data, None, N.GHS_KNN_EUCLIDEAN, u.ctypes.data, v.ctypes.data, w.ctypes.data,
                         ctypes.byref(res))
    assert rc == N.GHS_E_ARG and b"non-finite coordinate" in L.ghs_last_error()
    X[2, 1] = 1.0
    core = np.array([0, 1, -2, 3], np.float32)
    rc = L.ghs_emst_host(4, 3, X.ctypes.data, core.ctypes.data, N.GHS_KNN_EUCLIDEAN, u.ctypes.data, v.ctypes.data,
                         w.ctypes.data, ctypes.byref(res))
    assert rc == N.GHS_E_ARG and b"bad core distance" in L.ghs_last_error()
