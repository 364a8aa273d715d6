"""The weight-rank pass's C-ABI boundary without a GPU (ghs_weight_ranks_temp_bytes /
ghs_weight_ranks_device, rank_weights=True on the Python calls): sizes, every argument check that
comes before any device work, and no CPU fallback."""
import ctypes

import numpy as np
import pytest

from distributed_ghs_implementation_amd import _native

WTYPES = (_native.GHS_W_FLOAT32, _native.GHS_W_FLOAT64, _native.GHS_W_INT64, _native.GHS_W_UINT64)
ELEM = {_native.GHS_W_FLOAT32: 4, _native.GHS_W_FLOAT64: 8, _native.GHS_W_INT64: 8, _native.GHS_W_UINT64: 8}
# host addresses standing in for device pointers: every check below fails before anything is read
BASE = 1 << 20
W_PTR, R_PTR, T_PTR = BASE, BASE + (1 << 16), BASE + (1 << 17)


def _call(L, wtype, m, w, r, t, tb, distinct=None):
    d = ctypes.c_uint64(7) if distinct is None else distinct
    return L.ghs_weight_ranks_device(wtype, m, w, r, ctypes.byref(d), t, tb, None), d.value


def test_constants_match_the_header():
    assert WTYPES == (0, 1, 2, 3)
    assert {"ghs_weight_ranks_temp_bytes", "ghs_weight_ranks_device"} <= set(_native.EXPORTED_SYMBOLS)
    assert _native.load().ghs_abi_version() == 10


@pytest.mark.parametrize("wtype", WTYPES)
def test_temp_bytes_without_a_gpu(wtype):
    L = _native.load()
    assert L.ghs_weight_ranks_temp_bytes(wtype, 0) == 0
    ms = (1, 2, 63, 64, 4095, 4096, 4097, 5000, 100000, 1 << 20, (1 << 20) + 1, 1 << 26)
    sizes = [L.ghs_weight_ranks_temp_bytes(wtype, m) for m in ms]
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] > sizes[0]
    # keys in / out + indices in / out + the status block
    assert all(s >= m * (2 * ELEM[wtype] + 2 * 4) + 256 for s, m in zip(sizes, ms))
    assert L.ghs_weight_ranks_temp_bytes(wtype, 1 << 32) == 0  # over the cap: the call refuses it


def test_unknown_weight_type():
    L = _native.load()
    for bad in (4, 5, 0xFFFFFFFF):
        rc, _ = _call(L, bad, 3, W_PTR, R_PTR, T_PTR, 1 << 16)
        assert rc == _native.GHS_E_ARG and b"weight type" in L.ghs_last_error()
        assert _call(L, bad, 0, None, None, None, 0)[0] == _native.GHS_E_ARG
        assert L.ghs_weight_ranks_temp_bytes(bad, 100) == 0


@pytest.mark.parametrize("wtype", WTYPES)
def test_null_pointers_rejected_before_device_work(wtype):
    L = _native.load()
    tb = L.ghs_weight_ranks_temp_bytes(wtype, 3)
    for w, r, t in ((None, R_PTR, T_PTR), (W_PTR, None, T_PTR), (W_PTR, R_PTR, None), (None, None, None)):
        rc, _ = _call(L, wtype, 3, w, r, t, tb)
        assert rc == _native.GHS_E_ARG  # not GHS_E_NODEVICE: the check comes first
        assert b"NULL" in L.ghs_last_error()
    assert L.ghs_weight_ranks_device(wtype, 3, W_PTR, R_PTR, None, T_PTR, tb, None) == _native.GHS_E_ARG
    assert b"NULL" in L.ghs_last_error()


@pytest.mark.parametrize("wtype", WTYPES)
def test_misaligned_pointers(wtype):
    L = _native.load()
    tb = L.ghs_weight_ranks_temp_bytes(wtype, 3)
    offs = (1, 2, 3) if ELEM[wtype] == 4 else (1, 2, 4, 7)
    for k in offs:  # the weights: their element's own size
        rc, _ = _call(L, wtype, 3, W_PTR + k, R_PTR, T_PTR, tb)
        assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), k
    for k in (1, 2, 3):  # the ranks: 4 bytes
        rc, _ = _call(L, wtype, 3, W_PTR, R_PTR + k, T_PTR, tb)
        assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), k
    for k in (1, 4, 8, 12):  # temp: 16 bytes
        rc, _ = _call(L, wtype, 3, W_PTR, R_PTR, T_PTR + k, tb)
        assert rc == _native.GHS_E_ARG and b"aligned" in L.ghs_last_error(), k


@pytest.mark.parametrize("wtype", WTYPES)
def test_count_cap_and_short_temp(wtype):
    L = _native.load()
    rc, _ = _call(L, wtype, 1 << 32, W_PTR, R_PTR, T_PTR, 1 << 40)
    assert rc == _native.GHS_E_ARG and b"2^32" in L.ghs_last_error()
    tb = L.ghs_weight_ranks_temp_bytes(wtype, 5000)
    for short in (0, 1, tb - 1):
        rc, _ = _call(L, wtype, 5000, W_PTR, R_PTR + (1 << 20), T_PTR + (1 << 21), short)
        assert rc == _native.GHS_E_NOMEM, short


@pytest.mark.parametrize("wtype", WTYPES)
def test_overlapping_ranks(wtype):
    L = _native.load()
    tb = L.ghs_weight_ranks_temp_bytes(wtype, 64)
    for r in (W_PTR, W_PTR + 64 * ELEM[wtype] - 4, T_PTR, T_PTR + tb - 4):
        rc, _ = _call(L, wtype, 64, W_PTR, r, T_PTR, tb)
        assert rc == _native.GHS_E_ARG and b"overlap" in L.ghs_last_error(), r


@pytest.mark.parametrize("wtype", WTYPES)
def test_empty_input_is_ok_with_null_pointers(wtype):
    L = _native.load()
    rc, distinct = _call(L, wtype, 0, None, None, None, 0)
    assert rc == _native.GHS_OK and distinct == 0


@pytest.mark.parametrize("w", [np.array(["a", "b", "c"]), np.array([1j, 2.0, 3.0]),
                               np.array([b"x", b"y", b"z"]), np.array([None, 1, 2], dtype=object)])
def test_rank_weights_refuses_what_is_not_a_number(w):
    from distributed_ghs_implementation_amd import minimum_spanning_forest_edges
    from distributed_ghs_implementation_amd.device import DeviceEdges
    u, v = np.array([0, 0, 2]), np.array([1, 2, 1])
    with pytest.raises(ValueError, match="rank_weights"):
        minimum_spanning_forest_edges(3, u, v, w, rank_weights=True)
    with pytest.raises(ValueError, match="rank_weights"):
        DeviceEdges.from_raw(3, u, v, w, rank_weights=True)


def test_rank_weights_keeps_the_rules_of_u_and_v():
    from distributed_ghs_implementation_amd import minimum_spanning_forest_edges
    w = np.array([0.5, -1.5])
    with pytest.raises(ValueError):
        minimum_spanning_forest_edges(3, [0, -1], [1, 2], w, rank_weights=True)
    with pytest.raises(ValueError):
        minimum_spanning_forest_edges(3, [0.0, 1.0], [1, 2], w, rank_weights=True)
    with pytest.raises(ValueError):
        minimum_spanning_forest_edges(3, [0, 1], [1, 1 << 32], w, rank_weights=True)
    with pytest.raises(ValueError):
        minimum_spanning_forest_edges(3, [0, 1], [1, 2], w[:1], rank_weights=True)
    with pytest.raises(ValueError):
        minimum_spanning_forest_edges(-1, [], [], [], rank_weights=True)


@pytest.mark.skipif(_native.device_count() > 0, reason="CPU-only behaviour")
def test_no_cpu_fallback_without_gpu():
    """Float weights with rank_weights=True are accepted (no ValueError) and then need the GPU."""
    from distributed_ghs_implementation_amd import minimum_spanning_forest_edges
    from distributed_ghs_implementation_amd.device import DeviceEdges
    u, v = np.array([0, 0, 2]), np.array([1, 2, 1])
    for w in ([0.5, 1.5, 2.5], np.array([-3, 1 << 40, 7]), np.array([1, 2, 3], np.uint64),
              np.array([0.5, 1.5, 2.5], np.float16), np.array([-1, 2, 3], np.int8)):
        with pytest.raises(_native.GHSError) as ei:
            minimum_spanning_forest_edges(3, u, v, w, rank_weights=True)
        assert ei.value.code == _native.GHS_E_NODEVICE
        with pytest.raises(_native.GHSError) as ei:
            DeviceEdges.from_raw(3, u, v, w, rank_weights=True)
        assert ei.value.code == _native.GHS_E_NODEVICE


def test_device_edges_weights_default_to_none():
    from distributed_ghs_implementation_amd.device import DeviceEdges
    e = DeviceEdges(2, None, None, None)
    assert e.weights is None and e.src is None and e.off is None
