"""The device ingest's C-ABI boundary without a GPU (ghs_canonicalize_temp_bytes /
ghs_canonicalize_device, minimum_spanning_forest_edges): sizes, argument checks that come before
any device work, and no CPU fallback."""
import ctypes

import numpy as np
import pytest

from distributed_ghs_implementation_amd import _native


def _call(L, n, m_raw, m_out):
    return L.ghs_canonicalize_device(n, m_raw, None, None, None, None, None, None, None, ctypes.byref(m_out), None, 0,
                                     None)


def test_temp_bytes_without_a_gpu():
    L = _native.load()
    assert L.ghs_canonicalize_temp_bytes(1000, 5000) >= 5000 * (2 * 8 + 2 * 4)
    sizes = [L.ghs_canonicalize_temp_bytes(1000, m) for m in (1, 2, 63, 64, 4095, 4096, 4097, 5000, 5001, 100000,
                                                               1 << 20, (1 << 20) + 1, 1 << 26)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    assert L.ghs_canonicalize_temp_bytes((1 << 32) - 1, 1 << 26) >= (1 << 26) * 24


def test_null_pointers_rejected_before_device_work():
    L = _native.load()
    m = ctypes.c_uint64(7)
    assert _call(L, 5, 3, m) == _native.GHS_E_ARG  # not GHS_E_NODEVICE: the check comes first
    assert b"NULL" in L.ghs_last_error()
    assert L.ghs_canonicalize_device(5, 3, None, None, None, None, None, None, None, None, None, 0, None) \
        == _native.GHS_E_ARG


def test_raw_count_cap():
    L = _native.load()
    m = ctypes.c_uint64(7)
    assert _call(L, 5, 1 << 32, m) == _native.GHS_E_ARG
    assert b"2^32" in L.ghs_last_error()


def test_empty_input_is_ok_with_null_pointers():
    L = _native.load()
    m = ctypes.c_uint64(7)
    assert _call(L, 5, 0, m) == _native.GHS_OK
    assert m.value == 0
    assert L.ghs_canonicalize_temp_bytes(5, 0) == 0


@pytest.mark.parametrize("w", [[3, -1], [1.0, 2.0], [1, 1 << 32]])
def test_edges_call_refuses_other_weights(w):
    from distributed_ghs_implementation_amd import minimum_spanning_forest_edges
    with pytest.raises(ValueError, match="canonicalize"):
        minimum_spanning_forest_edges(3, [0, 1], [1, 2], w)


def test_edges_call_refuses_bad_endpoints_and_shapes():
    from distributed_ghs_implementation_amd import minimum_spanning_forest_edges
    with pytest.raises(ValueError):
        minimum_spanning_forest_edges(3, [0, -1], [1, 2], [1, 2])
    with pytest.raises(ValueError):
        minimum_spanning_forest_edges(3, [0, 1], [1, 2], [1])
    with pytest.raises(ValueError):
        minimum_spanning_forest_edges(-1, [], [], [])


@pytest.mark.skipif(_native.device_count() > 0, reason="CPU-only behaviour")
def test_no_cpu_fallback_without_gpu():
    from distributed_ghs_implementation_amd import minimum_spanning_forest_edges
    from distributed_ghs_implementation_amd.device import DeviceEdges
    u, v, w = np.array([0, 0, 2]), np.array([1, 2, 1]), np.array([1, 2, 3])
    with pytest.raises(_native.GHSError) as ei:
        minimum_spanning_forest_edges(3, u, v, w)
    assert ei.value.code == _native.GHS_E_NODEVICE
    with pytest.raises(_native.GHSError) as ei:
        DeviceEdges.from_raw(3, u, v, w)
    assert ei.value.code == _native.GHS_E_NODEVICE


def test_result_attribute_defaults_to_none():
    from distributed_ghs_implementation_amd import CanonicalGraph, MSTResult
    g = CanonicalGraph(2, [0], [1], [5])
    assert MSTResult(g, np.array([1], np.uint8), 5, 1, [], 0.0).raw_ids is None
