"""GPU: the device ingest (ghs_canonicalize_device: k_canon_keys, rocPRIM pairs sort, k_canon_count /
k_uniq_scan / k_canon_write) against the host references oracle.canonicalize_c and
graph.canonicalize, bit for bit: u, v, w, m, the raw-index map `src` (identities, and that it names
the LARGEST raw index of its pair), and ghs_check_canonical on the result."""
import ctypes

import numpy as np
import pytest

from conftest import load_fixture

pytestmark = pytest.mark.gpu

T = 4096  # the compaction's tile (csrc/ingest.hip UQ_TILE)
U32 = (1 << 32) - 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from distributed_ghs_implementation_amd import _native
    assert _native.device_count() > 0
    return torch


def _N():
    from distributed_ghs_implementation_amd import _native
    return _native


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view("int32").copy()).cuda()


def _h(t):
    return t.cpu().numpy().view("uint32")


def _host_last(u, v):
    """Per unordered pair (self-loops dropped), in canonical order: the largest raw index."""
    a, b = u.astype(np.uint64), v.astype(np.uint64)
    keep = a != b
    key = (np.minimum(a, b) << np.uint64(32)) | np.maximum(a, b)
    uniq, inv = np.unique(key[keep], return_inverse=True)
    last = np.full(len(uniq), -1, dtype=np.int64)
    np.maximum.at(last, inv.ravel(), np.flatnonzero(keep))
    return last


def _device(n, ru, rv, rw, **kw):
    from distributed_ghs_implementation_amd.device import canonicalize_device
    return canonicalize_device(n, _t(ru), _t(rv), _t(rw), **kw)


def _check_against(e, n, ru, rv, rw, ref, graph_ref=True):
    """e: DeviceEdges from the device ingest of (ru, rv, rw); ref: oracle.canonicalize_c's arrays."""
    from distributed_ghs_implementation_amd import canonicalize
    N = _N()
    ou, ov, ow = ref
    cu, cv, cw, src = _h(e.u), _h(e.v), _h(e.w), _h(e.src).astype(np.int64)
    assert e.n == n and e.m == len(ou) == len(cu) == len(cv) == len(cw) == len(src)
    assert np.array_equal(cu, ou) and np.array_equal(cv, ov) and np.array_equal(cw, ow)
    if graph_ref:
        g = canonicalize(n, u=ru.astype(np.int64), v=rv.astype(np.int64), w=rw)
        assert g.weights is None
        assert np.array_equal(cu, g.u) and np.array_equal(cv, g.v) and np.array_equal(cw, g.w)
    # src: the raw edge every canonical edge came from, and the last of its pair
    assert np.array_equal(np.minimum(ru[src], rv[src]), cu)
    assert np.array_equal(np.maximum(ru[src], rv[src]), cv)
    assert np.array_equal(rw[src], cw)
    assert np.array_equal(src, _host_last(ru, rv))
    ok = ctypes.c_int(0)
    from distributed_ghs_implementation_amd.device import _ptr, _stream
    N.check(N.load().ghs_check_canonical(n, e.m, _ptr(e.u), _ptr(e.v), _stream(), ctypes.byref(ok)))
    assert ok.value == 1


def _check(n, u, v, w, graph_ref=True):
    from oracle import oracle
    ru, rv, rw = (np.ascontiguousarray(a, dtype=np.uint32) for a in (u, v, w))
    e = _device(n, ru, rv, rw)
    _check_against(e, n, ru, rv, rw, oracle.canonicalize_c(n, ru, rv, rw), graph_ref)
    return e


def _random(rng, n, m, vmax=None):
    hi = n if vmax is None else vmax
    return (rng.integers(0, hi, m, dtype=np.uint64).astype(np.uint32), rng.integers(0, hi, m, dtype=np.uint64).astype(np.uint32),
            rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32))


# ---------------------------------------------------------------- tiny
def test_tiny(torch_cuda):
    z = np.zeros(0, np.uint32)
    assert _check(0, z, z, z).m == 0
    assert _check(1, z, z, z).m == 0
    assert _check(1, [0, 0, 0], [0, 0, 0], [1, 2, 3]).m == 0  # only self-loops
    e = _check(2, [1], [0], [7])  # one edge given reversed
    assert (_h(e.u).tolist(), _h(e.v).tolist(), _h(e.w).tolist(), _h(e.src).tolist()) == ([0], [1], [7], [0])


@pytest.mark.parametrize("name", ["selfloops.json"] + [f"ties_{i}.json" for i in range(6)])
def test_fixtures_doubled_and_shuffled(name, torch_cuda):
    fx = load_fixture(name)
    edges = [tuple(e) for e in fx["edges"]]
    both = edges + [(b, a, c) for a, b, c in edges]
    order = np.random.default_rng(1234).permutation(len(both))
    u, v, w = (np.array([both[i][k] for i in order], dtype=np.uint32) for k in range(3))
    _check(fx["num_nodes"], u, v, w)


# ---------------------------------------------------------------- last write wins
@pytest.mark.parametrize("n", [3, 2])
def test_last_write_wins_over_long_runs(n, torch_cuda):
    """Runs of thousands of equal keys cross lane, wave and tile boundaries."""
    rng = np.random.default_rng(5 + n)
    u, v, w = _random(rng, n, 10000)
    e = _check(n, u, v, w)
    pairs = list(zip(_h(e.u).tolist(), _h(e.v).tolist()))
    assert pairs == ([(0, 1), (0, 2), (1, 2)] if n == 3 else [(0, 1)])


# ---------------------------------------------------------------- tile edges
@pytest.mark.parametrize("m_raw", [T - 1, T, T + 1, 2 * T + 1])
def test_tile_sizes(m_raw, torch_cuda):
    rng = np.random.default_rng(m_raw)
    _check(64, *_random(rng, 64, m_raw))


@pytest.mark.parametrize("end", [T - 1, T])
def test_duplicate_run_ending_at_a_tile_edge(end, torch_cuda):
    """Sorted, the run of one pair's copies ends exactly at slot `end`: the last slot of tile 0 or the
    first slot of tile 1 (every other pair is unique, no self-loops, so sorted slots are known)."""
    L = 5
    before = end + 1 - L  # unique pairs sorting in front of the run
    j = np.concatenate([np.arange(1, before + 1), np.full(L, before + 1), np.arange(before + 2, before + 40)])
    assert np.flatnonzero(j == before + 1).tolist() == list(range(end + 1 - L, end + 1))
    rng = np.random.default_rng(end)
    order = rng.permutation(len(j))
    v = j[order].astype(np.uint32)
    u = np.zeros(len(v), np.uint32)
    flip = rng.random(len(v)) < 0.5
    u, v = np.where(flip, v, u), np.where(flip, u, v)
    w = rng.integers(0, 1 << 32, len(v), dtype=np.uint64).astype(np.uint32)
    e = _check(T + 100, u, v, w)
    assert e.m == len(j) - (L - 1)
    # the run's survivor sits at canonical slot `before`, with the last-given weight
    copies = np.flatnonzero(np.maximum(u, v) == before + 1)
    assert int(_h(e.src)[before]) == int(copies.max()) and int(_h(e.w)[before]) == int(w[copies.max()])


# ---------------------------------------------------------------- more tiles than the scan block is wide
def test_more_tiles_than_the_scan_block(torch_cuda):
    rng = np.random.default_rng(77)
    m_raw = 1024 * T + 5
    e = _check(1 << 16, *_random(rng, 1 << 16, m_raw), graph_ref=False)
    assert 0 < e.m < m_raw


# ---------------------------------------------------------------- key width
@pytest.mark.parametrize("n", [2, 3, 4, 5, 1 << 16, (1 << 16) + 1])
def test_key_widths(n, torch_cuda):
    rng = np.random.default_rng(n)
    _check(n, *_random(rng, n, 5000))
    # the top vertices of the range, where the key's fields are all ones
    top = np.array([n - 1, n - 2 if n > 2 else 0, 0], dtype=np.uint32)
    _check(n, rng.choice(top, 500), rng.choice(top, 500), rng.integers(0, 100, 500))


def test_marker_against_a_real_edge(torch_cuda):
    """n = 4, bits = 2: the self-loop (3, 3) IS the marker 0b1111; (2, 3) = 0b1011 must survive."""
    e = _check(4, [3, 3, 2, 0], [3, 2, 3, 3], [9, 10, 11, 12])
    assert list(zip(_h(e.u).tolist(), _h(e.v).tolist(), _h(e.w).tolist())) == [(0, 3, 12), (2, 3, 11)]
    assert _h(e.src).tolist() == [3, 2]


def test_full_width_keys(torch_cuda):
    """n = 2^32 - 1: 64-bit keys, int32 bit patterns >= 2^31."""
    n = U32
    rng = np.random.default_rng(32)
    ends = np.array([0, 5, n - 2, n - 1], dtype=np.uint32)
    u, v = rng.choice(ends, 300), rng.choice(ends, 300)
    u[7], v[7] = n - 1, n - 1
    u[299], v[299] = n - 1, 0
    e = _check(n, u, v, rng.integers(0, 1 << 32, 300, dtype=np.uint64))
    assert e.m == 6


# ---------------------------------------------------------------- out of range
def test_out_of_range_endpoints(torch_cuda):
    """An endpoint >= n anywhere in the list: GHS_E_ARG from the kernel's own range check, nothing
    out of bounds — the next call on the same stream succeeds."""
    N = _N()
    n, m_raw = 64, T + 1
    rng = np.random.default_rng(9)
    u0, v0, w0 = _random(rng, n, m_raw)
    for bad in (n, U32):
        for pos in (0, m_raw // 2, m_raw - 1):
            for side in (0, 1):
                u, v = u0.copy(), v0.copy()
                (u if side == 0 else v)[pos] = bad
                with pytest.raises(N.GHSError) as ei:
                    _device(n, u, v, w0)
                assert ei.value.code == N.GHS_E_ARG and "vertex id out of range" in str(ei.value), (bad, pos, side)
    _check(n, u0, v0, w0)


# ---------------------------------------------------------------- alignment, temp
def _raw_call(n, ru, rv, rw, cu, cv, cw, src, tmp, tb):
    from distributed_ghs_implementation_amd.device import _ptr, _stream
    m = ctypes.c_uint64(0)
    rc = _N().load().ghs_canonicalize_device(n, ru.numel(), _ptr(ru), _ptr(rv), _ptr(rw), _ptr(cu), _ptr(cv),
                                             _ptr(cw), _ptr(src), ctypes.byref(m), _ptr(tmp), tb, _stream())
    return rc, m.value


@pytest.mark.parametrize("m_raw", [2, 2 * T + 1])
def test_unaligned_raw_inputs(m_raw, torch_cuda):
    """Raw inputs that are only 4-byte aligned (tensor[k:] slices) give what aligned copies give: the
    same offset on u and v (vector body behind a scalar head) and different offsets (all scalar)."""
    from distributed_ghs_implementation_amd.device import canonicalize_device
    rng = np.random.default_rng(m_raw)
    n = 64
    u, v, w = _random(rng, n, m_raw)
    ref = _device(n, u, v, w)
    want = [_h(x).copy() for x in (ref.u, ref.v, ref.w, ref.src)]

    def sliced(a, k):
        t = _t(np.concatenate([np.zeros(k, np.uint32), a]))[k:]
        assert t.data_ptr() % 16 == (4 * k) % 16
        return t
    for ku, kv, kw in [(1, 1, 1), (3, 3, 0), (1, 2, 3), (0, 1, 0), (2, 0, 1), (2, 2, 2)]:
        e = canonicalize_device(n, sliced(u, ku), sliced(v, kv), sliced(w, kw))
        got = [_h(x) for x in (e.u, e.v, e.w, e.src)]
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), (ku, kv, kw)


def test_misaligned_output_and_short_temp(torch_cuda):
    import torch
    N = _N()
    L = N.load()
    n, m_raw = 64, T + 1
    u, v, w = (_t(a) for a in _random(np.random.default_rng(3), n, m_raw))
    tb = int(L.ghs_canonicalize_temp_bytes(n, m_raw))
    tmp = torch.empty(tb + 16, dtype=torch.uint8, device="cuda")
    out = [torch.empty(m_raw + 4, dtype=torch.int32, device="cuda") for _ in range(4)]
    cu, cv, cw, src = (o[:m_raw] for o in out)
    for k in range(4):  # each output in turn as a 4-byte-aligned slice
        args = [cu, cv, cw, src]
        args[k] = out[k][1:m_raw + 1]
        rc, _ = _raw_call(n, u, v, w, *args, tmp, tb)
        assert rc == N.GHS_E_ARG and b"aligned" in L.ghs_last_error(), k
    rc, _ = _raw_call(n, u, v, w, cu, cv, cw, src, tmp[4:], tb)
    assert rc == N.GHS_E_ARG and b"aligned" in L.ghs_last_error()
    rc, _ = _raw_call(n, u, v, w, cu, cv, cw, src, tmp, tb - 1)
    assert rc == N.GHS_E_NOMEM
    rc, m = _raw_call(n, u, v, w, cu, cv, cw, None, tmp, tb)  # src may be NULL
    assert rc == N.GHS_OK
    ref = _device(n, _h(u), _h(v), _h(w), keep_src=False)
    assert ref.src is None and m == ref.m
    assert all(torch.equal(a[:m], b) for a, b in zip((cu, cv, cw), (ref.u, ref.v, ref.w)))


def test_deterministic(torch_cuda):
    rng = np.random.default_rng(15)
    u, v, w = _random(rng, 200, 3 * T + 17)
    a, b = _device(200, u, v, w), _device(200, u, v, w)
    assert a.m == b.m
    for x, y in zip((a.u, a.v, a.w, a.src), (b.u, b.v, b.w, b.src)):
        assert _h(x).tobytes() == _h(y).tobytes()


# ---------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def multigraph():
    rng = np.random.default_rng(2000)
    n, m_raw = 2000, 20000
    u = rng.integers(0, n, m_raw).astype(np.uint32)
    v = rng.integers(0, n, m_raw).astype(np.uint32)
    w = rng.integers(0, 9, m_raw).astype(np.uint32)
    from oracle import oracle
    ou, ov, ow = oracle.canonicalize_c(n, u, v, w)
    return n, u, v, w, (ou, ov, ow), oracle.kruskal_c(n, ou, ov, ow)


def test_solve_on_the_device_canonical_list(multigraph, torch_cuda):
    from distributed_ghs_implementation_amd.device import DeviceMST
    n, u, v, w, ref, (ref_in, ref_tw, ref_k) = multigraph
    e = _device(n, u, v, w)
    _check_against(e, n, u, v, w, ref)
    for edges in (e, _device(n, u, v, w).with_csr()):
        eng = DeviceMST(edges)
        res, _ = eng.run()
        assert np.array_equal(eng.in_mst_host(), ref_in.astype(bool))
        assert res.total_weight == ref_tw and res.num_mst_edges == ref_k
        ids = edges.raw_eids(eng.in_mst).cpu().numpy()
        assert ids.dtype == np.int64 and len(ids) == ref_k
        sel = ref_in.astype(bool)
        assert np.array_equal(np.minimum(u[ids], v[ids]), ref[0][sel])
        assert np.array_equal(np.maximum(u[ids], v[ids]), ref[1][sel])
        assert np.array_equal(w[ids], ref[2][sel])
        assert int(w[ids].astype(np.uint64).sum()) == res.total_weight


def test_raw_eids_needs_src(multigraph, torch_cuda):
    from distributed_ghs_implementation_amd.device import DeviceMST
    n, u, v, w, _, _ = multigraph
    e = _device(n, u, v, w, keep_src=False)
    eng = DeviceMST(e)
    eng.run()
    with pytest.raises(ValueError):
        e.raw_eids(eng.in_mst)


def test_edges_call_equals_host_canonicalize(multigraph, torch_cuda):
    from distributed_ghs_implementation_amd import canonicalize, minimum_spanning_forest, minimum_spanning_forest_edges
    n, u, v, w, _, _ = multigraph
    got = minimum_spanning_forest_edges(n, u, v, w)
    want = minimum_spanning_forest(canonicalize(n, u=u, v=v, w=w))
    assert want.raw_ids is None
    assert np.array_equal(got.in_mst, want.in_mst) and got.total_weight == want.total_weight
    assert got.triples() == want.triples() and got.edges() == want.edges()
    assert got.to_dict() == want.to_dict()
    ids = got.raw_ids
    assert ids.dtype == np.int64
    assert [(int(min(a, b)), int(max(a, b)), int(c)) for a, b, c in zip(u[ids], v[ids], w[ids])] == got.triples()


def test_int64_tensors(multigraph, torch_cuda):
    import torch
    from distributed_ghs_implementation_amd.device import DeviceEdges, canonicalize_device
    n, u, v, w, ref, _ = multigraph
    big = w.astype(np.int64) + (np.arange(len(w)) % 2) * ((1 << 32) - 9)  # weights on both sides of 2^31
    tu, tv, tw = (torch.from_numpy(a.astype(np.int64)).cuda() for a in (u, v, big))
    e = canonicalize_device(n, tu, tv, tw)
    from oracle import oracle
    _check_against(e, n, u, v, big.astype(np.uint32), oracle.canonicalize_c(n, u, v, big.astype(np.uint32)))
    f = DeviceEdges.from_raw(n, u.astype(np.int64), v.astype(np.int64), big)
    assert all(torch.equal(a, b) for a, b in zip((e.u, e.v, e.w, e.src), (f.u, f.v, f.w, f.src)))
    for k in range(3):
        bad = [tu.clone(), tv.clone(), tw.clone()]
        bad[k][len(u) // 2] = 1 << 32
        with pytest.raises(ValueError):
            canonicalize_device(n, *bad)
        bad[k][len(u) // 2] = -1
        with pytest.raises(ValueError):
            canonicalize_device(n, *bad)
