"""GPU: the weight-rank pass (ghs_weight_ranks_device: k_weight_keys, rocPRIM pairs sort,
k_rank_count / k_uniq_scan / k_rank_write) against numpy's np.searchsorted(np.unique(w), w), bit for
bit, for the four weight types; and rank_weights=True end to end against graph.canonicalize and
minimum_spanning_forest on the host-ranked graph."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 4096  # the head-flag pass's tile (csrc/ingest.hip UQ_TILE)
TYPES = ["f32", "f64", "i64", "u64"]
DTYPE = {"f32": np.float32, "f64": np.float64, "i64": np.int64, "u64": np.uint64}


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


def _wtype(t):
    N = _N()
    return {"f32": N.GHS_W_FLOAT32, "f64": N.GHS_W_FLOAT64, "i64": N.GHS_W_INT64, "u64": N.GHS_W_UINT64}[t]


def _tensor(w):
    """numpy array of one of the four dtypes -> GPU tensor with the same bits (uint64 as int64)."""
    import torch
    w = np.ascontiguousarray(w)
    return torch.from_numpy(w.view(np.int64).copy() if w.dtype == np.uint64 else w.copy()).cuda()


def _device(t, w):
    from distributed_ghs_implementation_amd.device import weight_ranks
    ranks, distinct = weight_ranks(_tensor(w), _wtype(t))
    return ranks.cpu().numpy().view("uint32"), distinct


def _reference(w):
    uniq = np.unique(w)
    return np.searchsorted(uniq, w).astype(np.uint32), len(uniq)


def _check(t, w):
    w = np.ascontiguousarray(w, dtype=DTYPE[t])
    got, distinct = _device(t, w)
    want, k = _reference(w)
    assert distinct == k
    assert got.dtype == want.dtype and np.array_equal(got, want)
    return got


def _specials(t):
    if t in ("f32", "f64"):
        dt = DTYPE[t]
        fi = np.finfo(dt)
        one = dt(1.0)
        pos = [dt(0.0), dt(np.inf), fi.tiny, fi.smallest_subnormal, fi.max, one, np.nextafter(one, dt(2.0)),
               dt(2.5), dt(1e-3), dt(12345.678)]
        vals = pos + [-x for x in pos]  # holds -0.0 next to +0.0
        if t == "f64":  # pairs that are one value once rounded to float32
            for a, b in ((1.0, 1.0 + 2.0 ** -40), (3.0, 3.0 - 2.0 ** -45), (-7.5, -7.5 - 2.0 ** -35),
                         (1e30, np.nextafter(1e30, 2e30))):
                assert a != b and np.float32(a) == np.float32(b)
                vals += [a, b]
        return np.array(vals, dtype=dt)
    if t == "i64":
        ii = np.iinfo(np.int64)
        return np.array([ii.min, ii.min + 1, -(1 << 32), -1, 0, 1, (1 << 32) - 1, 1 << 32, ii.max - 1, ii.max], dtype=np.int64)
    return np.array([0, 1, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 1], dtype=np.uint64)


def _random(t, rng, k):
    """k random values of the type over its whole range (no NaN)."""
    if t in ("f32", "f64"):
        ut = np.uint32 if t == "f32" else np.uint64
        bits = rng.integers(0, np.iinfo(ut).max, k, dtype=ut, endpoint=True)
        x = bits.view(DTYPE[t])
        return np.where(np.isnan(x), DTYPE[t](0.25), x)
    if t == "i64":
        return rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, k, dtype=np.int64, endpoint=True)
    return rng.integers(0, np.iinfo(np.uint64).max, k, dtype=np.uint64, endpoint=True)


def _ladder(t, k):
    """k strictly ascending values of the type, on both sides of zero (of 2^63 for uint64)."""
    if t in ("f32", "f64"):
        return (np.arange(k, dtype=np.float64) - k // 2).astype(DTYPE[t]) / DTYPE[t](4)
    if t == "i64":
        return (np.arange(k, dtype=np.int64) - k // 2) * np.int64(1 << 33)
    return np.arange(k, dtype=np.uint64) + np.uint64((1 << 63) - k // 2)


def _mixed(t, rng, m):
    """m weights drawn (with ties) from the type's special values and about m / 2 random ones."""
    pool = np.concatenate([_specials(t), _random(t, rng, max(1, m // 2))])
    return rng.choice(pool, m)


# ---------------------------------------------------------------- the key map on the special values
@pytest.mark.parametrize("t", TYPES)
def test_special_values(t, torch_cuda):
    s = _specials(t)
    got = _check(t, s)
    if t in ("f32", "f64"):
        dt = DTYPE[t]
        fi = np.finfo(dt)
        zeros = got[s == 0]
        assert len(zeros) == 2 and zeros[0] == zeros[1]  # -0.0 and +0.0 are one value
        assert got[np.flatnonzero(s == -np.inf)[0]] == 0 and got[np.flatnonzero(s == np.inf)[0]] == got.max()
        # denormals and neighbours in the last mantissa bit are values of their own
        r = {float(x): int(g) for x, g in zip(s, got)}
        assert r[0.0] + 1 == r[float(fi.smallest_subnormal)] < r[float(fi.tiny)]
        assert r[1.0] + 1 == r[float(np.nextafter(dt(1.0), dt(2.0)))]
    rng = np.random.default_rng(11)
    _check(t, rng.permutation(np.concatenate([s, s, s])))


def test_float64_is_not_narrowed(torch_cuda):
    a = np.array([1.0, 1.0 + 2.0 ** -40, 1.0 + 2.0 ** -41, 1.0 - 2.0 ** -50, 1.0], dtype=np.float64)
    assert len(np.unique(a.astype(np.float32))) == 1
    assert _check("f64", a).tolist() == [1, 3, 2, 0, 1]


# ---------------------------------------------------------------- sizes around the tile
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("m", [1, 2, T - 1, T, T + 1, 2 * T + 1])
def test_tile_sizes(t, m, torch_cuda):
    _check(t, _mixed(t, np.random.default_rng(m), m))


@pytest.mark.parametrize("t", TYPES)
def test_more_tiles_than_the_scan_block(t, torch_cuda):
    rng = np.random.default_rng(77)
    m = 1024 * T + 5
    w = _random(t, rng, m)
    w[rng.integers(0, m, m // 4)] = w[rng.integers(0, m, m // 4)]  # about a quarter repeated
    _check(t, w)


def test_empty(torch_cuda):
    for t in TYPES:
        got, distinct = _device(t, np.zeros(0, DTYPE[t]))
        assert len(got) == 0 and distinct == 0


# ---------------------------------------------------------------- ties
@pytest.mark.parametrize("t", TYPES)
def test_all_equal_all_distinct_two_values(t, torch_cuda):
    rng = np.random.default_rng(5)
    m = 2 * T + 1
    lad = _ladder(t, m)
    assert np.all(lad[1:] > lad[:-1])
    for x in (lad[0], lad[m // 2], lad[-1]):
        got = _check(t, np.full(m, x))
        assert not got.any()
    got = _check(t, rng.permutation(lad))
    assert sorted(got.tolist()) == list(range(m))
    two = _specials(t)[[1, -1]]
    got = _check(t, rng.choice(two, m))
    assert set(got.tolist()) == {0, 1}


@pytest.mark.parametrize("t", TYPES)
def test_runs_meeting_at_a_tile_edge(t, torch_cuda):
    """Sorted, a run of equal values ends exactly at the last slot of tile 0 and another starts at
    the first slot of tile 1 (every other value is distinct, so sorted slots are known)."""
    L1, L2 = 5, 7
    lad = _ladder(t, T + 50)
    before = T - L1  # distinct values sorting in front of the first run
    sorted_w = np.concatenate([lad[:before], np.full(L1, lad[before]), np.full(L2, lad[before + 1]),
                               lad[before + 2:before + 40]])
    assert np.flatnonzero(sorted_w == lad[before]).tolist() == list(range(T - L1, T))
    assert np.flatnonzero(sorted_w == lad[before + 1]).tolist() == list(range(T, T + L2))
    rng = np.random.default_rng(3)
    w = rng.permutation(sorted_w)
    got = _check(t, w)
    assert set(got[w == lad[before]].tolist()) == {before} and set(got[w == lad[before + 1]].tolist()) == {before + 1}
    # the same with the runs shifted by one slot to either side of the edge
    for shift in (-1, 1):
        s2 = np.concatenate([lad[:before + shift], np.full(L1, lad[before + shift]), np.full(L2, lad[before + shift + 1]),
                             lad[before + shift + 2:before + 40]])
        _check(t, rng.permutation(s2))


@pytest.mark.parametrize("t", TYPES)
def test_run_spanning_three_whole_tiles(t, torch_cuda):
    """Sorted: 100 distinct values, one value 4 T times (tiles 1, 2, 3 hold no head at all), 100
    distinct values."""
    lad = _ladder(t, 201)
    sorted_w = np.concatenate([lad[:100], np.full(4 * T, lad[100]), lad[101:]])
    rng = np.random.default_rng(4)
    w = rng.permutation(sorted_w)
    got = _check(t, w)
    assert set(got[w == lad[100]].tolist()) == {100} and int(got.max()) == 200


# ---------------------------------------------------------------- the raw entry: NaN, slices, arguments
def _raw_call(wtype, m, w_ptr, ranks_ptr, tmp, tb):
    from distributed_ghs_implementation_amd.device import _ptr, _stream
    d = ctypes.c_uint64(0)
    rc = _N().load().ghs_weight_ranks_device(wtype, m, w_ptr, ranks_ptr, ctypes.byref(d), _ptr(tmp), tb, _stream())
    return rc, d.value


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_nan_anywhere_then_a_good_call_on_the_same_temp(t, torch_cuda):
    import torch
    from distributed_ghs_implementation_amd.device import _ptr
    N = _N()
    L = N.load()
    m = 2 * T + 1
    ut = np.uint32 if t == "f32" else np.uint64
    exp = 0x7f800000 if t == "f32" else 0x7ff0000000000000
    quiet = 0x00400000 if t == "f32" else 0x0008000000000000
    sign = 1 << (31 if t == "f32" else 63)
    nans = [exp | quiet, exp | 1, sign | exp | quiet, sign | exp | 1, exp | (quiet - 1), (sign << 1) - 1]
    good = _mixed(t, np.random.default_rng(8), m).astype(DTYPE[t])
    want, k = _reference(good)
    tb = int(L.ghs_weight_ranks_temp_bytes(_wtype(t), m))
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    ranks = torch.empty(m, dtype=torch.int32, device="cuda")
    gw = _tensor(good)
    for bits in nans:
        assert np.isnan(np.array([bits], dtype=ut).view(DTYPE[t])[0])
        for pos in (0, m // 2, m - 1):
            bad = good.copy()
            bad.view(ut)[pos] = bits
            bw = _tensor(bad)
            rc, _ = _raw_call(_wtype(t), m, _ptr(bw), _ptr(ranks), tmp, tb)
            assert rc == N.GHS_E_ARG and b"NaN weight" in L.ghs_last_error(), (hex(bits), pos)
        rc, distinct = _raw_call(_wtype(t), m, _ptr(gw), _ptr(ranks), tmp, tb)
        assert rc == N.GHS_OK and distinct == k
        assert np.array_equal(ranks.cpu().numpy().view("uint32"), want)
    from distributed_ghs_implementation_amd.device import weight_ranks
    with pytest.raises(N.GHSError) as ei:
        weight_ranks(bw)
    assert ei.value.code == N.GHS_E_ARG and "NaN weight" in str(ei.value)


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("m", [1, 2, 5, 2 * T + 1])
def test_sliced_inputs(t, m, torch_cuda):
    """Inputs that have only their element's own alignment (tensor[k:] slices) give what an aligned
    copy gives."""
    from distributed_ghs_implementation_amd.device import weight_ranks
    w = _mixed(t, np.random.default_rng(m), m).astype(DTYPE[t])
    want, k = _reference(w)
    size = w.dtype.itemsize
    for pad in ((1, 2, 3) if size == 4 else (1,)):
        sl = _tensor(np.concatenate([np.zeros(pad, w.dtype), w]))[pad:]
        assert sl.data_ptr() % 16 == (size * pad) % 16 != 0
        ranks, distinct = weight_ranks(sl, _wtype(t))
        assert distinct == k and np.array_equal(ranks.cpu().numpy().view("uint32"), want), pad


def test_short_temp_and_misaligned_ranks(torch_cuda):
    import torch
    from distributed_ghs_implementation_amd.device import _ptr
    N = _N()
    L = N.load()
    m = T + 1
    for t in TYPES:
        w = _tensor(_mixed(t, np.random.default_rng(2), m).astype(DTYPE[t]))
        tb = int(L.ghs_weight_ranks_temp_bytes(_wtype(t), m))
        tmp = torch.empty(tb + 16, dtype=torch.uint8, device="cuda")
        ranks = torch.empty(m + 4, dtype=torch.int32, device="cuda")
        rc, _ = _raw_call(_wtype(t), m, _ptr(w), _ptr(ranks), tmp, tb - 1)
        assert rc == N.GHS_E_NOMEM
        for k in (1, 2, 3):
            rc, _ = _raw_call(_wtype(t), m, _ptr(w), ctypes.c_void_p(ranks.data_ptr() + k), tmp, tb)
            assert rc == N.GHS_E_ARG and b"aligned" in L.ghs_last_error(), k
        rc, _ = _raw_call(_wtype(t), m, _ptr(w), _ptr(ranks), tmp[4:], tb)
        assert rc == N.GHS_E_ARG and b"aligned" in L.ghs_last_error()
        rc, _ = _raw_call(_wtype(t), m, ctypes.c_void_p(w.data_ptr() + 2), _ptr(ranks), tmp, tb)
        assert rc == N.GHS_E_ARG and b"aligned" in L.ghs_last_error()
        rc, _ = _raw_call(_wtype(t), m, _ptr(w), _ptr(tmp), tmp, tb)
        assert rc == N.GHS_E_ARG and b"overlap" in L.ghs_last_error()
        # ranks at a 4-byte (not 16-byte) aligned slice is fine
        rc, distinct = _raw_call(_wtype(t), m, _ptr(w), _ptr(ranks[1:]), tmp, tb)
        want, k = _reference(w.cpu().numpy().view(DTYPE[t]))
        assert rc == N.GHS_OK and distinct == k
        assert np.array_equal(ranks[1:m + 1].cpu().numpy().view("uint32"), want)


@pytest.mark.parametrize("t", TYPES)
def test_deterministic(t, torch_cuda):
    w = _mixed(t, np.random.default_rng(15), 3 * T + 17).astype(DTYPE[t])
    (a, ka), (b, kb) = _device(t, w), _device(t, w)
    assert ka == kb and a.tobytes() == b.tobytes()


def test_dtype_rules_of_the_python_call(torch_cuda):
    import torch
    from distributed_ghs_implementation_amd.device import weight_ranks
    N = _N()
    for bad in (torch.zeros(3, dtype=torch.int32, device="cuda"), torch.zeros(3, dtype=torch.float16, device="cuda"),
                torch.zeros(3, dtype=torch.complex64, device="cuda"), torch.zeros((2, 2), device="cuda"), [1.0, 2.0]):
        with pytest.raises(ValueError):
            weight_ranks(bad)
    with pytest.raises(ValueError):
        weight_ranks(torch.zeros(3, device="cuda"), N.GHS_W_UINT64)
    ranks, distinct = weight_ranks(torch.tensor([2.5, -1.0, 2.5, 0.0], device="cuda"))
    assert ranks.dtype == torch.int32 and ranks.tolist() == [2, 0, 2, 1] and distinct == 3
    # every second element: copied, not read with a stride
    ranks, distinct = weight_ranks(torch.tensor([5, 0, -5, 0, 7, 0], device="cuda")[::2])
    assert ranks.tolist() == [1, 0, 2] and distinct == 3


# ---------------------------------------------------------------- end to end
def _host_last(u, v):
    """Per unordered pair (self-loops dropped), in canonical order: the largest raw index."""
    a, b = u.astype(np.uint64), v.astype(np.uint64)
    keep = a != b
    key = (np.minimum(a, b) << np.uint64(32)) | np.maximum(a, b)
    uniq, inv = np.unique(key[keep], return_inverse=True)
    last = np.full(len(uniq), -1, dtype=np.int64)
    np.maximum.at(last, inv.ravel(), np.flatnonzero(keep))
    return last


@pytest.fixture(scope="module")
def multigraph():
    """n = 2000, 20000 raw edges with self-loops and repeated pairs in both orientations."""
    rng = np.random.default_rng(2000)
    n, m_raw = 2000, 20000
    u = rng.integers(0, n, m_raw).astype(np.int64)
    v = rng.integers(0, n, m_raw).astype(np.int64)
    u[::97] = v[::97]                       # self-loops
    u[1::50], v[1::50] = v[0:-1:50].copy(), u[0:-1:50].copy()  # the previous edge again, reversed
    return n, u, v


def _weights(kind, m_raw):
    rng = np.random.default_rng(len(kind))
    if kind == "f64-ties":
        w = rng.integers(-40, 40, m_raw).astype(np.float64) / 8.0
        w[::13] += 2.0 ** -45  # apart only below float32's precision
        return w
    if kind == "i64-negative":
        w = rng.integers(-50, 50, m_raw).astype(np.int64)
        w[::7] -= np.int64(1) << 40
        w[3::11] += np.int64(1) << 33
        return w
    if kind == "f32":
        return np.round(rng.normal(0.0, 10.0, m_raw), 1).astype(np.float32)
    raise AssertionError(kind)


KINDS = ["f64-ties", "i64-negative", "f32"]


@pytest.fixture(scope="module")
def host_results(multigraph):
    """graph.canonicalize's rank-mapped graph per weight kind (the host reference), made once."""
    from distributed_ghs_implementation_amd import canonicalize
    n, u, v = multigraph
    out = {}
    for kind in KINDS:
        w = _weights(kind, len(u))
        g = canonicalize(n, u=u, v=v, w=w)
        assert g.weights is not None and g.m < len(u)
        out[kind] = (w, g)
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_canonicalize_device_with_rank_weights(kind, multigraph, host_results, torch_cuda):
    import torch
    from distributed_ghs_implementation_amd.device import canonicalize_device
    n, u, v = multigraph
    w, g = host_results[kind]
    tu, tv, tw = (torch.from_numpy(a).cuda() for a in (u, v, w))
    for keep_src in (True, False):  # forced on either way
        e = canonicalize_device(n, tu, tv, tw, keep_src=keep_src, rank_weights=True)
        cu, cv, cw = (x.cpu().numpy().view("uint32") for x in (e.u, e.v, e.w))
        assert e.m == g.m
        assert np.array_equal(cu, g.u) and np.array_equal(cv, g.v) and np.array_equal(cw, g.w)
        src = e.src.cpu().numpy().view("uint32").astype(np.int64)
        assert np.array_equal(src, _host_last(u, v))
        got_w = e.weights.cpu().numpy()
        assert got_w.dtype == g.weights.dtype and got_w.tobytes() == g.weights.tobytes()
        assert np.array_equal(w[src], got_w)
        h = e.to_host()
        assert h.weights.tobytes() == g.weights.tobytes() and np.array_equal(h.w, g.w)
        assert e.csr_only().weights is e.weights
    # the default call on the same input keeps its refusal
    with pytest.raises(ValueError):
        canonicalize_device(n, tu, tv, tw)


@pytest.mark.parametrize("kind", KINDS)
def test_edges_call_with_rank_weights_equals_the_host_path(kind, multigraph, host_results, torch_cuda):
    from distributed_ghs_implementation_amd import minimum_spanning_forest, minimum_spanning_forest_edges
    n, u, v = multigraph
    w, g = host_results[kind]
    want = minimum_spanning_forest(g)
    got = minimum_spanning_forest_edges(n, u, v, w, rank_weights=True)
    assert np.array_equal(got.in_mst, want.in_mst)
    assert got.triples() == want.triples() and got.edges() == want.edges()
    assert got.to_dict() == want.to_dict()
    assert got.total_weight == want.total_weight and type(got.total_weight) is type(want.total_weight)
    ids = got.raw_ids
    assert ids.dtype == np.int64 and len(ids) == got.num_edges
    assert [(int(min(a, b)), int(max(a, b)), c.item()) for a, b, c in zip(u[ids], v[ids], w[ids])] == got.triples()
    with pytest.raises(ValueError, match="canonicalize"):
        minimum_spanning_forest_edges(n, u, v, w)


def test_widened_and_unsigned_inputs(multigraph, torch_cuda):
    """float16 / narrow integers are widened (exactly), uint64 goes through at full width."""
    import torch
    from distributed_ghs_implementation_amd import canonicalize
    from distributed_ghs_implementation_amd.device import DeviceEdges, canonicalize_device
    n, u, v = multigraph
    rng = np.random.default_rng(6)
    m_raw = len(u)
    cases = [rng.integers(-100, 100, m_raw).astype(np.int8), rng.integers(-9, 9, m_raw).astype(np.int32),
             (rng.integers(-40, 40, m_raw) / 4.0).astype(np.float16),
             rng.integers(0, 50, m_raw).astype(np.uint64) + np.uint64((1 << 63) - 25)]
    for w in cases:
        g = canonicalize(n, u=u, v=v, w=w)
        assert g.weights is not None
        e = DeviceEdges.from_raw(n, u, v, w, rank_weights=True)
        for a, b in ((e.u, g.u), (e.v, g.v), (e.w, g.w)):
            assert np.array_equal(a.cpu().numpy().view("uint32"), b)
        got_w = e.weights.cpu().numpy()
        assert np.array_equal(got_w, g.weights) and got_w.dtype.kind == g.weights.dtype.kind
        if w.dtype != np.uint64:
            f = canonicalize_device(n, torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda(),
                                    torch.from_numpy(w).cuda(), rank_weights=True)
            assert torch.equal(f.w, e.w) and torch.equal(f.src, e.src) and torch.equal(f.weights, e.weights)
    with pytest.raises(_N().GHSError) as ei:
        DeviceEdges.from_raw(n, u, v, np.where(np.arange(m_raw) == 5, np.nan, 1.0), rank_weights=True)
    assert ei.value.code == _N().GHS_E_ARG and "NaN weight" in str(ei.value)
