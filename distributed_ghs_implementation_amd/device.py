"""Device-resident pipeline (torch supplies device memory and the stream; HIP does the work).

    edges = generate_rmat(24)                    # canonical u, v, w in HBM (BASELINE config 3)
    eng = DeviceMST(edges)                       # workspace allocated once
    res, stats = eng.run()                       # canonical edges -> in_mst flags + weight

`DeviceMST.run()` is the timed unit of bench.py: from the device-resident canonical edge list to
the in_mst flags and total weight (BASELINE.md "Definitions") — validation, the weight-level
plan, every level's filter + arc build, and all Boruvka rounds. Nothing falls back to the CPU:
without the HIP library or a GPU the constructors raise.
"""
import ctypes

import torch

from . import _native


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class DeviceEdges:
    """Canonical edge list in HBM: n, u/v/w as int32 tensors holding uint32 bit patterns. `off`
    (ABI 9, optional): the CSR row offsets of the same list (n + 1 entries, `with_csr()`); an
    engine built with csr=True streams (off, v, w) — 8 B per edge instead of 12 — and u may then
    be dropped (`csr_only()`). `src` (optional, lists made by `canonicalize_device` / `from_raw`):
    per canonical edge, the index of the caller's raw edge it came from (int32, uint32 bits).
    `weights` (optional, lists made with rank_weights=True): the caller's own weights in canonical
    order (w_raw[src], on the device) when w holds their ranks; `to_host()` hands them on as
    `CanonicalGraph.weights`, so results report the caller's values."""

    def __init__(self, n, u, v, w, off=None, src=None, weights=None):
        self.n = int(n)
        self.u, self.v, self.w = u, v, w
        self.off = off
        self.src = src
        self.weights = weights

    @property
    def m(self):
        return int(self.v.numel())

    def with_csr(self):
        """Add the CSR row offsets (built on the device from the sorted u)."""
        if self.off is None:
            L = _native.load()
            off = torch.empty(self.n + 1, dtype=torch.int32, device=self.device)
            _native.check(L.ghs_csr_offsets(self.n, self.m, _ptr(self.u), _ptr(off), _stream()))
            self.off = off
        return self

    def csr_only(self):
        """The CSR form alone (u released): off, v, w."""
        self.with_csr()
        return DeviceEdges(self.n, None, self.v, self.w, self.off, self.src, self.weights)

    @property
    def device(self):
        return self.v.device

    @classmethod
    def from_host(cls, graph, device="cuda"):
        """CanonicalGraph (numpy) -> device tensors (H2D copy)."""
        def dev(a):
            return torch.from_numpy(a.view("int32").copy()).to(device)
        return cls(graph.n, dev(graph.u), dev(graph.v), dev(graph.w))

    @classmethod
    def from_raw(cls, n, u, v, w, device="cuda", rank_weights=False):
        """Raw numpy integer arrays (any order, either orientation, repeats, self-loops) -> the
        canonical list, sorted and de-duplicated on the device (`canonicalize_device`): one H2D copy
        of the three arrays, no host sort. Values outside [0, 2^32) raise ValueError.
        rank_weights=True: w may be any float or integer array (float16 is widened to float32,
        integers narrower than 64 bits to int64; uint64 is accepted); it travels in its own H2D copy
        at full width and is rank-mapped on the device (`weight_ranks`), and the result's `weights`
        holds the caller's values. A NaN raises GHSError (GHS_E_ARG)."""
        if not rank_weights:
            packed = _pack_raw(u, v, w)
            _native.load()
            _native.require_gpu()
            dev = torch.from_numpy(packed.view("int32")).to(device)
            return canonicalize_device(n, dev[0], dev[1], dev[2])
        import numpy as np
        wa = np.asarray(w)
        if wa.ndim != 1:
            raise ValueError("u, v, w must be one-dimensional arrays of equal length")
        packed = _pack_u32((("u", u), ("v", v)), len(wa))
        wa, wtype = _rankable_array(wa)
        _native.load()
        _native.require_gpu()
        dev = torch.from_numpy(packed.view("int32")).to(device)
        wt = torch.from_numpy(np.ascontiguousarray(wa)).to(device)
        return _canonicalize_ranked(n, dev[0], dev[1], wt, wtype)

    def raw_eids(self, in_mst):
        """The caller's edge indices of the MSF edges (in_mst: the m flags of a solve of this list),
        in canonical order, as an int64 device tensor."""
        if self.src is None:
            raise ValueError("this edge list carries no raw indices (build it with canonicalize_device / from_raw)")
        eids = flags_to_eids(in_mst, 0, self.m)
        return self.src[eids].to(torch.int64) & 0xFFFFFFFF

    def mutual_reachability(self, min_samples=5, short_rows="error", include_self=False, in_place=False):
        """`mutual_reachability` of this list: the core distances and the weights HDBSCAN wants."""
        return mutual_reachability(self, min_samples=min_samples, short_rows=short_rows, include_self=include_self,
                                   in_place=in_place)

    def hdbscan(self, min_cluster_size=5, min_samples=None, method="eom", allow_single_cluster=False, short_rows="error",
                include_self=False):
        """`hdbscan` of this list: mutual reachability, the solve, the dendrogram and the clusters."""
        return hdbscan(self, min_cluster_size=min_cluster_size, min_samples=min_samples, method=method,
                       allow_single_cluster=allow_single_cluster, short_rows=short_rows, include_self=include_self)

    def u_host(self):
        """u as a host uint32 array (expanded from the offsets for a CSR-only list)."""
        import numpy as np
        if self.u is not None:
            return self.u.cpu().numpy().view("uint32")
        off = self.off.cpu().numpy().view("uint32").astype(np.int64)
        return np.repeat(np.arange(self.n, dtype=np.uint32), np.diff(off))

    def to_host(self):
        from .graph import CanonicalGraph
        weights = None if self.weights is None else self.weights.cpu().numpy()
        return CanonicalGraph(self.n, self.u_host(), self.v.cpu().numpy().view("uint32"),
                              self.w.cpu().numpy().view("uint32"), weights=weights)


def _pack_raw(u, v, w):
    """Raw numpy integer arrays -> one (3, m) uint32 array (a single H2D copy); ValueError for
    anything but integers in [0, 2^32)."""
    return _pack_u32((("u", u), ("v", v), ("w", w)))


def _pack_u32(named, m=None):
    """[(name, array)] -> one (k, m) uint32 array; m: the length every array must have (default:
    the first one's)."""
    import numpy as np
    names = [name for name, _ in named]
    arrs = [np.asarray(a) for _, a in named]
    if m is None:
        m = len(arrs[0]) if arrs[0].ndim == 1 else -1
    if any(a.ndim != 1 or len(a) != m for a in arrs):
        raise ValueError("u, v, w must be one-dimensional arrays of equal length")
    packed = np.empty((len(arrs), m), dtype=np.uint32)
    for k, (name, a) in enumerate(zip(names, arrs)):
        if a.size == 0:
            continue
        if a.dtype.kind not in "iu":
            raise ValueError(f"{name}: the device ingest takes integers in [0, 2^32) only "
                             "(graph.canonicalize accepts any numeric weights)")
        if int(a.min()) < 0 or int(a.max()) >= (1 << 32):
            raise ValueError(f"{name}: values must be in [0, 2^32) "
                             "(graph.canonicalize accepts any numeric weights)")
        packed[k] = a.astype(np.uint32, copy=False)
    return packed


def _as_u32_tensor(t, name):
    """A device tensor of uint32 bit patterns: int32 as it is, int64 range-checked on the device
    (one flag read back) and narrowed."""
    if t.dtype == torch.int32:
        return t.contiguous()
    if t.dtype != torch.int64:
        raise ValueError(f"{name}: int32 (uint32 bit patterns) or int64 tensor expected, got {t.dtype}")
    if t.numel() and bool(((t < 0) | (t >= (1 << 32))).any()):
        raise ValueError(f"{name}: values must be in [0, 2^32)")
    return torch.where(t >= (1 << 31), t - (1 << 32), t).to(torch.int32)


def _rankable_array(w):
    """A numpy weight array -> (array of a dtype ghs_weight_ranks_device takes, its GHS_W_* code):
    float32 / float64 / int64 / uint64 as they are, float16 widened to float32, bool and narrower
    integers to int64 (both exact). Anything else (strings, complex, objects): ValueError."""
    import numpy as np
    if w.dtype == np.float32:
        return w, _native.GHS_W_FLOAT32
    if w.dtype == np.float64:
        return w, _native.GHS_W_FLOAT64
    if w.dtype == np.float16:
        return w.astype(np.float32), _native.GHS_W_FLOAT32
    if w.dtype == np.uint64:
        return w.view(np.int64), _native.GHS_W_UINT64  # torch moves it as int64 bits
    if w.dtype.kind in "iub":
        return w.astype(np.int64, copy=False), _native.GHS_W_INT64
    raise ValueError(f"w: rank_weights takes float16 / float32 / float64 or integer weights, got {w.dtype}")


_W_TYPES = {torch.float32: _native.GHS_W_FLOAT32, torch.float64: _native.GHS_W_FLOAT64,
            torch.int64: _native.GHS_W_INT64}
_W_WIDEN = {torch.float16: torch.float32, torch.bfloat16: torch.float32, torch.bool: torch.int64,
            torch.uint8: torch.int64, torch.int8: torch.int64, torch.int16: torch.int64, torch.int32: torch.int64}


def weight_ranks(w, wtype=None):
    """Dense ranks of a weight tensor, on the device (ghs_weight_ranks_device: key pass, rocPRIM
    pairs sort, head-flag scan + scatter): w is a one-dimensional GPU tensor of float32, float64 or
    int64; returns (ranks, distinct) with ranks an int32 tensor of uint32 bit patterns equal to
    np.searchsorted(np.unique(w), w) (-0.0 == +0.0, +-inf ordinary, denormals distinct, float64 never
    narrowed) and distinct the number of distinct values. wtype: the GHS_W_* code when it is not the
    dtype's own — _native.GHS_W_UINT64 for an int64 tensor holding uint64 bit patterns. Runs on
    torch's current stream; a NaN raises GHSError (GHS_E_ARG)."""
    if not (isinstance(w, torch.Tensor) and w.dim() == 1):
        raise ValueError("w: a one-dimensional GPU tensor expected")
    if hasattr(torch, "uint64") and w.dtype == torch.uint64:
        w, wtype = w.view(torch.int64), _native.GHS_W_UINT64
    if w.dtype not in _W_TYPES:
        raise ValueError(f"w: float32, float64 or int64 tensor expected, got {w.dtype}")
    if wtype is None:
        wtype = _W_TYPES[w.dtype]
    elif wtype != _W_TYPES[w.dtype] and not (wtype == _native.GHS_W_UINT64 and w.dtype == torch.int64):
        raise ValueError(f"w: weight type {wtype} does not fit a {w.dtype} tensor")
    L = _native.load()
    _native.require_gpu()
    if not w.is_cuda:
        raise ValueError("w: a one-dimensional GPU tensor expected")
    if w.numel() and w.stride(0) != 1:
        w = w.contiguous()  # a slice stays a view: only its element's own alignment is needed
    m, dev = int(w.numel()), w.device
    if m >= (1 << 32):
        raise ValueError("at most 2^32 - 1 weights")
    with torch.cuda.device(dev):
        ranks = torch.empty(m, dtype=torch.int32, device=dev)
        tb = int(L.ghs_weight_ranks_temp_bytes(wtype, m))
        tmp = torch.empty(max(tb, 16), dtype=torch.uint8, device=dev)
        distinct = ctypes.c_uint64(0)
        _native.check(L.ghs_weight_ranks_device(wtype, m, _ptr(w), _ptr(ranks), ctypes.byref(distinct), _ptr(tmp), tb,
                                                _stream()))
    del tmp
    return ranks, distinct.value


def _canonicalize_ranked(n, u, v, w, wtype=None):
    """canonicalize_device's rank_weights=True path: w (float32 / float64 / int64 GPU tensor; wtype
    as weight_ranks takes it) -> ranks -> the canonicalisation with the raw indices kept -> the
    caller's values gathered into canonical order."""
    for name, t in (("u", u), ("v", v), ("w", w)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 1):
            raise ValueError(f"{name}: a one-dimensional GPU tensor expected (DeviceEdges.from_raw takes numpy arrays)")
    if not (u.numel() == v.numel() == w.numel()):
        raise ValueError("u, v, w must have equal length")
    if not (u.device == v.device == w.device):
        raise ValueError("u, v, w must be on one device")
    if hasattr(torch, "uint64") and w.dtype == torch.uint64:
        w, wtype = w.view(torch.int64), _native.GHS_W_UINT64
    ranks, _ = weight_ranks(w, wtype)
    e = canonicalize_device(n, u, v, ranks, keep_src=True)
    # raw indices below 2^31 index as the int32 they are (no widening pass over src)
    weights = w[e.src if w.numel() <= (1 << 31) else e.src.to(torch.int64) & 0xFFFFFFFF]
    if wtype == _native.GHS_W_UINT64:
        weights = weights.view(torch.uint64)
    e.weights = weights
    return e


def canonicalize_device(n, u, v, w, keep_src=True, rank_weights=False):
    """Raw edges in HBM -> canonical DeviceEdges, without leaving the device
    (ghs_canonicalize_device: key pass, stable pairs sort, last-of-run compaction). u, v, w: torch
    tensors on the GPU, int32 (uint32 bit patterns) or int64 (range-checked, ValueError outside
    [0, 2^32)); any vertex order, either orientation, repeats and self-loops allowed, with
    nx.Graph semantics (self-loops dropped, the LAST weight given for a pair wins). keep_src: the
    result's `src` holds, per canonical edge, the index of the raw edge it came from (`raw_eids`).
    Runs on torch's current stream; a vertex id >= n raises GHSError (GHS_E_ARG).
    rank_weights=True: w may be a float (float16 / bfloat16 widened to float32, float32, float64)
    or any integer tensor holding any values (widened to int64; torch.uint64 accepted): the engine
    weights are their dense ranks (`weight_ranks`: order kept, ties kept, so the same MSF as the
    host path's rank map), keep_src is forced on, and the result's `weights` holds the caller's
    values in canonical order. A NaN raises GHSError (GHS_E_ARG)."""
    n = int(n)
    if n < 0 or n >= (1 << 32):
        raise ValueError("n must be in [0, 2^32)")
    L = _native.load()
    _native.require_gpu()
    if rank_weights:
        if isinstance(w, torch.Tensor) and w.dtype in _W_WIDEN:
            w = w.to(_W_WIDEN[w.dtype])
        return _canonicalize_ranked(n, u, v, w)
    for name, t in (("u", u), ("v", v), ("w", w)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 1):
            raise ValueError(f"{name}: a one-dimensional GPU tensor expected (DeviceEdges.from_raw takes numpy arrays)")
    if not (u.numel() == v.numel() == w.numel()):
        raise ValueError("u, v, w must have equal length")
    if not (u.device == v.device == w.device):
        raise ValueError("u, v, w must be on one device")
    ru, rv, rw = _as_u32_tensor(u, "u"), _as_u32_tensor(v, "v"), _as_u32_tensor(w, "w")
    m_raw, dev = int(ru.numel()), ru.device
    if m_raw >= (1 << 32):
        raise ValueError("at most 2^32 - 1 raw edges")
    with torch.cuda.device(dev):
        cu = torch.empty(m_raw, dtype=torch.int32, device=dev)
        cv = torch.empty(m_raw, dtype=torch.int32, device=dev)
        cw = torch.empty(m_raw, dtype=torch.int32, device=dev)
        src = torch.empty(m_raw, dtype=torch.int32, device=dev) if keep_src else None
        tb = int(L.ghs_canonicalize_temp_bytes(n, m_raw))
        tmp = torch.empty(max(tb, 16), dtype=torch.uint8, device=dev)
        m = ctypes.c_uint64(0)
        _native.check(L.ghs_canonicalize_device(n, m_raw, _ptr(ru), _ptr(rv), _ptr(rw), _ptr(cu), _ptr(cv), _ptr(cw),
                                                _ptr(src), ctypes.byref(m), _ptr(tmp), tb, _stream()))
    del tmp
    mm = m.value
    # views of the first m entries, as generate_rmat returns them
    return DeviceEdges(n, cu[:mm], cv[:mm], cw[:mm], src=src[:mm] if keep_src else None)


def generate_rmat(scale, edgefactor=16, seed=1, wseed=2, device="cuda"):
    """R-MAT (Graph500 A,B,C,D = .57,.19,.19,.05), self-loops dropped, de-duplicated, canonical,
    unique hashed weights — generated and sorted on the GPU."""
    L = _native.load()
    _native.require_gpu()
    T = edgefactor << scale
    dev = torch.device(device)
    u = torch.empty(T, dtype=torch.int32, device=dev)
    v = torch.empty(T, dtype=torch.int32, device=dev)
    w = torch.empty(T, dtype=torch.int32, device=dev)
    tb = L.ghs_rmat_temp_bytes(scale, edgefactor)
    tmp = torch.empty(tb, dtype=torch.uint8, device=dev)
    m = ctypes.c_uint64(0)
    _native.check(L.ghs_rmat_generate(scale, edgefactor, seed, wseed, _ptr(u), _ptr(v), _ptr(w), ctypes.byref(m),
                                      _ptr(tmp), tb, _stream()))
    del tmp
    mm = m.value
    # views of the first m entries (the buffers hold T >= m; at edgefactor 16 m is ~97% of T, so
    # keeping the tail is cheaper than copying 12 B per edge into exact-size tensors)
    return DeviceEdges(1 << scale, u[:mm], v[:mm], w[:mm])


def generate_grid(k, mode=0, wseed=2, device="cuda"):
    """k x k grid graph (right + down edges), canonical; mode 1 = gradient ("road-like") weights."""
    L = _native.load()
    _native.require_gpu()
    dev = torch.device(device)
    m = 2 * k * (k - 1) if k >= 2 else 0
    u = torch.empty(m, dtype=torch.int32, device=dev)
    v = torch.empty(m, dtype=torch.int32, device=dev)
    w = torch.empty(m, dtype=torch.int32, device=dev)
    _native.check(L.ghs_grid_generate(k, mode, wseed, _ptr(u), _ptr(v), _ptr(w), _stream()))
    return DeviceEdges(k * k, u, v, w)


# The ranks' edge ranges are balanced by a cost density over the canonical list instead of by edge
# count: c(x) = 1 + RANGE_BETA * (1 - x) at relative position x = e / m. A canonical edge is stored at
# its smaller end, so the list's early edges have small u and their heavier ends spread over the
# whole vertex range: rank 0's k_filter probes reach all of the giant bitmap (8 MiB at s26, beyond
# one XCD's L2) and the last rank's only its top part — R-MAT s26 x 8 with equal counts ran k_filter
# 1.70 ms on rank 0 against 1.16 on rank 7 (profiles/r05/final/emu_s26_w8_per_rank.txt). The same
# closed form is in csrc/multi.hip (ghs_mst_multi / ghs_mst_emulated). beta = 0.2 measured best over
# {0, 0.2, 0.4} on the s26 x 8 emulation: slowest rank's kernels 6.46 -> 6.08 ms (profiles/r06/).
RANGE_BETA = 0.2


def range_split(m, k, world, beta=None):
    """The first edge of rank k's range: F(x_k) = k / world * F(1) for F(x) = x + beta (x - x^2 / 2),
    4-aligned (the 16-byte vector loads of the level pass stay aligned)."""
    import math
    b = RANGE_BETA if beta is None else float(beta)
    if k <= 0:
        return 0
    if k >= world:
        return m
    if b == 0.0:
        return ((m * k) // world) & ~3
    t = k / world * (1.0 + b / 2.0)
    x = ((1.0 + b) - math.sqrt((1.0 + b) ** 2 - 2.0 * b * t)) / b
    return min(m, int(x * m)) & ~3


def edge_range(m, rank, world, beta=None):
    """Contiguous canonical-edge range owned by `rank` (range_split: cost-balanced, 4-aligned)."""
    lo = range_split(m, rank, world, beta)
    hi = m if rank == world - 1 else range_split(m, rank + 1, world, beta)
    return lo, max(lo, hi)


class DeviceMST:
    """Preallocated single-GPU engine for one DeviceEdges graph (or one rank's edge range).
    csr=None: the CSR entry (ghs_mst_device_csr) whenever the edges carry offsets."""

    def __init__(self, edges, e_lo=0, e_hi=None, config=None, csr=None):
        L = self.L = _native.load()
        _native.require_gpu()
        self.edges = edges
        n, m = edges.n, edges.m
        self.e_lo = int(e_lo)
        self.e_hi = m if e_hi is None else int(e_hi)
        self.config = config if config is not None else _native.make_config()
        dev = edges.device
        self.ws_bytes = int(L.ghs_workspace_bytes(n, m, self.e_hi - self.e_lo))
        self.ws = torch.empty(max(self.ws_bytes, 256), dtype=torch.uint8, device=dev)
        self.in_mst = torch.zeros(max(m, 1), dtype=torch.uint8, device=dev)
        self.csr = (edges.off is not None) if csr is None else bool(csr)
        if self.csr:
            edges.with_csr()

    def run(self):
        """Canonical edges (HBM) -> in_mst flags + totals. Returns (Result, [round stats])."""
        e = self.edges
        res = _native.Result()
        stats = (_native.RoundStats * _native.GHS_MAX_ROUND_STATS)()
        if self.csr:
            _native.check(self.L.ghs_mst_device_csr(e.n, e.m, _ptr(e.off), _ptr(e.u), _ptr(e.v), _ptr(e.w),
                                                    ctypes.byref(self.config), _ptr(self.ws), self.ws_bytes,
                                                    _ptr(self.in_mst), _stream(), ctypes.byref(res), stats))
        else:
            _native.check(self.L.ghs_mst_device(e.n, e.m, _ptr(e.u), _ptr(e.v), _ptr(e.w), ctypes.byref(self.config),
                                                _ptr(self.ws), self.ws_bytes, _ptr(self.in_mst), _stream(),
                                                ctypes.byref(res), stats))
        return res, _native.RoundStatsList(stats, res.num_stats)

    def in_mst_host(self):
        return self.in_mst[: self.edges.m].cpu().numpy().astype(bool)

    def verify(self):
        """`verify_msf` of the engine's own flags (after `run()`)."""
        return verify_msf(self.edges, self.in_mst)

    def labels(self, max_weight=None, num_clusters=None):
        """`forest_labels` of the engine's own flags (after `run()`): with no cut, the connected
        components of the graph."""
        return forest_labels(self.edges, self.in_mst, max_weight=max_weight, num_clusters=num_clusters)

    def rooted(self, order=True):
        """`forest_root` of the engine's own flags (after `run()`): the MSF with every tree rooted at
        its smallest vertex."""
        return forest_root(self.edges, self.in_mst, order=order)

    def dendrogram(self, children=True, sizes=True):
        """`forest_dendrogram` of the engine's own flags (after `run()`): the single-linkage merge
        order of the graph."""
        return forest_dendrogram(self.edges, self.in_mst, children=children, sizes=sizes)

    def clusters(self, min_cluster_size=5, method="eom", allow_single_cluster=False, probabilities=True):
        """HDBSCAN clusters of the engine's own forest (after `run()`): `dendrogram()`, then
        `forest_clusters` with the merge heights in the edge list's own weights."""
        return self.dendrogram().clusters(self.edges, min_cluster_size=min_cluster_size, method=method,
                                          allow_single_cluster=allow_single_cluster, probabilities=probabilities)

    def paths(self):
        """`forest_paths` of the engine's own flags (after `run()`): a PathIndex answering bottleneck
        edge / LCA / hop-count queries on the MSF."""
        return forest_paths(self.edges, self.in_mst)

    def replacements(self, by_edge=True):
        """`forest_replacements` of the engine's own flags (after `run()`): per forest edge the lightest
        edge that takes its place when it fails, the bridges and the best swap. Returns (Replacements,
        info); the index built on the way is released."""
        index, _ = self.paths()
        try:
            return forest_replacements(self.edges, index, by_edge=by_edge)
        finally:
            index.close()

    def distances(self, a, b, hops=False):
        """`forest_distances` on the engine's own flags (after `run()`): how far it is from a[i] to
        b[i] along the MSF, as a uint64 tensor. The index built on the way is released; keep a
        `paths()` index and call `PathIndex.distances` for repeated queries."""
        index, _ = self.paths()
        try:
            return forest_distances(index, a, b, hops=hops)
        finally:
            index.close()

    def edge_distances(self, by_edge=True):
        """`forest_edge_distances` of the graph's own edges over the engine's own flags (after `run()`):
        an EdgeDistances with the per-edge distances, their stretch and the exact sums."""
        index, _ = self.paths()
        try:
            return forest_edge_distances(self.edges, index, by_edge=by_edge)
        finally:
            index.close()

    def diameters(self, ecc=True, hops=False):
        """`forest_diameters` of the engine's own flags (after `run()`): a TreeMetrics with every
        tree's diameter, far ends and eccentricities, and the centre of the widest tree."""
        index, _ = self.paths()
        try:
            return forest_diameters(index, ecc=ecc, hops=hops)
        finally:
            index.close()


def verify_msf(edges, in_mst):
    """Is `in_mst` THE minimum spanning forest of `edges`? Checked on the device, exactly, without a
    second solve (ghs_verify_msf_device: Boruvka over the flagged edges alone, then one walk per edge
    of the graph up the Boruvka tree — csrc/verify.hip, which shares no code with the solver).
    edges: a DeviceEdges with `u` present (a CSR-only list raises ValueError); in_mst: a uint8 / bool
    GPU tensor of at least m flags (nonzero = in the MSF), only read. Returns the fields of
    ghs_verify_result_t as a dict: ok, rounds, overfull, tree_edges, components, total_weight,
    cyclic_edges, unspanned_edges, lighter_edges, first_bad_eid, ms_total. ok is True iff the flags
    equal canonical Kruskal's under the key (w, eid), byte for byte. Runs on torch's current stream; a
    non-canonical list raises GHSError (GHS_E_NONCANON)."""
    if edges.u is None:
        raise ValueError("verify_msf needs the COO form (u present); a CSR-only list is not supported")
    if not isinstance(in_mst, torch.Tensor) or in_mst.dim() != 1:
        raise ValueError("in_mst: a one-dimensional GPU tensor of flags expected")
    if in_mst.dtype == torch.bool:
        in_mst = in_mst.view(torch.uint8)
    if in_mst.dtype != torch.uint8:
        raise ValueError(f"in_mst: uint8 or bool flags expected, got {in_mst.dtype}")
    n, m = edges.n, edges.m
    if in_mst.numel() < m:
        raise ValueError(f"in_mst holds {in_mst.numel()} flags, the edge list {m} edges")
    L = _native.load()
    res = _native.VerifyResult()
    if m == 0:
        _native.check(L.ghs_verify_msf_device(n, 0, None, None, None, None, None, 0, None, ctypes.byref(res)))
        return res.as_dict()
    _native.require_gpu()
    if not in_mst.is_cuda or in_mst.device != edges.device:
        raise ValueError("in_mst must be on the edge list's device")
    if in_mst.stride(0) != 1:
        in_mst = in_mst.contiguous()
    with torch.cuda.device(edges.device):
        ws_bytes = int(L.ghs_verify_workspace_bytes(n, m))
        ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=edges.device)
        _native.check(L.ghs_verify_msf_device(n, m, _ptr(edges.u), _ptr(edges.v), _ptr(edges.w), _ptr(in_mst),
                                              _ptr(ws), ws_bytes, _stream(), ctypes.byref(res)))
    del ws
    return res.as_dict()


def _int_threshold(t, lo, hi):
    """floor(t) clamped to [lo - 1, hi] as a Python int (lo - 1: below every value of the range)."""
    import math
    import numbers
    if not isinstance(t, numbers.Integral):
        t = float(t)
        if math.isnan(t):
            raise ValueError("max_weight must not be NaN")
        if math.isinf(t):
            return hi if t > 0 else lo - 1
        t = math.floor(t)
    return max(lo - 1, min(hi, int(t)))


def _rank_threshold(edges, max_weight):
    """The largest engine weight (rank) among the edges whose own weight is <= max_weight, found on
    the device; None when no edge qualifies. Integer weights are compared as integers (exact at any
    magnitude), float weights as float64 / float32 values."""
    wt = edges.weights
    if wt.numel() == 0:
        return None
    if hasattr(torch, "uint64") and wt.dtype == torch.uint64:
        t = _int_threshold(max_weight, 0, (1 << 64) - 1)
        if t < 0:
            return None
        ok = (wt.view(torch.int64) ^ (-(1 << 63))) <= (t - (1 << 63))  # order of uint64 on int64 bits
    elif not wt.dtype.is_floating_point:
        t = _int_threshold(max_weight, -(1 << 63), (1 << 63) - 1)
        if t < -(1 << 63):
            return None
        ok = wt <= t
    else:
        t = float(max_weight)
        if t != t:
            raise ValueError("max_weight must not be NaN")
        ok = wt.to(torch.float64) <= t
    ranks = edges.w.to(torch.int64) & 0xFFFFFFFF
    best = int(torch.where(ok, ranks, torch.full_like(ranks, -1)).max())
    return None if best < 0 else best


def forest_labels(edges, in_mst, max_weight=None, num_clusters=None):
    """Label every vertex by its component of the flagged forest, on the device
    (ghs_forest_labels_device, csrc/labels.hip): the flagged edges T, optionally cut, then min-root
    hooking and a dense ranking of the roots. No cut: with the engine's flags, the connected
    components of the graph. max_weight=t: only flagged edges with weight <= t are kept — single
    linkage at distance t. num_clusters=k >= 1: the heaviest flagged edges under (w, eid) are dropped
    until k clusters remain (never fewer than the forest has components) — single linkage into k
    clusters. Giving both raises ValueError.
    edges: a DeviceEdges with `u` present (a CSR-only list raises ValueError); in_mst: a uint8 / bool
    GPU tensor of at least m flags (nonzero = in T), only read; it need not be a forest, but more
    than min(m, n - 1) flags raise GHSError (GHS_E_ARG). max_weight is an integer in [0, 2^32) — or,
    when `edges.weights` is set (rank-mapped weights), a value in the caller's own units, mapped on the
    device to the largest rank whose value is <= it (none: every flagged edge is dropped).
    Returns (labels, info): labels an int32 GPU tensor of n entries holding uint32 bit patterns —
    the rank of the vertex's cluster, clusters ordered by their smallest vertex, so vertex 0 has label
    0 and labels are dense in [0, num_clusters); info the fields of ghs_labels_result_t as a dict:
    flagged_edges, kept_edges, dropped_edges, num_clusters, cut_key, rounds, is_forest, ms_total.
    Runs on torch's current stream; a non-canonical list raises GHSError (GHS_E_NONCANON)."""
    if edges.u is None:
        raise ValueError("forest_labels needs the COO form (u present); a CSR-only list is not supported")
    if not isinstance(in_mst, torch.Tensor) or in_mst.dim() != 1:
        raise ValueError("in_mst: a one-dimensional GPU tensor of flags expected")
    if in_mst.dtype == torch.bool:
        in_mst = in_mst.view(torch.uint8)
    if in_mst.dtype != torch.uint8:
        raise ValueError(f"in_mst: uint8 or bool flags expected, got {in_mst.dtype}")
    n, m = edges.n, edges.m
    if in_mst.numel() < m:
        raise ValueError(f"in_mst holds {in_mst.numel()} flags, the edge list {m} edges")
    if max_weight is not None and num_clusters is not None:
        raise ValueError("give max_weight or num_clusters, not both")
    mode, param = _native.GHS_CUT_NONE, 0
    if num_clusters is not None:
        mode, param = _native.GHS_CUT_COUNT, int(num_clusters)
        if param < 1:
            raise ValueError("num_clusters must be >= 1")
        param = min(param, (1 << 64) - 1)
    elif max_weight is not None and edges.weights is None:
        if int(max_weight) != max_weight or not 0 <= int(max_weight) < (1 << 32):
            raise ValueError("max_weight must be an integer in [0, 2^32) (the list carries no rank-mapped weights)")
        mode, param = _native.GHS_CUT_WEIGHT, int(max_weight)
    L = _native.load()
    _native.require_gpu()
    if m and (not in_mst.is_cuda or in_mst.device != edges.device):
        raise ValueError("in_mst must be on the edge list's device")
    if m and in_mst.stride(0) != 1:
        in_mst = in_mst.contiguous()
    drop_all = False
    with torch.cuda.device(edges.device):
        if max_weight is not None and edges.weights is not None:
            thr = _rank_threshold(edges, max_weight)
            if thr is None:
                # below every weight: nothing is kept. A count cut into n clusters drops exactly every
                # flagged edge; it is reported as the weight cut it stands for (no cut key)
                drop_all, mode, param = True, _native.GHS_CUT_COUNT, max(n, 1)
            else:
                mode, param = _native.GHS_CUT_WEIGHT, thr
        res = _native.LabelsResult()
        labels = torch.empty(n, dtype=torch.int32, device=edges.device)
        ws_bytes = int(L.ghs_forest_labels_workspace_bytes(n, m)) if m else 0
        ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=edges.device)
        _native.check(L.ghs_forest_labels_device(n, m, _ptr(edges.u), _ptr(edges.v), _ptr(edges.w),
                                                 _ptr(in_mst) if m else None, mode, param, _ptr(labels), _ptr(ws),
                                                 ws_bytes, _stream(), ctypes.byref(res)))
    del ws
    info = res.as_dict()
    if drop_all:
        info["cut_key"] = (1 << 64) - 1
    return labels, info


class RootedForest:
    """The flagged forest rooted at every tree's smallest vertex (`forest_root`): int32 GPU tensors of
    n entries holding uint32 bit patterns. parent / parent_eid are 0xffffffff (-1 as int32) for a
    root; pre and size are None when the call was made with order=False."""

    def __init__(self, parent, parent_eid, depth, pre, size):
        self.parent, self.parent_eid, self.depth, self.pre, self.size = parent, parent_eid, depth, pre, size

    def is_ancestor(self, a, b):
        """a is an ancestor of b, or b itself: pre[a] <= pre[b] < pre[a] + size[a], elementwise on
        index tensors (or ints) a, b. Returns a bool GPU tensor."""
        if self.pre is None or self.size is None:
            raise ValueError("is_ancestor needs pre and size (forest_root(..., order=True))")
        a = torch.as_tensor(a, device=self.pre.device).long()
        b = torch.as_tensor(b, device=self.pre.device).long()
        pa = self.pre[a].long() & 0xFFFFFFFF
        pb = self.pre[b].long() & 0xFFFFFFFF
        return (pa <= pb) & (pb < pa + (self.size[a].long() & 0xFFFFFFFF))


def forest_root(edges, in_mst, order=True):
    """Root the flagged forest on the device (ghs_forest_root_device, csrc/root.hip): every tree at
    its smallest vertex (the convention of `forest_labels`), by an Euler tour and a splitter list
    ranking, so a path costs what a star costs.
    edges: a DeviceEdges with `u` present (a CSR-only list raises ValueError); in_mst: a uint8 / bool
    GPU tensor of at least m flags (nonzero = in the forest), only read. More than min(m, n - 1) flags
    raise GHSError (GHS_E_ARG); flags that close a cycle are reported as info["is_forest"] = False, and
    the arrays are then unspecified.
    Returns (rooted, info): rooted a RootedForest with .parent (0xffffffff for a root), .parent_eid
    (the canonical id of the edge to the parent), .depth, .pre (a DFS preorder: trees in root order,
    children in ascending id cyclically after the parent) and .size (subtree sizes), so that a is an
    ancestor-or-self of b iff pre[a] <= pre[b] < pre[a] + size[a] (`rooted.is_ancestor`). order=False
    leaves pre and size out (None). info: the fields of ghs_root_result_t as a dict: flagged_edges,
    num_trees, max_depth, rounds, is_forest, ms_total. Runs on torch's current stream; a non-canonical
    list raises GHSError (GHS_E_NONCANON)."""
    if edges.u is None:
        raise ValueError("forest_root needs the COO form (u present); a CSR-only list is not supported")
    if not isinstance(in_mst, torch.Tensor) or in_mst.dim() != 1:
        raise ValueError("in_mst: a one-dimensional GPU tensor of flags expected")
    if in_mst.dtype == torch.bool:
        in_mst = in_mst.view(torch.uint8)
    if in_mst.dtype != torch.uint8:
        raise ValueError(f"in_mst: uint8 or bool flags expected, got {in_mst.dtype}")
    n, m = edges.n, edges.m
    if in_mst.numel() < m:
        raise ValueError(f"in_mst holds {in_mst.numel()} flags, the edge list {m} edges")
    L = _native.load()
    _native.require_gpu()
    if m and (not in_mst.is_cuda or in_mst.device != edges.device):
        raise ValueError("in_mst must be on the edge list's device")
    if m and in_mst.stride(0) != 1:
        in_mst = in_mst.contiguous()
    with torch.cuda.device(edges.device):
        res = _native.RootResult()
        out = [torch.empty(n, dtype=torch.int32, device=edges.device) for _ in range(5 if order else 3)]
        out += [None] * (5 - len(out))
        ws_bytes = int(L.ghs_forest_root_workspace_bytes(n, m)) if m else 0
        ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=edges.device)
        _native.check(L.ghs_forest_root_device(n, m, _ptr(edges.u), _ptr(edges.v), _ptr(in_mst) if m else None,
                                               *[_ptr(t) for t in out], _ptr(ws), ws_bytes, _stream(),
                                               ctypes.byref(res)))
    del ws
    return RootedForest(*out), res.as_dict()


class Dendrogram:
    """The single-linkage dendrogram of a flagged forest (`forest_dendrogram`): int32 GPU tensors
    holding uint32 bit patterns. n vertices, t merges; vertex v is node v, merge j (the j-th lightest
    forest edge under (w, eid)) is node n + j, as in scipy. leaf_parent[n]: the merge that first
    absorbs a vertex (-1: isolated); merge_eid[t]: the canonical edge of a merge; merge_parent[t]: the
    merge that absorbs its cluster next (-1: the last merge of a tree); child_a[t] < child_b[t]: the
    two nodes it joins; size[t]: the vertices of its cluster. child_a / child_b / size are None when
    the call left them out. info: the fields of ghs_dendro_result_t as a dict."""

    def __init__(self, n, leaf_parent, merge_eid, merge_parent, child_a, child_b, size, info=None):
        self.n = int(n)
        self.leaf_parent, self.merge_eid, self.merge_parent = leaf_parent, merge_eid, merge_parent
        self.child_a, self.child_b, self.size, self.info = child_a, child_b, size, info

    @property
    def t(self):
        return int(self.merge_eid.numel())

    def heights(self, edges):
        """The merge heights in the caller's own units, in merge order: edges.weights[merge_eid] (of
        that tensor's dtype) for rank-mapped weights, otherwise the engine's uint32 weights as int64."""
        eid = self.merge_eid.to(torch.int64) & 0xFFFFFFFF
        if edges.weights is not None:
            return edges.weights[eid]
        return edges.w[eid].to(torch.int64) & 0xFFFFFFFF

    def linkage(self, edges):
        """scipy's linkage matrix: a numpy float64 (t, 4) array [child_a, child_b, height, size]. Needs
        the children and the sizes, and a forest that is one tree (t == n - 1): ValueError otherwise."""
        import numpy as np
        if self.child_a is None or self.child_b is None or self.size is None:
            raise ValueError("linkage needs the children and the sizes (forest_dendrogram(children=True, sizes=True))")
        if self.info is not None and not self.info.get("is_forest", True):
            raise ValueError("the flags close a cycle: there is no dendrogram")
        if self.n < 1 or self.t != self.n - 1:
            raise ValueError(f"linkage needs one tree: {self.t} merges on {self.n} vertices")
        Z = np.empty((self.t, 4), np.float64)
        for k, col in enumerate((self.child_a, self.child_b)):
            Z[:, k] = (col.to(torch.int64) & 0xFFFFFFFF).cpu().numpy()
        Z[:, 2] = self.heights(edges).cpu().numpy()
        Z[:, 3] = (self.size.to(torch.int64) & 0xFFFFFFFF).cpu().numpy()
        return Z

    def clusters(self, edges, min_cluster_size=5, method="eom", allow_single_cluster=False, probabilities=True):
        """`forest_clusters` of this dendrogram with the heights taken from `heights(edges)`: the HDBSCAN
        condensed tree, stabilities, selection, labels and probabilities, in the caller's own units."""
        return forest_clusters(self, edges=edges, min_cluster_size=min_cluster_size, method=method,
                               allow_single_cluster=allow_single_cluster, probabilities=probabilities)


def forest_dendrogram(edges, in_mst, children=True, sizes=True):
    """The single-linkage dendrogram (the Kruskal merge tree) of the flagged forest on the device
    (ghs_forest_dendro_device, csrc/dendro.hip), at any depth: nothing walks a path or a chain.
    edges: a DeviceEdges with `u` present (a CSR-only list raises ValueError); in_mst: a uint8 / bool
    GPU tensor of at least m flags (nonzero = in the forest), only read. More than min(m, n - 1) flags
    raise GHSError (GHS_E_ARG); flags that close a cycle are reported as info["is_forest"] = False, and
    the arrays are then unspecified.
    Returns a Dendrogram (tensors trimmed to the t merges found, and .info: flagged_edges, num_trees,
    max_height, levels, rounds, is_forest, ms_total). children=False leaves child_a / child_b out,
    sizes=False leaves size out (None). Runs on torch's current stream; a non-canonical list raises
    GHSError (GHS_E_NONCANON)."""
    if edges.u is None:
        raise ValueError("forest_dendrogram needs the COO form (u present); a CSR-only list is not supported")
    if not isinstance(in_mst, torch.Tensor) or in_mst.dim() != 1:
        raise ValueError("in_mst: a one-dimensional GPU tensor of flags expected")
    if in_mst.dtype == torch.bool:
        in_mst = in_mst.view(torch.uint8)
    if in_mst.dtype != torch.uint8:
        raise ValueError(f"in_mst: uint8 or bool flags expected, got {in_mst.dtype}")
    n, m = edges.n, edges.m
    if in_mst.numel() < m:
        raise ValueError(f"in_mst holds {in_mst.numel()} flags, the edge list {m} edges")
    L = _native.load()
    _native.require_gpu()
    if m and (not in_mst.is_cuda or in_mst.device != edges.device):
        raise ValueError("in_mst must be on the edge list's device")
    if m and in_mst.stride(0) != 1:
        in_mst = in_mst.contiguous()
    cap = min(m, max(n - 1, 0))
    with torch.cuda.device(edges.device):
        res = _native.DendroResult()
        leaf = torch.empty(n, dtype=torch.int32, device=edges.device)
        want = (True, True, children, children, sizes)
        out = [torch.empty(cap, dtype=torch.int32, device=edges.device) if k else None for k in want]
        ws_bytes = int(L.ghs_forest_dendro_workspace_bytes(n, m)) if m else 0
        ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=edges.device)
        _native.check(L.ghs_forest_dendro_device(n, m, _ptr(edges.u), _ptr(edges.v), _ptr(edges.w),
                                                 _ptr(in_mst) if m else None, _ptr(leaf), *[_ptr(t) for t in out],
                                                 _ptr(ws), ws_bytes, _stream(), ctypes.byref(res)))
    del ws
    t = int(res.flagged_edges)
    out = [None if x is None else x[:t] for x in out]
    return Dendrogram(n, leaf, *out, info=res.as_dict())


class Clusters:
    """What `forest_clusters` found (ghs_forest_cluster_device), as GPU tensors. Per vertex (n entries):
    label (int32, -1: noise), probability (float64, None when left out), point_cluster (int32 holding
    uint32 bits, -1: none) and point_lambda (float64). Per cluster, trimmed to the K clusters found:
    cluster_head (the head merge), cluster_parent (-1: a tree top), cluster_size, cluster_birth,
    cluster_stability (float64) and cluster_selected (uint8). Cluster ids run by head merge index
    descending: a parent has a smaller id than its children. info: the fields of ghs_cluster_result_t."""

    def __init__(self, n, label, probability, point_cluster, point_lambda, cluster_head, cluster_parent, cluster_size,
                 cluster_birth, cluster_stability, cluster_selected, info=None):
        self.n = int(n)
        self.label, self.probability = label, probability
        self.point_cluster, self.point_lambda = point_cluster, point_lambda
        self.cluster_head, self.cluster_parent, self.cluster_size = cluster_head, cluster_parent, cluster_size
        self.cluster_birth, self.cluster_stability, self.cluster_selected = cluster_birth, cluster_stability, cluster_selected
        self.info = info

    @property
    def num_clusters(self):
        return int(self.cluster_head.numel())

    def condensed_tree(self):
        """The condensed tree as a numpy structured array of (parent, child, lambda_val, child_size)
        rows: one row per cluster with a parent (child = n + its id, lambda_val = its birth), then one
        per vertex with a cluster (child = the vertex, child_size 1). Parents are n + cluster id."""
        import numpy as np
        dt = np.dtype([("parent", np.int64), ("child", np.int64), ("lambda_val", np.float64), ("child_size", np.int64)])
        cpar = self.cluster_parent.cpu().numpy().astype(np.int64)
        kids = np.nonzero(cpar >= 0)[0]
        pc = self.point_cluster.cpu().numpy().astype(np.int64)
        pts = np.nonzero(pc >= 0)[0]
        rows = np.empty(len(kids) + len(pts), dt)
        k = len(kids)
        rows["parent"][:k] = self.n + cpar[kids]
        rows["child"][:k] = self.n + kids
        rows["lambda_val"][:k] = self.cluster_birth.cpu().numpy()[kids]
        rows["child_size"][:k] = (self.cluster_size.to(torch.int64) & 0xFFFFFFFF).cpu().numpy()[kids]
        rows["parent"][k:] = self.n + pc[pts]
        rows["child"][k:] = pts
        rows["lambda_val"][k:] = self.point_lambda.cpu().numpy()[pts]
        rows["child_size"][k:] = 1
        return rows


def forest_clusters(dendrogram, edges=None, heights=None, min_cluster_size=5, method="eom", allow_single_cluster=False,
                    probabilities=True):
    """HDBSCAN cluster extraction from a `Dendrogram` on the device (ghs_forest_cluster_device,
    csrc/cluster.hip): the condensed tree for min_cluster_size, every cluster's stability, the
    excess-of-mass (method="eom") or leaf (method="leaf") selection, and per vertex a label, noise (-1)
    and a membership probability; scikit-learn's rule for its defaults. The heights, one per merge in
    merge order, are `dendrogram.heights(edges)` (give `edges`) or a tensor / array of t numbers (give
    `heights`), cast to float64: exactly one of the two. They must be finite, > 0 and non-decreasing: a
    zero height (an integer weight 0, duplicate points) raises GHSError (GHS_E_ARG), as does any
    malformed dendrogram. Several trees are treated as joined at infinite distance; a tree with fewer
    than min_cluster_size vertices is noise. ValueError for a dendrogram without children or sizes, for
    one whose flags closed a cycle, and for min_cluster_size < 2. probabilities=False leaves them out.
    Returns a `Clusters`. Runs on torch's current stream."""
    if (edges is None) == (heights is None):
        raise ValueError("forest_clusters needs exactly one of edges= (heights from the dendrogram) and heights=")
    if dendrogram.child_a is None or dendrogram.child_b is None or dendrogram.size is None:
        raise ValueError("forest_clusters needs the children and the sizes (forest_dendrogram(children=True, sizes=True))")
    if dendrogram.info is not None and not dendrogram.info.get("is_forest", True):
        raise ValueError("the flags close a cycle: there is no dendrogram")
    mcs, flags = _native.cluster_args(min_cluster_size, method, allow_single_cluster)
    n, t = dendrogram.n, dendrogram.t
    L = _native.load()
    _native.require_gpu()
    dev = dendrogram.leaf_parent.device
    if heights is None:
        heights = dendrogram.heights(edges)
    if not isinstance(heights, torch.Tensor):
        import numpy as np
        heights = torch.from_numpy(np.ascontiguousarray(np.asarray(heights, dtype=np.float64)))
    h = heights.to(device=dev, dtype=torch.float64).contiguous()
    if h.dim() != 1 or h.numel() != t:
        raise ValueError(f"heights: {t} numbers expected, one per merge")
    cap = int(L.ghs_forest_cluster_capacity(n, t, mcs))
    with torch.cuda.device(dev):
        res = _native.ClusterResult()
        i32 = dict(dtype=torch.int32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        label = torch.empty(n, **i32)
        prob = torch.empty(n, **f64) if probabilities else None
        pc = torch.empty(n, **i32)
        pl = torch.empty(n, **f64)
        c_head, c_par, c_size = (torch.empty(cap, **i32) for _ in range(3))
        c_birth, c_stab = (torch.empty(cap, **f64) for _ in range(2))
        c_sel = torch.empty(cap, dtype=torch.uint8, device=dev)
        ws_bytes = int(L.ghs_forest_cluster_workspace_bytes(n, t, mcs))
        ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
        ins = [t_.contiguous() for t_ in (dendrogram.leaf_parent, dendrogram.merge_parent, dendrogram.child_a,
                                          dendrogram.child_b, dendrogram.size)]
        _native.check(L.ghs_forest_cluster_device(n, t, *[_ptr(x) for x in ins], _ptr(h), mcs, flags, _ptr(label),
                                                  _ptr(prob), _ptr(pc), _ptr(pl), _ptr(c_head), _ptr(c_par),
                                                  _ptr(c_size), _ptr(c_birth), _ptr(c_stab), _ptr(c_sel), _ptr(ws),
                                                  ws_bytes, _stream(), ctypes.byref(res)))
    del ws
    K = int(res.num_clusters)
    return Clusters(n, label, prob, pc, pl, c_head[:K], c_par[:K], c_size[:K], c_birth[:K], c_stab[:K], c_sel[:K],
                    info=res.as_dict())


class MutualReachability:
    """What `mutual_reachability` found. edges: the re-weighted DeviceEdges (the input's u, v, off and
    src, the new w; the input itself after in_place=True). core: per vertex the core distance as the
    engine's uint32 weight (an int32 GPU tensor of uint32 bits; a rank for a rank-mapped list). info: the
    fields of ghs_mreach_result_t as a dict, plus k (what the library was asked for)."""

    def __init__(self, edges, core, info=None, rank_values=None):
        self.edges, self.core, self.info = edges, core, info
        self._rank_values = rank_values  # rank-mapped lists: the caller's value of every rank, as its bits

    def core_values(self):
        """The core distances in the caller's own units: for a rank-mapped list the caller's values of
        the core ranks (of `edges.weights`' dtype; 0 for an isolated vertex), otherwise the uint32
        weights as int64."""
        idx = self.core.to(torch.int64) & 0xFFFFFFFF
        e = self.edges
        if e.weights is None:
            return idx
        if self._rank_values is None or e.m == 0:
            return torch.zeros(e.n, dtype=e.weights.dtype, device=self.core.device)
        vals = self._rank_values[idx].view(e.weights.dtype)
        if self.info is None or self.info.get("isolated", 1):
            touched = torch.zeros(e.n, dtype=torch.bool, device=self.core.device)
            touched[e.u.to(torch.int64) & 0xFFFFFFFF] = True
            touched[e.v.to(torch.int64) & 0xFFFFFFFF] = True
            vals = torch.where(touched, vals, torch.zeros_like(vals))
        return vals


_BITS_OF = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _rank_value_table(ranks, weights):
    """The caller's value of every rank, as an integer tensor of the values' bits: table[r] = the bits
    of weights[e] for any e with ranks[e] == r. Values that share a rank without sharing their bits
    (-0.0 and +0.0) resolve to the larger bit pattern, the same on every run."""
    bits = weights.view(_BITS_OF[weights.element_size()])
    idx = ranks.to(torch.int64) & 0xFFFFFFFF
    size = int(idx.max()) + 1
    table = torch.zeros(size, dtype=bits.dtype, device=bits.device)
    return table.scatter_reduce_(0, idx, bits, "amax", include_self=False)


def mutual_reachability(edges, min_samples=5, short_rows="error", include_self=False, in_place=False):
    """Core distances and mutual-reachability weights of a canonical edge list on the device
    (ghs_mutual_reach_device, csrc/mreach.hip): the weights HDBSCAN wants. core[x] is the min_samples-th
    smallest weight among the edges at x (repeated weights count separately), and every edge gets
    max(core[u], core[v], w). Exact, the same bytes on every run, and only w changes: the result is
    canonical with the same edge ids, offsets and `src`, so the solver and every forest module take it
    as it is.
    edges: a DeviceEdges with `u` present (a CSR-only list raises ValueError). min_samples >= 1, any
    size. short_rows: what to do with a vertex that has edges but fewer than min_samples of them:
    "error" raises ValueError naming their number; "clamp" takes the largest weight at that vertex (k
    clamped to the degree). An isolated vertex has core 0 and is no error: it ends up as noise. The
    policy "infinite core distance, drop the vertex's edges" would change the edge ids and is not
    offered. include_self=True: the dense scikit-learn convention, where a point is its own first
    neighbour: k = min_samples - 1, and for min_samples == 1 the weights come back unchanged with every
    core 0, without a library call. in_place=True overwrites the input's w (and weights) instead of
    allocating new ones.
    For a rank-mapped list (`edges.weights` set) the new `weights` are the caller's values of the new
    ranks, looked up in a rank -> value table scattered from (w, weights) in torch, and
    `MutualReachability.core_values()` gives the core distances in the caller's units.
    Returns a `MutualReachability` (edges, core, info). Runs on torch's current stream; a non-canonical
    list raises GHSError (GHS_E_NONCANON)."""
    k = _native.mreach_args(min_samples, short_rows, include_self)
    if edges.u is None:
        raise ValueError("mutual_reachability needs the COO form (u present); a CSR-only list is not supported")
    n, m = edges.n, edges.m
    L = _native.load()
    _native.require_gpu()
    dev = edges.device
    ranked = edges.weights is not None and m > 0
    with torch.cuda.device(dev):
        core = torch.empty(n, dtype=torch.int32, device=dev)
        res = _native.MreachResult()
        if k == 0:
            core.zero_()
            w_out = edges.w if in_place else edges.w.clone()
        else:
            w_in = edges.w if edges.w.stride(0) == 1 or m == 0 else edges.w.contiguous()
            w_out = w_in if in_place and w_in is edges.w else torch.empty(m, dtype=torch.int32, device=dev)
            table = _rank_value_table(w_in, edges.weights) if ranked else None
            ws_bytes = int(L.ghs_mutual_reach_workspace_bytes(n, m))
            ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
            _native.check(L.ghs_mutual_reach_device(n, m, _ptr(edges.u), _ptr(edges.v), _ptr(w_in), k, _ptr(core),
                                                    _ptr(w_out), _ptr(ws), ws_bytes, _stream(), ctypes.byref(res)))
            del ws
    info = res.as_dict()
    info["k"] = k
    if k == 0:
        out = edges if in_place else DeviceEdges(n, edges.u, edges.v, w_out, edges.off, edges.src,
                                                 None if edges.weights is None else edges.weights.clone())
        return MutualReachability(out, core, info)
    if info["short_rows"] and short_rows == "error":
        raise ValueError(f"{info['short_rows']} vertices have edges but fewer than min_samples = {min_samples}"
                         f"{' (the point itself included)' if include_self else ''} of them; give every vertex at "
                         "least that many neighbours, or pass short_rows='clamp' to use each one's largest weight")
    weights = edges.weights
    if ranked:
        weights = table[w_out.to(torch.int64) & 0xFFFFFFFF].view(edges.weights.dtype)
    if in_place:
        if w_out is not edges.w:
            edges.w.copy_(w_out)
        if ranked:
            edges.weights.copy_(weights)
        out = edges
    else:
        out = DeviceEdges(n, edges.u, edges.v, w_out, edges.off, edges.src, weights)
    return MutualReachability(out, core, info, rank_values=table if ranked else None)


class HDBSCANResult:
    """What `hdbscan` ran: reach (the MutualReachability), mst (the DeviceMST after run(), over
    reach.edges), dendrogram, clusters (a Clusters) and labels (clusters.label: int32, -1 noise)."""

    def __init__(self, reach, mst, dendrogram, clusters):
        self.reach, self.mst, self.dendrogram, self.clusters = reach, mst, dendrogram, clusters

    @property
    def labels(self):
        return self.clusters.label


def hdbscan(edges, min_cluster_size=5, min_samples=None, method="eom", allow_single_cluster=False, short_rows="error",
            include_self=False):
    """HDBSCAN of a canonical edge list (a k-NN graph, a sparse distance matrix) end to end on the
    device: `mutual_reachability` -> `DeviceMST(...).run()` -> `dendrogram()` -> `clusters()`.
    min_samples=None means min_cluster_size; short_rows and include_self as `mutual_reachability` takes
    them, method and allow_single_cluster as `forest_clusters` does. The input list is left as it is.
    Returns an `HDBSCANResult` (reach, mst, dendrogram, clusters, labels). The binary merge order inside
    a level of equal mutual-reachability weights is the engine's own ((w, eid)), as it is every
    implementation's own: labels may differ from another HDBSCAN's where ties decide."""
    _native.cluster_args(min_cluster_size, method, allow_single_cluster)
    reach = mutual_reachability(edges, min_samples=min_cluster_size if min_samples is None else min_samples,
                                short_rows=short_rows, include_self=include_self)
    mst = DeviceMST(reach.edges)
    mst.run()
    dg = mst.dendrogram()
    cl = dg.clusters(reach.edges, min_cluster_size=min_cluster_size, method=method,
                     allow_single_cluster=allow_single_cluster)
    return HDBSCANResult(reach, mst, dg, cl)


class KNN:
    """What `knn` found. idx: (n, k) int32 GPU tensor of uint32 bits, row i the neighbours of point i in
    ascending (distance, index) order; dist: (n, k) float32, their distances (squared for
    metric="sqeuclidean"); info: the fields of ghs_knn_result_t as a dict, plus k and metric."""

    def __init__(self, idx, dist, info=None):
        self.idx, self.dist, self.info = idx, dist, info


class KNNGraph:
    """What `knn_graph` built. edges: the canonical DeviceEdges of the symmetrised k-NN graph (`w` the
    ranks of the distances, `weights` the float32 distances, `src` the index into the flattened (n, k)
    table); knn: the KNN it came from."""

    def __init__(self, edges, knn):
        self.edges, self.knn = edges, knn


_INT_POINT_TYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)


def _points_f32(points):
    """points as a contiguous float32 GPU matrix: float32 as it is, float16 / bfloat16 widened (exact),
    integers when every |x| < 2^24 (exact; checked on the device). ValueError for anything else; float64
    is never narrowed silently. Everything that needs no device comes first."""
    if not (isinstance(points, torch.Tensor) and points.dim() == 2):
        raise ValueError("points: a two-dimensional (n, d) GPU tensor expected")
    if points.dtype == torch.float64:
        raise ValueError("points: float64 is never narrowed silently; cast with points.to(torch.float32) "
                         "if float32 distances are what you want")
    if points.dtype not in (torch.float32, torch.float16, torch.bfloat16) + _INT_POINT_TYPES:
        raise ValueError(f"points: float32 / float16 / bfloat16 or an integer tensor expected, got {points.dtype}")
    return points


def knn(points, k, metric="euclidean", slices=0):
    """The exact k nearest neighbours of every row of `points`, by brute force on the device
    (ghs_knn_device, csrc/knn.hip). points: a 2-D GPU tensor (n, d), d <= 4096; float32 is used as it is
    (made contiguous if needed), float16 / bfloat16 are widened to float32 and integer dtypes converted
    when every |x| < 2^24 (both exact; ValueError otherwise); float64 raises ValueError: cast it yourself.
    1 <= k <= min(128, n - 1). metric: "euclidean" or "sqeuclidean".
    Exact means: the squared distance is the float32 chain s = a[t] - b[t], acc = fmaf(s, s, acc) over
    t ascending (relative error at most (d + 3) * 2^-23, symmetric bit for bit, 0 for equal rows), the
    neighbours of i are the k points j != i with the smallest (that value, j), ties to the smaller index,
    and "euclidean" is its correctly rounded square root. A duplicate of a point is its neighbour at
    distance 0 (info["zero_neighbours"] counts such entries). The same bytes on every call and for every
    `slices` (0: chosen from n; a tuning knob only). Runs on torch's current stream; a NaN or infinite
    coordinate raises GHSError (GHS_E_ARG). Returns a `KNN` (idx, dist, info)."""
    points = _points_f32(points)
    n, dim = int(points.shape[0]), int(points.shape[1])
    kk, mcode, ss = _native.knn_args(k, metric, slices, n=n, dim=dim)
    L = _native.load()
    _native.require_gpu()
    if not points.is_cuda:
        raise ValueError("points: a two-dimensional (n, d) GPU tensor expected")
    dev = points.device
    with torch.cuda.device(dev):
        if points.dtype in (torch.int32, torch.int64) and points.numel():  # the narrower ones cannot reach 2^24
            if bool(((points >= (1 << 24)) | (points <= -(1 << 24))).any()):
                raise ValueError("points: integer coordinates must satisfy |x| < 2^24 to be exact in float32")
        x = points.to(torch.float32).contiguous()
        if x.data_ptr() % 16:
            x = x.clone()  # a view that starts off a 16-byte boundary
        idx = torch.empty((n, kk), dtype=torch.int32, device=dev)
        dist = torch.empty((n, kk), dtype=torch.float32, device=dev)
        res = _native.KnnResult()
        ws_bytes = int(L.ghs_knn_workspace_bytes(n, dim, kk, ss))
        ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
        _native.check(L.ghs_knn_device(n, dim, _ptr(x), kk, mcode, ss, _ptr(idx), _ptr(dist), _ptr(ws), ws_bytes, _stream(),
                                       ctypes.byref(res)))
        del ws
    info = res.as_dict()
    info["k"], info["metric"] = kk, metric
    return KNN(idx, dist, info)


def knn_graph(points, k, metric="euclidean"):
    """The symmetrised k-NN graph of `points` as a canonical edge list, without leaving the device: `knn`,
    then the raw edges (i, idx[i, j], dist[i, j]) through `canonicalize_device(..., rank_weights=True)`.
    edges.w holds the ranks of the distances, edges.weights the float32 distances and edges.src the index
    into the flattened (n, k) table; n * k / 2 <= m <= n * k. Every vertex has degree >= k. Returns a
    `KNNGraph` (edges, knn)."""
    nn = knn(points, k, metric=metric)
    n, kk = int(nn.idx.shape[0]), int(nn.idx.shape[1])
    dev = nn.idx.device
    with torch.cuda.device(dev):
        # the row ids are plumbing: no kernel of ours
        ru = torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(kk)
        # A pair that both ends chose appears twice, as (i, j) and as (j, i). The ingest keeps the last
        # occurrence; the squared distance is symmetric bit for bit (and so is its square root), so both
        # occurrences carry the same weight and which one wins cannot matter.
        edges = canonicalize_device(n, ru, nn.idx.reshape(-1), nn.dist.reshape(-1), rank_weights=True)
    return KNNGraph(edges, nn)


class EMST:
    """What `emst` found: the n - 1 edges of the exact minimum spanning tree of the complete graph on the
    points, a canonical edge list. u, v: int32 GPU tensors of uint32 bits, u[e] < v[e], (u, v) strictly
    ascending; w: float32, the weights (squared for metric="sqeuclidean"); info: the fields of
    ghs_emst_result_t as a dict, plus n and metric."""

    def __init__(self, n, u, v, w, info=None):
        self.n, self.u, self.v, self.w, self.info = int(n), u, v, w, info
        self._edges = None

    def edges(self):
        """The tree as `DeviceEdges` (through `canonicalize_device(..., rank_weights=True)`): `w` the ranks
        of the weights, `weights` the float32 weights. The list is canonical already, so `src` is the
        identity."""
        if self._edges is None:
            self._edges = canonicalize_device(self.n, self.u, self.v, self.w, rank_weights=True)
        return self._edges


def emst(points, core2=None, metric="euclidean", slices=0):
    """The exact minimum spanning tree of the complete graph on the rows of `points`, on the device
    (ghs_emst_device, csrc/emst.hip): the Euclidean MST, or with `core2` (n float32 SQUARED core distances,
    finite and >= 0, on the points' device) the mutual-reachability MST HDBSCAN is defined on. points: as
    `knn` takes them (float32 as it is, float16 / bfloat16 / small integers widened exactly, float64
    refused). The weight of {i, j} is max(d2(i, j), core2[i], core2[j]) with d2 the float32 chain of `knn`;
    pairs are ordered by (weight bits, min, max), so the tree is unique: canonical Kruskal's over all
    n (n - 1) / 2 pairs. The same bytes on every call and for every `slices` (0: chosen from n; a tuning
    knob only). Boruvka rounds, each one brute-force sweep: O(n^2 d log n) work, no k. Runs on torch's
    current stream; a NaN or infinite coordinate, or a core2 that is NaN, infinite or negative, raises
    GHSError (GHS_E_ARG). Returns an `EMST` (u, v, w, info, edges())."""
    points = _points_f32(points)
    n, dim = int(points.shape[0]), int(points.shape[1])
    mcode, ss = _native.emst_args(metric, slices, n=n, dim=dim)
    if core2 is not None:
        if not (isinstance(core2, torch.Tensor) and core2.dim() == 1 and core2.dtype == torch.float32):
            raise ValueError("core2: a one-dimensional float32 GPU tensor of squared core distances expected")
        if int(core2.numel()) != n:
            raise ValueError(f"core2: {n} entries expected (one per point), got {int(core2.numel())}")
    L = _native.load()
    _native.require_gpu()
    if not points.is_cuda:
        raise ValueError("points: a two-dimensional (n, d) GPU tensor expected")
    if core2 is not None and core2.device != points.device:
        raise ValueError("core2 must be on the points' device")
    dev = points.device
    t = max(n - 1, 0)
    with torch.cuda.device(dev):
        if points.dtype in (torch.int32, torch.int64) and points.numel():  # the narrower ones cannot reach 2^24
            if bool(((points >= (1 << 24)) | (points <= -(1 << 24))).any()):
                raise ValueError("points: integer coordinates must satisfy |x| < 2^24 to be exact in float32")
        x = points.to(torch.float32).contiguous()
        if x.data_ptr() % 16:
            x = x.clone()  # a view that starts off a 16-byte boundary
        c2 = core2.contiguous() if core2 is not None else None
        u = torch.empty(t, dtype=torch.int32, device=dev)
        v = torch.empty(t, dtype=torch.int32, device=dev)
        w = torch.empty(t, dtype=torch.float32, device=dev)
        res = _native.EmstResult()
        ws_bytes = int(L.ghs_emst_workspace_bytes(n, dim, ss))
        ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
        _native.check(L.ghs_emst_device(n, dim, _ptr(x), _ptr(c2) if c2 is not None else None, mcode, ss, _ptr(u), _ptr(v),
                                        _ptr(w), _ptr(ws), ws_bytes, _stream(), ctypes.byref(res)))
        del ws
    info = res.as_dict()
    info["n"], info["metric"] = n, metric
    return EMST(n, u, v, w, info)


def _rounded_sqrt(t):
    """the correctly rounded float32 square root of a small GPU vector, as the kernels' sqrtf gives it (numpy's is
    IEEE's; n values through the host, next to n^2 work on the device)"""
    import numpy as np
    return torch.from_numpy(np.sqrt(t.cpu().numpy())).to(t.device)


def _hdbscan_points_exact(points, min_cluster_size, ms, metric, method, allow_single_cluster):
    """hdbscan_points(exact=True): the cores from the k-NN table, the exact mutual-reachability MST, then
    the dendrogram and the clusters of that tree."""
    n = int(points.shape[0])
    if n < 2:
        raise ValueError(f"exact=True needs at least 2 points, got n = {n}")
    _native.emst_args(metric, 0, n=n, dim=int(points.shape[1]))
    if ms >= 2:
        nn = knn(points, ms - 1, metric="sqeuclidean")   # include_self=True: the point is its own first neighbour
        core2 = nn.dist[:, ms - 2].contiguous()
    else:
        core2 = torch.zeros(n, dtype=torch.float32, device=points.device)
    tree = emst(points, core2=core2, metric=metric)
    edges = tree.edges()
    mst = DeviceMST(edges)
    res, _ = mst.run()
    flagged = int(mst.in_mst[: edges.m].sum()) if edges.m else 0
    if edges.m != n - 1 or res.num_mst_edges != n - 1 or flagged != n - 1:
        raise _native.GHSError(_native.GHS_E_STATE, f"the exact MST's {edges.m} edges are no spanning tree of {n} points: "
                               f"the solve flagged {flagged}")
    dg = mst.dendrogram()
    try:
        cl = dg.clusters(edges, min_cluster_size=min_cluster_size, method=method, allow_single_cluster=allow_single_cluster)
    except _native.GHSError as e:
        zeros = tree.info["zero_edges"]
        if e.code == _native.GHS_E_ARG and zeros:
            raise _native.GHSError(e.code, f"{str(e).split(': ', 1)[-1]}; the exact MST holds {zeros} edges of weight zero "
                                   "(info['zero_edges']): duplicate points make zero heights, which forest_clusters refuses") from e
        raise
    out = HDBSCANResult(None, mst, dg, cl)
    out.emst = tree
    out.core = _rounded_sqrt(core2) if metric == "euclidean" else core2
    return out


def hdbscan_points(points, min_cluster_size=5, min_samples=None, k=None, metric="euclidean", method="eom",
                   allow_single_cluster=False, exact=False):
    """HDBSCAN of points end to end on the device: `knn_graph(points, k)` -> `hdbscan(edges, ...,
    include_self=True, short_rows="error")`. include_self=True is scikit-learn's convention for points (a
    point is its own first neighbour), min_samples=None means min_cluster_size, k=None means
    max(1, min_samples). k < max(1, min_samples - 1) or k > n - 1 raises ValueError.
    What is exact: the core distances. Row x of the symmetrised graph holds x's own k nearest plus the
    points that chose x; a point that chose x without being among x's k nearest is no nearer than x's
    k-th; so the (min_samples - 1)-th smallest of the row is the true one whenever k >= min_samples - 1:
    the cores equal those of the dense definition.
    What is not exact: the forest. It is the minimum spanning forest of the k-NN graph under the
    mutual-reachability weights. It equals the MST of the complete mutual-reachability graph exactly when
    that MST uses edges of the k-NN graph only, which is certain at k = n - 1 and likely for k well above
    min_samples; otherwise the forest has several trees, joined at infinite distance as `forest_clusters`
    documents.
    Duplicate points give zero distances; a zero mutual-reachability forest edge is `forest_clusters`'
    error (zero is no valid height), here re-raised with the number of zero entries in the k-NN table
    (info["zero_neighbours"]). Returns the `HDBSCANResult` of `hdbscan` with one more attribute, `knn`
    (the KNNGraph).
    exact=True takes the exact path instead, and the forest is exact too: the cores come from
    `knn(points, max(1, min_samples - 1), metric="sqeuclidean")` (column min_samples - 2; zero for
    min_samples == 1: the same include_self=True convention), then `emst(points, core2=...)` gives THE minimum
    spanning tree of the complete mutual-reachability graph, `DeviceMST(tree.edges()).run()` flags every
    edge of it (anything else raises), then `dendrogram()` and `clusters()`. `k` is ignored: nothing depends
    on it. The result has reach=None and two more attributes: `emst` (the EMST) and `core` (float32, in the
    metric's units). A zero-weight tree edge is `forest_clusters`' error, re-raised with the tree's number of
    zero edges (info["zero_edges"]). Cost: O(n^2 d log n) instead of O(n^2 d)."""
    _native.cluster_args(min_cluster_size, method, allow_single_cluster)
    ms = _native.mreach_args(min_cluster_size if min_samples is None else min_samples, "error")
    _points_f32(points)
    n = int(points.shape[0])
    if exact:
        if metric not in _native.KNN_METRICS:
            raise ValueError(f"metric: 'euclidean' or 'sqeuclidean' expected, got {metric!r}")
        return _hdbscan_points_exact(points, min_cluster_size, ms, metric, method, allow_single_cluster)
    kk = max(1, ms) if k is None else k
    kk, _, _ = _native.knn_args(kk, metric, 0)
    if kk < max(1, ms - 1):
        raise ValueError(f"k = {kk} is below min_samples - 1 = {ms - 1}: the core distances would not be exact")
    if kk > n - 1:
        raise ValueError(f"k = {kk} needs at least k + 1 points, got n = {n}"
                         + (" (pass a smaller k or min_samples)" if k is None else ""))
    g = knn_graph(points, kk, metric=metric)
    try:
        out = hdbscan(g.edges, min_cluster_size=min_cluster_size, min_samples=ms, method=method,
                      allow_single_cluster=allow_single_cluster, short_rows="error", include_self=True)
    except _native.GHSError as e:
        zeros = g.knn.info["zero_neighbours"]
        if e.code == _native.GHS_E_ARG and zeros:
            raise _native.GHSError(e.code, f"{str(e).split(': ', 1)[-1]}; the k-NN table holds {zeros} zero distances (info['zero_neighbours']): "
                                   "duplicate points make zero heights, which forest_clusters refuses") from e
        raise
    out.knn = g
    return out


class PathAnswers:
    """What `PathIndex.query` returns, one entry per pair, on the device.
    key: int64 holding the uint64 w << 32 | eid of the heaviest edge (largest key) on the forest path;
    all ones (-1) when a == b or the ends are in different trees. eid / w: its two halves as int32
    holding uint32 bit patterns (-1 where there is no edge). lca, hops: int32 holding uint32; -1 where
    the ends are in different trees (lca = a and hops = 0 when a == b). A field left out of the query
    is None. info: the fields of ghs_paths_query_result_t as a dict (queries, connected, ms_total)."""

    def __init__(self, key, lca, hops, info=None):
        self.key, self.lca, self.hops, self.info = key, lca, hops, info

    def _need(self, name):
        t = getattr(self, name)
        if t is None:
            raise ValueError(f"the query was made without {name}")
        return t

    @property
    def eid(self):
        return self._need("key").view(torch.int32).view(-1, 2)[:, 0]

    @property
    def w(self):
        return self._need("key").view(torch.int32).view(-1, 2)[:, 1]

    @property
    def has_edge(self):
        """bool: the path has an edge (the ends are distinct and in one tree)."""
        return self._need("key") != -1

    @property
    def connected(self):
        """bool: the ends are in one tree (a == b included)."""
        return self._need("lca") != -1

    def weights(self, edges):
        """The bottleneck weights in the caller's own units: (values, has_edge). With rank-mapped
        weights (`edges.weights` set) values = edges.weights[eid], of that tensor's dtype; otherwise the
        engine's uint32 weights as int64. Where has_edge is False the value is NaN for float weights
        and 0 for integer ones."""
        mask = self.has_edge
        eid = torch.where(mask, self.eid.to(torch.int64) & 0xFFFFFFFF, torch.zeros_like(self.key))
        if edges.weights is None:
            vals = self.w.to(torch.int64) & 0xFFFFFFFF
            return torch.where(mask, vals, torch.zeros_like(vals)), mask
        wt = edges.weights
        if wt.numel() == 0:
            return torch.zeros(eid.numel(), dtype=wt.dtype, device=eid.device), mask
        vals = wt[eid]
        none = float("nan") if wt.dtype.is_floating_point else 0
        return torch.where(mask, vals, torch.full_like(vals, none)), mask


class PathIndex:
    """The jump-pointer index of a rooted forest (`forest_paths`; ghs_forest_paths_create). Keeps the
    index tensor alive; `close()` (or deletion) destroys the native handle. One query at a time per
    index: the calls' status block lives in the index."""

    def __init__(self, handle, index, n, device, ranked=False):
        self._h, self._index, self.n, self.device = handle, index, int(n), device
        # the index was built over rank-mapped weights (edges.weights set): its keys hold ranks
        self.ranked = bool(ranked)
        self._wdepth = {}
        self.last_distance_info = None

    def query(self, a, b, key=True, lca=True, hops=True):
        """a, b: int32 (uint32 bit patterns) or int64 GPU tensors of equal length, or ints. Returns a
        PathAnswers; key / lca / hops = False leaves that output out. An id >= n raises GHSError
        (GHS_E_ARG), a value outside [0, 2^32) ValueError. Runs on torch's current stream."""
        if not self._h:
            raise ValueError("the index is closed")
        ta = torch.as_tensor(a, device=self.device).reshape(-1) if not isinstance(a, torch.Tensor) else a
        tb = torch.as_tensor(b, device=self.device).reshape(-1) if not isinstance(b, torch.Tensor) else b
        for name, t in (("a", ta), ("b", tb)):
            if t.dim() != 1 or t.device != self.device:
                raise ValueError(f"{name}: a one-dimensional tensor on the index's device (or an int) expected")
        if ta.numel() != tb.numel():
            raise ValueError("a and b must have equal length")
        ta, tb = _as_u32_tensor(ta, "a"), _as_u32_tensor(tb, "b")
        q = int(ta.numel())
        if q >= (1 << 32):
            raise ValueError("at most 2^32 - 1 pairs")
        with torch.cuda.device(self.device):
            okey = torch.empty(q, dtype=torch.int64, device=self.device) if key else None
            olca = torch.empty(q, dtype=torch.int32, device=self.device) if lca else None
            ohops = torch.empty(q, dtype=torch.int32, device=self.device) if hops else None
            res = _native.PathsQueryResult()
            _native.check(_native.load().ghs_forest_paths_query(self._h, q, _ptr(ta), _ptr(tb), _ptr(okey), _ptr(olca),
                                                                _ptr(ohops), _stream(), ctypes.byref(res)))
        return PathAnswers(okey, olca, ohops, res.as_dict())

    def replacements(self, edges, by_edge=True):
        """`forest_replacements(edges, self)`: the edge list must be the one this index was built over."""
        return forest_replacements(edges, self, by_edge=by_edge)

    def _metric(self, hops):
        if not hops and self.ranked:
            raise ValueError("the index was built over rank-mapped weights (edges.weights is set): a sum of ranks "
                             "means nothing; use hops=True for distances in edges")
        return _native.GHS_DIST_HOPS if hops else _native.GHS_DIST_WEIGHT

    def wdepth(self, hops=False):
        """Every vertex's distance to its tree's root (ghs_forest_wdepth_device, csrc/dist.hip): a uint64
        GPU tensor of n entries, the sum of the weights on the path (hops=True: the number of edges),
        0 for a root. Built on the first call by pointer doubling over the index's levels and cached on
        the index, one array per metric. Rank-mapped weights raise ValueError unless hops=True."""
        if not self._h:
            raise ValueError("the index is closed")
        metric = self._metric(hops)
        if metric not in self._wdepth:
            L = _native.load()
            pi = _native.PathsInfo()
            _native.check(L.ghs_forest_paths_info(self._h, ctypes.byref(pi)))
            _native.require_gpu()
            with torch.cuda.device(self.device):
                wb = int(L.ghs_forest_dist_workspace_bytes(self.n, pi.max_depth))
                wd = torch.empty(self.n, dtype=torch.int64, device=self.device)
                ws = torch.empty(wb, dtype=torch.uint8, device=self.device)
                _native.check(L.ghs_forest_wdepth_device(self._h, metric, _ptr(wd), _ptr(ws), wb, _stream()))
            del ws
            self._wdepth[metric] = wd.view(torch.uint64)
        return self._wdepth[metric]

    def distances(self, a, b, hops=False, lca=False):
        """`forest_distances(self, a, b)`: the distance between a[i] and b[i] along the forest."""
        return forest_distances(self, a, b, hops=hops, lca=lca)

    def edge_distances(self, edges, by_edge=True):
        """`forest_edge_distances(edges, self)`: the edge list must be the one this index was built over."""
        return forest_edge_distances(edges, self, by_edge=by_edge)

    def diameters(self, ecc=True, hops=False):
        """`forest_diameters(self)`: diameter, far ends and eccentricities of every tree."""
        return forest_diameters(self, ecc=ecc, hops=hops)

    def close(self):
        if self._h:
            _native.load().ghs_forest_paths_destroy(self._h)
            self._h = None
        self._index = None
        self._wdepth = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def forest_paths(edges, in_mst=None, rooted=None, max_depth=None):
    """Index the flagged forest for path queries, on the device (ghs_forest_paths_create,
    csrc/paths.hip): jump pointers over parent / parent_eid / depth, K = max(1, bit_length(max_depth))
    levels of n 16-byte nodes. `PathIndex.query(a, b)` then gives, per pair, the heaviest edge of the
    forest path (with the engine's MSF: the minimax distance in the graph, the edge a new edge (a, b)
    would displace, the single-linkage merge height), the lowest common ancestor and the hop count.
    Give the flags (in_mst: a uint8 / bool GPU tensor of at least m flags, only read; rooted here with
    `forest_root(order=False)`; flags that close a cycle raise ValueError) or a RootedForest together
    with its max_depth (an upper bound of the depths: info["max_depth"] of `forest_root`). The arrays
    are validated on the device; anything that is not a rooted forest of this edge list raises
    GHSError (GHS_E_ARG). edges: a DeviceEdges with `u` present.
    Returns (index, info): info the fields of ghs_paths_result_t as a dict: levels, max_depth,
    num_trees, index_bytes, ms_total. Runs on torch's current stream."""
    if edges.u is None:
        raise ValueError("forest_paths needs the COO form (u present); a CSR-only list is not supported")
    if (in_mst is None) == (rooted is None):
        raise ValueError("give in_mst or rooted (with max_depth), not both and not neither")
    if rooted is not None and max_depth is None:
        raise ValueError("a RootedForest needs its max_depth (info['max_depth'] of forest_root)")
    n, m = edges.n, edges.m
    if rooted is None:
        rooted, rinfo = forest_root(edges, in_mst, order=False)
        if not rinfo["is_forest"]:
            raise ValueError("in_mst is not a forest (the flags close a cycle)")
        max_depth = rinfo["max_depth"]
    max_depth = int(max_depth)
    if max_depth < 0:
        raise ValueError("max_depth must be >= 0")
    for name in ("parent", "parent_eid", "depth"):
        t = getattr(rooted, name)
        if not (isinstance(t, torch.Tensor) and t.dim() == 1 and t.dtype == torch.int32 and t.numel() >= n):
            raise ValueError(f"rooted.{name}: an int32 tensor of n entries expected")
    L = _native.load()
    _native.require_gpu()
    dev = edges.device
    par, peid, dep = (getattr(rooted, k).contiguous() for k in ("parent", "parent_eid", "depth"))
    if n and not all(t.is_cuda and t.device == dev for t in (par, peid, dep)):
        raise ValueError("the rooted arrays must be on the edge list's device")
    with torch.cuda.device(dev):
        ib = int(L.ghs_forest_paths_index_bytes(n, max_depth))
        index = torch.empty(max(ib, 256), dtype=torch.uint8, device=dev)
        res = _native.PathsResult()
        h = ctypes.c_void_p(0)
        _native.check(L.ghs_forest_paths_create(n, m, _ptr(edges.u), _ptr(edges.v), _ptr(edges.w), _ptr(par), _ptr(peid),
                                                _ptr(dep), max_depth, _ptr(index), ib, _stream(), ctypes.byref(res),
                                                ctypes.byref(h)))
    return PathIndex(h, index, n, dev, ranked=edges.weights is not None), res.as_dict()


class Replacements:
    """What `forest_replacements` returns, on the device. Every non-root vertex x stands for its parent
    edge (x, parent[x]).
    key: int64[n] holding the uint64 w << 32 | eid of the lightest non-forest edge that reconnects the
    two halves when x's edge fails; all ones (-1) for a root and for a bridge. eid / w: its two halves as
    int32 holding uint32 bit patterns. has_replacement: bool[n]. eid_by_edge: int32[m] (uint32 bits), for
    a forest edge the replacement's eid, -1 for a bridge and for every non-forest edge; None when left
    out. info: the fields of ghs_replace_result_t as a dict."""

    def __init__(self, key, eid_by_edge, info=None):
        self.key, self.eid_by_edge, self.info = key, eid_by_edge, info

    @property
    def eid(self):
        return self.key.view(torch.int32).view(-1, 2)[:, 0]

    @property
    def w(self):
        return self.key.view(torch.int32).view(-1, 2)[:, 1]

    @property
    def has_replacement(self):
        return self.key != -1


def forest_replacements(edges, index, by_edge=True):
    """For every forest edge the edge that takes its place when it fails, on the device
    (ghs_forest_replace_device, csrc/replace.hip). `index`: the PathIndex of `forest_paths` over this
    edge list. A non-forest edge (a, b) inside one tree covers the forest edges of the path a .. b; per
    forest edge the smallest covering key w << 32 | eid is its replacement, none makes it a bridge of
    the graph. info counts tree_edges, covering_edges, cross_edges (non-forest edges between two
    trees), bridges and improving (forest edges with a lighter replacement: 0 for the MSF), and names the
    best swap: best_out_eid -> best_in_eid changes the total weight by best_delta, the least possible
    (the second-best spanning forest); both eids are 0xffffffff when every forest edge is a bridge.
    Returns (Replacements, info). A closed index or edges on another device raise ValueError. Runs on
    torch's current stream; one query or replacement at a time per index."""
    if not isinstance(index, PathIndex) or not index._h:
        raise ValueError("the index is closed")
    if edges.u is None:
        raise ValueError("forest_replacements needs the COO form (u present); a CSR-only list is not supported")
    if edges.device != index.device:
        raise ValueError(f"the edges are on device {edges.device}, the index on device {index.device}")
    if edges.n != index.n:
        raise ValueError(f"the index covers {index.n} vertices, the edge list {edges.n}")
    L = _native.load()
    n, m, dev = edges.n, edges.m, index.device
    pi = _native.PathsInfo()
    _native.check(L.ghs_forest_paths_info(index._h, ctypes.byref(pi)))
    _native.require_gpu()
    with torch.cuda.device(dev):
        wb = int(L.ghs_forest_replace_workspace_bytes(n, pi.max_depth))
        key = torch.empty(n, dtype=torch.int64, device=dev)
        eid = torch.empty(m, dtype=torch.int32, device=dev) if by_edge else None
        ws = torch.empty(wb, dtype=torch.uint8, device=dev)
        res = _native.ReplaceResult()
        _native.check(L.ghs_forest_replace_device(index._h, m, _ptr(edges.u), _ptr(edges.v), _ptr(edges.w), _ptr(key),
                                                  _ptr(eid) if by_edge else None, _ptr(ws), wb, _stream(),
                                                  ctypes.byref(res)))
    info = res.as_dict()
    return Replacements(key, eid, info), info


def _live_index(index):
    if not isinstance(index, PathIndex) or not index._h:
        raise ValueError("the index is closed")
    return index


def forest_distances(index, a, b, hops=False, lca=False):
    """How far is it from a[i] to b[i] along the forest? On the device (ghs_forest_dist_query,
    csrc/dist.hip): dist = wd[a] + wd[b] - 2 wd[lca(a, b)] over `index.wdepth(hops)`, one fused kernel
    (the path query's LCA walk, then three gathers). `index`: the PathIndex of `forest_paths`.
    a, b: int32 (uint32 bit patterns) or int64 GPU tensors of equal length, or ints.
    Returns a uint64 GPU tensor, one entry per pair: 0 where a == b, all ones (UINT64_MAX) where the
    ends are in different trees. Every finite distance is below 2^63, so `.view(torch.int64)` is exact,
    with -1 for different trees. hops=True counts edges instead of summing weights; rank-mapped weights
    (`edges.weights` set) raise ValueError unless hops=True. lca=True: returns (dist, lca) with lca
    int32 (uint32 bits, -1 for different trees). An id >= n raises GHSError (GHS_E_ARG). Runs on torch's
    current stream; one call at a time per index. `index.last_distance_info` keeps the fields of
    ghs_dist_query_result_t (queries, connected, disconnected, max_dist, ms_total)."""
    index = _live_index(index)
    wd = index.wdepth(hops)
    dev = index.device
    ta = torch.as_tensor(a, device=dev).reshape(-1) if not isinstance(a, torch.Tensor) else a
    tb = torch.as_tensor(b, device=dev).reshape(-1) if not isinstance(b, torch.Tensor) else b
    for name, t in (("a", ta), ("b", tb)):
        if t.dim() != 1 or t.device != dev:
            raise ValueError(f"{name}: a one-dimensional tensor on the index's device (or an int) expected")
    if ta.numel() != tb.numel():
        raise ValueError("a and b must have equal length")
    ta, tb = _as_u32_tensor(ta, "a"), _as_u32_tensor(tb, "b")
    q = int(ta.numel())
    if q >= (1 << 32):
        raise ValueError("at most 2^32 - 1 pairs")
    with torch.cuda.device(dev):
        odist = torch.empty(q, dtype=torch.int64, device=dev)
        olca = torch.empty(q, dtype=torch.int32, device=dev) if lca else None
        res = _native.DistQueryResult()
        _native.check(_native.load().ghs_forest_dist_query(index._h, _ptr(wd), q, _ptr(ta), _ptr(tb), _ptr(odist),
                                                           _ptr(olca), ctypes.byref(res), _stream()))
    index.last_distance_info = res.as_dict()
    odist = odist.view(torch.uint64)
    return (odist, olca) if lca else odist


class EdgeDistances:
    """What `forest_edge_distances` returns. dist: uint64[m] on the device, the forest distance between
    every graph edge's ends (all ones for an edge between two trees); None when left out. w: the edge
    weights (int32 holding uint32 bits). info: the fields of ghs_edge_dist_result_t as a dict, with the
    128-bit sum as the Python int sum_dist: edges, sum_dist, sum_w, max_dist, max_eid, cross_edges,
    tight_edges, ms_total."""

    def __init__(self, dist, w, info=None):
        self.dist, self.w, self.info = dist, w, info

    def stretch(self):
        """dist / w per edge as float64 on the device: inf where w == 0 and dist > 0 (and for an edge
        between two trees), 1.0 where both are 0. A forest edge has stretch 1."""
        if self.dist is None:
            raise ValueError("the call was made without the per-edge array (by_edge=False)")
        d = self.dist.view(torch.int64)
        w = self.w.to(torch.int64) & 0xFFFFFFFF
        s = d.to(torch.float64) / w.to(torch.float64)
        s = torch.where((d == 0) & (w == 0), torch.ones_like(s), s)
        return torch.where(d < 0, torch.full_like(s, float("inf")), s)

    def average_stretch(self):
        """sum_dist / sum_w over the edges inside one tree (the weighted average stretch), as a float;
        nan when the weights sum to 0."""
        return self.info["sum_dist"] / self.info["sum_w"] if self.info["sum_w"] else float("nan")


def forest_edge_distances(edges, index, by_edge=True):
    """The forest distance between the ends of every edge of the graph, on the device
    (ghs_forest_edge_dist_device, csrc/dist.hip): what the stretch dist / w of a spanning forest is
    made of. `index`: the PathIndex of `forest_paths` over this edge list. The kernel stays in exact
    integers: info carries sum_dist (a Python int, 128 bits wide on the device), sum_w, max_dist with
    the smallest edge id attaining it (max_eid), cross_edges (ends in different trees: 0 for a spanning
    forest) and tight_edges (dist == w: every forest edge and its ties). by_edge=False leaves the
    per-edge array out (the arg-max then repeats the walk). Rank-mapped weights (`edges.weights` set)
    raise ValueError: a sum of ranks means nothing.
    Returns an EdgeDistances (.dist, .stretch(), .info). Runs on torch's current stream; one call at a
    time per index."""
    index = _live_index(index)
    if edges.u is None:
        raise ValueError("forest_edge_distances needs the COO form (u present); a CSR-only list is not supported")
    if edges.device != index.device:
        raise ValueError(f"the edges are on device {edges.device}, the index on device {index.device}")
    if edges.n != index.n:
        raise ValueError(f"the index covers {index.n} vertices, the edge list {edges.n}")
    if edges.weights is not None or index.ranked:
        raise ValueError("rank-mapped weights (edges.weights is set): a sum of ranks means nothing; "
                         "use distances(..., hops=True) for distances in edges")
    wd = index.wdepth(False)
    m, dev = edges.m, index.device
    with torch.cuda.device(dev):
        dist = torch.empty(m, dtype=torch.int64, device=dev) if by_edge else None
        res = _native.EdgeDistResult()
        _native.check(_native.load().ghs_forest_edge_dist_device(index._h, _ptr(wd), m, _ptr(edges.u), _ptr(edges.v),
                                                                 _ptr(edges.w), _ptr(dist), ctypes.byref(res), _stream()))
    return EdgeDistances(dist.view(torch.uint64) if by_edge else None, edges.w, res.as_dict())


class TreeMetrics:
    """What `forest_diameters` returns, on the device. root_of: int32[n] (uint32 bits), every vertex's
    root. diameter: uint64[n] indexed by root (0 in every other slot). end_a / end_b: int32[n] indexed
    by root, the two far ends p and q (-1 in every other slot). ecc: uint64[n], every vertex's distance
    to the farthest vertex of its tree; None when left out. info: the fields of ghs_diameter_result_t
    as a dict: num_trees, max_diameter, max_root, min_ecc, center, ms_total."""

    def __init__(self, root_of, diameter, end_a, end_b, ecc, info=None):
        self.root_of, self.diameter, self.end_a, self.end_b, self.ecc, self.info = root_of, diameter, end_a, end_b, ecc, info

    def roots(self):
        """The roots in ascending order (int64 GPU tensor): the slots of diameter / end_a / end_b in use."""
        return torch.nonzero(self.end_a != -1).reshape(-1)

    def center(self):
        """(vertex, radius) of the tree with the largest diameter: the vertex with the smallest
        eccentricity (ties: the smallest id) and that eccentricity. None for an empty graph."""
        if not self.info or not self.info["num_trees"]:
            return None
        return self.info["center"], self.info["min_ecc"]


def forest_diameters(index, ecc=True, hops=False):
    """Diameter, far ends and eccentricities of every tree of the forest, on the device
    (ghs_forest_diameter_device, csrc/dist.hip). Two sweeps, exact for non-negative weights: p = the
    vertex farthest from the root, q = the vertex farthest from p (ties: the smallest id), diameter =
    dist(p, q), ecc[v] = max(dist(v, p), dist(v, q)). A single-vertex tree has diameter 0 and both ends
    equal to itself. `index`: the PathIndex of `forest_paths`. ecc=False leaves the eccentricities out
    of the result (the centre is found either way). hops=True counts edges; rank-mapped weights
    (`edges.weights` set) raise ValueError unless hops=True.
    Returns a TreeMetrics (.root_of, .diameter, .end_a, .end_b, .ecc, .center(), .info). Runs on torch's
    current stream; one call at a time per index."""
    index = _live_index(index)
    wd = index.wdepth(hops)
    L = _native.load()
    n, dev = index.n, index.device
    pi = _native.PathsInfo()
    _native.check(L.ghs_forest_paths_info(index._h, ctypes.byref(pi)))
    with torch.cuda.device(dev):
        wb = int(L.ghs_forest_dist_workspace_bytes(n, pi.max_depth))
        root_of, end_a, end_b = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
        diam = torch.empty(n, dtype=torch.int64, device=dev)
        oecc = torch.empty(n, dtype=torch.int64, device=dev) if ecc else None
        ws = torch.empty(wb, dtype=torch.uint8, device=dev)
        res = _native.DiameterResult()
        _native.check(L.ghs_forest_diameter_device(index._h, _ptr(wd), _ptr(root_of), _ptr(diam), _ptr(end_a), _ptr(end_b),
                                                   _ptr(oecc), _ptr(ws), wb, ctypes.byref(res), _stream()))
    del ws
    return TreeMetrics(root_of, diam.view(torch.uint64), end_a, end_b, oecc.view(torch.uint64) if ecc else None,
                       res.as_dict())


class DeviceBatch:
    """Many small graphs in batch-canonical form as torch tensors (int32 holding uint32 bit
    patterns): nvert[B], eoff[B + 1], u / v / w of eoff[B] entries, vertex ids local to each graph,
    graph g's canonical slice at [eoff[g], eoff[g + 1]) (include/ghs_mst.h, "batched solve")."""

    def __init__(self, nvert, eoff, u, v, w):
        self.nvert, self.eoff, self.u, self.v, self.w = nvert, eoff, u, v, w

    @property
    def num_graphs(self):
        return int(self.nvert.numel())

    @property
    def m(self):
        return int(self.u.numel())

    @property
    def device(self):
        return self.nvert.device

    @classmethod
    def from_graphs(cls, graphs, device="cuda"):
        """[CanonicalGraph] -> one packed batch (H2D copy). Graphs over the batch caps are packed as
        they are: batch_mst reports them with status 3."""
        from .mst import pack_batch

        def dev(a):
            return torch.from_numpy(a.view("int32").copy()).to(device)
        return cls(*(dev(a) for a in pack_batch(list(graphs))))

    def to_host(self):
        """The batch as a list of CanonicalGraph (D2H copy)."""
        from .graph import CanonicalGraph
        nvert = self.nvert.cpu().numpy().view("uint32")
        eoff = self.eoff.cpu().numpy().view("uint32").tolist()
        u, v, w = (t.cpu().numpy().view("uint32") for t in (self.u, self.v, self.w))
        return [CanonicalGraph(int(nvert[g]), u[eoff[g]:eoff[g + 1]], v[eoff[g]:eoff[g + 1]], w[eoff[g]:eoff[g + 1]])
                for g in range(len(nvert))]


def batch_mst(batch):
    """Solve every graph of a DeviceBatch in one launch on torch's current stream
    (ghs_mst_batch_device: one workgroup per graph, no host sync while enqueueing). Returns
    (in_mst uint8 device tensor of batch.m flags, results): results is a structured numpy array
    (_native.BATCH_RESULT_DTYPE, one entry per graph) read after the stream's sync; per-graph
    problems are reported only in results["status"]."""
    import numpy as np
    L = _native.load()
    _native.require_gpu()
    B, dev = batch.num_graphs, batch.device
    in_mst = torch.empty(max(batch.m, 1), dtype=torch.uint8, device=dev)
    if B == 0:
        return in_mst[:0], np.zeros(0, dtype=_native.BATCH_RESULT_DTYPE)
    ws_bytes = int(L.ghs_batch_workspace_bytes(B))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    res = torch.empty(B * ctypes.sizeof(_native.BatchResult), dtype=torch.uint8, device=dev)
    _native.check(L.ghs_mst_batch_device(B, _ptr(batch.nvert), _ptr(batch.eoff), _ptr(batch.u), _ptr(batch.v),
                                         _ptr(batch.w), _ptr(ws), ws_bytes, _ptr(in_mst), _ptr(res), _stream()))
    torch.cuda.current_stream().synchronize()
    return in_mst[: batch.m], res.cpu().numpy().view(_native.BATCH_RESULT_DTYPE)


def flags_to_eids(in_mst, lo, hi, capacity=None):
    """The edge ids e in [lo, hi) with in_mst[e] != 0, ascending, as an int64 device tensor — on the
    device (ghs_flags_to_eids: a flagged select), never through torch.nonzero (whose first call per
    process loaded for ~100 s with 4 ranks sharing one GPU, the gloo rehearsal's stall)."""
    lo, hi = int(lo), int(hi)
    cap = (hi - lo) if capacity is None else int(capacity)
    out = torch.empty(max(cap, 1), dtype=torch.int32, device=in_mst.device)
    cnt = ctypes.c_uint64(0)
    _native.check(_native.load().ghs_flags_to_eids(_ptr(in_mst), lo, hi, _ptr(out), cap, ctypes.byref(cnt), _stream()))
    return out[: cnt.value].to(torch.int64)


def emulated_mst(edges, num_ranks, config=None):
    """The multi-rank loop of an N-GPU solve (ghs_solver_run, every rank its own solver, stream
    and host thread over its edge range) with all N ranks on THIS device and in-process
    collectives (ghs_mst_emulated) — the N-rank protocol checked on one GPU. Returns
    (Result, [round stats], in_mst uint8 tensor of m flags)."""
    L = _native.load()
    _native.require_gpu()
    cfg = config if config is not None else _native.make_config()
    in_mst = torch.zeros(max(edges.m, 1), dtype=torch.uint8, device=edges.device)
    torch.cuda.synchronize(edges.device)  # the rank streams read u/v/w written on torch's stream
    res = _native.Result()
    stats = (_native.RoundStats * _native.GHS_MAX_ROUND_STATS)()
    _native.check(L.ghs_mst_emulated(edges.n, edges.m, _ptr(edges.u), _ptr(edges.v), _ptr(edges.w), int(num_ranks),
                                     ctypes.byref(cfg), _ptr(in_mst), ctypes.byref(res), stats))
    return res, _native.RoundStatsList(stats, res.num_stats), in_mst[: edges.m]
