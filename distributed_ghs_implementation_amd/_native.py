"""ctypes binding of libghs_mst.so (the C-ABI declared in include/ghs_mst.h).

The product path has exactly one implementation of the MST: the gfx950 HIP kernels in this
library. There is no CPU fallback — if the library is missing or no GPU is visible, every
compute entry point raises. (The CPU restatement used to CHECK results lives in oracle/, which
this package never imports.)
"""
import atexit
import collections.abc
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GHS_MST_LIB", os.path.join(_HERE, "lib", "libghs_mst.so"))

GHS_OK = 0
GHS_NEED_EXCHANGE = 1  # positive status of ghs_solver_minedge (several ranks opened a level)
GHS_E_ARG = -1
GHS_E_NONCANON = -2
GHS_E_HIP = -3
GHS_E_ROUNDCAP = -4
GHS_E_NODEVICE = -5
GHS_E_NOMEM = -6
GHS_E_STATE = -7
GHS_MAX_ROUND_STATS = 64
# ghs_weight_ranks_device's weight types (include/ghs_mst.h GHS_W_*)
GHS_W_FLOAT32 = 0
GHS_W_FLOAT64 = 1
GHS_W_INT64 = 2
GHS_W_UINT64 = 3
# ghs_forest_labels_device's cut modes (include/ghs_mst.h GHS_CUT_*)
GHS_CUT_NONE = 0
GHS_CUT_WEIGHT = 1
GHS_CUT_COUNT = 2
# the metrics of ghs_forest_wdepth_device (include/ghs_mst.h GHS_DIST_*)
GHS_DIST_WEIGHT = 0
GHS_DIST_HOPS = 1

_ERR_NAMES = {
    GHS_E_ARG: "GHS_E_ARG", GHS_E_NONCANON: "GHS_E_NONCANON", GHS_E_HIP: "GHS_E_HIP",
    GHS_E_ROUNDCAP: "GHS_E_ROUNDCAP", GHS_E_NODEVICE: "GHS_E_NODEVICE", GHS_E_NOMEM: "GHS_E_NOMEM",
    GHS_E_STATE: "GHS_E_STATE",
}

# every symbol include/ghs_mst.h declares (tests check the .so exports all of them)
EXPORTED_SYMBOLS = (
    "ghs_abi_version", "ghs_last_error", "ghs_device_count", "ghs_mst_host", "ghs_mst_multi",
    "ghs_default_config", "ghs_workspace_bytes", "ghs_mst_device",
    "ghs_check_canonical",
    "ghs_solver_create", "ghs_solver_minedge", "ghs_solver_exchange_buffer", "ghs_solver_pack_best",
    "ghs_solver_flag_bits", "ghs_solver_merge_flag_bits",
    "ghs_solver_unpack_best", "ghs_solver_best_slots",
    "ghs_solver_contract", "ghs_solver_finish", "ghs_solver_reset", "ghs_solver_cancel", "ghs_solver_destroy",
    "ghs_solver_hook_local", "ghs_solver_unpack_hook",
    "ghs_solver_hook_slots", "ghs_solver_hook_owner", "ghs_solver_apply_hooks", "ghs_solver_tail_begin",
    "ghs_solver_tail_buffers", "ghs_solver_tail_agree", "ghs_solver_tail_round",
    "ghs_rmat_temp_bytes", "ghs_rmat_generate", "ghs_rmat_tuples", "ghs_grid_generate",
    "ghs_profile_enable", "ghs_profile_read", "ghs_kernel_name",
    "ghs_comm_unique_id", "ghs_comm_init", "ghs_comm_destroy", "ghs_solver_run", "ghs_mst_emulated",
    "ghs_release_cache", "ghs_slot_retries", "ghs_flags_to_eids",
    "ghs_mst_device_csr", "ghs_csr_offsets", "ghs_solver_create_csr",
    "ghs_batch_workspace_bytes", "ghs_mst_batch_device", "ghs_mst_batch_host",
    "ghs_canonicalize_temp_bytes", "ghs_canonicalize_device",
    "ghs_weight_ranks_temp_bytes", "ghs_weight_ranks_device",
    "ghs_verify_workspace_bytes", "ghs_verify_msf_device",
    "ghs_forest_labels_workspace_bytes", "ghs_forest_labels_device", "ghs_forest_labels_host",
    "ghs_forest_root_workspace_bytes", "ghs_forest_root_device", "ghs_forest_root_host",
    "ghs_forest_paths_index_bytes", "ghs_forest_paths_create", "ghs_forest_paths_query", "ghs_forest_paths_destroy",
    "ghs_forest_paths_host", "ghs_forest_paths_info",
    "ghs_forest_replace_workspace_bytes", "ghs_forest_replace_device", "ghs_forest_replace_host",
    "ghs_forest_replace_phases",
    "ghs_forest_dist_workspace_bytes", "ghs_forest_wdepth_device", "ghs_forest_dist_query",
    "ghs_forest_edge_dist_device", "ghs_forest_diameter_device", "ghs_forest_dist_host", "ghs_forest_diameter_host",
    "ghs_forest_dendro_workspace_bytes", "ghs_forest_dendro_device", "ghs_forest_dendro_host",
    "ghs_forest_cluster_workspace_bytes", "ghs_forest_cluster_capacity", "ghs_forest_cluster_device",
    "ghs_forest_cluster_host",
    "ghs_mutual_reach_workspace_bytes", "ghs_mutual_reach_device", "ghs_mutual_reach_host", "ghs_mutual_reach_phases",
    "ghs_knn_workspace_bytes", "ghs_knn_device", "ghs_knn_host",
    "ghs_emst_workspace_bytes", "ghs_emst_device", "ghs_emst_host", "ghs_emst_rounds",
)


class GHSError(RuntimeError):
    """A negative GHS_E_* return code from libghs_mst.so."""

    def __init__(self, code, message):
        super().__init__(f"{_ERR_NAMES.get(code, code)}: {message}")
        self.code = code


class RoundStats(ctypes.Structure):
    _fields_ = [
        ("level", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("level_arcs", ctypes.c_uint64),
        ("live_arcs", ctypes.c_uint64),
        ("active_components", ctypes.c_uint64),
        ("hooks", ctypes.c_uint64),
        ("ms_minedge", ctypes.c_float),
        ("ms_hook", ctypes.c_float),
        ("ms_jump", ctypes.c_float),
        ("ms_active", ctypes.c_float),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class RoundStatsList(collections.abc.Sequence):
    """The per-round stats of one solve as a read-only sequence of dicts, converted on access
    (a solve returns up to 64 rounds; building every dict eagerly cost ~27 us per solve)."""

    def __init__(self, arr, n):
        self._arr, self._n = arr, int(n)

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self._n))]
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError(i)
        return self._arr[i].as_dict()

    def __repr__(self):
        return repr(list(self))


ABI_VERSION = 10  # include/ghs_mst.h GHS_MST_ABI_VERSION


class Result(ctypes.Structure):
    _fields_ = [
        ("num_mst_edges", ctypes.c_uint64),
        ("total_weight", ctypes.c_uint64),
        ("rounds", ctypes.c_uint32),
        ("num_stats", ctypes.c_uint32),
        ("levels", ctypes.c_uint32),
        ("pass_flags", ctypes.c_uint32),
        ("ms_total", ctypes.c_double),
        ("ms_select", ctypes.c_float),
        ("ms_filter", ctypes.c_float),
        ("canon_edges", ctypes.c_uint64),
        ("select_out", ctypes.c_uint64),
        ("filter_out", ctypes.c_uint64),
        # ABI 7: the multi-rank drivers' host phases (max over ranks) and cache reuse
        ("ms_setup", ctypes.c_double),
        ("ms_solve", ctypes.c_double),
        ("ms_gather", ctypes.c_double),
        ("reused", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


class BatchResult(ctypes.Structure):
    """ghs_batch_result_t: one graph of a batched solve (ghs_mst_batch_device / ghs_mst_batch_host)."""
    _fields_ = [
        ("total_weight", ctypes.c_uint64),
        ("num_mst_edges", ctypes.c_uint32),
        ("rounds", ctypes.c_uint32),
        ("status", ctypes.c_uint32),  # 0 ok, 1 not canonical, 2 round cap, 3 over the size caps
        ("reserved", ctypes.c_uint32),
    ]


class VerifyResult(ctypes.Structure):
    """ghs_verify_result_t: the device verifier's verdict (ghs_verify_msf_device)."""
    _fields_ = [
        ("ok", ctypes.c_uint32),
        ("rounds", ctypes.c_uint32),
        ("overfull", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("tree_edges", ctypes.c_uint64),
        ("components", ctypes.c_uint64),
        ("total_weight", ctypes.c_uint64),
        ("cyclic_edges", ctypes.c_uint64),
        ("unspanned_edges", ctypes.c_uint64),
        ("lighter_edges", ctypes.c_uint64),
        ("first_bad_eid", ctypes.c_uint64),  # UINT64_MAX: none
        ("ms_total", ctypes.c_double),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        d["ok"], d["overfull"] = bool(d["ok"]), bool(d["overfull"])
        return d


class LabelsResult(ctypes.Structure):
    """ghs_labels_result_t: what ghs_forest_labels_device / ghs_forest_labels_host found."""
    _fields_ = [
        ("flagged_edges", ctypes.c_uint64),
        ("kept_edges", ctypes.c_uint64),
        ("dropped_edges", ctypes.c_uint64),
        ("num_clusters", ctypes.c_uint64),
        ("cut_key", ctypes.c_uint64),  # UINT64_MAX: nothing dropped by a count cut
        ("rounds", ctypes.c_uint32),
        ("is_forest", ctypes.c_uint32),
        ("ms_total", ctypes.c_double),
        ("reserved", ctypes.c_uint64),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        d["is_forest"] = bool(d["is_forest"])
        return d


class RootResult(ctypes.Structure):
    """ghs_root_result_t: what ghs_forest_root_device / ghs_forest_root_host found."""
    _fields_ = [
        ("flagged_edges", ctypes.c_uint64),
        ("num_trees", ctypes.c_uint64),
        ("max_depth", ctypes.c_uint64),
        ("rounds", ctypes.c_uint32),
        ("is_forest", ctypes.c_uint32),
        ("ms_total", ctypes.c_double),
        ("reserved", ctypes.c_uint64),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        d["is_forest"] = bool(d["is_forest"])
        return d


class DendroResult(ctypes.Structure):
    """ghs_dendro_result_t: what ghs_forest_dendro_device / ghs_forest_dendro_host found."""
    _fields_ = [
        ("flagged_edges", ctypes.c_uint64),
        ("num_trees", ctypes.c_uint64),
        ("max_height", ctypes.c_uint64),
        ("levels", ctypes.c_uint32),
        ("rounds", ctypes.c_uint32),
        ("is_forest", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("ms_total", ctypes.c_double),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        d["is_forest"] = bool(d["is_forest"])
        return d


GHS_CLUSTER_ALLOW_SINGLE = 1
GHS_CLUSTER_LEAF = 2


class ClusterResult(ctypes.Structure):
    """ghs_cluster_result_t: what ghs_forest_cluster_device / ghs_forest_cluster_host found."""
    _fields_ = [
        ("num_clusters", ctypes.c_uint32),
        ("num_selected", ctypes.c_uint32),
        ("num_noise", ctypes.c_uint32),
        ("num_top", ctypes.c_uint32),
        ("cluster_height", ctypes.c_uint32),
        ("rounds", ctypes.c_uint32),
        ("select_launches", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("ms_total", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


def cluster_args(min_cluster_size, method, allow_single_cluster):
    """(min_cluster_size, flags) of the cluster entry points; ValueError for what they would refuse."""
    mcs = int(min_cluster_size)
    if mcs < 2:
        raise ValueError(f"min_cluster_size must be >= 2, got {min_cluster_size}")
    if method not in ("eom", "leaf"):
        raise ValueError(f"method: 'eom' or 'leaf' expected, got {method!r}")
    return mcs, (GHS_CLUSTER_LEAF if method == "leaf" else 0) | (GHS_CLUSTER_ALLOW_SINGLE if allow_single_cluster else 0)


# the row classes of ghs_mutual_reach_device (include/ghs_mst.h GHS_MREACH_*): degrees from which one
# workgroup, and from which the whole grid, selects a row
GHS_MREACH_LANE_ROW_MAX = 32
GHS_MREACH_BLOCK_ROW_MIN = 256
GHS_MREACH_GRID_ROW_MIN = 32768


class MreachResult(ctypes.Structure):
    """ghs_mreach_result_t: what ghs_mutual_reach_device / ghs_mutual_reach_host found."""
    _fields_ = [
        ("short_rows", ctypes.c_uint64),
        ("isolated", ctypes.c_uint64),
        ("raised_edges", ctypes.c_uint64),
        ("max_degree", ctypes.c_uint32),
        ("block_rows", ctypes.c_uint32),
        ("grid_rows", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("ms_total", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


def mreach_args(min_samples, short_rows, include_self=False):
    """k of the mutual-reachability entry points (0: include_self left nothing to select); ValueError
    for what they would refuse."""
    try:
        k = int(min_samples)
    except (TypeError, ValueError):
        raise ValueError(f"min_samples must be an integer >= 1, got {min_samples!r}") from None
    if k < 1 or k != min_samples:
        raise ValueError(f"min_samples must be an integer >= 1, got {min_samples!r}")
    if k >= (1 << 32):
        raise ValueError(f"min_samples must be < 2^32, got {min_samples!r}")
    if short_rows not in ("error", "clamp"):
        raise ValueError(f"short_rows: 'error' or 'clamp' expected, got {short_rows!r}")
    return k - 1 if include_self else k


# ghs_knn_device's limits, metrics and tile shape (include/ghs_mst.h GHS_KNN_*)
GHS_KNN_MAX_K = 128
GHS_KNN_MAX_DIM = 4096
GHS_KNN_MAX_SLICES = 64
GHS_KNN_SQEUCLIDEAN = 0
GHS_KNN_EUCLIDEAN = 1
GHS_KNN_TILE_Q = 64
GHS_KNN_TILE_C = 64
GHS_KNN_DIM_CHUNK = 32
KNN_METRICS = {"sqeuclidean": GHS_KNN_SQEUCLIDEAN, "euclidean": GHS_KNN_EUCLIDEAN}


class KnnResult(ctypes.Structure):
    """ghs_knn_result_t: what ghs_knn_device / ghs_knn_host found."""
    _fields_ = [
        ("pairs", ctypes.c_uint64),
        ("zero_neighbours", ctypes.c_uint64),
        ("slices", ctypes.c_uint32),
        ("query_tiles", ctypes.c_uint32),
        ("ms_total", ctypes.c_double),
        ("reserved", ctypes.c_uint64 * 2),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


def knn_args(k, metric, slices=0, n=None, dim=None):
    """(k, metric code, slices) of the k-NN entry points; ValueError for what they would refuse, before
    anything touches the device. n, dim: the points' shape when it is known."""
    try:
        kk = int(k)
    except (TypeError, ValueError):
        raise ValueError(f"k must be an integer in [1, {GHS_KNN_MAX_K}], got {k!r}") from None
    if kk != k or not 1 <= kk <= GHS_KNN_MAX_K:
        raise ValueError(f"k must be an integer in [1, {GHS_KNN_MAX_K}], got {k!r}")
    if metric not in KNN_METRICS:
        raise ValueError(f"metric: 'euclidean' or 'sqeuclidean' expected, got {metric!r}")
    try:
        ss = int(slices)
    except (TypeError, ValueError):
        raise ValueError(f"slices must be an integer in [0, {GHS_KNN_MAX_SLICES}] (0: chosen from n), got {slices!r}") from None
    if ss != slices or not 0 <= ss <= GHS_KNN_MAX_SLICES:
        raise ValueError(f"slices must be an integer in [0, {GHS_KNN_MAX_SLICES}] (0: chosen from n), got {slices!r}")
    if dim is not None and not 1 <= int(dim) <= GHS_KNN_MAX_DIM:
        raise ValueError(f"points must have between 1 and {GHS_KNN_MAX_DIM} columns, got {dim}")
    if n is not None:
        if int(n) >= (1 << 32):
            raise ValueError("at most 2^32 - 1 points")
        if int(n) >= 1 and kk > int(n) - 1:
            raise ValueError(f"k = {kk} needs at least k + 1 points (a point is not its own neighbour), got n = {n}")
        if int(n) * kk >= (1 << 32):
            raise ValueError("n * k must be < 2^32")
    return kk, KNN_METRICS[metric], ss


class EmstResult(ctypes.Structure):
    """ghs_emst_result_t: what ghs_emst_device / ghs_emst_host found."""
    _fields_ = [
        ("num_edges", ctypes.c_uint64),
        ("pairs", ctypes.c_uint64),
        ("zero_edges", ctypes.c_uint64),
        ("rounds", ctypes.c_uint32),
        ("slices", ctypes.c_uint32),
        ("query_tiles", ctypes.c_uint32),
        ("reserved0", ctypes.c_uint32),
        ("components_after_first_round", ctypes.c_uint64),
        ("ms_total", ctypes.c_double),
        ("reserved", ctypes.c_uint64 * 1),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


def emst_args(metric, slices=0, n=None, dim=None):
    """(metric code, slices) of the exact-MST entry points; ValueError for what they would refuse, before
    anything touches the device. n, dim: the points' shape when it is known."""
    if metric not in KNN_METRICS:
        raise ValueError(f"metric: 'euclidean' or 'sqeuclidean' expected, got {metric!r}")
    try:
        ss = int(slices)
    except (TypeError, ValueError):
        raise ValueError(f"slices must be an integer in [0, {GHS_KNN_MAX_SLICES}] (0: chosen from n), got {slices!r}") from None
    if ss != slices or not 0 <= ss <= GHS_KNN_MAX_SLICES:
        raise ValueError(f"slices must be an integer in [0, {GHS_KNN_MAX_SLICES}] (0: chosen from n), got {slices!r}")
    if dim is not None and not 1 <= int(dim) <= GHS_KNN_MAX_DIM:
        raise ValueError(f"points must have between 1 and {GHS_KNN_MAX_DIM} columns, got {dim}")
    if n is not None and int(n) - 1 >= (1 << 31):
        raise ValueError("at most 2^31 points (n - 1 tree edges must be < 2^31)")
    return KNN_METRICS[metric], ss


class PathsResult(ctypes.Structure):
    """ghs_paths_result_t: what ghs_forest_paths_create built."""
    _fields_ = [
        ("levels", ctypes.c_uint64),
        ("max_depth", ctypes.c_uint64),
        ("num_trees", ctypes.c_uint64),
        ("index_bytes", ctypes.c_uint64),
        ("ms_total", ctypes.c_double),
        ("reserved", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class PathsQueryResult(ctypes.Structure):
    """ghs_paths_query_result_t: one ghs_forest_paths_query / ghs_forest_paths_host call."""
    _fields_ = [
        ("queries", ctypes.c_uint64),
        ("connected", ctypes.c_uint64),
        ("ms_total", ctypes.c_double),
        ("reserved", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class PathsInfo(ctypes.Structure):
    """ghs_paths_info_t: what a live ghs_paths_t indexes (ghs_forest_paths_info)."""
    _fields_ = [
        ("n", ctypes.c_uint64),
        ("levels", ctypes.c_uint64),
        ("max_depth", ctypes.c_uint64),
        ("d_index", ctypes.c_void_p),
    ]

    def as_dict(self):
        return {"n": self.n, "levels": self.levels, "max_depth": self.max_depth, "d_index": self.d_index or 0}


class ReplaceResult(ctypes.Structure):
    """ghs_replace_result_t: one ghs_forest_replace_device / ghs_forest_replace_host call."""
    _fields_ = [
        ("tree_edges", ctypes.c_uint64),
        ("covering_edges", ctypes.c_uint64),
        ("cross_edges", ctypes.c_uint64),
        ("bridges", ctypes.c_uint32),
        ("improving", ctypes.c_uint32),
        ("best_delta", ctypes.c_int64),
        ("best_out_eid", ctypes.c_uint32),
        ("best_in_eid", ctypes.c_uint32),
        ("ms_total", ctypes.c_double),
        ("reserved", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class DistQueryResult(ctypes.Structure):
    """ghs_dist_query_result_t: one ghs_forest_dist_query / ghs_forest_dist_host call."""
    _fields_ = [
        ("queries", ctypes.c_uint64),
        ("connected", ctypes.c_uint64),
        ("disconnected", ctypes.c_uint64),
        ("max_dist", ctypes.c_uint64),
        ("ms_total", ctypes.c_double),
        ("reserved", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class EdgeDistResult(ctypes.Structure):
    """ghs_edge_dist_result_t: one ghs_forest_edge_dist_device call. as_dict joins the two words of the
    128-bit sum into the Python int sum_dist."""
    _fields_ = [
        ("edges", ctypes.c_uint64),
        ("sum_dist_lo", ctypes.c_uint64),
        ("sum_dist_hi", ctypes.c_uint64),
        ("sum_w", ctypes.c_uint64),
        ("max_dist", ctypes.c_uint64),
        ("cross_edges", ctypes.c_uint64),
        ("tight_edges", ctypes.c_uint64),
        ("max_eid", ctypes.c_uint32),
        ("reserved32", ctypes.c_uint32),
        ("ms_total", ctypes.c_double),
        ("reserved", ctypes.c_uint64),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}
        d["sum_dist"] = (d.pop("sum_dist_hi") << 64) | d.pop("sum_dist_lo")
        return d


class DiameterResult(ctypes.Structure):
    """ghs_diameter_result_t: one ghs_forest_diameter_device / ghs_forest_diameter_host call."""
    _fields_ = [
        ("num_trees", ctypes.c_uint64),
        ("max_diameter", ctypes.c_uint64),
        ("min_ecc", ctypes.c_uint64),
        ("max_root", ctypes.c_uint32),
        ("center", ctypes.c_uint32),
        ("ms_total", ctypes.c_double),
        ("reserved", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


# the same layout as a numpy structured dtype (a device buffer of results viewed on the host)
BATCH_RESULT_DTYPE = [("total_weight", "<u8"), ("num_mst_edges", "<u4"), ("rounds", "<u4"), ("status", "<u4"),
                      ("reserved", "<u4")]
BATCH_MAX_VERTICES = 4096   # GHS_BATCH_MAX_VERTICES
BATCH_MAX_EDGES = 1 << 20   # GHS_BATCH_MAX_EDGES
# largest vertex count of each size class of the batch kernel (csrc/batch.hip CLS_N): a graph runs in
# the first class it fits, on 64 / 256 / 1024 threads with 12 B of LDS per class vertex
BATCH_CLASS_LIMITS = (64, 512, 4096)


class KernelRecord(ctypes.Structure):
    """ghs_kernel_record_t: one profiled launch (ghs_profile_enable / ghs_profile_read)."""
    _fields_ = [
        ("kernel", ctypes.c_uint32),
        ("round", ctypes.c_uint32),
        ("level", ctypes.c_uint32),
        ("solver", ctypes.c_uint32),
        ("items", ctypes.c_uint64),
        ("ms", ctypes.c_float),
        ("reserved2", ctypes.c_float),
    ]


def profile_enable(on=True):
    check(load().ghs_profile_enable(1 if on else 0))


def profile_read():
    """Drain the per-launch profile: [{"kernel": name, "round", "level", "items", "ms"}, ...]."""
    L = load()
    out = []
    while True:
        buf = (KernelRecord * 4096)()
        c = ctypes.c_uint32(0)
        check(L.ghs_profile_read(buf, 4096, ctypes.byref(c)))
        for i in range(c.value):
            r = buf[i]
            out.append({"kernel": L.ghs_kernel_name(r.kernel).decode(), "round": r.round, "level": r.level,
                        "solver": r.solver, "items": r.items, "ms": r.ms})
        if c.value < 4096:
            return out


# ghs_config_t.options bits (include/ghs_mst.h GHS_OPT_*)
OPT_NO_SEED_RUNS = 0x1
OPT_NO_DENSE = 0x2
OPT_BUCKETED = 0x4
OPT_NO_BUCKETED = 0x8
OPT_DEBUG = 0x10
OPT_TIME_ROUNDS = 0x20
OPT_DETAIL = 0x40
OPT_BUCKETED_FIRST = 0x80
OPT_NO_WINDOW = 0x100
OPT_NO_TAIL = 0x200
OPT_CHECK_TOTALS = 0x400  # ABI 8: per level, report totals vs a stream-ordered copy of the counters
OPT_KEEP_CACHE = 0x800    # ABI 8: the multi-rank drivers keep their per-rank state for the next call

# ghs_result_t.pass_flags bits
PASS_BUCKETED = 0x1
PASS_LATTICE = 0x2
PASS_WINDOWED = 0x4
PASS_TAIL = 0x8


class Config(ctypes.Structure):
    """ghs_config_t: the weight-level plan of the filter and the path options (speed only;
    results never change). The library reads no environment variable that changes its path."""
    _fields_ = [
        ("max_levels", ctypes.c_uint32),
        ("num_ranks", ctypes.c_uint32),
        ("level1_edges_per_vertex", ctypes.c_double),
        ("level_growth", ctypes.c_double),
        ("options", ctypes.c_uint32),
        ("dedup_max", ctypes.c_uint32),
        ("fault_rank", ctypes.c_uint32),
        ("fault_round", ctypes.c_uint32),
    ]


def make_config(max_levels=None, level1_edges_per_vertex=None, level_growth=None, num_ranks=None, options=None,
                dedup_max=None, fault_rank=None, fault_round=None):
    c = Config()
    load().ghs_default_config(ctypes.byref(c))
    if options is not None:
        c.options = int(options)
    if dedup_max is not None:
        c.dedup_max = int(dedup_max)
    if fault_rank is not None:
        c.fault_rank = int(fault_rank)
    if fault_round is not None:
        c.fault_round = int(fault_round)
    if num_ranks is not None:
        c.num_ranks = int(num_ranks)
    if max_levels is not None:
        c.max_levels = int(max_levels)
    if level1_edges_per_vertex is not None:
        c.level1_edges_per_vertex = float(level1_edges_per_vertex)
    if level_growth is not None:
        c.level_growth = float(level_growth)
    return c


_lib = None
_lock = threading.Lock()


def load():
    """Load the library once; raise loudly if it is missing (no fallback)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        # Load torch's HIP runtime first when torch is installed: libghs_mst.so then binds to the
        # same libamdhip64.so.7 (same SONAME) instead of bringing up a second runtime, so torch's
        # device pointers and streams are valid in both.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"libghs_mst.so not found at {LIB_PATH}; build it with "
                "`make -C distributed_ghs_implementation_amd/csrc` (or __graft_entry__.build())")
        L = ctypes.CDLL(LIB_PATH)
        u32, u64, i32, sz, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p
        P = ctypes.POINTER
        sigs = {
            "ghs_abi_version": (i32, []),
            "ghs_last_error": (ctypes.c_char_p, []),
            "ghs_device_count": (i32, [P(i32)]),
            "ghs_mst_host": (i32, [u32, u64, vp, vp, vp, vp, P(Result), P(RoundStats)]),
            "ghs_mst_multi": (i32, [u32, u64, vp, vp, vp, i32, vp, vp, vp, P(Result), P(RoundStats)]),
            "ghs_default_config": (None, [P(Config)]),
            "ghs_check_canonical": (i32, [u32, u64, vp, vp, vp, P(i32)]),
            "ghs_workspace_bytes": (sz, [u32, u64, u64]),
            "ghs_mst_device": (i32, [u32, u64, vp, vp, vp, P(Config), vp, sz, vp, vp, P(Result), P(RoundStats)]),
            "ghs_solver_create": (i32, [u32, u64, vp, vp, vp, u64, u64, P(Config), vp, sz, vp, vp, P(vp)]),
            "ghs_solver_minedge": (i32, [vp, P(u64)]),
            "ghs_solver_exchange_buffer": (i32, [vp, P(vp), P(u64)]),
            "ghs_solver_flag_bits": (i32, [vp, P(vp), P(u64)]),
            "ghs_solver_merge_flag_bits": (i32, [vp, vp, u32]),
            "ghs_solver_pack_best": (i32, [vp, vp]),
            "ghs_solver_unpack_best": (i32, [vp, vp]),
            "ghs_solver_best_slots": (i32, [vp, P(vp), P(u64)]),
            "ghs_solver_contract": (i32, [vp, P(i32)]),
            "ghs_solver_finish": (i32, [vp, P(Result), P(RoundStats)]),
            "ghs_solver_hook_local": (i32, [vp, vp, P(ctypes.c_uint64)]),
            "ghs_solver_unpack_hook": (i32, [vp, vp]),
            "ghs_solver_hook_slots": (i32, [vp, u32, P(vp), P(u64)]),
            "ghs_solver_hook_owner": (i32, [vp, u32, u64, vp]),
            "ghs_solver_apply_hooks": (i32, [vp, vp, P(vp)]),
            "ghs_solver_tail_begin": (i32, [vp, P(u64)]),
            "ghs_solver_tail_buffers": (i32, [vp, P(vp), P(vp)]),
            "ghs_solver_tail_agree": (i32, [vp]),
            "ghs_solver_tail_round": (i32, [vp, P(i32)]),
            "ghs_solver_reset": (i32, [vp]),
            "ghs_solver_cancel": (i32, [vp]),
            "ghs_solver_destroy": (i32, [vp]),
            "ghs_rmat_temp_bytes": (sz, [u32, u32]),
            "ghs_rmat_generate": (i32, [u32, u32, u64, u64, vp, vp, vp, P(u64), vp, sz, vp]),
            "ghs_rmat_tuples": (i32, [u32, u32, u64, vp, vp]),
            "ghs_profile_enable": (i32, [i32]),
            "ghs_profile_read": (i32, [vp, u32, P(u32)]),
            "ghs_kernel_name": (ctypes.c_char_p, [u32]),
            "ghs_grid_generate": (i32, [u32, u32, u64, vp, vp, vp, vp]),
            "ghs_comm_unique_id": (i32, [vp]),
            "ghs_comm_init": (i32, [i32, i32, vp, P(vp)]),
            "ghs_comm_destroy": (i32, [vp]),
            "ghs_solver_run": (i32, [vp, vp]),
            "ghs_mst_emulated": (i32, [u32, u64, vp, vp, vp, i32, P(Config), vp, P(Result), P(RoundStats)]),
            "ghs_release_cache": (i32, []),
            "ghs_slot_retries": (i32, [P(u64)]),
            "ghs_flags_to_eids": (i32, [vp, u64, u64, vp, u64, P(u64), vp]),
            # ABI 9: the CSR form of the canonical list
            "ghs_mst_device_csr": (i32, [u32, u64, vp, vp, vp, vp, P(Config), vp, sz, vp, vp, P(Result), P(RoundStats)]),
            "ghs_csr_offsets": (i32, [u32, u64, vp, vp, vp]),
            "ghs_solver_create_csr": (i32, [u32, u64, vp, vp, vp, vp, u64, u64, P(Config), vp, sz, vp, vp, P(vp)]),
            # ABI 10 addition: the batched solve
            "ghs_batch_workspace_bytes": (sz, [u32]),
            "ghs_mst_batch_device": (i32, [u32, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp]),
            "ghs_mst_batch_host": (i32, [u32, vp, vp, vp, vp, vp, vp, vp]),
            # ABI 10 addition: device ingest (raw edge list -> canonical list + raw indices)
            "ghs_canonicalize_temp_bytes": (sz, [u32, u64]),
            "ghs_canonicalize_device": (i32, [u32, u64, vp, vp, vp, vp, vp, vp, vp, P(u64), vp, sz, vp]),
            # ABI 10 addition: float / 64-bit weights -> dense ranks (the uint32 engine weights)
            "ghs_weight_ranks_temp_bytes": (sz, [u32, u64]),
            "ghs_weight_ranks_device": (i32, [u32, u64, vp, vp, P(u64), vp, sz, vp]),
            # ABI 10 addition: the device verifier (flags == the MSF, exactly)
            "ghs_verify_workspace_bytes": (sz, [u32, u64]),
            "ghs_verify_msf_device": (i32, [u32, u64, vp, vp, vp, vp, vp, sz, vp, P(VerifyResult)]),
            # ABI 10 addition: vertex labels of a flagged forest, with weight / count cuts
            "ghs_forest_labels_workspace_bytes": (sz, [u32, u64]),
            "ghs_forest_labels_device": (i32, [u32, u64, vp, vp, vp, vp, u32, u64, vp, vp, sz, vp, P(LabelsResult)]),
            "ghs_forest_labels_host": (i32, [u32, u64, vp, vp, vp, vp, u32, u64, vp, P(LabelsResult)]),
            # ABI 10 addition: the flagged forest rooted (parent, parent edge, depth, preorder, subtree size)
            "ghs_forest_root_workspace_bytes": (sz, [u32, u64]),
            "ghs_forest_root_device": (i32, [u32, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, P(RootResult)]),
            "ghs_forest_root_host": (i32, [u32, u64, vp, vp, vp, vp, vp, vp, vp, vp, P(RootResult)]),
            # ABI 10 addition: path queries on the rooted forest (bottleneck edge, LCA, hop count)
            "ghs_forest_paths_index_bytes": (sz, [u32, u64]),
            "ghs_forest_paths_create": (i32, [u32, u64, vp, vp, vp, vp, vp, vp, u64, vp, sz, vp, P(PathsResult), P(vp)]),
            "ghs_forest_paths_query": (i32, [vp, u64, vp, vp, vp, vp, vp, vp, P(PathsQueryResult)]),
            "ghs_forest_paths_destroy": (i32, [vp]),
            "ghs_forest_paths_host": (i32, [u32, u64, vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, P(PathsQueryResult)]),
            "ghs_forest_paths_info": (i32, [vp, P(PathsInfo)]),
            # ABI 10 addition: replacement edges, bridges and the best swap of the rooted forest
            "ghs_forest_replace_workspace_bytes": (sz, [u32, u64]),
            "ghs_forest_replace_device": (i32, [vp, u64, vp, vp, vp, vp, vp, vp, sz, vp, P(ReplaceResult)]),
            "ghs_forest_replace_host": (i32, [u32, u64, vp, vp, vp, vp, vp, vp, P(ReplaceResult)]),
            "ghs_forest_replace_phases": (i32, [i32, P(ctypes.c_double)]),
            # ABI 10 addition: tree distances, edge stretch and tree diameters on the rooted forest
            "ghs_forest_dist_workspace_bytes": (sz, [u32, u64]),
            "ghs_forest_wdepth_device": (i32, [vp, u32, vp, vp, sz, vp]),
            "ghs_forest_dist_query": (i32, [vp, vp, u64, vp, vp, vp, vp, P(DistQueryResult), vp]),
            "ghs_forest_edge_dist_device": (i32, [vp, vp, u64, vp, vp, vp, vp, P(EdgeDistResult), vp]),
            "ghs_forest_diameter_device": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, sz, P(DiameterResult), vp]),
            "ghs_forest_dist_host": (i32, [u32, u64, vp, vp, vp, vp, u32, u64, vp, vp, vp, vp, P(DistQueryResult)]),
            "ghs_forest_diameter_host": (i32, [u32, u64, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, P(DiameterResult)]),
            # ABI 10 addition: the single-linkage dendrogram (Kruskal merge tree) of the flagged forest
            "ghs_forest_dendro_workspace_bytes": (sz, [u32, u64]),
            "ghs_forest_dendro_device": (i32, [u32, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp,
                                               P(DendroResult)]),
            "ghs_forest_dendro_host": (i32, [u32, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, P(DendroResult)]),
            # ABI 10 addition: HDBSCAN cluster extraction from a dendrogram and one height per merge
            "ghs_forest_cluster_workspace_bytes": (sz, [u32, u64, u32]),
            "ghs_forest_cluster_capacity": (u64, [u32, u64, u32]),
            "ghs_forest_cluster_device": (i32, [u32, u64] + [vp] * 6 + [u32, u32] + [vp] * 10 + [vp, sz, vp,
                                                P(ClusterResult)]),
            "ghs_forest_cluster_host": (i32, [u32, u64] + [vp] * 6 + [u32, u32] + [vp] * 10 + [P(ClusterResult)]),
            # ABI 10 addition: core distances and mutual-reachability weights of a canonical edge list
            "ghs_mutual_reach_workspace_bytes": (sz, [u32, u64]),
            "ghs_mutual_reach_device": (i32, [u32, u64, vp, vp, vp, u32, vp, vp, vp, sz, vp, P(MreachResult)]),
            "ghs_mutual_reach_host": (i32, [u32, u64, vp, vp, vp, u32, vp, vp, P(MreachResult)]),
            "ghs_mutual_reach_phases": (i32, [i32, P(ctypes.c_double)]),
            # ABI 10 addition: exact brute-force k nearest neighbours of float32 points
            "ghs_knn_workspace_bytes": (sz, [u32, u32, u32, u32]),
            "ghs_knn_device": (i32, [u32, u32, vp, u32, u32, u32, vp, vp, vp, sz, vp, P(KnnResult)]),
            "ghs_knn_host": (i32, [u32, u32, vp, u32, u32, vp, vp, P(KnnResult)]),
            "ghs_emst_workspace_bytes": (sz, [u32, u32, u32]),
            "ghs_emst_device": (i32, [u32, u32, vp, vp, u32, u32, vp, vp, vp, vp, sz, vp, P(EmstResult)]),
            "ghs_emst_host": (i32, [u32, u32, vp, vp, u32, vp, vp, vp, P(EmstResult)]),
            "ghs_emst_rounds": (i32, [i32, u32, P(u32), P(ctypes.c_double), P(u32)]),
        }
        for name, (res, args) in sigs.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.ghs_abi_version() != ABI_VERSION:
            raise ImportError(f"libghs_mst.so ABI {L.ghs_abi_version()} != {ABI_VERSION}")
        _lib = L
        # a driver call with OPT_KEEP_CACHE leaves per-rank workspaces (and an RCCL clique) cached:
        # free them before the interpreter tears the HIP runtime down
        atexit.register(_release_at_exit)
        return _lib


def _release_at_exit():
    if _lib is not None:
        try:
            _lib.ghs_release_cache()
        except Exception:
            pass


def check(rc):
    """Raise GHSError for a negative return code (positive statuses are returned)."""
    if rc < GHS_OK:
        msg = load().ghs_last_error()
        raise GHSError(rc, msg.decode() if msg else "")
    return rc


GHS_COMM_ID_BYTES = 128  # include/ghs_mst.h


def comm_unique_id():
    """Rank 0's RCCL unique id (bytes) for ghs_comm_init on every rank."""
    buf = (ctypes.c_uint8 * GHS_COMM_ID_BYTES)()
    check(load().ghs_comm_unique_id(buf))
    return bytes(buf)


class Comm:
    """ghs_comm_t: one rank's RCCL communicator for ghs_solver_run (bound to the current device)."""

    def __init__(self, nranks, rank, uid):
        if len(uid) != GHS_COMM_ID_BYTES:
            raise ValueError("the unique id must be GHS_COMM_ID_BYTES bytes")
        buf = (ctypes.c_uint8 * GHS_COMM_ID_BYTES).from_buffer_copy(uid)
        h = ctypes.c_void_p(0)
        check(load().ghs_comm_init(int(nranks), int(rank), buf, ctypes.byref(h)))
        self.h = h
        self.nranks, self.rank = int(nranks), int(rank)

    def close(self):
        if self.h:
            load().ghs_comm_destroy(self.h)
            self.h = ctypes.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def release_cache():
    """Free the multi-rank drivers' cached per-rank state (ghs_release_cache)."""
    check(load().ghs_release_cache())


def slot_retries():
    """Round reports the host re-read because their checksum failed (seq landed before a field)."""
    c = ctypes.c_uint64(0)
    check(load().ghs_slot_retries(ctypes.byref(c)))
    return c.value


def device_count():
    c = ctypes.c_int(0)
    check(load().ghs_device_count(ctypes.byref(c)))
    return c.value


def require_gpu():
    """The product path runs only on a GPU: fail loudly, never fall back to the CPU."""
    if device_count() == 0:
        raise GHSError(GHS_E_NODEVICE, "no HIP device visible: the MST engine runs only on MI355X (gfx950)")
