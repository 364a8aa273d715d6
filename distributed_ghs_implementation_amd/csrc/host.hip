// Host-buffer entry point: GHSAlgorithm.run / MPI collect_results equivalent
// (ghs_implementation.py:442-490, ghs_implementation_mpi.py:673-779) for callers that hold the
// canonical edge list in host memory (the reference's own FFI-free Python flow, small graphs).
#include <hip/hip_runtime.h>

#include <string>

#include "common.h"

namespace {
struct DevBuf {
  void *p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};
}  // namespace

extern "C" int ghs_mst_host(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w,
                            uint8_t *in_mst, ghs_result_t *result, ghs_round_stats_t *stats) {
  if (m && (!u || !v || !w || !in_mst)) GHS_FAIL(GHS_E_ARG, "NULL host pointer");
  if (m >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "m must be < 2^31");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");
  // canonicity is validated on the device by the solve's first pass (k_select, GHS_E_NONCANON
  // before any id indexes an array): no serial host loop in front of the copy
  const size_t ws = ghs_workspace_bytes(n, m, m);
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t off_u = 0, off_v = off_u + al(m * 4), off_w = off_v + al(m * 4), off_mst = off_w + al(m * 4),
               off_ws = off_mst + al(m ? m : 1), total = off_ws + al(ws);
  DevBuf buf;
  GHS_HIP_CHECK(hipMalloc(&buf.p, total));
  char *b = (char *)buf.p;
  hipStream_t st = nullptr;
  if (m) {
    GHS_HIP_CHECK(hipMemcpyAsync(b + off_u, u, m * 4, hipMemcpyHostToDevice, st));
    GHS_HIP_CHECK(hipMemcpyAsync(b + off_v, v, m * 4, hipMemcpyHostToDevice, st));
    GHS_HIP_CHECK(hipMemcpyAsync(b + off_w, w, m * 4, hipMemcpyHostToDevice, st));
  }
  int rc = ghs_mst_device(n, m, (uint32_t *)(b + off_u), (uint32_t *)(b + off_v), (uint32_t *)(b + off_w), nullptr,
                          b + off_ws, ws, (uint8_t *)(b + off_mst), st, result, stats);
  if (rc) return rc;
  if (m) GHS_HIP_CHECK(hipMemcpy(in_mst, b + off_mst, m, hipMemcpyDeviceToHost));
  return GHS_OK;
}

// Host-buffer form of ghs_forest_labels_device (the nx.connected_components step a reference user runs
// on a result, check_mst.py:1-20): copy in, run, copy out.
extern "C" int ghs_forest_labels_host(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w,
                                      const uint8_t *in_mst, uint32_t mode, uint64_t param, uint32_t *labels,
                                      ghs_labels_result_t *result) {
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_labels_result_t{};
  result->cut_key = ~0ull;
  if (mode != GHS_CUT_NONE && mode != GHS_CUT_WEIGHT && mode != GHS_CUT_COUNT) GHS_FAIL(GHS_E_ARG, "unknown cut mode");
  if (mode == GHS_CUT_WEIGHT && param >= (1ull << 32)) GHS_FAIL(GHS_E_ARG, "GHS_CUT_WEIGHT: the threshold must be < 2^32");
  if (mode == GHS_CUT_COUNT && param == 0) GHS_FAIL(GHS_E_ARG, "GHS_CUT_COUNT: k must be >= 1");
  if (n == 0) {
    result->is_forest = 1;
    return GHS_OK;
  }
  if (m >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "m must be < 2^31");
  if (!labels || (m && (!u || !v || !w || !in_mst))) GHS_FAIL(GHS_E_ARG, "NULL host pointer");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");
  const size_t ws = m ? ghs_forest_labels_workspace_bytes(n, m) : 0;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t off_u = 0, off_v = off_u + al(m * 4), off_w = off_v + al(m * 4), off_f = off_w + al(m * 4),
               off_l = off_f + al(m ? m : 1), off_ws = off_l + al((size_t)n * 4), total = off_ws + al(ws ? ws : 1);
  DevBuf buf;
  GHS_HIP_CHECK(hipMalloc(&buf.p, total));
  char *b = (char *)buf.p;
  hipStream_t st = nullptr;
  if (m) {
    GHS_HIP_CHECK(hipMemcpyAsync(b + off_u, u, m * 4, hipMemcpyHostToDevice, st));
    GHS_HIP_CHECK(hipMemcpyAsync(b + off_v, v, m * 4, hipMemcpyHostToDevice, st));
    GHS_HIP_CHECK(hipMemcpyAsync(b + off_w, w, m * 4, hipMemcpyHostToDevice, st));
    GHS_HIP_CHECK(hipMemcpyAsync(b + off_f, in_mst, m, hipMemcpyHostToDevice, st));
  }
  int rc = ghs_forest_labels_device(n, m, (uint32_t *)(b + off_u), (uint32_t *)(b + off_v), (uint32_t *)(b + off_w),
                                    (uint8_t *)(b + off_f), mode, param, (uint32_t *)(b + off_l), b + off_ws, ws, st,
                                    result);
  if (rc) return rc;
  GHS_HIP_CHECK(hipMemcpy(labels, b + off_l, (size_t)n * 4, hipMemcpyDeviceToHost));
  return GHS_OK;
}

// Host-buffer form of ghs_forest_root_device (the in_branch pointers a reference node holds after a
// run, ghs_implementation.py:63,212): copy in, run, copy out.
extern "C" int ghs_forest_root_host(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint8_t *in_mst,
                                    uint32_t *parent, uint32_t *parent_eid, uint32_t *depth, uint32_t *pre,
                                    uint32_t *size, ghs_root_result_t *result) {
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_root_result_t{};
  if (n == 0) {
    result->is_forest = 1;
    return GHS_OK;
  }
  if (m >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "m must be < 2^31");
  if (!parent || !parent_eid || !depth || (m && (!u || !v || !in_mst))) GHS_FAIL(GHS_E_ARG, "NULL host pointer");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");
  const size_t ws = m ? ghs_forest_root_workspace_bytes(n, m) : 0;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t nb = al((size_t)n * 4);
  const size_t off_u = 0, off_v = off_u + al(m * 4), off_f = off_v + al(m * 4), off_o = off_f + al(m ? m : 1),
               off_ws = off_o + 5 * nb, total = off_ws + al(ws ? ws : 1);
  DevBuf buf;
  GHS_HIP_CHECK(hipMalloc(&buf.p, total));
  char *b = (char *)buf.p;
  hipStream_t st = nullptr;
  if (m) {
    GHS_HIP_CHECK(hipMemcpyAsync(b + off_u, u, m * 4, hipMemcpyHostToDevice, st));
    GHS_HIP_CHECK(hipMemcpyAsync(b + off_v, v, m * 4, hipMemcpyHostToDevice, st));
    GHS_HIP_CHECK(hipMemcpyAsync(b + off_f, in_mst, m, hipMemcpyHostToDevice, st));
  }
  uint32_t *d_out[5];
  for (int k = 0; k < 5; ++k) d_out[k] = (uint32_t *)(b + off_o + k * nb);
  int rc = ghs_forest_root_device(n, m, (uint32_t *)(b + off_u), (uint32_t *)(b + off_v), (uint8_t *)(b + off_f), d_out[0],
                                  d_out[1], d_out[2], pre ? d_out[3] : nullptr, size ? d_out[4] : nullptr, b + off_ws, ws,
                                  st, result);
  if (rc) return rc;
  uint32_t *h_out[5] = {parent, parent_eid, depth, pre, size};
  for (int k = 0; k < 5; ++k)
    if (h_out[k]) GHS_HIP_CHECK(hipMemcpy(h_out[k], d_out[k], (size_t)n * 4, hipMemcpyDeviceToHost));
  return GHS_OK;
}

// Host-buffer form of the path queries (what a reference user asks of a result by walking in_branch,
// ghs_implementation.py:235-387): copy in, root the flags, build the jump-pointer index, query, copy out.
extern "C" int ghs_forest_paths_host(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w,
                                     const uint8_t *in_mst, uint64_t q, const uint32_t *a, const uint32_t *b,
                                     uint64_t *key, uint32_t *lca, uint32_t *hops, ghs_paths_query_result_t *result) {
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_paths_query_result_t{};
  if (m >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "m must be < 2^31");
  if (q >= (1ull << 32)) GHS_FAIL(GHS_E_ARG, "q must be < 2^32");
  if ((m && (!u || !v || !w || !in_mst)) || (q && (!a || !b))) GHS_FAIL(GHS_E_ARG, "NULL host pointer");
  if (q == 0) return GHS_OK;
  result->queries = q;
  if (n == 0) GHS_FAIL(GHS_E_ARG, "vertex id out of range");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  hipStream_t st = nullptr;
  // stage 1: the edges, the flags, the rooted arrays, the rooting's workspace
  const size_t ws = m ? ghs_forest_root_workspace_bytes(n, m) : 0;
  const size_t nb = al((size_t)n * 4);
  const size_t off_u = 0, off_v = off_u + al(m * 4), off_w = off_v + al(m * 4), off_f = off_w + al(m * 4),
               off_o = off_f + al(m ? m : 1), off_ws = off_o + 3 * nb, total = off_ws + al(ws ? ws : 1);
  DevBuf buf;
  GHS_HIP_CHECK(hipMalloc(&buf.p, total));
  char *d = (char *)buf.p;
  if (m) {
    GHS_HIP_CHECK(hipMemcpyAsync(d + off_u, u, m * 4, hipMemcpyHostToDevice, st));
    GHS_HIP_CHECK(hipMemcpyAsync(d + off_v, v, m * 4, hipMemcpyHostToDevice, st));
    GHS_HIP_CHECK(hipMemcpyAsync(d + off_w, w, m * 4, hipMemcpyHostToDevice, st));
    GHS_HIP_CHECK(hipMemcpyAsync(d + off_f, in_mst, m, hipMemcpyHostToDevice, st));
  }
  uint32_t *d_par = (uint32_t *)(d + off_o), *d_peid = (uint32_t *)(d + off_o + nb), *d_dep = (uint32_t *)(d + off_o + 2 * nb);
  ghs_root_result_t rr;
  int rc = ghs_forest_root_device(n, m, (uint32_t *)(d + off_u), (uint32_t *)(d + off_v), (uint8_t *)(d + off_f), d_par,
                                  d_peid, d_dep, nullptr, nullptr, d + off_ws, ws, st, &rr);
  if (rc) return rc;
  if (!rr.is_forest) GHS_FAIL(GHS_E_ARG, "flags are not a forest");
  // stage 2: the index, the pairs, the answers
  const size_t ib = ghs_forest_paths_index_bytes(n, rr.max_depth);
  const size_t qb = al(q * 4);
  const size_t off_a = al(ib), off_b = off_a + qb, off_k = off_b + qb, off_l = off_k + al(q * 8), off_h = off_l + qb;
  DevBuf ibuf;
  GHS_HIP_CHECK(hipMalloc(&ibuf.p, off_h + qb));
  char *x = (char *)ibuf.p;
  GHS_HIP_CHECK(hipMemcpyAsync(x + off_a, a, q * 4, hipMemcpyHostToDevice, st));
  GHS_HIP_CHECK(hipMemcpyAsync(x + off_b, b, q * 4, hipMemcpyHostToDevice, st));
  ghs_paths_result_t pr;
  ghs_paths_t *h = nullptr;
  rc = ghs_forest_paths_create(n, m, (uint32_t *)(d + off_u), (uint32_t *)(d + off_v), (uint32_t *)(d + off_w), d_par, d_peid,
                               d_dep, rr.max_depth, x, ib, st, &pr, &h);
  if (rc) return rc;
  rc = ghs_forest_paths_query(h, q, (uint32_t *)(x + off_a), (uint32_t *)(x + off_b), key ? (uint64_t *)(x + off_k) : nullptr,
                              lca ? (uint32_t *)(x + off_l) : nullptr, hops ? (uint32_t *)(x + off_h) : nullptr, st, result);
  (void)ghs_forest_paths_destroy(h);
  if (rc) return rc;
  if (key) GHS_HIP_CHECK(hipMemcpy(key, x + off_k, q * 8, hipMemcpyDeviceToHost));
  if (lca) GHS_HIP_CHECK(hipMemcpy(lca, x + off_l, q * 4, hipMemcpyDeviceToHost));
  if (hops) GHS_HIP_CHECK(hipMemcpy(hops, x + off_h, q * 4, hipMemcpyDeviceToHost));
  return GHS_OK;
}

// Host-buffer form of the replacement edges (what a reference user asks when a link fails; the
// reference reruns the protocol, ghs_implementation.py:442-490): copy in, root the flags, build the
// jump-pointer index, replace, copy out. Public calls only.
extern "C" int ghs_forest_replace_host(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w,
                                       const uint8_t *in_mst, uint64_t *repl, uint32_t *repl_eid_by_edge,
                                       ghs_replace_result_t *result) {
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_replace_result_t{};
  result->best_out_eid = result->best_in_eid = 0xffffffffu;
  if (m >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "m must be < 2^31");
  if (m && (!u || !v || !w || !in_mst)) GHS_FAIL(GHS_E_ARG, "NULL host pointer");
  if (n == 0) return GHS_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  hipStream_t st = nullptr;
  // stage 1: the edges, the flags, the rooted arrays, the rooting's workspace
  const size_t ws = m ? ghs_forest_root_workspace_bytes(n, m) : 0;
  const size_t nb = al((size_t)n * 4);
  const size_t off_u = 0, off_v = off_u + al(m * 4), off_w = off_v + al(m * 4), off_f = off_w + al(m * 4),
               off_o = off_f + al(m ? m : 1), off_ws = off_o + 3 * nb, total = off_ws + al(ws ? ws : 1);
  DevBuf buf;
  GHS_HIP_CHECK(hipMalloc(&buf.p, total));
  char *d = (char *)buf.p;
  if (m) {
    GHS_HIP_CHECK(hipMemcpyAsync(d + off_u, u, m * 4, hipMemcpyHostToDevice, st));
    GHS_HIP_CHECK(hipMemcpyAsync(d + off_v, v, m * 4, hipMemcpyHostToDevice, st));
    GHS_HIP_CHECK(hipMemcpyAsync(d + off_w, w, m * 4, hipMemcpyHostToDevice, st));
    GHS_HIP_CHECK(hipMemcpyAsync(d + off_f, in_mst, m, hipMemcpyHostToDevice, st));
  }
  uint32_t *d_u = (uint32_t *)(d + off_u), *d_v = (uint32_t *)(d + off_v), *d_w = (uint32_t *)(d + off_w);
  uint32_t *d_par = (uint32_t *)(d + off_o), *d_peid = (uint32_t *)(d + off_o + nb), *d_dep = (uint32_t *)(d + off_o + 2 * nb);
  ghs_root_result_t rr;
  int rc = ghs_forest_root_device(n, m, d_u, d_v, (uint8_t *)(d + off_f), d_par, d_peid, d_dep, nullptr, nullptr, d + off_ws,
                                  ws, st, &rr);
  if (rc) return rc;
  if (!rr.is_forest) GHS_FAIL(GHS_E_ARG, "flags are not a forest");
  // stage 2: the index, the cover levels, the answers
  const size_t ib = ghs_forest_paths_index_bytes(n, rr.max_depth), rb = ghs_forest_replace_workspace_bytes(n, rr.max_depth);
  const size_t off_rws = al(ib), off_r = off_rws + al(rb), off_e = off_r + al((size_t)n * 8);
  DevBuf ibuf;
  GHS_HIP_CHECK(hipMalloc(&ibuf.p, off_e + al(m ? m * 4 : 1)));
  char *x = (char *)ibuf.p;
  ghs_paths_result_t pr;
  ghs_paths_t *h = nullptr;
  rc = ghs_forest_paths_create(n, m, d_u, d_v, d_w, d_par, d_peid, d_dep, rr.max_depth, x, ib, st, &pr, &h);
  if (rc) return rc;
  rc = ghs_forest_replace_device(h, m, d_u, d_v, d_w, (uint64_t *)(x + off_r),
                                 repl_eid_by_edge && m ? (uint32_t *)(x + off_e) : nullptr, x + off_rws, rb, st, result);
  (void)ghs_forest_paths_destroy(h);
  if (rc) return rc;
  if (repl) GHS_HIP_CHECK(hipMemcpy(repl, x + off_r, (size_t)n * 8, hipMemcpyDeviceToHost));
  if (repl_eid_by_edge && m) GHS_HIP_CHECK(hipMemcpy(repl_eid_by_edge, x + off_e, m * 4, hipMemcpyDeviceToHost));
  return GHS_OK;
}

// Host-buffer forms of the tree distances (a reference user would walk in_branch edge by edge and add
// the weights up, ghs_implementation.py:63,212): copy in, root the flags, build the jump-pointer index
// and the weighted depth, answer, copy out. Public calls only.
namespace {
// what both forms share: the edges and flags on the device, the rooted arrays, the index, the weighted depth
struct DistStage {
  DevBuf buf, ibuf;
  ghs_paths_t *h = nullptr;
  uint64_t *d_wd = nullptr;
  char *extra = nullptr;  // extra_bytes for the caller, 256-byte aligned
  void *d_ws = nullptr;   // the dist workspace (scratch again after run)
  size_t ws_bytes = 0;
  ~DistStage() { (void)ghs_forest_paths_destroy(h); }
  int run(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w, const uint8_t *in_mst,
          uint32_t metric, size_t extra_bytes, hipStream_t st) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t ws = m ? ghs_forest_root_workspace_bytes(n, m) : 0;
    const size_t nb = al((size_t)n * 4);
    const size_t off_u = 0, off_v = off_u + al(m * 4), off_w = off_v + al(m * 4), off_f = off_w + al(m * 4),
                 off_o = off_f + al(m ? m : 1), off_ws = off_o + 3 * nb, total = off_ws + al(ws ? ws : 1);
    GHS_HIP_CHECK(hipMalloc(&buf.p, total));
    char *d = (char *)buf.p;
    if (m) {
      GHS_HIP_CHECK(hipMemcpyAsync(d + off_u, u, m * 4, hipMemcpyHostToDevice, st));
      GHS_HIP_CHECK(hipMemcpyAsync(d + off_v, v, m * 4, hipMemcpyHostToDevice, st));
      GHS_HIP_CHECK(hipMemcpyAsync(d + off_w, w, m * 4, hipMemcpyHostToDevice, st));
      GHS_HIP_CHECK(hipMemcpyAsync(d + off_f, in_mst, m, hipMemcpyHostToDevice, st));
    }
    uint32_t *d_u = (uint32_t *)(d + off_u), *d_v = (uint32_t *)(d + off_v), *d_w = (uint32_t *)(d + off_w);
    uint32_t *d_par = (uint32_t *)(d + off_o), *d_peid = (uint32_t *)(d + off_o + nb), *d_dep = (uint32_t *)(d + off_o + 2 * nb);
    ghs_root_result_t rr;
    int rc = ghs_forest_root_device(n, m, d_u, d_v, (uint8_t *)(d + off_f), d_par, d_peid, d_dep, nullptr, nullptr, d + off_ws,
                                    ws, st, &rr);
    if (rc) return rc;
    if (!rr.is_forest) GHS_FAIL(GHS_E_ARG, "flags are not a forest");
    const size_t ib = ghs_forest_paths_index_bytes(n, rr.max_depth);
    ws_bytes = ghs_forest_dist_workspace_bytes(n, rr.max_depth);
    const size_t off_dws = al(ib), off_wd = off_dws + al(ws_bytes), off_x = off_wd + al((size_t)n * 8);
    GHS_HIP_CHECK(hipMalloc(&ibuf.p, off_x + al(extra_bytes ? extra_bytes : 1)));
    char *x = (char *)ibuf.p;
    ghs_paths_result_t pr;
    rc = ghs_forest_paths_create(n, m, d_u, d_v, d_w, d_par, d_peid, d_dep, rr.max_depth, x, ib, st, &pr, &h);
    if (rc) return rc;
    d_ws = x + off_dws;
    d_wd = (uint64_t *)(x + off_wd);
    extra = x + off_x;
    return ghs_forest_wdepth_device(h, metric, d_wd, d_ws, ws_bytes, st);
  }
};
}  // namespace

extern "C" int ghs_forest_dist_host(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w,
                                    const uint8_t *in_mst, uint32_t metric, uint64_t q, const uint32_t *a, const uint32_t *b,
                                    uint64_t *dist, uint32_t *lca, ghs_dist_query_result_t *result) {
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_dist_query_result_t{};
  if (metric != GHS_DIST_WEIGHT && metric != GHS_DIST_HOPS) GHS_FAIL(GHS_E_ARG, "unknown metric");
  if (m >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "m must be < 2^31");
  if (q >= (1ull << 32)) GHS_FAIL(GHS_E_ARG, "q must be < 2^32");
  if ((m && (!u || !v || !w || !in_mst)) || (q && (!a || !b))) GHS_FAIL(GHS_E_ARG, "NULL host pointer");
  if (q == 0) return GHS_OK;
  result->queries = q;
  if (n == 0) GHS_FAIL(GHS_E_ARG, "vertex id out of range");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  hipStream_t st = nullptr;
  const size_t qb = al(q * 4);
  const size_t off_a = 0, off_b = off_a + qb, off_d = off_b + qb, off_l = off_d + al(q * 8);
  DistStage s;
  if (int rc = s.run(n, m, u, v, w, in_mst, metric, off_l + qb, st)) return rc;
  char *x = s.extra;
  GHS_HIP_CHECK(hipMemcpyAsync(x + off_a, a, q * 4, hipMemcpyHostToDevice, st));
  GHS_HIP_CHECK(hipMemcpyAsync(x + off_b, b, q * 4, hipMemcpyHostToDevice, st));
  int rc = ghs_forest_dist_query(s.h, s.d_wd, q, (uint32_t *)(x + off_a), (uint32_t *)(x + off_b), (uint64_t *)(x + off_d),
                                 lca ? (uint32_t *)(x + off_l) : nullptr, result, st);
  if (rc) return rc;
  if (dist) GHS_HIP_CHECK(hipMemcpy(dist, x + off_d, q * 8, hipMemcpyDeviceToHost));
  if (lca) GHS_HIP_CHECK(hipMemcpy(lca, x + off_l, q * 4, hipMemcpyDeviceToHost));
  return GHS_OK;
}

extern "C" int ghs_forest_diameter_host(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w,
                                        const uint8_t *in_mst, uint32_t metric, uint32_t *root_of, uint64_t *diam,
                                        uint32_t *end_a, uint32_t *end_b, uint64_t *ecc, ghs_diameter_result_t *result) {
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_diameter_result_t{};
  result->max_root = result->center = 0xffffffffu;
  if (metric != GHS_DIST_WEIGHT && metric != GHS_DIST_HOPS) GHS_FAIL(GHS_E_ARG, "unknown metric");
  if (m >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "m must be < 2^31");
  if (m && (!u || !v || !w || !in_mst)) GHS_FAIL(GHS_E_ARG, "NULL host pointer");
  if (n == 0) return GHS_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  hipStream_t st = nullptr;
  const size_t nb4 = al((size_t)n * 4), nb8 = al((size_t)n * 8);
  const size_t off_r = 0, off_a = off_r + nb4, off_b = off_a + nb4, off_d = off_b + nb4, off_e = off_d + nb8;
  DistStage s;
  if (int rc = s.run(n, m, u, v, w, in_mst, metric, off_e + nb8, st)) return rc;
  char *x = s.extra;
  int rc = ghs_forest_diameter_device(s.h, s.d_wd, (uint32_t *)(x + off_r), (uint64_t *)(x + off_d), (uint32_t *)(x + off_a),
                                      (uint32_t *)(x + off_b), ecc ? (uint64_t *)(x + off_e) : nullptr, s.d_ws, s.ws_bytes,
                                      result, st);
  if (rc) return rc;
  if (root_of) GHS_HIP_CHECK(hipMemcpy(root_of, x + off_r, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (diam) GHS_HIP_CHECK(hipMemcpy(diam, x + off_d, (size_t)n * 8, hipMemcpyDeviceToHost));
  if (end_a) GHS_HIP_CHECK(hipMemcpy(end_a, x + off_a, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (end_b) GHS_HIP_CHECK(hipMemcpy(end_b, x + off_b, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (ecc) GHS_HIP_CHECK(hipMemcpy(ecc, x + off_e, (size_t)n * 8, hipMemcpyDeviceToHost));
  return GHS_OK;
}
