// Host-buffer entry point: GHSAlgorithm.run / MPI collect_results equivalent
// (ghs_implementation.py:442-490, ghs_implementation_mpi.py:673-779) for callers that hold the
// canonical edge list in host memory (the reference's own FFI-free Python flow, small graphs).
#include <hip/hip_runtime.h>

#include <string>

#include "common.h"

using ghs::Staging;

extern "C" int ghs_mst_host(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w,
                            uint8_t *in_mst, ghs_result_t *result, ghs_round_stats_t *stats) {
  if (m && (!u || !v || !w || !in_mst)) GHS_FAIL(GHS_E_ARG, "NULL host pointer");
  if (m >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "m must be < 2^31");
  if (int e = ghs::require_device()) return e;
  // canonicity is validated on the device by the solve's first pass (k_select, GHS_E_NONCANON
  // before any id indexes an array): no serial host loop in front of the copy
  const size_t ws = ghs_workspace_bytes(n, m, m);
  Staging s;
  const auto d_u = s.take<uint32_t>(m), d_v = s.take<uint32_t>(m), d_w = s.take<uint32_t>(m);
  const auto d_mst = s.take<uint8_t>(m);
  const auto d_ws = s.take<char>(ws);
  GHS_HIP_CHECK(s.alloc());
  hipStream_t st = nullptr;
  GHS_HIP_CHECK(s.up(d_u, u, st));
  GHS_HIP_CHECK(s.up(d_v, v, st));
  GHS_HIP_CHECK(s.up(d_w, w, st));
  int rc = ghs_mst_device(n, m, s.at(d_u), s.at(d_v), s.at(d_w), nullptr, s.at(d_ws), ws, s.at(d_mst), st, result, stats);
  if (rc) return rc;
  GHS_HIP_CHECK(s.down(in_mst, d_mst, m));
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
  if (int e = ghs::require_device()) return e;
  const size_t ws = m ? ghs_forest_labels_workspace_bytes(n, m) : 0;
  Staging s;
  const auto d_u = s.take<uint32_t>(m), d_v = s.take<uint32_t>(m), d_w = s.take<uint32_t>(m);
  const auto d_f = s.take<uint8_t>(m);
  const auto d_l = s.take<uint32_t>(n);
  const auto d_ws = s.take<char>(ws);
  GHS_HIP_CHECK(s.alloc());
  hipStream_t st = nullptr;
  GHS_HIP_CHECK(s.up(d_u, u, st));
  GHS_HIP_CHECK(s.up(d_v, v, st));
  GHS_HIP_CHECK(s.up(d_w, w, st));
  GHS_HIP_CHECK(s.up(d_f, in_mst, st));
  int rc = ghs_forest_labels_device(n, m, s.at(d_u), s.at(d_v), s.at(d_w), s.at(d_f), mode, param, s.at(d_l), s.at(d_ws), ws,
                                    st, result);
  if (rc) return rc;
  GHS_HIP_CHECK(s.down(labels, d_l, n));
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
  if (int e = ghs::require_device()) return e;
  const size_t ws = m ? ghs_forest_root_workspace_bytes(n, m) : 0;
  Staging s;
  const auto d_u = s.take<uint32_t>(m), d_v = s.take<uint32_t>(m);
  const auto d_f = s.take<uint8_t>(m);
  uint32_t *h_out[5] = {parent, parent_eid, depth, pre, size};
  Staging::Piece<uint32_t> d_out[5];
  for (auto &p : d_out) p = s.take<uint32_t>(n);
  const auto d_ws = s.take<char>(ws);
  GHS_HIP_CHECK(s.alloc());
  hipStream_t st = nullptr;
  GHS_HIP_CHECK(s.up(d_u, u, st));
  GHS_HIP_CHECK(s.up(d_v, v, st));
  GHS_HIP_CHECK(s.up(d_f, in_mst, st));
  int rc = ghs_forest_root_device(n, m, s.at(d_u), s.at(d_v), s.at(d_f), s.at(d_out[0]), s.at(d_out[1]), s.at(d_out[2]),
                                  s.at(d_out[3], pre), s.at(d_out[4], size), s.at(d_ws), ws, st, result);
  if (rc) return rc;
  for (int k = 0; k < 5; ++k) GHS_HIP_CHECK(s.down(h_out[k], d_out[k], n));
  return GHS_OK;
}

namespace {
// What the path, replacement and distance forms share. root(): the edges and the flags on the device,
// the flags rooted (ghs_forest_root_device without pre and size; flags that close a cycle are refused),
// the index as the first piece of a second buffer, `ix`. The form then takes its own pieces from ix, and
// index() allocates ix and builds the jump-pointer index. Public calls only.
struct Rooted {
  Staging in, ix;
  Staging::Piece<uint32_t> u, v, w, parent, parent_eid, depth;
  Staging::Piece<char> levels;
  uint32_t n = 0;
  uint64_t m = 0, max_depth = 0;
  ghs_paths_t *h = nullptr;
  ~Rooted() { (void)ghs_forest_paths_destroy(h); }
  int root(uint32_t n_, uint64_t m_, const uint32_t *h_u, const uint32_t *h_v, const uint32_t *h_w, const uint8_t *in_mst,
           hipStream_t st) {
    n = n_, m = m_;
    const size_t ws = m ? ghs_forest_root_workspace_bytes(n, m) : 0;
    u = in.take<uint32_t>(m), v = in.take<uint32_t>(m), w = in.take<uint32_t>(m);
    const auto f = in.take<uint8_t>(m);
    parent = in.take<uint32_t>(n), parent_eid = in.take<uint32_t>(n), depth = in.take<uint32_t>(n);
    const auto d_ws = in.take<char>(ws);
    GHS_HIP_CHECK(in.alloc());
    GHS_HIP_CHECK(in.up(u, h_u, st));
    GHS_HIP_CHECK(in.up(v, h_v, st));
    GHS_HIP_CHECK(in.up(w, h_w, st));
    GHS_HIP_CHECK(in.up(f, in_mst, st));
    ghs_root_result_t rr;
    int rc = ghs_forest_root_device(n, m, in.at(u), in.at(v), in.at(f), in.at(parent), in.at(parent_eid), in.at(depth),
                                    nullptr, nullptr, in.at(d_ws), ws, st, &rr);
    if (rc) return rc;
    if (!rr.is_forest) GHS_FAIL(GHS_E_ARG, "flags are not a forest");
    max_depth = rr.max_depth;
    levels = ix.take<char>(ghs_forest_paths_index_bytes(n, max_depth));
    return GHS_OK;
  }
  int index(hipStream_t st) {
    GHS_HIP_CHECK(ix.alloc());
    ghs_paths_result_t pr;
    return ghs_forest_paths_create(n, m, in.at(u), in.at(v), in.at(w), in.at(parent), in.at(parent_eid), in.at(depth),
                                   max_depth, ix.at(levels), levels.count, st, &pr, &h);
  }
};
}  // namespace

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
  if (int e = ghs::require_device()) return e;
  hipStream_t st = nullptr;
  Rooted s;
  if (int rc = s.root(n, m, u, v, w, in_mst, st)) return rc;
  // next to the index: the pairs, the answers
  const auto d_a = s.ix.take<uint32_t>(q), d_b = s.ix.take<uint32_t>(q);
  const auto d_k = s.ix.take<uint64_t>(q);
  const auto d_l = s.ix.take<uint32_t>(q), d_h = s.ix.take<uint32_t>(q);
  if (int rc = s.index(st)) return rc;
  GHS_HIP_CHECK(s.ix.up(d_a, a, st));
  GHS_HIP_CHECK(s.ix.up(d_b, b, st));
  int rc = ghs_forest_paths_query(s.h, q, s.ix.at(d_a), s.ix.at(d_b), s.ix.at(d_k, key), s.ix.at(d_l, lca), s.ix.at(d_h, hops),
                                  st, result);
  if (rc) return rc;
  GHS_HIP_CHECK(s.ix.down(key, d_k, q));
  GHS_HIP_CHECK(s.ix.down(lca, d_l, q));
  GHS_HIP_CHECK(s.ix.down(hops, d_h, q));
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
  if (int e = ghs::require_device()) return e;
  hipStream_t st = nullptr;
  Rooted s;
  if (int rc = s.root(n, m, u, v, w, in_mst, st)) return rc;
  // next to the index: the cover levels, the answers
  const size_t rb = ghs_forest_replace_workspace_bytes(n, s.max_depth);
  const auto d_ws = s.ix.take<char>(rb);
  const auto d_r = s.ix.take<uint64_t>(n);
  const auto d_e = s.ix.take<uint32_t>(m);
  if (int rc = s.index(st)) return rc;
  int rc = ghs_forest_replace_device(s.h, m, s.in.at(s.u), s.in.at(s.v), s.in.at(s.w), s.ix.at(d_r),
                                     s.ix.at(d_e, m ? repl_eid_by_edge : nullptr), s.ix.at(d_ws), rb, st, result);
  if (rc) return rc;
  GHS_HIP_CHECK(s.ix.down(repl, d_r, n));
  GHS_HIP_CHECK(s.ix.down(repl_eid_by_edge, d_e, m));
  return GHS_OK;
}

// Host-buffer forms of the tree distances (a reference user would walk in_branch edge by edge and add
// the weights up, ghs_implementation.py:63,212): copy in, root the flags, build the jump-pointer index
// and the weighted depth, answer, copy out. Public calls only.
namespace {
// what both forms share on top of the rooted stage: the dist workspace and the weighted depth next to the index
struct DistStage : Rooted {
  Staging::Piece<char> ws;  // the dist workspace (scratch again after depths())
  Staging::Piece<uint64_t> wdepth;
  // root(), then the form's own pieces from ix, then depths()
  int depths(uint32_t metric, hipStream_t st) {
    ws = ix.take<char>(ghs_forest_dist_workspace_bytes(n, max_depth));
    wdepth = ix.take<uint64_t>(n);
    if (int rc = index(st)) return rc;
    return ghs_forest_wdepth_device(h, metric, ix.at(wdepth), ix.at(ws), ws.count, st);
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
  if (int e = ghs::require_device()) return e;
  hipStream_t st = nullptr;
  DistStage s;
  if (int rc = s.root(n, m, u, v, w, in_mst, st)) return rc;
  const auto d_a = s.ix.take<uint32_t>(q), d_b = s.ix.take<uint32_t>(q);
  const auto d_d = s.ix.take<uint64_t>(q);
  const auto d_l = s.ix.take<uint32_t>(q);
  if (int rc = s.depths(metric, st)) return rc;
  GHS_HIP_CHECK(s.ix.up(d_a, a, st));
  GHS_HIP_CHECK(s.ix.up(d_b, b, st));
  int rc = ghs_forest_dist_query(s.h, s.ix.at(s.wdepth), q, s.ix.at(d_a), s.ix.at(d_b), s.ix.at(d_d), s.ix.at(d_l, lca), result,
                                 st);
  if (rc) return rc;
  GHS_HIP_CHECK(s.ix.down(dist, d_d, q));
  GHS_HIP_CHECK(s.ix.down(lca, d_l, q));
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
  if (int e = ghs::require_device()) return e;
  hipStream_t st = nullptr;
  DistStage s;
  if (int rc = s.root(n, m, u, v, w, in_mst, st)) return rc;
  const auto d_r = s.ix.take<uint32_t>(n), d_a = s.ix.take<uint32_t>(n), d_b = s.ix.take<uint32_t>(n);
  const auto d_d = s.ix.take<uint64_t>(n), d_e = s.ix.take<uint64_t>(n);
  if (int rc = s.depths(metric, st)) return rc;
  int rc = ghs_forest_diameter_device(s.h, s.ix.at(s.wdepth), s.ix.at(d_r), s.ix.at(d_d), s.ix.at(d_a), s.ix.at(d_b),
                                      s.ix.at(d_e, ecc), s.ix.at(s.ws), s.ws.count, result, st);
  if (rc) return rc;
  GHS_HIP_CHECK(s.ix.down(root_of, d_r, n));
  GHS_HIP_CHECK(s.ix.down(diam, d_d, n));
  GHS_HIP_CHECK(s.ix.down(end_a, d_a, n));
  GHS_HIP_CHECK(s.ix.down(end_b, d_b, n));
  GHS_HIP_CHECK(s.ix.down(ecc, d_e, n));
  return GHS_OK;
}
