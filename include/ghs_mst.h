/*
 * ghs_mst.h — C-ABI of the MI355X-native MST engine (libghs_mst.so).
 *
 * The reference (Trisanu-007/Distributed_GHS_Implementation) computes an MST with the GHS
 * message protocol: one Python thread (ghs_implementation.py:46-413) or one MPI rank
 * (ghs_implementation_mpi.py:37-757) per vertex exchanging CONNECT/INITIATE/TEST/ACCEPT/
 * REJECT/REPORT/CHANGEROOT. It has no FFI; its path sits behind two call surfaces:
 *   (1) GHSAlgorithm(num_nodes, edges).run(timeout) -> [(u, v)]   ghs_implementation.py:417-490
 *   (2) MPINode(...).run() + collect_results() -> [(u, v, w)]       ghs_implementation_mpi.py:673-779
 * This library replaces the protocol with a level-synchronous Boruvka fragment contraction
 * (one GHS level == one Boruvka round) in hand-written gfx950 HIP kernels. Every entry point
 * below names the reference interface it stands in for. Conventions:
 *   - all functions return GHS_OK (0) or a negative GHS_E_* code and never abort;
 *     ghs_last_error() returns a thread-local message for the last failure;
 *   - "canonical edge list": u[e] < v[e] < n, strictly ascending (u, v), no duplicates;
 *     eid = e. Size limits: m < 2^31 (edge ids are 32-bit inside the 64-bit keys and the
 *     kernels' byte offsets) and n <= 2^32 - 1 (ids < n, so 0xffffffff never names a vertex
 *     and marks dead entries); every entry point that takes m returns GHS_E_ARG past the cap. Ties resolve under the strict key (w, u, v) == (w, eid) — the order in which
 *     NetworkX Kruskal (the reference's verifier, ghs_implementation.py:746) visits edges on a
 *     canonically built graph. The result is a minimum spanning FOREST.
 *   - d_* pointers are device pointers (HIP / torch device memory) on the current device;
 *     `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - 64-bit keys: key = (uint64)w << 32 | eid; UINT64_MAX = "no outgoing edge" (the
 *     reference's best_weight = float('inf'), ghs_implementation.py:61).
 */
#ifndef GHS_MST_H
#define GHS_MST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GHS_MST_ABI_VERSION 10

#define GHS_OK 0
#define GHS_NEED_EXCHANGE 1   /* ghs_solver_minedge on a multi-rank solver opened a level: OR-combine
                                 the level's fragment flags across ranks, then call it again */
#define GHS_E_ARG (-1)        /* bad argument (null pointer, size, alignment) */
#define GHS_E_NONCANON (-2)   /* input edge list is not canonical */
#define GHS_E_HIP (-3)        /* HIP runtime error */
#define GHS_E_ROUNDCAP (-4)   /* round cap exceeded (never expected: hang guard) */
#define GHS_E_NODEVICE (-5)   /* no usable gfx950 device */
#define GHS_E_NOMEM (-6)      /* workspace too small / allocation failed */
#define GHS_E_STATE (-7)      /* solver handle used out of order */

#define GHS_MAX_ROUND_STATS 64
#define GHS_MAX_RANKS 64       /* ranks of one multi-rank solve (ghs_config_t.num_ranks, communicators) */

/* Per-round record (one Boruvka round == one GHS level of the reference). */
typedef struct ghs_round_stats {
  uint32_t level;             /* weight level this round belongs to */
  uint32_t reserved;
  uint64_t level_arcs;        /* first round of a level: arcs built for the level, else 0 */
  uint64_t live_arcs;         /* arcs scanned by the min-edge kernel this round */
  uint64_t active_components; /* fragments that searched for an outgoing edge */
  uint64_t hooks;             /* fragments that merged (== MST edges added) */
  float ms_minedge;           /* min-outgoing-edge (+ fused compaction) kernel */
  float ms_hook;              /* hook (CONNECT) kernel */
  float ms_jump;              /* pointer-jump relabel (INITIATE) kernel */
  float ms_active;            /* next-fragment-list compaction */
} ghs_round_stats_t;

typedef struct ghs_result {
  uint64_t num_mst_edges;     /* n - (#components) */
  uint64_t total_weight;      /* sum of w over MST edges */
  uint32_t rounds;            /* Boruvka rounds executed (all levels) */
  uint32_t num_stats;         /* entries filled in the stats array (<= GHS_MAX_ROUND_STATS) */
  uint32_t levels;            /* weight levels planned */
  uint32_t pass_flags;        /* bit 0: the solve ran bucketed rounds (k_bucket / k_bmin);
                                 bit 1: the plan's span sample found the graph lattice-like;
                                 bit 2: level 0's round 0 ran windowed (k_wmin over the edge list;
                                 unset when k_select's span flag sent it to k_bucket / k_bmin);
                                 bit 3: a level finished in the LDS tail (k_tail_*) */
  double ms_total;            /* host wall time of the solve (device-resident input -> flags) */
  /* The two full streams over the canonical list (HIP events on the solve's stream). */
  float ms_select;            /* k_select: validation + level-0 split */
  float ms_filter;            /* k_filter: giant-bitmap filter + level-1 split (0 if not run) */
  uint64_t canon_edges;       /* canonical edges each pass streams (the solver's range) */
  uint64_t select_out;        /* entries k_select wrote (level-0 edges, incl. region padding) */
  uint64_t filter_out;        /* entries k_filter wrote (level-1 + pending edges, incl. padding) */
  /* ABI 7: host-side phases of the multi-rank drivers (ghs_mst_multi / ghs_mst_emulated; 0
     elsewhere), the maximum over the ranks: setup (stream, workspace, H2D copy, solver creation,
     agreement), the ghs_solver_run loop, the flags' D2H gather. reused = 1 when the call ran on
     the rank state cached by an earlier call of the same shape (no hipMalloc, no RCCL init). */
  double ms_setup;
  double ms_solve;
  double ms_gather;
  uint32_t reused;
  uint32_t reserved;
} ghs_result_t;

/* Weight-level plan of the filter. Level 1 holds roughly the
 * level1_edges_per_vertex * n lightest edges, each further level level_growth times more, the
 * last level the rest; max_levels = 1 runs plain Boruvka over every edge at once. Thresholds
 * are weight quantiles of a fixed sample of the canonical list, so every rank plans the same
 * levels. level1_edges_per_vertex <= 0 (the default) = auto: 0.5 when m >= 4n, else 1.2.
 * Results do not depend on the plan (only speed does).
 * ABI 5: every path option lives here (the library reads no environment variable that changes the
 * algorithm or a launch shape); options = 0 and dedup_max = 0 select the default path. */
#define GHS_OPT_NO_SEED_RUNS 0x1u  /* level 0, round 0: a-side minima through the min-edge kernel
                                      instead of the single-writer run seeding */
#define GHS_OPT_NO_DENSE 0x2u      /* several ranks: levels in vertex labels, not dense labels */
#define GHS_OPT_BUCKETED 0x4u      /* one rank: every round bucketed, whatever the graph (default:
                                      a lattice-like graph's level-0 rounds with >= 2^23 active
                                      fragments, another graph's first round of every level —
                                      decided from the plan's span sample; tests force it) */
#define GHS_OPT_NO_BUCKETED 0x8u   /* one rank: never bucketed rounds */
#define GHS_OPT_DEBUG 0x10u        /* per-level sizes on stderr (diagnostic) */
#define GHS_OPT_TIME_ROUNDS 0x20u  /* HIP events around the compacting min-edge launches
                                      (ghs_round_stats_t.ms_minedge; idles the GPU ~6 us each) */
#define GHS_OPT_DETAIL 0x40u       /* HIP events around every stage of every round (diagnostic) */
#define GHS_OPT_NO_WINDOW 0x100u   /* one rank, lattice-like: level 0 round 0 through k_bucket / k_bmin
                                      records instead of the windowed k_wmin over the edge list */
#define GHS_OPT_BUCKETED_FIRST 0x80u /* one rank: bucketed first rounds of every level (whatever the
                                        graph), the other rounds unbucketed */
#define GHS_OPT_NO_TAIL 0x200u     /* one rank: no LDS tail — every round of a level through the
                                      per-round kernels (default: once a level's active fragments fit
                                      the tail's LDS, its remaining rounds run in k_tail_*) */
/* ABI 8 */
#define GHS_OPT_CHECK_TOTALS 0x400u /* one rank: at the end of every level the device counters are copied
                                       behind the level's last kernel (stream-ordered) and compared with
                                       the totals of the level's last round report (GHS_E_STATE if they
                                       differ); the solve's totals then come from that copy (test /
                                       diagnostic: one host sync per level) */
#define GHS_OPT_KEEP_CACHE 0x800u  /* ghs_mst_multi / ghs_mst_emulated: keep the per-rank state for the
                                      next call of the same shape (default: freed when the call returns;
                                      see ghs_release_cache) */
typedef struct ghs_config {
  uint32_t max_levels;
  uint32_t num_ranks;         /* ranks sharing the solve (1 = single GPU; >1: identical rounds on
                                 every rank, so empty levels are not skipped) */
  double level1_edges_per_vertex;
  double level_growth;
  uint32_t options;           /* GHS_OPT_* bits (0 = default path) */
  uint32_t dedup_max;         /* cross-component parallel-edge filter in the compacting rounds once
                                 at most this many fragments are active (0 = off, the default) */
  uint32_t fault_rank;        /* test hook of the multi-rank drivers: 1 + the rank whose setup is
                                 made to fail (ghs_mst_multi / ghs_mst_emulated); 0 = none */
  uint32_t fault_round;       /* ABI 7 test hook: with fault_rank set, that rank fails in the round
                                 loop (ghs_solver_run) once it has completed this many rounds instead
                                 of at setup; 0 = the setup failure above. ABI 8: GHS_E_ARG with
                                 num_ranks == 1 (a one-rank loop has no exchange to fail in) */
} ghs_config_t;

/* ---- library / device ------------------------------------------------------------------- */
int ghs_abi_version(void);
const char *ghs_last_error(void);
/* number of visible HIP devices (0 on a host without GPU; never an error) */
int ghs_device_count(int *count);

/* ---- host-buffer convenience -------------------------------------------------------------
 * Replaces GHSAlgorithm.run (ghs_implementation.py:442-490: starts n threads, polls
 * termination, sweeps BRANCH edges) and MPINode.run + collect_results
 * (ghs_implementation_mpi.py:673-779). Input: canonical edge list on the HOST. Output:
 * in_mst[e] = 1 iff canonical edge e is in the MSF (m bytes, host). Copies in/out, runs on the
 * current device, serialised per process. stats may be NULL (else GHS_MAX_ROUND_STATS entries). */
int ghs_mst_host(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w,
                 uint8_t *in_mst, ghs_result_t *result, ghs_round_stats_t *stats);

/* ---- one process, several GPUs ------------------------------------------------------------
 * Replaces the MPI path as ONE call (ghs_implementation_mpi.py:884-954: mpiexec with one rank per
 * vertex, pickled p2p messages, Barrier, gather of the BRANCH edges to rank 0 at :760-779):
 * num_gpus devices of this node (devices: their HIP ids, NULL = 0..num_gpus-1, distinct) form an
 * RCCL clique (ncclCommInitAll); one host thread per device copies the canonical list (host
 * arrays, as ghs_mst_host) to its device and runs the stepwise solver below over its own edge
 * range [r*m/N, (r+1)*m/N) (4-aligned), with the round's collectives over RCCL (all-gather of the
 * level-flag bitmaps, int64 MIN of the best keys, int32 MAX of the owner-computed hooks). in_mst
 * (host, m bytes) = the devices' own-range flags; result/stats are device 0's (the totals are
 * checked equal on every device). cfg may be NULL (defaults; num_ranks is set to num_gpus).
 * An input error (non-canonical list) fails the call on every device together (the error byte
 * of the flag exchange); a device fault (GHS_E_HIP) is not recoverable. */
int ghs_mst_multi(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w,
                  int num_gpus, const int *devices, const ghs_config_t *cfg, uint8_t *in_mst,
                  ghs_result_t *result, ghs_round_stats_t *stats);
/* ABI 7/8: with GHS_OPT_KEEP_CACHE the multi-rank drivers (ghs_mst_multi, ghs_mst_emulated) keep
 * their per-rank state — streams, workspaces, replicated canonical copies, pinned report rings,
 * collective scratch, and ghs_mst_multi's RCCL clique — in one process-wide cache keyed by (driver,
 * devices, ranks, n, m); a later call of the same shape allocates nothing (ghs_result_t.reused = 1),
 * a call of another shape or a failed call frees it first. Without the option (ABI 8 default) a
 * call frees its state before returning. ghs_release_cache frees it now (device memory back to the
 * caller; safe to call at any time outside a driver call), and (ABI 9) ghs_flags_to_eids' cached
 * temporary storage with it. */
int ghs_release_cache(void);
/* ABI 8: the MSF edge ids of the flag range [lo, hi) in order — d_eids[k] = the k-th e with
 * d_in_mst[e] != 0 (uint32; room for `capacity` ids), *count (host) = how many — on the device
 * (a flagged select), the form a rank's own-range MSF is gathered in (the reference's
 * collect_results, ghs_implementation_mpi.py:760-779). Returns once *count is known (one stream
 * sync); GHS_E_NOMEM without writing when more than `capacity` edges are flagged. hi < 2^32. */
int ghs_flags_to_eids(const uint8_t *d_in_mst, uint64_t lo, uint64_t hi, uint32_t *d_eids, uint64_t capacity,
                      uint64_t *count, void *stream);

/* ---- device-resident API -----------------------------------------------------------------
 * Input: the canonical edge list in HBM (d_u, d_v, d_w: m uint32 each, 16-byte aligned) — the
 * device form of the reference's per-node neighbour files node_<id>.json
 * (create_graph_files.py:56-74), each edge once, key = w<<32 | eid. Each weight level's edges
 * are streamed out of it (edge-centric: every edge is a candidate for both of its fragments). */
void ghs_default_config(ghs_config_t *cfg);

/* workspace bytes for ghs_mst_device / a solver handle owning local_edges canonical edges. The solver
 * carves 256-byte aligned arrays out of its workspace: d_workspace must be 256-byte aligned (GHS_E_ARG
 * otherwise; ghs_mst_device, ghs_mst_device_csr, ghs_solver_create, ghs_solver_create_csr). Every other
 * entry point takes a 16-byte aligned workspace. */
size_t ghs_workspace_bytes(uint32_t n, uint64_t m, uint64_t local_edges);

/* Whole MST on one device: canonical edges -> d_in_mst (m bytes, 1 = in the MSF) + totals.
 * cfg may be NULL (defaults). Returns once *result is final (the host polls the rounds'
 * reports; one sync for the level plan). d_in_mst is written by work enqueued on `stream`:
 * complete once the stream is synchronized (a trailing no-op round may still run on return).
 * Reference: GHSAlgorithm.run, ghs_implementation.py:442-490. */
int ghs_mst_device(uint32_t n, uint64_t m, const uint32_t *d_u, const uint32_t *d_v, const uint32_t *d_w,
                   const ghs_config_t *cfg, void *d_workspace, size_t workspace_bytes, uint8_t *d_in_mst,
                   void *stream, ghs_result_t *result, ghs_round_stats_t *stats);

/* ABI 9: the same canonical list in CSR form — the north_star's "CSR edge list in HBM" and the
 * reference's per-node neighbour files (create_graph_files.py:56-74: node u lists its neighbours)
 * with each edge stored once at its smaller end: d_off = n + 1 uint32 row offsets (d_off[0] = 0,
 * nondecreasing, d_off[n] = m), edge e of row u (d_off[u] <= e < d_off[u + 1]) joins u and d_v[e]
 * with weight d_w[e]; d_v strictly ascending inside a row, u < d_v[e] < n. eid = e as in the COO
 * form (same keys, same MSF flags). The streaming passes read 8 B per edge (+ 4 B per row) instead
 * of 12. d_u may be NULL, or the caller's expanded u (16-byte aligned): then gathers of u by edge
 * id read it instead of searching d_off, and the level-opening filter pass streams (u, v, w) — the
 * faster form for that pass — while the first pass streams the CSR form. The offsets are validated
 * with the rest (GHS_E_NONCANON). */
int ghs_mst_device_csr(uint32_t n, uint64_t m, const uint32_t *d_off, const uint32_t *d_u, const uint32_t *d_v,
                       const uint32_t *d_w, const ghs_config_t *cfg, void *d_workspace, size_t workspace_bytes,
                       uint8_t *d_in_mst, void *stream, ghs_result_t *result, ghs_round_stats_t *stats);
/* d_off (n + 1 uint32) from a canonical COO list's d_u (u ascending), on the device */
int ghs_csr_offsets(uint32_t n, uint64_t m, const uint32_t *d_u, uint32_t *d_off, void *stream);

/* ---- batched solve: many small graphs in one launch (ABI 10 addition) ----------------------
 * Replaces the reference's experiment loop (ghs_implementation.py main(): six Erdos-Renyi graphs
 * of a few dozen vertices solved one after another into ghs_experiments.json) as ONE call: B graphs
 * concatenated in "batch-canonical" form — nvert[B] vertex counts, eoff[B + 1] edge offsets
 * (eoff[0] = 0, nondecreasing, eoff[B] = M < 2^31), u / v / w of M uint32 each (16-byte aligned on
 * the device); graph g owns the slice [eoff[g], eoff[g + 1]) with vertex ids LOCAL to the graph
 * (u < v < nvert[g]), canonical on its own; its edge ids are e - eoff[g] and its keys
 * (uint64)w << 32 | local eid, so every graph's flags equal canonical Kruskal's bit for bit.
 * One workgroup solves one graph entirely in LDS (csrc/batch.hip); graphs are validated by the same
 * kernel and a bad graph never disturbs its neighbours: per-graph problems are reported only in
 * ghs_batch_result_t.status, and every flag byte of a slice with monotone offsets is written (0 for
 * a graph with status 1 or 3). The two caps are design choices (one workgroup must not become the
 * batch's long pole; past them ghs_mst_device is the right tool). */
#define GHS_BATCH_MAX_VERTICES 4096u
#define GHS_BATCH_MAX_EDGES (1u << 20)
typedef struct ghs_batch_result {   /* 24 bytes, one per graph */
  uint64_t total_weight;
  uint32_t num_mst_edges;
  uint32_t rounds;    /* edge scans executed */
  uint32_t status;    /* 0 ok, 1 not canonical, 2 round cap, 3 over the size caps */
  uint32_t reserved;
} ghs_batch_result_t;
size_t ghs_batch_workspace_bytes(uint32_t num_graphs);
/* Asynchronous on `stream`: enqueues the classify + solve kernels and returns without a host sync;
 * d_in_mst (M bytes) and d_results (num_graphs entries) are complete once the stream is
 * synchronized. GHS_E_ARG: NULL / misaligned pointers; GHS_E_NOMEM: workspace_bytes short. */
int ghs_mst_batch_device(uint32_t num_graphs, const uint32_t *d_nvert, const uint32_t *d_eoff,
                         const uint32_t *d_u, const uint32_t *d_v, const uint32_t *d_w,
                         void *d_workspace, size_t workspace_bytes, uint8_t *d_in_mst,
                         ghs_batch_result_t *d_results, void *stream);
/* Host arrays: copies in, runs, copies out, syncs. results and the healthy graphs' flags are filled
 * in even when the call returns GHS_E_NONCANON / GHS_E_ROUNDCAP / GHS_E_ARG for a graph of status
 * 1 / 2 / 3 (the first such graph's index is in ghs_last_error()). num_graphs == 0: GHS_OK. */
int ghs_mst_batch_host(uint32_t num_graphs, const uint32_t *nvert, const uint32_t *eoff,
                       const uint32_t *u, const uint32_t *v, const uint32_t *w,
                       uint8_t *in_mst, ghs_batch_result_t *results);

/* ---- device ingest: raw edge list -> canonical edge list (ABI 10 addition) ------------------
 * Replaces the graph construction every reference entry point starts with (nx.Graph.add_edge over
 * the caller's triples, ghs_implementation.py:425-426, check_mst.py:6-7) for edges that are already
 * in HBM: m_raw raw edges (d_ru, d_rv, d_rw: uint32 each, any vertex ids, either orientation, repeats
 * and self-loops allowed) become the canonical list the solver entry points take, without leaving the
 * device. Semantics are nx.Graph's: self-loops are dropped; each unordered pair appears once as
 * (min, max) with the weight of its LAST raw occurrence (in raw index order, whichever orientation
 * that occurrence had); the output is ascending by (u, v). d_src (may be NULL) receives the raw index
 * of that last occurrence per canonical edge, so min(ru[src[e]], rv[src[e]]) == u[e],
 * max(...) == v[e], rw[src[e]] == w[e]: the map from the solver's edge ids back to the caller's.
 * Sizes: d_u, d_v, d_w (and d_src) must have room for m_raw entries; *m_out (host) = the canonical
 * count. Outputs and d_temp must be 16-byte aligned (what the solver requires of its inputs); the raw
 * inputs only 4-byte (slices are fine). Outputs and d_temp must not overlap the inputs or each other:
 * the inputs are read after the outputs are first written.
 * d_temp: ghs_canonicalize_temp_bytes(n, m_raw) bytes (24 B per raw edge + the sort's storage, about 36 B per
 * raw edge in all; computed on the host, no GPU needed; 0 for m_raw = 0).
 * Pipeline: a key pass (min << bits | max with bits = max(1, ceil(log2 n)), value = raw index), a
 * stable rocPRIM pairs sort over the 2 * bits key bits, a last-of-run compaction. Everything is
 * enqueued on `stream`; the call returns after ONE stream synchronise that brings back the count and
 * the error flag together.
 * Errors, checked before any device work (so GHS_E_ARG, not GHS_E_NODEVICE, on a host without GPU):
 * NULL / misaligned pointers, m_raw >= 2^32: GHS_E_ARG; temp_bytes short: GHS_E_NOMEM. m_raw == 0:
 * GHS_OK, *m_out = 0, no device work, pointers may be NULL. After the sync: any raw endpoint >= n:
 * GHS_E_ARG ("vertex id out of range"; the outputs are then unspecified, nothing was read or written
 * out of bounds); a canonical count >= 2^31 (over the solver's cap): GHS_E_ARG. */
size_t ghs_canonicalize_temp_bytes(uint32_t n, uint64_t m_raw);
int ghs_canonicalize_device(uint32_t n, uint64_t m_raw,
                            const uint32_t *d_ru, const uint32_t *d_rv, const uint32_t *d_rw,
                            uint32_t *d_u, uint32_t *d_v, uint32_t *d_w, uint32_t *d_src /* may be NULL */,
                            uint64_t *m_out, void *d_temp, size_t temp_bytes, void *stream);

/* ---- weight ranks: float / 64-bit weights -> uint32 engine weights (ABI 10 addition) --------
 * The reference accepts any comparable weight (nx.Graph, ghs_implementation.py:417-440); the engine
 * computes on uint32. Its key is (w, eid), so any order-preserving map that keeps ties tied gives the
 * same flags: d_ranks[i] = the dense rank of d_weights[i] among the DISTINCT values of the whole
 * array (0 the smallest, *distinct - 1 the largest, equal values equal ranks) — bit for bit
 * np.searchsorted(np.unique(w), w), the host path's map (graph.canonicalize). -0.0 and +0.0 are one
 * value, +-inf ordinary values, denormals distinct values; float64 is never narrowed. d_ranks is what
 * ghs_canonicalize_device takes as d_rw (the raw weights, before the canonicalisation).
 * d_weights: m elements of the type `wtype` names, aligned to their own size only (slices are fine);
 * d_ranks: m uint32, 4-byte aligned, not overlapping d_weights or d_temp; d_temp: 16-byte aligned,
 * ghs_weight_ranks_temp_bytes(wtype, m) bytes (12 B per weight for float32, 24 B otherwise, + the
 * sort's storage; computed on the host, no GPU needed; 0 for m = 0).
 * Pipeline: a key pass (an unsigned key that orders as the value does, value = index), a rocPRIM
 * pairs sort over 32 (float32) or 64 key bits, head flags over the sorted keys and a scatter of every
 * element's head count to d_ranks[index]. Everything is enqueued on `stream`; the call returns after
 * ONE stream synchronise that brings back *distinct and the NaN flag together.
 * Errors, checked before any device work (so GHS_E_ARG, not GHS_E_NODEVICE, on a host without GPU):
 * unknown wtype, NULL / misaligned / overlapping pointers, m >= 2^32: GHS_E_ARG; temp_bytes short:
 * GHS_E_NOMEM. m == 0: GHS_OK, *distinct = 0, no device work, pointers may be NULL. After the sync: a
 * NaN anywhere: GHS_E_ARG ("NaN weight"; the ranks are then unspecified, nothing was read or written
 * out of bounds). */
#define GHS_W_FLOAT32 0u
#define GHS_W_FLOAT64 1u
#define GHS_W_INT64   2u
#define GHS_W_UINT64  3u
size_t ghs_weight_ranks_temp_bytes(uint32_t wtype, uint64_t m);
int ghs_weight_ranks_device(uint32_t wtype, uint64_t m, const void *d_weights, uint32_t *d_ranks,
                            uint64_t *distinct /* host */, void *d_temp, size_t temp_bytes, void *stream);

/* ---- device verifier: is this flag vector THE MSF? (ABI 10 addition) -------------------------
 * Replaces the reference's check of a run against a recomputed NetworkX MST (check_mst.py:1-20,
 * ghs_implementation.py:746) at every size the engine solves, on the device, exactly, and without a
 * second solve: csrc/verify.hip shares no code with the solver and launches none of its kernels.
 * Let T be the flagged edges (a nonzero flag byte means "in the MSF", as in ghs_flags_to_eids) and
 * F = MSF(T) under the strict key (w, eid); if T is a forest, F = T.
 *   cyclic_edges    = |T| - |F|: flagged edges that close a cycle;
 *   unspanned_edges = edges of G (flagged or not) whose ends lie in different components of T;
 *   lighter_edges   = unflagged edges whose ends lie in one component of T and whose key is smaller
 *                     than the largest key on the F-path between its ends.
 * ok = all three are 0. Keys are distinct, so the MSF is unique: cyclic = 0 makes T a forest,
 * unspanned = 0 makes it span every component of G, lighter = 0 is the cycle property for every
 * non-tree edge — hence ok <=> the flags equal canonical Kruskal's, byte for byte. This is not a
 * weight comparison: a forest of the right total weight with the wrong tie-break fails it.
 * Method (King's Boruvka-tree lemma): plain Boruvka over T alone (|T| <= n - 1); every fragment f
 * alive at round r leaves a 16-byte node {the key f chose in round r, the dense id of its fragment at
 * round r + 1}; a fragment with no outgoing T-edge is finished (parent NONE) and dropped. Unfinished
 * fragments at least halve per round, so all levels hold <= 2n nodes. The largest key on the F-path
 * between u and v is the largest key met while walking both ends up the levels until they meet; one
 * kernel walks all m edges (an end that reaches a finished fragment first is in another component).
 * tree_edges = |T|, components = n - |F|, total_weight = the sum of w over T, rounds = Boruvka
 * rounds over T, first_bad_eid = the smallest eid counted in any of the three (UINT64_MAX if none).
 * d_in_mst (m bytes, any alignment) is only read. Work is enqueued on `stream`; the call returns once
 * *result is final (one host sync per round, <= 33, + 2). The workspace holds at most min(m, n - 1)
 * tree edges: if more are flagged the call returns GHS_OK with ok = 0, overfull = 1, tree_edges exact
 * and cyclic_edges = tree_edges - (n - 1) as a lower bound; the other counts are then unspecified.
 * Workspace: 32 B per vertex of nodes + 9 B per vertex + 32 B per possible tree edge (computed on
 * the host, no GPU needed). A verdict of ok = 0 is a result, not an error code.
 * Errors, checked before any device work (so they hold on a host without GPU): NULL or misaligned
 * pointers (16 bytes for u / v / w / workspace) or m >= 2^31: GHS_E_ARG; workspace_bytes short:
 * GHS_E_NOMEM. m == 0: GHS_OK, ok = 1, components = n, no device work, pointers may be NULL. A
 * non-canonical list (ghs_check_canonical): GHS_E_NONCANON before any index is formed from it.
 * GHS_E_ROUNDCAP: the round-cap guard (never expected). */
typedef struct ghs_verify_result {   /* 80 bytes */
  uint32_t ok, rounds, overfull, reserved;
  uint64_t tree_edges, components, total_weight;
  uint64_t cyclic_edges, unspanned_edges, lighter_edges;
  uint64_t first_bad_eid;            /* smallest eid counted above, UINT64_MAX if none */
  double ms_total;                   /* host wall time of the call */
} ghs_verify_result_t;
size_t ghs_verify_workspace_bytes(uint32_t n, uint64_t m);   /* host only, no GPU needed */
int ghs_verify_msf_device(uint32_t n, uint64_t m, const uint32_t *d_u, const uint32_t *d_v,
                          const uint32_t *d_w, const uint8_t *d_in_mst, void *d_workspace,
                          size_t workspace_bytes, void *stream, ghs_verify_result_t *result);

/* ---- vertex labels and forest cuts: which component is every vertex in? (ABI 10 addition) -----
 * The reference has no such call: the nearest things are nx.connected_components and the nx.Graph
 * that check_mst.py:1-20 builds from a result, both host passes over the edge list. This entry labels
 * the vertices by the components of a flagged forest on the device, optionally after a cut — the step
 * that turns an MSF into connected components or into a single-linkage clustering.
 * T = the edges with a nonzero flag byte (as in ghs_flags_to_eids and the verifier); K = the kept
 * edges after the cut; d_labels[v] = the rank of v's component of (V, K), components ordered by their
 * smallest vertex: vertex 0 gets label 0, labels are dense in [0, num_clusters), an isolated vertex is
 * a cluster of its own. The answer is exact and deterministic.
 *   GHS_CUT_NONE    K = T. With the engine's flags: the connected components of the graph.
 *   GHS_CUT_WEIGHT  K = the edges of T with w <= param: single linkage at distance param.
 *   GHS_CUT_COUNT   param = k >= 1 target clusters: K = T minus its d heaviest edges under the key
 *                   (w, eid), d = clamp(k - (n - |T|), 0, |T|): single linkage into k clusters. On a
 *                   forest that gives exactly max(k, n - |T|) clusters for k <= n.
 * T need not be a forest: the labels are the components of K whatever its shape, and is_forest says
 * whether K closed a cycle. More than min(m, n - 1) flagged edges cannot be a forest and do not fit
 * the workspace: GHS_E_ARG ("more flags than a forest can hold") after the count, nothing else written.
 * Method: the flags are streamed 16 per lane (any byte alignment: scalar head and tail), the kept
 * edges' ends gathered into a compact list (the weight cut is a predicate of that pass; the count cut
 * a radix select of the |T| keys for the smallest one dropped, then one pass). Components by min-root
 * hooking: par[v] = v; per round every live edge, whose ends are roots, does a read-checked
 * atomicMin(&par[max], min); the live ends are pointer-jumped to a star forest (8 hops per launch, a
 * launch that moved nothing ends the jumping); edges inside one tree leave the list, the others are
 * renamed to their roots. par[x] <= x throughout, so a component's root is its smallest vertex. A
 * root that is a local minimum and absorbs nothing in round t sees only smaller neighbours in round
 * t + 1 and hooks then, so the roots with a live edge at least halve every two rounds:
 * rounds <= 2 ceil(log2 n). Last: roots flagged, scanned, d_labels[v] = rank[par[v]].
 * d_in_mst (m bytes, any alignment) is only read. Work is enqueued on `stream`; the call returns once
 * *result and d_labels are final (one host sync per hook round + 3).
 * Workspace (ghs_forest_labels_workspace_bytes, computed on the host, no GPU needed): 8 B per vertex
 * (par, ranks) + 24 B per possible kept edge (two lists of ends, the keys of the count cut) + tile
 * counts.
 * Errors, checked before any device work (so they hold on a host without GPU): result NULL, an
 * unknown mode, GHS_CUT_WEIGHT with param >= 2^32, GHS_CUT_COUNT with param = 0, m >= 2^31, NULL or
 * misaligned pointers (16 bytes for u / v / w / workspace, 4 for labels): GHS_E_ARG; workspace_bytes
 * short: GHS_E_NOMEM. n == 0: GHS_OK, nothing written. m == 0, n > 0: identity labels (one kernel;
 * pointers other than d_labels may be NULL). A non-canonical list (ghs_check_canonical):
 * GHS_E_NONCANON before any index is formed from it. GHS_E_ROUNDCAP: more than 80 rounds;
 * GHS_E_STATE: two consecutive rounds did not halve the live roots (neither is ever expected). */
#define GHS_CUT_NONE   0u   /* keep every flagged edge */
#define GHS_CUT_WEIGHT 1u   /* keep flagged edges with w <= param (param < 2^32) */
#define GHS_CUT_COUNT  2u   /* param = k >= 1 target clusters: drop the d heaviest flagged edges under
                               the key (w, eid), d = clamp(k - (n - |T|), 0, |T|) */
typedef struct ghs_labels_result {   /* 64 bytes */
  uint64_t flagged_edges;   /* |T| */
  uint64_t kept_edges;      /* |T| - dropped */
  uint64_t dropped_edges;
  uint64_t num_clusters;    /* distinct labels written */
  uint64_t cut_key;         /* GHS_CUT_COUNT: the smallest key dropped (w << 32 | eid); UINT64_MAX if
                               nothing was dropped or in the other modes */
  uint32_t rounds;          /* hook rounds executed */
  uint32_t is_forest;       /* 1 iff num_clusters == n - kept_edges (the kept edges close no cycle) */
  double ms_total;          /* host wall time of the call */
  uint64_t reserved;        /* 0: pads the record to 64 bytes */
} ghs_labels_result_t;
size_t ghs_forest_labels_workspace_bytes(uint32_t n, uint64_t m);   /* host only, no GPU needed */
int ghs_forest_labels_device(uint32_t n, uint64_t m, const uint32_t *d_u, const uint32_t *d_v,
                             const uint32_t *d_w, const uint8_t *d_in_mst, uint32_t mode, uint64_t param,
                             uint32_t *d_labels /* n */, void *d_workspace, size_t workspace_bytes,
                             void *stream, ghs_labels_result_t *result);
/* the same for host arrays (copy in, run, copy out on the default stream); the argument errors above
 * except the alignments, then GHS_E_NODEVICE without a GPU */
int ghs_forest_labels_host(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w,
                           const uint8_t *in_mst, uint32_t mode, uint64_t param, uint32_t *labels,
                           ghs_labels_result_t *result);

/* ---- rooted forest: parent, depth and preorder of every vertex (ABI 10 addition) ---------------
 * The reference's nodes end a run with in_branch, the neighbour towards their fragment's core
 * (ghs_implementation.py:63,212, ghs_implementation_mpi.py:57,309), and its REPORT / CHANGEROOT
 * convergecasts walk those pointers; the flags this engine returns carry no orientation. This entry
 * roots the flagged forest on the device, at any depth (a path costs what a star costs: nothing is
 * level-synchronous). T = the edges with a nonzero flag byte, as everywhere else. Exact and
 * deterministic: two calls give identical bytes.
 *   root        the root of a tree is its smallest vertex (the convention of the labels call: label
 *               order = root order); an isolated vertex is a root.
 *   parent[v]   the neighbour of v on the T-path to its root; 0xffffffff for a root.
 *   parent_eid[v]  the canonical edge id of {v, parent[v]}; 0xffffffff for a root.
 *   depth[v]    the number of edges to the root.
 *   size[v]     the number of vertices in v's subtree, v included.
 *   pre[v]      a DFS preorder number, a permutation of 0..n-1. Trees take consecutive blocks of
 *               numbers in order of their roots. Inside a tree the root gets the block's first number
 *               and visits its children in ascending id. A vertex x entered from parent p visits its
 *               children in ascending id cyclically, starting after p: first the children greater
 *               than p, then those less than p. (The order the Euler tour gives: with every adjacency
 *               sorted by neighbour id, succ(x -> y) is the arc after (y -> x) in y's cyclic
 *               adjacency.) It is a genuine DFS preorder: a is an ancestor-or-self of b exactly when
 *               pre[a] <= pre[b] < pre[a] + size[a], and every subtree is one contiguous range.
 * d_pre and d_size may be NULL, independently (not written then).
 * A T that closes a cycle is a result, not an error: GHS_OK with is_forest = 0 and flagged_edges exact;
 * all other fields and the five arrays are then unspecified (written only in bounds; no loop depends
 * on T being acyclic). More than min(m, n - 1) flagged edges cannot be a forest and do not fit the
 * workspace: GHS_E_ARG ("more flags than a forest can hold") after the count, nothing else written.
 * Method (csrc/root.hip): the flags are streamed 16 per lane (any byte alignment) and (u, v, eid) of
 * the flagged edges gathered in eid order; a stable rocPRIM pairs sort by v gives the reverse arcs,
 * so a vertex's reverse block then forward block is its adjacency in ascending neighbour id, with no
 * atomics; the Euler successor permutation over the 2|T| arcs; a splitter list ranking (splitters: the
 * first arc of every vertex that is the smallest within two hops + a hashed 1-in-64 sample; one lane walks each
 * sublist; Wyllie doubling with min-carry on the circular list of splitters finds each tour's smallest
 * vertex and breaks the tour at its first arc, a second doubling ranks the splitters; a second walk
 * writes every arc's tour position); the earlier arc of a tree edge is its down arc (parent,
 * parent_eid, size), and a scan of the down arcs in tour order gives depth and pre.
 * rounds = the doubling rounds of both phases, each ended by a round that changes nothing:
 * rounds <= 2 ceil(log2(2 |T|)) + 2 (DESIGN.md "Rooted forest" has the proof); GHS_E_ROUNDCAP past
 * it is never expected. T is a forest iff every arc lies on a tour with a splitter and the number of
 * roots (isolated vertices + smallest vertices of tours) is n - |T|.
 * d_in_mst (m bytes, any alignment) is only read. Work is enqueued on `stream`; the call returns once
 * *result and the arrays are final (4 host syncs + one per round).
 * Workspace (ghs_forest_root_workspace_bytes, computed on the host, no GPU needed; C = min(m, n - 1)
 * possible tree edges): 29 B per vertex (adjacency ranges 16, tree size 4, root prefix 8, a flag 1) + 24 B per
 * possible tree edge (u, v, eid, sorted keys, permutation, inverse) + 84 B per possible arc (2 C: arc
 * record 8, tour position 4, and per possible splitter its arc 4, length 4, predecessor 4, key 8, root
 * 4, two 16-byte and two 8-byte doubling buffers) + 12 B per 64 arcs of splitter bits + the tile sums
 * of the largest scan + rocPRIM's sort storage + 1 KiB of status.
 * Errors, checked before any device work (so they hold on a host without GPU): result NULL,
 * m >= 2^31, NULL or misaligned pointers (16 bytes for u / v / workspace, 4 for the five outputs):
 * GHS_E_ARG; workspace_bytes short: GHS_E_NOMEM. n == 0: GHS_OK, nothing written. m == 0, n > 0: every
 * vertex is a root (parent and parent_eid 0xffffffff, depth 0, pre[v] = v, size 1; only the output
 * pointers are needed). A non-canonical list (ghs_check_canonical): GHS_E_NONCANON before any index is
 * formed from it. */
typedef struct ghs_root_result {   /* 48 bytes */
  uint64_t flagged_edges;   /* |T| */
  uint64_t num_trees;       /* roots written (isolated vertices included) */
  uint64_t max_depth;
  uint32_t rounds;          /* data-dependent launch rounds of the ranking */
  uint32_t is_forest;       /* 1 iff T closes no cycle */
  double   ms_total;        /* host wall time of the call */
  uint64_t reserved;        /* 0 */
} ghs_root_result_t;
size_t ghs_forest_root_workspace_bytes(uint32_t n, uint64_t m);   /* host only, no GPU needed */
int ghs_forest_root_device(uint32_t n, uint64_t m, const uint32_t *d_u, const uint32_t *d_v,
                           const uint8_t *d_in_mst,
                           uint32_t *d_parent, uint32_t *d_parent_eid, uint32_t *d_depth,
                           uint32_t *d_pre /* may be NULL */, uint32_t *d_size /* may be NULL */,
                           void *d_workspace, size_t workspace_bytes, void *stream,
                           ghs_root_result_t *result);
/* the same for host arrays (copy in, run, copy out on the default stream; pre and size may be NULL);
 * the argument errors above except the alignments, then GHS_E_NODEVICE without a GPU */
int ghs_forest_root_host(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint8_t *in_mst,
                         uint32_t *parent, uint32_t *parent_eid, uint32_t *depth, uint32_t *pre, uint32_t *size,
                         ghs_root_result_t *result);

/* ---- path queries: what lies between a and b? (ABI 10 addition) ---------------------------------
 * The reference's nodes answer questions about the tree by walking in_branch (the REPORT / CHANGEROOT
 * convergecasts, ghs_implementation.py:235-387). These calls are the device form of that walk over
 * the arrays ghs_forest_root_device writes, in O(log depth) dependent loads per query at any depth.
 * For a pair (a, b):
 *   key    the largest key w << 32 | eid among the edges of the forest path a .. b: the bottleneck
 *          (minimax) edge. With the engine's MSF it is the minimax distance in the graph itself, the
 *          edge a new edge (a, b, w) would displace from the MSF, and the single-linkage merge height
 *          of a and b. UINT64_MAX when a == b (no edge) or when a and b are in different trees.
 *   lca    the lowest common ancestor under the rooting given; a itself when a == b; 0xffffffff when a
 *          and b are in different trees.
 *   hops   the number of edges on the path, depth[a] + depth[b] - 2 depth[lca]; 0 when a == b;
 *          0xffffffff when a and b are in different trees.
 * Exact and deterministic: two calls give identical bytes.
 * Index (ghs_forest_paths_create, csrc/paths.hip): K = max(1, bit_length(max_depth)) levels of n
 * 16-byte nodes {uint64 key, uint32 up, uint32 aux}. Level 0: up = parent (the vertex itself for a
 * root), key = w[parent_eid] << 32 | parent_eid (0 for a root), aux = depth. Level k: up_k[v] =
 * up_{k-1}[up_{k-1}[v]], key_k[v] = max(key_{k-1}[v], key_{k-1}[up_{k-1}[v]]), aux = depth: K - 1
 * stream-ordered launches, no host sync between them. A root points at itself with key 0, so a jump
 * past a root is harmless. Key 0 is also the key of edge 0 with weight 0: a == b is decided before
 * any key is looked at. The index keeps no reference to the caller's arrays: u, v, w, parent,
 * parent_eid and depth may be released after create.
 * The level-0 pass validates parent / parent_eid / depth, which become gather indices. Every vertex v
 * is a root (parent == parent_eid == 0xffffffff and depth 0) or has parent < n, parent_eid < m,
 * {u[e], v[e]} == {v, parent[v]}, depth[v] == depth[parent[v]] + 1 and depth[v] <= max_depth. Depth
 * falls by one along every parent pointer, so what passes is acyclic and no later loop depends on
 * trust. Anything else: GHS_E_ARG ("not a rooted forest") after the one host sync of the call, no
 * handle; nothing is read or written out of bounds. max_depth is an upper bound of the depths (the
 * max_depth of ghs_root_result_t); result->max_depth is the largest depth found.
 * Memory: ghs_forest_paths_index_bytes(n, max_depth) = 16 K n rounded up to 256, + 256 bytes of status
 * (computed on the host, no GPU needed), caller-owned, to be kept alive and unchanged until destroy.
 * The handle is a small host object. The status block lives in the index, so one query at a time per
 * handle; queries on different handles, or create on different indexes, may run concurrently.
 * Query (ghs_forest_paths_query): q pairs d_a[i], d_b[i] -> d_key[i], d_lca[i], d_hops[i]; each output
 * pointer may be NULL, independently (not written then). 4 queries per lane advance together: both
 * level-0 nodes give the depths, the deeper end is lifted by the set bits of the depth difference,
 * then levels bit_length(common depth) - 1 .. 1 are tried from the top (both ends jump where their
 * targets differ) and one or two level-0 steps finish; hops comes from the jump counts. Work is
 * enqueued on `stream`; the call returns once the outputs and *result are final (one host sync).
 * connected counts the pairs with an lca (a == b included). An id >= n anywhere in d_a / d_b:
 * GHS_E_ARG ("vertex id out of range") after the sync; the outputs are then unspecified and nothing
 * was indexed out of range (the rule of ghs_canonicalize_device).
 * Errors, checked before any device work (so they hold on a host without GPU): result, out or handle
 * NULL, m >= 2^31, max_depth >= n (n > 0), q >= 2^32, NULL or misaligned pointers (16 bytes for u / v /
 * w / index, 4 for parent / parent_eid / depth / a / b / lca / hops, 8 for key): GHS_E_ARG;
 * index_bytes short: GHS_E_NOMEM. q == 0: GHS_OK, no device work. n == 0: create succeeds with 0
 * trees and no device work (all pointers may be NULL); a query with q > 0 on it is GHS_E_ARG (every id
 * is out of range). m == 0: every vertex must be a root; d_u / d_v / d_w may be NULL.
 * ghs_forest_paths_destroy frees the handle only (NULL is accepted). */
typedef struct ghs_paths ghs_paths_t;            /* host handle over caller-owned device memory */
typedef struct ghs_paths_result {   /* 48 bytes */
  uint64_t levels;          /* K */
  uint64_t max_depth;       /* the largest depth found (<= the bound given) */
  uint64_t num_trees;       /* roots */
  uint64_t index_bytes;     /* ghs_forest_paths_index_bytes(n, max_depth) */
  double   ms_total;        /* host wall time of the call */
  uint64_t reserved;        /* 0 */
} ghs_paths_result_t;
typedef struct ghs_paths_query_result {   /* 32 bytes */
  uint64_t queries;         /* q */
  uint64_t connected;       /* pairs in one tree (a == b included) */
  double   ms_total;        /* host wall time of the call */
  uint64_t reserved;        /* 0 */
} ghs_paths_query_result_t;
size_t ghs_forest_paths_index_bytes(uint32_t n, uint64_t max_depth);          /* host only, no GPU needed */
int ghs_forest_paths_create(uint32_t n, uint64_t m, const uint32_t *d_u, const uint32_t *d_v, const uint32_t *d_w,
                            const uint32_t *d_parent, const uint32_t *d_parent_eid, const uint32_t *d_depth,
                            uint64_t max_depth, void *d_index, size_t index_bytes, void *stream,
                            ghs_paths_result_t *result, ghs_paths_t **out);
int ghs_forest_paths_query(ghs_paths_t *h, uint64_t q, const uint32_t *d_a, const uint32_t *d_b,
                           uint64_t *d_key /* may be NULL */, uint32_t *d_lca /* may be NULL */,
                           uint32_t *d_hops /* may be NULL */, void *stream, ghs_paths_query_result_t *result);
int ghs_forest_paths_destroy(ghs_paths_t *h);
/* the same for host arrays and flags: copy in, root the flags (ghs_forest_root_device without pre and
 * size), build the index, run the q queries, copy out; key, lca and hops may be NULL. The argument
 * errors above except the alignments (and NULL u / v / w / in_mst with m > 0, NULL a / b with q > 0),
 * then GHS_E_NODEVICE without a GPU. q == 0: GHS_OK, no device work. Flags that close a cycle:
 * GHS_E_ARG ("flags are not a forest"). */
int ghs_forest_paths_host(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w,
                          const uint8_t *in_mst, uint64_t q, const uint32_t *a, const uint32_t *b,
                          uint64_t *key, uint32_t *lca, uint32_t *hops, ghs_paths_query_result_t *result);
/* what a live handle indexes: n, K, the depth bound given to create and the device address of level 0
 * (level k starts 16 k n bytes further; NULL when n == 0). Host only, no device work. NULL or
 * destroyed handle, NULL out: GHS_E_ARG. */
typedef struct ghs_paths_info {   /* 32 bytes */
  uint64_t n;
  uint64_t levels;          /* K (0 when n == 0) */
  uint64_t max_depth;       /* the bound given to ghs_forest_paths_create */
  const void *d_index;      /* the caller's index memory */
} ghs_paths_info_t;
int ghs_forest_paths_info(const ghs_paths_t *h, ghs_paths_info_t *out);

/* ---- replacement edges: what takes e's place when e fails? (ABI 10 addition) ----------------------
 * The path query looks from a non-forest edge into the forest; this is the opposite question, the
 * other half of MST sensitivity analysis, and what a network asks when a link fails (the reference
 * rebuilds from scratch, ghs_implementation.py:442-490). Input: the edge list and a rooted forest of
 * it, as indexed by ghs_forest_paths_create. Every non-root vertex x stands for the forest edge
 * (x, parent[x]). A non-forest edge f = (a, b) with both ends in one tree covers the forest edges on
 * the tree path a .. b; an edge whose ends lie in different trees covers nothing and is only counted.
 *   d_repl[x]                 the smallest key w[f] << 32 | f over the non-forest edges that cover x's
 *                             edge: the edge that reconnects the two halves at the least weight.
 *                             UINT64_MAX for a root, or when no edge covers it: a bridge of the graph.
 *   d_repl_eid_by_edge[e]     (optional, m entries) for a forest edge e the low word of that key,
 *                             0xffffffff for a bridge and for every non-forest edge.
 * Edge e is a forest edge exactly when one of its ends is not a root and has e as the eid of its
 * level-0 node. No flag array is read: the index was validated against u, v, w at create, which must
 * be the same arrays (or copies) here.
 * A forest edge whose replacement key is below its own key (`improving`) shows that the flags are not
 * the MSF; with the engine's MSF improving == 0. The smallest w[repl] - w[e] over all forest edges is
 * the best swap: total weight + best_delta is the weight of the second-best spanning forest.
 * Algorithm (csrc/replace.hip): K levels of n uint64 slots cover[j][x] = "the 2^j forest edges going
 * up from x are covered by this key", all UINT64_MAX at first; level 0 is d_repl itself. (1) One pass
 * over the m edges finds each non-forest edge's meeting point with the query's lift-then-descend walk
 * (four edges per lane), which gives L = depth[end] - depth[lca] per end; for L > 0 and j = floor(log2
 * L) the key is min-ed into cover[j][end] and cover[j][end lifted by L - 2^j]: two ranges that overlap
 * and are exactly the L edges. (2) For j = K - 1 .. 1 one launch over n mins a set cover[j][x] into
 * cover[j-1][x] and cover[j-1][up_{j-1}(x)]. (3) One pass over n sets root slots, scatters the
 * per-edge array, and reduces the counts and the best swap. Every minimum reads the slot first and
 * skips the atomic when the slot is not larger (slots only decrease, so a stale read never hides a
 * needed update). Integer minima commute: two calls give identical bytes. One host sync, at the end.
 * Memory: ghs_forest_replace_workspace_bytes(n, max_depth) = 8 (K - 1) n rounded up to 256, + 256
 * bytes of status, K = max(1, bit_length(max_depth)) (computed on the host, no GPU needed); max_depth
 * is the bound the index was created with. The workspace is scratch. The index is only read, but the
 * handle's one-call-at-a-time rule holds here too.
 * Errors, in this order, before any device work (so they hold on a host without GPU): NULL or
 * destroyed handle, NULL result, m >= 2^31, NULL or misaligned pointers (16 bytes for u / v / w / the
 * workspace, 8 for d_repl, 4 for d_repl_eid_by_edge, which may be NULL): GHS_E_ARG; workspace short:
 * GHS_E_NOMEM. An index over n == 0: no device work, d_repl may be NULL, GHS_OK when m == 0 (with
 * m > 0 every endpoint is out of range). m == 0: d_u / d_v / d_w may be NULL, every slot is
 * UINT64_MAX. An edge endpoint >= n: GHS_E_ARG ("edge endpoint out of range") after the sync; the
 * outputs are then unspecified and nothing was read or written out of range. */
typedef struct ghs_replace_result {   /* 64 bytes */
  uint64_t tree_edges;      /* forest edges (non-root vertices) */
  uint64_t covering_edges;  /* non-forest edges with both ends in one tree */
  uint64_t cross_edges;     /* non-forest edges between two trees */
  uint32_t bridges;         /* forest edges without a replacement */
  uint32_t improving;       /* forest edges whose replacement key is below their own: 0 for the MSF */
  int64_t  best_delta;      /* the smallest w[repl] - w[e]; 0 when every forest edge is a bridge */
  uint32_t best_out_eid;    /* the forest edge of the best swap (ties: the smallest eid); 0xffffffff: none */
  uint32_t best_in_eid;     /* its replacement; 0xffffffff: none */
  double   ms_total;        /* host wall time of the call */
  uint64_t reserved;        /* 0 */
} ghs_replace_result_t;
size_t ghs_forest_replace_workspace_bytes(uint32_t n, uint64_t max_depth);    /* host only, no GPU needed */
int ghs_forest_replace_device(ghs_paths_t *h, uint64_t m, const uint32_t *d_u, const uint32_t *d_v, const uint32_t *d_w,
                              uint64_t *d_repl /* n */, uint32_t *d_repl_eid_by_edge /* m or NULL */,
                              void *d_workspace, size_t workspace_bytes, void *stream, ghs_replace_result_t *result);
/* where the time of ghs_forest_replace_device goes, for benchmarks: enable != 0 makes this thread's later
 * calls record HIP events around their four phases (five event records per call; off by default); ms,
 * when not NULL, first receives the last recorded call's times in milliseconds: ms[0] the memsets,
 * ms[1] the cover pass, ms[2] the K - 1 push-down launches, ms[3] the finish passes. Always GHS_OK. */
int ghs_forest_replace_phases(int enable, double *ms /* 4, may be NULL */);
/* the same for host arrays and flags: copy in, root the flags (ghs_forest_root_device without pre and
 * size), build the index, replace, copy out; repl (n entries, indexed by vertex under the rooting at
 * every tree's smallest vertex) and repl_eid_by_edge (m entries) may each be NULL. The argument errors
 * above except the alignments (and NULL u / v / w / in_mst with m > 0), then GHS_E_NODEVICE without a
 * GPU. n == 0: GHS_OK, no device work. Flags that close a cycle: GHS_E_ARG ("flags are not a forest"). */
int ghs_forest_replace_host(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w,
                            const uint8_t *in_mst, uint64_t *repl, uint32_t *repl_eid_by_edge,
                            ghs_replace_result_t *result);

/* ---- tree distances: how far is it from a to b? (ABI 10 addition) ----------------------------------
 * The path query gives the heaviest edge between a and b; these calls give the sum of the edges, the
 * number a spanning-tree user asks for first (a reference node knows its level and its in_branch only,
 * ghs_implementation.py:63,212, and would walk edge by edge). Built on it: the stretch dist_T(u, v) / w
 * of every graph edge over the forest, and the diameter, the two far ends, every vertex's eccentricity
 * and the centre of every tree. All calls work on the index of ghs_forest_paths_create (csrc/dist.hip
 * reaches it through ghs_forest_paths_info), read it only, and obey the handle's one-call-at-a-time
 * rule: the two calls without a workspace keep their counters in the index's status block. Exact
 * integers throughout; two calls give identical bytes.
 *
 * Weighted depth (ghs_forest_wdepth_device): d_wdepth[v] = the sum of the weights on the path from v
 * to its tree's root, 0 for a root. metric = GHS_DIST_WEIGHT uses the weights in the index's level-0
 * keys (key >> 32); GHS_DIST_HOPS uses 1 per edge, so the result is the depth. Nothing is
 * level-synchronous over the depth: with S_k[v] = the sum of the (up to) 2^k edges going up from v,
 * S_{k+1}[v] = S_k[v] + S_k[up_k[v]]; a root points at itself with key 0 and up_k of a vertex with
 * fewer than 2^k ancestors is its root, so a jump past a root adds 0. K launches over n, ping-ponging
 * between d_wdepth and one workspace slab; 2^K > max_depth makes the last one final. The sums are exact
 * in uint64: depth < 2^31 and w < 2^32 keep every sum below 2^63, so wd[a] + wd[b] never wraps either.
 * One host sync. The array is the caller's: the later calls take it as an argument, read its values
 * and never use them as indices (a wrong array gives wrong distances, nothing else).
 * Workspace: ghs_forest_dist_workspace_bytes(n, max_depth) = 8 n rounded up to 256, + 256 bytes of
 * status, at any K (computed on the host, no GPU needed; max_depth is the bound the index was created
 * with). One formula for this call and for ghs_forest_diameter_device. The workspace is scratch.
 * Errors, in this order, before any device work (so they hold on a host without GPU): NULL or
 * destroyed handle, unknown metric, NULL or misaligned pointers (8 bytes for d_wdepth, 16 for the
 * workspace): GHS_E_ARG; workspace short: GHS_E_NOMEM. An index over n == 0: GHS_OK, no device work,
 * d_wdepth may be NULL.
 *
 * Distance queries (ghs_forest_dist_query): q pairs d_a[i], d_b[i] -> d_dist[i] = wd[a] + wd[b] -
 * 2 wd[lca(a, b)]: 0 when a == b, UINT64_MAX when a and b are in different trees. d_lca (may be NULL)
 * receives the lowest common ancestor as the path query defines it (a when a == b, 0xffffffff across
 * trees). One fused kernel: the path query's LCA walk without its keys (four pairs per lane advancing
 * together on 16-byte node loads), then the three 8-byte gathers; no LCA array goes through memory.
 * One host sync. An id >= n anywhere in d_a / d_b: GHS_E_ARG ("vertex id out of range") after the sync;
 * the outputs are then unspecified and nothing was read or written out of range.
 * Errors before any device work: NULL result, NULL or destroyed handle, q >= 2^32, then (q > 0) NULL
 * d_a / d_b / d_dist / d_wdepth, misaligned pointers (4 bytes for a / b / lca, 8 for wdepth / dist):
 * GHS_E_ARG. q == 0: GHS_OK, no device work, every pointer may be NULL. An index over n == 0 with
 * q > 0: GHS_E_ARG (every id is out of range).
 *
 * The graph's own edges (ghs_forest_edge_dist_device): the canonical list as m pairs (u[e], v[e]) with
 * their weights; d_dist_by_edge[e] (may be NULL) = dist(u[e], v[e]), UINT64_MAX for an edge between two
 * trees. The sums and the maximum run over the edges with both ends in one tree. The stretch of edge e
 * is dist / w; ratios are left to the caller, the kernel stays in integers. tight_edges counts dist ==
 * w: every forest edge, and with positive weights only forest edges and their ties. The same walk as
 * the query; the smallest eid attaining max_dist is found by a second pass (over d_dist_by_edge when it
 * was written; otherwise the walk is repeated, which doubles the call's time). One host sync.
 * Errors before any device work: NULL result, NULL or destroyed handle, m >= 2^31, then (m > 0) NULL
 * d_u / d_v / d_w / d_wdepth, misaligned pointers (16 bytes for u / v / w, 8 for wdepth /
 * dist_by_edge): GHS_E_ARG. m == 0: GHS_OK, no device work. An endpoint >= n: GHS_E_ARG ("edge endpoint
 * out of range") after the sync.
 *
 * Diameters (ghs_forest_diameter_device): non-negative weights make two sweeps exact on a tree.
 *   d_root_of[v]   the root of v's tree (under the index's rooting).
 *   p              the vertex farthest from the root; among ties the smallest id.
 *   q              the vertex farthest from p; among ties the smallest id.
 *   d_diam[r]      for a root r: dist(p, q), the diameter of its tree. 0 for every non-root slot.
 *   d_end_a[r], d_end_b[r]   for a root r: p and q. 0xffffffff for every non-root slot. A single-vertex
 *                  tree has diameter 0 and both ends equal to itself.
 *   d_ecc[v]       (may be NULL) max(dist(v, p), dist(v, q)): the distance to the farthest vertex of the tree.
 * Each sweep is n fused distance queries and a per-tree arg-max in two steps (a 63-bit distance and an
 * id do not fit one 64-bit key): a maximum of the distance into the root's slot, then a minimum of the
 * id among the vertices attaining it. The eccentricities are formed whether or not d_ecc is given (in
 * the workspace otherwise): the centre is their arg-min. One host sync.
 * Errors, in this order, before any device work: NULL result, NULL or destroyed handle, NULL pointers
 * (d_ecc excepted), misaligned pointers (4 bytes for root_of / end_a / end_b, 8 for wdepth / diam / ecc,
 * 16 for the workspace): GHS_E_ARG; workspace short (ghs_forest_dist_workspace_bytes): GHS_E_NOMEM. An
 * index over n == 0: GHS_OK, no device work, 0 trees. */
#define GHS_DIST_WEIGHT 0u   /* sum the weights of the index's level-0 keys */
#define GHS_DIST_HOPS   1u   /* 1 per edge: the weighted depth is the depth */
typedef struct ghs_dist_query_result {   /* 48 bytes */
  uint64_t queries;         /* q */
  uint64_t connected;       /* pairs in one tree (a == b included) */
  uint64_t disconnected;    /* pairs across two trees: q - connected */
  uint64_t max_dist;        /* the largest finite distance; 0 when no pair is connected */
  double   ms_total;        /* host wall time of the call */
  uint64_t reserved;        /* 0 */
} ghs_dist_query_result_t;
typedef struct ghs_edge_dist_result {   /* 80 bytes */
  uint64_t edges;           /* m */
  uint64_t sum_dist_lo;     /* the sum of the finite distances, a 128-bit value: low word ... */
  uint64_t sum_dist_hi;     /* ... high word (260M edges times 2^40 and more do not fit 64 bits) */
  uint64_t sum_w;           /* the sum of the weights of the same edges */
  uint64_t max_dist;        /* the largest finite distance */
  uint64_t cross_edges;     /* edges whose ends lie in different trees: 0 for a spanning forest */
  uint64_t tight_edges;     /* edges with dist == w */
  uint32_t max_eid;         /* the smallest eid attaining max_dist; 0xffffffff when every edge is a cross edge */
  uint32_t reserved32;      /* 0 */
  double   ms_total;        /* host wall time of the call */
  uint64_t reserved;        /* 0 */
} ghs_edge_dist_result_t;
typedef struct ghs_diameter_result {   /* 48 bytes */
  uint64_t num_trees;       /* roots */
  uint64_t max_diameter;    /* the largest diameter */
  uint64_t min_ecc;         /* the smallest eccentricity in the tree of max_root: its radius */
  uint32_t max_root;        /* the root of the tree with the largest diameter (ties: the smallest root) */
  uint32_t center;          /* the vertex of that tree attaining min_ecc (ties: the smallest id) */
  double   ms_total;        /* host wall time of the call */
  uint64_t reserved;        /* 0 */
} ghs_diameter_result_t;
size_t ghs_forest_dist_workspace_bytes(uint32_t n, uint64_t max_depth);       /* host only, no GPU needed */
int ghs_forest_wdepth_device(ghs_paths_t *h, uint32_t metric, uint64_t *d_wdepth /* n */, void *d_workspace,
                             size_t workspace_bytes, void *stream);
int ghs_forest_dist_query(ghs_paths_t *h, const uint64_t *d_wdepth, uint64_t q, const uint32_t *d_a, const uint32_t *d_b,
                          uint64_t *d_dist /* q */, uint32_t *d_lca /* q, may be NULL */,
                          ghs_dist_query_result_t *result, void *stream);
int ghs_forest_edge_dist_device(ghs_paths_t *h, const uint64_t *d_wdepth, uint64_t m, const uint32_t *d_u,
                                const uint32_t *d_v, const uint32_t *d_w, uint64_t *d_dist_by_edge /* m, may be NULL */,
                                ghs_edge_dist_result_t *result, void *stream);
int ghs_forest_diameter_device(ghs_paths_t *h, const uint64_t *d_wdepth, uint32_t *d_root_of /* n */,
                               uint64_t *d_diam /* n, by root */, uint32_t *d_end_a /* n, by root */,
                               uint32_t *d_end_b /* n, by root */, uint64_t *d_ecc /* n, may be NULL */,
                               void *d_workspace, size_t workspace_bytes, ghs_diameter_result_t *result, void *stream);
/* the same for host arrays and flags: copy in, root the flags (ghs_forest_root_device without pre and
 * size), build the index and the weighted depth under `metric`, answer, copy out. dist_host: q pairs,
 * dist and lca may each be NULL. diameter_host: n entries per array, indexed as above under the rooting
 * at every tree's smallest vertex; each array may be NULL. The argument errors above except the
 * alignments (and NULL u / v / w / in_mst with m > 0, NULL a / b with q > 0, an unknown metric), then
 * GHS_E_NODEVICE without a GPU. q == 0 (dist_host) and n == 0 (diameter_host): GHS_OK, no device work.
 * Flags that close a cycle: GHS_E_ARG ("flags are not a forest"). */
int ghs_forest_dist_host(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w,
                         const uint8_t *in_mst, uint32_t metric, uint64_t q, const uint32_t *a, const uint32_t *b,
                         uint64_t *dist, uint32_t *lca, ghs_dist_query_result_t *result);
int ghs_forest_diameter_host(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w,
                             const uint8_t *in_mst, uint32_t metric, uint32_t *root_of, uint64_t *diam, uint32_t *end_a,
                             uint32_t *end_b, uint64_t *ecc, ghs_diameter_result_t *result);

/* ---- single-linkage dendrogram: in which order do the clusters merge? (ABI 10 addition) -----------
 * ghs_forest_labels_device answers one cut and the path query one pair per call; this call gives the
 * whole merge order: the Kruskal merge tree of the flagged forest T (t = |T| edges with a nonzero flag
 * byte), scipy's linkage matrix for the engine's MSF. Merge j, 0 <= j < t, is the j-th lightest edge
 * of T under the key (w, eid). Node ids are scipy's: vertex v is node v, merge j is node n + j.
 *   d_leaf_parent[n]    the merge that first absorbs vertex v = the rank of v's lightest incident
 *                       T-edge; 0xffffffff for an isolated vertex.
 *   d_merge_eid[t]      the canonical edge id of merge j.
 *   d_merge_parent[t]   the merge that next absorbs the cluster made by merge j; 0xffffffff for the
 *                       last merge of a tree.
 *   d_child_a[t], d_child_b[t]   the two node ids joined by merge j, child_a < child_b.
 *   d_size[t]           the number of vertices of the cluster after merge j.
 * All arrays have capacity C = min(m, n - 1); entries at index >= t are not written. d_child_a,
 * d_child_b and d_size may be NULL, independently. Exact integers; two calls give identical bytes. For
 * a connected graph with distinct weights [child_a, child_b, w[merge_eid], size] is
 * scipy.cluster.hierarchy.linkage(y, 'single').
 * A T that closes a cycle is a result, not an error: GHS_OK with is_forest = 0 and flagged_edges exact;
 * the other fields and the arrays are then unspecified (written only in bounds). More than
 * min(m, n - 1) flagged edges: GHS_E_ARG ("more flags than a forest can hold") after the count.
 * Method (csrc/dendro.hip): a dendrogram is as high as a path is long, so nothing is level-synchronous
 * in the depth of the forest or of the dendrogram. The t keys are sorted by rocPRIM; an edge is its
 * rank from there on. A level takes supervertices and a forest of edges on them: every supervertex
 * finds its lightest incident edge (atomicMin; at level 0 this is leaf_parent); an edge that is the
 * lightest of an end is chosen, the others are alpha edges (at most half); the groups are the
 * components of the chosen edges, found by pointer doubling and numbered by a scan; the alpha edges
 * over the groups are the next level. On the way back a chosen edge e of group S hangs under the
 * highest node among S and its ancestors in the deeper level's dendrogram that is lighter than e,
 * found by binary lifting; a stable sort by that node lines the chosen edges up in chains, each one's
 * parent the next. Children come from atomicMin / atomicMax into the parent's two slots, sizes and the
 * height from doubling up the finished parents with integer atomicAdd.
 * levels <= ceil(log2(max(n, 2))) contraction levels with an edge. rounds = the data-dependent
 * doubling rounds: per level at most ceil(log2 nv) + 1 pointer jumps and ceil(log2 ne') + 2 lifting
 * tables, then at most ceil(log2 t) + 3 size rounds, so rounds <= levels (2 ceil(log2 n) + 3) +
 * ceil(log2 n) + 3 (DESIGN.md "Dendrogram"); GHS_E_ROUNDCAP past either bound is never expected.
 * d_in_mst (m bytes, any alignment) is only read. Work is enqueued on `stream`; the call returns once
 * *result and the arrays are final (one host sync per round and three per level).
 * Workspace (ghs_forest_dendro_workspace_bytes, computed on the host, no GPU needed), sized by
 * C = min(m, n - 1) possible merges, not by m: kept per level 20 B per edge of the level (+ 16 B past
 * level 0), at most C >> l edges at level l: at most 56 B per possible merge over all levels; + a
 * scratch that is the largest of: the key sort (16 B per possible merge + 4 B per 4096 edges of m), a
 * level (28 B per vertex + 8 B per possible merge), an expansion (2 (ceil(log2(C / 2)) + 2) + 12 B
 * per possible merge: the lifting tables), sizes (20 B per possible merge); + rocPRIM's sort / scan
 * storage + 1 KiB of status.
 * Errors, checked before any device work (so they hold on a host without GPU): result NULL,
 * m >= 2^31, n + min(m, n - 1) > 2^32 (node ids), NULL or misaligned pointers (16 bytes for u / v / w /
 * workspace, 4 for the six outputs): GHS_E_ARG; workspace_bytes short: GHS_E_NOMEM. n == 0: GHS_OK,
 * nothing written. m == 0, n > 0: every leaf_parent is 0xffffffff (only that pointer is needed). A
 * non-canonical list (ghs_check_canonical): GHS_E_NONCANON before any index is formed from it. */
typedef struct ghs_dendro_result {   /* 48 bytes */
  uint64_t flagged_edges;   /* t = |T| */
  uint64_t num_trees;       /* n - t (isolated vertices included) */
  uint64_t max_height;      /* the dendrogram's height in merges: the longest chain of parents */
  uint32_t levels;          /* contraction levels that held an edge */
  uint32_t rounds;          /* data-dependent doubling / jumping rounds */
  uint32_t is_forest;       /* 1 iff T closes no cycle */
  uint32_t reserved;        /* 0 */
  double   ms_total;        /* host wall time of the call */
} ghs_dendro_result_t;
size_t ghs_forest_dendro_workspace_bytes(uint32_t n, uint64_t m);   /* host only, no GPU needed */
int ghs_forest_dendro_device(uint32_t n, uint64_t m, const uint32_t *d_u, const uint32_t *d_v, const uint32_t *d_w,
                             const uint8_t *d_in_mst,
                             uint32_t *d_leaf_parent /* n */, uint32_t *d_merge_eid, uint32_t *d_merge_parent,
                             uint32_t *d_child_a /* may be NULL */, uint32_t *d_child_b /* may be NULL */,
                             uint32_t *d_size /* may be NULL */,
                             void *d_workspace, size_t workspace_bytes, void *stream,
                             ghs_dendro_result_t *result);
/* the same for host arrays (copy in, run, copy out on the default stream; child_a, child_b and size may
 * be NULL; nothing but leaf_parent is copied out when is_forest = 0); the argument errors above except
 * the alignments, then GHS_E_NODEVICE without a GPU */
int ghs_forest_dendro_host(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w,
                           const uint8_t *in_mst, uint32_t *leaf_parent, uint32_t *merge_eid, uint32_t *merge_parent,
                           uint32_t *child_a, uint32_t *child_b, uint32_t *size, ghs_dendro_result_t *result);

/* ---- HDBSCAN cluster extraction from the dendrogram (ABI 10 addition) ----------------------------------
 * The back half of HDBSCAN on a single-linkage dendrogram: the condensed tree for a min_cluster_size,
 * every cluster's stability, the excess-of-mass (or leaf) selection, and per vertex a label, noise (-1)
 * and a membership probability; scikit-learn's rule for its defaults (allow_single_cluster=False,
 * cluster_selection_epsilon=0, no max_cluster_size). Its special labelling of points that fall straight
 * out of a selected root under allow_single_cluster=True is not copied.
 * Input: a dendrogram as ghs_forest_dendro_device writes it (n, t, d_leaf_parent[n], d_merge_parent[t],
 * d_child_a[t], d_child_b[t], d_size[t]) and d_height[t]: one float64 height per merge, in merge order,
 * in the caller's own units. No edge list. Heights must be finite, > 0 and non-decreasing: a zero
 * height (an integer weight 0, duplicate points) is an error (GHS_E_ARG), not an infinite lambda.
 * Semantics, mcs = min_cluster_size >= 2, a vertex has size 1, lambda(j) = 1.0 / height[j] (IEEE):
 *   merge j is a true split iff both children have size >= mcs; a merge with size >= mcs is a cluster
 *   head iff it is the last merge of its tree or its parent is a true split. Clusters are the heads,
 *   numbered 0 .. K-1 by head merge index DESCENDING (a parent has a smaller id than its children);
 *   K <= cap = min(t, 2 floor(n / mcs)) = ghs_forest_cluster_capacity, the capacity of every cluster
 *   array; entries at index >= K are not written.
 *   d_cluster_head[c], d_cluster_parent[c] (0xffffffff: a tree top), d_cluster_size[c] = size[head],
 *   d_cluster_birth[c] = lambda(merge_parent[head]), 0.0 for a tree top: the trees of a forest are
 *   joined at infinite distance. A tree with < mcs vertices and an isolated vertex are noise.
 *   A vertex's anchor is its first ancestor merge with size >= mcs; d_point_cluster[v] = the cluster of
 *   the nearest ancestor-or-self head of the anchor (0xffffffff: none), d_point_lambda[v] =
 *   lambda(anchor) (0.0: none).
 *   stability(C) = sum over v with point_cluster C of (point_lambda[v] - birth(C))
 *                + sum over child clusters D of size(D) (birth(D) - birth(C)).
 *   EOM, bottom-up, s = the sum of best over the children (0 for a leaf): a tree top when it is the only
 *   one (num_top == 1) and GHS_CLUSTER_ALLOW_SINGLE is off is not chosen, best = s; else a leaf is
 *   chosen; else s > stability(C): best = s; else C is chosen, best = stability(C). GHS_CLUSTER_LEAF:
 *   the clusters without children are chosen (the lone-top rule applies the same). A cluster is selected
 *   iff it is chosen and no ancestor is. Selected clusters in id order are the labels 0 .. S-1;
 *   d_label[v] = the nearest selected ancestor-or-self of point_cluster[v], else -1.
 *   d_probability[v] = min(point_lambda[v], M) / M, M = the maximum over the selected cluster's own rows
 *   (the point_lambda of its own vertices, the birth of its child clusters); 1.0 if M == 0; 0.0 for noise.
 * d_probability and d_point_lambda may be NULL. Stabilities are summed in a fixed order (no floating-point
 * atomics): two calls give identical bytes in every array.
 * Validation, on the device, before anything follows a pointer: leaf_parent[v] is none or < t;
 * merge_parent[j] is none or j < merge_parent[j] < t; child_a[j] < child_b[j] < n + j; each child's parent
 * pointer is j; exactly 2 t nodes have a parent; size[j] is the sum of its children's sizes; the heights
 * as above. What passes is acyclic; anything else: GHS_E_ARG, nothing indexed out of bounds.
 * Method (csrc/cluster.hip): heads and anchors by one fused pointer doubling over merge_parent
 * (<= ceil(log2 t) + 1 rounds); cluster ids by a scan of the head flags; the vertices' lambdas sorted by
 * cluster (stable rocPRIM radix sort) and each segment summed by one wave (a block past 4096 rows) in a
 * fixed order; the EOM sweep over frontiers, synchronous in the condensed tree's height H_c only, one
 * launch per level while a frontier is wider than 1024 clusters and one single-workgroup launch for all
 * the remaining levels: select_launches <= min(H_c, ceil(K / 2048)) + 2; the topmost chosen ancestor by
 * pointer doubling over cluster_parent (<= ceil(log2 K) + 1 rounds). rounds counts both doublings.
 * Workspace (ghs_forest_cluster_workspace_bytes; it asks rocPRIM for its sort / scan storage, and that
 * query answers 0 on a host without a GPU: take the size on the machine that runs the call): 16 B per merge + 24 B per vertex + 84 B per
 * cluster of capacity + rocPRIM's sort / scan storage + 1 KiB of status.
 * Errors, checked before any device work (so they hold on a host without GPU): result NULL,
 * min_cluster_size < 2, unknown flags, n + t > 2^32 (node ids), NULL or misaligned pointers (4 bytes for
 * the 32-bit arrays, 8 for the float64 arrays, 16 for the workspace): GHS_E_ARG; workspace_bytes short:
 * GHS_E_NOMEM. n == 0: GHS_OK, nothing written. t == 0 (only label and point_cluster are needed) or
 * cap == 0: every vertex is noise, K = 0. One host sync per doubling round and per sweep launch. */
#define GHS_CLUSTER_ALLOW_SINGLE 1u   /* a lone tree top may be selected (allow_single_cluster) */
#define GHS_CLUSTER_LEAF 2u           /* cluster_selection_method = "leaf" instead of "eom" */
typedef struct ghs_cluster_result {   /* 40 bytes */
  uint32_t num_clusters;    /* K: clusters of the condensed tree */
  uint32_t num_selected;    /* S: labels are 0 .. S-1 */
  uint32_t num_noise;       /* vertices with label -1 */
  uint32_t num_top;         /* tree tops with >= min_cluster_size vertices */
  uint32_t cluster_height;  /* H_c: levels of the condensed tree (a leaf cluster alone: 1) */
  uint32_t rounds;          /* data-dependent doubling rounds (heads / anchors, selected ancestors) */
  uint32_t select_launches; /* launches of the selection sweep, the first frontier's included */
  uint32_t reserved;        /* 0 */
  double   ms_total;        /* host wall time of the call */
} ghs_cluster_result_t;
size_t ghs_forest_cluster_workspace_bytes(uint32_t n, uint64_t t, uint32_t min_cluster_size);  /* no device work */
uint64_t ghs_forest_cluster_capacity(uint32_t n, uint64_t t, uint32_t min_cluster_size);       /* host only */
int ghs_forest_cluster_device(uint32_t n, uint64_t t, const uint32_t *d_leaf_parent, const uint32_t *d_merge_parent,
                              const uint32_t *d_child_a, const uint32_t *d_child_b, const uint32_t *d_size,
                              const double *d_height, uint32_t min_cluster_size, uint32_t flags,
                              int32_t *d_label /* n */, double *d_probability /* n, may be NULL */,
                              uint32_t *d_point_cluster /* n */, double *d_point_lambda /* n, may be NULL */,
                              uint32_t *d_cluster_head /* cap */, uint32_t *d_cluster_parent, uint32_t *d_cluster_size,
                              double *d_cluster_birth, double *d_cluster_stability, uint8_t *d_cluster_selected,
                              void *d_workspace, size_t workspace_bytes, void *stream,
                              ghs_cluster_result_t *result);
/* the same for host arrays (copy in, run, copy out on the default stream); the argument errors above
 * except the alignments, then GHS_E_NODEVICE without a GPU */
int ghs_forest_cluster_host(uint32_t n, uint64_t t, const uint32_t *leaf_parent, const uint32_t *merge_parent,
                            const uint32_t *child_a, const uint32_t *child_b, const uint32_t *size, const double *height,
                            uint32_t min_cluster_size, uint32_t flags, int32_t *label, double *probability,
                            uint32_t *point_cluster, double *point_lambda, uint32_t *cluster_head, uint32_t *cluster_parent,
                            uint32_t *cluster_size, double *cluster_birth, double *cluster_stability,
                            uint8_t *cluster_selected, ghs_cluster_result_t *result);

/* ---- core distances and mutual reachability: which weights does HDBSCAN want? (ABI 10 addition) -----
 * HDBSCAN clusters the minimum spanning forest of the mutual-reachability weights, not of the weights
 * it is given: w_out[e] = max(core[u[e]], core[v[e]], w[e]), core[x] = the distance from x to its k-th
 * nearest neighbour (k = min_samples). On a canonical edge list (a k-NN graph, a sparse distance
 * matrix):
 *   deg(x)   the canonical edges with x at either end;
 *   core[x]  deg(x) >= k: the k-th smallest weight among the edges at x (k counts from 1, repeated
 *            weights count separately); 0 < deg(x) < k (a short row): the largest weight at x (k clamped
 *            to the degree); deg(x) == 0 (isolated): 0.
 * Any k >= 1. A k-th smallest element and a max are order statistics: exact on uint32, the same bytes on
 * every run, and they commute with the monotone rank map of rank-mapped weights. Only w changes, so the
 * re-weighted list is canonical with the same edge ids. d_w_out may be exactly d_w (in place) or NULL
 * (core distances only).
 * Method (csrc/mreach.hip). Rows: the forward row of x is the run of x in the sorted u (offsets by one
 * lower bound per vertex); the reverse row is the run of x in w sorted by v (stable rocPRIM pairs sort
 * over the bits of n, one lower bound per vertex). Select, by degree: below
 * GHS_MREACH_BLOCK_ROW_MIN the row stays in registers (4 values per lane; 8 lanes per row up to
 * GHS_MREACH_LANE_ROW_MAX, a wave above) and the k-th value is built bit by bit from the top with
 * ballots and popcounts; from GHS_MREACH_BLOCK_ROW_MIN one workgroup per row runs a four-pass 8-bit
 * radix select over an LDS histogram; from GHS_MREACH_GRID_ROW_MIN the rows are listed and every digit
 * pass histograms all of them with the whole grid (integer atomics: any order gives the same counts).
 * Re-weight: one streaming pass, four edges per lane. Host syncs: the canonicity check's and one more.
 * Workspace (ghs_mutual_reach_workspace_bytes): 8 B per vertex + 8 B per edge + rocPRIM's sort storage
 * + the row lists (4 B per GHS_MREACH_LANE_ROW_MAX + 1 edge ends and less) + 1 KiB + 12 B per possible
 * grid row. m == 0: 0.
 * Errors, checked before any device work (so GHS_E_ARG, not GHS_E_NODEVICE, on a host without GPU): a
 * NULL result, k == 0, m >= 2^31, NULL or misaligned pointers (16 bytes for u / v / w / w_out /
 * workspace, 4 for core), d_w_out overlapping d_w without being equal to it (or overlapping u, v or
 * core), d_core overlapping u, v or w: GHS_E_ARG; workspace_bytes short: GHS_E_NOMEM. n == 0: GHS_OK,
 * nothing written. m == 0, n > 0: every core is 0 and only d_core is needed. A non-canonical list
 * (ghs_check_canonical): GHS_E_NONCANON before any index is formed from it. */
#define GHS_MREACH_LANE_ROW_MAX 32u       /* up to here 8 lanes hold a row */
#define GHS_MREACH_BLOCK_ROW_MIN 256u     /* from here one workgroup selects a row (below: one wave at most) */
#define GHS_MREACH_GRID_ROW_MIN 32768u    /* from here every workgroup takes tiles of the row */
typedef struct ghs_mreach_result {   /* 48 bytes */
  uint64_t short_rows;      /* vertices with 0 < deg < k (k was clamped to the degree) */
  uint64_t isolated;        /* vertices with deg == 0 (core 0) */
  uint64_t raised_edges;    /* edges with w_out > w (0 when d_w_out is NULL) */
  uint32_t max_degree;
  uint32_t block_rows;      /* rows selected by one workgroup each */
  uint32_t grid_rows;       /* rows selected by the whole grid */
  uint32_t reserved;
  double   ms_total;        /* host wall time of the call */
} ghs_mreach_result_t;
size_t ghs_mutual_reach_workspace_bytes(uint32_t n, uint64_t m);   /* host only, no GPU needed */
int ghs_mutual_reach_device(uint32_t n, uint64_t m, const uint32_t *d_u, const uint32_t *d_v, const uint32_t *d_w,
                            uint32_t k, uint32_t *d_core /* n */,
                            uint32_t *d_w_out /* m; may be NULL; may be exactly d_w (in place) */,
                            void *d_workspace, size_t workspace_bytes, void *stream, ghs_mreach_result_t *result);
/* the same for host arrays (copy in, run, copy out on the default stream); the argument errors above
 * except the alignments and the workspace, then GHS_E_NODEVICE without a GPU */
int ghs_mutual_reach_host(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w, uint32_t k,
                          uint32_t *core, uint32_t *w_out, ghs_mreach_result_t *result);
/* opt-in HIP-event times of the calling thread's last ghs_mutual_reach_device: ms[3] = rows, select,
 * re-weight (read before `enable` takes effect for the next call); diagnostic */
int ghs_mutual_reach_phases(int enable, double *ms);

/* ---- k-NN graph: where does the edge list come from? (ABI 10 addition) --------------------------------
 * The exact k nearest neighbours of every row of an (n, dim) float32 array, by brute force: the front
 * of HDBSCAN on points. Row i of d_idx / d_dist holds the neighbours of point i.
 * Distance. d2(a, b) is the float32 value of the chain acc = 0; for t = 0 .. dim-1 in ascending order:
 * s = a[t] - b[t] (one rounding), acc = fmaf(s, s, acc). It is never negative, bit for bit symmetric in
 * (a, b), 0 for equal rows, and has no cancellation: its relative error against exact arithmetic is at
 * most (dim + 3) * 2^-23 (one rounding in s, one per fmaf, all terms >= 0, a factor 2 for the second
 * order). The form |a|^2 + |b|^2 - 2ab has none of these properties, and the f32 MFMA that would compute
 * it runs at the vector rate on gfx950 anyway.
 * Metric. GHS_KNN_SQEUCLIDEAN writes d2, GHS_KNN_EUCLIDEAN the correctly rounded sqrt(d2); the selection
 * is always on d2.
 * Neighbours of i: the k candidates j != i with the smallest 64-bit key (float_bits(d2(i, j)) << 32) | j
 * (non-negative floats order as their bits do). Keys are distinct, so the answer is unique: ties go to the
 * smaller index. i is excluded by index, never by distance: a duplicate of i is an ordinary neighbour at
 * distance 0. A row holds its neighbours in ascending key order.
 * Determinism. The output is a pure function of (x, k, metric): the same bytes for every `slices`, every
 * launch shape and every arrival order of candidates, and from call to call.
 * Method (csrc/knn.hip). One workgroup owns GHS_KNN_TILE_Q queries and sweeps the candidates of its
 * slice GHS_KNN_TILE_C at a time, both sides staged through LDS GHS_KNN_DIM_CHUNK dims at a time (tail
 * candidates and dims padded with zeros: fmaf(0, 0, acc) == acc), 4 x 4 accumulators per lane that see
 * the dims in ascending order. Per query a sorted list of k keys lives in LDS; a finished key that beats
 * the list's last entry goes to the query's LDS queue and is inserted. With slices > 1 every slice
 * writes its lists to the workspace and a merge kernel takes the k smallest. slices == 0: chosen from n
 * alone (a fixed target of workgroups, clamped to [1, GHS_KNN_MAX_SLICES]). Everything runs on `stream`;
 * one host sync per call. Workspace (ghs_knn_workspace_bytes): 256 B of status, and 8 B * slices * n * k
 * of keys when slices > 1.
 * Errors, checked before any device work (so GHS_E_ARG, not GHS_E_NODEVICE, on a host without GPU): a
 * NULL result; k == 0, k > GHS_KNN_MAX_K; dim == 0, dim > GHS_KNN_MAX_DIM; an unknown metric; slices >
 * GHS_KNN_MAX_SLICES; then, for n >= 1: k > n - 1; n * k >= 2^32; NULL pointers; misaligned pointers
 * (16 bytes for d_x and the workspace, 4 for d_idx / d_dist; the rows of d_x are only 4-byte aligned when
 * dim % 4 != 0); overlapping pointers: GHS_E_ARG; workspace_bytes short: GHS_E_NOMEM. n == 0: GHS_OK, no
 * device work, the pointers may be NULL. After the sync: a NaN or +-inf coordinate gives GHS_E_ARG
 * ("non-finite coordinate"); the outputs are then unspecified, nothing was read or written out of bounds
 * and no key was formed from a NaN. A d2 that overflows to +inf for finite coordinates is an ordinary
 * value. */
#define GHS_KNN_MAX_K      128u
#define GHS_KNN_MAX_DIM    4096u
#define GHS_KNN_MAX_SLICES 64u
#define GHS_KNN_SQEUCLIDEAN 0u
#define GHS_KNN_EUCLIDEAN   1u
#define GHS_KNN_TILE_Q     64u    /* queries of one workgroup */
#define GHS_KNN_TILE_C     64u    /* candidates of one sweep step */
#define GHS_KNN_DIM_CHUNK  32u    /* dims staged through LDS at a time */
typedef struct ghs_knn_result {   /* 48 bytes */
  uint64_t pairs;            /* ordered pairs evaluated: n * (n - 1) */
  uint64_t zero_neighbours;  /* entries of d_dist equal to 0: duplicate points among the neighbours */
  uint32_t slices;           /* candidate slices the scan ran with */
  uint32_t query_tiles;
  double   ms_total;         /* host wall time of the call */
  uint64_t reserved[2];      /* 0 */
} ghs_knn_result_t;
size_t ghs_knn_workspace_bytes(uint32_t n, uint32_t dim, uint32_t k, uint32_t slices);   /* host only, no GPU needed */
int ghs_knn_device(uint32_t n, uint32_t dim, const float *d_x /* n*dim, row-major */, uint32_t k,
                   uint32_t metric, uint32_t slices /* 0 = auto */,
                   uint32_t *d_idx /* n*k */, float *d_dist /* n*k */,
                   void *d_workspace, size_t workspace_bytes, void *stream, ghs_knn_result_t *result);
/* the same for host arrays (copy in, run, copy out on the default stream, slices = auto); the argument
 * errors above except the alignments and the workspace, then GHS_E_NODEVICE without a GPU */
int ghs_knn_host(uint32_t n, uint32_t dim, const float *x, uint32_t k, uint32_t metric,
                 uint32_t *idx, float *dist, ghs_knn_result_t *result);

/* device-side canonicity check: *ok = 1 iff u < v < n and (u, v) strictly ascending */
int ghs_check_canonical(uint32_t n, uint64_t m, const uint32_t *d_u, const uint32_t *d_v, void *stream, int *ok);

/* ---- exact MST from points: the tree the k-NN forest only approximates (ABI 10 addition) -----------------
 * The minimum spanning tree of the complete graph on the rows of an (n, dim) float32 array, exactly: the
 * Euclidean MST (single linkage on points), or with core distances the mutual-reachability MST that HDBSCAN
 * is defined on. No k, no forest: one tree of n - 1 edges.
 * Inputs. d_x: (n, dim) float32, row-major. d_core2: NULL, or n float32 SQUARED core distances, every value
 * finite and >= 0; NULL means all zero.
 * Weight. w2(i, j) = max(d2(i, j), core2[i], core2[j]) for the unordered pair {i, j}. d2 is bit for bit the
 * chain of ghs_knn_device: acc = 0; for t = 0 .. dim-1 in ascending order: s = a[t] - b[t] (one rounding),
 * acc = fmaf(s, s, acc). The max is taken on float32 values, so it is exact. A d2 that overflows to +inf for
 * finite coordinates is an ordinary value.
 * Order. The key of the pair (u, v), u < v, is the triple (float_bits(w2), u, v), compared
 * lexicographically: the (w, eid) key of this library on the canonical list of all n (n - 1) / 2 pairs.
 * Keys are distinct, so the MST is unique: the tree canonical Kruskal builds over all pairs in that order.
 * Output. The n - 1 tree edges as a canonical edge list: d_u[e] < d_v[e], (u, v) strictly ascending.
 * d_w[e] is float32: w2 for GHS_KNN_SQEUCLIDEAN, the correctly rounded sqrt(w2) for GHS_KNN_EUCLIDEAN.
 * Determinism. The output is a pure function of (x, core2, metric): the same bytes for every `slices`,
 * every launch shape and from call to call.
 * Method (csrc/emst.hip). Boruvka rounds, at most ceil(log2 n) of them (GHS_E_ROUNDCAP guards the loop). In
 * a round one brute-force sweep (the tile shape of ghs_knn_device: GHS_KNN_TILE_Q queries x GHS_KNN_TILE_C
 * candidates, GHS_KNN_DIM_CHUNK dims at a time) finds for every point i the smallest (float_bits(w2) << 32
 * | j) over the points j of another component, kept in registers and combined by one 64-bit atomicMin per
 * query and slice: for a fixed i that is also i's smallest pair key, because among equal weights any j < i
 * beats every j > i and a smaller j beats a larger one. Two passes over the points reduce them to each
 * component's smallest 96-bit key; a component hooks to the component of its edge's far end (of a mutual
 * pair the smaller label stays root and only it emits the edge), pointer jumping makes stars. One host sync
 * per round brings back the edge count. A pairs sort by u << 32 | v fixes the byte order, a last pass writes
 * d_w. Integer atomics only. `slices`: 0 = chosen from n alone, as ghs_knn_device does.
 * Workspace (ghs_emst_workspace_bytes): 256 B of status, 28 B per point, 24 B per edge, the sort's scratch.
 * Errors, checked before any device work (so GHS_E_ARG, not GHS_E_NODEVICE, on a host without GPU): a NULL
 * result; dim == 0, dim > GHS_KNN_MAX_DIM; an unknown metric; slices > GHS_KNN_MAX_SLICES; then n == 0:
 * GHS_OK, no device work, the pointers may be NULL; n == 1: GHS_OK, zero edges, d_u / d_v / d_w may be NULL;
 * then n - 1 >= 2^31; NULL pointers (d_core2 may be NULL); misaligned pointers (16 bytes for d_x and the
 * workspace, 4 for the rest); overlapping pointers: GHS_E_ARG; workspace_bytes short: GHS_E_NOMEM. Checked on
 * the device before any key is formed: a NaN or +-inf coordinate gives GHS_E_ARG ("non-finite coordinate"),
 * a core2 that is NaN, infinite or negative GHS_E_ARG ("bad core distance"); the outputs are then
 * unspecified and nothing was read or written out of bounds. */
typedef struct ghs_emst_result {   /* 64 bytes */
  uint64_t num_edges;        /* n - 1 */
  uint64_t pairs;            /* ordered pairs evaluated, summed over rounds: rounds * n * (n - 1) */
  uint64_t zero_edges;       /* tree edges of weight 0: duplicate points */
  uint32_t rounds;           /* Boruvka rounds, <= ceil(log2 n) */
  uint32_t slices;           /* candidate slices every round's sweep ran with */
  uint32_t query_tiles;
  uint32_t reserved0;        /* 0 */
  uint64_t components_after_first_round;
  double   ms_total;         /* host wall time of the call */
  uint64_t reserved[1];      /* 0 */
} ghs_emst_result_t;
size_t ghs_emst_workspace_bytes(uint32_t n, uint32_t dim, uint32_t slices);   /* host only, no GPU needed */
int ghs_emst_device(uint32_t n, uint32_t dim, const float *d_x /* n*dim, row-major */,
                    const float *d_core2 /* n squared core distances, may be NULL */,
                    uint32_t metric, uint32_t slices /* 0 = auto */,
                    uint32_t *d_u /* n-1 */, uint32_t *d_v /* n-1 */, float *d_w /* n-1 */,
                    void *d_workspace, size_t workspace_bytes, void *stream, ghs_emst_result_t *result);
/* the same for host arrays (copy in, run, copy out on the default stream, slices = auto); the argument
 * errors above except the 16-byte alignment and the workspace, then GHS_E_NODEVICE without a GPU */
int ghs_emst_host(uint32_t n, uint32_t dim, const float *x, const float *core2 /* may be NULL */, uint32_t metric,
                  uint32_t *u, uint32_t *v, float *w, ghs_emst_result_t *result);
/* the rounds of the calling thread's last ghs_emst_device: *rounds = their number, components[r] = the
 * components left after round r, scan_ms[r] = the HIP-event time of round r's sweep (0 unless the call ran
 * after ghs_emst_rounds(1, ...): `enable` takes effect for the next call); at most `capacity` entries are
 * written, any pointer may be NULL; diagnostic */
int ghs_emst_rounds(int enable, uint32_t capacity, uint32_t *components, double *scan_ms, uint32_t *rounds);

/* ---- stepwise solver (multi-GPU: one process per GPU, RCCL all-reduce between steps) ------
 * Replaces the per-rank protocol loop of ghs_implementation_mpi.py:673-748 and its
 * collectives (:907 bcast, :929 Barrier, :766 gather). Every rank holds the replicated
 * canonical list and owns the contiguous edge range [e_lo, e_hi); per round it scans the arcs of
 * ITS edges and the per-fragment best keys are combined with an all-reduce MIN by the caller:
 *   h = ghs_solver_create(...)
 *   loop: rc = ghs_solver_minedge(h, &C)       local min-edge per fragment (opens levels)
 *         while rc == GHS_NEED_EXCHANGE:       a level was opened (several ranks): its active
 *           <caller: all_reduce(flags, MAX)>     fragments = those with a level edge on ANY rank
 *           rc = ghs_solver_minedge(h, &C)       (ghs_solver_exchange_buffer: n uint8 flags)
 *         ghs_solver_pack_best(h, d_dense)     C int64 slots, order-preserving (key ^ 2^63)
 *         <caller: all_reduce(d_dense[0:C], MIN)>
 *         ghs_solver_unpack_best(h, d_dense)
 *         ghs_solver_contract(h, &done)        hook + pointer-jump + next fragment list
 *   ghs_solver_finish(h, result, stats); ghs_solver_destroy(h)
 * Identical inputs on every rank => identical hook decisions => identical totals (ghs_solver_finish)
 * on every rank. MSF flags are owner-written: a solver clears and writes d_in_mst[e] only for its
 * own range e in [e_lo, e_hi) and never touches the rest, so the MSF is the concatenation of the
 * ranks' slices (an all-gather of [e_lo, e_hi) from every rank; the reference gathered BRANCH
 * edges to rank 0, ghs_implementation_mpi.py:760-779).
 * Errors: a rank that finds its edge range non-canonical records it in the exchanged flag
 * buffer (its last byte), so after the caller's MAX every rank returns GHS_E_NONCANON from the
 * same ghs_solver_minedge call — no rank is left waiting in a collective. */
typedef struct ghs_solver ghs_solver_t;
int ghs_solver_create(uint32_t n, uint64_t m, const uint32_t *d_u, const uint32_t *d_v, const uint32_t *d_w,
                      uint64_t e_lo, uint64_t e_hi, const ghs_config_t *cfg, void *d_workspace,
                      size_t workspace_bytes, uint8_t *d_in_mst, void *stream, ghs_solver_t **out);
/* ABI 9: a rank of the same loop over the CSR form (d_off, optional d_u; see ghs_mst_device_csr) */
int ghs_solver_create_csr(uint32_t n, uint64_t m, const uint32_t *d_off, const uint32_t *d_u, const uint32_t *d_v,
                          const uint32_t *d_w, uint64_t e_lo, uint64_t e_hi, const ghs_config_t *cfg, void *d_workspace,
                          size_t workspace_bytes, uint8_t *d_in_mst, void *stream, ghs_solver_t **out);
/* runs the min-edge kernel; *num_active = fragments whose best slot must be all-reduced */
int ghs_solver_minedge(ghs_solver_t *h, uint64_t *num_active);
/* the flag array to OR-combine (uint8 MAX all-reduce) after GHS_NEED_EXCHANGE: n fragment flags
 * + 1 error byte (*bytes = n + 1) */
int ghs_solver_exchange_buffer(ghs_solver_t *h, uint8_t **d_flags, uint64_t *bytes);
/* the same exchange as bitmaps (half the wire bytes of the MAX all-reduce per rank): flag_bits
 * packs the n + 1 flags into *words uint64 words; the caller all-gathers every rank's words
 * (rank-major, nranks x words) and hands the gathered buffer to merge_flag_bits (OR), then calls
 * ghs_solver_minedge again — instead of exchange_buffer + MAX all-reduce */
int ghs_solver_flag_bits(ghs_solver_t *h, uint64_t **d_bits, uint64_t *words);
int ghs_solver_merge_flag_bits(ghs_solver_t *h, const uint64_t *d_all, uint32_t nranks);
int ghs_solver_pack_best(ghs_solver_t *h, int64_t *d_dense);
int ghs_solver_unpack_best(ghs_solver_t *h, const int64_t *d_dense);
/* optional, instead of pack_best / int64 MIN / unpack_best: a dense level's first round keeps its
 * *count slots contiguous in the solver's own minima (identity order), so the caller may MIN
 * all-reduce *d_slots in place as UNSIGNED 64-bit (ncclUint64 + ncclMin). *d_slots = NULL: this
 * round needs pack / unpack. (ghs_solver_run uses it; ABI 4 addition) */
int ghs_solver_best_slots(ghs_solver_t *h, uint64_t **d_slots, uint64_t *count);
/* optional, after unpack_best (a level's first round, several ranks): owner-computes CONNECT.
 * Each rank hooks the fragments whose winning edge it holds and fills *count int32 slots
 * (par ^ fragment, 0 where another rank owns the winner); the caller all-reduces them with MAX
 * and hands them to unpack_hook, after which contract skips its own hook. *count = 0: not
 * applicable this round (contract hooks in fragment form, as without the call). Replaces the
 * per-fragment gathers of the fragment-form hook with 4 bytes per active fragment on the wire.
 * The MSF flag of such a hook is set only on the rank that owns the edge (as every flag: see
 * above); the totals of ghs_solver_finish are complete on every rank. */
int ghs_solver_hook_local(ghs_solver_t *h, int32_t *d_dense, uint64_t *count);
int ghs_solver_unpack_hook(ghs_solver_t *h, const int32_t *d_dense);
/* optional (ABI 6), a dense level's opening round instead of best_slots / MIN all-reduce /
 * hook_local / MAX all-reduce / unpack_hook — half the wire of a ring all-reduce per slot, the
 * reference's collect of the CONNECT decisions (ghs_implementation_mpi.py:582-671) as 16 bytes:
 *   hook_slots(h, N, &slots, &S)      S = 0: not applicable this round (use the calls above);
 *                                     else `slots` = S uint64 (a multiple of N, padding = UINT64_MAX)
 *   <caller: reduce-scatter MIN (uint64, in place): rank r keeps slots[r*S/N, (r+1)*S/N)>
 *   hook_owner(h, r, S/N, pairs)      pairs[c] for the rank's slots: eid << 32 | the other dense
 *                                     fragment of c's minimum edge (UINT64_MAX: no edge); the ends
 *                                     come from the replicated canonical list
 *   <caller: all-gather the S/N-slot slices (in place into pairs, S uint64)>
 *   apply_hooks(h, pairs, &partial)   par for every fragment (a mutual pair stays a 2-cycle that the
 *                                     jump resolves: its smaller fragment keeps the root), the MSF
 *                                     flags of the rank's own edge range, and in `partial` (2 uint64,
 *                                     device) the weight and count of those own-range MSF edges
 *   <caller: all-reduce SUM (uint64) of partial, in place>
 * then contract as usual (it adds the summed partial totals to the solve's totals). (Replaces
 * 2(N-1)/N x 12 bytes per slot with (N-1)/N x 16, + 16 bytes.) */
int ghs_solver_hook_slots(ghs_solver_t *h, uint32_t nranks, uint64_t **d_slots, uint64_t *padded);
int ghs_solver_hook_owner(ghs_solver_t *h, uint32_t rank, uint64_t per_rank, uint64_t *d_pairs);
int ghs_solver_apply_hooks(ghs_solver_t *h, const uint64_t *d_pairs, uint64_t **d_partial);
/* optional (ABI 10), at the top of the loop (before minedge), several ranks: the LDS tail of a
 * dense level — its last rounds (ghs_implementation_mpi.py:673-748 once few fragments remain, the
 * REPORT / CHANGEROOT convergecasts of ghs_implementation.py:235-387) with the fragments renumbered
 * 0..F-1 and each round's minima kept in LDS, so a round moves 12 bytes per fragment on the wire
 * instead of a min-edge + hook over n-sized arrays:
 *   tail_begin(h, &F)              F = 0: not applicable now (call minedge as usual); else the tail
 *                                  opened and this rank's minima of its round 0 are in `keys`
 *   loop: tail_buffers(h, &keys, &hooks)    F uint64 keys, F int32 CONNECT targets (device)
 *     <caller: all-reduce MIN (UNSIGNED 64-bit) of keys[0:F], in place>
 *     tail_agree(h)                the owner of each minimum keeps its target and writes the MSF
 *                                  flag of its own edge; the other ranks withdraw theirs (-1)
 *     <caller: all-reduce MAX (int32) of hooks[0:F], in place>
 *     tail_round(h, &state)        the hooks applied, the next round streamed (one host sync);
 *                                  state 0: the next round's minima are in keys (loop); 1: the level
 *                                  is complete (continue with minedge); 2: so is the solve (finish)
 * Every rank takes the same branch (the counts are identical on every rank). ghs_solver_run runs the
 * same tail with its own collectives (several rounds per host sync). */
int ghs_solver_tail_begin(ghs_solver_t *h, uint64_t *num_fragments);
int ghs_solver_tail_buffers(ghs_solver_t *h, uint64_t **d_keys, int32_t **d_hooks);
int ghs_solver_tail_agree(ghs_solver_t *h);
int ghs_solver_tail_round(ghs_solver_t *h, int *state);
/* hook + jump + next list; *done = 1 when every level is complete */
int ghs_solver_contract(ghs_solver_t *h, int *done);
int ghs_solver_finish(ghs_solver_t *h, ghs_result_t *result, ghs_round_stats_t *stats);
/* start the next solve of the same inputs on the same handle (keeps the workspace layout and the
 * pinned host resources: a multi-GPU caller's per-solve create/destroy becomes one reset) */
int ghs_solver_reset(ghs_solver_t *h);
/* thread-safe, callable while another thread is inside ghs_solver_run (ABI 5): a rank whose peer
 * failed ends its waits — the call in progress returns GHS_E_STATE instead of waiting forever
 * behind a collective the peer never joins (DistributedMST: a watchdog thread calls it when
 * another rank reports a failure). The handle is then only good for reset or destroy. */
int ghs_solver_cancel(ghs_solver_t *h);
int ghs_solver_destroy(ghs_solver_t *h);

/* ---- the round loop in the library --------------------------------------------------------
 * ghs_solver_run drives the loop above to completion on the solver's stream — minedge, the
 * level-flag bitmap all-gather, pack / int64 MIN / unpack, the owner-computed hooks' int32 MAX,
 * contract — with the collectives of `comm` enqueued on that same stream (RCCL): one host call
 * per solve instead of ~6 library calls + 2-3 collective launches per round from the caller.
 * comm: one per rank from ghs_comm_init, after rank 0's ghs_comm_unique_id has reached every
 * rank (torch.distributed / MPI broadcast of GHS_COMM_ID_BYTES bytes); NULL for a single-rank
 * solver. Collective: every rank calls it; then ghs_solver_finish as usual. The communicator is
 * bound to the device current at ghs_comm_init and keeps its own device scratch (grown on demand,
 * n-sized). */
#define GHS_COMM_ID_BYTES 128
typedef struct ghs_comm ghs_comm_t;
int ghs_comm_unique_id(uint8_t *id);
int ghs_comm_init(int nranks, int rank, const uint8_t *id, ghs_comm_t **out);
int ghs_comm_destroy(ghs_comm_t *comm);
int ghs_solver_run(ghs_solver_t *h, ghs_comm_t *comm);
/* Test / diagnostic entry: the ghs_solver_run loop of a num_ranks-GPU solve, every rank on the
 * CURRENT device (one host thread and stream per rank, in-process collectives with the same
 * semantics as RCCL's) — exercises the exact multi-rank loop on one GPU. Device pointers; every
 * rank writes its own range of d_in_mst (m flags). result/stats: rank 0's (checked equal on every
 * rank). */
int ghs_mst_emulated(uint32_t n, uint64_t m, const uint32_t *d_u, const uint32_t *d_v, const uint32_t *d_w,
                     int num_ranks, const ghs_config_t *cfg, uint8_t *d_in_mst, ghs_result_t *result,
                     ghs_round_stats_t *stats);

/* ABI 8 diagnostic: round reports whose sequence number the host read before every field had
 * landed (the checksum of the report failed and the host polled again), since the process started */
int ghs_slot_retries(uint64_t *count);

/* ---- per-launch profile ------------------------------------------------------------------
 * The reference measured only wall time (time.time(), ghs_implementation.py:453-464,
 * ghs_implementation_mpi.py:920-933). With profiling on, every kernel launch of later solves is
 * bracketed by two HIP events on the solve's stream and its duration lands in a process-wide
 * list (read and drained by ghs_profile_read). The events idle the GPU ~6 us each between
 * launches: profile a separate solve, not the timed ones. */
enum ghs_kernel_id {
  GHS_K_SELECT = 0, GHS_K_FILTER, GHS_K_LEVEL_PASS, GHS_K_SEED_RUNS, GHS_K_MINEDGE_IDENT, GHS_K_MINEDGE_COMPACT,
  GHS_K_WIN, GHS_K_HOOK, GHS_K_JUMP_IDENT, GHS_K_JUMP, GHS_K_SELECT_LB, GHS_K_RESOLVE, GHS_K_GIANT, GHS_K_SCAN,
  GHS_K_PLAN, GHS_K_INIT, GHS_K_PACK, GHS_K_UNPACK, GHS_K_ROUND_REPORT, GHS_K_PACK_HOOK, GHS_K_UNPACK_HOOK,
  GHS_K_DENSE, GHS_K_FLAG_BITS, GHS_K_BUCKET, GHS_K_BMIN, GHS_K_WSTARTS, GHS_K_WMIN, GHS_K_HOT_HOOK,
  GHS_K_TAIL_OPEN, GHS_K_TAIL_ROUND, GHS_K_TAIL_HOOK, GHS_K_CSR_TROW /* ABI 9 */, GHS_K_COUNT
};
typedef struct ghs_kernel_record {
  uint32_t kernel;  /* ghs_kernel_id */
  uint32_t round;   /* round index (all levels) when launched; a lookahead no-op round past a
                       level's end reuses the next level's index with its own (older) level */
  uint32_t level;   /* weight level when launched */
  uint32_t solver;  /* the launching solver handle (creation order in the process) */
  uint64_t items;   /* host-known work count at launch (edges / vertices / fragments), 0 = unknown */
  float ms;         /* event-to-event duration */
  float reserved2;
} ghs_kernel_record_t;
int ghs_profile_enable(int on);  /* also clears the list */
int ghs_profile_read(ghs_kernel_record_t *out, uint32_t capacity, uint32_t *count);
const char *ghs_kernel_name(uint32_t kernel);

/* ---- synthetic graph generators (device; BASELINE.json configs 3-5) ----------------------
 * R-MAT (Graph500 A,B,C,D = .57,.19,.19,.05, edgefactor ef, 2^scale vertices, seeded vertex
 * permutation), self-loops dropped, duplicates removed, canonical order, unique weights
 * w = bijective_hash32(eid ^ wseed) (distinct by construction). d_u/d_v/d_w must hold
 * edgefactor * 2^scale entries (the tuple count, an upper bound); *m_out = canonical edge count.
 * d_temp: ghs_rmat_temp_bytes(scale, edgefactor) bytes. */
size_t ghs_rmat_temp_bytes(uint32_t scale, uint32_t edgefactor);
int ghs_rmat_generate(uint32_t scale, uint32_t edgefactor, uint64_t seed, uint64_t wseed,
                      uint32_t *d_u, uint32_t *d_v, uint32_t *d_w, uint64_t *m_out,
                      void *d_temp, size_t temp_bytes, void *stream);
/* The raw R-MAT tuples of ghs_rmat_generate before its canonical sort/dedupe (generator parity
 * tests): d_keys[t] = min << scale | max of tuple t, or 2^(2 scale) - 1 for a self-loop;
 * edgefactor * 2^scale entries. */
int ghs_rmat_tuples(uint32_t scale, uint32_t edgefactor, uint64_t seed, uint64_t *d_keys, void *stream);
/* k x k grid, vertex r*k+c, right + down edges (m = 2k(k-1)), canonical order.
 * mode 0: unique hashed weights; mode 1: "road-like" gradient weights w = eid (unique, forces
 * long hook chains). */
int ghs_grid_generate(uint32_t k, uint32_t mode, uint64_t wseed, uint32_t *d_u, uint32_t *d_v, uint32_t *d_w,
                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GHS_MST_H */
