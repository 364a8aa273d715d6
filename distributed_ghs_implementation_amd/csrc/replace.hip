// Replacement edges of the rooted forest (ABI 10 addition, ghs_forest_replace_*): for every forest
// edge the lightest non-forest edge that reconnects the two halves when it fails. The opposite
// question to the path query, which looks from a non-forest edge into the forest; the same pass gives
// the bridges of the graph (forest edges nothing replaces), the forest edges a lighter edge replaces
// (the flags are then not the MSF) and the cheapest swap: the second-best spanning forest.
//
// The reference is a protocol for networks whose links fail (ghs_implementation.py:235-387 rebuilds
// from scratch); this is the sensitivity half of that question, answered for every link at once.
//
// A non-root vertex x stands for its parent edge. A non-forest edge f = (a, b) inside one tree covers
// the forest edges of the path a .. b; repl[x] is the smallest key w[f] << 32 | f over the edges that
// cover x's edge, UINT64_MAX for a root or when nothing covers it. Walking every path edge by edge
// would cost the depth per edge (forests here are tens of thousands deep), so the cover is left on
// power-of-two ranges instead: cover[j][x] = "the 2^j forest edges going up from x are covered by
// this key". Level 0 is the caller's output array; levels 1 .. K - 1 live in the workspace.
//   cover      one pass over the m edges. The meeting point of a and b is found with the lift-then-
//              descend walk of the path query (without its keys), four edges per lane advancing
//              together; it gives L_a = depth[a] - depth[lca] and L_b. An end z with L > 0 and j =
//              floor(log2 L) leaves the key at cover[j][z] and at cover[j][z'], z' = z lifted by
//              L - 2^j through that number's set bits: two ranges of 2^j edges that overlap and together
//              are exactly the L edges.
//   push-down  j = K - 1 .. 1, one launch per level over n, stream-ordered: a set cover[j][x] is
//              min-ed into cover[j-1][x] and cover[j-1][up_{j-1}(x)].
//   finish     roots to UINT64_MAX, the optional per-edge scatter, the counts and the best swap.
// Every minimum is a read-checked atomicMin: the slot is read first and the atomic skipped when it
// already holds a key that is not larger. Slots only ever decrease, so a stale read is never smaller
// than the slot and a skipped atomic is always a correct skip. Integer minima commute: the output is
// byte-identical from run to run. One host sync, at the end, for the status block; no loop's trip
// count depends on unvalidated data (depths and up pointers come from the index, which its level-0
// pass validated; edge endpoints are range-checked here before they index anything).
//
// This translation unit includes common.h only, launches only its own kernels and reaches the index
// through ghs_forest_paths_info.
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>

#include "common.h"

namespace ghs {
namespace replace {

constexpr int RP_BLOCK = 256;
constexpr int RP_EPL = 4;  // edges per lane
constexpr uint64_t RP_TILE = (uint64_t)RP_BLOCK * RP_EPL;  // edges per block
constexpr uint32_t RP_NONE = 0xffffffffu;
constexpr uint64_t RP_UNSET = ~0ull;
constexpr size_t RP_STATUS_BYTES = 256;

// status block (uint64 slots, device): the last 256 bytes of the workspace. The counters are zeroed,
// ST_BEST starts at all ones (an atomicMin slot), ST_BEST_IN is written by at most one lane.
enum { ST_BAD = 0, ST_TREE, ST_COVERING, ST_CROSS, ST_BRIDGES, ST_IMPROVING, ST_COUNTERS, ST_BEST = ST_COUNTERS, ST_BEST_IN, ST_SLOTS };

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static inline uint32_t levels_for(uint64_t max_depth) {
  uint32_t b = 0;
  while (b < 64 && (max_depth >> b)) ++b;
  return b ? b : 1;
}

static inline size_t cover_bytes(uint32_t n, uint32_t levels) {
  return align256((size_t)8 * (levels ? levels - 1 : 0) * n);
}

static inline unsigned grid_for(uint64_t items, unsigned per_block, unsigned cap = 2048) {
  uint64_t g = (items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

static inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

__device__ __forceinline__ uint64_t key_of(const u32x4 q) { return ((uint64_t)q.y << 32) | q.x; }

__device__ __forceinline__ uint32_t block_sum(uint32_t c, uint32_t *s_w) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x / 64] = c;
  __syncthreads();
  uint32_t t = 0;
#pragma unroll
  for (int w = 0; w < RP_BLOCK / 64; ++w) t += s_w[w];
  __syncthreads();
  return t;
}

__device__ __forceinline__ uint64_t block_min64(uint64_t c, uint64_t *s_w) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint64_t o = __shfl_xor(c, d);
    c = o < c ? o : c;
  }
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x / 64] = c;
  __syncthreads();
  uint64_t t = RP_UNSET;
#pragma unroll
  for (int w = 0; w < RP_BLOCK / 64; ++w) t = s_w[w] < t ? s_w[w] : t;
  __syncthreads();
  return t;
}

// cover[j][x]: level 0 is the output array, level j >= 1 the workspace's slab j - 1
__device__ __forceinline__ uint64_t *slot(uint64_t *__restrict__ repl, uint64_t *__restrict__ upper, uint32_t n, uint32_t j,
                                          uint32_t x) {
  return j ? upper + (uint64_t)(j - 1) * n + x : repl + x;
}

// read-checked minimum: slots only decrease, so a stale read is never below the slot
__device__ __forceinline__ void min_into(uint64_t *p, uint64_t key) {
  if (*p > key) atomicMin((unsigned long long *)p, (unsigned long long)key);
}

// ---- cover: every non-forest edge leaves its key on at most four power-of-two ranges -------------------
// Lane t of block g owns edges g * 1024 + j * 256 + t, j = 0 .. 3 (coalesced 4-byte loads of u, v, w).
// An edge that is finished, a forest edge or out of range keeps loading node 0 of level 0: one cached
// address for the whole wave.
__global__ __launch_bounds__(RP_BLOCK) void k_rp_cover(uint32_t n, uint32_t K, uint64_t m, const uint32_t *__restrict__ eu,
                                                       const uint32_t *__restrict__ ev, const uint32_t *__restrict__ ew,
                                                       const u32x4 *__restrict__ idx, uint64_t *__restrict__ repl,
                                                       uint64_t *__restrict__ upper, uint64_t *__restrict__ status) {
  __shared__ uint32_t s_w[RP_BLOCK / 64];
  const uint64_t e0 = blockIdx.x * RP_TILE + threadIdx.x;
  uint32_t a[RP_EPL], b[RP_EPL], x[RP_EPL], y[RP_EPL], da[RP_EPL], db[RP_EPL], diff[RP_EPL], cd[RP_EPL];
  int lvl[RP_EPL];
  bool live[RP_EPL], found[RP_EPL], skip[RP_EPL];  // skip: a forest edge, or an endpoint out of range
  uint32_t badid = 0, covering = 0, cross = 0;
#pragma unroll
  for (int j = 0; j < RP_EPL; ++j) {
    const uint64_t e = e0 + (uint64_t)j * RP_BLOCK;
    const bool valid = e < m;
    a[j] = valid ? eu[e] : 0u;
    b[j] = valid ? ev[e] : 0u;
    live[j] = valid;
    skip[j] = false;
    if (a[j] >= n || b[j] >= n) {
      badid = 1;
      a[j] = b[j] = 0;
      live[j] = false;
      skip[j] = true;
    }
    found[j] = false;
    diff[j] = 0;
    cd[j] = 0;
    lvl[j] = 0;
    da[j] = db[j] = 0;
  }
  // both ends' level-0 nodes: the depths, and whether this edge is a forest edge
  {
    u32x4 ea[RP_EPL], eb[RP_EPL];
#pragma unroll
    for (int j = 0; j < RP_EPL; ++j) {
      ea[j] = idx[a[j]];
      eb[j] = idx[b[j]];
    }
#pragma unroll
    for (int j = 0; j < RP_EPL; ++j) {
      x[j] = a[j];
      y[j] = b[j];
      if (!live[j]) continue;
      const uint32_t e = (uint32_t)(e0 + (uint64_t)j * RP_BLOCK);
      if ((ea[j].x == e && ea[j].z != a[j]) || (eb[j].x == e && eb[j].z != b[j])) {  // some end's parent edge
        live[j] = false;
        skip[j] = true;
        continue;
      }
      da[j] = ea[j].w;
      db[j] = eb[j].w;
      if (a[j] == b[j]) {  // a loop covers nothing (canonical lists have none)
        found[j] = true;
        cd[j] = da[j];
        live[j] = false;
        continue;
      }
      if (da[j] < db[j]) {  // x is the deeper end
        x[j] = b[j];
        y[j] = a[j];
      }
      diff[j] = da[j] < db[j] ? db[j] - da[j] : da[j] - db[j];
      cd[j] = da[j] < db[j] ? da[j] : db[j];
    }
  }
  // lift the deeper end by the set bits of the depth difference (bits below K: depths <= max_depth)
  for (;;) {
    bool any = false;
#pragma unroll
    for (int j = 0; j < RP_EPL; ++j) any |= live[j] && diff[j] != 0;
    if (!any) break;
    u32x4 e[RP_EPL];
#pragma unroll
    for (int j = 0; j < RP_EPL; ++j) {
      const bool act = live[j] && diff[j] != 0;
      const uint32_t k = act ? (uint32_t)__ffs(diff[j]) - 1u : 0u;
      e[j] = idx[(uint64_t)k * n + (act ? x[j] : 0u)];
    }
#pragma unroll
    for (int j = 0; j < RP_EPL; ++j) {
      if (!(live[j] && diff[j] != 0)) continue;
      x[j] = e[j].z;
      diff[j] &= diff[j] - 1;
    }
  }
#pragma unroll
  for (int j = 0; j < RP_EPL; ++j) {
    if (!live[j]) continue;
    if (x[j] == y[j]) {  // one end is an ancestor of the other: the meeting point is at depth cd
      found[j] = true;
      live[j] = false;
    } else if (cd[j] == 0) {  // two different roots
      live[j] = false;
    } else {
      const int top = 32 - __clz(cd[j]);
      lvl[j] = (top < (int)K ? top : (int)K) - 1;
    }
  }
  // levels lvl .. 1 from the top: both ends jump where their targets differ
  for (;;) {
    bool any = false;
#pragma unroll
    for (int j = 0; j < RP_EPL; ++j) any |= live[j] && lvl[j] >= 1;
    if (!any) break;
    u32x4 ex[RP_EPL], ey[RP_EPL];
#pragma unroll
    for (int j = 0; j < RP_EPL; ++j) {
      const bool act = live[j] && lvl[j] >= 1;
      const uint64_t base = act ? (uint64_t)lvl[j] * n : 0ull;
      ex[j] = idx[base + (act ? x[j] : 0u)];
      ey[j] = idx[base + (act ? y[j] : 0u)];
    }
#pragma unroll
    for (int j = 0; j < RP_EPL; ++j) {
      if (!(live[j] && lvl[j] >= 1)) continue;
      if (ex[j].z != ey[j].z) {
        x[j] = ex[j].z;
        y[j] = ey[j].z;
      }
      --lvl[j];
    }
  }
  // level 0: the ends are now one or two steps below the meeting point, or in different trees
#pragma unroll 1
  for (int step = 0; step < 2; ++step) {
    bool any = false;
#pragma unroll
    for (int j = 0; j < RP_EPL; ++j) any |= live[j];
    if (!any) break;
    u32x4 ex[RP_EPL], ey[RP_EPL];
#pragma unroll
    for (int j = 0; j < RP_EPL; ++j) {
      ex[j] = idx[live[j] ? x[j] : 0u];
      ey[j] = idx[live[j] ? y[j] : 0u];
    }
#pragma unroll
    for (int j = 0; j < RP_EPL; ++j) {
      if (!live[j]) continue;
      if (ex[j].z == ey[j].z) {  // a common parent (two roots differ: each is its own target)
        cd[j] = ex[j].w - 1;     // x's depth - 1: the meeting point's depth
        found[j] = true;
        live[j] = false;
      } else {
        x[j] = ex[j].z;
        y[j] = ey[j].z;
      }
    }
  }
  // the ranges: end z with L edges up to the meeting point -> cover[jl][z] and cover[jl][z lifted by L - 2^jl]
  constexpr int RP_ENDS = 2 * RP_EPL;
  uint32_t z[RP_ENDS], rem[RP_ENDS], jl[RP_ENDS];
  uint64_t key[RP_ENDS];
  bool act[RP_ENDS];
#pragma unroll
  for (int j = 0; j < RP_EPL; ++j) {
    const uint64_t e = e0 + (uint64_t)j * RP_BLOCK;
    const bool valid = e < m;
    const bool inside = found[j];
    covering += inside;
    cross += valid && !inside && !skip[j];  // no meeting point: the ends are in different trees
    const uint64_t k = inside ? ((uint64_t)ew[e] << 32) | (uint32_t)e : RP_UNSET;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int t = 2 * j + s;
      const uint32_t L = inside ? (s ? db[j] : da[j]) - cd[j] : 0u;
      z[t] = s ? b[j] : a[j];
      act[t] = L != 0;
      jl[t] = act[t] ? 31u - (uint32_t)__clz(L) : 0u;
      rem[t] = act[t] ? L - (1u << jl[t]) : 0u;
      key[t] = k;
      if (act[t]) min_into(slot(repl, upper, n, jl[t], z[t]), k);
      act[t] = act[t] && rem[t] != 0;  // L a power of two: the second range is the first
    }
  }
  for (;;) {
    bool any = false;
#pragma unroll
    for (int t = 0; t < RP_ENDS; ++t) any |= act[t] && rem[t] != 0;
    if (!any) break;
    u32x4 e[RP_ENDS];
#pragma unroll
    for (int t = 0; t < RP_ENDS; ++t) {
      const bool go = act[t] && rem[t] != 0;
      const uint32_t k = go ? (uint32_t)__ffs(rem[t]) - 1u : 0u;  // rem < 2^jl: every bit is below jl < K
      e[t] = idx[(uint64_t)k * n + (go ? z[t] : 0u)];
    }
#pragma unroll
    for (int t = 0; t < RP_ENDS; ++t) {
      if (!(act[t] && rem[t] != 0)) continue;
      z[t] = e[t].z;
      rem[t] &= rem[t] - 1;
    }
  }
#pragma unroll
  for (int t = 0; t < RP_ENDS; ++t)
    if (act[t]) min_into(slot(repl, upper, n, jl[t], z[t]), key[t]);
  const uint32_t cv = block_sum(covering, s_w), cr = block_sum(cross, s_w), bd = block_sum(badid, s_w);
  if (threadIdx.x == 0) {
    if (cv) atomicAdd((unsigned long long *)(status + ST_COVERING), (unsigned long long)cv);
    if (cr) atomicAdd((unsigned long long *)(status + ST_CROSS), (unsigned long long)cr);
    if (bd) atomicMax((unsigned long long *)(status + ST_BAD), 1ull);
  }
}

// ---- push-down: level j into level j - 1 ----------------------------------------------------------------
// up: level j - 1 of the index (the 2^(j-1)-ancestors); hi = cover[j], lo = cover[j-1]
__global__ __launch_bounds__(RP_BLOCK) void k_rp_push(uint32_t n, const u32x4 *__restrict__ up, const uint64_t *__restrict__ hi,
                                                      uint64_t *__restrict__ lo) {
  for (uint64_t x = blockIdx.x * (uint64_t)RP_BLOCK + threadIdx.x; x < n; x += (uint64_t)gridDim.x * RP_BLOCK) {
    const uint64_t c = hi[x];
    if (c == RP_UNSET) continue;
    const uint32_t t = up[x].z;
    min_into(lo + x, c);
    if (t < n) min_into(lo + t, c);  // always: the index holds only ids below n
  }
}

// ---- finish: roots, the per-edge scatter, the counts, the best swap ---------------------------------------
// best swap key: (delta + 2^32) << 31 | out eid, delta = w[repl] - w[e] in (-2^32, 2^32), eid < 2^31
__global__ __launch_bounds__(RP_BLOCK) void k_rp_finish(uint32_t n, uint64_t m, const u32x4 *__restrict__ lv0,
                                                        uint64_t *__restrict__ repl, uint32_t *__restrict__ by_edge,
                                                        uint64_t *__restrict__ status) {
  __shared__ uint32_t s_w[RP_BLOCK / 64];
  __shared__ uint64_t s_m[RP_BLOCK / 64];
  uint32_t tree = 0, bridges = 0, improving = 0;
  uint64_t best = RP_UNSET;
  for (uint64_t x = blockIdx.x * (uint64_t)RP_BLOCK + threadIdx.x; x < n; x += (uint64_t)gridDim.x * RP_BLOCK) {
    const u32x4 node = lv0[x];
    if (node.z == (uint32_t)x) {  // a root stands for no edge
      repl[x] = RP_UNSET;
      continue;
    }
    const uint64_t r = repl[x], own = key_of(node);
    ++tree;
    if (by_edge && node.x < m) by_edge[node.x] = r == RP_UNSET ? RP_NONE : (uint32_t)r;
    if (r == RP_UNSET) {
      ++bridges;
      continue;
    }
    improving += r < own;
    const uint64_t shifted = (uint64_t)((int64_t)(r >> 32) - (int64_t)(own >> 32) + (1ll << 32));
    const uint64_t k = (shifted << 31) | node.x;
    best = k < best ? k : best;
  }
  const uint32_t t = block_sum(tree, s_w), b = block_sum(bridges, s_w), im = block_sum(improving, s_w);
  const uint64_t bm = block_min64(best, s_m);
  if (threadIdx.x == 0) {
    if (t) atomicAdd((unsigned long long *)(status + ST_TREE), (unsigned long long)t);
    if (b) atomicAdd((unsigned long long *)(status + ST_BRIDGES), (unsigned long long)b);
    if (im) atomicAdd((unsigned long long *)(status + ST_IMPROVING), (unsigned long long)im);
    if (bm != RP_UNSET && status[ST_BEST] > bm) atomicMin((unsigned long long *)(status + ST_BEST), (unsigned long long)bm);
  }
}

// the incoming edge of the best swap: the one vertex whose parent edge is the winner writes it
__global__ __launch_bounds__(RP_BLOCK) void k_rp_pick(uint32_t n, const u32x4 *__restrict__ lv0,
                                                      const uint64_t *__restrict__ repl, uint64_t *__restrict__ status) {
  const uint64_t best = status[ST_BEST];
  if (best == RP_UNSET) return;
  const uint32_t out = (uint32_t)(best & 0x7fffffffu);
  for (uint64_t x = blockIdx.x * (uint64_t)RP_BLOCK + threadIdx.x; x < n; x += (uint64_t)gridDim.x * RP_BLOCK) {
    const u32x4 node = lv0[x];
    if (node.z != (uint32_t)x && node.x == out) status[ST_BEST_IN] = repl[x] & 0xffffffffull;
  }
}

}  // namespace replace
}  // namespace ghs

using namespace ghs;
using namespace ghs::replace;

namespace {
// opt-in HIP-event times of the last call's phases on this thread (ghs_forest_replace_phases)
thread_local bool t_phases_on = false;
thread_local double t_phase_ms[4] = {0, 0, 0, 0};  // init, cover, push-down, finish

struct PhaseEvents {
  hipEvent_t ev[5] = {};
  int made = 0;
  bool on = false;
  int start(bool enable) {
    on = enable;
    if (!on) return GHS_OK;
    for (; made < 5; ++made) GHS_HIP_CHECK(hipEventCreate(&ev[made]));
    return GHS_OK;
  }
  int mark(int k, hipStream_t st) {
    if (on) GHS_HIP_CHECK(hipEventRecord(ev[k], st));
    return GHS_OK;
  }
  int read(double *ms) {  // after the stream synchronise
    if (!on) return GHS_OK;
    for (int k = 0; k < 4; ++k) {
      float f = 0.f;
      GHS_HIP_CHECK(hipEventElapsedTime(&f, ev[k], ev[k + 1]));
      ms[k] = f;
    }
    return GHS_OK;
  }
  ~PhaseEvents() {
    for (int k = 0; k < made; ++k) (void)hipEventDestroy(ev[k]);
  }
};
}  // namespace

extern "C" {

int ghs_forest_replace_phases(int enable, double *ms) {
  if (ms)
    for (int k = 0; k < 4; ++k) ms[k] = t_phase_ms[k];
  t_phases_on = enable != 0;
  return GHS_OK;
}

size_t ghs_forest_replace_workspace_bytes(uint32_t n, uint64_t max_depth) {
  return cover_bytes(n, levels_for(max_depth)) + RP_STATUS_BYTES;
}

int ghs_forest_replace_device(ghs_paths_t *h, uint64_t m, const uint32_t *d_u, const uint32_t *d_v, const uint32_t *d_w,
                              uint64_t *d_repl, uint32_t *d_repl_eid_by_edge, void *d_workspace, size_t workspace_bytes,
                              void *stream, ghs_replace_result_t *result) {
  hipStream_t st = (hipStream_t)stream;
  ghs_paths_info_t pi;
  if (ghs_forest_paths_info(h, &pi) != GHS_OK) GHS_FAIL(GHS_E_ARG, "handle is NULL or destroyed");
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_replace_result_t{};
  result->best_out_eid = result->best_in_eid = RP_NONE;
  if (m >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "m must be < 2^31");
  const uint32_t n = (uint32_t)pi.n, K = (uint32_t)pi.levels;
  // u, v, w are touched only at an index e < m and d_repl only at a vertex x < n
  if ((n && !d_repl) || !d_workspace || (m && (!d_u || !d_v || !d_w))) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if (m && (((uintptr_t)d_u | (uintptr_t)d_v | (uintptr_t)d_w) & 15)) GHS_FAIL(GHS_E_ARG, "u, v and w must be 16-byte aligned");
  if ((uintptr_t)d_workspace & 15) GHS_FAIL(GHS_E_ARG, "the workspace must be 16-byte aligned");
  if ((uintptr_t)d_repl & 7) GHS_FAIL(GHS_E_ARG, "repl must be 8-byte aligned");
  if ((uintptr_t)d_repl_eid_by_edge & 3) GHS_FAIL(GHS_E_ARG, "repl_eid_by_edge must be 4-byte aligned");
  if (workspace_bytes < cover_bytes(n, K) + RP_STATUS_BYTES) GHS_FAIL(GHS_E_NOMEM, "workspace too small");
  if (n == 0) {  // no slot to write; any edge's endpoints are out of range
    if (m) GHS_FAIL(GHS_E_ARG, "edge endpoint out of range");
    return GHS_OK;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");
  const auto t0 = std::chrono::steady_clock::now();
  const size_t cb = cover_bytes(n, K);
  uint64_t *upper = (uint64_t *)d_workspace;
  uint64_t *status = (uint64_t *)((char *)d_workspace + cb);
  const u32x4 *idx = (const u32x4 *)pi.d_index;
  const unsigned vgrid = grid_for(n, RP_BLOCK);
  uint64_t hst[ST_SLOTS] = {};
  PhaseEvents pe;
  if (int e = pe.start(t_phases_on)) return e;
  if (int e = pe.mark(0, st)) return e;
  // every cover slot and the best-swap slot start at all ones, the counters at zero
  GHS_HIP_CHECK(hipMemsetAsync(d_repl, 0xff, (size_t)n * 8, st));
  GHS_HIP_CHECK(hipMemsetAsync(d_workspace, 0xff, cb + RP_STATUS_BYTES, st));
  GHS_HIP_CHECK(hipMemsetAsync(status, 0, (size_t)ST_COUNTERS * 8, st));
  if (d_repl_eid_by_edge && m) GHS_HIP_CHECK(hipMemsetAsync(d_repl_eid_by_edge, 0xff, (size_t)m * 4, st));
  if (int e = pe.mark(1, st)) return e;
  if (m) {
    const unsigned grid = (unsigned)((m + RP_TILE - 1) / RP_TILE);  // <= 2^21
    k_rp_cover<<<grid, RP_BLOCK, 0, st>>>(n, K, m, d_u, d_v, d_w, idx, d_repl, upper, status);
  }
  if (int e = pe.mark(2, st)) return e;
  if (m) {
    for (uint32_t j = K - 1; j >= 1; --j)
      k_rp_push<<<vgrid, RP_BLOCK, 0, st>>>(n, idx + (size_t)(j - 1) * n, upper + (size_t)(j - 1) * n,
                                            j >= 2 ? upper + (size_t)(j - 2) * n : d_repl);
  }
  if (int e = pe.mark(3, st)) return e;
  k_rp_finish<<<vgrid, RP_BLOCK, 0, st>>>(n, m, idx, d_repl, m ? d_repl_eid_by_edge : nullptr, status);
  k_rp_pick<<<vgrid, RP_BLOCK, 0, st>>>(n, idx, d_repl, status);
  GHS_HIP_CHECK(hipGetLastError());
  if (int e = pe.mark(4, st)) return e;
  GHS_HIP_CHECK(hipMemcpyAsync(hst, status, sizeof(hst), hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipStreamSynchronize(st));
  if (int e = pe.read(t_phase_ms)) return e;
  if (hst[ST_BAD]) GHS_FAIL(GHS_E_ARG, "edge endpoint out of range");
  result->tree_edges = hst[ST_TREE];
  result->covering_edges = hst[ST_COVERING];
  result->cross_edges = hst[ST_CROSS];
  result->bridges = (uint32_t)hst[ST_BRIDGES];
  result->improving = (uint32_t)hst[ST_IMPROVING];
  if (hst[ST_BEST] != RP_UNSET) {
    result->best_delta = (int64_t)(hst[ST_BEST] >> 31) - (1ll << 32);
    result->best_out_eid = (uint32_t)(hst[ST_BEST] & 0x7fffffffu);
    result->best_in_eid = (uint32_t)hst[ST_BEST_IN];
  }
  result->ms_total = ms_since(t0);
  return GHS_OK;
}

}  // extern "C"
