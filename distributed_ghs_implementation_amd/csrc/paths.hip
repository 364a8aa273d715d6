// Path queries on the rooted forest (ABI 10 addition, ghs_forest_paths_*): for a pair (a, b) the
// heaviest edge on the forest path between them (the minimax / bottleneck distance, the edge a new
// edge (a, b, w) would displace, the single-linkage merge height), their lowest common ancestor and
// the number of edges between them.
//
// The reference's nodes answer such questions by walking in_branch towards the core (the REPORT /
// CHANGEROOT convergecasts, ghs_implementation.py:235-387). This is the device form of that walk, in
// O(log depth) dependent loads per query at any depth: jump pointers over parent / parent_eid / depth
// as ghs_forest_root_device writes them.
//
// Index: K = max(1, bit_length(max_depth)) levels of n 16-byte nodes {key, up, aux}:
//   level 0   up = parent (the vertex itself for a root), key = w[parent_eid] << 32 | parent_eid (0 for
//             a root), aux = depth;
//   level k   up_k[v] = up_{k-1}[up_{k-1}[v]], key_k[v] = max(key_{k-1}[v], key_{k-1}[up_{k-1}[v]]),
//             aux = depth again: one launch per level, stream-ordered, no host sync between them.
// A root points at itself with key 0, so a jump past a root stays on the root and adds nothing to a
// maximum. Key 0 is also the key of edge 0 with weight 0: the query decides a == b before it looks at
// any key, and every other connected pair has at least one edge on its path.
// The level-0 pass validates the caller's arrays before they become gather indices: a vertex is a root
// (parent == parent_eid == 0xffffffff, depth 0) or has parent < n, parent_eid < m, {u[e], v[e]} ==
// {v, parent}, depth == depth[parent] + 1 and depth <= max_depth. Depth falls by one along every
// parent pointer, so the structure is acyclic and every chain ends in a root after at most max_depth
// steps: no later loop depends on trust. A vertex that fails is written as a root (every index stays in
// range) and the call returns GHS_E_ARG after its one sync.
//
// Query (k_pa_query): 4 queries per lane, advanced together, so up to 8 independent 16-byte node
// loads are in flight per lane. Per pair: both level-0 nodes (the depths); the deeper end is lifted by
// the set bits of the depth difference, lowest first; if the ends differ, levels
// bit_length(common depth) - 1 .. 1 are tried from the top, both ends jumping where their targets
// differ; one or two level-0 steps finish: the ends are then children of the LCA (equal level-0
// targets) or two distinct roots. hops comes from the jump counts.
//
// This translation unit includes common.h only and launches only its own kernels.
#include <hip/hip_runtime.h>

#include <chrono>
#include <new>
#include <string>

#include "common.h"

namespace ghs {
namespace paths {

constexpr int PA_BLOCK = 256;
constexpr int PA_QPL = 4;  // queries per lane
constexpr uint64_t PA_QTILE = (uint64_t)PA_BLOCK * PA_QPL;  // queries per block
constexpr uint32_t PA_NONE = 0xffffffffu;
constexpr uint32_t PA_MAGIC = 0x50415448u;
constexpr size_t PA_STATUS_BYTES = 256;

// status block (uint64 slots, device): the last 256 bytes of the index
enum { ST_BAD = 0, ST_ROOTS, ST_MAXDEPTH, ST_QBAD, ST_CONNECTED, ST_SLOTS };

// a node as one 16-byte load: x, y = key (low, high word), z = up, w = aux
__device__ __forceinline__ uint64_t key_of(const u32x4 q) { return ((uint64_t)q.y << 32) | q.x; }
__device__ __forceinline__ uint64_t max64(uint64_t a, uint64_t b) { return a > b ? a : b; }

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static inline uint32_t levels_for(uint64_t max_depth) {
  uint32_t b = 0;
  while (b < 64 && (max_depth >> b)) ++b;
  return b ? b : 1;
}

static inline size_t levels_bytes(uint32_t n, uint64_t max_depth) {
  return align256((size_t)16 * levels_for(max_depth) * n);
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

__device__ __forceinline__ uint32_t block_sum(uint32_t c, uint32_t *s_w) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x / 64] = c;
  __syncthreads();
  uint32_t t = 0;
#pragma unroll
  for (int w = 0; w < PA_BLOCK / 64; ++w) t += s_w[w];
  __syncthreads();
  return t;
}

__device__ __forceinline__ uint32_t block_max(uint32_t c, uint32_t *s_w) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t o = __shfl_xor(c, d);
    c = o > c ? o : c;
  }
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x / 64] = c;
  __syncthreads();
  uint32_t t = 0;
#pragma unroll
  for (int w = 0; w < PA_BLOCK / 64; ++w) t = s_w[w] > t ? s_w[w] : t;
  __syncthreads();
  return t;
}

// ---- level 0: validate parent / parent_eid / depth, write the first level, count the roots -----------
// u, v, w are touched only at an index e < m, so they may be NULL when m == 0.
__global__ __launch_bounds__(PA_BLOCK) void k_pa_level0(uint32_t n, uint64_t m, const uint32_t *__restrict__ u,
                                                        const uint32_t *__restrict__ v, const uint32_t *__restrict__ w,
                                                        const uint32_t *__restrict__ parent,
                                                        const uint32_t *__restrict__ parent_eid,
                                                        const uint32_t *__restrict__ depth, uint64_t max_depth,
                                                        u32x4 *__restrict__ lv0, uint64_t *__restrict__ status) {
  __shared__ uint32_t s_w[PA_BLOCK / 64];
  uint32_t roots = 0, deepest = 0, bad = 0;
  for (uint64_t x = blockIdx.x * (uint64_t)PA_BLOCK + threadIdx.x; x < n; x += (uint64_t)gridDim.x * PA_BLOCK) {
    const uint32_t p = parent[x], e = parent_eid[x], d = depth[x];
    u32x4 node = {0u, 0u, (uint32_t)x, 0u};  // a root; also what a vertex that fails becomes
    if (p == PA_NONE && e == PA_NONE && d == 0) {
      ++roots;
    } else {
      bool ok = p < n && e < m && d <= max_depth;
      if (ok) {
        const uint32_t ue = u[e], ve = v[e];
        ok = ((ue == x && ve == p) || (ue == p && ve == x)) && (uint64_t)depth[p] + 1 == d;
      }
      if (ok) {
        node.x = e;
        node.y = w[e];
        node.z = p;
        node.w = d;
        deepest = d > deepest ? d : deepest;
      } else {
        bad = 1;
      }
    }
    lv0[x] = node;
  }
  const uint32_t r = block_sum(roots, s_w), dm = block_max(deepest, s_w), b = block_max(bad, s_w);
  if (threadIdx.x == 0) {
    if (r) atomicAdd((unsigned long long *)(status + ST_ROOTS), (unsigned long long)r);
    if (dm) atomicMax((unsigned long long *)(status + ST_MAXDEPTH), (unsigned long long)dm);
    if (b) atomicMax((unsigned long long *)(status + ST_BAD), 1ull);
  }
}

// ---- level k from level k - 1 ---------------------------------------------------------------------------
__global__ __launch_bounds__(PA_BLOCK) void k_pa_level(uint32_t n, const u32x4 *__restrict__ prev,
                                                       u32x4 *__restrict__ cur) {
  for (uint64_t x = blockIdx.x * (uint64_t)PA_BLOCK + threadIdx.x; x < n; x += (uint64_t)gridDim.x * PA_BLOCK) {
    const u32x4 a = prev[x];
    const uint32_t up = a.z < n ? a.z : (uint32_t)x;  // never: level 0 wrote every up below n
    const u32x4 b = prev[up];
    const uint64_t k = max64(key_of(a), key_of(b));
    u32x4 node = {(uint32_t)k, (uint32_t)(k >> 32), b.z, a.w};
    cur[x] = node;
  }
}

// ---- the queries -----------------------------------------------------------------------------------------
// Lane t of block g owns queries g * 1024 + j * 256 + t, j = 0 .. 3: the loads of a / b and the stores
// of the outputs are coalesced 4-byte accesses, so slices at any 4-byte offset work. A query that is
// finished (or out of range) keeps loading node 0 of level 0: one cached address for the whole wave.
__global__ __launch_bounds__(PA_BLOCK) void k_pa_query(uint32_t n, uint32_t K, uint64_t Q, const uint32_t *__restrict__ qa,
                                                       const uint32_t *__restrict__ qb, const u32x4 *__restrict__ idx,
                                                       uint64_t *__restrict__ okey, uint32_t *__restrict__ olca,
                                                       uint32_t *__restrict__ ohops, uint64_t *__restrict__ status) {
  __shared__ uint32_t s_w[PA_BLOCK / 64];
  const uint64_t q0 = blockIdx.x * PA_QTILE + threadIdx.x;
  uint32_t x[PA_QPL], y[PA_QPL], diff[PA_QPL], hops[PA_QPL], lca[PA_QPL], cdep[PA_QPL];
  uint64_t key[PA_QPL];
  int lvl[PA_QPL];
  bool live[PA_QPL];
  uint32_t badid = 0;
#pragma unroll
  for (int j = 0; j < PA_QPL; ++j) {
    const uint64_t q = q0 + (uint64_t)j * PA_BLOCK;
    const bool valid = q < Q;
    x[j] = valid ? qa[q] : 0u;
    y[j] = valid ? qb[q] : 0u;
    live[j] = valid;
    if (x[j] >= n || y[j] >= n) {
      badid = 1;
      x[j] = y[j] = 0;
      live[j] = false;
    }
    key[j] = ~0ull;
    lca[j] = PA_NONE;
    hops[j] = PA_NONE;
    diff[j] = 0;
    cdep[j] = 0;
    lvl[j] = 0;
  }
  // both ends' depths
  {
    u32x4 ex[PA_QPL], ey[PA_QPL];
#pragma unroll
    for (int j = 0; j < PA_QPL; ++j) {
      ex[j] = idx[x[j]];
      ey[j] = idx[y[j]];
    }
#pragma unroll
    for (int j = 0; j < PA_QPL; ++j) {
      if (!live[j]) continue;
      if (x[j] == y[j]) {  // decided before any key is looked at
        lca[j] = x[j];
        hops[j] = 0;
        live[j] = false;
        continue;
      }
      uint32_t dx = ex[j].w, dy = ey[j].w;
      if (dx < dy) {
        const uint32_t t = x[j];
        x[j] = y[j];
        y[j] = t;
        const uint32_t s = dx;
        dx = dy;
        dy = s;
      }
      diff[j] = dx - dy;
      hops[j] = diff[j];  // the lift's part of the hop count
      cdep[j] = dy;
      key[j] = 0;
    }
  }
  // lift the deeper end x by the set bits of the depth difference (bits below K: depths <= max_depth)
  for (;;) {
    bool any = false;
#pragma unroll
    for (int j = 0; j < PA_QPL; ++j) any |= live[j] && diff[j] != 0;
    if (!any) break;
    u32x4 e[PA_QPL];
#pragma unroll
    for (int j = 0; j < PA_QPL; ++j) {
      const bool act = live[j] && diff[j] != 0;
      const uint32_t k = act ? (uint32_t)__ffs(diff[j]) - 1u : 0u;
      e[j] = idx[(uint64_t)k * n + (act ? x[j] : 0u)];
    }
#pragma unroll
    for (int j = 0; j < PA_QPL; ++j) {
      if (!(live[j] && diff[j] != 0)) continue;
      key[j] = max64(key[j], key_of(e[j]));
      x[j] = e[j].z;
      diff[j] &= diff[j] - 1;
    }
  }
#pragma unroll
  for (int j = 0; j < PA_QPL; ++j) {
    if (!live[j]) continue;
    if (x[j] == y[j]) {  // b was an ancestor of a (or the other way round)
      lca[j] = y[j];
      live[j] = false;
    } else if (cdep[j] == 0) {  // two different roots
      key[j] = ~0ull;
      hops[j] = PA_NONE;
      live[j] = false;
    } else {
      // below the LCA the ends are at most cdep - 1 steps away: bits below bit_length(cdep)
      const int top = 32 - __clz(cdep[j]);
      lvl[j] = (top < (int)K ? top : (int)K) - 1;
    }
  }
  // levels lvl .. 1 from the top: both ends jump where their targets differ
  for (;;) {
    bool any = false;
#pragma unroll
    for (int j = 0; j < PA_QPL; ++j) any |= live[j] && lvl[j] >= 1;
    if (!any) break;
    u32x4 ex[PA_QPL], ey[PA_QPL];
#pragma unroll
    for (int j = 0; j < PA_QPL; ++j) {
      const bool act = live[j] && lvl[j] >= 1;
      const uint64_t base = act ? (uint64_t)lvl[j] * n : 0ull;
      ex[j] = idx[base + (act ? x[j] : 0u)];
      ey[j] = idx[base + (act ? y[j] : 0u)];
    }
#pragma unroll
    for (int j = 0; j < PA_QPL; ++j) {
      if (!(live[j] && lvl[j] >= 1)) continue;
      if (ex[j].z != ey[j].z) {
        key[j] = max64(key[j], max64(key_of(ex[j]), key_of(ey[j])));
        x[j] = ex[j].z;
        y[j] = ey[j].z;
        hops[j] += 2u << lvl[j];
      }
      --lvl[j];
    }
  }
  // level 0: the ends are now one or two steps below the LCA, or in different trees
#pragma unroll 1
  for (int step = 0; step < 2; ++step) {
    bool any = false;
#pragma unroll
    for (int j = 0; j < PA_QPL; ++j) any |= live[j];
    if (!any) break;
    u32x4 ex[PA_QPL], ey[PA_QPL];
#pragma unroll
    for (int j = 0; j < PA_QPL; ++j) {
      ex[j] = idx[live[j] ? x[j] : 0u];
      ey[j] = idx[live[j] ? y[j] : 0u];
    }
#pragma unroll
    for (int j = 0; j < PA_QPL; ++j) {
      if (!live[j]) continue;
      key[j] = max64(key[j], max64(key_of(ex[j]), key_of(ey[j])));
      hops[j] += 2;
      if (ex[j].z == ey[j].z) {
        lca[j] = ex[j].z;
        live[j] = false;
      } else {
        x[j] = ex[j].z;
        y[j] = ey[j].z;
      }
    }
  }
  uint32_t connected = 0;
#pragma unroll
  for (int j = 0; j < PA_QPL; ++j) {
    const uint64_t q = q0 + (uint64_t)j * PA_BLOCK;
    if (live[j]) {  // still apart after the last step: different trees
      key[j] = ~0ull;
      hops[j] = PA_NONE;
    }
    if (q < Q) {
      if (okey) okey[q] = key[j];
      if (olca) olca[q] = lca[j];
      if (ohops) ohops[q] = hops[j];
      connected += lca[j] != PA_NONE;
    }
  }
  const uint32_t c = block_sum(connected, s_w), b = block_max(badid, s_w);
  if (threadIdx.x == 0) {
    if (c) atomicAdd((unsigned long long *)(status + ST_CONNECTED), (unsigned long long)c);
    if (b) atomicMax((unsigned long long *)(status + ST_QBAD), 1ull);
  }
}

}  // namespace paths
}  // namespace ghs

using namespace ghs;
using namespace ghs::paths;

// host handle over the caller's index memory
struct ghs_paths {
  uint32_t magic;
  uint32_t n;
  uint32_t levels;
  uint64_t max_depth;
  char *index;
  uint64_t *status;
};

extern "C" {

size_t ghs_forest_paths_index_bytes(uint32_t n, uint64_t max_depth) {
  return levels_bytes(n, max_depth) + PA_STATUS_BYTES;
}

int ghs_forest_paths_create(uint32_t n, uint64_t m, const uint32_t *d_u, const uint32_t *d_v, const uint32_t *d_w,
                            const uint32_t *d_parent, const uint32_t *d_parent_eid, const uint32_t *d_depth,
                            uint64_t max_depth, void *d_index, size_t index_bytes, void *stream,
                            ghs_paths_result_t *result, ghs_paths_t **out) {
  hipStream_t st = (hipStream_t)stream;
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_paths_result_t{};
  if (!out) GHS_FAIL(GHS_E_ARG, "out is NULL");
  *out = nullptr;
  if (m >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "m must be < 2^31");
  if (n) {
    if (max_depth >= n) GHS_FAIL(GHS_E_ARG, "max_depth must be < n");
    if (!d_parent || !d_parent_eid || !d_depth || !d_index) GHS_FAIL(GHS_E_ARG, "NULL pointer");
    if (((uintptr_t)d_parent | (uintptr_t)d_parent_eid | (uintptr_t)d_depth) & 3)
      GHS_FAIL(GHS_E_ARG, "parent, parent_eid and depth must be 4-byte aligned");
    if ((uintptr_t)d_index & 15) GHS_FAIL(GHS_E_ARG, "the index must be 16-byte aligned");
    if (m) {
      if (!d_u || !d_v || !d_w) GHS_FAIL(GHS_E_ARG, "NULL pointer");
      if (((uintptr_t)d_u | (uintptr_t)d_v | (uintptr_t)d_w) & 15) GHS_FAIL(GHS_E_ARG, "u, v and w must be 16-byte aligned");
    }
    if (index_bytes < ghs_forest_paths_index_bytes(n, max_depth)) GHS_FAIL(GHS_E_NOMEM, "index too small");
  }
  ghs_paths *h = new (std::nothrow) ghs_paths{};
  if (!h) GHS_FAIL(GHS_E_NOMEM, "out of host memory");
  h->magic = PA_MAGIC;
  h->n = n;
  h->levels = n ? levels_for(max_depth) : 0;
  h->max_depth = max_depth;
  if (n == 0) {  // nothing to index: every query id is out of range
    *out = h;
    return GHS_OK;
  }
  h->index = (char *)d_index;
  h->status = (uint64_t *)(h->index + levels_bytes(n, max_depth));
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    delete h;
    GHS_FAIL(GHS_E_NODEVICE, "no HIP device");
  }
  const auto t0 = std::chrono::steady_clock::now();
  const unsigned vgrid = grid_for(n, PA_BLOCK);
  uint64_t hst[ST_SLOTS] = {};
  auto enqueue = [&]() -> int {
    GHS_HIP_CHECK(hipMemsetAsync(h->status, 0, PA_STATUS_BYTES, st));
    u32x4 *lv = (u32x4 *)h->index;
    k_pa_level0<<<vgrid, PA_BLOCK, 0, st>>>(n, m, d_u, d_v, d_w, d_parent, d_parent_eid, d_depth, max_depth, lv,
                                            h->status);
    for (uint32_t k = 1; k < h->levels; ++k)
      k_pa_level<<<vgrid, PA_BLOCK, 0, st>>>(n, lv + (size_t)(k - 1) * n, lv + (size_t)k * n);
    GHS_HIP_CHECK(hipGetLastError());
    GHS_HIP_CHECK(hipMemcpyAsync(hst, h->status, sizeof(hst), hipMemcpyDeviceToHost, st));
    GHS_HIP_CHECK(hipStreamSynchronize(st));
    return GHS_OK;
  };
  if (int e = enqueue()) {
    delete h;
    return e;
  }
  if (hst[ST_BAD]) {
    delete h;
    GHS_FAIL(GHS_E_ARG, "not a rooted forest");
  }
  result->levels = h->levels;
  result->max_depth = hst[ST_MAXDEPTH];
  result->num_trees = hst[ST_ROOTS];
  result->index_bytes = ghs_forest_paths_index_bytes(n, max_depth);
  result->ms_total = ms_since(t0);
  *out = h;
  return GHS_OK;
}

int ghs_forest_paths_query(ghs_paths_t *h, uint64_t q, const uint32_t *d_a, const uint32_t *d_b, uint64_t *d_key,
                           uint32_t *d_lca, uint32_t *d_hops, void *stream, ghs_paths_query_result_t *result) {
  hipStream_t st = (hipStream_t)stream;
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_paths_query_result_t{};
  if (!h || h->magic != PA_MAGIC) GHS_FAIL(GHS_E_ARG, "handle is NULL or destroyed");
  if (q >= (1ull << 32)) GHS_FAIL(GHS_E_ARG, "q must be < 2^32");
  if (q == 0) return GHS_OK;
  if (!d_a || !d_b) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if (((uintptr_t)d_a | (uintptr_t)d_b | (uintptr_t)d_lca | (uintptr_t)d_hops) & 3)
    GHS_FAIL(GHS_E_ARG, "a, b, lca and hops must be 4-byte aligned");
  if ((uintptr_t)d_key & 7) GHS_FAIL(GHS_E_ARG, "key must be 8-byte aligned");
  result->queries = q;
  if (h->n == 0) GHS_FAIL(GHS_E_ARG, "vertex id out of range");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");
  const auto t0 = std::chrono::steady_clock::now();
  uint64_t hst[ST_SLOTS] = {};
  GHS_HIP_CHECK(hipMemsetAsync(h->status, 0, PA_STATUS_BYTES, st));
  const unsigned grid = (unsigned)((q + PA_QTILE - 1) / PA_QTILE);  // <= 2^22
  k_pa_query<<<grid, PA_BLOCK, 0, st>>>(h->n, h->levels, q, d_a, d_b, (const u32x4 *)h->index, d_key, d_lca, d_hops,
                                        h->status);
  GHS_HIP_CHECK(hipGetLastError());
  GHS_HIP_CHECK(hipMemcpyAsync(hst, h->status, sizeof(hst), hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipStreamSynchronize(st));
  if (hst[ST_QBAD]) GHS_FAIL(GHS_E_ARG, "vertex id out of range");
  result->connected = hst[ST_CONNECTED];
  result->ms_total = ms_since(t0);
  return GHS_OK;
}

int ghs_forest_paths_info(const ghs_paths_t *h, ghs_paths_info_t *out) {
  if (!h || h->magic != PA_MAGIC) GHS_FAIL(GHS_E_ARG, "handle is NULL or destroyed");
  if (!out) GHS_FAIL(GHS_E_ARG, "out is NULL");
  out->n = h->n;
  out->levels = h->levels;
  out->max_depth = h->max_depth;
  out->d_index = h->index;
  return GHS_OK;
}

int ghs_forest_paths_destroy(ghs_paths_t *h) {
  if (!h) return GHS_OK;
  if (h->magic != PA_MAGIC) GHS_FAIL(GHS_E_ARG, "handle is not a live ghs_paths_t");
  h->magic = 0;
  delete h;
  return GHS_OK;
}

}  // extern "C"
