// Tree distances on the rooted forest (ABI 10 addition, ghs_forest_wdepth_* / ghs_forest_dist_* /
// ghs_forest_edge_dist_* / ghs_forest_diameter_*): how far is it from a to b along the forest? The
// path query gives the heaviest edge between two vertices; this gives the sum of the edges, and from
// it the stretch of every graph edge over the forest and the diameter, the two far ends, the
// eccentricities and the centre of every tree.
//
// The reference's nodes know their level and their in_branch only (ghs_implementation.py:63,212); a
// user who wants a distance walks in_branch edge by edge. This is the device form of that walk at any
// depth.
//
//   wdepth     wd[v] = the sum of the weights from v to its root. Pointer doubling over the index's
//              own levels: with S_k[v] = the sum of the (up to) 2^k edges going up from v,
//              S_{k+1}[v] = S_k[v] + S_k[up_k[v]]. A root points at itself with key 0, and up_k of a
//              vertex with fewer than 2^k ancestors is its root, so a jump past a root adds S_k[root] =
//              0. Pass 0 forms S_1 from the level-0 nodes alone; passes 1 .. K - 1 ping-pong between
//              the output and one workspace slab, so that pass K - 1 lands in the output. 2^K >
//              max_depth: S_K is the whole sum. K launches over n, none over the depth.
//   distance   dist(a, b) = wd[a] + wd[b] - 2 wd[lca(a, b)]. The LCA walk is the path query's (lift
//              the deeper end by the set bits of the depth difference, descend from the top level where
//              the targets differ, one or two level-0 steps), without its keys, four pairs per lane
//              advancing together on 16-byte node loads; the three 8-byte gathers follow in the same
//              kernel. The same walk serves the pairs of a query, the graph's own edges and the sweeps.
//   diameter   non-negative weights make two sweeps exact on a tree: p = the vertex farthest from the
//              root, q = the vertex farthest from p, diameter = dist(p, q) and ecc[v] = max(dist(v, p),
//              dist(v, q)). Each arg-max is two launches over n: a maximum of the distance into the
//              root's slot, then a minimum of the vertex id among the vertices that attain it (a
//              63-bit distance and an id do not fit one 64-bit key). Ties go to the smallest id.
// Every maximum / minimum is read-checked: the slot is read first and the atomic skipped when it
// already holds a value that is not smaller / larger. Slots move one way only, so a stale read never
// hides a needed update. Integer maxima, minima and sums commute: the output is byte-identical from
// run to run. One host sync per call; no loop's trip count depends on unvalidated data (depths and up
// pointers come from the index, which its level-0 pass validated; the caller's ids are range-checked
// here before they index anything; wd values are only ever added, never used as indices).
//
// This translation unit includes common.h only, launches only its own kernels and reaches the index
// through ghs_forest_paths_info. The calls without a workspace keep their counters in the index's
// status block (the last 256 bytes of the index): the handle's one-call-at-a-time rule covers them.
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>

#include "common.h"

namespace ghs {
namespace dist {

constexpr int DS_BLOCK = 256;
constexpr int DS_QPL = 4;  // pairs per lane
constexpr uint64_t DS_TILE = (uint64_t)DS_BLOCK * DS_QPL;  // pairs per tile
constexpr uint32_t DS_NONE = 0xffffffffu;
constexpr uint64_t DS_INF = ~0ull;
constexpr size_t DS_STATUS_BYTES = 256;

// status block (uint64 slots, device). Counters and maxima start at zero, minima at all ones.
enum {
  ST_BAD = 0,
  ST_CONNECTED,  // pairs / edges with both ends in one tree
  ST_MAX,        // the largest finite distance; the largest diameter
  ST_SUM_LO,
  ST_SUM_HI,
  ST_SUM_W,
  ST_TIGHT,  // edges with dist == w
  ST_TREES,
  ST_ZEROED,             // slots below start at all ones
  ST_ARGMAX = ST_ZEROED,  // the smallest eid / root attaining ST_MAX
  ST_MINECC,
  ST_CENTER,
  ST_SLOTS
};

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

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
  for (int w = 0; w < DS_BLOCK / 64; ++w) t += s_w[w];
  __syncthreads();
  return t;
}

__device__ __forceinline__ uint64_t block_sum64(uint64_t c, uint64_t *s_m) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x / 64] = c;
  __syncthreads();
  uint64_t t = 0;
#pragma unroll
  for (int w = 0; w < DS_BLOCK / 64; ++w) t += s_m[w];
  __syncthreads();
  return t;
}

__device__ __forceinline__ uint64_t block_max64(uint64_t c, uint64_t *s_m) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint64_t o = __shfl_xor(c, d);
    c = o > c ? o : c;
  }
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x / 64] = c;
  __syncthreads();
  uint64_t t = 0;
#pragma unroll
  for (int w = 0; w < DS_BLOCK / 64; ++w) t = s_m[w] > t ? s_m[w] : t;
  __syncthreads();
  return t;
}

__device__ __forceinline__ uint64_t block_min64(uint64_t c, uint64_t *s_m) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint64_t o = __shfl_xor(c, d);
    c = o < c ? o : c;
  }
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x / 64] = c;
  __syncthreads();
  uint64_t t = DS_INF;
#pragma unroll
  for (int w = 0; w < DS_BLOCK / 64; ++w) t = s_m[w] < t ? s_m[w] : t;
  __syncthreads();
  return t;
}

// read-checked maximum / minimum: slots move one way only, so a stale read is never past the slot
__device__ __forceinline__ void max_into(uint64_t *p, uint64_t x) {
  if (*p < x) atomicMax((unsigned long long *)p, (unsigned long long)x);
}
__device__ __forceinline__ void min_into(uint64_t *p, uint64_t x) {
  if (*p > x) atomicMin((unsigned long long *)p, (unsigned long long)x);
}
__device__ __forceinline__ void min_into(uint32_t *p, uint32_t x) {
  if (*p > x) atomicMin(p, x);
}

// ---- the LCA walk of the path query, without its keys ---------------------------------------------------
// In: DS_QPL pairs x[j], y[j], both below n; live[j] marks the pairs to answer. Out: lca[j] = the lowest
// common ancestor, DS_NONE for a pair that was not live or whose ends are in different trees. x, y and
// live are used up. A pair that is finished keeps loading node 0 of level 0: one cached address for the
// whole wave.
__device__ __forceinline__ void lca_walk(uint32_t n, uint32_t K, const u32x4 *__restrict__ idx, uint32_t (&x)[DS_QPL],
                                         uint32_t (&y)[DS_QPL], bool (&live)[DS_QPL], uint32_t (&lca)[DS_QPL]) {
  uint32_t diff[DS_QPL], cdep[DS_QPL];
  int lvl[DS_QPL];
#pragma unroll
  for (int j = 0; j < DS_QPL; ++j) {
    lca[j] = DS_NONE;
    diff[j] = 0;
    cdep[j] = 0;
    lvl[j] = 0;
  }
  // both ends' depths
  {
    u32x4 ex[DS_QPL], ey[DS_QPL];
#pragma unroll
    for (int j = 0; j < DS_QPL; ++j) {
      ex[j] = idx[live[j] ? x[j] : 0u];
      ey[j] = idx[live[j] ? y[j] : 0u];
    }
#pragma unroll
    for (int j = 0; j < DS_QPL; ++j) {
      if (!live[j]) continue;
      if (x[j] == y[j]) {
        lca[j] = x[j];
        live[j] = false;
        continue;
      }
      uint32_t dx = ex[j].w, dy = ey[j].w;
      if (dx < dy) {  // x is the deeper end
        const uint32_t t = x[j];
        x[j] = y[j];
        y[j] = t;
        const uint32_t s = dx;
        dx = dy;
        dy = s;
      }
      diff[j] = dx - dy;
      cdep[j] = dy;
    }
  }
  // lift the deeper end by the set bits of the depth difference (bits below K: depths <= max_depth)
  for (;;) {
    bool any = false;
#pragma unroll
    for (int j = 0; j < DS_QPL; ++j) any |= live[j] && diff[j] != 0;
    if (!any) break;
    u32x4 e[DS_QPL];
#pragma unroll
    for (int j = 0; j < DS_QPL; ++j) {
      const bool act = live[j] && diff[j] != 0;
      uint32_t k = act ? (uint32_t)__ffs(diff[j]) - 1u : 0u;
      k = k < K ? k : K - 1;  // never: the index validated every depth against max_depth < 2^K
      e[j] = idx[(uint64_t)k * n + (act ? x[j] : 0u)];
    }
#pragma unroll
    for (int j = 0; j < DS_QPL; ++j) {
      if (!(live[j] && diff[j] != 0)) continue;
      x[j] = e[j].z;
      diff[j] &= diff[j] - 1;
    }
  }
#pragma unroll
  for (int j = 0; j < DS_QPL; ++j) {
    if (!live[j]) continue;
    if (x[j] == y[j]) {  // one end is an ancestor of the other
      lca[j] = y[j];
      live[j] = false;
    } else if (cdep[j] == 0) {  // two different roots
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
    for (int j = 0; j < DS_QPL; ++j) any |= live[j] && lvl[j] >= 1;
    if (!any) break;
    u32x4 ex[DS_QPL], ey[DS_QPL];
#pragma unroll
    for (int j = 0; j < DS_QPL; ++j) {
      const bool act = live[j] && lvl[j] >= 1;
      const uint64_t base = act ? (uint64_t)lvl[j] * n : 0ull;
      ex[j] = idx[base + (act ? x[j] : 0u)];
      ey[j] = idx[base + (act ? y[j] : 0u)];
    }
#pragma unroll
    for (int j = 0; j < DS_QPL; ++j) {
      if (!(live[j] && lvl[j] >= 1)) continue;
      if (ex[j].z != ey[j].z) {
        x[j] = ex[j].z;
        y[j] = ey[j].z;
      }
      --lvl[j];
    }
  }
  // level 0: the ends are now one or two steps below the LCA, or in different trees
#pragma unroll 1
  for (int step = 0; step < 2; ++step) {
    bool any = false;
#pragma unroll
    for (int j = 0; j < DS_QPL; ++j) any |= live[j];
    if (!any) break;
    u32x4 ex[DS_QPL], ey[DS_QPL];
#pragma unroll
    for (int j = 0; j < DS_QPL; ++j) {
      ex[j] = idx[live[j] ? x[j] : 0u];
      ey[j] = idx[live[j] ? y[j] : 0u];
    }
#pragma unroll
    for (int j = 0; j < DS_QPL; ++j) {
      if (!live[j]) continue;
      if (ex[j].z == ey[j].z) {  // a common parent (two roots differ: each is its own target)
        lca[j] = ex[j].z;
        live[j] = false;
      } else {
        x[j] = ex[j].z;
        y[j] = ey[j].z;
      }
    }
  }
  // still live: apart after the last step, different trees; lca stays DS_NONE
}

// the three gathers: wd[a] + wd[b] - 2 wd[lca], DS_INF without an lca. a, b and lca are below n.
__device__ __forceinline__ void gather_dist(const uint64_t *__restrict__ wd, const uint32_t (&a)[DS_QPL],
                                            const uint32_t (&b)[DS_QPL], const uint32_t (&lca)[DS_QPL],
                                            uint64_t (&d)[DS_QPL]) {
  uint64_t wa[DS_QPL], wb[DS_QPL], wl[DS_QPL];
#pragma unroll
  for (int j = 0; j < DS_QPL; ++j) {
    const bool ok = lca[j] != DS_NONE;
    wa[j] = wd[ok ? a[j] : 0u];
    wb[j] = wd[ok ? b[j] : 0u];
    wl[j] = wd[ok ? lca[j] : 0u];
  }
#pragma unroll
  for (int j = 0; j < DS_QPL; ++j) d[j] = lca[j] != DS_NONE ? wa[j] + wb[j] - 2 * wl[j] : DS_INF;
}

// ---- weighted depth ---------------------------------------------------------------------------------------
// GHS_DIST_HOPS: the depth itself
__global__ __launch_bounds__(DS_BLOCK) void k_ds_hops(uint32_t n, const u32x4 *__restrict__ lv0, uint64_t *__restrict__ out) {
  for (uint64_t x = blockIdx.x * (uint64_t)DS_BLOCK + threadIdx.x; x < n; x += (uint64_t)gridDim.x * DS_BLOCK)
    out[x] = lv0[x].w;
}

// pass 0: S_1[v] = w0[v] + w0[parent[v]] from the level-0 nodes (a root's key is 0); K == 1: S_1 is final
__global__ __launch_bounds__(DS_BLOCK) void k_ds_wd0(uint32_t n, const u32x4 *__restrict__ lv0, uint64_t *__restrict__ out) {
  for (uint64_t x = blockIdx.x * (uint64_t)DS_BLOCK + threadIdx.x; x < n; x += (uint64_t)gridDim.x * DS_BLOCK) {
    const u32x4 a = lv0[x];
    const uint32_t up = a.z < n ? a.z : (uint32_t)x;  // never: the index holds only ids below n
    const u32x4 b = lv0[up];
    out[x] = (uint64_t)a.y + (up != (uint32_t)x ? (uint64_t)b.y : 0ull);
  }
}

// pass k >= 1: S_{k+1}[v] = S_k[v] + S_k[up_k[v]]; up_k[v] == v only for a root, whose sums are 0
__global__ __launch_bounds__(DS_BLOCK) void k_ds_wdk(uint32_t n, const u32x4 *__restrict__ lvk, const uint64_t *__restrict__ in,
                                                     uint64_t *__restrict__ out) {
  for (uint64_t x = blockIdx.x * (uint64_t)DS_BLOCK + threadIdx.x; x < n; x += (uint64_t)gridDim.x * DS_BLOCK) {
    const uint32_t t = lvk[x].z;
    const uint32_t up = t < n ? t : (uint32_t)x;  // never
    out[x] = in[x] + (up != (uint32_t)x ? in[up] : 0ull);
  }
}

// ---- distance queries -------------------------------------------------------------------------------------
// A block takes the tiles g, g + gridDim, ... of 1024 pairs; in a tile lane t owns pairs j * 256 + t,
// j = 0 .. 3: coalesced loads of a / b and stores of the outputs at any 4- / 8-byte offset. The grid is
// what the chip holds at once (tile_grid), so the counters see a few atomics per resident block, not per
// tile: tens of thousands of blocks adding to one cache line cost more than the walk.
__global__ __launch_bounds__(DS_BLOCK) void k_ds_query(uint32_t n, uint32_t K, uint64_t Q, const uint32_t *__restrict__ qa,
                                                       const uint32_t *__restrict__ qb, const u32x4 *__restrict__ idx,
                                                       const uint64_t *__restrict__ wd, uint64_t *__restrict__ odist,
                                                       uint32_t *__restrict__ olca, uint64_t *__restrict__ status) {
  __shared__ uint32_t s_w[DS_BLOCK / 64];
  __shared__ uint64_t s_m[DS_BLOCK / 64];
  const uint64_t tiles = (Q + DS_TILE - 1) / DS_TILE;
  uint32_t badid = 0, connected = 0;
  uint64_t far = 0;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t q0 = tile * DS_TILE + threadIdx.x;
    uint32_t a[DS_QPL], b[DS_QPL], x[DS_QPL], y[DS_QPL], lca[DS_QPL];
    bool live[DS_QPL];
#pragma unroll
    for (int j = 0; j < DS_QPL; ++j) {
      const uint64_t q = q0 + (uint64_t)j * DS_BLOCK;
      const bool valid = q < Q;
      a[j] = valid ? qa[q] : 0u;
      b[j] = valid ? qb[q] : 0u;
      live[j] = valid;
      if (a[j] >= n || b[j] >= n) {
        badid = 1;
        a[j] = b[j] = 0;
        live[j] = false;
      }
      x[j] = a[j];
      y[j] = b[j];
    }
    lca_walk(n, K, idx, x, y, live, lca);
    uint64_t d[DS_QPL];
    gather_dist(wd, a, b, lca, d);
#pragma unroll
    for (int j = 0; j < DS_QPL; ++j) {
      const uint64_t q = q0 + (uint64_t)j * DS_BLOCK;
      if (q < Q) {
        odist[q] = d[j];
        if (olca) olca[q] = lca[j];
        if (lca[j] != DS_NONE) {
          ++connected;
          far = d[j] > far ? d[j] : far;
        }
      }
    }
  }
  // a lane counts at most its share of 2^32 - 1 pairs: no 32-bit counter wraps before the block sum,
  // which is taken in 64 bits
  const uint64_t c = block_sum64(connected, s_m);
  const uint32_t bd = block_sum(badid, s_w);
  const uint64_t fm = block_max64(far, s_m);
  if (threadIdx.x == 0) {
    if (c) atomicAdd((unsigned long long *)(status + ST_CONNECTED), (unsigned long long)c);
    if (fm) max_into(status + ST_MAX, fm);
    if (bd) atomicMax((unsigned long long *)(status + ST_BAD), 1ull);
  }
}

// ---- the graph's own edges -------------------------------------------------------------------------------
// PICK = false: the distances, their sums and their maximum. PICK = true: the same walk again, for the
// smallest eid whose distance is the maximum found (used when no per-edge array was written).
template <bool PICK>
__global__ __launch_bounds__(DS_BLOCK) void k_ds_edges(uint32_t n, uint32_t K, uint64_t m, const uint32_t *__restrict__ eu,
                                                       const uint32_t *__restrict__ ev, const uint32_t *__restrict__ ew,
                                                       const u32x4 *__restrict__ idx, const uint64_t *__restrict__ wd,
                                                       uint64_t *__restrict__ odist, uint64_t *__restrict__ status) {
  __shared__ uint32_t s_w[DS_BLOCK / 64];
  __shared__ uint64_t s_m[DS_BLOCK / 64];
  const uint64_t tiles = (m + DS_TILE - 1) / DS_TILE;
  const uint64_t picked = PICK ? status[ST_MAX] : 0ull;
  uint32_t badid = 0;
  uint64_t first = DS_INF;                                            // PICK
  uint32_t connected = 0, tight = 0, hi = 0;                          // !PICK: a lane sees fewer than 2^31 edges
  uint64_t far = 0, lo = 0, sw = 0;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // tiles as in k_ds_query
    const uint64_t e0 = tile * DS_TILE + threadIdx.x;
    uint32_t a[DS_QPL], b[DS_QPL], x[DS_QPL], y[DS_QPL], lca[DS_QPL];
    bool live[DS_QPL];
#pragma unroll
    for (int j = 0; j < DS_QPL; ++j) {
      const uint64_t e = e0 + (uint64_t)j * DS_BLOCK;
      const bool valid = e < m;
      a[j] = valid ? eu[e] : 0u;
      b[j] = valid ? ev[e] : 0u;
      live[j] = valid;
      if (a[j] >= n || b[j] >= n) {
        badid = 1;
        a[j] = b[j] = 0;
        live[j] = false;
      }
      x[j] = a[j];
      y[j] = b[j];
    }
    lca_walk(n, K, idx, x, y, live, lca);
    uint64_t d[DS_QPL];
    gather_dist(wd, a, b, lca, d);
#pragma unroll
    for (int j = 0; j < DS_QPL; ++j) {
      const uint64_t e = e0 + (uint64_t)j * DS_BLOCK;
      if (e >= m) continue;
      if (PICK) {
        if (lca[j] != DS_NONE && d[j] == picked) first = e < first ? e : first;
        continue;
      }
      if (odist) odist[e] = d[j];
      if (lca[j] == DS_NONE) continue;
      const uint32_t w = ew[e];
      ++connected;
      tight += d[j] == (uint64_t)w;
      far = d[j] > far ? d[j] : far;
      sw += w;
      lo += d[j];
      hi += lo < d[j];  // the carry of this lane's 128-bit sum
    }
  }
  if (PICK) {
    const uint64_t f = block_min64(first, s_m);
    if (threadIdx.x == 0 && f != DS_INF) min_into(status + ST_ARGMAX, f);
    return;
  }
  // the block's 128-bit sum: the lanes' low words are added by 32-bit halves (256 halves stay below
  // 2^40, so nothing wraps), what overflows 64 bits joins the lanes' carries
  const uint64_t lo_l = block_sum64(lo & 0xffffffffull, s_m), lo_h = block_sum64(lo >> 32, s_m);
  const uint64_t bhi = block_sum64(hi, s_m);
  const uint64_t bsw = block_sum64(sw, s_m), fm = block_max64(far, s_m);
  const uint64_t c = block_sum64(connected, s_m), t = block_sum64(tight, s_m);  // summed in 64 bits
  const uint32_t bd = block_sum(badid, s_w);
  if (threadIdx.x == 0) {
    // lo_l, lo_h < 2^40: mid < 2^41, its upper part goes to the high word
    const uint64_t mid = lo_h + (lo_l >> 32);
    const uint64_t blo = (mid << 32) | (lo_l & 0xffffffffull);
    uint64_t carry = bhi + (mid >> 32);
    if (blo) {
      const uint64_t old = atomicAdd((unsigned long long *)(status + ST_SUM_LO), (unsigned long long)blo);
      carry += (uint64_t)(old + blo < old);
    }
    if (carry) atomicAdd((unsigned long long *)(status + ST_SUM_HI), (unsigned long long)carry);
    if (bsw) atomicAdd((unsigned long long *)(status + ST_SUM_W), (unsigned long long)bsw);
    if (c) atomicAdd((unsigned long long *)(status + ST_CONNECTED), (unsigned long long)c);
    if (t) atomicAdd((unsigned long long *)(status + ST_TIGHT), (unsigned long long)t);
    if (fm) max_into(status + ST_MAX, fm);
    if (bd) atomicMax((unsigned long long *)(status + ST_BAD), 1ull);
  }
}

// the smallest eid whose written distance is the maximum: one stream over the per-edge array
__global__ __launch_bounds__(DS_BLOCK) void k_ds_pick(uint64_t m, const uint64_t *__restrict__ dist, uint64_t *__restrict__ status) {
  __shared__ uint64_t s_m[DS_BLOCK / 64];
  const uint64_t far = status[ST_MAX];
  uint64_t first = DS_INF;
  for (uint64_t e = blockIdx.x * (uint64_t)DS_BLOCK + threadIdx.x; e < m; e += (uint64_t)gridDim.x * DS_BLOCK)
    if (dist[e] == far) first = e < first ? e : first;  // far is finite: no cross edge matches
  const uint64_t f = block_min64(first, s_m);
  if (threadIdx.x == 0 && f != DS_INF) min_into(status + ST_ARGMAX, f);
}

// ---- diameters ---------------------------------------------------------------------------------------------
// every vertex's root (two jumps at the top level: 2 * 2^(K-1) > max_depth) and, per root, the largest wd
__global__ __launch_bounds__(DS_BLOCK) void k_ds_roots(uint32_t n, uint32_t K, const u32x4 *__restrict__ idx,
                                                       const uint64_t *__restrict__ wd, uint32_t *__restrict__ root_of,
                                                       uint64_t *__restrict__ best) {
  const u32x4 *top = idx + (uint64_t)(K - 1) * n;
  for (uint64_t x = blockIdx.x * (uint64_t)DS_BLOCK + threadIdx.x; x < n; x += (uint64_t)gridDim.x * DS_BLOCK) {
    uint32_t r = top[x].z;
    r = r < n ? r : (uint32_t)x;  // never
    r = top[r].z;
    r = r < n ? r : (uint32_t)x;  // never
    root_of[x] = r;
    max_into(best + r, wd[x]);
  }
}

// the smallest vertex of every tree whose value is the tree's maximum
__global__ __launch_bounds__(DS_BLOCK) void k_ds_argmax(uint32_t n, const uint32_t *__restrict__ root_of,
                                                        const uint64_t *__restrict__ val, const uint64_t *__restrict__ best,
                                                        uint32_t *__restrict__ arg) {
  for (uint64_t x = blockIdx.x * (uint64_t)DS_BLOCK + threadIdx.x; x < n; x += (uint64_t)gridDim.x * DS_BLOCK) {
    const uint32_t r = root_of[x];
    if (val[x] == best[r]) min_into(arg + r, (uint32_t)x);
  }
}

// one sweep: d = dist(v, target[root_of[v]]) for every vertex v, four per lane; out[v] = max(d, prev[v])
// (prev may be NULL and may be out itself: every lane reads and writes its own vertices only); with
// best, the tree's maximum of d is left in best[root].
__global__ __launch_bounds__(DS_BLOCK) void k_ds_sweep(uint32_t n, uint32_t K, const u32x4 *__restrict__ idx,
                                                       const uint64_t *__restrict__ wd, const uint32_t *__restrict__ root_of,
                                                       const uint32_t *__restrict__ target, const uint64_t *prev, uint64_t *out,
                                                       uint64_t *__restrict__ best) {
  const uint64_t v0 = blockIdx.x * DS_TILE + threadIdx.x;
  uint32_t a[DS_QPL], b[DS_QPL], x[DS_QPL], y[DS_QPL], lca[DS_QPL], r[DS_QPL];
  bool live[DS_QPL];
#pragma unroll
  for (int j = 0; j < DS_QPL; ++j) {
    const uint64_t v = v0 + (uint64_t)j * DS_BLOCK;
    const bool valid = v < n;
    a[j] = valid ? (uint32_t)v : 0u;
    r[j] = valid ? root_of[v] : 0u;
    r[j] = r[j] < n ? r[j] : a[j];  // never: k_ds_roots wrote ids below n
    const uint32_t t = target[r[j]];
    b[j] = t < n ? t : a[j];  // never: every tree's arg-max slot holds one of its vertices
    live[j] = valid;
    x[j] = a[j];
    y[j] = b[j];
  }
  lca_walk(n, K, idx, x, y, live, lca);
  uint64_t d[DS_QPL];
  gather_dist(wd, a, b, lca, d);
#pragma unroll
  for (int j = 0; j < DS_QPL; ++j) {
    const uint64_t v = v0 + (uint64_t)j * DS_BLOCK;
    if (v >= n) continue;
    uint64_t e = lca[j] != DS_NONE ? d[j] : 0ull;  // always an lca: both are in r's tree
    if (prev) {
      const uint64_t p = prev[v];
      e = p > e ? p : e;
    }
    out[v] = e;
    if (best) max_into(best + r[j], e);
  }
}

// the summary, four launches: trees and the largest diameter; its smallest root; the smallest
// eccentricity in that tree; the smallest vertex attaining it
__global__ __launch_bounds__(DS_BLOCK) void k_ds_sum_diam(uint32_t n, const uint32_t *__restrict__ root_of,
                                                          const uint64_t *__restrict__ diam, uint64_t *__restrict__ status) {
  __shared__ uint32_t s_w[DS_BLOCK / 64];
  __shared__ uint64_t s_m[DS_BLOCK / 64];
  uint32_t trees = 0;
  uint64_t far = 0;
  for (uint64_t x = blockIdx.x * (uint64_t)DS_BLOCK + threadIdx.x; x < n; x += (uint64_t)gridDim.x * DS_BLOCK) {
    if (root_of[x] != (uint32_t)x) continue;
    ++trees;
    const uint64_t d = diam[x];
    far = d > far ? d : far;
  }
  const uint32_t t = block_sum(trees, s_w);
  const uint64_t fm = block_max64(far, s_m);
  if (threadIdx.x == 0) {
    if (t) atomicAdd((unsigned long long *)(status + ST_TREES), (unsigned long long)t);
    if (fm) max_into(status + ST_MAX, fm);
  }
}

__global__ __launch_bounds__(DS_BLOCK) void k_ds_sum_root(uint32_t n, const uint32_t *__restrict__ root_of,
                                                          const uint64_t *__restrict__ diam, uint64_t *__restrict__ status) {
  __shared__ uint64_t s_m[DS_BLOCK / 64];
  const uint64_t far = status[ST_MAX];
  uint64_t first = DS_INF;
  for (uint64_t x = blockIdx.x * (uint64_t)DS_BLOCK + threadIdx.x; x < n; x += (uint64_t)gridDim.x * DS_BLOCK)
    if (root_of[x] == (uint32_t)x && diam[x] == far) first = x < first ? x : first;
  const uint64_t f = block_min64(first, s_m);
  if (threadIdx.x == 0 && f != DS_INF) min_into(status + ST_ARGMAX, f);
}

// CENTER = false: the smallest eccentricity of the widest tree; true: the smallest vertex attaining it
template <bool CENTER>
__global__ __launch_bounds__(DS_BLOCK) void k_ds_sum_ecc(uint32_t n, const uint32_t *__restrict__ root_of,
                                                         const uint64_t *__restrict__ ecc, uint64_t *__restrict__ status) {
  __shared__ uint64_t s_m[DS_BLOCK / 64];
  const uint64_t root = status[ST_ARGMAX], least = CENTER ? status[ST_MINECC] : 0ull;
  uint64_t best = DS_INF;
  for (uint64_t x = blockIdx.x * (uint64_t)DS_BLOCK + threadIdx.x; x < n; x += (uint64_t)gridDim.x * DS_BLOCK) {
    if (root_of[x] != root) continue;
    const uint64_t e = ecc[x];
    const uint64_t c = CENTER ? (e == least ? x : DS_INF) : e;
    best = c < best ? c : best;
  }
  const uint64_t f = block_min64(best, s_m);
  if (threadIdx.x == 0 && f != DS_INF) min_into(status + (CENTER ? ST_CENTER : ST_MINECC), f);
}

}  // namespace dist
}  // namespace ghs

using namespace ghs;
using namespace ghs::dist;

namespace {
// counters and maxima to zero, minima to all ones
int reset_status(uint64_t *status, hipStream_t st) {
  GHS_HIP_CHECK(hipMemsetAsync(status, 0, (size_t)ST_ZEROED * 8, st));
  GHS_HIP_CHECK(hipMemsetAsync(status + ST_ZEROED, 0xff, DS_STATUS_BYTES - (size_t)ST_ZEROED * 8, st));
  return GHS_OK;
}

// the grid of a kernel that loops over tiles: as many blocks as the device holds at once (every block
// then reports to the counters once), never more than there are tiles; 2048 when the device will not say
template <typename Kernel>
unsigned tile_grid(Kernel kernel, uint64_t items) {
  const uint64_t tiles = (items + DS_TILE - 1) / DS_TILE;
  int dev = 0, cus = 0, per_cu = 0;
  uint64_t g = 2048;
  if (hipGetDevice(&dev) == hipSuccess &&
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, DS_BLOCK, 0) == hipSuccess && cus > 0 && per_cu > 0)
    g = (uint64_t)cus * per_cu;
  if (g > tiles) g = tiles;
  return (unsigned)(g ? g : 1);
}

// the index's own status block: behind its K levels (ghs_forest_paths_index_bytes)
uint64_t *index_status(const ghs_paths_info_t &pi) {
  return (uint64_t *)((char *)pi.d_index + align256((size_t)16 * pi.levels * pi.n));
}
}  // namespace

extern "C" {

size_t ghs_forest_dist_workspace_bytes(uint32_t n, uint64_t max_depth) {
  (void)max_depth;  // one slab of n sums at any K: the passes ping-pong between it and the output
  return align256((size_t)8 * n) + DS_STATUS_BYTES;
}

int ghs_forest_wdepth_device(ghs_paths_t *h, uint32_t metric, uint64_t *d_wdepth, void *d_workspace, size_t workspace_bytes,
                             void *stream) {
  hipStream_t st = (hipStream_t)stream;
  ghs_paths_info_t pi;
  if (ghs_forest_paths_info(h, &pi) != GHS_OK) GHS_FAIL(GHS_E_ARG, "handle is NULL or destroyed");
  if (metric != GHS_DIST_WEIGHT && metric != GHS_DIST_HOPS) GHS_FAIL(GHS_E_ARG, "unknown metric");
  const uint32_t n = (uint32_t)pi.n, K = (uint32_t)pi.levels;
  if ((n && !d_wdepth) || !d_workspace) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if ((uintptr_t)d_wdepth & 7) GHS_FAIL(GHS_E_ARG, "wdepth must be 8-byte aligned");
  if ((uintptr_t)d_workspace & 15) GHS_FAIL(GHS_E_ARG, "the workspace must be 16-byte aligned");
  if (workspace_bytes < ghs_forest_dist_workspace_bytes(n, pi.max_depth)) GHS_FAIL(GHS_E_NOMEM, "workspace too small");
  if (n == 0) return GHS_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");
  const u32x4 *idx = (const u32x4 *)pi.d_index;
  const unsigned vgrid = grid_for(n, DS_BLOCK);
  if (metric == GHS_DIST_HOPS) {
    k_ds_hops<<<vgrid, DS_BLOCK, 0, st>>>(n, idx, d_wdepth);
  } else {
    // pass j writes the output when K - 1 - j is even, so that pass K - 1 does
    uint64_t *slab = (uint64_t *)d_workspace;
    auto buf = [&](uint32_t j) { return ((K - 1 - j) & 1) ? slab : d_wdepth; };
    k_ds_wd0<<<vgrid, DS_BLOCK, 0, st>>>(n, idx, buf(0));
    for (uint32_t j = 1; j < K; ++j) k_ds_wdk<<<vgrid, DS_BLOCK, 0, st>>>(n, idx + (size_t)j * n, buf(j - 1), buf(j));
  }
  GHS_HIP_CHECK(hipGetLastError());
  GHS_HIP_CHECK(hipStreamSynchronize(st));
  return GHS_OK;
}

int ghs_forest_dist_query(ghs_paths_t *h, const uint64_t *d_wdepth, uint64_t q, const uint32_t *d_a, const uint32_t *d_b,
                          uint64_t *d_dist, uint32_t *d_lca, ghs_dist_query_result_t *result, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_dist_query_result_t{};
  ghs_paths_info_t pi;
  if (ghs_forest_paths_info(h, &pi) != GHS_OK) GHS_FAIL(GHS_E_ARG, "handle is NULL or destroyed");
  if (q >= (1ull << 32)) GHS_FAIL(GHS_E_ARG, "q must be < 2^32");
  if (q == 0) return GHS_OK;
  if (!d_a || !d_b || !d_dist || (pi.n && !d_wdepth)) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if (((uintptr_t)d_a | (uintptr_t)d_b | (uintptr_t)d_lca) & 3) GHS_FAIL(GHS_E_ARG, "a, b and lca must be 4-byte aligned");
  if (((uintptr_t)d_wdepth | (uintptr_t)d_dist) & 7) GHS_FAIL(GHS_E_ARG, "wdepth and dist must be 8-byte aligned");
  result->queries = q;
  if (pi.n == 0) GHS_FAIL(GHS_E_ARG, "vertex id out of range");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");
  const auto t0 = std::chrono::steady_clock::now();
  uint64_t *status = index_status(pi);
  uint64_t hst[ST_SLOTS] = {};
  if (int e = reset_status(status, st)) return e;
  const unsigned grid = tile_grid(k_ds_query, q);
  k_ds_query<<<grid, DS_BLOCK, 0, st>>>((uint32_t)pi.n, (uint32_t)pi.levels, q, d_a, d_b, (const u32x4 *)pi.d_index, d_wdepth,
                                        d_dist, d_lca, status);
  GHS_HIP_CHECK(hipGetLastError());
  GHS_HIP_CHECK(hipMemcpyAsync(hst, status, sizeof(hst), hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipStreamSynchronize(st));
  if (hst[ST_BAD]) GHS_FAIL(GHS_E_ARG, "vertex id out of range");
  result->connected = hst[ST_CONNECTED];
  result->disconnected = q - hst[ST_CONNECTED];
  result->max_dist = hst[ST_MAX];
  result->ms_total = ms_since(t0);
  return GHS_OK;
}

int ghs_forest_edge_dist_device(ghs_paths_t *h, const uint64_t *d_wdepth, uint64_t m, const uint32_t *d_u, const uint32_t *d_v,
                                const uint32_t *d_w, uint64_t *d_dist_by_edge, ghs_edge_dist_result_t *result, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_edge_dist_result_t{};
  result->max_eid = DS_NONE;
  ghs_paths_info_t pi;
  if (ghs_forest_paths_info(h, &pi) != GHS_OK) GHS_FAIL(GHS_E_ARG, "handle is NULL or destroyed");
  if (m >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "m must be < 2^31");
  if (m == 0) return GHS_OK;
  if (!d_u || !d_v || !d_w || (pi.n && !d_wdepth)) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if (((uintptr_t)d_u | (uintptr_t)d_v | (uintptr_t)d_w) & 15) GHS_FAIL(GHS_E_ARG, "u, v and w must be 16-byte aligned");
  if (((uintptr_t)d_wdepth | (uintptr_t)d_dist_by_edge) & 7) GHS_FAIL(GHS_E_ARG, "wdepth and dist_by_edge must be 8-byte aligned");
  result->edges = m;
  if (pi.n == 0) GHS_FAIL(GHS_E_ARG, "edge endpoint out of range");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t n = (uint32_t)pi.n, K = (uint32_t)pi.levels;
  const u32x4 *idx = (const u32x4 *)pi.d_index;
  uint64_t *status = index_status(pi);
  uint64_t hst[ST_SLOTS] = {};
  if (int e = reset_status(status, st)) return e;
  const unsigned grid = tile_grid(k_ds_edges<false>, m);
  k_ds_edges<false><<<grid, DS_BLOCK, 0, st>>>(n, K, m, d_u, d_v, d_w, idx, d_wdepth, d_dist_by_edge, status);
  if (d_dist_by_edge)
    k_ds_pick<<<grid_for(m, DS_BLOCK), DS_BLOCK, 0, st>>>(m, d_dist_by_edge, status);
  else
    k_ds_edges<true><<<tile_grid(k_ds_edges<true>, m), DS_BLOCK, 0, st>>>(n, K, m, d_u, d_v, d_w, idx, d_wdepth, nullptr, status);
  GHS_HIP_CHECK(hipGetLastError());
  GHS_HIP_CHECK(hipMemcpyAsync(hst, status, sizeof(hst), hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipStreamSynchronize(st));
  if (hst[ST_BAD]) GHS_FAIL(GHS_E_ARG, "edge endpoint out of range");
  result->sum_dist_lo = hst[ST_SUM_LO];
  result->sum_dist_hi = hst[ST_SUM_HI];
  result->sum_w = hst[ST_SUM_W];
  result->max_dist = hst[ST_MAX];
  result->cross_edges = m - hst[ST_CONNECTED];
  result->tight_edges = hst[ST_TIGHT];
  result->max_eid = hst[ST_ARGMAX] == DS_INF ? DS_NONE : (uint32_t)hst[ST_ARGMAX];
  result->ms_total = ms_since(t0);
  return GHS_OK;
}

int ghs_forest_diameter_device(ghs_paths_t *h, const uint64_t *d_wdepth, uint32_t *d_root_of, uint64_t *d_diam,
                               uint32_t *d_end_a, uint32_t *d_end_b, uint64_t *d_ecc, void *d_workspace, size_t workspace_bytes,
                               ghs_diameter_result_t *result, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_diameter_result_t{};
  result->max_root = result->center = DS_NONE;
  ghs_paths_info_t pi;
  if (ghs_forest_paths_info(h, &pi) != GHS_OK) GHS_FAIL(GHS_E_ARG, "handle is NULL or destroyed");
  const uint32_t n = (uint32_t)pi.n, K = (uint32_t)pi.levels;
  if ((n && (!d_wdepth || !d_root_of || !d_diam || !d_end_a || !d_end_b)) || !d_workspace) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if (((uintptr_t)d_root_of | (uintptr_t)d_end_a | (uintptr_t)d_end_b) & 3)
    GHS_FAIL(GHS_E_ARG, "root_of, end_a and end_b must be 4-byte aligned");
  if (((uintptr_t)d_wdepth | (uintptr_t)d_diam | (uintptr_t)d_ecc) & 7)
    GHS_FAIL(GHS_E_ARG, "wdepth, diam and ecc must be 8-byte aligned");
  if ((uintptr_t)d_workspace & 15) GHS_FAIL(GHS_E_ARG, "the workspace must be 16-byte aligned");
  if (workspace_bytes < ghs_forest_dist_workspace_bytes(n, pi.max_depth)) GHS_FAIL(GHS_E_NOMEM, "workspace too small");
  if (n == 0) return GHS_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");
  const auto t0 = std::chrono::steady_clock::now();
  const u32x4 *idx = (const u32x4 *)pi.d_index;
  uint64_t *slab = (uint64_t *)d_workspace;
  uint64_t *status = (uint64_t *)((char *)d_workspace + align256((size_t)8 * n));
  uint64_t *ecc = d_ecc ? d_ecc : slab;  // the eccentricities are formed either way: the centre needs them
  const unsigned vgrid = grid_for(n, DS_BLOCK);
  const unsigned sgrid = (unsigned)(((uint64_t)n + DS_TILE - 1) / DS_TILE);  // <= 2^22
  uint64_t hst[ST_SLOTS] = {};
  if (int e = reset_status(status, st)) return e;
  GHS_HIP_CHECK(hipMemsetAsync(ecc, 0, (size_t)n * 8, st));
  GHS_HIP_CHECK(hipMemsetAsync(d_diam, 0, (size_t)n * 8, st));
  GHS_HIP_CHECK(hipMemsetAsync(d_end_a, 0xff, (size_t)n * 4, st));
  GHS_HIP_CHECK(hipMemsetAsync(d_end_b, 0xff, (size_t)n * 4, st));
  // sweep 0, from the roots: wd is the distance. The ecc array holds the per-root maxima until sweep 1
  // overwrites every entry of it.
  k_ds_roots<<<vgrid, DS_BLOCK, 0, st>>>(n, K, idx, d_wdepth, d_root_of, ecc);
  k_ds_argmax<<<vgrid, DS_BLOCK, 0, st>>>(n, d_root_of, d_wdepth, ecc, d_end_a);
  // sweep 1, from p: the diameter and q
  k_ds_sweep<<<sgrid, DS_BLOCK, 0, st>>>(n, K, idx, d_wdepth, d_root_of, d_end_a, nullptr, ecc, d_diam);
  k_ds_argmax<<<vgrid, DS_BLOCK, 0, st>>>(n, d_root_of, ecc, d_diam, d_end_b);
  // sweep 2, from q: the eccentricities
  k_ds_sweep<<<sgrid, DS_BLOCK, 0, st>>>(n, K, idx, d_wdepth, d_root_of, d_end_b, ecc, ecc, nullptr);
  k_ds_sum_diam<<<vgrid, DS_BLOCK, 0, st>>>(n, d_root_of, d_diam, status);
  k_ds_sum_root<<<vgrid, DS_BLOCK, 0, st>>>(n, d_root_of, d_diam, status);
  k_ds_sum_ecc<false><<<vgrid, DS_BLOCK, 0, st>>>(n, d_root_of, ecc, status);
  k_ds_sum_ecc<true><<<vgrid, DS_BLOCK, 0, st>>>(n, d_root_of, ecc, status);
  GHS_HIP_CHECK(hipGetLastError());
  GHS_HIP_CHECK(hipMemcpyAsync(hst, status, sizeof(hst), hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipStreamSynchronize(st));
  result->num_trees = hst[ST_TREES];
  result->max_diameter = hst[ST_MAX];
  result->min_ecc = hst[ST_MINECC];
  result->max_root = (uint32_t)hst[ST_ARGMAX];
  result->center = (uint32_t)hst[ST_CENTER];
  result->ms_total = ms_since(t0);
  return GHS_OK;
}

}  // extern "C"
