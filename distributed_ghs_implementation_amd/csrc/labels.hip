// Vertex labels and forest cuts (ABI 10 addition, ghs_forest_labels_device): which component of
// the flagged forest does every vertex lie in — after keeping every flagged edge (the connected
// components of the graph when the flags are the engine's), only those with w <= t (single linkage
// at distance t) or all but the d heaviest (single linkage into k clusters)?
//
// The reference has nothing closer than nx.connected_components / the nx.Graph that check_mst.py
// builds from a result (check_mst.py:1-20): a host pass over the edge list. Here T = the flagged
// edges, K = the kept ones, and labels[v] = the rank of v's component of (V, K) with components
// ordered by their smallest vertex — exact and deterministic whatever the shape of K.
//
// Pipeline (everything on `stream`; one host sync per hook round + 3):
//   1. count the flags per 4096-flag tile (the weight cut is a predicate of the same pass), scan the
//      tile counts, gather (u, v) of every kept edge to its rank (GHS_CUT_COUNT: and its key);
//   2. GHS_CUT_COUNT: a radix select (8 passes of 8 bits, most significant first) finds the smallest
//      key to drop; one pass keeps the edges below it;
//   3. components of K by min-root hooking: par[max] = min(par[max], min) for every live edge (both
//      ends are roots), pointer-jump the live ends to a star forest, drop the edges whose ends now
//      share a root and rename the others to their roots;
//   4. jump every vertex, flag the roots, scan, labels[v] = rank[par[v]].
// par[x] <= x always, so par is acyclic and a component's root is its smallest vertex.
//
// This translation unit includes common.h only and launches only its own kernels; it calls the
// public ghs_check_canonical first, so every index below is in range.
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <utility>

#include "common.h"

namespace ghs {
namespace labels {

constexpr int LB_BLOCK = 256;
constexpr int LB_FLAGS_PER_THREAD = 16;                                      // one 16-byte load
constexpr uint64_t LB_FLAG_TILE = (uint64_t)LB_BLOCK * LB_FLAGS_PER_THREAD;  // flags per block
constexpr int LB_VERTS_PER_THREAD = 4;                                       // one 16-byte load of par
constexpr uint64_t LB_VERT_TILE = (uint64_t)LB_BLOCK * LB_VERTS_PER_THREAD;  // vertices per block of the root scan
constexpr int LB_JUMP_HOPS = 8;
constexpr int LB_MAX_JUMPS = 11;        // ceil(log8 2^32): launches that resolve any hook chain
constexpr uint32_t LB_MAX_ROUNDS = 80;  // 2 ceil(log2 n) + 2 <= 66 for n < 2^32
constexpr int LB_KEYS_PER_THREAD = 8;   // keys per thread of a radix-select histogram pass

constexpr int LB_ITEMS = 8;             // list entries per thread and iteration of the appending passes

// status block (uint64 slots, device). ST_LIVE, ST_ROOTS and the LB_MAX_JUMPS jump flags (uint32)
// that follow the slots are cleared together, with one memset, before a round.
enum { ST_FLAGGED = 0, ST_KEPT, ST_CLUSTERS, ST_CUTKEY, ST_SEL_PREFIX, ST_SEL_RANK, ST_LIVE, ST_ROOTS, ST_SLOTS };
constexpr size_t LB_ROUND_CLEAR = 2 * sizeof(uint64_t) + LB_MAX_JUMPS * sizeof(uint32_t);

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static inline unsigned grid_for(uint64_t items, unsigned per_block, unsigned cap = 2048) {
  uint64_t g = (items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

__device__ __forceinline__ uint32_t block_sum(uint32_t c, uint32_t *s_w) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x / 64] = c;
  __syncthreads();
  uint32_t t = 0;
#pragma unroll
  for (int w = 0; w < LB_BLOCK / 64; ++w) t += s_w[w];
  __syncthreads();
  return t;
}

// the rank of this thread's first item: tile offset + the block's exclusive prefix of c
__device__ __forceinline__ uint32_t rank_base(uint32_t c, uint32_t tile_off, uint32_t *s_w) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x / 64;
  uint32_t inc = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  if (lane == 63) s_w[wid] = inc;
  __syncthreads();
  uint32_t before = 0;
#pragma unroll
  for (int x = 0; x < LB_BLOCK / 64; ++x) before += x < wid ? s_w[x] : 0u;
  return tile_off + before + inc - c;
}

// exclusive scan of the tile counts in place (one block of 1024), the total to *total; `extra`
// (may be NULL): a second count per tile that is only summed, to *total2
__global__ __launch_bounds__(1024) void k_lb_tile_scan(uint32_t *__restrict__ cnt, uint32_t ntiles,
                                                       uint64_t *__restrict__ total,
                                                       const uint32_t *__restrict__ extra,
                                                       uint64_t *__restrict__ total2) {
  __shared__ uint32_t s_part[1024];
  const uint32_t per = (ntiles + 1023) / 1024;
  const uint64_t b = (uint64_t)threadIdx.x * per;
  uint32_t sum = 0;
  for (uint32_t i = 0; i < per && b + i < ntiles; ++i) sum += cnt[b + i];
  s_part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const uint32_t o = threadIdx.x >= (unsigned)d ? s_part[threadIdx.x - d] : 0;
    __syncthreads();
    s_part[threadIdx.x] += o;
    __syncthreads();
  }
  uint32_t run = s_part[threadIdx.x] - sum;
  for (uint32_t i = 0; i < per && b + i < ntiles; ++i) {
    const uint32_t c = cnt[b + i];
    cnt[b + i] = run;
    run += c;
  }
  if (threadIdx.x == 1023) *total = s_part[1023];
  if (extra) {
    uint32_t sum2 = 0;
    for (uint32_t i = 0; i < per && b + i < ntiles; ++i) sum2 += extra[b + i];
    __syncthreads();
    s_part[threadIdx.x] = sum2;
    __syncthreads();
    for (int d = 512; d > 0; d >>= 1) {
      if (threadIdx.x < (unsigned)d) s_part[threadIdx.x] += s_part[threadIdx.x + d];
      __syncthreads();
    }
    if (threadIdx.x == 0) *total2 = s_part[0];
  }
}

// ---- step 1: the flagged (and kept) edges, counted and gathered ------------------------------------
// The flags may start at any byte. They are read in the 16-byte-aligned frame that contains them:
// frame byte p holds the flag of edge p - lo for p in [lo, hi), lo = the pointer's low 4 bits. A
// thread owns 16 frame bytes: one 16-byte load when all of them are flags (always aligned), byte
// loads with a bound check at the head and the tail. Nothing outside [lo, hi) is read.
__device__ __forceinline__ uint32_t flag_mask16(uintptr_t frame, uint64_t p, uint64_t lo, uint64_t hi) {
  uint32_t mask = 0;
  if (p >= hi || p + LB_FLAGS_PER_THREAD <= lo) return 0;
  if (p >= lo && p + LB_FLAGS_PER_THREAD <= hi) {
    const u32x4 q = *reinterpret_cast<const u32x4 *>(frame + p);
    const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((wd[k] >> (8 * j)) & 0xffu) mask |= 1u << (4 * k + j);
  } else {
    for (int j = 0; j < LB_FLAGS_PER_THREAD; ++j)
      if (p + j >= lo && p + j < hi && *reinterpret_cast<const uint8_t *>(frame + p + j)) mask |= 1u << j;
  }
  return mask;
}

// GHS_CUT_WEIGHT: drop the flagged edges heavier than thr (one gather of w per flagged edge)
__device__ __forceinline__ uint32_t weight_cut(uint32_t mask, const uint32_t *__restrict__ w, uint64_t e0, uint32_t thr) {
  uint32_t keep = mask;
  while (mask) {
    const int j = __ffs(mask) - 1;
    mask &= mask - 1;
    if (w[e0 + j] > thr) keep &= ~(1u << j);
  }
  return keep;
}

template <bool WCUT>
__global__ __launch_bounds__(LB_BLOCK) void k_lb_flag_count(uintptr_t frame, uint64_t lo, uint64_t hi,
                                                            const uint32_t *__restrict__ w, uint32_t thr,
                                                            uint32_t *__restrict__ tile_cnt,
                                                            uint32_t *__restrict__ tile_flagged) {
  __shared__ uint32_t s_w[LB_BLOCK / 64];
  const uint64_t p = blockIdx.x * LB_FLAG_TILE + (uint64_t)threadIdx.x * LB_FLAGS_PER_THREAD;
  uint32_t mask = flag_mask16(frame, p, lo, hi);
  const uint32_t flagged = block_sum((uint32_t)__popc(mask), s_w);
  uint32_t kept = flagged;
  if (WCUT) {
    mask = weight_cut(mask, w, p - lo, thr);  // a set bit j has p + j >= lo
    kept = block_sum((uint32_t)__popc(mask), s_w);
  }
  if (threadIdx.x == 0) {  // no atomic here: tens of thousands of blocks on one address serialise
    tile_cnt[blockIdx.x] = kept;
    if (WCUT) tile_flagged[blockIdx.x] = flagged;
  }
}

// kept edge e at rank o -> ends[o] = (u[e], v[e]) and, for the count cut, keys[o] = w[e] << 32 | e
template <bool WCUT, bool KEYS>
__global__ __launch_bounds__(LB_BLOCK) void k_lb_write_edges(uintptr_t frame, uint64_t lo, uint64_t hi,
                                                             const uint32_t *__restrict__ u,
                                                             const uint32_t *__restrict__ v,
                                                             const uint32_t *__restrict__ w, uint32_t thr,
                                                             const uint32_t *__restrict__ tile_off,
                                                             uint2 *__restrict__ ends, uint64_t *__restrict__ keys,
                                                             uint64_t cap) {
  __shared__ uint32_t s_w[LB_BLOCK / 64];
  const uint64_t p = blockIdx.x * LB_FLAG_TILE + (uint64_t)threadIdx.x * LB_FLAGS_PER_THREAD;
  uint32_t mask = flag_mask16(frame, p, lo, hi);
  if (WCUT) mask = weight_cut(mask, w, p - lo, thr);
  uint64_t o = rank_base((uint32_t)__popc(mask), tile_off[blockIdx.x], s_w);
  while (mask) {
    const int j = __ffs(mask) - 1;
    mask &= mask - 1;
    const uint64_t e = p + j - lo;
    if (o < cap) {  // the host has checked the count against cap already
      ends[o] = make_uint2(u[e], v[e]);
      if (KEYS) keys[o] = ((uint64_t)w[e] << 32) | e;
    }
    ++o;
  }
}

// ---- step 2: GHS_CUT_COUNT — the key at ascending position ST_SEL_RANK among T distinct keys ----------
// One pass per key byte, most significant first: a histogram of that byte over the keys that match the
// prefix chosen so far, then one thread picks the bin the position falls into. A thread folds runs of
// equal bins before it touches the LDS histogram (small weights make the upper bytes all zero).
__global__ __launch_bounds__(LB_BLOCK) void k_lb_sel_hist(const uint64_t *__restrict__ keys, uint64_t T, int shift,
                                                          const uint64_t *__restrict__ status,
                                                          uint32_t *__restrict__ hist) {
  __shared__ uint32_t s_h[256];
  s_h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t prefix = status[ST_SEL_PREFIX];
  const uint64_t chunk = (uint64_t)LB_BLOCK * LB_KEYS_PER_THREAD;
  for (uint64_t base = blockIdx.x * chunk; base < T; base += (uint64_t)gridDim.x * chunk) {
    uint32_t bin = 0, run = 0;
#pragma unroll
    for (int i = 0; i < LB_KEYS_PER_THREAD; ++i) {
      const uint64_t t = base + (uint64_t)i * LB_BLOCK + threadIdx.x;
      if (t >= T) continue;
      const uint64_t k = keys[t];
      // shift == 56: no prefix yet (a shift by 64 is undefined)
      if (shift < 56 && (k >> (shift + 8)) != (prefix >> (shift + 8))) continue;
      const uint32_t b = (uint32_t)(k >> shift) & 0xffu;
      if (run && b != bin) {
        atomicAdd(&s_h[bin], run);
        run = 0;
      }
      bin = b;
      ++run;
    }
    if (run) atomicAdd(&s_h[bin], run);
  }
  __syncthreads();
  if (s_h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], s_h[threadIdx.x]);
}

// the bin holding position ST_SEL_RANK: prefix |= bin << shift, rank -= the keys below it; clears hist
// for the next pass
__global__ __launch_bounds__(256) void k_lb_sel_pick(uint32_t *__restrict__ hist, int shift, uint64_t rank0,
                                                     uint64_t *__restrict__ status) {
  __shared__ uint32_t s_h[256];
  s_h[threadIdx.x] = hist[threadIdx.x];
  hist[threadIdx.x] = 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    // the first pass starts the search: position rank0, no prefix
    uint64_t r = shift == 56 ? rank0 : status[ST_SEL_RANK], below = 0;
    const uint64_t prefix = shift == 56 ? 0ull : status[ST_SEL_PREFIX];
    uint32_t b = 0;
    for (; b < 255; ++b) {
      if (r < below + s_h[b]) break;
      below += s_h[b];
    }
    status[ST_SEL_RANK] = r - below;
    status[ST_SEL_PREFIX] = prefix | ((uint64_t)b << shift);
    if (shift == 0) status[ST_CUTKEY] = prefix | (uint64_t)b;
  }
}

// reserves room in out[] for the kept items of one block iteration (c per thread, up to LB_ITEMS)
// with ONE atomic per block — 2048 entries per atomic: one per 256 serialised on the counter's
// address and cost more than the pass's bytes. Returns the slot of this thread's first item.
__device__ __forceinline__ uint64_t block_append(uint32_t c, uint32_t *s_w, uint64_t *s_base, uint64_t *count) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x / 64;
  uint32_t inc = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  if (lane == 63) s_w[wid] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tot = 0;
    for (int x = 0; x < LB_BLOCK / 64; ++x) tot += s_w[x];
    *s_base = tot ? atomicAdd((unsigned long long *)count, (unsigned long long)tot) : 0ull;
  }
  __syncthreads();
  uint32_t before = 0;
#pragma unroll
  for (int x = 0; x < LB_BLOCK / 64; ++x) before += x < wid ? s_w[x] : 0u;
  const uint64_t o = *s_base + before + inc - c;
  __syncthreads();
  return o;
}

// K = the edges of T whose key is below the cut key (order does not matter from here on)
__global__ __launch_bounds__(LB_BLOCK) void k_lb_cut(const uint2 *__restrict__ in, const uint64_t *__restrict__ keys,
                                                     uint64_t T, uint2 *__restrict__ out, uint64_t cap,
                                                     uint64_t *__restrict__ status) {
  __shared__ uint32_t s_w[LB_BLOCK / 64];
  __shared__ uint64_t s_base;
  const uint64_t cut = status[ST_CUTKEY];
  const uint64_t chunk = (uint64_t)LB_BLOCK * LB_ITEMS;
  for (uint64_t base = blockIdx.x * chunk; base < T; base += (uint64_t)gridDim.x * chunk) {
    uint32_t keep = 0;
#pragma unroll
    for (int i = 0; i < LB_ITEMS; ++i) {
      const uint64_t t = base + (uint64_t)i * LB_BLOCK + threadIdx.x;
      if (t < T && keys[t] < cut) keep |= 1u << i;
    }
    uint64_t o = block_append((uint32_t)__popc(keep), s_w, &s_base, status + ST_KEPT);
#pragma unroll
    for (int i = 0; i < LB_ITEMS; ++i)
      if ((keep >> i) & 1u) {
        if (o < cap) out[o] = in[base + (uint64_t)i * LB_BLOCK + threadIdx.x];
        ++o;
      }
  }
}

// ---- step 3: components of K ----------------------------------------------------------------------
__global__ __launch_bounds__(LB_BLOCK) void k_lb_init(uint32_t *__restrict__ par, uint32_t *__restrict__ mark, uint64_t n) {
  const uint64_t quads = (n + 3) / 4;
  for (uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; q < quads; q += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t v0 = 4 * q;
    if (v0 + 4 <= n) {
      u32x4 id, z;
      id.x = (uint32_t)v0; id.y = (uint32_t)v0 + 1; id.z = (uint32_t)v0 + 2; id.w = (uint32_t)v0 + 3;
      z.x = z.y = z.z = z.w = 0;
      *reinterpret_cast<u32x4 *>(par + v0) = id;
      if (mark) *reinterpret_cast<u32x4 *>(mark + v0) = z;
    } else {
      for (uint64_t x = v0; x < n; ++x) {
        par[x] = (uint32_t)x;
        if (mark) mark[x] = 0;
      }
    }
  }
}

// hook: both ends of a live edge are roots (the list holds roots: vertices in round 1, renamed ends
// later), so the larger one takes the smaller as its parent unless it already has a smaller one. A
// stale read is never smaller than the slot, so a skipped atomic is always right.
__global__ __launch_bounds__(LB_BLOCK) void k_lb_hook(const uint2 *__restrict__ ends, uint64_t live,
                                                      uint32_t *__restrict__ par) {
  for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < live; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint2 e = ends[t];
    const uint32_t hi = e.x > e.y ? e.x : e.y, lo = e.x > e.y ? e.y : e.x;
    if (hi != lo && par[hi] > lo) atomicMin(&par[hi], lo);
  }
}

// up to LB_JUMP_HOPS hops from x; true when the walk ran out of hops before it saw a root
__device__ __forceinline__ bool jump_one(uint32_t *__restrict__ par, uint32_t x) {
  const uint32_t p0 = par[x];
  uint32_t p = p0;
  bool open = true;
#pragma unroll 1
  for (int h = 0; h < LB_JUMP_HOPS; ++h) {
    const uint32_t g = par[p];
    if (g == p) {
      open = false;
      break;
    }
    p = g;
  }
  if (p != p0) par[x] = p;
  return open;
}

// pointer jump of the live ends, in place: up to LB_JUMP_HOPS hops per launch. Every vertex on a
// hook chain was a root with a live edge at the round's start, so it is an end of the list. Every
// value read is an ancestor at least as far as the previous launch left it: launch j reaches
// min(8^j, depth) levels up. No root changes while the jumps run, so an end whose walk saw a root
// has its final parent: a launch in which every walk did leaves its flag 0 and the launches after
// it return at once (no loop depends on the data beyond LB_JUMP_HOPS).
__global__ __launch_bounds__(LB_BLOCK) void k_lb_jump_ends(const uint2 *__restrict__ ends, uint64_t live,
                                                           uint32_t *__restrict__ par, const uint32_t *chg_prev,
                                                           uint32_t *chg_cur) {
  if (chg_prev && *chg_prev == 0) return;
  bool open = false;
  for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < live; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint2 e = ends[t];
    open |= jump_one(par, e.x);
    open |= jump_one(par, e.y);
  }
  if (open) *chg_cur = 1;
}

// the same for every vertex (once, after the last round: depth <= rounds)
__global__ __launch_bounds__(LB_BLOCK) void k_lb_jump_all(uint32_t *__restrict__ par, uint64_t n, const uint32_t *chg_prev,
                                                          uint32_t *chg_cur) {
  if (chg_prev && *chg_prev == 0) return;
  bool open = false;
  for (uint64_t x = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; x < n; x += (uint64_t)gridDim.x * blockDim.x)
    open |= jump_one(par, (uint32_t)x);
  if (open) *chg_cur = 1;
}

// the live list of the next round: ends renamed to their roots, edges inside one tree dropped, one
// atomic per block and iteration (LB_ITEMS edges per thread, their 2 LB_ITEMS gathers in flight). A root seen for the first time this round (mark[r] != round) is
// counted: the live roots of the next round, for the host's halving guard.
__global__ __launch_bounds__(LB_BLOCK) void k_lb_compact(const uint2 *__restrict__ in, uint64_t live,
                                                         const uint32_t *__restrict__ par, uint2 *__restrict__ out,
                                                         uint64_t cap, uint32_t *__restrict__ mark, uint32_t round,
                                                         uint64_t *__restrict__ status) {
  __shared__ uint32_t s_w[LB_BLOCK / 64];
  __shared__ uint64_t s_base;
  uint32_t roots = 0;
  const uint64_t chunk = (uint64_t)LB_BLOCK * LB_ITEMS;
  for (uint64_t base = blockIdx.x * chunk; base < live; base += (uint64_t)gridDim.x * chunk) {
    uint2 e[LB_ITEMS];
    uint32_t keep = 0;
#pragma unroll
    for (int i = 0; i < LB_ITEMS; ++i) {
      const uint64_t t = base + (uint64_t)i * LB_BLOCK + threadIdx.x;
      e[i] = t < live ? in[t] : make_uint2(0, 0);
    }
#pragma unroll
    for (int i = 0; i < LB_ITEMS; ++i) {
      const uint64_t t = base + (uint64_t)i * LB_BLOCK + threadIdx.x;
      if (t < live) {
        e[i].x = par[e[i].x];
        e[i].y = par[e[i].y];
        if (e[i].x != e[i].y) keep |= 1u << i;
      }
    }
#pragma unroll
    for (int i = 0; i < LB_ITEMS; ++i)
      if ((keep >> i) & 1u) {
        if (mark[e[i].x] != round && atomicExch(&mark[e[i].x], round) != round) ++roots;
        if (mark[e[i].y] != round && atomicExch(&mark[e[i].y], round) != round) ++roots;
      }
    uint64_t o = block_append((uint32_t)__popc(keep), s_w, &s_base, status + ST_LIVE);
#pragma unroll
    for (int i = 0; i < LB_ITEMS; ++i)
      if ((keep >> i) & 1u) {
        if (o < cap) out[o] = e[i];
        ++o;
      }
  }
  const uint32_t tot = block_sum(roots, s_w);
  if (threadIdx.x == 0 && tot) atomicAdd((unsigned long long *)(status + ST_ROOTS), (unsigned long long)tot);
}

// ---- step 4: dense labels ----------------------------------------------------------------------------
__device__ __forceinline__ uint32_t root_mask4(const uint32_t *__restrict__ par, uint64_t v0, uint64_t n) {
  uint32_t mask = 0;
  if (v0 + 4 <= n) {
    const u32x4 q = *reinterpret_cast<const u32x4 *>(par + v0);
    mask = (q.x == (uint32_t)v0 ? 1u : 0u) | (q.y == (uint32_t)v0 + 1 ? 2u : 0u) | (q.z == (uint32_t)v0 + 2 ? 4u : 0u) |
           (q.w == (uint32_t)v0 + 3 ? 8u : 0u);
  } else {
    for (int j = 0; j < 4; ++j)
      if (v0 + j < n && par[v0 + j] == (uint32_t)(v0 + j)) mask |= 1u << j;
  }
  return mask;
}

__global__ __launch_bounds__(LB_BLOCK) void k_lb_root_count(const uint32_t *__restrict__ par, uint64_t n,
                                                            uint32_t *__restrict__ tile_cnt) {
  __shared__ uint32_t s_w[LB_BLOCK / 64];
  const uint64_t v0 = blockIdx.x * LB_VERT_TILE + (uint64_t)threadIdx.x * LB_VERTS_PER_THREAD;
  const uint32_t t = block_sum((uint32_t)__popc(root_mask4(par, v0, n)), s_w);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = t;
}

// root r at rank o (roots in vertex order = components by smallest vertex) -> rank[r] = o
__global__ __launch_bounds__(LB_BLOCK) void k_lb_root_rank(const uint32_t *__restrict__ par, uint64_t n,
                                                           const uint32_t *__restrict__ tile_off,
                                                           uint32_t *__restrict__ rank) {
  __shared__ uint32_t s_w[LB_BLOCK / 64];
  const uint64_t v0 = blockIdx.x * LB_VERT_TILE + (uint64_t)threadIdx.x * LB_VERTS_PER_THREAD;
  uint32_t mask = root_mask4(par, v0, n);
  uint32_t o = rank_base((uint32_t)__popc(mask), tile_off[blockIdx.x], s_w);
  while (mask) {
    const int j = __ffs(mask) - 1;
    mask &= mask - 1;
    rank[v0 + j] = o++;
  }
}

// labels[v] = rank[par[v]]: 4 vertices per lane, a 16-byte store when labels is 16-byte aligned
__global__ __launch_bounds__(LB_BLOCK) void k_lb_labels(const uint32_t *__restrict__ par, const uint32_t *__restrict__ rank,
                                                        uint32_t *__restrict__ labels, uint64_t n, bool lvec) {
  const uint64_t quads = (n + 3) / 4;
  for (uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; q < quads; q += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t v0 = 4 * q;
    if (v0 + 4 <= n) {
      const u32x4 p = *reinterpret_cast<const u32x4 *>(par + v0);
      u32x4 l;
      l.x = rank[p.x]; l.y = rank[p.y]; l.z = rank[p.z]; l.w = rank[p.w];
      if (lvec) {
        *reinterpret_cast<u32x4 *>(labels + v0) = l;
      } else {
        labels[v0] = l.x; labels[v0 + 1] = l.y; labels[v0 + 2] = l.z; labels[v0 + 3] = l.w;
      }
    } else {
      for (uint64_t x = v0; x < n; ++x) labels[x] = rank[par[x]];
    }
  }
}

// m == 0: every vertex is a cluster of its own
__global__ __launch_bounds__(LB_BLOCK) void k_lb_identity(uint32_t *__restrict__ labels, uint64_t n) {
  for (uint64_t x = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; x < n; x += (uint64_t)gridDim.x * blockDim.x)
    labels[x] = (uint32_t)x;
}

// ---- workspace ------------------------------------------------------------------------------------
// par and rank (the rounds' root marks until step 4): 8 B per vertex; two lists of min(m, n - 1) ends
// (8 B each: the compaction is out of place) and as many keys for the count cut; the tile counts of
// the larger of the two scans (and the weight cut's flagged counts); the status block with the jump
// flags and the select's histogram.
struct Layout {
  uint64_t cap;
  size_t par, rank, ea, eb, keys, tiles, tiles2, status, hist, total;
};

static inline uint64_t flag_tiles(uint64_t m) { return (m + 15 + LB_FLAG_TILE - 1) / LB_FLAG_TILE; }  // any of 16 starts

static Layout layout(uint32_t n, uint64_t m) {
  Layout l;
  l.cap = n ? (m < (uint64_t)n - 1 ? m : (uint64_t)n - 1) : 0;
  const uint64_t ft = flag_tiles(m), vt = ((uint64_t)n + LB_VERT_TILE - 1) / LB_VERT_TILE;
  size_t o = 0;
  l.par = o; o += align256((size_t)n * 4);
  l.rank = o; o += align256((size_t)n * 4);
  l.ea = o; o += align256((size_t)l.cap * 8);
  l.eb = o; o += align256((size_t)l.cap * 8);
  l.keys = o; o += align256((size_t)l.cap * 8);
  l.tiles = o; o += align256((size_t)(ft > vt ? ft : vt) * 4);
  l.tiles2 = o; o += align256((size_t)ft * 4);  // the weight cut's second count per tile: flagged
  l.status = o; o += 256;                       // ST_SLOTS slots + the jump flags
  l.hist = o; o += 1024;
  l.total = o;
  return l;
}

static int read_status(uint64_t *h, const uint64_t *d_status, hipStream_t st) {
  GHS_HIP_CHECK(hipMemcpyAsync(h, d_status, ST_SLOTS * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipStreamSynchronize(st));
  return GHS_OK;
}

static inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace labels
}  // namespace ghs

using namespace ghs;
using namespace ghs::labels;

extern "C" {

size_t ghs_forest_labels_workspace_bytes(uint32_t n, uint64_t m) { return layout(n, m).total; }

int ghs_forest_labels_device(uint32_t n, uint64_t m, const uint32_t *d_u, const uint32_t *d_v, const uint32_t *d_w,
                             const uint8_t *d_in_mst, uint32_t mode, uint64_t param, uint32_t *d_labels,
                             void *d_workspace, size_t workspace_bytes, void *stream, ghs_labels_result_t *result) {
  hipStream_t st = (hipStream_t)stream;
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
  if (!d_labels) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if ((uintptr_t)d_labels & 3) GHS_FAIL(GHS_E_ARG, "labels must be 4-byte aligned");
  const Layout l = layout(n, m);
  if (m) {
    if (!d_u || !d_v || !d_w || !d_in_mst || !d_workspace) GHS_FAIL(GHS_E_ARG, "NULL pointer");
    if (((uintptr_t)d_u | (uintptr_t)d_v | (uintptr_t)d_w | (uintptr_t)d_workspace) & 15)
      GHS_FAIL(GHS_E_ARG, "u, v, w and the workspace must be 16-byte aligned");
    if (workspace_bytes < l.total) GHS_FAIL(GHS_E_NOMEM, "workspace too small");
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");

  const auto t0 = std::chrono::steady_clock::now();
  if (m == 0) {
    k_lb_identity<<<grid_for(n, LB_BLOCK), LB_BLOCK, 0, st>>>(d_labels, n);
    GHS_HIP_CHECK(hipGetLastError());
    GHS_HIP_CHECK(hipStreamSynchronize(st));
    result->num_clusters = n;
    result->is_forest = 1;
    result->ms_total = ms_since(t0);
    return GHS_OK;
  }
  int canon = 0;
  const int rc = ghs_check_canonical(n, m, d_u, d_v, stream, &canon);
  if (rc != GHS_OK) return rc;
  if (!canon) GHS_FAIL(GHS_E_NONCANON, "edge list is not canonical");

  char *base = (char *)d_workspace;
  uint32_t *par = (uint32_t *)(base + l.par);
  uint32_t *rank = (uint32_t *)(base + l.rank), *mark = rank;
  uint2 *cur = (uint2 *)(base + l.ea), *nxt = (uint2 *)(base + l.eb);
  uint64_t *keys = (uint64_t *)(base + l.keys);
  uint32_t *tiles = (uint32_t *)(base + l.tiles);
  uint64_t *status = (uint64_t *)(base + l.status);
  uint32_t *tiles2 = (uint32_t *)(base + l.tiles2);
  uint32_t *chg = (uint32_t *)(status + ST_SLOTS);
  uint32_t *hist = (uint32_t *)(base + l.hist);
  uint64_t h[ST_SLOTS];

  // step 1: count (the weight cut fused), the count comes back first
  GHS_HIP_CHECK(hipMemsetAsync(status, 0, ST_SLOTS * sizeof(uint64_t), st));
  const uint64_t lo = (uintptr_t)d_in_mst & 15, hi = lo + m;
  const uintptr_t frame = (uintptr_t)d_in_mst - lo;
  const unsigned ftiles = (unsigned)((hi + LB_FLAG_TILE - 1) / LB_FLAG_TILE);  // <= flag_tiles(m)
  const uint32_t thr = (uint32_t)param;
  const bool wcut = mode == GHS_CUT_WEIGHT;
  if (wcut) k_lb_flag_count<true><<<ftiles, LB_BLOCK, 0, st>>>(frame, lo, hi, d_w, thr, tiles, tiles2);
  else k_lb_flag_count<false><<<ftiles, LB_BLOCK, 0, st>>>(frame, lo, hi, d_w, thr, tiles, tiles2);
  k_lb_tile_scan<<<1, 1024, 0, st>>>(tiles, ftiles, status + ST_KEPT, wcut ? tiles2 : nullptr, status + ST_FLAGGED);
  k_lb_init<<<grid_for(((uint64_t)n + 3) / 4, LB_BLOCK), LB_BLOCK, 0, st>>>(par, mark, n);
  GHS_HIP_CHECK(hipGetLastError());
  if (int e = read_status(h, status, st)) return e;
  const uint64_t T = wcut ? h[ST_FLAGGED] : h[ST_KEPT];  // without the weight cut every flagged edge is kept
  if (T > l.cap) GHS_FAIL(GHS_E_ARG, "more flags than a forest can hold");
  uint64_t kept = h[ST_KEPT];
  if (kept > T) GHS_FAIL(GHS_E_STATE, "labels: more edges kept than flagged");
  uint64_t d = 0;
  if (mode == GHS_CUT_COUNT) {  // d = clamp(k - (n - |T|), 0, |T|); n - |T| >= 1
    const uint64_t comps = (uint64_t)n - T;
    d = param > comps ? (param - comps < T ? param - comps : T) : 0;
  }
  if (mode == GHS_CUT_WEIGHT) k_lb_write_edges<true, false><<<ftiles, LB_BLOCK, 0, st>>>(frame, lo, hi, d_u, d_v, d_w, thr, tiles, cur, keys, l.cap);
  else if (d) k_lb_write_edges<false, true><<<ftiles, LB_BLOCK, 0, st>>>(frame, lo, hi, d_u, d_v, d_w, thr, tiles, cur, keys, l.cap);
  else k_lb_write_edges<false, false><<<ftiles, LB_BLOCK, 0, st>>>(frame, lo, hi, d_u, d_v, d_w, thr, tiles, cur, keys, l.cap);
  GHS_HIP_CHECK(hipGetLastError());

  // step 2: the count cut — the smallest key dropped is the one at ascending position |T| - d
  if (d) {
    GHS_HIP_CHECK(hipMemsetAsync(hist, 0, 1024, st));
    GHS_HIP_CHECK(hipMemsetAsync(status + ST_KEPT, 0, sizeof(uint64_t), st));  // the cut counts K again
    const unsigned sgrid = grid_for(T, LB_BLOCK * LB_KEYS_PER_THREAD);
    for (int shift = 56; shift >= 0; shift -= 8) {
      k_lb_sel_hist<<<sgrid, LB_BLOCK, 0, st>>>(keys, T, shift, status, hist);
      k_lb_sel_pick<<<1, 256, 0, st>>>(hist, shift, T - d, status);
    }
    k_lb_cut<<<grid_for(T, LB_BLOCK * LB_ITEMS), LB_BLOCK, 0, st>>>(cur, keys, T, nxt, l.cap, status);
    GHS_HIP_CHECK(hipGetLastError());
    std::swap(cur, nxt);
    kept = T - d;  // keys are distinct: exactly |T| - d lie below the cut key (checked with the last read)
  }

  // step 3: hook rounds
  uint64_t live = kept;
  uint64_t roots_at[LB_MAX_ROUNDS + 1];  // live roots after round r; [0]: a bound before round 1
  roots_at[0] = 2 * kept < n ? 2 * kept : n;
  uint32_t rounds = 0;
  while (live) {
    if (rounds >= LB_MAX_ROUNDS) GHS_FAIL(GHS_E_ROUNDCAP, "labels: round cap exceeded");
    ++rounds;
    GHS_HIP_CHECK(hipMemsetAsync(status + ST_LIVE, 0, LB_ROUND_CLEAR, st));
    const unsigned egrid = grid_for(live, LB_BLOCK);
    k_lb_hook<<<egrid, LB_BLOCK, 0, st>>>(cur, live, par);
    int j = 0;
    for (uint64_t reach = 1; reach < roots_at[rounds - 1] && j < LB_MAX_JUMPS; reach *= LB_JUMP_HOPS, ++j)
      k_lb_jump_ends<<<egrid, LB_BLOCK, 0, st>>>(cur, live, par, j ? chg + j - 1 : nullptr, chg + j);
    k_lb_compact<<<grid_for(live, LB_BLOCK * LB_ITEMS), LB_BLOCK, 0, st>>>(cur, live, par, nxt, l.cap, mark, rounds, status);
    GHS_HIP_CHECK(hipGetLastError());
    if (int e = read_status(h, status, st)) return e;
    roots_at[rounds] = h[ST_ROOTS];
    if (h[ST_LIVE] > live) GHS_FAIL(GHS_E_STATE, "labels: a round grew the live list");
    if (rounds >= 2 && roots_at[rounds] > roots_at[rounds - 2] / 2)
      GHS_FAIL(GHS_E_STATE, "labels: two rounds did not halve the live roots");
    live = h[ST_LIVE];
    std::swap(cur, nxt);
  }

  // step 4: every vertex to its root, roots ranked in vertex order, labels gathered
  GHS_HIP_CHECK(hipMemsetAsync(chg, 0, LB_MAX_JUMPS * sizeof(uint32_t), st));
  if (rounds) {
    const unsigned vgrid = grid_for(n, LB_BLOCK);
    int j = 0;
    for (uint64_t reach = 1; reach < (uint64_t)rounds + 1 && j < LB_MAX_JUMPS; reach *= LB_JUMP_HOPS, ++j)
      k_lb_jump_all<<<vgrid, LB_BLOCK, 0, st>>>(par, n, j ? chg + j - 1 : nullptr, chg + j);
  }
  const unsigned vtiles = (unsigned)(((uint64_t)n + LB_VERT_TILE - 1) / LB_VERT_TILE);
  k_lb_root_count<<<vtiles, LB_BLOCK, 0, st>>>(par, n, tiles);
  k_lb_tile_scan<<<1, 1024, 0, st>>>(tiles, vtiles, status + ST_CLUSTERS, nullptr, nullptr);
  k_lb_root_rank<<<vtiles, LB_BLOCK, 0, st>>>(par, n, tiles, rank);
  k_lb_labels<<<grid_for(((uint64_t)n + 3) / 4, LB_BLOCK), LB_BLOCK, 0, st>>>(par, rank, d_labels, n,
                                                                             ((uintptr_t)d_labels & 15) == 0);
  GHS_HIP_CHECK(hipGetLastError());
  if (int e = read_status(h, status, st)) return e;
  if (h[ST_KEPT] != kept) GHS_FAIL(GHS_E_STATE, "labels: the cut kept another number of edges than |T| - d");

  result->flagged_edges = T;
  result->kept_edges = kept;
  result->dropped_edges = T - kept;
  result->num_clusters = h[ST_CLUSTERS];
  result->cut_key = d ? h[ST_CUTKEY] : ~0ull;
  result->rounds = rounds;
  result->is_forest = result->num_clusters == (uint64_t)n - kept ? 1u : 0u;
  result->ms_total = ms_since(t0);
  return GHS_OK;
}

}  // extern "C"
