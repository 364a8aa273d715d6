// Rooted forest (ABI 10 addition, ghs_forest_root_device): parent, parent edge, depth, DFS preorder
// and subtree size of every vertex of the flagged forest, each tree rooted at its smallest vertex.
//
// The reference's nodes end a run with in_branch, the neighbour towards their fragment's core
// (ghs_implementation.py:63,212, ghs_implementation_mpi.py:57,309); its REPORT / CHANGEROOT
// convergecasts walk those pointers. The Boruvka engine returns flags only; this entry gives the
// orientation back, on the device, for forests of any depth: no pass is level-synchronous.
//
// Pipeline (everything on `stream`; host syncs: 4 + one per ranking round):
//   1. count the flags per 4096-flag tile, scan, gather (u, v, eid) of the flagged edges in eid order:
//      forward arc j = u -> v, already grouped by u with v ascending;
//   2. a stable rocPRIM pairs sort of the tree edges by v gives the reverse arcs v -> u grouped by v
//      with u ascending (arc id T + k); run boundaries of both orders give every vertex its adjacency
//      {reverse block, forward block} = its neighbours in ascending id, with no merge and no atomics;
//   3. succ(x -> y) = the arc after (y -> x) in y's cyclic adjacency: a permutation of the 2|T| arcs
//      whatever T is, one cycle per tree (its Euler tour) when T is a forest;
//   4. splitters = the first arc of every vertex that is the smallest within two hops (no smaller
//      neighbour, and the smallest neighbour of each of its neighbours: a tree's root is one) + a
//      hashed 1 in 64 sample of the arc ids; one lane walks a splitter's sublist to the next splitter:
//      length and the smallest arc key (source vertex, position in its adjacency) seen;
//   5. Wyllie doubling with min-carry on the circular list of splitters gives every tour its smallest
//      key = the first arc of its smallest vertex, which on a forest is a splitter: the tour is broken
//      there; a second doubling along the predecessor links ranks the splitters (tour positions);
//   6. tree sizes (tour length / 2 + 1) scanned over the roots in vertex order give every tour its
//      base; a second walk writes every arc's global tour position;
//   7. of the two arcs of a tree edge the one met first is the down arc: parent, parent_eid and
//      size = (pos(up) - pos(down) + 1) / 2; a scan of the down-arc marks in tour order gives
//      D = down arcs so far, depth = 2 D - (pos + 1), pre = D + (roots up to this tree) - 1.
// No loop depends on T being acyclic: succ is a permutation, so every walk returns to a splitter.
//
// This translation unit includes common.h only and launches only its own kernels; it calls the
// public ghs_check_canonical first, so every index below is in range.
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <utility>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "common.h"

namespace ghs {
namespace root {

constexpr int RT_BLOCK = 256;
constexpr int RT_FLAGS_PER_THREAD = 16;                                      // one 16-byte load
constexpr uint64_t RT_FLAG_TILE = (uint64_t)RT_BLOCK * RT_FLAGS_PER_THREAD;  // flags per block
constexpr int RT_SCAN_ITEMS = 4;                                             // items per thread of a scan pass
constexpr uint64_t RT_SCAN_TILE = (uint64_t)RT_BLOCK * RT_SCAN_ITEMS;        // items per block of a scan pass
constexpr uint32_t RT_SAMPLE_MASK = 63;  // hashed splitters: mix32(arc) & mask == 0 (1 in 64; measured 8 .. 128)
constexpr uint32_t RT_NONE = 0xffffffffu;
constexpr int RT_MAX_PHASE_ROUNDS = 34;  // ceil(log2 2|T|) + 1 <= 33 for |T| < 2^31

// status block (uint64 slots, device), then 2 * RT_MAX_PHASE_ROUNDS round flags (uint32)
enum { ST_FLAGGED = 0, ST_NODES, ST_REACHED, ST_VTOTAL, ST_MAXDEPTH, ST_MARKS, ST_SLOTS };

struct Adj {  // a vertex's arcs: reverse arcs T + [rs, re) (smaller neighbours), forward arcs [fs, fe)
  uint32_t rs, re, fs, fe;
};
struct Arc {  // 8 bytes: one gather per hop of a walk
  uint32_t succ, src;
};
struct MinNode {  // 16 bytes: a splitter in the min-carry doubling
  uint64_t key;
  uint32_t nxt, pad;
};
struct RankNode {  // 8 bytes: a splitter in the ranking
  uint32_t ptr, w;
};
// 8 bytes per tour position. Summed along the tour: downs adds (down arcs so far), roots takes the
// maximum (set at a tour's first position to the number of roots up to its own, which grows from
// tour to tour: the scan carries it to every position of the tour).
struct alignas(8) Mark {
  uint32_t downs, roots;
  Mark() = default;
  __host__ __device__ Mark(int) : downs(0), roots(0) {}
  __host__ __device__ Mark(uint32_t d, uint32_t r) : downs(d), roots(r) {}
  __host__ __device__ Mark operator+(const Mark &o) const { return Mark(downs + o.downs, roots > o.roots ? roots : o.roots); }
  __host__ __device__ Mark &operator+=(const Mark &o) { return *this = *this + o; }
};

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static inline unsigned grid_for(uint64_t items, unsigned per_block, unsigned cap = 2048) {
  uint64_t g = (items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

static inline uint32_t ceil_log2(uint64_t x) {
  uint32_t b = 0;
  while (((uint64_t)1 << b) < x) ++b;
  return b;
}

__device__ __forceinline__ uint32_t block_sum(uint32_t c, uint32_t *s_w) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x / 64] = c;
  __syncthreads();
  uint32_t t = 0;
#pragma unroll
  for (int w = 0; w < RT_BLOCK / 64; ++w) t += s_w[w];
  __syncthreads();
  return t;
}

// exclusive prefix of x over the block's 256 threads (type-generic: an LDS scan); *total: the sum
template <typename V>
__device__ __forceinline__ V block_excl(V x, V *s_v, V *total) {
  s_v[threadIdx.x] = x;
  __syncthreads();
#pragma unroll
  for (int d = 1; d < RT_BLOCK; d <<= 1) {
    const V o = threadIdx.x >= (unsigned)d ? s_v[threadIdx.x - d] : (V)0;
    __syncthreads();
    s_v[threadIdx.x] = o + s_v[threadIdx.x];
    __syncthreads();
  }
  const V exc = threadIdx.x ? s_v[threadIdx.x - 1] : (V)0;  // Mark's sum has no inverse: no inc - x
  *total = s_v[RT_BLOCK - 1];
  __syncthreads();
  return exc;
}

// ---- scans: tile sums, one block over the tile sums, the tiles in place ------------------------------
template <typename V>
__global__ __launch_bounds__(RT_BLOCK) void k_rt_scan_sums(const V *__restrict__ in, uint64_t N, V *__restrict__ tile_sum) {
  __shared__ V s_v[RT_BLOCK];
  const uint64_t i0 = blockIdx.x * RT_SCAN_TILE + (uint64_t)threadIdx.x * RT_SCAN_ITEMS;
  V s = 0;
#pragma unroll
  for (int k = 0; k < RT_SCAN_ITEMS; ++k)
    if (i0 + k < N) s += in[i0 + k];
  V tot;
  (void)block_excl<V>(s, s_v, &tot);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = tot;
}

// exclusive scan of the tile sums in place (one block of 1024), the total to *total
template <typename V>
__global__ __launch_bounds__(1024) void k_rt_tile_scan(V *__restrict__ cnt, uint32_t ntiles, V *__restrict__ total) {
  __shared__ V s_part[1024];
  const uint32_t per = (ntiles + 1023) / 1024;
  const uint64_t b = (uint64_t)threadIdx.x * per;
  V sum = 0;
  for (uint32_t i = 0; i < per && b + i < ntiles; ++i) sum += cnt[b + i];
  s_part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const V o = threadIdx.x >= (unsigned)d ? s_part[threadIdx.x - d] : (V)0;
    __syncthreads();
    s_part[threadIdx.x] = o + s_part[threadIdx.x];
    __syncthreads();
  }
  V run = threadIdx.x ? s_part[threadIdx.x - 1] : (V)0;
  for (uint32_t i = 0; i < per && b + i < ntiles; ++i) {
    const V c = cnt[b + i];
    cnt[b + i] = run;
    run += c;
  }
  if (threadIdx.x == 1023) *total = s_part[1023];
}

template <typename V, bool INCLUSIVE>
__global__ __launch_bounds__(RT_BLOCK) void k_rt_scan_apply(V *__restrict__ data, uint64_t N, const V *__restrict__ tile_off) {
  __shared__ V s_v[RT_BLOCK];
  const uint64_t i0 = blockIdx.x * RT_SCAN_TILE + (uint64_t)threadIdx.x * RT_SCAN_ITEMS;
  V x[RT_SCAN_ITEMS];
  V s = 0;
#pragma unroll
  for (int k = 0; k < RT_SCAN_ITEMS; ++k) {
    x[k] = i0 + k < N ? data[i0 + k] : (V)0;
    s += x[k];
  }
  V tot;
  V run = tile_off[blockIdx.x] + block_excl<V>(s, s_v, &tot);
#pragma unroll
  for (int k = 0; k < RT_SCAN_ITEMS; ++k) {
    if (i0 + k < N) data[i0 + k] = INCLUSIVE ? run + x[k] : run;
    run += x[k];
  }
}

// ---- step 1: the flagged edges, counted and gathered --------------------------------------------------
// The flags may start at any byte. They are read in the 16-byte-aligned frame that contains them:
// frame byte p holds the flag of edge p - lo for p in [lo, hi), lo = the pointer's low 4 bits. A
// thread owns 16 frame bytes: one 16-byte load when all of them are flags (always aligned), byte
// loads with a bound check at the head and the tail. Nothing outside [lo, hi) is read.
__device__ __forceinline__ uint32_t flag_mask16(uintptr_t frame, uint64_t p, uint64_t lo, uint64_t hi) {
  uint32_t mask = 0;
  if (p >= hi || p + RT_FLAGS_PER_THREAD <= lo) return 0;
  if (p >= lo && p + RT_FLAGS_PER_THREAD <= hi) {
    const u32x4 q = *reinterpret_cast<const u32x4 *>(frame + p);
    const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((wd[k] >> (8 * j)) & 0xffu) mask |= 1u << (4 * k + j);
  } else {
    for (int j = 0; j < RT_FLAGS_PER_THREAD; ++j)
      if (p + j >= lo && p + j < hi && *reinterpret_cast<const uint8_t *>(frame + p + j)) mask |= 1u << j;
  }
  return mask;
}

__global__ __launch_bounds__(RT_BLOCK) void k_rt_flag_count(uintptr_t frame, uint64_t lo, uint64_t hi,
                                                            uint32_t *__restrict__ tile_cnt) {
  __shared__ uint32_t s_w[RT_BLOCK / 64];
  const uint64_t p = blockIdx.x * RT_FLAG_TILE + (uint64_t)threadIdx.x * RT_FLAGS_PER_THREAD;
  const uint32_t t = block_sum((uint32_t)__popc(flag_mask16(frame, p, lo, hi)), s_w);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = t;
}

// flagged edge e at rank j -> eu[j], ev[j], eeid[j] (eid order = sorted by (u, v))
__global__ __launch_bounds__(RT_BLOCK) void k_rt_gather_edges(uintptr_t frame, uint64_t lo, uint64_t hi,
                                                              const uint32_t *__restrict__ u,
                                                              const uint32_t *__restrict__ v,
                                                              const uint32_t *__restrict__ tile_off,
                                                              uint32_t *__restrict__ eu, uint32_t *__restrict__ ev,
                                                              uint32_t *__restrict__ eeid, uint64_t cap) {
  __shared__ uint32_t s_v[RT_BLOCK];
  const uint64_t p = blockIdx.x * RT_FLAG_TILE + (uint64_t)threadIdx.x * RT_FLAGS_PER_THREAD;
  uint32_t mask = flag_mask16(frame, p, lo, hi);
  uint32_t tot;
  uint64_t o = (uint64_t)tile_off[blockIdx.x] + block_excl<uint32_t>((uint32_t)__popc(mask), s_v, &tot);
  while (mask) {
    const int j = __ffs(mask) - 1;
    mask &= mask - 1;
    const uint64_t e = p + j - lo;
    if (o < cap) {  // the host has checked the count against cap already
      eu[o] = u[e];
      ev[o] = v[e];
      eeid[o] = (uint32_t)e;
    }
    ++o;
  }
}

// ---- step 2: adjacency ---------------------------------------------------------------------------------
// inv[perm[k]] = k: the reverse arc of tree edge j is T + inv[j]
__global__ __launch_bounds__(RT_BLOCK) void k_rt_inverse(const uint32_t *__restrict__ perm, uint32_t *__restrict__ inv,
                                                         uint64_t T) {
  for (uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; k < T; k += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t j = perm[k];
    if (j < T) inv[j] = (uint32_t)k;
  }
}

// run boundaries of a sorted key array: adj[key].{rs, re} (FWD = false) or .{fs, fe} (FWD = true).
// adj was cleared: a vertex without a run keeps an empty range. Every slot has one writer.
template <bool FWD>
__global__ __launch_bounds__(RT_BLOCK) void k_rt_bounds(const uint32_t *__restrict__ keys, uint64_t T,
                                                        Adj *__restrict__ adj) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < T; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t k = keys[i];
    if (i == 0 || keys[i - 1] != k) (FWD ? adj[k].fs : adj[k].rs) = (uint32_t)i;
    if (i + 1 == T || keys[i + 1] != k) (FWD ? adj[k].fe : adj[k].re) = (uint32_t)i + 1;
  }
}

// A local minimum x (no reverse arc) is demoted when a neighbour y has a neighbour below x: y's
// smallest neighbour is the source of its first reverse arc. Every writer stores the same byte. A
// tree's smallest vertex is never demoted.
__global__ __launch_bounds__(RT_BLOCK) void k_rt_demote(uint32_t T, const uint32_t *__restrict__ eu,
                                                        const uint32_t *__restrict__ ev,
                                                        const uint32_t *__restrict__ perm, const Adj *__restrict__ adj,
                                                        uint8_t *__restrict__ demoted) {
  for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < T; j += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t x = eu[j];
    const Adj ax = adj[x];
    if (ax.rs != ax.re) continue;
    const Adj ay = adj[ev[j]];
    if (ay.rs >= ay.re) continue;  // never: x itself is a smaller neighbour of y
    const uint32_t k = perm[ay.rs];
    if (k < T && eu[k] < x) demoted[x] = 1;
  }
}

// ---- step 3 + 4a: the Euler successor of every arc and the splitter bits -----------------------------
// One thread per arc, whole waves (the ballot is the bit word). Arc a < T: forward arc of tree edge a;
// arc T + k: the k-th reverse arc in (v, u) order.
__global__ __launch_bounds__(RT_BLOCK) void k_rt_succ(uint32_t T, const uint32_t *__restrict__ eu,
                                                      const uint32_t *__restrict__ ev,
                                                      const uint32_t *__restrict__ kv,
                                                      const uint32_t *__restrict__ perm,
                                                      const uint32_t *__restrict__ inv, const Adj *__restrict__ adj,
                                                      const uint8_t *__restrict__ demoted, Arc *__restrict__ arcs,
                                                      uint64_t *__restrict__ bits,
                                                      uint32_t *__restrict__ wcnt) {
  const uint64_t a64 = blockIdx.x * (uint64_t)RT_BLOCK + threadIdx.x;
  const uint64_t A = 2ull * T;
  bool spl = false;
  if (a64 < A) {
    const uint32_t a = (uint32_t)a64;
    spl = (mix32(a) & RT_SAMPLE_MASK) == 0;
    Arc r;
    if (a < T) {
      const uint32_t x = eu[a], y = ev[a];
      const uint32_t k = inv[a];  // the twin y -> x is reverse arc k; what follows it around y?
      const Adj ay = adj[y];
      r.succ = k + 1 < ay.re ? T + k + 1 : (ay.fs < ay.fe ? ay.fs : T + ay.rs);
      r.src = x;
      const Adj ax = adj[x];
      if (ax.rs == ax.re && ax.fs == a && !demoted[x]) spl = true;  // the first arc of a two-hop minimum
    } else {
      const uint32_t k = a - T;
      uint32_t j = perm[k];
      if (j >= T) j = 0;  // never: perm is a permutation of [0, T)
      const uint32_t y = eu[j];  // the twin y -> x is forward arc j
      const Adj ay = adj[y];
      r.succ = j + 1 < ay.fe ? j + 1 : (ay.rs < ay.re ? T + ay.rs : ay.fs);
      r.src = kv[k];
    }
    if (r.succ >= A) r.succ = a;  // never on a canonical list; keeps every later index in range
    arcs[a] = r;
  }
  const uint64_t word = __ballot(spl);
  if ((threadIdx.x & 63) == 0 && (a64 & ~63ull) < A) {
    bits[a64 >> 6] = word;
    wcnt[a64 >> 6] = (uint32_t)__popcll(word);
  }
}

__device__ __forceinline__ bool is_splitter(const uint64_t *__restrict__ bits, uint32_t a) {
  return (bits[a >> 6] >> (a & 63)) & 1ull;
}

__device__ __forceinline__ uint32_t node_of(const uint64_t *__restrict__ bits, const uint32_t *__restrict__ wpre,
                                            uint32_t a) {
  return wpre[a >> 6] + (uint32_t)__popcll(bits[a >> 6] & ((1ull << (a & 63)) - 1ull));
}

// the splitters in arc order: arc0[node]
__global__ __launch_bounds__(RT_BLOCK) void k_rt_nodes(const uint64_t *__restrict__ bits,
                                                       const uint32_t *__restrict__ wpre, uint64_t words,
                                                       uint32_t *__restrict__ arc0, uint64_t cap) {
  for (uint64_t w = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; w < words; w += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t b = bits[w];
    uint64_t o = wpre[w];
    while (b) {
      const int j = __ffsll((unsigned long long)b) - 1;
      b &= b - 1;
      if (o < cap) arc0[o] = (uint32_t)(w * 64 + j);
      ++o;
    }
  }
}

// ---- step 4b: one lane per splitter walks its sublist ---------------------------------------------------
// Arc key = source vertex << 32 | position class: reverse arcs before forward arcs, so the smallest
// key of a vertex's arcs is its first adjacency entry. Keys are distinct. succ is a permutation, so
// the walk meets a splitter (its own at the latest) after at most 2|T| hops.
__global__ __launch_bounds__(RT_BLOCK) void k_rt_walk_measure(uint32_t nodes, uint32_t T,
                                                              const uint32_t *__restrict__ arc0,
                                                              const Arc *__restrict__ arcs,
                                                              const uint64_t *__restrict__ bits,
                                                              const uint32_t *__restrict__ wpre,
                                                              MinNode *__restrict__ mn, uint64_t *__restrict__ nkey,
                                                              uint32_t *__restrict__ nlen, uint32_t *__restrict__ prv,
                                                              uint64_t *__restrict__ status) {
  __shared__ uint64_t s_v[RT_BLOCK];
  const uint64_t A = 2ull * T;
  uint64_t reached = 0;
  for (uint64_t s0 = blockIdx.x * (uint64_t)blockDim.x; s0 < nodes; s0 += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t s = s0 + threadIdx.x;
    uint32_t len = 0;
    if (s < nodes) {
      uint32_t a = arc0[s];
      uint64_t key = ~0ull;
      do {
        const Arc r = arcs[a];
        const uint64_t k = ((uint64_t)r.src << 32) | (a < T ? a + T : a - T);
        key = k < key ? k : key;
        ++len;
        a = r.succ;
      } while (!is_splitter(bits, a) && len < A);
      uint32_t nx = node_of(bits, wpre, a);
      if (nx >= nodes) nx = (uint32_t)s;  // never: a is a splitter
      MinNode m;
      m.key = key;
      m.nxt = nx;
      m.pad = 0;
      mn[s] = m;
      nkey[s] = key;
      nlen[s] = len;
      prv[nx] = (uint32_t)s;
    }
    reached += len;
  }
  uint64_t tot;
  (void)block_excl<uint64_t>(reached, s_v, &tot);
  if (threadIdx.x == 0 && tot) atomicAdd((unsigned long long *)(status + ST_REACHED), (unsigned long long)tot);
}

// ---- step 5: doubling over the circular list of splitters ----------------------------------------------
// key[s] <- min over the next 2^r nodes. A round that changes no key ends the phase: every orbit of
// the 2^r-step tiles its cycle, so equal windows along it all hold the cycle's minimum.
__global__ __launch_bounds__(RT_BLOCK) void k_rt_min_round(uint32_t nodes, const MinNode *__restrict__ in,
                                                           MinNode *__restrict__ out, uint32_t *__restrict__ chg) {
  bool any = false;
  for (uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; s < nodes; s += (uint64_t)gridDim.x * blockDim.x) {
    MinNode m = in[s];
    const MinNode o = in[m.nxt];
    if (o.key < m.key) {
      m.key = o.key;
      any = true;
    }
    m.nxt = o.nxt < nodes ? o.nxt : m.nxt;
    out[s] = m;
  }
  if (any) *chg = 1;
}

// the head of a cycle is the node that holds its smallest key; the list is broken in front of it and
// ranked along the predecessor links: w[s] = arcs in the tour before s's sublist
__global__ __launch_bounds__(RT_BLOCK) void k_rt_rank_init(uint32_t nodes, const MinNode *__restrict__ mn,
                                                           const uint64_t *__restrict__ nkey,
                                                           const uint32_t *__restrict__ nlen,
                                                           const uint32_t *__restrict__ prv,
                                                           RankNode *__restrict__ rk, uint32_t *__restrict__ nroot) {
  for (uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; s < nodes; s += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t cyc = mn[s].key;
    nroot[s] = (uint32_t)(cyc >> 32);
    RankNode r;
    if (nkey[s] == cyc) {
      r.ptr = RT_NONE;
      r.w = 0;
    } else {
      uint32_t p = prv[s];
      if (p >= nodes) p = (uint32_t)s;  // never: prv is a permutation
      r.ptr = p;
      r.w = nlen[p];
    }
    rk[s] = r;
  }
}

__global__ __launch_bounds__(RT_BLOCK) void k_rt_rank_round(uint32_t nodes, const RankNode *__restrict__ in,
                                                            RankNode *__restrict__ out, uint32_t *__restrict__ chg) {
  bool open = false;
  for (uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; s < nodes; s += (uint64_t)gridDim.x * blockDim.x) {
    RankNode r = in[s];
    if (r.ptr != RT_NONE) {
      const RankNode o = in[r.ptr];
      r.w += o.w;
      r.ptr = o.ptr < nodes ? o.ptr : RT_NONE;
      open |= r.ptr != RT_NONE;
    }
    out[s] = r;
  }
  if (open) *chg = 1;
}

// ---- step 6: tree sizes, tour bases ---------------------------------------------------------------------
// the head (w == 0; every other node has w >= 1): tour length = w + len of the node in front of it
__global__ __launch_bounds__(RT_BLOCK) void k_rt_tree_sizes(uint32_t nodes, const RankNode *__restrict__ rk,
                                                            const uint32_t *__restrict__ nlen,
                                                            const uint32_t *__restrict__ prv,
                                                            const uint32_t *__restrict__ nroot, uint32_t n,
                                                            uint32_t *__restrict__ tsz) {
  for (uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; s < nodes; s += (uint64_t)gridDim.x * blockDim.x) {
    if (rk[s].w != 0) continue;
    uint32_t t = prv[s];
    if (t >= nodes) t = (uint32_t)s;
    const uint32_t len = rk[t].w + nlen[t];
    const uint32_t r = nroot[s];
    if (r < n) tsz[r] = len / 2 + 1;
  }
}

// a root's scan value: tree size << 32 | 1 (an isolated vertex: size 1); 0 for every other vertex
__global__ __launch_bounds__(RT_BLOCK) void k_rt_vert_values(uint32_t n, const Adj *__restrict__ adj,
                                                             const uint32_t *__restrict__ tsz, uint64_t *__restrict__ vinfo) {
  for (uint64_t x = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; x < n; x += (uint64_t)gridDim.x * blockDim.x) {
    const Adj a = adj[x];
    const uint32_t sz = (a.rs == a.re && a.fs == a.fe) ? 1u : tsz[x];
    vinfo[x] = sz ? ((uint64_t)sz << 32) | 1ull : 0ull;
  }
}

// vinfo is now the exclusive prefix: vertices in trees before x << 32 | roots before x. The roots'
// outputs, and at the base of an edged root's tour the number of roots up to it (the high word of
// the mark the down-arc scan sums; the low word is written with the other down arcs).
__global__ __launch_bounds__(RT_BLOCK) void k_rt_roots(uint32_t n, const Adj *__restrict__ adj,
                                                       const uint32_t *__restrict__ tsz, const uint64_t *__restrict__ vinfo,
                                                       uint32_t *__restrict__ parent, uint32_t *__restrict__ parent_eid,
                                                       uint32_t *__restrict__ depth, uint32_t *__restrict__ pre,
                                                       uint32_t *__restrict__ size, Mark *__restrict__ marks, uint64_t A) {
  for (uint64_t x = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; x < n; x += (uint64_t)gridDim.x * blockDim.x) {
    const Adj a = adj[x];
    const bool isolated = a.rs == a.re && a.fs == a.fe;
    const uint32_t sz = isolated ? 1u : tsz[x];
    if (!sz) continue;
    const uint64_t p = vinfo[x];
    const uint32_t before = (uint32_t)(p >> 32), roots = (uint32_t)p;
    parent[x] = RT_NONE;
    parent_eid[x] = RT_NONE;
    depth[x] = 0;
    if (pre) pre[x] = before;
    if (size) size[x] = sz;
    if (!isolated) {
      const uint64_t base = 2ull * (before - roots);
      if (base < A) marks[base].roots = roots + 1;
    }
  }
}

// the second walk: every arc's global tour position
__global__ __launch_bounds__(RT_BLOCK) void k_rt_walk_place(uint32_t nodes, uint32_t T, const uint32_t *__restrict__ arc0,
                                                            const Arc *__restrict__ arcs,
                                                            const uint64_t *__restrict__ bits,
                                                            const RankNode *__restrict__ rk,
                                                            const uint32_t *__restrict__ nroot, uint32_t n,
                                                            const uint64_t *__restrict__ vinfo, uint32_t *__restrict__ gpos) {
  const uint64_t A = 2ull * T;
  for (uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; s < nodes; s += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = nroot[s];
    const uint64_t p = r < n ? vinfo[r] : 0ull;
    uint32_t g = 2u * ((uint32_t)(p >> 32) - (uint32_t)p) + rk[s].w;
    uint32_t a = arc0[s], len = 0;
    do {
      gpos[a] = g++;
      a = arcs[a].succ;
      ++len;
    } while (!is_splitter(bits, a) && len < A);
  }
}

// ---- step 7: down arcs, their scan, the outputs -----------------------------------------------------------
__global__ __launch_bounds__(RT_BLOCK) void k_rt_mark_down(uint32_t T, const uint32_t *__restrict__ inv,
                                                           const uint32_t *__restrict__ gpos, Mark *__restrict__ marks) {
  const uint64_t A = 2ull * T;
  for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < T; j += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t ga = gpos[j], gb = gpos[T + inv[j]];
    const uint32_t g = ga < gb ? ga : gb;
    if (g < A) marks[g].downs = 1;
  }
}

__global__ __launch_bounds__(RT_BLOCK) void k_rt_outputs(uint32_t T, const uint32_t *__restrict__ eu,
                                                         const uint32_t *__restrict__ ev,
                                                         const uint32_t *__restrict__ eeid,
                                                         const uint32_t *__restrict__ inv, const uint32_t *__restrict__ gpos,
                                                         const Mark *__restrict__ scanned,
                                                         uint32_t *__restrict__ parent, uint32_t *__restrict__ parent_eid,
                                                         uint32_t *__restrict__ depth, uint32_t *__restrict__ pre,
                                                         uint32_t *__restrict__ size, uint64_t *__restrict__ status) {
  __shared__ uint32_t s_w[RT_BLOCK / 64];
  const uint64_t A = 2ull * T;
  uint32_t deepest = 0;
  for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < T; j += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t x = eu[j], y = ev[j];
    const uint32_t ga = gpos[j], gb = gpos[T + inv[j]];
    const bool fwd_down = ga < gb;
    const uint32_t child = fwd_down ? y : x, par = fwd_down ? x : y;
    const uint32_t gd = fwd_down ? ga : gb, gu = fwd_down ? gb : ga;
    parent[child] = par;
    parent_eid[child] = eeid[j];
    if (size) size[child] = (gu - gd + 1) / 2;
    uint32_t d = 0, pr = 0;
    if (gd < A) {
      const Mark s = scanned[gd];
      const uint32_t downs = s.downs, roots = s.roots;
      d = 2u * downs - (gd + 1u);
      pr = downs + roots - 1u;
    }
    depth[child] = d;
    if (pre) pre[child] = pr;
    deepest = d > deepest ? d : deepest;
  }
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) {
    const uint32_t o = __shfl_xor(deepest, k);
    deepest = o > deepest ? o : deepest;
  }
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x / 64] = deepest;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < RT_BLOCK / 64; ++w) deepest = s_w[w] > deepest ? s_w[w] : deepest;
    if (deepest) atomicMax((unsigned int *)(status + ST_MAXDEPTH), deepest);
  }
}

// no flagged edge: every vertex is a root
__global__ __launch_bounds__(RT_BLOCK) void k_rt_identity(uint32_t n, uint32_t *__restrict__ parent,
                                                          uint32_t *__restrict__ parent_eid, uint32_t *__restrict__ depth,
                                                          uint32_t *__restrict__ pre, uint32_t *__restrict__ size) {
  for (uint64_t x = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; x < n; x += (uint64_t)gridDim.x * blockDim.x) {
    parent[x] = RT_NONE;
    parent_eid[x] = RT_NONE;
    depth[x] = 0;
    if (pre) pre[x] = (uint32_t)x;
    if (size) size[x] = 1;
  }
}

// ---- workspace ------------------------------------------------------------------------------------------
// C = min(m, n - 1) possible tree edges, A = 2 C arcs, at most A splitters.
//   per vertex (29 B): adjacency ranges 16, tree size 4, root prefix 8, demoted flag 1;
//   per possible tree edge (24 B): eu, ev, eeid, the sorted keys, the sort's permutation, its inverse;
//   per possible arc (84 B): arc record 8, tour position 4, arc0 4, sublist length 4, predecessor 4,
//     sublist key 8, tour root 4, two min-carry buffers 2 x 16 (reused by the down-arc marks, 8),
//     two rank buffers 2 x 8; + 12 B per 64 arcs of splitter bits and their prefix;
//   tile sums of the largest scan, rocPRIM's sort storage, the status block.
struct Layout {
  uint64_t cap;
  size_t adj, tsz, vinfo, demoted, eu, ev, eeid, kv, perm, inv, arcs, gpos, bits, wpre, arc0, nlen, prv, nkey, nroot, ma, mb, ra,
      rb, tiles, prim, prim_bytes, status, total;
};

static inline uint64_t flag_tiles(uint64_t m) { return (m + 15 + RT_FLAG_TILE - 1) / RT_FLAG_TILE; }  // any of 16 starts
static inline uint64_t scan_tiles(uint64_t items) { return (items + RT_SCAN_TILE - 1) / RT_SCAN_TILE; }

static inline unsigned key_bits(uint32_t n) { return n > 2 ? ceil_log2(n) : 1u; }  // keys are < n

static size_t sort_bytes(uint64_t T, uint32_t n) {
  size_t b = 0;
  if (T == 0) return 0;
  (void)rocprim::radix_sort_pairs(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                  rocprim::counting_iterator<uint32_t>(0), (uint32_t *)nullptr, (size_t)T, 0u,
                                  key_bits(n));
  return b;
}

static Layout layout(uint32_t n, uint64_t m) {
  Layout l;
  l.cap = n ? (m < (uint64_t)n - 1 ? m : (uint64_t)n - 1) : 0;
  const uint64_t C = l.cap, A = 2 * C, W = (A + 63) / 64;
  uint64_t tiles = flag_tiles(m);
  if (scan_tiles(n) > tiles) tiles = scan_tiles(n);
  if (scan_tiles(A) > tiles) tiles = scan_tiles(A);
  size_t o = 0;
  l.adj = o; o += align256((size_t)n * 16);
  l.tsz = o; o += align256((size_t)n * 4);
  l.vinfo = o; o += align256((size_t)n * 8);
  l.demoted = o; o += align256((size_t)n);
  l.eu = o; o += align256((size_t)C * 4);
  l.ev = o; o += align256((size_t)C * 4);
  l.eeid = o; o += align256((size_t)C * 4);
  l.kv = o; o += align256((size_t)C * 4);
  l.perm = o; o += align256((size_t)C * 4);
  l.inv = o; o += align256((size_t)C * 4);
  l.arcs = o; o += align256((size_t)A * 8);
  l.gpos = o; o += align256((size_t)A * 4);
  l.bits = o; o += align256((size_t)W * 8);
  l.wpre = o; o += align256((size_t)W * 4);
  l.arc0 = o; o += align256((size_t)A * 4);
  l.nlen = o; o += align256((size_t)A * 4);
  l.prv = o; o += align256((size_t)A * 4);
  l.nkey = o; o += align256((size_t)A * 8);
  l.nroot = o; o += align256((size_t)A * 4);
  l.ma = o; o += align256((size_t)A * 16);
  l.mb = o; o += align256((size_t)A * 16);
  l.ra = o; o += align256((size_t)A * 8);
  l.rb = o; o += align256((size_t)A * 8);
  l.tiles = o; o += align256((size_t)tiles * 8);
  l.prim_bytes = align256(sort_bytes(C, n));
  l.prim = o; o += l.prim_bytes;
  l.status = o; o += 1024;
  l.total = o;
  return l;
}

static int read_status(uint64_t *h, const uint64_t *d_status, hipStream_t st) {
  GHS_HIP_CHECK(hipMemcpyAsync(h, d_status, ST_SLOTS * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipStreamSynchronize(st));
  return GHS_OK;
}

static int read_flag(uint32_t *h, const uint32_t *d_flag, hipStream_t st) {
  GHS_HIP_CHECK(hipMemcpyAsync(h, d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipStreamSynchronize(st));
  return GHS_OK;
}

static inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// in-place scan of data[0, N): tile sums, the tile sums, the tiles; the total to *total (device)
template <typename V, bool INCLUSIVE>
static int scan_in_place(V *data, uint64_t N, V *tiles, V *total, hipStream_t st) {
  const unsigned nt = (unsigned)scan_tiles(N);
  k_rt_scan_sums<V><<<nt, RT_BLOCK, 0, st>>>(data, N, tiles);
  k_rt_tile_scan<V><<<1, 1024, 0, st>>>(tiles, nt, total);
  k_rt_scan_apply<V, INCLUSIVE><<<nt, RT_BLOCK, 0, st>>>(data, N, tiles);
  GHS_HIP_CHECK(hipGetLastError());
  return GHS_OK;
}

}  // namespace root
}  // namespace ghs

using namespace ghs;
using namespace ghs::root;

extern "C" {

size_t ghs_forest_root_workspace_bytes(uint32_t n, uint64_t m) { return layout(n, m).total; }

int ghs_forest_root_device(uint32_t n, uint64_t m, const uint32_t *d_u, const uint32_t *d_v, const uint8_t *d_in_mst,
                           uint32_t *d_parent, uint32_t *d_parent_eid, uint32_t *d_depth, uint32_t *d_pre,
                           uint32_t *d_size, void *d_workspace, size_t workspace_bytes, void *stream,
                           ghs_root_result_t *result) {
  hipStream_t st = (hipStream_t)stream;
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_root_result_t{};
  if (n == 0) {
    result->is_forest = 1;
    return GHS_OK;
  }
  if (m >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "m must be < 2^31");
  if (!d_parent || !d_parent_eid || !d_depth) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if (((uintptr_t)d_parent | (uintptr_t)d_parent_eid | (uintptr_t)d_depth | (uintptr_t)d_pre | (uintptr_t)d_size) & 3)
    GHS_FAIL(GHS_E_ARG, "parent, parent_eid, depth, pre and size must be 4-byte aligned");
  if (m) {
    if (!d_u || !d_v || !d_in_mst || !d_workspace) GHS_FAIL(GHS_E_ARG, "NULL pointer");
    if (((uintptr_t)d_u | (uintptr_t)d_v | (uintptr_t)d_workspace) & 15)
      GHS_FAIL(GHS_E_ARG, "u, v and the workspace must be 16-byte aligned");
    if (workspace_bytes < ghs_forest_root_workspace_bytes(n, m)) GHS_FAIL(GHS_E_NOMEM, "workspace too small");
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");

  const auto t0 = std::chrono::steady_clock::now();
  const unsigned vgrid = grid_for(n, RT_BLOCK);
  if (m == 0) {
    k_rt_identity<<<vgrid, RT_BLOCK, 0, st>>>(n, d_parent, d_parent_eid, d_depth, d_pre, d_size);
    GHS_HIP_CHECK(hipGetLastError());
    GHS_HIP_CHECK(hipStreamSynchronize(st));
    result->num_trees = n;
    result->is_forest = 1;
    result->ms_total = ms_since(t0);
    return GHS_OK;
  }
  int canon = 0;
  const int rc = ghs_check_canonical(n, m, d_u, d_v, stream, &canon);
  if (rc != GHS_OK) return rc;
  if (!canon) GHS_FAIL(GHS_E_NONCANON, "edge list is not canonical");

  const Layout l = layout(n, m);
  char *base = (char *)d_workspace;
  Adj *adj = (Adj *)(base + l.adj);
  uint32_t *tsz = (uint32_t *)(base + l.tsz);
  uint64_t *vinfo = (uint64_t *)(base + l.vinfo);
  uint8_t *demoted = (uint8_t *)(base + l.demoted);
  uint32_t *eu = (uint32_t *)(base + l.eu), *ev = (uint32_t *)(base + l.ev), *eeid = (uint32_t *)(base + l.eeid);
  uint32_t *kv = (uint32_t *)(base + l.kv), *perm = (uint32_t *)(base + l.perm), *inv = (uint32_t *)(base + l.inv);
  Arc *arcs = (Arc *)(base + l.arcs);
  uint32_t *gpos = (uint32_t *)(base + l.gpos);
  uint64_t *bits = (uint64_t *)(base + l.bits);
  uint32_t *wpre = (uint32_t *)(base + l.wpre);
  uint32_t *arc0 = (uint32_t *)(base + l.arc0), *nlen = (uint32_t *)(base + l.nlen), *prv = (uint32_t *)(base + l.prv);
  uint64_t *nkey = (uint64_t *)(base + l.nkey);
  uint32_t *nroot = (uint32_t *)(base + l.nroot);
  MinNode *mcur = (MinNode *)(base + l.ma), *mnxt = (MinNode *)(base + l.mb);
  RankNode *rcur = (RankNode *)(base + l.ra), *rnxt = (RankNode *)(base + l.rb);
  Mark *marks = (Mark *)(base + l.ma);  // the down-arc marks, once the min-carry buffers are dead
  void *tiles = base + l.tiles;
  uint64_t *status = (uint64_t *)(base + l.status);
  uint32_t *chg = (uint32_t *)(status + ST_SLOTS);
  uint64_t h[ST_SLOTS];

  // step 1: count, the count comes back first
  GHS_HIP_CHECK(hipMemsetAsync(status, 0, 1024, st));
  const uint64_t lo = (uintptr_t)d_in_mst & 15, hi = lo + m;
  const uintptr_t frame = (uintptr_t)d_in_mst - lo;
  const unsigned ftiles = (unsigned)((hi + RT_FLAG_TILE - 1) / RT_FLAG_TILE);  // <= flag_tiles(m)
  k_rt_flag_count<<<ftiles, RT_BLOCK, 0, st>>>(frame, lo, hi, (uint32_t *)tiles);
  k_rt_tile_scan<uint32_t><<<1, 1024, 0, st>>>((uint32_t *)tiles, ftiles, (uint32_t *)(status + ST_FLAGGED));
  GHS_HIP_CHECK(hipGetLastError());
  if (int e = read_status(h, status, st)) return e;
  const uint64_t T64 = h[ST_FLAGGED];
  if (T64 > l.cap) GHS_FAIL(GHS_E_ARG, "more flags than a forest can hold");
  result->flagged_edges = T64;
  if (T64 == 0) {
    k_rt_identity<<<vgrid, RT_BLOCK, 0, st>>>(n, d_parent, d_parent_eid, d_depth, d_pre, d_size);
    GHS_HIP_CHECK(hipGetLastError());
    GHS_HIP_CHECK(hipStreamSynchronize(st));
    result->num_trees = n;
    result->is_forest = 1;
    result->ms_total = ms_since(t0);
    return GHS_OK;
  }
  const uint32_t T = (uint32_t)T64;
  const uint64_t A = 2ull * T, words = (A + 63) / 64;
  const unsigned egrid = grid_for(T, RT_BLOCK);
  k_rt_gather_edges<<<ftiles, RT_BLOCK, 0, st>>>(frame, lo, hi, d_u, d_v, (const uint32_t *)tiles, eu, ev, eeid, l.cap);
  GHS_HIP_CHECK(hipGetLastError());

  // step 2: reverse arcs, adjacency ranges
  size_t need = sort_bytes(T, n);
  if (need > l.prim_bytes) GHS_FAIL(GHS_E_STATE, "root: the sort needs more storage than the workspace holds");
  GHS_HIP_CHECK(rocprim::radix_sort_pairs(base + l.prim, need, (const uint32_t *)ev, kv,
                                          rocprim::counting_iterator<uint32_t>(0), perm, (size_t)T, 0u, key_bits(n), st));
  GHS_HIP_CHECK(hipMemsetAsync(adj, 0, (size_t)n * sizeof(Adj), st));
  GHS_HIP_CHECK(hipMemsetAsync(tsz, 0, (size_t)n * 4, st));
  GHS_HIP_CHECK(hipMemsetAsync(demoted, 0, (size_t)n, st));
  k_rt_inverse<<<egrid, RT_BLOCK, 0, st>>>(perm, inv, T);
  k_rt_bounds<true><<<egrid, RT_BLOCK, 0, st>>>(eu, T, adj);
  k_rt_bounds<false><<<egrid, RT_BLOCK, 0, st>>>(kv, T, adj);
  k_rt_demote<<<egrid, RT_BLOCK, 0, st>>>(T, eu, ev, perm, adj, demoted);

  // steps 3, 4: successors, splitters
  k_rt_succ<<<(unsigned)((A + RT_BLOCK - 1) / RT_BLOCK), RT_BLOCK, 0, st>>>(T, eu, ev, kv, perm, inv, adj, demoted, arcs, bits,
                                                                              wpre);
  GHS_HIP_CHECK(hipGetLastError());
  if (int e = scan_in_place<uint32_t, false>(wpre, words, (uint32_t *)tiles, (uint32_t *)(status + ST_NODES), st)) return e;
  if (int e = read_status(h, status, st)) return e;
  const uint64_t nodes64 = h[ST_NODES];
  if (nodes64 == 0 || nodes64 > A) GHS_FAIL(GHS_E_STATE, "root: splitter count out of range");
  const uint32_t nodes = (uint32_t)nodes64;
  const unsigned ngrid = grid_for(nodes, RT_BLOCK);
  k_rt_nodes<<<grid_for(words, RT_BLOCK), RT_BLOCK, 0, st>>>(bits, wpre, words, arc0, nodes);
  k_rt_walk_measure<<<ngrid, RT_BLOCK, 0, st>>>(nodes, T, arc0, arcs, bits, wpre, mcur, nkey, nlen, prv, status);
  GHS_HIP_CHECK(hipGetLastError());

  // step 5: the tours' smallest keys, then the splitters' positions; one flag read per round
  const uint32_t phase_cap = ceil_log2(A) + 1;
  uint32_t rounds = 0, flag = 1;
  for (uint32_t r = 0; flag; ++r) {
    if (r >= phase_cap || r >= (uint32_t)RT_MAX_PHASE_ROUNDS) GHS_FAIL(GHS_E_ROUNDCAP, "root: round cap exceeded");
    k_rt_min_round<<<ngrid, RT_BLOCK, 0, st>>>(nodes, mcur, mnxt, chg + r);
    GHS_HIP_CHECK(hipGetLastError());
    if (int e = read_flag(&flag, chg + r, st)) return e;
    std::swap(mcur, mnxt);
    ++rounds;
  }
  k_rt_rank_init<<<ngrid, RT_BLOCK, 0, st>>>(nodes, mcur, nkey, nlen, prv, rcur, nroot);
  flag = 1;
  for (uint32_t r = 0; flag; ++r) {
    if (r >= phase_cap || r >= (uint32_t)RT_MAX_PHASE_ROUNDS) GHS_FAIL(GHS_E_ROUNDCAP, "root: round cap exceeded");
    k_rt_rank_round<<<ngrid, RT_BLOCK, 0, st>>>(nodes, rcur, rnxt, chg + RT_MAX_PHASE_ROUNDS + r);
    GHS_HIP_CHECK(hipGetLastError());
    if (int e = read_flag(&flag, chg + RT_MAX_PHASE_ROUNDS + r, st)) return e;
    std::swap(rcur, rnxt);
    ++rounds;
  }

  // step 6: tree sizes, roots in vertex order, tour bases, positions
  k_rt_tree_sizes<<<ngrid, RT_BLOCK, 0, st>>>(nodes, rcur, nlen, prv, nroot, n, tsz);
  k_rt_vert_values<<<vgrid, RT_BLOCK, 0, st>>>(n, adj, tsz, vinfo);
  GHS_HIP_CHECK(hipGetLastError());
  if (int e = scan_in_place<uint64_t, false>(vinfo, n, (uint64_t *)tiles, status + ST_VTOTAL, st)) return e;
  GHS_HIP_CHECK(hipMemsetAsync(marks, 0, (size_t)A * 8, st));
  k_rt_roots<<<vgrid, RT_BLOCK, 0, st>>>(n, adj, tsz, vinfo, d_parent, d_parent_eid, d_depth, d_pre, d_size,
                                         marks, A);
  k_rt_walk_place<<<ngrid, RT_BLOCK, 0, st>>>(nodes, T, arc0, arcs, bits, rcur, nroot, n, vinfo, gpos);

  // step 7: down arcs, their scan, the outputs
  k_rt_mark_down<<<egrid, RT_BLOCK, 0, st>>>(T, inv, gpos, marks);
  GHS_HIP_CHECK(hipGetLastError());
  if (int e = scan_in_place<Mark, true>(marks, A, (Mark *)tiles, (Mark *)(status + ST_MARKS), st)) return e;
  k_rt_outputs<<<egrid, RT_BLOCK, 0, st>>>(T, eu, ev, eeid, inv, gpos, marks, d_parent, d_parent_eid, d_depth, d_pre,
                                           d_size, status);
  GHS_HIP_CHECK(hipGetLastError());
  if (int e = read_status(h, status, st)) return e;

  result->num_trees = h[ST_VTOTAL] & 0xffffffffull;
  result->max_depth = h[ST_MAXDEPTH] & 0xffffffffull;
  result->rounds = rounds;
  result->is_forest = (h[ST_REACHED] == A && result->num_trees == (uint64_t)n - T) ? 1u : 0u;
  result->ms_total = ms_since(t0);
  return GHS_OK;
}

}  // extern "C"
