// Device verifier (ABI 10 addition, ghs_verify_msf_device): is a flag vector THE minimum spanning
// forest of a canonical edge list — exactly, at any size, without a second solve or a CPU?
//
// The reference checks a run by recomputing the MST with NetworkX (check_mst.py:1-20,
// ghs_implementation.py:746); that stops at a few million edges. MST verification is cheaper than
// construction: with T = the flagged edges and F = MSF(T) under the strict key (w, eid),
//   cyclic_edges    = |T| - |F|                          flagged edges that close a cycle,
//   unspanned_edges = edges of G whose ends lie in different components of T,
//   lighter_edges   = unflagged edges inside one component of T whose key is smaller than the
//                     largest key on the F-path between their ends,
// and the flags are the MSF iff all three are 0. Keys are distinct, so the MSF is unique and that
// verdict is the same statement as "the flags equal canonical Kruskal's, byte for byte".
//
// Path maxima come from King's Boruvka-tree lemma: run plain Boruvka over T alone (|T| <= n - 1, so
// this is cheap) and record, for every fragment f alive at round r, a 16-byte node {the key f chose
// in round r, the dense id of f's fragment at round r + 1}. A fragment with no outgoing T-edge is
// finished (its component is complete): parent NONE, dropped from later rounds. Unfinished fragments
// at least halve per round, so all levels together hold <= 2n nodes. The largest key on the F-path
// between u and v equals the largest key met while walking both ends up the levels until they meet;
// one kernel does that walk for all m edges (k_vf_query).
//
// This translation unit shares no code with the solver (boruvka.hip / batch.hip): it includes
// common.h only and launches only its own kernels, so its verdict is independent evidence. It calls
// the public ghs_check_canonical first, so every index below is in range.
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <utility>

#include "common.h"

namespace ghs {
namespace verify {

constexpr int VF_BLOCK = 256;
constexpr int VF_PER_THREAD = 16;                                 // flag bytes per thread: one 16-B load
constexpr uint64_t VF_TILE = (uint64_t)VF_BLOCK * VF_PER_THREAD;  // flags per block of the compaction
constexpr uint32_t VF_MAX_LEVELS = 40;                            // n < 2^32 halves to 0 in 33
constexpr int VF_JUMP_HOPS = 8;

struct alignas(16) VNode {  // one fragment of one level
  uint64_t key;             // the key it chose this round (KEY_NONE: finished)
  uint32_t parent;          // dense id of its fragment at the next level (LABEL_NONE: finished)
  uint32_t pad;
};
struct alignas(16) VEdge {  // a live T-edge: its ends' fragments at the current level
  uint32_t a, b;
  uint64_t key;
};
struct VfLevels {
  uint64_t off[VF_MAX_LEVELS];  // first node of every level
};

// status block (uint64 slots, device)
enum { ST_SCAN = 0, ST_WEIGHT, ST_HOOKS, ST_LIVE, ST_UNSPANNED, ST_LIGHTER, ST_CYCLIC, ST_FIRST_BAD, ST_SLOTS };

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static inline unsigned grid_for(uint64_t items, unsigned per_block, unsigned cap = 2048) {
  uint64_t g = (items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

__device__ __forceinline__ uint64_t key_of(const u32x4 q, int lo) { return lo ? ((uint64_t)q.w << 32) | q.z : ((uint64_t)q.y << 32) | q.x; }

__device__ __forceinline__ u32x4 load16(const void *p) { return *reinterpret_cast<const u32x4 *>(p); }

__device__ __forceinline__ uint32_t block_sum(uint32_t c, uint32_t *s_w) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x / 64] = c;
  __syncthreads();
  uint32_t t = 0;
#pragma unroll
  for (int w = 0; w < VF_BLOCK / 64; ++w) t += s_w[w];
  __syncthreads();
  return t;
}

__global__ __launch_bounds__(VF_BLOCK) void k_vf_init_nodes(VNode *__restrict__ lvl, uint64_t cnt) {
  u32x4 none;
  none.x = none.y = none.z = 0xffffffffu;
  none.w = 0;
  for (uint64_t f = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; f < cnt; f += (uint64_t)gridDim.x * blockDim.x)
    *reinterpret_cast<u32x4 *>(lvl + f) = none;
}

// ---- flag compaction: nonzero flag bytes -> dense ranks, in order -------------------------------
// A tile is VF_TILE flags, 16 consecutive bytes per thread (one 16-byte load when the array is
// 16-byte aligned and the 16 bytes lie inside it). Pass 1 counts per tile, one block scans the tile
// counts, pass 2 hands every set flag its rank. Two users: the flagged edges of the input (rank ->
// a VEdge record) and the surviving roots of a round (rank -> the root's dense id at the next level).
__device__ __forceinline__ uint32_t flag_mask16(const uint8_t *__restrict__ flags, uint64_t i, uint64_t N, bool vec) {
  uint32_t mask = 0;
  if (i >= N) return 0;
  if (vec && i + VF_PER_THREAD <= N) {
    const u32x4 q = load16(flags + i);
    const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((wd[k] >> (8 * j)) & 0xffu) mask |= 1u << (4 * k + j);
  } else {
    for (int j = 0; j < VF_PER_THREAD; ++j)
      if (i + j < N && flags[i + j]) mask |= 1u << j;
  }
  return mask;
}

__global__ __launch_bounds__(VF_BLOCK) void k_vf_flag_count(const uint8_t *__restrict__ flags, uint64_t N, bool vec,
                                                            uint32_t *__restrict__ tile_cnt) {
  __shared__ uint32_t s_w[VF_BLOCK / 64];
  const uint64_t i = blockIdx.x * VF_TILE + (uint64_t)threadIdx.x * VF_PER_THREAD;
  const uint32_t t = block_sum((uint32_t)__popc(flag_mask16(flags, i, N, vec)), s_w);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = t;
}

// exclusive scan of the tile counts in place (one block of 1024), the total to *total
__global__ __launch_bounds__(1024) void k_vf_tile_scan(uint32_t *__restrict__ cnt, uint32_t ntiles,
                                                       uint64_t *__restrict__ total) {
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
}

// the rank of this thread's first set flag: tile offset + the block's exclusive prefix
__device__ __forceinline__ uint32_t flag_rank_base(uint32_t c, uint32_t tile_off, uint32_t *s_w) {
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
  for (int x = 0; x < VF_BLOCK / 64; ++x) before += x < wid ? s_w[x] : 0u;
  return tile_off + before + inc - c;
}

// flagged edge e at rank o -> edges[o] = {u[e], v[e], w[e] << 32 | e} (o < cap only: the host
// returns `overfull` without reading the records when more than cap edges are flagged), sum of w
__global__ __launch_bounds__(VF_BLOCK) void k_vf_write_edges(const uint8_t *__restrict__ flags, uint64_t m, bool vec,
                                                             const uint32_t *__restrict__ tile_off,
                                                             const uint32_t *__restrict__ u,
                                                             const uint32_t *__restrict__ v,
                                                             const uint32_t *__restrict__ w, VEdge *__restrict__ edges,
                                                             uint64_t cap, uint64_t *__restrict__ status) {
  __shared__ uint32_t s_w[VF_BLOCK / 64];
  __shared__ uint64_t s_sum[VF_BLOCK / 64];
  const uint64_t i = blockIdx.x * VF_TILE + (uint64_t)threadIdx.x * VF_PER_THREAD;
  uint32_t mask = flag_mask16(flags, i, m, vec);
  uint64_t o = flag_rank_base((uint32_t)__popc(mask), tile_off[blockIdx.x], s_w);
  uint64_t sum = 0;
  while (mask) {
    const int j = __ffs(mask) - 1;
    mask &= mask - 1;
    const uint64_t e = i + j;
    const uint32_t we = w[e];
    sum += we;
    if (o < cap) {
      u32x4 rec;
      rec.x = u[e];
      rec.y = v[e];
      rec.z = (uint32_t)e;
      rec.w = we;
      *reinterpret_cast<u32x4 *>(edges + o) = rec;
    }
    ++o;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x / 64] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t t = 0;
    for (int x = 0; x < VF_BLOCK / 64; ++x) t += s_sum[x];
    if (t) atomicAdd((unsigned long long *)(status + ST_WEIGHT), (unsigned long long)t);
  }
}

// surviving root f at rank o -> newid[f] = o
__global__ __launch_bounds__(VF_BLOCK) void k_vf_write_ids(const uint8_t *__restrict__ alive, uint64_t cnt,
                                                           const uint32_t *__restrict__ tile_off,
                                                           uint32_t *__restrict__ newid) {
  __shared__ uint32_t s_w[VF_BLOCK / 64];
  const uint64_t i = blockIdx.x * VF_TILE + (uint64_t)threadIdx.x * VF_PER_THREAD;
  uint32_t mask = flag_mask16(alive, i, cnt, true);
  uint32_t o = flag_rank_base((uint32_t)__popc(mask), tile_off[blockIdx.x], s_w);
  while (mask) {
    const int j = __ffs(mask) - 1;
    mask &= mask - 1;
    newid[i + j] = o++;
  }
}

// ---- one Boruvka round over T ---------------------------------------------------------------------
// every live T-edge is a candidate for both of its fragments: a read-checked 64-bit atomicMin into
// the node record (a stale read is never smaller than the slot, so a skipped atomic is always right)
__global__ __launch_bounds__(VF_BLOCK) void k_vf_minedge(const VEdge *__restrict__ edges, uint64_t live,
                                                         VNode *__restrict__ lvl) {
  for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < live; t += (uint64_t)gridDim.x * blockDim.x) {
    const u32x4 q = load16(edges + t);
    const uint64_t key = key_of(q, 1);
    unsigned long long *ka = reinterpret_cast<unsigned long long *>(&lvl[q.x].key);
    unsigned long long *kb = reinterpret_cast<unsigned long long *>(&lvl[q.y].key);
    if (*ka > key) atomicMin(ka, (unsigned long long)key);
    if (*kb > key) atomicMin(kb, (unsigned long long)key);
  }
}

// the edge that won a fragment's slot names the fragment at its other end (keys are distinct: one
// writer per slot)
__global__ __launch_bounds__(VF_BLOCK) void k_vf_winner(const VEdge *__restrict__ edges, uint64_t live,
                                                        const VNode *__restrict__ lvl, uint32_t *__restrict__ other) {
  for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < live; t += (uint64_t)gridDim.x * blockDim.x) {
    const u32x4 q = load16(edges + t);
    const uint64_t key = key_of(q, 1);
    if (lvl[q.x].key == key) other[q.x] = q.y;
    if (lvl[q.y].key == key) other[q.y] = q.x;
  }
}

// hook: a fragment without an edge is finished (its own root, not alive); a mutual pair — both chose
// the same key, hence the same edge — keeps the smaller id as the root; every other fragment hooks
// onto the fragment across its edge. alive[f] = 1 for the roots that go on to the next level.
__global__ __launch_bounds__(VF_BLOCK) void k_vf_hook(const VNode *__restrict__ lvl, uint64_t cnt,
                                                      const uint32_t *__restrict__ other, uint32_t *__restrict__ par,
                                                      uint8_t *__restrict__ alive, uint64_t *__restrict__ status) {
  __shared__ uint32_t s_w[VF_BLOCK / 64];
  uint32_t hooks = 0;
  for (uint64_t f = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; f < cnt; f += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t k = lvl[f].key;
    uint32_t p = (uint32_t)f;
    uint8_t root = 0;
    if (k != KEY_NONE) {
      const uint32_t o = other[f];
      root = (lvl[o].key == k && f < o) ? 1 : 0;
      if (!root) {
        p = o;
        ++hooks;
      }
    }
    par[f] = p;
    alive[f] = root;
  }
  const uint32_t t = block_sum(hooks, s_w);
  if (threadIdx.x == 0 && t) atomicAdd((unsigned long long *)(status + ST_HOOKS), (unsigned long long)t);
}

// pointer jump, in place: up to VF_JUMP_HOPS hops per launch. Every value a thread reads is an
// ancestor at least as far as the previous launch left it, so launch j reaches min(8^j, depth)
// levels up: ceil(log8 cnt) launches resolve a hook chain cnt long. No loop depends on the data
// beyond that bound.
__global__ __launch_bounds__(VF_BLOCK) void k_vf_jump(uint32_t *__restrict__ par, uint64_t cnt) {
  for (uint64_t f = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; f < cnt; f += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t p0 = par[f];
    uint32_t p = p0;
#pragma unroll 1
    for (int h = 0; h < VF_JUMP_HOPS; ++h) {
      const uint32_t g = par[p];
      if (g == p) break;
      p = g;
    }
    if (p != p0) par[f] = p;
  }
}

// the node's parent: the dense id its root got for the next level (finished fragments keep NONE)
__global__ __launch_bounds__(VF_BLOCK) void k_vf_setparent(VNode *__restrict__ lvl, uint64_t cnt,
                                                           const uint32_t *__restrict__ par,
                                                           const uint32_t *__restrict__ newid) {
  for (uint64_t f = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; f < cnt; f += (uint64_t)gridDim.x * blockDim.x)
    if (lvl[f].key != KEY_NONE) lvl[f].parent = newid[par[f]];
}

// the live list of the next round: ends renamed to the next level's ids, edges inside one fragment
// dropped. Order does not matter (minima and counts only), so survivors are appended with one
// atomic per block and iteration.
__global__ __launch_bounds__(VF_BLOCK) void k_vf_relabel(const VEdge *__restrict__ in, uint64_t live,
                                                         const VNode *__restrict__ lvl, VEdge *__restrict__ out,
                                                         uint64_t *__restrict__ count) {
  __shared__ uint32_t s_w[VF_BLOCK / 64];
  __shared__ uint64_t s_base;
  const int lane = threadIdx.x & 63, wid = threadIdx.x / 64;
  for (uint64_t base = blockIdx.x * (uint64_t)VF_BLOCK; base < live; base += (uint64_t)gridDim.x * VF_BLOCK) {
    const uint64_t t = base + threadIdx.x;
    bool keep = false;
    u32x4 q;
    q.x = q.y = q.z = q.w = 0;
    if (t < live) {
      q = load16(in + t);
      q.x = lvl[q.x].parent;
      q.y = lvl[q.y].parent;
      keep = q.x != q.y && q.x != LABEL_NONE && q.y != LABEL_NONE;
    }
    const uint64_t mask = __ballot(keep);
    if (lane == 0) s_w[wid] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t tot = 0;
      for (int x = 0; x < VF_BLOCK / 64; ++x) tot += s_w[x];
      s_base = tot ? atomicAdd((unsigned long long *)count, (unsigned long long)tot) : 0ull;
    }
    __syncthreads();
    if (keep) {
      uint32_t before = 0;
#pragma unroll
      for (int x = 0; x < VF_BLOCK / 64; ++x) before += x < wid ? s_w[x] : 0u;
      const uint64_t o = s_base + before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      *reinterpret_cast<u32x4 *>(out + o) = q;
    }
    __syncthreads();
  }
}

// ---- the query: every edge of G against the levels ------------------------------------------------
// 4 edges per lane (16-byte loads of u, v, w, one 4-byte load of the flags), walked in lock step: a
// step is one 16-byte node load per end, up to 8 in flight per lane. mx = the largest key met below
// the meeting point = the largest key on the F-path (King). An end that reaches a finished fragment
// before meeting the other lies in another component (tested BEFORE a == b: NONE == NONE is not a
// meeting). Verdict per edge: unspanned; unflagged and key < mx: lighter; flagged and key > mx: the
// flagged edge is not in F (cyclic). Counts are reduced per block before one atomic each.
struct QueryAcc {
  uint32_t uns, lig, cyc;
  uint64_t bad;
};

__device__ __forceinline__ void query4(uint32_t n, const uint32_t (&ua)[4], const uint32_t (&va)[4],
                                       const uint32_t (&wa)[4], uint32_t f4, uint64_t e0, uint32_t valid,
                                       const VNode *__restrict__ nodes, const VfLevels &lv, uint32_t nlev, QueryAcc &acc) {
  uint32_t a[4], b[4];
  uint64_t mx[4];
  uint32_t act = 0, uns = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    a[j] = ua[j];
    b[j] = va[j];
    mx[j] = 0;
    if ((valid >> j) & 1u) {
      // never index out of range, whatever the list (the host has checked it canonical)
      if (a[j] < n && b[j] < n && a[j] != b[j]) act |= 1u << j;
      else uns |= 1u << j;
    }
  }
  for (uint32_t r = 0; r < nlev && act; ++r) {
    const VNode *__restrict__ lvl = nodes + lv.off[r];
    u32x4 qa[4], qb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((act >> j) & 1u) {
        qa[j] = load16(lvl + a[j]);
        qb[j] = load16(lvl + b[j]);
      }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((act >> j) & 1u) {
        const uint64_t ka = key_of(qa[j], 0), kb = key_of(qb[j], 0);
        const uint64_t k = ka > kb ? ka : kb;
        if (k > mx[j]) mx[j] = k;
        const uint32_t pa = qa[j].z, pb = qb[j].z;
        if (pa == LABEL_NONE || pb == LABEL_NONE) {
          uns |= 1u << j;
          act &= ~(1u << j);
        } else if (pa == pb) {
          act &= ~(1u << j);
        } else {
          a[j] = pa;
          b[j] = pb;
        }
      }
  }
  uns |= act;  // ran out of levels without meeting
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!((valid >> j) & 1u)) continue;
    const uint64_t e = e0 + j;
    const uint64_t key = ((uint64_t)wa[j] << 32) | e;
    const bool flagged = ((f4 >> (8 * j)) & 0xffu) != 0;
    bool bad = true;
    if ((uns >> j) & 1u) ++acc.uns;
    else if (!flagged && key < mx[j]) ++acc.lig;
    else if (flagged && key > mx[j]) ++acc.cyc;
    else bad = false;
    if (bad && e < acc.bad) acc.bad = e;
  }
}

__global__ __launch_bounds__(VF_BLOCK) void k_vf_query(uint32_t n, uint64_t m, const uint32_t *__restrict__ u,
                                                       const uint32_t *__restrict__ v, const uint32_t *__restrict__ w,
                                                       const uint8_t *__restrict__ flags, bool fvec,
                                                       const VNode *__restrict__ nodes, const VfLevels lv, uint32_t nlev,
                                                       uint64_t *__restrict__ status) {
  __shared__ uint32_t s_c[3][VF_BLOCK / 64];
  __shared__ uint64_t s_bad[VF_BLOCK / 64];
  QueryAcc acc;
  acc.uns = acc.lig = acc.cyc = 0;
  acc.bad = ~0ull;
  const uint64_t gid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t nquads = (m + 3) / 4;
  for (uint64_t q = gid; q < nquads; q += stride) {
    const uint64_t e0 = 4 * q;
    uint32_t ua[4], va[4], wa[4], f4 = 0, valid = 0xf;
    if (e0 + 4 <= m) {
      const u32x4 x = load16(u + e0), y = load16(v + e0), z = load16(w + e0);
      ua[0] = x.x; ua[1] = x.y; ua[2] = x.z; ua[3] = x.w;
      va[0] = y.x; va[1] = y.y; va[2] = y.z; va[3] = y.w;
      wa[0] = z.x; wa[1] = z.y; wa[2] = z.z; wa[3] = z.w;
      if (fvec) {
        f4 = *reinterpret_cast<const uint32_t *>(flags + e0);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) f4 |= (uint32_t)flags[e0 + j] << (8 * j);
      }
    } else {  // the last, partial quad
      valid = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ua[j] = va[j] = wa[j] = 0;
        if (e0 + j < m) {
          valid |= 1u << j;
          ua[j] = u[e0 + j];
          va[j] = v[e0 + j];
          wa[j] = w[e0 + j];
          f4 |= (uint32_t)flags[e0 + j] << (8 * j);
        }
      }
    }
    query4(n, ua, va, wa, f4, e0, valid, nodes, lv, nlev, acc);
  }
  uint32_t c[3] = {acc.uns, acc.lig, acc.cyc};
  uint64_t bad = acc.bad;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] += __shfl_xor(c[k], d);
    const uint64_t o = __shfl_xor(bad, d);
    bad = o < bad ? o : bad;
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) s_c[k][threadIdx.x / 64] = c[k];
    s_bad[threadIdx.x / 64] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t t[3] = {0, 0, 0}, tb = ~0ull;
    for (int x = 0; x < VF_BLOCK / 64; ++x) {
      for (int k = 0; k < 3; ++k) t[k] += s_c[k][x];
      tb = s_bad[x] < tb ? s_bad[x] : tb;
    }
    if (t[0]) atomicAdd((unsigned long long *)(status + ST_UNSPANNED), (unsigned long long)t[0]);
    if (t[1]) atomicAdd((unsigned long long *)(status + ST_LIGHTER), (unsigned long long)t[1]);
    if (t[2]) atomicAdd((unsigned long long *)(status + ST_CYCLIC), (unsigned long long)t[2]);
    if (tb != ~0ull) atomicMin((unsigned long long *)(status + ST_FIRST_BAD), (unsigned long long)tb);
  }
}

// ---- workspace ------------------------------------------------------------------------------------
// nodes: 2n x 16 B (all levels); par, other / newid (one array: `other` is dead once the hook has
// run), alive: 9 B per vertex; two live-edge lists of min(m, n - 1) x 16 B; the tile counts of the
// larger compaction; the status block.
struct Layout {
  uint64_t cap;
  size_t nodes, par, other, alive, ea, eb, tiles, status, total;
};

static Layout layout(uint32_t n, uint64_t m) {
  Layout l;
  l.cap = n ? (m < (uint64_t)n - 1 ? m : (uint64_t)n - 1) : 0;
  const uint64_t big = m > n ? m : n;
  size_t o = 0;
  l.nodes = o; o += align256((size_t)2 * n * sizeof(VNode));
  l.par = o; o += align256((size_t)n * 4);
  l.other = o; o += align256((size_t)n * 4);
  l.alive = o; o += align256((size_t)n);
  l.ea = o; o += align256((size_t)l.cap * sizeof(VEdge));
  l.eb = o; o += align256((size_t)l.cap * sizeof(VEdge));
  l.tiles = o; o += align256((size_t)((big + VF_TILE - 1) / VF_TILE) * 4);
  l.status = o; o += 256;
  l.total = o;
  return l;
}

static int read_status(uint64_t *h, const uint64_t *d_status, hipStream_t st) {
  GHS_HIP_CHECK(hipMemcpyAsync(h, d_status, ST_SLOTS * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipStreamSynchronize(st));
  return GHS_OK;
}

}  // namespace verify
}  // namespace ghs

using namespace ghs;
using namespace ghs::verify;

extern "C" {

size_t ghs_verify_workspace_bytes(uint32_t n, uint64_t m) { return layout(n, m).total; }

int ghs_verify_msf_device(uint32_t n, uint64_t m, const uint32_t *d_u, const uint32_t *d_v, const uint32_t *d_w,
                          const uint8_t *d_in_mst, void *d_workspace, size_t workspace_bytes, void *stream,
                          ghs_verify_result_t *result) {
  hipStream_t st = (hipStream_t)stream;
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_verify_result_t{};
  result->first_bad_eid = ~0ull;
  if (m == 0) {
    result->ok = 1;
    result->components = n;
    return GHS_OK;
  }
  if (m >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "m must be < 2^31");
  if (!d_u || !d_v || !d_w || !d_in_mst || !d_workspace) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if (((uintptr_t)d_u | (uintptr_t)d_v | (uintptr_t)d_w | (uintptr_t)d_workspace) & 15)
    GHS_FAIL(GHS_E_ARG, "u, v, w and the workspace must be 16-byte aligned");
  const Layout l = layout(n, m);
  if (workspace_bytes < l.total) GHS_FAIL(GHS_E_NOMEM, "workspace too small");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");

  const auto t0 = std::chrono::steady_clock::now();
  int canon = 0;
  const int rc = ghs_check_canonical(n, m, d_u, d_v, stream, &canon);
  if (rc != GHS_OK) return rc;
  if (!canon) GHS_FAIL(GHS_E_NONCANON, "edge list is not canonical");

  char *base = (char *)d_workspace;
  VNode *nodes = (VNode *)(base + l.nodes);
  uint32_t *par = (uint32_t *)(base + l.par);
  uint32_t *other = (uint32_t *)(base + l.other);
  uint32_t *newid = other;
  uint8_t *alive = (uint8_t *)(base + l.alive);
  VEdge *cur = (VEdge *)(base + l.ea), *nxt = (VEdge *)(base + l.eb);
  uint32_t *tiles = (uint32_t *)(base + l.tiles);
  uint64_t *status = (uint64_t *)(base + l.status);
  uint64_t h[ST_SLOTS];

  // T: the flagged edges, counted, then written as records
  GHS_HIP_CHECK(hipMemsetAsync(status, 0, ST_SLOTS * sizeof(uint64_t), st));
  GHS_HIP_CHECK(hipMemsetAsync(status + ST_FIRST_BAD, 0xff, sizeof(uint64_t), st));
  const bool vec16 = ((uintptr_t)d_in_mst & 15) == 0, vec4 = ((uintptr_t)d_in_mst & 3) == 0;
  const uint64_t mtiles = (m + VF_TILE - 1) / VF_TILE;
  k_vf_flag_count<<<(unsigned)mtiles, VF_BLOCK, 0, st>>>(d_in_mst, m, vec16, tiles);
  k_vf_tile_scan<<<1, 1024, 0, st>>>(tiles, (uint32_t)mtiles, status + ST_SCAN);
  GHS_HIP_CHECK(hipGetLastError());
  if (int e = read_status(h, status, st)) return e;
  const uint64_t T = h[ST_SCAN];
  result->tree_edges = T;
  if (T > l.cap) {  // more than n - 1 flagged edges: a cycle for certain, nothing else is computed
    result->overfull = 1;
    result->cyclic_edges = T - ((uint64_t)n - 1);
    result->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GHS_OK;
  }
  k_vf_write_edges<<<(unsigned)mtiles, VF_BLOCK, 0, st>>>(d_in_mst, m, vec16, tiles, d_u, d_v, d_w, cur, l.cap, status);
  GHS_HIP_CHECK(hipGetLastError());

  // Boruvka over T, one level of nodes per round
  VfLevels lv;
  for (uint32_t i = 0; i < VF_MAX_LEVELS; ++i) lv.off[i] = 0;
  uint64_t off = 0, cnt = n, live = T, hooks = 0;
  uint32_t r = 0, rounds = 0;
  for (;;) {
    if (r >= VF_MAX_LEVELS) GHS_FAIL(GHS_E_ROUNDCAP, "verifier: round cap exceeded");
    if (off + cnt > (uint64_t)2 * n) GHS_FAIL(GHS_E_STATE, "verifier: level sizes exceed 2n nodes");
    lv.off[r] = off;
    VNode *lvl = nodes + off;
    k_vf_init_nodes<<<grid_for(cnt, VF_BLOCK), VF_BLOCK, 0, st>>>(lvl, cnt);
    ++r;
    if (live == 0) break;  // every remaining fragment is finished: this level is the last
    ++rounds;
    k_vf_minedge<<<grid_for(live, VF_BLOCK), VF_BLOCK, 0, st>>>(cur, live, lvl);
    k_vf_winner<<<grid_for(live, VF_BLOCK), VF_BLOCK, 0, st>>>(cur, live, lvl, other);
    k_vf_hook<<<grid_for(cnt, VF_BLOCK), VF_BLOCK, 0, st>>>(lvl, cnt, other, par, alive, status);
    for (uint64_t reach = 1; reach < cnt; reach *= VF_JUMP_HOPS)
      k_vf_jump<<<grid_for(cnt, VF_BLOCK), VF_BLOCK, 0, st>>>(par, cnt);
    const uint64_t ctiles = (cnt + VF_TILE - 1) / VF_TILE;
    k_vf_flag_count<<<(unsigned)ctiles, VF_BLOCK, 0, st>>>(alive, cnt, true, tiles);
    k_vf_tile_scan<<<1, 1024, 0, st>>>(tiles, (uint32_t)ctiles, status + ST_SCAN);
    k_vf_write_ids<<<(unsigned)ctiles, VF_BLOCK, 0, st>>>(alive, cnt, tiles, newid);
    k_vf_setparent<<<grid_for(cnt, VF_BLOCK), VF_BLOCK, 0, st>>>(lvl, cnt, par, newid);
    GHS_HIP_CHECK(hipMemsetAsync(status + ST_LIVE, 0, sizeof(uint64_t), st));
    k_vf_relabel<<<grid_for(live, VF_BLOCK), VF_BLOCK, 0, st>>>(cur, live, lvl, nxt, status + ST_LIVE);
    GHS_HIP_CHECK(hipGetLastError());
    if (int e = read_status(h, status, st)) return e;
    if (h[ST_SCAN] > cnt / 2 || h[ST_LIVE] > live) GHS_FAIL(GHS_E_STATE, "verifier: a round did not contract");
    off += cnt;
    cnt = h[ST_SCAN];
    hooks = h[ST_HOOKS];
    live = h[ST_LIVE];
    std::swap(cur, nxt);
    if (cnt == 0) break;
  }
  GHS_HIP_CHECK(hipGetLastError());

  const unsigned qgrid = grid_for((m + 3) / 4, VF_BLOCK);
  k_vf_query<<<qgrid, VF_BLOCK, 0, st>>>(n, m, d_u, d_v, d_w, d_in_mst, vec4, nodes, lv, r, status);
  GHS_HIP_CHECK(hipGetLastError());
  if (int e = read_status(h, status, st)) return e;
  if (hooks > T || h[ST_CYCLIC] != T - hooks)
    GHS_FAIL(GHS_E_STATE, "verifier: the query's cyclic count disagrees with the rounds' hook count");

  result->rounds = rounds;
  result->components = (uint64_t)n - hooks;
  result->total_weight = h[ST_WEIGHT];
  result->cyclic_edges = T - hooks;
  result->unspanned_edges = h[ST_UNSPANNED];
  result->lighter_edges = h[ST_LIGHTER];
  result->first_bad_eid = h[ST_FIRST_BAD];
  result->ok = (result->cyclic_edges | result->unspanned_edges | result->lighter_edges) == 0 ? 1u : 0u;
  result->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return GHS_OK;
}

}  // extern "C"
