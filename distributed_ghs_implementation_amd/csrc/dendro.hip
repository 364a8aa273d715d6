// Single-linkage dendrogram (ABI 10 addition, ghs_forest_dendro_device): the Kruskal merge tree of the
// flagged forest T. Merge j is the j-th lightest edge of T under (w, eid); vertex v is node v, merge j
// is node n + j. Forests here are tens of thousands of edges deep and a dendrogram is as high as a
// path is long, so no pass is level-synchronous in the depth of either.
//
// Pipeline (everything on `stream`):
//   1. count the flags per 4096-flag tile, scan, gather the keys w << eb | eid (eb = bits of m) of the
//      flagged edges; a rocPRIM radix sort ranks them: from here an edge is its rank r in [0, t), and
//      positions in every later edge list are in rank order;
//   2. contraction levels (down): on nv supervertices and ne edges (a, b) in rank order
//        mn[x]  = the lightest incident edge (atomicMin of positions; level 0: leaf_parent);
//        an edge is chosen when it is mn of an end, alpha otherwise;
//        x points to the other end of mn[x]; the mutual pair (both ends chose the same edge) is broken
//        at its smaller id; pointer doubling finds every group's root;
//        one scan numbers the groups (all of them: sort ids; those with an alpha edge: the next
//        level's supervertices), one scan numbers the alpha edges; alpha edges go to the next level as
//        (S(a), S(b)) with their position here (back); chosen edges keep their group's two ids.
//      A forest halves its edges every level (ne' <= ne / 2); an alpha edge inside one group, or a
//      level that does not halve, is a cycle: is_forest = 0.
//   3. expansion (up), deepest level first: the level below has given D_alpha, a parent for every
//      group (mn') and every alpha edge (par'). A chosen edge e of group S hangs under b(e), the
//      highest node among S and its D_alpha ancestors that is lighter than e: a predecessor search by
//      binary lifting over par' (tables built by doubling until a table is empty). A stable pairs sort
//      by b puts the chosen edges of one b in rank order: a chain, each one's parent the next, the
//      last one's parent b's D_alpha parent, and b (an alpha edge) re-parented to the chain's head.
//   4. children by atomicMin / atomicMax of the node ids into the parent's two slots; cluster sizes
//      and the height by doubling up the finished parents: in round k a node adds its partial sum to
//      its 2^k-th ancestor (integer atomicAdd: exact in any order) and its hop count doubles.
//
// This translation unit includes common.h only and launches only its own kernels; it calls the
// public ghs_check_canonical first, so every index below is in range.
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <utility>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "common.h"

namespace ghs {
namespace dendro {

constexpr int DG_BLOCK = 256;
constexpr int DG_FLAGS_PER_THREAD = 16;                                      // one 16-byte load
constexpr uint64_t DG_FLAG_TILE = (uint64_t)DG_BLOCK * DG_FLAGS_PER_THREAD;  // flags per block
constexpr uint32_t DG_NONE = 0xffffffffu;
constexpr int DG_MAX_LEVELS = 32;

// status block (uint32 slots, device), then DG_FLAG_SLOTS round flags. Few slots on purpose: a deep
// forest needs more rounds than that, so their reuse is on the path every test of such a forest takes.
enum { ST_FLAGGED = 0, ST_CYC, ST_MAXD, ST_SLOTS };
constexpr uint32_t DG_FLAG_SLOTS = 16;

struct alignas(8) Up {  // 8 bytes: a merge's 2^k-th ancestor and the hops to its highest ancestor found so far
  uint32_t anc, hop;
};

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static inline unsigned grid_for(uint64_t items, unsigned per_block = DG_BLOCK, unsigned cap = 2048) {
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

#define DG_FOR(i, N) \
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < (N); i += (uint64_t)gridDim.x * blockDim.x)

// exclusive prefix of x over the block's 256 threads; *total: the sum
__device__ __forceinline__ uint32_t block_excl(uint32_t x, uint32_t *s_v, uint32_t *total) {
  s_v[threadIdx.x] = x;
  __syncthreads();
#pragma unroll
  for (int d = 1; d < DG_BLOCK; d <<= 1) {
    const uint32_t o = threadIdx.x >= (unsigned)d ? s_v[threadIdx.x - d] : 0u;
    __syncthreads();
    s_v[threadIdx.x] = o + s_v[threadIdx.x];
    __syncthreads();
  }
  const uint32_t inc = s_v[threadIdx.x];
  *total = s_v[DG_BLOCK - 1];
  __syncthreads();
  return inc - x;
}

// ---- step 1: the flagged edges, counted and gathered --------------------------------------------------
// The flags may start at any byte. They are read in the 16-byte-aligned frame that contains them:
// frame byte p holds the flag of edge p - lo for p in [lo, hi), lo = the pointer's low 4 bits. A
// thread owns 16 frame bytes: one 16-byte load when all of them are flags (always aligned), byte
// loads with a bound check at the head and the tail. Nothing outside [lo, hi) is read.
__device__ __forceinline__ uint32_t flag_mask16(uintptr_t frame, uint64_t p, uint64_t lo, uint64_t hi) {
  uint32_t mask = 0;
  if (p >= hi || p + DG_FLAGS_PER_THREAD <= lo) return 0;
  if (p >= lo && p + DG_FLAGS_PER_THREAD <= hi) {
    const u32x4 q = *reinterpret_cast<const u32x4 *>(frame + p);
    const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((wd[k] >> (8 * j)) & 0xffu) mask |= 1u << (4 * k + j);
  } else {
    for (int j = 0; j < DG_FLAGS_PER_THREAD; ++j)
      if (p + j >= lo && p + j < hi && *reinterpret_cast<const uint8_t *>(frame + p + j)) mask |= 1u << j;
  }
  return mask;
}

__global__ __launch_bounds__(DG_BLOCK) void k_dg_flag_count(uintptr_t frame, uint64_t lo, uint64_t hi,
                                                            uint32_t *__restrict__ tile_cnt) {
  __shared__ uint32_t s_v[DG_BLOCK];
  const uint64_t p = blockIdx.x * DG_FLAG_TILE + (uint64_t)threadIdx.x * DG_FLAGS_PER_THREAD;
  uint32_t tot;
  (void)block_excl((uint32_t)__popc(flag_mask16(frame, p, lo, hi)), s_v, &tot);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
}

// exclusive scan of the tile counts in place (one block of 1024), the total to *total
__global__ __launch_bounds__(1024) void k_dg_tile_scan(uint32_t *__restrict__ cnt, uint32_t ntiles,
                                                       uint32_t *__restrict__ total) {
  __shared__ uint32_t s_part[1024];
  const uint32_t per = (ntiles + 1023) / 1024;
  const uint64_t b = (uint64_t)threadIdx.x * per;
  uint32_t sum = 0;
  for (uint32_t i = 0; i < per && b + i < ntiles; ++i) sum += cnt[b + i];
  s_part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const uint32_t o = threadIdx.x >= (unsigned)d ? s_part[threadIdx.x - d] : 0u;
    __syncthreads();
    s_part[threadIdx.x] = o + s_part[threadIdx.x];
    __syncthreads();
  }
  uint32_t run = threadIdx.x ? s_part[threadIdx.x - 1] : 0u;
  for (uint32_t i = 0; i < per && b + i < ntiles; ++i) {
    const uint32_t c = cnt[b + i];
    cnt[b + i] = run;
    run += c;
  }
  if (threadIdx.x == 1023) *total = s_part[1023];
}

// flagged edge e -> key w[e] << eb | e at its place in eid order
__global__ __launch_bounds__(DG_BLOCK) void k_dg_gather_keys(uintptr_t frame, uint64_t lo, uint64_t hi,
                                                             const uint32_t *__restrict__ w,
                                                             const uint32_t *__restrict__ tile_off, uint32_t eb,
                                                             uint64_t *__restrict__ keys, uint64_t cap) {
  __shared__ uint32_t s_v[DG_BLOCK];
  const uint64_t p = blockIdx.x * DG_FLAG_TILE + (uint64_t)threadIdx.x * DG_FLAGS_PER_THREAD;
  uint32_t mask = flag_mask16(frame, p, lo, hi);
  uint32_t tot;
  uint64_t o = (uint64_t)tile_off[blockIdx.x] + block_excl((uint32_t)__popc(mask), s_v, &tot);
  while (mask) {
    const int j = __ffs(mask) - 1;
    mask &= mask - 1;
    const uint64_t e = p + j - lo;
    if (o < cap) keys[o] = ((uint64_t)w[e] << eb) | e;  // the host has checked the count against cap already
    ++o;
  }
}

// rank r -> its edge id and its two ends (level 0's edge list)
__global__ __launch_bounds__(DG_BLOCK) void k_dg_unpack(uint32_t t, const uint64_t *__restrict__ keys, uint32_t eb,
                                                        uint64_t m, const uint32_t *__restrict__ u,
                                                        const uint32_t *__restrict__ v, uint32_t *__restrict__ merge_eid,
                                                        uint32_t *__restrict__ ea, uint32_t *__restrict__ eb_out) {
  DG_FOR(r, t) {
    uint64_t e = keys[r] & (((uint64_t)1 << eb) - 1);
    if (e >= m) e = 0;  // never: the keys were built from ids < m
    merge_eid[r] = (uint32_t)e;
    ea[r] = u[e];
    eb_out[r] = v[e];
  }
}

// ---- step 2: a contraction level -------------------------------------------------------------------------
__global__ __launch_bounds__(DG_BLOCK) void k_dg_minedge(uint32_t ne, const uint32_t *__restrict__ ea,
                                                         const uint32_t *__restrict__ eb, uint32_t nv,
                                                         uint32_t *__restrict__ mn) {
  DG_FOR(i, ne) {
    const uint32_t a = ea[i], b = eb[i];
    if (a < nv && mn[a] > (uint32_t)i) atomicMin(&mn[a], (uint32_t)i);
    if (b < nv && mn[b] > (uint32_t)i) atomicMin(&mn[b], (uint32_t)i);
  }
}

// x -> the other end of its lightest edge; itself when it has none or is the smaller end of the
// mutual pair (both ends chose the same edge)
__global__ __launch_bounds__(DG_BLOCK) void k_dg_point(uint32_t nv, uint32_t ne, const uint32_t *__restrict__ mn,
                                                       const uint32_t *__restrict__ ea, const uint32_t *__restrict__ eb,
                                                       uint32_t *__restrict__ ptr, uint32_t *__restrict__ hasa) {
  DG_FOR(x, nv) {
    const uint32_t i = mn[x];
    uint32_t p = (uint32_t)x;
    if (i < ne) {
      const uint32_t a = ea[i], b = eb[i];
      const uint32_t y = a == (uint32_t)x ? b : a;
      if (y < nv && !(mn[y] == i && (uint32_t)x < y)) p = y;
    }
    ptr[x] = p;
    hasa[x] = 0;
  }
}

__global__ __launch_bounds__(DG_BLOCK) void k_dg_jump(uint32_t nv, const uint32_t *__restrict__ in,
                                                      uint32_t *__restrict__ out, uint32_t *__restrict__ chg) {
  bool any = false;
  DG_FOR(x, nv) {
    const uint32_t p = in[x];
    const uint32_t q = in[p];
    out[x] = q;
    any |= q != p;
  }
  if (any) *chg = 1;
}

// alpha edges: not the lightest edge of either end. aflag has ne + 1 entries (the last one 0: the
// scan's total lands there); a group with an alpha edge lives on in the next level.
__global__ __launch_bounds__(DG_BLOCK) void k_dg_mark_alpha(uint32_t ne, const uint32_t *__restrict__ ea,
                                                            const uint32_t *__restrict__ eb,
                                                            const uint32_t *__restrict__ mn,
                                                            const uint32_t *__restrict__ ptr,
                                                            uint32_t *__restrict__ aflag, uint32_t *__restrict__ hasa) {
  DG_FOR(i, (uint64_t)ne + 1) {
    uint32_t alpha = 0;
    if (i < ne) {
      const uint32_t a = ea[i], b = eb[i];
      alpha = (mn[a] != (uint32_t)i && mn[b] != (uint32_t)i) ? 1u : 0u;
      if (alpha) {
        hasa[ptr[a]] = 1;
        hasa[ptr[b]] = 1;
      }
    }
    aflag[i] = alpha;
  }
}

// a group's root with at least one edge: 1 << 32 | (has an alpha edge); gval has nv + 1 entries
__global__ __launch_bounds__(DG_BLOCK) void k_dg_group_vals(uint32_t nv, const uint32_t *__restrict__ mn,
                                                            const uint32_t *__restrict__ ptr,
                                                            const uint32_t *__restrict__ hasa,
                                                            uint64_t *__restrict__ gval) {
  DG_FOR(x, (uint64_t)nv + 1) {
    uint64_t g = 0;
    if (x < nv && ptr[x] == (uint32_t)x && mn[x] != DG_NONE) g = ((uint64_t)1 << 32) | (hasa[x] ? 1u : 0u);
    gval[x] = g;
  }
}

// alpha edge i at alpha position j -> the next level's edge j; chosen edge i at chosen position q ->
// clist[q] = i, cg[q] = its group's sort id, cs[q] = its group's id in the next level (or none)
__global__ __launch_bounds__(DG_BLOCK) void k_dg_split(uint32_t ne, const uint32_t *__restrict__ ea,
                                                       const uint32_t *__restrict__ eb, const uint32_t *__restrict__ ptr,
                                                       const uint32_t *__restrict__ hasa,
                                                       const uint32_t *__restrict__ aflag,
                                                       const uint32_t *__restrict__ apre,
                                                       const uint64_t *__restrict__ gpre, uint32_t ne2,
                                                       uint32_t *__restrict__ ea2, uint32_t *__restrict__ eb2,
                                                       uint32_t *__restrict__ back2, uint32_t *__restrict__ clist,
                                                       uint32_t *__restrict__ cg, uint32_t *__restrict__ cs,
                                                       uint32_t *__restrict__ cyc) {
  bool loop = false;
  DG_FOR(i, ne) {
    const uint32_t ra = ptr[ea[i]], rb = ptr[eb[i]];
    const uint32_t j = apre[i];
    if (aflag[i]) {
      loop |= ra == rb;
      if (j < ne2) {
        ea2[j] = (uint32_t)gpre[ra];
        eb2[j] = (uint32_t)gpre[rb];
        back2[j] = (uint32_t)i;
      }
    } else {
      const uint32_t q = (uint32_t)i - j;
      const uint64_t g = gpre[ra];
      clist[q] = (uint32_t)i;
      cg[q] = (uint32_t)(g >> 32);
      cs[q] = hasa[ra] ? (uint32_t)g : DG_NONE;
    }
  }
  if (loop) *cyc = 1;
}

// ---- step 3: expansion ---------------------------------------------------------------------------------------
// the lifting tables: up[0] = par', up[k + 1][j] = up[k][up[k][j]]; *chg: the table written has an entry
__global__ __launch_bounds__(DG_BLOCK) void k_dg_lift_first(uint32_t ne2, const uint32_t *__restrict__ par2,
                                                            uint32_t *__restrict__ up0, uint32_t *__restrict__ chg) {
  bool any = false;
  DG_FOR(j, ne2) {
    uint32_t p = par2[j];
    if (p >= ne2) p = DG_NONE;
    up0[j] = p;
    any |= p != DG_NONE;
  }
  if (any) *chg = 1;
}

__global__ __launch_bounds__(DG_BLOCK) void k_dg_lift_next(uint32_t ne2, const uint32_t *__restrict__ in,
                                                           uint32_t *__restrict__ out, uint32_t *__restrict__ chg) {
  bool any = false;
  DG_FOR(j, ne2) {
    const uint32_t p = in[j];
    const uint32_t q = p == DG_NONE ? DG_NONE : in[p];
    out[j] = q;
    any |= q != DG_NONE;
  }
  if (any) *chg = 1;
}

// an alpha edge keeps its D_alpha parent unless a chain is hung above it (k_dg_chain, later)
__global__ __launch_bounds__(DG_BLOCK) void k_dg_alpha_par(uint32_t ne2, const uint32_t *__restrict__ par2,
                                                           const uint32_t *__restrict__ back2, uint32_t ne,
                                                           uint32_t *__restrict__ par) {
  DG_FOR(j, ne2) {
    const uint32_t p = par2[j], i = back2[j];
    if (i < ne) par[i] = p < ne2 ? back2[p] : DG_NONE;
  }
}

// b(e) of every chosen edge: its group's leaf, or the highest D_alpha ancestor lighter than e.
// Positions are in rank order on both levels: the alpha edges lighter than the chosen edge at position i
// (the q-th chosen one) are exactly the i - q alpha edges in front of it, so a D_alpha node is lighter
// than e iff its position in the level below is < i - q. One dependent load per table.
__global__ __launch_bounds__(DG_BLOCK) void k_dg_lift(uint32_t nc, const uint32_t *__restrict__ clist,
                                                      const uint32_t *__restrict__ cg, const uint32_t *__restrict__ cs,
                                                      uint32_t nv2, const uint32_t *__restrict__ mn2, uint32_t ne2,
                                                      const uint32_t *__restrict__ up, int tables, uint32_t ngroups,
                                                      uint32_t *__restrict__ kb) {
  DG_FOR(q, nc) {
    const uint32_t i = clist[q], s = cs[q];
    const uint32_t c = s < nv2 ? mn2[s] : DG_NONE;
    uint32_t thr = i - (uint32_t)q;
    if (thr > ne2) thr = ne2;
    uint32_t b = cg[q];
    if (c < thr) {
      uint32_t cur = c;
      for (int k = tables - 1; k >= 0; --k) {
        const uint32_t nx = up[(size_t)k * ne2 + cur];
        if (nx < thr) cur = nx;
      }
      b = ngroups + cur;
    }
    kb[q] = b;
  }
}

// the chosen edges sorted by b (stable: rank order within one b): each one's parent is the next, the
// last one's parent is b's D_alpha parent, and an alpha b is re-parented to the head of its chain
__global__ __launch_bounds__(DG_BLOCK) void k_dg_chain(uint32_t nc, const uint32_t *__restrict__ kbs,
                                                       const uint32_t *__restrict__ perm,
                                                       const uint32_t *__restrict__ clist,
                                                       const uint32_t *__restrict__ cs, uint32_t nv2,
                                                       const uint32_t *__restrict__ mn2, uint32_t ne2,
                                                       const uint32_t *__restrict__ par2,
                                                       const uint32_t *__restrict__ back2, uint32_t ngroups, uint32_t ne,
                                                       uint32_t *__restrict__ par) {
  DG_FOR(k, nc) {
    const uint32_t b = kbs[k];
    uint32_t q = perm[k];
    if (q >= nc) q = 0;  // never: perm is a permutation of [0, nc)
    const uint32_t i = clist[q];
    if (i >= ne) continue;  // never
    uint32_t p = DG_NONE;
    if (k + 1 < nc && kbs[k + 1] == b) {
      const uint32_t q1 = perm[k + 1];
      p = q1 < nc ? clist[q1] : DG_NONE;
    } else if (b < ngroups) {
      const uint32_t s = cs[q];
      const uint32_t c = s < nv2 ? mn2[s] : DG_NONE;
      p = c < ne2 ? back2[c] : DG_NONE;
    } else if (b - ngroups < ne2) {
      const uint32_t c = par2[b - ngroups];
      p = c < ne2 ? back2[c] : DG_NONE;
    }
    par[i] = p;
    if (b >= ngroups && b - ngroups < ne2 && (k == 0 || kbs[k - 1] != b)) {
      const uint32_t ia = back2[b - ngroups];
      if (ia < ne) par[ia] = i;
    }
  }
}

// ---- step 4: children, sizes, height -----------------------------------------------------------------------
__global__ __launch_bounds__(DG_BLOCK) void k_dg_leaf_children(uint32_t n, uint32_t t, const uint32_t *__restrict__ leaf_parent,
                                                               uint32_t *__restrict__ child_a, uint32_t *__restrict__ child_b,
                                                               uint32_t *__restrict__ acc) {
  DG_FOR(x, n) {
    const uint32_t p = leaf_parent[x];
    if (p >= t) continue;
    if (child_a) atomicMin(&child_a[p], (uint32_t)x);
    if (child_b) atomicMax(&child_b[p], (uint32_t)x);
    if (acc) atomicAdd(&acc[p], 1u);
  }
}

// up[j] = (the parent, 1 hop when there is one); *chg: some merge has a parent
__global__ __launch_bounds__(DG_BLOCK) void k_dg_merge_children(uint32_t n, uint32_t t, const uint32_t *__restrict__ par,
                                                                uint32_t *__restrict__ child_a,
                                                                uint32_t *__restrict__ child_b, Up *__restrict__ up,
                                                                uint32_t *__restrict__ chg) {
  bool any = false;
  DG_FOR(j, t) {
    uint32_t p = par[j];
    if (p >= t) p = DG_NONE;
    up[j] = Up{p, p != DG_NONE ? 1u : 0u};
    if (p != DG_NONE) {
      any = true;
      if (child_a) atomicMin(&child_a[p], n + (uint32_t)j);
      if (child_b) atomicMax(&child_b[p], n + (uint32_t)j);
    }
  }
  if (any) *chg = 1;
}

// acc_out holds a copy of acc_in: add every node's partial sum (its descendants less than 2^k merges
// below) to its 2^k-th ancestor, double the hop count and the pointer
// (acc may be NULL: the hops alone, for the height)
__global__ __launch_bounds__(DG_BLOCK) void k_dg_size_round(uint32_t t, const Up *__restrict__ up_in,
                                                            Up *__restrict__ up_out,
                                                            const uint32_t *__restrict__ acc_in,
                                                            uint32_t *__restrict__ acc_out, uint32_t *__restrict__ chg) {
  bool any = false;
  DG_FOR(j, t) {
    Up me = up_in[j];
    if (me.anc < t) {
      if (acc_out) atomicAdd(&acc_out[me.anc], acc_in[j]);
      const Up o = up_in[me.anc];  // one 8-byte gather: the ancestor's pointer and its hops
      me.hop += o.hop;
      me.anc = o.anc < t ? o.anc : DG_NONE;
    } else {
      me.anc = DG_NONE;
    }
    up_out[j] = me;
    any |= me.anc != DG_NONE;
  }
  if (any) *chg = 1;
}

__global__ __launch_bounds__(DG_BLOCK) void k_dg_max_hop(uint32_t t, const Up *__restrict__ up,
                                                         uint32_t *__restrict__ maxd) {
  __shared__ uint32_t s_w[DG_BLOCK / 64];
  uint32_t deepest = 0;
  DG_FOR(j, t) deepest = up[j].hop > deepest ? up[j].hop : deepest;
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) {
    const uint32_t o = __shfl_xor(deepest, k);
    deepest = o > deepest ? o : deepest;
  }
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x / 64] = deepest;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < DG_BLOCK / 64; ++w) deepest = s_w[w] > deepest ? s_w[w] : deepest;
    if (deepest) atomicMax(maxd, deepest);
  }
}

// ---- workspace ------------------------------------------------------------------------------------------
// C = min(m, n - 1) possible merges. Level l holds at most C >> l edges and, for l >= 1, twice as many
// supervertices, so everything kept per level sums to a constant per possible merge:
//   kept, per possible merge: level 0 20 B (the two ends, chosen list, two group ids), levels >= 1
//     together at most 36 B (the same + back, par and mn of 2 supervertices each);
//   scratch, the largest of four phases that follow one another:
//     the key sort        16 B per possible merge + 4 B per 4096 edges of m (tile counts),
//     a level             28 B per vertex (two pointer buffers 8, alpha mark 4, scan in / out 16)
//                         + 8 B per possible merge (alpha flags, their scan),
//     an expansion        2 (ceil(log2(C / 2)) + 2) B per possible merge (the lifting tables:
//                         4 B x C / 2 entries each) + 12 B (b, sorted b, permutation),
//     sizes and height    20 B per possible merge (two buffers of (ancestor, hops), one of sums: the
//                         other one is d_size);
//   rocPRIM's sort / scan storage, 1 KiB of status.
struct Layout {
  uint64_t cap;
  int levels;                     // levels that can hold an edge
  uint64_t E[DG_MAX_LEVELS + 1];  // edge capacity per level
  size_t ea[DG_MAX_LEVELS + 1], eb[DG_MAX_LEVELS + 1], clist[DG_MAX_LEVELS + 1], cg[DG_MAX_LEVELS + 1],
      cs[DG_MAX_LEVELS + 1], back[DG_MAX_LEVELS + 1], par[DG_MAX_LEVELS + 1], mn[DG_MAX_LEVELS + 1];
  size_t scratch, scratch_bytes, prim, prim_bytes, status, total;
  // offsets within the scratch, per phase
  size_t a_keys, a_keys2, a_tiles;
  size_t d_ptra, d_ptrb, d_hasa, d_gval, d_gpre, d_aflag, d_apre;
  size_t u_up, u_kb, u_kbs, u_perm;
  size_t f_upa, f_upb, f_acca;
  uint32_t tables;  // lifting tables the scratch holds
};

static inline uint64_t flag_tiles(uint64_t m) { return (m + 15 + DG_FLAG_TILE - 1) / DG_FLAG_TILE; }  // any of 16 starts

static inline unsigned key_end_bit(uint64_t m) { return 32u + (m > 1 ? ceil_log2(m) : 1u); }
static inline unsigned b_bits(uint64_t ids) { return ids > 2 ? ceil_log2(ids) : 1u; }

static size_t sort_keys_bytes(uint64_t T, uint64_t m) {
  size_t b = 0;
  if (T == 0) return 0;
  (void)rocprim::radix_sort_keys(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)T, 0u, key_end_bit(m));
  return b;
}
static size_t sort_pairs_bytes(uint64_t T, unsigned bits) {
  size_t b = 0;
  if (T == 0) return 0;
  (void)rocprim::radix_sort_pairs(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                  rocprim::counting_iterator<uint32_t>(0), (uint32_t *)nullptr, (size_t)T, 0u, bits);
  return b;
}
template <typename V>
static size_t scan_bytes(uint64_t N) {
  size_t b = 0;
  if (N == 0) return 0;
  (void)rocprim::exclusive_scan(nullptr, b, (const V *)nullptr, (V *)nullptr, (V)0, (size_t)N, rocprim::plus<V>());
  return b;
}

static Layout layout(uint32_t n, uint64_t m) {
  Layout l{};
  l.cap = n ? (m < (uint64_t)n - 1 ? m : (uint64_t)n - 1) : 0;
  const uint64_t C = l.cap;
  size_t o = 0;
  int lv = 0;
  for (; lv < DG_MAX_LEVELS && (C >> lv) > 0; ++lv) {
    const uint64_t E = C >> lv;
    l.E[lv] = E;
    l.ea[lv] = o; o += align256((size_t)E * 4);
    l.eb[lv] = o; o += align256((size_t)E * 4);
    l.clist[lv] = o; o += align256((size_t)E * 4);
    l.cg[lv] = o; o += align256((size_t)E * 4);
    l.cs[lv] = o; o += align256((size_t)E * 4);
    if (lv) {
      l.back[lv] = o; o += align256((size_t)E * 4);
      l.par[lv] = o; o += align256((size_t)E * 4);
      l.mn[lv] = o; o += align256((size_t)E * 8);
    }
  }
  l.levels = lv;
  l.E[lv] = 0;
  // scratch phases
  size_t s = 0;
  l.a_keys = s; s += align256((size_t)C * 8);
  l.a_keys2 = s; s += align256((size_t)C * 8);
  l.a_tiles = s; s += align256((size_t)flag_tiles(m) * 4);
  size_t big = s;
  s = 0;
  l.d_ptra = s; s += align256((size_t)n * 4);
  l.d_ptrb = s; s += align256((size_t)n * 4);
  l.d_hasa = s; s += align256((size_t)n * 4);
  l.d_gval = s; s += align256(((size_t)n + 1) * 8);
  l.d_gpre = s; s += align256(((size_t)n + 1) * 8);
  l.d_aflag = s; s += align256(((size_t)C + 1) * 4);
  l.d_apre = s; s += align256(((size_t)C + 1) * 4);
  if (s > big) big = s;
  const uint64_t E1 = C / 2;
  l.tables = E1 ? ceil_log2(E1) + 2 : 0;
  s = 0;
  l.u_up = s; s += align256((size_t)l.tables * E1 * 4);
  l.u_kb = s; s += align256((size_t)C * 4);
  l.u_kbs = s; s += align256((size_t)C * 4);
  l.u_perm = s; s += align256((size_t)C * 4);
  if (s > big) big = s;
  s = 0;
  l.f_upa = s; s += align256((size_t)C * 8);
  l.f_upb = s; s += align256((size_t)C * 8);
  l.f_acca = s; s += align256((size_t)C * 4);
  if (s > big) big = s;
  l.scratch = o;
  l.scratch_bytes = big;
  o += big;
  size_t pb = sort_keys_bytes(C, m);
  const size_t p2 = sort_pairs_bytes(C, 32), p3 = scan_bytes<uint64_t>((uint64_t)n + 1), p4 = scan_bytes<uint32_t>(C + 1);
  pb = p2 > pb ? p2 : pb;
  pb = p3 > pb ? p3 : pb;
  pb = p4 > pb ? p4 : pb;
  l.prim_bytes = align256(pb) + (C ? 65536 : 0);
  l.prim = o; o += l.prim_bytes;
  l.status = o; o += 1024;
  l.total = o;
  return l;
}

static int read_u32(uint32_t *h, const uint32_t *d, hipStream_t st) {
  GHS_HIP_CHECK(hipMemcpyAsync(h, d, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipStreamSynchronize(st));
  return GHS_OK;
}

// One round flag per launch out of the status block (cleared with it at the start): one memset per
// DG_FLAG_SLOTS rounds, not one per round. When the slots run out they are cleared again: every earlier
// flag has been read by then, and the memset is ordered behind the kernels that wrote them.
struct Flags {
  uint32_t *base;
  uint32_t used;
};
static int next_flag(Flags &f, hipStream_t st, uint32_t **out) {
  if (f.used == DG_FLAG_SLOTS) {
    GHS_HIP_CHECK(hipMemsetAsync(f.base, 0, DG_FLAG_SLOTS * sizeof(uint32_t), st));
    f.used = 0;
  }
  *out = f.base + f.used++;
  return GHS_OK;
}

static inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

struct LevelInfo {
  uint32_t nv, ne, ne2, nv2, ngroups;
};

}  // namespace dendro
}  // namespace ghs

using namespace ghs;
using namespace ghs::dendro;

extern "C" {

size_t ghs_forest_dendro_workspace_bytes(uint32_t n, uint64_t m) { return layout(n, m).total; }

int ghs_forest_dendro_device(uint32_t n, uint64_t m, const uint32_t *d_u, const uint32_t *d_v, const uint32_t *d_w,
                             const uint8_t *d_in_mst, uint32_t *d_leaf_parent, uint32_t *d_merge_eid,
                             uint32_t *d_merge_parent, uint32_t *d_child_a, uint32_t *d_child_b, uint32_t *d_size,
                             void *d_workspace, size_t workspace_bytes, void *stream, ghs_dendro_result_t *result) {
  hipStream_t st = (hipStream_t)stream;
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_dendro_result_t{};
  if (n == 0) {
    result->is_forest = 1;
    return GHS_OK;
  }
  if (m >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "m must be < 2^31");
  if (!d_leaf_parent) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if ((uint64_t)n + (m < (uint64_t)n - 1 ? m : (uint64_t)n - 1) > (1ull << 32))
    GHS_FAIL(GHS_E_ARG, "n + min(m, n - 1) node ids must fit 32 bits");
  if (((uintptr_t)d_leaf_parent | (uintptr_t)d_merge_eid | (uintptr_t)d_merge_parent | (uintptr_t)d_child_a |
       (uintptr_t)d_child_b | (uintptr_t)d_size) & 3)
    GHS_FAIL(GHS_E_ARG, "leaf_parent, merge_eid, merge_parent, child_a, child_b and size must be 4-byte aligned");
  if (m) {
    if (!d_u || !d_v || !d_w || !d_in_mst || !d_merge_eid || !d_merge_parent || !d_workspace)
      GHS_FAIL(GHS_E_ARG, "NULL pointer");
    if (((uintptr_t)d_u | (uintptr_t)d_v | (uintptr_t)d_w | (uintptr_t)d_workspace) & 15)
      GHS_FAIL(GHS_E_ARG, "u, v, w and the workspace must be 16-byte aligned");
    if (workspace_bytes < ghs_forest_dendro_workspace_bytes(n, m)) GHS_FAIL(GHS_E_NOMEM, "workspace too small");
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");

  const auto t0 = std::chrono::steady_clock::now();
  if (m == 0) {
    GHS_HIP_CHECK(hipMemsetAsync(d_leaf_parent, 0xff, (size_t)n * 4, st));
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
  char *scr = base + l.scratch;
  void *prim = base + l.prim;
  uint32_t *status = (uint32_t *)(base + l.status);
  Flags flags{status + ST_SLOTS, 0};
  uint32_t *chg = nullptr;
  uint32_t h32 = 0;

  // step 1: count, the count comes back first
  GHS_HIP_CHECK(hipMemsetAsync(status, 0, 1024, st));
  const uint64_t lo = (uintptr_t)d_in_mst & 15, hi = lo + m;
  const uintptr_t frame = (uintptr_t)d_in_mst - lo;
  const unsigned ftiles = (unsigned)((hi + DG_FLAG_TILE - 1) / DG_FLAG_TILE);  // <= flag_tiles(m)
  uint32_t *tiles = (uint32_t *)(scr + l.a_tiles);
  k_dg_flag_count<<<ftiles, DG_BLOCK, 0, st>>>(frame, lo, hi, tiles);
  k_dg_tile_scan<<<1, 1024, 0, st>>>(tiles, ftiles, status + ST_FLAGGED);
  GHS_HIP_CHECK(hipGetLastError());
  if (int e = read_u32(&h32, status + ST_FLAGGED, st)) return e;
  const uint64_t T64 = h32;
  if (T64 > l.cap) GHS_FAIL(GHS_E_ARG, "more flags than a forest can hold");
  result->flagged_edges = T64;
  GHS_HIP_CHECK(hipMemsetAsync(d_leaf_parent, 0xff, (size_t)n * 4, st));
  if (T64 == 0) {
    GHS_HIP_CHECK(hipStreamSynchronize(st));
    result->num_trees = n;
    result->is_forest = 1;
    result->ms_total = ms_since(t0);
    return GHS_OK;
  }
  const uint32_t t = (uint32_t)T64;
  uint32_t rounds = 0;
  {
    uint64_t *keys = (uint64_t *)(scr + l.a_keys), *keys2 = (uint64_t *)(scr + l.a_keys2);
    const uint32_t eb = key_end_bit(m) - 32;
    k_dg_gather_keys<<<ftiles, DG_BLOCK, 0, st>>>(frame, lo, hi, d_w, tiles, eb, keys, l.cap);
    GHS_HIP_CHECK(hipGetLastError());
    size_t need = sort_keys_bytes(t, m);
    if (need > l.prim_bytes) GHS_FAIL(GHS_E_STATE, "dendro: the sort needs more storage than the workspace holds");
    GHS_HIP_CHECK(rocprim::radix_sort_keys(prim, need, (const uint64_t *)keys, keys2, (size_t)t, 0u, key_end_bit(m), st));
    k_dg_unpack<<<grid_for(t), DG_BLOCK, 0, st>>>(t, keys2, eb, m, d_u, d_v, d_merge_eid, (uint32_t *)(base + l.ea[0]),
                                                  (uint32_t *)(base + l.eb[0]));
    GHS_HIP_CHECK(hipGetLastError());
  }

  // step 2: contraction levels
  LevelInfo lev[DG_MAX_LEVELS + 1];
  const uint32_t level_cap = ceil_log2(n > 2 ? n : 2);
  int L = 0;
  uint32_t nv = n, ne = t;
  bool forest = true;
  uint32_t *ptra = (uint32_t *)(scr + l.d_ptra), *ptrb = (uint32_t *)(scr + l.d_ptrb);
  uint32_t *hasa = (uint32_t *)(scr + l.d_hasa);
  uint64_t *gval = (uint64_t *)(scr + l.d_gval), *gpre = (uint64_t *)(scr + l.d_gpre);
  uint32_t *aflag = (uint32_t *)(scr + l.d_aflag), *apre = (uint32_t *)(scr + l.d_apre);
  while (ne > 0) {
    if ((uint32_t)L >= level_cap || L >= l.levels) GHS_FAIL(GHS_E_ROUNDCAP, "dendro: level cap exceeded");
    uint32_t *mn = L ? (uint32_t *)(base + l.mn[L]) : d_leaf_parent;
    const uint32_t *ea = (const uint32_t *)(base + l.ea[L]), *eb = (const uint32_t *)(base + l.eb[L]);
    const unsigned vgrid = grid_for(nv), egrid = grid_for(ne);
    if (L) GHS_HIP_CHECK(hipMemsetAsync(mn, 0xff, (size_t)nv * 4, st));
    k_dg_minedge<<<egrid, DG_BLOCK, 0, st>>>(ne, ea, eb, nv, mn);
    uint32_t *pcur = ptra, *pnxt = ptrb;
    k_dg_point<<<vgrid, DG_BLOCK, 0, st>>>(nv, ne, mn, ea, eb, pcur, hasa);
    GHS_HIP_CHECK(hipGetLastError());
    const uint32_t jump_cap = ceil_log2(nv) + 1;
    uint32_t flag = 1;
    for (uint32_t r = 0; flag; ++r) {
      if (r >= jump_cap) GHS_FAIL(GHS_E_ROUNDCAP, "dendro: round cap exceeded");
      if (int e = next_flag(flags, st, &chg)) return e;
      k_dg_jump<<<vgrid, DG_BLOCK, 0, st>>>(nv, pcur, pnxt, chg);
      GHS_HIP_CHECK(hipGetLastError());
      if (int e = read_u32(&flag, chg, st)) return e;
      std::swap(pcur, pnxt);
      ++rounds;
    }
    k_dg_mark_alpha<<<egrid, DG_BLOCK, 0, st>>>(ne, ea, eb, mn, pcur, aflag, hasa);
    k_dg_group_vals<<<vgrid, DG_BLOCK, 0, st>>>(nv, mn, pcur, hasa, gval);
    GHS_HIP_CHECK(hipGetLastError());
    size_t need = scan_bytes<uint32_t>((uint64_t)ne + 1);
    if (need > l.prim_bytes) GHS_FAIL(GHS_E_STATE, "dendro: the scan needs more storage than the workspace holds");
    GHS_HIP_CHECK(rocprim::exclusive_scan(prim, need, (const uint32_t *)aflag, apre, 0u, (size_t)ne + 1,
                                          rocprim::plus<uint32_t>(), st));
    need = scan_bytes<uint64_t>((uint64_t)nv + 1);
    if (need > l.prim_bytes) GHS_FAIL(GHS_E_STATE, "dendro: the scan needs more storage than the workspace holds");
    GHS_HIP_CHECK(rocprim::exclusive_scan(prim, need, (const uint64_t *)gval, gpre, (uint64_t)0, (size_t)nv + 1,
                                          rocprim::plus<uint64_t>(), st));
    uint32_t ne2 = 0;
    uint64_t gtot = 0;
    GHS_HIP_CHECK(hipMemcpyAsync(&ne2, apre + ne, 4, hipMemcpyDeviceToHost, st));
    GHS_HIP_CHECK(hipMemcpyAsync(&gtot, gpre + nv, 8, hipMemcpyDeviceToHost, st));
    GHS_HIP_CHECK(hipStreamSynchronize(st));
    const uint32_t nv2 = (uint32_t)gtot, ngroups = (uint32_t)(gtot >> 32);
    // a forest halves: ne' <= (ne - trees) / 2; its groups with an alpha edge number at most 2 ne'
    if (ne2 > ne / 2 || (uint64_t)ne2 > l.E[L + 1] || (uint64_t)nv2 > 2ull * ne2) {
      forest = false;
      break;
    }
    k_dg_split<<<egrid, DG_BLOCK, 0, st>>>(ne, ea, eb, pcur, hasa, aflag, apre, gpre, ne2,
                                           ne2 ? (uint32_t *)(base + l.ea[L + 1]) : nullptr,
                                           ne2 ? (uint32_t *)(base + l.eb[L + 1]) : nullptr,
                                           ne2 ? (uint32_t *)(base + l.back[L + 1]) : nullptr,
                                           (uint32_t *)(base + l.clist[L]), (uint32_t *)(base + l.cg[L]),
                                           (uint32_t *)(base + l.cs[L]), status + ST_CYC);
    GHS_HIP_CHECK(hipGetLastError());
    if (int e = read_u32(&h32, status + ST_CYC, st)) return e;
    if (h32) {
      forest = false;
      break;
    }
    lev[L] = LevelInfo{nv, ne, ne2, nv2, ngroups};
    ++L;
    nv = nv2;
    ne = ne2;
  }
  result->levels = (uint32_t)L;
  result->rounds = rounds;
  if (!forest) {
    result->levels = (uint32_t)L + 1;
    result->ms_total = ms_since(t0);
    return GHS_OK;  // is_forest = 0: the arrays are unspecified
  }

  // step 3: expansion, deepest level first
  uint32_t *up = (uint32_t *)(scr + l.u_up), *kb = (uint32_t *)(scr + l.u_kb), *kbs = (uint32_t *)(scr + l.u_kbs),
           *perm = (uint32_t *)(scr + l.u_perm);
  for (int lv = L - 1; lv >= 0; --lv) {
    const LevelInfo &I = lev[lv];
    const uint32_t nc = I.ne - I.ne2;
    uint32_t *par = lv ? (uint32_t *)(base + l.par[lv]) : d_merge_parent;
    const uint32_t *par2 = I.ne2 ? (const uint32_t *)(base + l.par[lv + 1]) : nullptr;
    const uint32_t *back2 = I.ne2 ? (const uint32_t *)(base + l.back[lv + 1]) : nullptr;
    const uint32_t *mn2 = I.ne2 ? (const uint32_t *)(base + l.mn[lv + 1]) : nullptr;
    const uint32_t *clist = (const uint32_t *)(base + l.clist[lv]), *cg = (const uint32_t *)(base + l.cg[lv]),
                   *cs = (const uint32_t *)(base + l.cs[lv]);
    int tables = 0;
    if (I.ne2) {
      const unsigned agrid = grid_for(I.ne2);
      const uint32_t table_cap = ceil_log2(I.ne2) + 2;
      uint32_t flag = 1;
      for (uint32_t r = 0; flag; ++r) {
        if (r >= table_cap || r >= l.tables) GHS_FAIL(GHS_E_ROUNDCAP, "dendro: round cap exceeded");
        if (int e = next_flag(flags, st, &chg)) return e;
        if (r == 0)
          k_dg_lift_first<<<agrid, DG_BLOCK, 0, st>>>(I.ne2, par2, up, chg);
        else
          k_dg_lift_next<<<agrid, DG_BLOCK, 0, st>>>(I.ne2, up + (size_t)(r - 1) * I.ne2, up + (size_t)r * I.ne2, chg);
        GHS_HIP_CHECK(hipGetLastError());
        if (int e = read_u32(&flag, chg, st)) return e;
        if (flag) ++tables;
        ++rounds;
      }
      k_dg_alpha_par<<<agrid, DG_BLOCK, 0, st>>>(I.ne2, par2, back2, I.ne, par);
    }
    const unsigned cgrid = grid_for(nc);
    k_dg_lift<<<cgrid, DG_BLOCK, 0, st>>>(nc, clist, cg, cs, I.nv2, mn2, I.ne2, up, tables, I.ngroups, kb);
    GHS_HIP_CHECK(hipGetLastError());
    const unsigned bits = b_bits((uint64_t)I.ngroups + I.ne2);
    size_t need = sort_pairs_bytes(nc, bits);
    if (need > l.prim_bytes) GHS_FAIL(GHS_E_STATE, "dendro: the sort needs more storage than the workspace holds");
    GHS_HIP_CHECK(rocprim::radix_sort_pairs(prim, need, (const uint32_t *)kb, kbs, rocprim::counting_iterator<uint32_t>(0),
                                            perm, (size_t)nc, 0u, bits, st));
    k_dg_chain<<<cgrid, DG_BLOCK, 0, st>>>(nc, kbs, perm, clist, cs, I.nv2, mn2, I.ne2, par2, back2, I.ngroups, I.ne, par);
    GHS_HIP_CHECK(hipGetLastError());
  }

  // step 4: children, sizes, height
  // (the sums are formed only when d_size is given: the first buffer is d_size itself)
  Up *upc = (Up *)(scr + l.f_upa), *upn = (Up *)(scr + l.f_upb);
  uint32_t *acc = d_size, *acc2 = d_size ? (uint32_t *)(scr + l.f_acca) : nullptr;
  const unsigned tgrid = grid_for(t);
  if (d_child_a) GHS_HIP_CHECK(hipMemsetAsync(d_child_a, 0xff, (size_t)t * 4, st));
  if (d_child_b) GHS_HIP_CHECK(hipMemsetAsync(d_child_b, 0, (size_t)t * 4, st));
  if (acc) GHS_HIP_CHECK(hipMemsetAsync(acc, 0, (size_t)t * 4, st));
  if (int e = next_flag(flags, st, &chg)) return e;
  k_dg_leaf_children<<<grid_for(n), DG_BLOCK, 0, st>>>(n, t, d_leaf_parent, d_child_a, d_child_b, acc);
  k_dg_merge_children<<<tgrid, DG_BLOCK, 0, st>>>(n, t, d_merge_parent, d_child_a, d_child_b, upc, chg);
  GHS_HIP_CHECK(hipGetLastError());
  uint32_t flag = 0;
  if (int e = read_u32(&flag, chg, st)) return e;
  ++rounds;
  const uint32_t size_cap = ceil_log2(t) + 2;
  for (uint32_t r = 0; flag; ++r) {
    if (r >= size_cap) GHS_FAIL(GHS_E_ROUNDCAP, "dendro: round cap exceeded");
    if (int e = next_flag(flags, st, &chg)) return e;
    if (acc) GHS_HIP_CHECK(hipMemcpyAsync(acc2, acc, (size_t)t * 4, hipMemcpyDeviceToDevice, st));
    k_dg_size_round<<<tgrid, DG_BLOCK, 0, st>>>(t, upc, upn, acc, acc2, chg);
    GHS_HIP_CHECK(hipGetLastError());
    if (int e = read_u32(&flag, chg, st)) return e;
    std::swap(upc, upn);
    std::swap(acc, acc2);
    ++rounds;
  }
  k_dg_max_hop<<<tgrid, DG_BLOCK, 0, st>>>(t, upc, status + ST_MAXD);
  GHS_HIP_CHECK(hipGetLastError());
  if (d_size && acc != d_size) GHS_HIP_CHECK(hipMemcpyAsync(d_size, acc, (size_t)t * 4, hipMemcpyDeviceToDevice, st));
  if (int e = read_u32(&h32, status + ST_MAXD, st)) return e;

  result->num_trees = (uint64_t)n - t;
  result->max_height = (uint64_t)h32 + 1;
  result->rounds = rounds;
  result->is_forest = 1;
  result->ms_total = ms_since(t0);
  return GHS_OK;
}

// Host-buffer form: copy in, run, copy out on the default stream
int ghs_forest_dendro_host(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w,
                           const uint8_t *in_mst, uint32_t *leaf_parent, uint32_t *merge_eid, uint32_t *merge_parent,
                           uint32_t *child_a, uint32_t *child_b, uint32_t *size, ghs_dendro_result_t *result) {
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_dendro_result_t{};
  if (n == 0) {
    result->is_forest = 1;
    return GHS_OK;
  }
  if (m >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "m must be < 2^31");
  if (!leaf_parent || (m && (!u || !v || !w || !in_mst || !merge_eid || !merge_parent)))
    GHS_FAIL(GHS_E_ARG, "NULL host pointer");
  if (int e = ghs::require_device()) return e;
  const size_t ws = m ? ghs_forest_dendro_workspace_bytes(n, m) : 0;
  const uint64_t C = m < (uint64_t)n - 1 ? m : (uint64_t)n - 1;
  ghs::Staging s;
  const auto d_u = s.take<uint32_t>(m), d_v = s.take<uint32_t>(m), d_w = s.take<uint32_t>(m);
  const auto d_f = s.take<uint8_t>(m);
  const auto d_l = s.take<uint32_t>(n);
  uint32_t *h_out[5] = {merge_eid, merge_parent, child_a, child_b, size};
  ghs::Staging::Piece<uint32_t> d_out[5];
  for (auto &p : d_out) p = s.take<uint32_t>(C);
  const auto d_ws = s.take<char>(ws);
  GHS_HIP_CHECK(s.alloc());
  hipStream_t st = nullptr;
  GHS_HIP_CHECK(s.up(d_u, u, st));
  GHS_HIP_CHECK(s.up(d_v, v, st));
  GHS_HIP_CHECK(s.up(d_w, w, st));
  GHS_HIP_CHECK(s.up(d_f, in_mst, st));
  int rc = ghs_forest_dendro_device(n, m, s.at(d_u), s.at(d_v), s.at(d_w), s.at(d_f), s.at(d_l), s.at(d_out[0]), s.at(d_out[1]),
                                    s.at(d_out[2], child_a), s.at(d_out[3], child_b), s.at(d_out[4], size), s.at(d_ws), ws, st,
                                    result);
  if (rc) return rc;
  GHS_HIP_CHECK(s.down(leaf_parent, d_l, n));
  // only the t merges that exist, and none of them when the flags close a cycle
  const size_t t = result->is_forest ? (size_t)result->flagged_edges : 0;
  for (int k = 0; k < 5; ++k) GHS_HIP_CHECK(s.down(h_out[k], d_out[k], t));
  return GHS_OK;
}

}  // extern "C"
