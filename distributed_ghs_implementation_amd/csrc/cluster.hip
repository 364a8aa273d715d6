// HDBSCAN cluster extraction (ABI 10 addition, ghs_forest_cluster_device): the condensed tree of a
// single-linkage dendrogram for a min_cluster_size, every cluster's stability, the excess-of-mass (or
// leaf) selection, and per vertex a label, noise (-1) and a membership probability. The input is a
// dendrogram as ghs_forest_dendro_device writes it plus one float64 height per merge; no edge list.
// A dendrogram is as high as a path is long, so nothing steps level by level in its height.
//
// Pipeline (everything on `stream`), mcs = min_cluster_size, big(j) = size[j] >= mcs:
//   0. validation, before anything follows a pointer: every index in range, merge_parent strictly
//      ascending (so every chain of parents ends), each child's parent pointer is the merge, the sizes
//      add up, the heights are finite, > 0 and non-decreasing, and exactly 2 t nodes have a parent (so a
//      node with a parent is a child of it). Anything else: GHS_E_ARG.
//   1. heads and anchors by pointer doubling, one array over the merges, fused: a small merge points
//      to its parent and doubles while its target is small (it ends at its first big ancestor, the
//      anchor of the vertices below it, or at none); a big merge that is no head points to its parent
//      and doubles until it stands on a head (heads are fixed points).
//   2. the heads are flagged, one integer scan numbers them, in reverse merge order (a parent cluster
//      has a smaller id than its children), one pass writes the cluster arrays and the two child slots
//      of every parent cluster (left = the smaller id).
//   3. every vertex: its anchor, its cluster, its lambda. A stable rocPRIM radix sort by cluster id
//      lines the lambdas up in segments (vertex order inside a segment); one wave (a 1024-thread block
//      for a long segment) sums a segment in a fixed order: lane partials over a stride, a butterfly,
//      then the two child rows in child-id order. No floating-point atomics, no scan over doubles:
//      two calls give the same bytes. The same pass takes the maximum lambda of the cluster's own rows.
//   4. the EOM sweep, synchronous in the condensed tree's height H_c only: frontiers, a finished
//      cluster writes its best into its own slot at the parent and decrements the parent's pending
//      count; whoever reaches zero appends the parent. Once a frontier fits one workgroup (<= 1024) a
//      single workgroup finishes all remaining levels with a barrier per level.
//   5. the topmost chosen ancestor-or-self of every cluster by pointer doubling over cluster_parent,
//      one scan numbers the selected clusters, one pass over the vertices writes labels and
//      probabilities.
//
// This translation unit includes common.h only and launches only its own kernels.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "common.h"

namespace ghs {
namespace cluster {

constexpr int CL_BLOCK = 256;
constexpr int CL_TAIL_BLOCK = 1024;       // the widest frontier one workgroup finishes
constexpr uint32_t CL_SEG_LONG = 4096;    // a longer segment is summed by a block, not a wave
constexpr uint32_t CL_NONE = 0xffffffffu;

// status block: uint32 slots, a uint64 at byte 32, CL_FLAG_SLOTS round flags from byte 64
enum { ST_BAD = 0, ST_NTOP, ST_NOISE, ST_NLONG, ST_FRONT, ST_LEVELS, ST_SLOTS = 8 };
constexpr uint32_t ST_PARENTS64 = 4;  // index as uint64: byte 32
constexpr uint32_t ST_FLAGS = 16;     // index as uint32: byte 64
constexpr uint32_t CL_FLAG_SLOTS = 16;

struct Opt {
  uint32_t single;  // allow_single_cluster
  uint32_t leaf;    // selection method leaf
};

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static inline unsigned grid_for(uint64_t items, unsigned per_block = CL_BLOCK, unsigned cap = 2048) {
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

#define CL_FOR(i, N) \
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < (N); i += (uint64_t)gridDim.x * blockDim.x)

// ---- step 0: validation --------------------------------------------------------------------------------
// Every load below is in bounds for any input: an index is compared with its bound before it is used.
__global__ __launch_bounds__(CL_BLOCK) void k_cl_validate(uint32_t n, uint32_t t, const uint32_t *__restrict__ leaf_parent,
                                                          const uint32_t *__restrict__ merge_parent,
                                                          const uint32_t *__restrict__ child_a,
                                                          const uint32_t *__restrict__ child_b,
                                                          const uint32_t *__restrict__ size,
                                                          const double *__restrict__ height, uint32_t *__restrict__ status) {
  bool bad = false;
  unsigned long long parents = 0;
  const uint64_t N = n > t ? n : t;
  CL_FOR(i, N) {
    if (i < n) {
      const uint32_t p = leaf_parent[i];
      if (p != CL_NONE) {
        ++parents;
        bad |= p >= t;
      }
    }
    if (i < t) {
      const uint32_t j = (uint32_t)i;
      const uint32_t p = merge_parent[j];
      if (p != CL_NONE) {
        ++parents;
        bad |= !(p > j && p < t);
      }
      const uint64_t ca = child_a[j], cb = child_b[j];
      if (!(ca < cb && cb < (uint64_t)n + j)) {
        bad = true;
      } else {
        uint64_t sum = 0;
        const uint64_t ch[2] = {ca, cb};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          if (ch[k] < n) {
            bad |= leaf_parent[ch[k]] != j;
            sum += 1;
          } else {
            bad |= merge_parent[ch[k] - n] != j;
            sum += size[ch[k] - n];
          }
        }
        bad |= sum != (uint64_t)size[j];
      }
      const double h = height[j];
      bad |= !(h > 0.0 && h < INFINITY);  // false for a NaN too
      if (j) bad |= !(h >= height[j - 1]);
    }
  }
  if (bad) status[ST_BAD] = 1;
  if (parents) atomicAdd(reinterpret_cast<unsigned long long *>(status) + ST_PARENTS64, parents);
}

// ---- step 1: heads and anchors --------------------------------------------------------------------------
__device__ __forceinline__ bool true_split(uint32_t s, uint32_t n, uint32_t t, uint32_t mcs,
                                           const uint32_t *__restrict__ child_a, const uint32_t *__restrict__ child_b,
                                           const uint32_t *__restrict__ size) {
  const uint32_t a = child_a[s], b = child_b[s];
  if (a < n || b < n) return false;  // a vertex has size 1 < mcs
  const uint32_t ja = a - n, jb = b - n;
  if (ja >= t || jb >= t) return false;  // never: validated
  return size[ja] >= mcs && size[jb] >= mcs;
}

// ptr[j]: a small merge -> its parent (or none); a big merge -> itself when it is a head, else its
// parent. flag has t + 1 entries (the last one 0: the scan's total lands there).
__global__ __launch_bounds__(CL_BLOCK) void k_cl_init_ptr(uint32_t n, uint32_t t, uint32_t mcs,
                                                          const uint32_t *__restrict__ merge_parent,
                                                          const uint32_t *__restrict__ child_a,
                                                          const uint32_t *__restrict__ child_b,
                                                          const uint32_t *__restrict__ size, uint32_t *__restrict__ ptr,
                                                          uint32_t *__restrict__ flag) {
  CL_FOR(i, (uint64_t)t + 1) {
    uint32_t head = 0;
    if (i < t) {
      const uint32_t j = (uint32_t)i;
      uint32_t p = merge_parent[j];
      if (p >= t) p = CL_NONE;
      if (size[j] >= mcs) {
        head = (p == CL_NONE || true_split(p, n, t, mcs, child_a, child_b, size)) ? 1u : 0u;
        if (head) p = j;
      }
      ptr[j] = p;
    }
    flag[i] = head;
  }
}

__global__ __launch_bounds__(CL_BLOCK) void k_cl_jump(uint32_t t, uint32_t mcs, const uint32_t *__restrict__ size,
                                                      const uint32_t *__restrict__ in, uint32_t *__restrict__ out,
                                                      uint32_t *__restrict__ chg) {
  bool any = false;
  CL_FOR(j, t) {
    const uint32_t p = in[j];
    uint32_t q = p;
    if (p < t) {
      if (size[j] >= mcs)
        q = in[p];  // big: towards the head (a fixed point)
      else if (size[p] < mcs)
        q = in[p];  // small over small: towards the first big ancestor, or none
    }
    if (q >= t) q = q == CL_NONE ? CL_NONE : p;  // never out of range
    out[j] = q;
    any |= q != p;
  }
  if (any) *chg = 1;
}

// ---- step 2: the cluster arrays --------------------------------------------------------------------------
// head j -> cluster K - 1 - pre[j] (pre: heads in front of j)
__global__ __launch_bounds__(CL_BLOCK) void k_cl_compact(uint32_t n, uint32_t t, uint32_t K,
                                                         const uint32_t *__restrict__ merge_parent,
                                                         const uint32_t *__restrict__ child_a,
                                                         const uint32_t *__restrict__ child_b,
                                                         const uint32_t *__restrict__ size,
                                                         const double *__restrict__ height, const uint32_t *__restrict__ ptr,
                                                         const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pre,
                                                         uint32_t *__restrict__ c_head, uint32_t *__restrict__ c_parent,
                                                         uint32_t *__restrict__ c_size, double *__restrict__ c_birth,
                                                         uint32_t *__restrict__ c_child, uint32_t *__restrict__ c_slot,
                                                         uint32_t *__restrict__ status) {
  uint32_t tops = 0;
  CL_FOR(i, t) {
    const uint32_t j = (uint32_t)i;
    if (!flag[j]) continue;
    const uint32_t c = K - 1 - pre[j];
    if (c >= K) {  // cannot happen after validation: reported, not skipped silently
      status[ST_BAD] = 1;
      continue;
    }
    uint32_t s = merge_parent[j];
    uint32_t pc = CL_NONE, slot = 0;
    double birth = 0.0;
    if (s < t) {
      birth = 1.0 / height[s];
      const uint32_t ph = ptr[s];  // the split's head
      if (ph < t && flag[ph]) pc = K - 1 - pre[ph];
      if (pc >= K) {
        pc = CL_NONE;
        status[ST_BAD] = 1;
      }
      const uint32_t a = child_a[s] - n, b = child_b[s] - n;  // both merges: s is a true split
      const uint32_t sib = a == j ? b : a;
      slot = j > sib ? 0u : 1u;  // the later merge has the smaller id
      if (pc != CL_NONE) c_child[2 * (size_t)pc + slot] = c;
    } else {
      ++tops;
    }
    c_head[c] = j;
    c_parent[c] = pc;
    c_size[c] = size[j];
    c_birth[c] = birth;
    c_slot[c] = slot;
  }
  if (tops) atomicAdd(&status[ST_NTOP], tops);
}

// ---- step 3: points, segments, stabilities ------------------------------------------------------------
// key[v]: the cluster id, K for noise (sorted last)
__global__ __launch_bounds__(CL_BLOCK) void k_cl_points(uint32_t n, uint32_t t, uint32_t mcs, uint32_t K,
                                                        const uint32_t *__restrict__ leaf_parent,
                                                        const uint32_t *__restrict__ size,
                                                        const double *__restrict__ height, const uint32_t *__restrict__ ptr,
                                                        const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pre,
                                                        uint32_t *__restrict__ point_cluster, uint32_t *__restrict__ key,
                                                        double *__restrict__ lambda, uint32_t *__restrict__ status) {
  CL_FOR(v, n) {
    uint32_t a = t ? leaf_parent[v] : CL_NONE;
    if (a < t && size[a] < mcs) a = ptr[a];  // the first big ancestor
    uint32_t c = CL_NONE;
    double lam = 0.0;
    if (a < t) {
      const uint32_t h = ptr[a];
      if (h < t && flag[h]) c = K - 1 - pre[h];
      if (c >= K) {  // an anchor always stands under a head
        c = CL_NONE;
        status[ST_BAD] = 1;
      }
      if (c != CL_NONE) lam = 1.0 / height[a];
    }
    point_cluster[v] = c;
    if (key) key[v] = c == CL_NONE ? K : c;
    lambda[v] = lam;
  }
}

// own[c] = the vertices of c outside its child clusters (own has K + 1 entries); pending, best slots
__global__ __launch_bounds__(CL_BLOCK) void k_cl_counts(uint32_t K, const uint32_t *__restrict__ c_size,
                                                        const uint32_t *__restrict__ c_child, uint32_t *__restrict__ own,
                                                        uint32_t *__restrict__ pending, double *__restrict__ slots) {
  CL_FOR(i, (uint64_t)K + 1) {
    uint32_t cnt = 0;
    if (i < K) {
      const uint32_t a = c_child[2 * i], b = c_child[2 * i + 1];
      uint32_t below = 0;
      if (a < K) below += c_size[a];
      if (b < K) below += c_size[b];
      cnt = c_size[i] >= below ? c_size[i] - below : 0;
      pending[i] = (a < K ? 1u : 0u) + (b < K ? 1u : 0u);
      slots[2 * i] = 0.0;
      slots[2 * i + 1] = 0.0;
    }
    own[i] = cnt;
  }
}

// the last steps of a segment's sum, by one lane: the two child rows in child-id order
__device__ __forceinline__ void finish_cluster(uint32_t c, uint32_t K, double sum, double mx, double birth,
                                               const uint32_t *__restrict__ c_child, const uint32_t *__restrict__ c_size,
                                               const double *__restrict__ c_birth, double *__restrict__ c_stab,
                                               double *__restrict__ c_maxl) {
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint32_t d = c_child[2 * (size_t)c + k];
    if (d < K) {
      const double bd = c_birth[d];
      sum += (double)c_size[d] * (bd - birth);
      mx = bd > mx ? bd : mx;
    }
  }
  c_stab[c] = sum;
  c_maxl[c] = mx;
}

// one wave per cluster: lane l adds rows l, l + 64, ... in that order, then a butterfly
__global__ __launch_bounds__(CL_BLOCK) void k_cl_stab_wave(uint32_t K, uint32_t n, const uint32_t *__restrict__ off,
                                                           const double *__restrict__ lam, const uint32_t *__restrict__ c_child,
                                                           const uint32_t *__restrict__ c_size,
                                                           const double *__restrict__ c_birth, double *__restrict__ c_stab,
                                                           double *__restrict__ c_maxl, uint32_t *__restrict__ long_list,
                                                           uint32_t long_cap, uint32_t *__restrict__ status) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
  const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  for (uint64_t c = wave; c < K; c += waves) {
    const uint32_t o = off[c], e = off[c + 1];
    if (e < o || e > n) {  // the offsets are a scan of counts that sum to at most n
      if (lane == 0) status[ST_BAD] = 1;
      continue;
    }
    const uint32_t cnt = e - o;
    if (cnt > CL_SEG_LONG) {
      if (lane == 0) {
        const uint32_t pos = atomicAdd(&status[ST_NLONG], 1u);
        if (pos < long_cap)
          long_list[pos] = (uint32_t)c;
        else
          status[ST_BAD] = 1;  // more long segments than n / 4096 + 1
      }
      continue;
    }
    const double birth = c_birth[c];
    double sum = 0.0, mx = 0.0;
    for (uint32_t i = lane; i < cnt; i += 64) {
      const double l = lam[(size_t)o + i];
      sum += l - birth;
      mx = l > mx ? l : mx;
    }
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) {
      const double os = __shfl_xor(sum, k), om = __shfl_xor(mx, k);
      sum += os;
      mx = om > mx ? om : mx;
    }
    if (lane == 0) finish_cluster((uint32_t)c, K, sum, mx, birth, c_child, c_size, c_birth, c_stab, c_maxl);
  }
}

// one 1024-thread block per long segment: thread partials over a stride of 1024, a butterfly per
// wave, the 16 wave sums in wave order
__global__ __launch_bounds__(CL_TAIL_BLOCK) void k_cl_stab_block(uint32_t K, uint32_t n, const uint32_t *__restrict__ off,
                                                                 const double *__restrict__ lam,
                                                                 const uint32_t *__restrict__ c_child,
                                                                 const uint32_t *__restrict__ c_size,
                                                                 const double *__restrict__ c_birth,
                                                                 double *__restrict__ c_stab, double *__restrict__ c_maxl,
                                                                 const uint32_t *__restrict__ long_list, uint32_t long_cap,
                                                                 uint32_t *__restrict__ status) {
  __shared__ double s_sum[CL_TAIL_BLOCK / 64], s_max[CL_TAIL_BLOCK / 64];
  uint32_t nlong = status[ST_NLONG];
  if (nlong > long_cap) nlong = long_cap;
  for (uint32_t b = blockIdx.x; b < nlong; b += gridDim.x) {
    const uint32_t c = long_list[b];
    const uint32_t o = c < K ? off[c] : 1u, e = c < K ? off[c + 1] : 0u;
    if (e < o || e > n) {  // block-uniform; cannot happen: reported, not skipped silently
      if (threadIdx.x == 0) status[ST_BAD] = 1;
      continue;
    }
    const uint32_t cnt = e - o;
    const double birth = c_birth[c];
    double sum = 0.0, mx = 0.0;
    for (uint32_t i = threadIdx.x; i < cnt; i += CL_TAIL_BLOCK) {
      const double l = lam[(size_t)o + i];
      sum += l - birth;
      mx = l > mx ? l : mx;
    }
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) {
      const double os = __shfl_xor(sum, k), om = __shfl_xor(mx, k);
      sum += os;
      mx = om > mx ? om : mx;
    }
    if ((threadIdx.x & 63) == 0) {
      s_sum[threadIdx.x >> 6] = sum;
      s_max[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      sum = s_sum[0];
      mx = s_max[0];
      for (int w = 1; w < CL_TAIL_BLOCK / 64; ++w) {
        sum += s_sum[w];
        mx = s_max[w] > mx ? s_max[w] : mx;
      }
      finish_cluster(c, K, sum, mx, birth, c_child, c_size, c_birth, c_stab, c_maxl);
    }
    __syncthreads();
  }
}

// ---- step 4: the selection sweep ---------------------------------------------------------------------------
// exclusive prefix of x over the block's 256 threads; *total: the sum
__device__ __forceinline__ uint32_t block_excl(uint32_t x, uint32_t *s_v, uint32_t *total) {
  s_v[threadIdx.x] = x;
  __syncthreads();
#pragma unroll
  for (int d = 1; d < CL_BLOCK; d <<= 1) {
    const uint32_t o = threadIdx.x >= (unsigned)d ? s_v[threadIdx.x - d] : 0u;
    __syncthreads();
    s_v[threadIdx.x] = o + s_v[threadIdx.x];
    __syncthreads();
  }
  const uint32_t inc = s_v[threadIdx.x];
  *total = s_v[CL_BLOCK - 1];
  __syncthreads();
  return inc - x;
}

// every thread of the block calls it: the wanted values go to list[*counter ...], one atomic per block
__device__ __forceinline__ void block_append(bool want, uint32_t value, uint32_t *__restrict__ list, uint32_t cap,
                                             uint32_t *__restrict__ counter, uint32_t *s_v, uint32_t *s_base) {
  uint32_t tot;
  const uint32_t at = block_excl(want ? 1u : 0u, s_v, &tot);
  if (threadIdx.x == 0 && tot) *s_base = atomicAdd(counter, tot);
  __syncthreads();
  if (want) {
    const uint64_t pos = (uint64_t)*s_base + at;
    if (pos < cap) list[pos] = value;
  }
  __syncthreads();
}

// the first frontier: the clusters without children
__global__ __launch_bounds__(CL_BLOCK) void k_cl_leaves(uint32_t K, const uint32_t *__restrict__ pending,
                                                        uint32_t *__restrict__ front, uint32_t *__restrict__ counter) {
  __shared__ uint32_t s_v[CL_BLOCK];
  __shared__ uint32_t s_base;
  const uint64_t span = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t b = blockIdx.x * (uint64_t)blockDim.x; b < K; b += span) {
    const uint64_t c = b + threadIdx.x;
    block_append(c < K && pending[c] == 0, (uint32_t)c, front, K, counter, s_v, &s_base);
  }
}

// one finished cluster: chosen or not, its best to its own slot at the parent; true: the parent is
// finished too (this was its last child)
__device__ __forceinline__ bool sweep_one(uint32_t c, uint32_t K, Opt opt, bool lone_top_out,
                                          const uint32_t *__restrict__ c_parent, const uint32_t *__restrict__ c_child,
                                          const uint32_t *__restrict__ c_slot, const double *__restrict__ c_stab,
                                          double *slots, uint32_t *pending, uint32_t *__restrict__ chosen, uint32_t *parent) {
  const bool leaf = c_child[2 * (size_t)c] >= K;
  const double s = leaf ? 0.0 : slots[2 * (size_t)c] + slots[2 * (size_t)c + 1];
  const double st = c_stab[c];
  const uint32_t p = c_parent[c];
  bool pick;
  double best;
  if (p >= K && lone_top_out) {
    pick = false;
    best = s;
  } else if (leaf) {
    pick = true;
    best = st;
  } else if (opt.leaf || s > st) {
    pick = false;
    best = s;
  } else {
    pick = true;
    best = st;
  }
  chosen[c] = pick ? 1u : 0u;
  *parent = p;
  if (p >= K) return false;
  slots[2 * (size_t)p + (c_slot[c] & 1u)] = best;
  __threadfence();
  return atomicSub(&pending[p], 1u) == 1u;
}

__global__ __launch_bounds__(CL_BLOCK) void k_cl_sweep(uint32_t count, uint32_t K, Opt opt, const uint32_t *__restrict__ front,
                                                       const uint32_t *__restrict__ c_parent,
                                                       const uint32_t *__restrict__ c_child,
                                                       const uint32_t *__restrict__ c_slot, const double *__restrict__ c_stab,
                                                       double *slots, uint32_t *pending, uint32_t *__restrict__ chosen,
                                                       uint32_t *__restrict__ next, uint32_t *__restrict__ counter,
                                                       const uint32_t *__restrict__ status) {
  __shared__ uint32_t s_v[CL_BLOCK];
  __shared__ uint32_t s_base;
  const bool lone_top_out = status[ST_NTOP] == 1 && !opt.single;
  const uint64_t span = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t b = blockIdx.x * (uint64_t)blockDim.x; b < count; b += span) {
    const uint64_t i = b + threadIdx.x;
    bool up = false;
    uint32_t p = CL_NONE;
    if (i < count) {
      const uint32_t c = front[i];
      if (c < K) up = sweep_one(c, K, opt, lone_top_out, c_parent, c_child, c_slot, c_stab, slots, pending, chosen, &p);
    }
    block_append(up, p, next, K, counter, s_v, &s_base);
  }
}

// a frontier of at most 1024 clusters: every remaining level in one workgroup, a barrier per level
// (frontiers never widen: every cluster of the next one has a child of its own in this one)
__global__ __launch_bounds__(CL_TAIL_BLOCK) void k_cl_sweep_tail(uint32_t count, uint32_t K, Opt opt,
                                                                 const uint32_t *__restrict__ front,
                                                                 const uint32_t *__restrict__ c_parent,
                                                                 const uint32_t *__restrict__ c_child,
                                                                 const uint32_t *__restrict__ c_slot,
                                                                 const double *__restrict__ c_stab, double *slots,
                                                                 uint32_t *pending, uint32_t *__restrict__ chosen,
                                                                 uint32_t *__restrict__ status) {
  __shared__ uint32_t s_front[2][CL_TAIL_BLOCK];
  __shared__ uint32_t s_count[2];
  const bool lone_top_out = status[ST_NTOP] == 1 && !opt.single;
  if (count > CL_TAIL_BLOCK) {  // the host hands over at <= 1024
    count = CL_TAIL_BLOCK;
    if (threadIdx.x == 0) status[ST_BAD] = 1;
  }
  if (threadIdx.x < count) s_front[0][threadIdx.x] = front[threadIdx.x];
  if (threadIdx.x == 0) {
    s_count[0] = count;
    s_count[1] = 0;
  }
  __syncthreads();
  uint32_t levels = 0;
  int cur = 0;
  for (uint32_t guard = 0; guard <= K; ++guard) {  // at most K levels
    const uint32_t cnt = s_count[cur];
    if (cnt == 0) break;
    if (threadIdx.x < cnt) {
      const uint32_t c = s_front[cur][threadIdx.x];
      uint32_t p = CL_NONE;
      if (c < K && sweep_one(c, K, opt, lone_top_out, c_parent, c_child, c_slot, c_stab, slots, pending, chosen, &p)) {
        const uint32_t pos = atomicAdd(&s_count[cur ^ 1], 1u);
        if (pos < CL_TAIL_BLOCK) s_front[cur ^ 1][pos] = p;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      s_count[cur] = 0;
      if (s_count[cur ^ 1] > CL_TAIL_BLOCK) {  // frontiers never widen
        s_count[cur ^ 1] = CL_TAIL_BLOCK;
        status[ST_BAD] = 1;
      }
    }
    __syncthreads();
    cur ^= 1;
    ++levels;
  }
  if (threadIdx.x == 0) status[ST_LEVELS] = levels;
}

// ---- step 5: selected ancestors, labels, probabilities ------------------------------------------------
__global__ __launch_bounds__(CL_BLOCK) void k_cl_top_init(uint32_t K, const uint32_t *__restrict__ c_parent,
                                                          const uint32_t *__restrict__ chosen, uint32_t *__restrict__ up,
                                                          uint32_t *__restrict__ top) {
  CL_FOR(c, K) {
    const uint32_t p = c_parent[c];
    up[c] = p < K ? p : CL_NONE;
    top[c] = chosen[c] ? (uint32_t)c : CL_NONE;
  }
}

// top[c]: the topmost chosen cluster among c and its ancestors below up[c]
__global__ __launch_bounds__(CL_BLOCK) void k_cl_top_round(uint32_t K, const uint32_t *__restrict__ up_in,
                                                           const uint32_t *__restrict__ top_in, uint32_t *__restrict__ up_out,
                                                           uint32_t *__restrict__ top_out, uint32_t *__restrict__ chg) {
  bool any = false;
  CL_FOR(c, K) {
    const uint32_t u = up_in[c];
    uint32_t tp = top_in[c], nu = CL_NONE;
    if (u < K) {
      const uint32_t tu = top_in[u];
      if (tu < K) tp = tu;
      nu = up_in[u];
      if (nu >= K) nu = CL_NONE;
    }
    up_out[c] = nu;
    top_out[c] = tp;
    any |= nu != CL_NONE;
  }
  if (any) *chg = 1;
}

// sel has K + 1 entries (the last one 0)
__global__ __launch_bounds__(CL_BLOCK) void k_cl_selected(uint32_t K, const uint32_t *__restrict__ top,
                                                          uint8_t *__restrict__ c_selected, uint32_t *__restrict__ sel) {
  CL_FOR(c, (uint64_t)K + 1) {
    const uint32_t s = (c < K && top[c] == (uint32_t)c) ? 1u : 0u;
    if (c < K) c_selected[c] = (uint8_t)s;
    sel[c] = s;
  }
}

__global__ __launch_bounds__(CL_BLOCK) void k_cl_labels(uint32_t n, uint32_t K, const uint32_t *__restrict__ point_cluster,
                                                        const double *__restrict__ lambda, const uint32_t *__restrict__ top,
                                                        const uint32_t *__restrict__ selpre, const double *__restrict__ c_maxl,
                                                        int32_t *__restrict__ label, double *__restrict__ prob,
                                                        uint32_t *__restrict__ status) {
  uint32_t noise = 0;
  CL_FOR(v, n) {
    const uint32_t c = point_cluster[v];
    int32_t lab = -1;
    double pr = 0.0;
    if (c < K) {
      const uint32_t s = top[c];
      if (s < K) {
        lab = (int32_t)selpre[s];
        const double M = c_maxl[s], l = lambda[v];
        pr = M == 0.0 ? 1.0 : (l < M ? l : M) / M;
      }
    }
    noise += lab < 0 ? 1u : 0u;
    label[v] = lab;
    if (prob) prob[v] = pr;
  }
  if (noise) atomicAdd(&status[ST_NOISE], noise);
}

// no cluster at all: every vertex is noise
__global__ __launch_bounds__(CL_BLOCK) void k_cl_all_noise(uint32_t n, int32_t *__restrict__ label, double *__restrict__ prob,
                                                           uint32_t *__restrict__ point_cluster, double *__restrict__ lambda) {
  CL_FOR(v, n) {
    label[v] = -1;
    point_cluster[v] = CL_NONE;
    if (prob) prob[v] = 0.0;
    if (lambda) lambda[v] = 0.0;
  }
}

// ---- workspace ------------------------------------------------------------------------------------------
//   per merge     16 B: two pointer buffers, the head flags and their scan (t + 1 entries each);
//   per vertex    24 B: the sort's keys in and out (4 + 4), lambda when the caller keeps none (8), the
//                 sorted lambdas (8);
//   per cluster of capacity cap = min(t, 2 floor(n / mcs)): 84 B: two child slots 8, slot 4, pending 4,
//                 two best slots 16, own counts and offsets 8, stability's maximum 8, chosen 4, two
//                 frontiers 8, (up, top) twice 16, selected flags and their scan 8; 4 B per 4096 vertices (long segments);
//   rocPRIM's sort / scan storage, 1 KiB of status.
struct Layout {
  uint64_t cap;
  size_t ptra, ptrb, flag, pre;
  size_t key, key2, lam, lam2;
  size_t child, slot, pending, slots, own, off, maxl, chosen, fronta, frontb, upa, upb, topa, topb, sel, selpre, longl;
  uint64_t long_cap;
  size_t prim, prim_bytes, status, total;
};

static inline uint64_t capacity(uint32_t n, uint64_t t, uint32_t mcs) {
  if (mcs < 2) return 0;
  const uint64_t c = 2ull * (n / mcs);
  return t < c ? t : c;
}

static size_t sort_bytes(uint64_t N, unsigned bits) {
  size_t b = 0;
  if (N == 0) return 0;
  (void)rocprim::radix_sort_pairs(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const double *)nullptr,
                                  (double *)nullptr, (size_t)N, 0u, bits);
  return b;
}
static size_t scan_bytes(uint64_t N) {
  size_t b = 0;
  if (N == 0) return 0;
  (void)rocprim::exclusive_scan(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)N,
                                rocprim::plus<uint32_t>());
  return b;
}

static Layout layout(uint32_t n, uint64_t t, uint32_t mcs) {
  Layout l{};
  l.cap = capacity(n, t, mcs);
  const size_t C = (size_t)l.cap;
  size_t o = 0;
  auto take = [&o](size_t bytes) {
    const size_t at = o;
    o += align256(bytes);
    return at;
  };
  l.ptra = take((size_t)t * 4);
  l.ptrb = take((size_t)t * 4);
  l.flag = take(((size_t)t + 1) * 4);
  l.pre = take(((size_t)t + 1) * 4);
  l.key = take((size_t)n * 4);
  l.key2 = take((size_t)n * 4);
  l.lam = take((size_t)n * 8);
  l.lam2 = take((size_t)n * 8);
  l.child = take(C * 8);
  l.slot = take(C * 4);
  l.pending = take(C * 4);
  l.slots = take(C * 16);
  l.own = take((C + 1) * 4);
  l.off = take((C + 1) * 4);
  l.maxl = take(C * 8);
  l.chosen = take(C * 4);
  l.fronta = take(C * 4);
  l.frontb = take(C * 4);
  l.upa = take(C * 4);
  l.upb = take(C * 4);
  l.topa = take(C * 4);
  l.topb = take(C * 4);
  l.sel = take((C + 1) * 4);
  l.selpre = take((C + 1) * 4);
  l.long_cap = (uint64_t)n / CL_SEG_LONG + 1;
  l.longl = take((size_t)l.long_cap * 4);
  size_t pb = sort_bytes(n, 32);
  const size_t p2 = scan_bytes((uint64_t)t + 1), p3 = scan_bytes((uint64_t)C + 1);
  pb = p2 > pb ? p2 : pb;
  pb = p3 > pb ? p3 : pb;
  l.prim_bytes = align256(pb) + 65536;
  l.prim = take(l.prim_bytes);
  l.status = take(1024);
  l.total = o;
  return l;
}

static int read_u32(uint32_t *h, const uint32_t *d, hipStream_t st) {
  GHS_HIP_CHECK(hipMemcpyAsync(h, d, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipStreamSynchronize(st));
  return GHS_OK;
}

// One round flag per launch out of the status block; cleared again when the slots run out: every
// earlier flag has been read by then, and the memset is ordered behind the kernels that wrote them.
struct Flags {
  uint32_t *base;
  uint32_t used;
};
static int next_flag(Flags &f, hipStream_t st, uint32_t **out) {
  if (f.used == CL_FLAG_SLOTS) {
    GHS_HIP_CHECK(hipMemsetAsync(f.base, 0, CL_FLAG_SLOTS * sizeof(uint32_t), st));
    f.used = 0;
  }
  *out = f.base + f.used++;
  return GHS_OK;
}

static inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

static int check_host_args(uint32_t n, uint64_t t, uint32_t mcs, uint32_t flags) {
  if (mcs < 2) GHS_FAIL(GHS_E_ARG, "min_cluster_size must be >= 2");
  if (flags & ~(uint32_t)(GHS_CLUSTER_ALLOW_SINGLE | GHS_CLUSTER_LEAF)) GHS_FAIL(GHS_E_ARG, "unknown cluster flags");
  if ((uint64_t)n + t > (1ull << 32)) GHS_FAIL(GHS_E_ARG, "n + t node ids must fit 32 bits");
  return GHS_OK;
}

}  // namespace cluster
}  // namespace ghs

using namespace ghs;
using namespace ghs::cluster;

extern "C" {

size_t ghs_forest_cluster_workspace_bytes(uint32_t n, uint64_t t, uint32_t min_cluster_size) {
  if (n == 0 || min_cluster_size < 2 || (uint64_t)n + t > (1ull << 32)) return 0;
  return layout(n, t, min_cluster_size).total;
}

uint64_t ghs_forest_cluster_capacity(uint32_t n, uint64_t t, uint32_t min_cluster_size) {
  return capacity(n, t, min_cluster_size);
}

int ghs_forest_cluster_device(uint32_t n, uint64_t t64, const uint32_t *d_leaf_parent, const uint32_t *d_merge_parent,
                              const uint32_t *d_child_a, const uint32_t *d_child_b, const uint32_t *d_size,
                              const double *d_height, uint32_t min_cluster_size, uint32_t flags, int32_t *d_label,
                              double *d_probability, uint32_t *d_point_cluster, double *d_point_lambda,
                              uint32_t *d_cluster_head, uint32_t *d_cluster_parent, uint32_t *d_cluster_size,
                              double *d_cluster_birth, double *d_cluster_stability, uint8_t *d_cluster_selected,
                              void *d_workspace, size_t workspace_bytes, void *stream, ghs_cluster_result_t *result) {
  hipStream_t st = (hipStream_t)stream;
  const uint32_t mcs = min_cluster_size;
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_cluster_result_t{};
  if (int e = check_host_args(n, t64, mcs, flags)) return e;
  if (n == 0) return GHS_OK;
  const uint64_t cap = capacity(n, t64, mcs);
  if (!d_label || !d_point_cluster || !d_workspace) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if (t64 && (!d_leaf_parent || !d_merge_parent || !d_child_a || !d_child_b || !d_size || !d_height))
    GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if (cap && (!d_cluster_head || !d_cluster_parent || !d_cluster_size || !d_cluster_birth || !d_cluster_stability ||
              !d_cluster_selected))
    GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if (((uintptr_t)d_leaf_parent | (uintptr_t)d_merge_parent | (uintptr_t)d_child_a | (uintptr_t)d_child_b |
       (uintptr_t)d_size | (uintptr_t)d_label | (uintptr_t)d_point_cluster | (uintptr_t)d_cluster_head |
       (uintptr_t)d_cluster_parent | (uintptr_t)d_cluster_size) & 3)
    GHS_FAIL(GHS_E_ARG, "the 32-bit arrays must be 4-byte aligned");
  if (((uintptr_t)d_height | (uintptr_t)d_probability | (uintptr_t)d_point_lambda | (uintptr_t)d_cluster_birth |
       (uintptr_t)d_cluster_stability) & 7)
    GHS_FAIL(GHS_E_ARG, "the float64 arrays must be 8-byte aligned");
  if ((uintptr_t)d_workspace & 15) GHS_FAIL(GHS_E_ARG, "the workspace must be 16-byte aligned");
  if (workspace_bytes < ghs_forest_cluster_workspace_bytes(n, t64, mcs)) GHS_FAIL(GHS_E_NOMEM, "workspace too small");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");

  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t t = (uint32_t)t64;  // n + t <= 2^32 and n >= 1
  const Layout l = layout(n, t64, mcs);
  char *base = (char *)d_workspace;
  uint32_t *status = (uint32_t *)(base + l.status);
  const unsigned ngrid = grid_for(n), tgrid = grid_for(t);
  GHS_HIP_CHECK(hipMemsetAsync(status, 0, 1024, st));

  // step 0: nothing below runs on a dendrogram that did not pass
  uint32_t hst[ST_SLOTS + 2] = {0};
  if (t) {
    k_cl_validate<<<grid_for(n > t ? n : t), CL_BLOCK, 0, st>>>(n, t, d_leaf_parent, d_merge_parent, d_child_a, d_child_b,
                                                                d_size, d_height, status);
    GHS_HIP_CHECK(hipGetLastError());
    GHS_HIP_CHECK(hipMemcpyAsync(hst, status, sizeof(hst), hipMemcpyDeviceToHost, st));
    GHS_HIP_CHECK(hipStreamSynchronize(st));
    uint64_t parents = 0;
    memcpy(&parents, hst + 2 * ST_PARENTS64, 8);
    if (hst[ST_BAD] || parents != 2ull * t)
      GHS_FAIL(GHS_E_ARG, "malformed dendrogram (indices, parent and child pointers, sizes, or heights not finite, "
                          "> 0 and non-decreasing)");
  }
  if (t == 0 || cap == 0) {
    k_cl_all_noise<<<ngrid, CL_BLOCK, 0, st>>>(n, d_label, d_probability, d_point_cluster, d_point_lambda);
    GHS_HIP_CHECK(hipGetLastError());
    GHS_HIP_CHECK(hipStreamSynchronize(st));
    result->num_noise = n;
    result->ms_total = ms_since(t0);
    return GHS_OK;
  }

  Flags rf{status + ST_FLAGS, 0};
  uint32_t *chg = nullptr;
  uint32_t rounds = 0;
  void *prim = base + l.prim;
  uint32_t *pcur = (uint32_t *)(base + l.ptra), *pnxt = (uint32_t *)(base + l.ptrb);
  uint32_t *flag = (uint32_t *)(base + l.flag), *pre = (uint32_t *)(base + l.pre);

  // step 1
  k_cl_init_ptr<<<tgrid, CL_BLOCK, 0, st>>>(n, t, mcs, d_merge_parent, d_child_a, d_child_b, d_size, pcur, flag);
  GHS_HIP_CHECK(hipGetLastError());
  {
    const uint32_t jump_cap = ceil_log2(t) + 1;
    uint32_t f = 1;
    for (uint32_t r = 0; f; ++r) {
      if (r >= jump_cap) GHS_FAIL(GHS_E_ROUNDCAP, "cluster: round cap exceeded");
      if (int e = next_flag(rf, st, &chg)) return e;
      k_cl_jump<<<tgrid, CL_BLOCK, 0, st>>>(t, mcs, d_size, pcur, pnxt, chg);
      GHS_HIP_CHECK(hipGetLastError());
      if (int e = read_u32(&f, chg, st)) return e;
      std::swap(pcur, pnxt);
      ++rounds;
    }
  }

  // step 2
  size_t need = scan_bytes((uint64_t)t + 1);
  if (need > l.prim_bytes) GHS_FAIL(GHS_E_STATE, "cluster: the scan needs more storage than the workspace holds");
  GHS_HIP_CHECK(rocprim::exclusive_scan(prim, need, (const uint32_t *)flag, pre, 0u, (size_t)t + 1,
                                        rocprim::plus<uint32_t>(), st));
  uint32_t K = 0;
  if (int e = read_u32(&K, pre + t, st)) return e;
  if (K > cap) GHS_FAIL(GHS_E_ARG, "malformed dendrogram (more clusters than its vertices can hold)");
  result->rounds = rounds;
  if (K == 0) {
    k_cl_all_noise<<<ngrid, CL_BLOCK, 0, st>>>(n, d_label, d_probability, d_point_cluster, d_point_lambda);
    GHS_HIP_CHECK(hipGetLastError());
    GHS_HIP_CHECK(hipStreamSynchronize(st));
    result->num_noise = n;
    result->ms_total = ms_since(t0);
    return GHS_OK;
  }
  const unsigned kgrid = grid_for(K), k1grid = grid_for((uint64_t)K + 1);
  uint32_t *c_child = (uint32_t *)(base + l.child), *c_slot = (uint32_t *)(base + l.slot);
  uint32_t *pending = (uint32_t *)(base + l.pending), *chosen = (uint32_t *)(base + l.chosen);
  double *slots = (double *)(base + l.slots), *c_maxl = (double *)(base + l.maxl);
  uint32_t *own = (uint32_t *)(base + l.own), *off = (uint32_t *)(base + l.off);
  GHS_HIP_CHECK(hipMemsetAsync(c_child, 0xff, (size_t)K * 8, st));
  k_cl_compact<<<tgrid, CL_BLOCK, 0, st>>>(n, t, K, d_merge_parent, d_child_a, d_child_b, d_size, d_height, pcur, flag,
                                           pre, d_cluster_head, d_cluster_parent, d_cluster_size, d_cluster_birth, c_child,
                                           c_slot, status);

  // step 3
  uint32_t *key = (uint32_t *)(base + l.key), *key2 = (uint32_t *)(base + l.key2);
  double *lam = d_point_lambda ? d_point_lambda : (double *)(base + l.lam), *lam2 = (double *)(base + l.lam2);
  k_cl_points<<<ngrid, CL_BLOCK, 0, st>>>(n, t, mcs, K, d_leaf_parent, d_size, d_height, pcur, flag, pre, d_point_cluster, key,
                                          lam, status);
  k_cl_counts<<<k1grid, CL_BLOCK, 0, st>>>(K, d_cluster_size, c_child, own, pending, slots);
  GHS_HIP_CHECK(hipGetLastError());
  need = scan_bytes((uint64_t)K + 1);
  if (need > l.prim_bytes) GHS_FAIL(GHS_E_STATE, "cluster: the scan needs more storage than the workspace holds");
  GHS_HIP_CHECK(rocprim::exclusive_scan(prim, need, (const uint32_t *)own, off, 0u, (size_t)K + 1, rocprim::plus<uint32_t>(),
                                        st));
  const unsigned kbits = ceil_log2((uint64_t)K + 1) ? ceil_log2((uint64_t)K + 1) : 1u;
  need = sort_bytes(n, kbits);
  if (need > l.prim_bytes) GHS_FAIL(GHS_E_STATE, "cluster: the sort needs more storage than the workspace holds");
  GHS_HIP_CHECK(rocprim::radix_sort_pairs(prim, need, (const uint32_t *)key, key2, (const double *)lam, lam2, (size_t)n, 0u,
                                          kbits, st));
  uint32_t *long_list = (uint32_t *)(base + l.longl);
  k_cl_stab_wave<<<grid_for((uint64_t)K * 64), CL_BLOCK, 0, st>>>(K, n, off, lam2, c_child, d_cluster_size, d_cluster_birth,
                                                                  d_cluster_stability, c_maxl, long_list,
                                                                  (uint32_t)l.long_cap, status);
  k_cl_stab_block<<<grid_for(l.long_cap, 1, 1024), CL_TAIL_BLOCK, 0, st>>>(K, n, off, lam2, c_child, d_cluster_size,
                                                                          d_cluster_birth, d_cluster_stability, c_maxl,
                                                                          long_list, (uint32_t)l.long_cap, status);
  GHS_HIP_CHECK(hipGetLastError());

  // step 4
  const Opt opt{(flags & GHS_CLUSTER_ALLOW_SINGLE) ? 1u : 0u, (flags & GHS_CLUSTER_LEAF) ? 1u : 0u};
  uint32_t *fcur = (uint32_t *)(base + l.fronta), *fnxt = (uint32_t *)(base + l.frontb);
  uint32_t launches = 0, levels = 0, count = 0;
  k_cl_leaves<<<kgrid, CL_BLOCK, 0, st>>>(K, pending, fcur, status + ST_FRONT);
  GHS_HIP_CHECK(hipGetLastError());
  ++launches;
  if (int e = read_u32(&count, status + ST_FRONT, st)) return e;
  while (count > CL_TAIL_BLOCK) {
    if (levels > K) GHS_FAIL(GHS_E_ROUNDCAP, "cluster: sweep cap exceeded");
    if (count > K) GHS_FAIL(GHS_E_STATE, "cluster: a frontier larger than the condensed tree");
    GHS_HIP_CHECK(hipMemsetAsync(status + ST_FRONT, 0, 4, st));
    k_cl_sweep<<<grid_for(count), CL_BLOCK, 0, st>>>(count, K, opt, fcur, d_cluster_parent, c_child, c_slot,
                                                     d_cluster_stability, slots, pending, chosen, fnxt, status + ST_FRONT,
                                                     status);
    GHS_HIP_CHECK(hipGetLastError());
    if (int e = read_u32(&count, status + ST_FRONT, st)) return e;
    std::swap(fcur, fnxt);
    ++launches;
    ++levels;
  }
  if (count) {
    k_cl_sweep_tail<<<1, CL_TAIL_BLOCK, 0, st>>>(count, K, opt, fcur, d_cluster_parent, c_child, c_slot, d_cluster_stability,
                                                 slots, pending, chosen, status);
    GHS_HIP_CHECK(hipGetLastError());
    ++launches;
  }

  // step 5
  uint32_t *upc = (uint32_t *)(base + l.upa), *upn = (uint32_t *)(base + l.upb);
  uint32_t *topc = (uint32_t *)(base + l.topa), *topn = (uint32_t *)(base + l.topb);
  k_cl_top_init<<<kgrid, CL_BLOCK, 0, st>>>(K, d_cluster_parent, chosen, upc, topc);
  GHS_HIP_CHECK(hipGetLastError());
  {
    const uint32_t top_cap = ceil_log2(K) + 1;
    uint32_t f = 1;
    for (uint32_t r = 0; f; ++r) {
      if (r >= top_cap) GHS_FAIL(GHS_E_ROUNDCAP, "cluster: round cap exceeded");
      if (int e = next_flag(rf, st, &chg)) return e;
      k_cl_top_round<<<kgrid, CL_BLOCK, 0, st>>>(K, upc, topc, upn, topn, chg);
      GHS_HIP_CHECK(hipGetLastError());
      if (int e = read_u32(&f, chg, st)) return e;
      std::swap(upc, upn);
      std::swap(topc, topn);
      ++rounds;
    }
  }
  uint32_t *sel = (uint32_t *)(base + l.sel), *selpre = (uint32_t *)(base + l.selpre);
  k_cl_selected<<<k1grid, CL_BLOCK, 0, st>>>(K, topc, d_cluster_selected, sel);
  GHS_HIP_CHECK(hipGetLastError());
  need = scan_bytes((uint64_t)K + 1);
  GHS_HIP_CHECK(rocprim::exclusive_scan(prim, need, (const uint32_t *)sel, selpre, 0u, (size_t)K + 1, rocprim::plus<uint32_t>(),
                                        st));
  k_cl_labels<<<ngrid, CL_BLOCK, 0, st>>>(n, K, d_point_cluster, lam, topc, selpre, c_maxl, d_label, d_probability, status);
  GHS_HIP_CHECK(hipGetLastError());
  uint32_t nsel = 0;
  GHS_HIP_CHECK(hipMemcpyAsync(hst, status, sizeof(hst), hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipMemcpyAsync(&nsel, selpre + K, 4, hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipStreamSynchronize(st));

  if (hst[ST_BAD]) GHS_FAIL(GHS_E_STATE, "cluster: an index left its range after validation (internal error)");
  result->num_clusters = K;
  result->num_selected = nsel;
  result->num_noise = hst[ST_NOISE];
  result->num_top = hst[ST_NTOP];
  result->cluster_height = levels + hst[ST_LEVELS];
  result->rounds = rounds;
  result->select_launches = launches;
  result->ms_total = ms_since(t0);
  return GHS_OK;
}

// Host-buffer form: copy in, run, copy out on the default stream
int ghs_forest_cluster_host(uint32_t n, uint64_t t, const uint32_t *leaf_parent, const uint32_t *merge_parent,
                            const uint32_t *child_a, const uint32_t *child_b, const uint32_t *size, const double *height,
                            uint32_t min_cluster_size, uint32_t flags, int32_t *label, double *probability,
                            uint32_t *point_cluster, double *point_lambda, uint32_t *cluster_head, uint32_t *cluster_parent,
                            uint32_t *cluster_size, double *cluster_birth, double *cluster_stability,
                            uint8_t *cluster_selected, ghs_cluster_result_t *result) {
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_cluster_result_t{};
  if (int e = check_host_args(n, t, min_cluster_size, flags)) return e;
  if (n == 0) return GHS_OK;
  const uint64_t cap = capacity(n, t, min_cluster_size);
  if (!label || !point_cluster || (t && (!leaf_parent || !merge_parent || !child_a || !child_b || !size || !height)) ||
      (cap && (!cluster_head || !cluster_parent || !cluster_size || !cluster_birth || !cluster_stability || !cluster_selected)))
    GHS_FAIL(GHS_E_ARG, "NULL host pointer");
  if (int e = ghs::require_device()) return e;
  const size_t ws = ghs_forest_cluster_workspace_bytes(n, t, min_cluster_size);
  ghs::Staging s;
  // t == 0: the six inputs may be NULL, and none is read
  const size_t n_in = t ? n : 0;
  const auto i_leaf = s.take<uint32_t>(n_in), i_mp = s.take<uint32_t>(t), i_ca = s.take<uint32_t>(t), i_cb = s.take<uint32_t>(t),
             i_sz = s.take<uint32_t>(t);
  const auto i_h = s.take<double>(t);
  const auto o_lab = s.take<int32_t>(n);
  const auto o_pc = s.take<uint32_t>(n);
  const auto o_pr = s.take<double>(n), o_pl = s.take<double>(n);
  const auto c_head = s.take<uint32_t>(cap), c_par = s.take<uint32_t>(cap), c_sz = s.take<uint32_t>(cap);
  const auto c_bi = s.take<double>(cap), c_st = s.take<double>(cap);
  const auto c_sel = s.take<uint8_t>(cap);
  const auto d_ws = s.take<char>(ws);
  GHS_HIP_CHECK(s.alloc());
  hipStream_t st = nullptr;
  GHS_HIP_CHECK(s.up(i_leaf, leaf_parent, st));
  GHS_HIP_CHECK(s.up(i_mp, merge_parent, st));
  GHS_HIP_CHECK(s.up(i_ca, child_a, st));
  GHS_HIP_CHECK(s.up(i_cb, child_b, st));
  GHS_HIP_CHECK(s.up(i_sz, size, st));
  GHS_HIP_CHECK(s.up(i_h, height, st));
  const int rc = ghs_forest_cluster_device(n, t, s.at(i_leaf), s.at(i_mp), s.at(i_ca), s.at(i_cb), s.at(i_sz), s.at(i_h),
                                           min_cluster_size, flags, s.at(o_lab), s.at(o_pr, probability), s.at(o_pc),
                                           s.at(o_pl, point_lambda), s.at(c_head), s.at(c_par), s.at(c_sz), s.at(c_bi),
                                           s.at(c_st), s.at(c_sel), s.at(d_ws), ws, st, result);
  if (rc) return rc;
  GHS_HIP_CHECK(s.down(label, o_lab, n));
  GHS_HIP_CHECK(s.down(point_cluster, o_pc, n));
  GHS_HIP_CHECK(s.down(probability, o_pr, n));
  GHS_HIP_CHECK(s.down(point_lambda, o_pl, n));
  const size_t K = result->num_clusters;  // only the clusters that exist
  GHS_HIP_CHECK(s.down(cluster_head, c_head, K));
  GHS_HIP_CHECK(s.down(cluster_parent, c_par, K));
  GHS_HIP_CHECK(s.down(cluster_size, c_sz, K));
  GHS_HIP_CHECK(s.down(cluster_birth, c_bi, K));
  GHS_HIP_CHECK(s.down(cluster_stability, c_st, K));
  GHS_HIP_CHECK(s.down(cluster_selected, c_sel, K));
  return GHS_OK;
}

}  // extern "C"
