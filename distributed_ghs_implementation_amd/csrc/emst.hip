// Exact minimum spanning tree of the complete graph on float32 points (ABI 10 addition, ghs_emst_device):
// Euclidean weights, or mutual-reachability weights when squared core distances are given. Semantics (the
// distance chain, the weight, the 96-bit pair key, the output order): include/ghs_mst.h.
//
// Boruvka rounds. comp[i] is the label of point i's component, the index of one of its points. A round:
//   k_emst_scan   best[i] = min over the points j of another component of (bits(w2(i, j)) << 32 | j)
//   k_emst_cmin   cmin[comp[i]] = min of (bits << 32 | min(i, j)) over the component's points
//   k_emst_cmax   cmax[comp[i]] = min of max(i, j) over the points that hold cmin: with cmin, the
//                 component's smallest pair key (bits, u, v)
//   k_emst_hook   a component points at the component of its edge's far end and emits the edge; of a mutual
//                 pair (both chose the same edge) the smaller label stays root and only it emits
//   k_emst_jump   pointer jumping to a star (EM_JUMP_HOPS hops per launch, flag-chained launches)
//   k_emst_relabel  comp[i] = par[comp[i]]; best, cmin, cmax reset
// and one host sync, which brings back the edge count. Pair keys are distinct, so every chosen edge is a
// tree edge, the hooks close no cycle but the mutual pairs, and the components at least halve per round.
//
// k_emst_scan, grid = query tiles x slices, 256 threads: the tile machinery of the k-NN scan, restated here
// (this file shares no code with it). A workgroup owns TQ = 64 queries and sweeps the candidate tiles
// (TC = 64) of its slice. A step is one (candidate tile, dim chunk) pair: both sides' CH = 32 dims go through
// LDS dim-major (row stride LD = TQ + 4 floats), fetched from global one step ahead into registers. Lane
// (tq, tc) = (tid / 16, tid % 16) keeps acc[4][4] for queries 4 tq + i and candidates 4 tc + j; every
// accumulator sees the dims in ascending order, s = a - b, acc = fmaf(s, s, acc), so the header's chain is
// reproduced bit for bit whatever the tiling. Rows and dims past the end are zeros in LDS. The labels and
// cores of a step's 64 + 64 points travel through LDS with the tile.
// Selection: no lists, no queues. After a tile's last chunk a lane forms the keys of its pairs with c < n and
// comp[q] != comp[c] and keeps the minimum per query in registers across the sweep; at the end the 16 lanes
// of a query row reduce once and one lane issues one atomicMin on best[q]. Slices need no merge, and a
// minimum does not depend on the arrival order. The max of the weight is taken on the bit patterns
// (non-negative floats order as their bits do).
//
// Validation (k_emst_check) runs first on the stream and raises flags in the status block; every later
// kernel of the round returns at once when a flag is up, so no key is formed from a bad value. No
// floating-point atomics. This translation unit includes common.h only and launches only its own kernels.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>

#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"

namespace ghs {
namespace emst {

constexpr int EM_BLOCK = 256;
constexpr int TQ = GHS_KNN_TILE_Q, TC = GHS_KNN_TILE_C, CH = GHS_KNN_DIM_CHUNK;
constexpr int LD = TQ + 4;             // LDS row stride in floats: rows stay 16-byte aligned
constexpr uint32_t TARGET_WGS = 1024;  // auto slices: 4 workgroups per CU
constexpr int EM_JUMP_HOPS = 8;        // hops per jump launch: launch j reaches min(8^j, depth) levels up
constexpr int EM_JUMPS = 12;           // 8^11 > 2^32
constexpr unsigned long long KEY_MAX = ~0ull;
static_assert(TQ == 64 && TC == 64 && EM_BLOCK == (TQ / 4) * (TC / 4), "4 x 4 accumulators per lane");
static_assert(CH % 4 == 0 && (TQ + TC) * (CH / 4) == 4 * EM_BLOCK, "four 16-byte staging loads per lane and step");
static_assert((LD * 4) % 16 == 0, "LDS rows are read 16 bytes at a time");

// status block (256 B) of uint32 slots
enum { ST_NONFINITE = 0, ST_BADCORE = 1, ST_EDGES = 2, ST_ZEROS = 3, ST_JUMP = 8 /* EM_JUMPS flags */, ST_SLOTS = 64 };
static_assert(ST_JUMP + EM_JUMPS <= ST_SLOTS, "the jump flags fit");

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

__device__ __forceinline__ bool halted(const uint32_t *__restrict__ status) {
  return (status[ST_NONFINITE] | status[ST_BADCORE]) != 0;
}

// the bit pattern a core distance competes with: -0.0 is 0
__device__ __forceinline__ uint32_t core_bits(const float *__restrict__ core2, uint64_t i) {
  const uint32_t b = __float_as_uint(core2[i]);
  return b == 0x80000000u ? 0u : b;
}

// The correctly rounded square root: sqrtf is that under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt (no fast-math in this build).
__device__ __forceinline__ float rounded_sqrt(float d2) { return sqrtf(d2); }

// every coordinate finite; every core distance finite and >= 0
__global__ __launch_bounds__(EM_BLOCK) void k_emst_check(uint32_t n, uint32_t dim, const float *__restrict__ x,
                                                        const float *__restrict__ core2, uint32_t *__restrict__ status) {
  const uint64_t total = (uint64_t)n * dim, stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t t0 = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  bool nonfinite = false, badcore = false;
  for (uint64_t t = t0; t < total; t += stride) nonfinite |= (__float_as_uint(x[t]) & 0x7f800000u) == 0x7f800000u;
  if (core2)
    for (uint64_t t = t0; t < n; t += stride) {
      const uint32_t b = __float_as_uint(core2[t]);
      badcore |= (b & 0x7f800000u) == 0x7f800000u || (b > 0x80000000u);
    }
  if (nonfinite) status[ST_NONFINITE] = 1;
  if (badcore) status[ST_BADCORE] = 1;
}

__global__ __launch_bounds__(EM_BLOCK) void k_emst_init(uint32_t n, uint32_t *__restrict__ comp, uint32_t *__restrict__ par,
                                                       unsigned long long *__restrict__ best,
                                                       unsigned long long *__restrict__ cmin, uint32_t *__restrict__ cmax) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    comp[i] = (uint32_t)i;
    par[i] = (uint32_t)i;
    best[i] = KEY_MAX;
    cmin[i] = KEY_MAX;
    cmax[i] = LABEL_NONE;
  }
}

// One staged piece: four consecutive dims of one row. Every load is unconditional, from the element itself or,
// past the row's or the array's end, from x[0]; bit e of the returned mask says that element e is real.
__device__ __forceinline__ uint32_t load_piece(const float *__restrict__ x, uint32_t n, uint32_t dim, uint64_t row, uint32_t d,
                                               bool vec, float4 &out) {
  const float *p = x + (size_t)(row < n ? row : 0) * dim;
  if (vec) {  // dim % 4 == 0: d + 3 < dim when d < dim, and p + d is 16-byte aligned
    const bool ok = row < n && d < dim;
    out = *reinterpret_cast<const float4 *>(ok ? p + d : x);
    return ok ? 0xfu : 0u;
  }
  uint32_t mask = 0;
  float c[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool ok = row < n && d + e < dim;
    c[e] = *(ok ? p + d + e : x);
    mask |= (uint32_t)ok << e;
  }
  out = make_float4(c[0], c[1], c[2], c[3]);
  return mask;
}

__global__ __launch_bounds__(EM_BLOCK) void k_emst_scan(uint32_t n, uint32_t dim, uint32_t slices, const float *__restrict__ x,
                                                       const float *__restrict__ core2, const uint32_t *__restrict__ comp,
                                                       unsigned long long *__restrict__ best,
                                                       const uint32_t *__restrict__ status) {
  __shared__ __attribute__((aligned(16))) float s_q[CH * LD];
  __shared__ __attribute__((aligned(16))) float s_c[CH * LD];
  __shared__ uint32_t s_qcomp[TQ], s_qcore[TQ], s_ccomp[TC], s_ccore[TC];

  if (halted(status)) return;  // block-uniform, before any barrier
  const uint32_t tid = threadIdx.x, tq = tid >> 4, tc = tid & 15;
  const uint64_t q0 = (uint64_t)blockIdx.x * TQ;
  const uint32_t slice = blockIdx.y;
  const uint32_t ctiles = (uint32_t)(((uint64_t)n + TC - 1) / TC), nchunks = (dim + CH - 1) / CH;
  const uint32_t t_lo = (uint32_t)((uint64_t)slice * ctiles / slices), t_hi = (uint32_t)((uint64_t)(slice + 1) * ctiles / slices);
  const bool vec = (dim & 3u) == 0;

  if (tid < (uint32_t)TQ) {
    const uint64_t row = q0 + tid;
    s_qcomp[tid] = row < n ? comp[row] : LABEL_NONE;
    s_qcore[tid] = row < n && core2 ? core_bits(core2, row) : 0u;
  }

  // a lane's staging pieces: r = 0, 1 of the query side, r = 2, 3 of the candidate side
  const uint32_t st_row[2] = {tid >> 3, (tid + EM_BLOCK) >> 3}, st_d = (tid & 7u) * 4;
  float4 pre[4];
  uint32_t real = 0;  // bit 4 r + e: element e of pre[r] is no padding
  uint32_t pre_comp = 0, pre_core = 0;  // lanes < TC: the label and core of candidate ct * TC + tid
  auto fetch = [&](uint32_t ct, uint32_t dc) {
    real = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      real |= load_piece(x, n, dim, (r < 2 ? q0 : (uint64_t)ct * TC) + st_row[r & 1], dc * CH + st_d, vec, pre[r]) << (4 * r);
    if (dc == 0 && tid < (uint32_t)TC) {
      const uint64_t c = (uint64_t)ct * TC + tid;
      pre_comp = c < n ? comp[c] : LABEL_NONE;
      pre_core = c < n && core2 ? core_bits(core2, c) : 0u;
    }
  };

  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  unsigned long long mine[4] = {KEY_MAX, KEY_MAX, KEY_MAX, KEY_MAX};  // the smallest key of query 4 tq + i so far

  uint32_t ct = t_lo, dc = 0;
  if (ct < t_hi) fetch(ct, dc);
  __syncthreads();  // the query side's labels and cores are in LDS
  uint32_t qcomp[4], qcore[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) qcomp[i] = s_qcomp[tq * 4 + i], qcore[i] = s_qcore[tq * 4 + i];

  while (ct < t_hi) {  // block-uniform
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float *dst = (r < 2 ? s_q : s_c) + st_d * LD + st_row[r & 1];
      const uint32_t m = real >> (4 * r);
      dst[0] = (m & 1u) ? pre[r].x : 0.f, dst[LD] = (m & 2u) ? pre[r].y : 0.f;
      dst[2 * LD] = (m & 4u) ? pre[r].z : 0.f, dst[3 * LD] = (m & 8u) ? pre[r].w : 0.f;
    }
    if (dc == 0 && tid < (uint32_t)TC) s_ccomp[tid] = pre_comp, s_ccore[tid] = pre_core;
    __syncthreads();
    const uint32_t left = dim - dc * CH, tcount = ((left < (uint32_t)CH ? left : (uint32_t)CH) + 3u) & ~3u;
    const uint32_t ct_now = ct;
    const bool last_chunk = dc + 1 == nchunks;
    if (last_chunk) {
      dc = 0;
      ++ct;
    } else {
      ++dc;
    }
    if (ct < t_hi) fetch(ct, dc);  // the next step's pieces travel while this one is computed

    for (uint32_t t = 0; t < tcount; t += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float4 a4 = *reinterpret_cast<const float4 *>(&s_q[(t + u) * LD + tq * 4]);
        const float4 b4 = *reinterpret_cast<const float4 *>(&s_c[(t + u) * LD + tc * 4]);
        const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float s = __fsub_rn(a[i], b[j]);
            acc[i][j] = fmaf(s, s, acc[i][j]);
          }
      }
    }

    if (last_chunk) {
      // a pair competes when the candidate is real and of another component (the query itself never is; a
      // padded query's label LABEL_NONE may differ, and its minimum is dropped at the end)
      const uint64_t c0 = (uint64_t)ct_now * TC + tc * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t cc = s_ccomp[tc * 4 + j], ck = s_ccore[tc * 4 + j];
        const bool creal = c0 + j < n;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          uint32_t wb = __float_as_uint(acc[i][j]);
          wb = wb > qcore[i] ? wb : qcore[i];
          wb = wb > ck ? wb : ck;
          const unsigned long long key = ((unsigned long long)wb << 32) | (uint32_t)(c0 + j);
          if (creal && cc != qcomp[i] && key < mine[i]) mine[i] = key;
          acc[i][j] = 0.f;
        }
      }
    }
    __syncthreads();  // every lane is done with the tiles before the next step overwrites them
  }

  // the 16 lanes of a query row (tc = 0 .. 15, consecutive lanes of one wave) reduce once
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned long long m = mine[i];
#pragma unroll
    for (int s = 8; s > 0; s >>= 1) {
      const unsigned long long o = __shfl_xor(m, s);
      m = o < m ? o : m;
    }
    const uint64_t row = q0 + tq * 4 + i;
    if (tc == 0 && row < n && m != KEY_MAX) atomicMin(&best[row], m);
  }
}

// the component's minimum of (bits, min(i, j))
__global__ __launch_bounds__(EM_BLOCK) void k_emst_cmin(uint32_t n, const uint32_t *__restrict__ comp,
                                                       const unsigned long long *__restrict__ best,
                                                       unsigned long long *__restrict__ cmin) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long b = best[i];
    if (b == KEY_MAX) continue;  // only when the scan did not run
    const uint32_t j = (uint32_t)b, lo = j < (uint32_t)i ? j : (uint32_t)i;
    atomicMin(&cmin[comp[i]], (b & 0xffffffff00000000ull) | lo);
  }
}

// among the points that hold it, the minimum of max(i, j)
__global__ __launch_bounds__(EM_BLOCK) void k_emst_cmax(uint32_t n, const uint32_t *__restrict__ comp,
                                                       const unsigned long long *__restrict__ best,
                                                       const unsigned long long *__restrict__ cmin, uint32_t *__restrict__ cmax) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long b = best[i];
    if (b == KEY_MAX) continue;
    const uint32_t j = (uint32_t)b, lo = j < (uint32_t)i ? j : (uint32_t)i, hi = j < (uint32_t)i ? (uint32_t)i : j;
    const uint32_t c = comp[i];
    if (((b & 0xffffffff00000000ull) | lo) == cmin[c]) atomicMin(&cmax[c], hi);
  }
}

// Component a (a root: comp[a] == a) chose the pair (lo, hi); exactly one of the two is its own point. It
// points at the other's component b, unless b chose the same pair and a < b: then a stays root. Every
// choosing component emits its edge but the larger of a mutual pair.
__global__ __launch_bounds__(EM_BLOCK) void k_emst_hook(uint32_t n, const uint32_t *__restrict__ comp,
                                                       const unsigned long long *__restrict__ cmin,
                                                       const uint32_t *__restrict__ cmax, uint32_t *__restrict__ par,
                                                       unsigned long long *__restrict__ ekey, uint32_t *__restrict__ ebits,
                                                       uint32_t *__restrict__ status) {
  for (uint64_t x = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; x < n; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t a = (uint32_t)x;
    if (comp[a] != a) continue;
    const unsigned long long k = cmin[a];
    if (k == KEY_MAX) continue;  // the last component, or the scan did not run
    const uint32_t lo = (uint32_t)k, hi = cmax[a];
    if (lo >= n || hi >= n) continue;  // never: both are point indices
    const uint32_t clo = comp[lo], b = clo == a ? comp[hi] : clo;
    const bool mutual = cmin[b] == k && cmax[b] == hi;
    if (mutual && a < b) {
      par[a] = a;
    } else {
      par[a] = b;
    }
    if (!mutual || a < b) {
      const uint32_t slot = atomicAdd(&status[ST_EDGES], 1u);
      if (slot < n - 1) {  // never more: every emitted edge is a tree edge
        ekey[slot] = ((unsigned long long)lo << 32) | hi;
        ebits[slot] = (uint32_t)(k >> 32);
      }
    }
  }
}

// Pointer jump, in place: up to EM_JUMP_HOPS hops per launch. Every value read is an ancestor at least as far
// as the previous launch left it, and no root changes while the jumps run, so a launch in which every walk
// saw a root leaves its flag 0 and the launches after it return at once.
__global__ __launch_bounds__(EM_BLOCK) void k_emst_jump(uint32_t n, uint32_t *__restrict__ par, const uint32_t *chg_prev,
                                                       uint32_t *chg_cur) {
  if (chg_prev && *chg_prev == 0) return;
  bool open = false;
  for (uint64_t x = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; x < n; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t p0 = par[x];
    uint32_t p = p0;
    bool o = true;
#pragma unroll 1
    for (int h = 0; h < EM_JUMP_HOPS; ++h) {
      const uint32_t g = par[p];
      if (g == p) {
        o = false;
        break;
      }
      p = g;
    }
    if (p != p0) par[x] = p;
    open |= o;
  }
  if (open) *chg_cur = 1;
}

__global__ __launch_bounds__(EM_BLOCK) void k_emst_relabel(uint32_t n, uint32_t *__restrict__ comp, const uint32_t *__restrict__ par,
                                                          unsigned long long *__restrict__ best,
                                                          unsigned long long *__restrict__ cmin, uint32_t *__restrict__ cmax,
                                                          uint32_t *__restrict__ status) {
  const uint64_t t0 = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  for (uint64_t i = t0; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    comp[i] = par[comp[i]];
    best[i] = KEY_MAX;
    cmin[i] = KEY_MAX;
    cmax[i] = LABEL_NONE;
  }
  if (t0 < (uint64_t)EM_JUMPS) status[ST_JUMP + t0] = 0;  // read by this round's jumps only, which are done
}

// the sorted edges in the caller's arrays, the weight in the metric's units
__global__ __launch_bounds__(EM_BLOCK) void k_emst_write(uint32_t t, uint32_t metric, const unsigned long long *__restrict__ ekey,
                                                        const uint32_t *__restrict__ ebits, uint32_t *__restrict__ u,
                                                        uint32_t *__restrict__ v, float *__restrict__ w,
                                                        uint32_t *__restrict__ status) {
  uint32_t zeros = 0;
  for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < t; e += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long k = ekey[e];
    const uint32_t bits = ebits[e];
    const float w2 = __uint_as_float(bits);
    u[e] = (uint32_t)(k >> 32);
    v[e] = (uint32_t)k;
    w[e] = metric == GHS_KNN_EUCLIDEAN ? rounded_sqrt(w2) : w2;
    zeros += bits == 0;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) zeros += __shfl_xor(zeros, s);
  if ((threadIdx.x & 63) == 0 && zeros) atomicAdd(&status[ST_ZEROS], zeros);
}

// ---- host side ----------------------------------------------------------------------------------------------
static inline uint32_t query_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + TQ - 1) / TQ); }

// a function of n alone, as the k-NN scan's: enough slices for TARGET_WGS workgroups
static inline uint32_t auto_slices(uint32_t n) {
  const uint32_t tiles = query_tiles(n);
  if (tiles == 0) return 1;
  uint32_t s = (TARGET_WGS + tiles - 1) / tiles;
  if (s < 1) s = 1;
  if (s > GHS_KNN_MAX_SLICES) s = GHS_KNN_MAX_SLICES;
  return s;
}

static inline uint32_t ceil_log2(uint32_t n) {
  uint32_t r = 0;
  while (r < 32 && (1ull << r) < n) ++r;
  return r;
}

// the sort key is u << 32 | v with u, v < n
static inline unsigned key_end_bit(uint32_t n) { return 32u + (ceil_log2(n) ? ceil_log2(n) : 1u); }

static size_t sort_bytes(uint32_t t, unsigned end_bit) {
  size_t b = 0;
  if (t == 0) return 0;
  (void)rocprim::radix_sort_pairs(nullptr, b, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                  (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)t, 0u, end_bit);
  return b;
}

struct Layout {
  size_t status, best, cmin, cmax, comp, par, ekey, ekey2, ebits, ebits2, prim, prim_bytes, total;
};

// the slices split the sweep and share best[]: they do not enter the size
static Layout layout(uint32_t n) {
  Layout l{};
  size_t o = 0;
  auto take = [&o](size_t bytes) {
    const size_t at = o;
    o += align256(bytes);
    return at;
  };
  const size_t t = n - 1;
  l.status = take(256);
  l.best = take((size_t)n * 8);
  l.cmin = take((size_t)n * 8);
  l.cmax = take((size_t)n * 4);
  l.comp = take((size_t)n * 4);
  l.par = take((size_t)n * 4);
  l.ekey = take(t * 8);
  l.ekey2 = take(t * 8);
  l.ebits = take(t * 4);
  l.ebits2 = take(t * 4);
  l.prim_bytes = sort_bytes((uint32_t)t, key_end_bit(n));
  l.prim = take(l.prim_bytes);
  l.total = o;
  return l;
}

static inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

static inline bool overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && abytes && bbytes && x < y + bbytes && y < x + abytes;
}

static inline unsigned vgrid(uint64_t items) {
  uint64_t g = (items + EM_BLOCK - 1) / EM_BLOCK;
  if (g < 1) g = 1;
  if (g > 2048) g = 2048;
  return (unsigned)g;
}

// everything that needs no device, in the order the header lists it; *slices becomes the count in use
static int check_args(uint32_t n, uint32_t dim, const float *x, const float *core2, uint32_t metric, uint32_t *slices,
                      const uint32_t *u, const uint32_t *v, const float *w, bool device_form, const void *ws, size_t ws_bytes) {
  if (dim == 0 || dim > GHS_KNN_MAX_DIM) GHS_FAIL(GHS_E_ARG, "dim must be in [1, GHS_KNN_MAX_DIM]");
  if (metric != GHS_KNN_SQEUCLIDEAN && metric != GHS_KNN_EUCLIDEAN) GHS_FAIL(GHS_E_ARG, "unknown metric");
  if (*slices > GHS_KNN_MAX_SLICES) GHS_FAIL(GHS_E_ARG, "slices must be <= GHS_KNN_MAX_SLICES");
  if (n <= 1) return GHS_OK;
  if ((uint64_t)n - 1 >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "n - 1 must be < 2^31");
  if (*slices == 0) *slices = auto_slices(n);
  if (!x || !u || !v || !w || (device_form && !ws)) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if (device_form && (((uintptr_t)x | (uintptr_t)ws) & 15)) GHS_FAIL(GHS_E_ARG, "d_x and the workspace must be 16-byte aligned");
  if (((uintptr_t)u | (uintptr_t)v | (uintptr_t)w | (uintptr_t)core2) & 3)
    GHS_FAIL(GHS_E_ARG, "core2, u, v and w must be 4-byte aligned");
  if (!device_form && ((uintptr_t)x & 3)) GHS_FAIL(GHS_E_ARG, "x must be 4-byte aligned");
  const size_t xb = (size_t)n * dim * 4, cb = (size_t)n * 4, ob = ((size_t)n - 1) * 4;
  const void *p[5] = {x, core2, u, v, w};
  const size_t pb[5] = {xb, cb, ob, ob, ob};
  for (int a = 0; a < 5; ++a)
    for (int b = a + 1; b < 5; ++b)
      if (b >= 2 && overlap(p[a], pb[a], p[b], pb[b])) GHS_FAIL(GHS_E_ARG, "x, core2, u, v and w overlap");
  if (device_form) {
    const size_t need = layout(n).total;
    for (int a = 0; a < 5; ++a)
      if (overlap(ws, need, p[a], pb[a])) GHS_FAIL(GHS_E_ARG, "the workspace overlaps x, core2, u, v or w");
    if (ws_bytes < need) GHS_FAIL(GHS_E_NOMEM, "workspace too small");
  }
  return GHS_OK;
}

// the last call's rounds on this thread (ghs_emst_rounds): the components left after each round, always; the
// HIP-event time of each round's sweep when the caller opted in
constexpr uint32_t ROUND_SLOTS = 32;  // ceil(log2 n) <= 32
thread_local bool t_times_on = false;
thread_local uint32_t t_rounds = 0;
thread_local uint32_t t_components[ROUND_SLOTS];
thread_local double t_scan_ms[ROUND_SLOTS];

struct ScanEvents {
  hipEvent_t ev[2] = {};
  int made = 0;
  bool on = false;
  int start(bool enable) {
    on = enable;
    if (!on) return GHS_OK;
    for (; made < 2; ++made) GHS_HIP_CHECK(hipEventCreate(&ev[made]));
    return GHS_OK;
  }
  int mark(int k, hipStream_t st) {
    if (on) GHS_HIP_CHECK(hipEventRecord(ev[k], st));
    return GHS_OK;
  }
  int read(double *ms) {  // after the round's sync
    float f = 0.f;
    if (on) GHS_HIP_CHECK(hipEventElapsedTime(&f, ev[0], ev[1]));
    *ms = f;
    return GHS_OK;
  }
  ~ScanEvents() {
    for (int k = 0; k < made; ++k) (void)hipEventDestroy(ev[k]);
  }
};

}  // namespace emst
}  // namespace ghs

using namespace ghs;
using namespace ghs::emst;

extern "C" {

size_t ghs_emst_workspace_bytes(uint32_t n, uint32_t dim, uint32_t slices) {
  if (n <= 1 || dim == 0 || dim > GHS_KNN_MAX_DIM || slices > GHS_KNN_MAX_SLICES) return 0;
  if ((uint64_t)n - 1 >= (1ull << 31)) return 0;
  return layout(n).total;
}

int ghs_emst_rounds(int enable, uint32_t capacity, uint32_t *components, double *scan_ms, uint32_t *rounds) {
  const uint32_t r = t_rounds < capacity ? t_rounds : capacity;
  for (uint32_t k = 0; k < r; ++k) {
    if (components) components[k] = t_components[k];
    if (scan_ms) scan_ms[k] = t_scan_ms[k];
  }
  if (rounds) *rounds = t_rounds;
  t_times_on = enable != 0;
  return GHS_OK;
}

int ghs_emst_device(uint32_t n, uint32_t dim, const float *d_x, const float *d_core2, uint32_t metric, uint32_t slices,
                    uint32_t *d_u, uint32_t *d_v, float *d_w, void *d_workspace, size_t workspace_bytes, void *stream,
                    ghs_emst_result_t *result) {
  hipStream_t st = (hipStream_t)stream;
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_emst_result_t{};
  if (int e = check_args(n, dim, d_x, d_core2, metric, &slices, d_u, d_v, d_w, true, d_workspace, workspace_bytes)) return e;
  if (n <= 1) return GHS_OK;
  if (int e = ghs::require_device()) return e;

  const auto t0 = std::chrono::steady_clock::now();
  const Layout l = layout(n);
  char *base = (char *)d_workspace;
  uint32_t *status = (uint32_t *)(base + l.status);
  unsigned long long *best = (unsigned long long *)(base + l.best), *cmin = (unsigned long long *)(base + l.cmin);
  uint32_t *cmax = (uint32_t *)(base + l.cmax), *comp = (uint32_t *)(base + l.comp), *par = (uint32_t *)(base + l.par);
  unsigned long long *ekey = (unsigned long long *)(base + l.ekey), *ekey2 = (unsigned long long *)(base + l.ekey2);
  uint32_t *ebits = (uint32_t *)(base + l.ebits), *ebits2 = (uint32_t *)(base + l.ebits2);
  const uint32_t t = n - 1, cap = ceil_log2(n);
  const unsigned g = vgrid(n);

  GHS_HIP_CHECK(hipMemsetAsync(status, 0, 256, st));
  k_emst_check<<<vgrid((uint64_t)n * dim), EM_BLOCK, 0, st>>>(n, dim, d_x, d_core2, status);
  k_emst_init<<<g, EM_BLOCK, 0, st>>>(n, comp, par, best, cmin, cmax);
  GHS_HIP_CHECK(hipGetLastError());
  const dim3 grid(query_tiles(n), slices);
  uint32_t edges = 0, rounds = 0;
  ScanEvents se;
  if (int e = se.start(t_times_on)) return e;
  t_rounds = 0;
  while (edges < t) {
    if (rounds == cap) GHS_FAIL(GHS_E_ROUNDCAP, "emst: more than ceil(log2 n) rounds (internal error)");
    if (int e = se.mark(0, st)) return e;
    k_emst_scan<<<grid, EM_BLOCK, 0, st>>>(n, dim, slices, d_x, d_core2, comp, best, status);
    if (int e = se.mark(1, st)) return e;
    k_emst_cmin<<<g, EM_BLOCK, 0, st>>>(n, comp, best, cmin);
    k_emst_cmax<<<g, EM_BLOCK, 0, st>>>(n, comp, best, cmin, cmax);
    k_emst_hook<<<g, EM_BLOCK, 0, st>>>(n, comp, cmin, cmax, par, ekey, ebits, status);
    for (int j = 0; j < EM_JUMPS; ++j)
      k_emst_jump<<<g, EM_BLOCK, 0, st>>>(n, par, j ? status + ST_JUMP + j - 1 : nullptr, status + ST_JUMP + j);
    k_emst_relabel<<<g, EM_BLOCK, 0, st>>>(n, comp, par, best, cmin, cmax, status);
    GHS_HIP_CHECK(hipGetLastError());
    uint32_t hst[4] = {0};
    GHS_HIP_CHECK(hipMemcpyAsync(hst, status, sizeof(hst), hipMemcpyDeviceToHost, st));
    GHS_HIP_CHECK(hipStreamSynchronize(st));  // the round's one host sync
    if (hst[ST_NONFINITE]) GHS_FAIL(GHS_E_ARG, "emst: non-finite coordinate (NaN or +-inf) in the points");
    if (hst[ST_BADCORE]) GHS_FAIL(GHS_E_ARG, "emst: bad core distance (NaN, infinite or negative)");
    if (hst[ST_EDGES] > t || hst[ST_EDGES] <= edges) GHS_FAIL(GHS_E_STATE, "emst: a round emitted no edge or too many (internal error)");
    edges = hst[ST_EDGES];
    if (rounds < ROUND_SLOTS) {
      t_components[rounds] = n - edges;
      if (int e = se.read(&t_scan_ms[rounds])) return e;
      t_rounds = rounds + 1;
    }
    if (rounds == 0) result->components_after_first_round = n - edges;
    ++rounds;
  }

  size_t need = l.prim_bytes;
  GHS_HIP_CHECK(rocprim::radix_sort_pairs(base + l.prim, need, (const unsigned long long *)ekey, ekey2, (const uint32_t *)ebits,
                                          ebits2, (size_t)t, 0u, key_end_bit(n), st));
  k_emst_write<<<vgrid(t), EM_BLOCK, 0, st>>>(t, metric, ekey2, ebits2, d_u, d_v, d_w, status);
  GHS_HIP_CHECK(hipGetLastError());
  uint32_t hst[4] = {0};
  GHS_HIP_CHECK(hipMemcpyAsync(hst, status, sizeof(hst), hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipStreamSynchronize(st));
  result->num_edges = edges;
  result->pairs = (uint64_t)rounds * n * (n - 1);
  result->zero_edges = hst[ST_ZEROS];
  result->rounds = rounds;
  result->slices = slices;
  result->query_tiles = query_tiles(n);
  result->ms_total = ms_since(t0);
  return GHS_OK;
}

// Host-buffer form: copy in, run, copy out on the default stream
int ghs_emst_host(uint32_t n, uint32_t dim, const float *x, const float *core2, uint32_t metric, uint32_t *u, uint32_t *v,
                  float *w, ghs_emst_result_t *result) {
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_emst_result_t{};
  uint32_t slices = 0;
  if (int e = check_args(n, dim, x, core2, metric, &slices, u, v, w, false, nullptr, 0)) return e;
  if (n <= 1) return GHS_OK;
  if (int e = ghs::require_device()) return e;
  const size_t ws = ghs_emst_workspace_bytes(n, dim, 0);
  ghs::Staging s;
  const auto i_x = s.take<float>((size_t)n * dim);
  const auto i_c = s.take<float>(core2 ? n : 0);
  const auto o_u = s.take<uint32_t>(n - 1);
  const auto o_v = s.take<uint32_t>(n - 1);
  const auto o_w = s.take<float>(n - 1);
  const auto d_ws = s.take<char>(ws);
  GHS_HIP_CHECK(s.alloc());
  hipStream_t st = nullptr;
  GHS_HIP_CHECK(s.up(i_x, x, st));
  if (core2) GHS_HIP_CHECK(s.up(i_c, core2, st));
  const int rc = ghs_emst_device(n, dim, s.at(i_x), s.at(i_c, core2), metric, 0, s.at(o_u), s.at(o_v), s.at(o_w), s.at(d_ws), ws, st,
                                 result);
  if (rc) return rc;
  GHS_HIP_CHECK(s.down(u, o_u, (size_t)n - 1));
  GHS_HIP_CHECK(s.down(v, o_v, (size_t)n - 1));
  GHS_HIP_CHECK(s.down(w, o_w, (size_t)n - 1));
  return GHS_OK;
}

}  // extern "C"
