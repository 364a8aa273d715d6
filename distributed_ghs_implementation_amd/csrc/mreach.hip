// Core distances and mutual reachability (ABI 10 addition, ghs_mutual_reach_device): per vertex the
// k-th smallest weight among its incident edges (core), per edge max(core[u], core[v], w). The front
// half of HDBSCAN on a canonical edge list; exact on uint32 and byte-identical from run to run: every
// step is an order statistic, a count or a max.
//
// Pipeline (everything on `stream`), after the public ghs_check_canonical (so u < v < n and u ascends):
//   1. rows. The forward row of x is the run of x in u: fwd[x] = lower_bound(u, x), one lane per vertex.
//      The reverse row is the run of x in the weights sorted by v (stable rocPRIM pairs sort, key v,
//      value w, over the bits of n): rev[x] = lower_bound(v sorted, x), the same lane. Row x is the
//      union of the two segments, deg(x) entries; kk = min(k, deg).
//   2. select, by degree:
//        deg <= GHS_MREACH_LANE_ROW_MAX (32)   8 lanes hold the row, 4 values per lane, 8 rows per wave;
//        deg <  GHS_MREACH_BLOCK_ROW_MIN (256) one wave holds the row, 4 values per lane;
//          both: the kk-th value is built from bit 31 down: a ballot per register slot counts the
//          candidates with a 0 there; kk <= that count keeps them, otherwise kk drops by it and the bit
//          is 1. 32 steps whatever k is; nothing is extracted k times.
//        deg <  GHS_MREACH_GRID_ROW_MIN (32768) one workgroup per row: four passes of 8 bits, an LDS
//          histogram of the entries that match the prefix so far, a 256-entry scan picks the digit.
//        otherwise the row joins the grid list: per digit pass every workgroup histograms tiles of
//          every listed row (LDS first, then integer atomicAdd into the row's 256 global counters) and
//          a second small kernel picks the digit per row. No workgroup streams such a row alone.
//      The first kernel does the 8-lane rows itself and lists the others (the lists' order varies from
//      run to run; every row's answer does not depend on it). Their lengths stay on the device.
//   3. re-weight: one streaming pass, 16-byte loads of u, v, w, four edges per lane, core[u] nearly
//      sequential, core[v] a 4-byte gather; counts the raised edges. Skipped when d_w_out is NULL.
// 16-byte loads read whole aligned quads of an array: a quad that ends past m is read entry by entry.
//
// This translation unit includes common.h only and launches only its own kernels.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>

#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"

namespace ghs {
namespace mreach {

constexpr int MR_BLOCK = 256;
constexpr uint32_t MR_LANE_MAX = GHS_MREACH_LANE_ROW_MAX;
constexpr uint32_t MR_BLOCK_MIN = GHS_MREACH_BLOCK_ROW_MIN;
constexpr uint32_t MR_GRID_MIN = GHS_MREACH_GRID_ROW_MIN;
constexpr uint32_t MR_TILE = 4096;  // entries of one grid-row tile: 256 threads x 4 quads
constexpr unsigned MR_GRID_BLOCKS = 1024;
static_assert(MR_LANE_MAX == 8 * 4, "8 lanes x 4 registers");
static_assert(MR_BLOCK_MIN == 64 * 4, "a wave x 4 registers holds every row below the block class");
static_assert(MR_GRID_MIN > MR_BLOCK_MIN && MR_GRID_MIN % MR_TILE == 0, "class boundaries");

// status block: uint32 slots, three uint64 from byte 32
enum { ST_NWAVE = 0, ST_NBLOCK, ST_NGRID, ST_MAXDEG, ST_BAD, ST_SLOTS = 8 };
enum { ST64_SHORT = 4, ST64_ISO, ST64_RAISED };  // index as uint64: bytes 32, 40, 48

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static inline unsigned grid_for(uint64_t items, unsigned per_block = MR_BLOCK, unsigned cap = 2048) {
  uint64_t g = (items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

static inline unsigned key_bits(uint32_t n) {  // keys are < n
  unsigned b = 1;
  while (b < 32 && ((uint64_t)1 << b) < n) ++b;
  return b;
}

// ---- stage 1: row offsets ---------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lower_bound(const uint32_t *__restrict__ a, uint32_t m, uint32_t x) {
  uint32_t lo = 0, hi = m;  // m < 2^31
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// fwd, rev: n + 1 entries each; one lane per vertex, nobody writes a gap alone
__global__ __launch_bounds__(MR_BLOCK) void k_mr_offsets(uint32_t n, uint32_t m, const uint32_t *__restrict__ u,
                                                         const uint32_t *__restrict__ vs, uint32_t *__restrict__ fwd,
                                                         uint32_t *__restrict__ rev) {
  for (uint64_t x = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; x <= n; x += (uint64_t)gridDim.x * blockDim.x) {
    fwd[x] = x == n ? m : lower_bound(u, m, (uint32_t)x);
    rev[x] = x == n ? m : lower_bound(vs, m, (uint32_t)x);
  }
}

// ---- stage 2: select --------------------------------------------------------------------------------------
struct Row {
  uint32_t fo, fd, ro, deg;  // forward offset and length, reverse offset, degree
};

__device__ __forceinline__ Row row_of(uint32_t x, uint32_t m, const uint32_t *__restrict__ fwd,
                                      const uint32_t *__restrict__ rev) {
  const uint32_t fo = fwd[x], fe = fwd[x + 1], ro = rev[x], re = rev[x + 1];
  Row r;
  // lower bounds over sorted arrays ascend and end at m; the clamps keep every later index in range
  r.fo = fo < m ? fo : m;
  r.ro = ro < m ? ro : m;
  r.fd = (fe > r.fo ? (fe < m ? fe : m) : r.fo) - r.fo;
  const uint32_t rd = (re > r.ro ? (re < m ? re : m) : r.ro) - r.ro;
  r.deg = r.fd + rd;  // <= 2 m < 2^32
  return r;
}

// entry i of the row: the forward segment first
__device__ __forceinline__ uint32_t row_entry(const Row &r, uint32_t i, const uint32_t *__restrict__ w,
                                              const uint32_t *__restrict__ wr) {
  return i < r.fd ? w[(size_t)r.fo + i] : wr[(size_t)r.ro + (i - r.fd)];
}

// The kk-th smallest (from 1) of the candidates that the GROUP lanes of a row hold, 4 per lane. Every
// lane of the wave calls it (the ballots are wave-wide); a lane outside any row passes no candidates.
template <int GROUP>
__device__ __forceinline__ uint32_t group_select(const uint32_t (&val)[4], bool (&cand)[4], uint32_t kk, uint32_t gshift) {
  constexpr unsigned long long gmask = GROUP == 64 ? ~0ull : ((1ull << (GROUP & 63)) - 1);
  uint32_t res = 0;
#pragma unroll 1
  for (int bit = 31; bit >= 0; --bit) {
    uint32_t zeros = 0;
    bool one[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      one[j] = (val[j] >> bit) & 1u;
      const unsigned long long b = __ballot(cand[j] && !one[j]);
      zeros += (uint32_t)__popcll((b >> gshift) & gmask);
    }
    const bool take_zero = kk <= zeros;
    if (!take_zero) {
      kk -= zeros;
      res |= 1u << bit;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) cand[j] = cand[j] && (one[j] != take_zero);
  }
  return res;
}

// Every vertex: its degree and class; the 8-lane rows are selected here, the others listed.
__global__ __launch_bounds__(MR_BLOCK) void k_mr_lane_rows(uint32_t n, uint32_t m, uint32_t k, const uint32_t *__restrict__ fwd,
                                                           const uint32_t *__restrict__ rev, const uint32_t *__restrict__ w,
                                                           const uint32_t *__restrict__ wr, uint32_t *__restrict__ core,
                                                           uint32_t *__restrict__ wave_list, uint32_t wave_cap,
                                                           uint32_t *__restrict__ block_list, uint32_t block_cap,
                                                           uint32_t *__restrict__ grid_row, uint32_t *__restrict__ grid_prefix,
                                                           uint32_t *__restrict__ grid_k, uint32_t *__restrict__ ghist,
                                                           uint32_t grid_cap, uint32_t *__restrict__ status) {
  const uint32_t lane = threadIdx.x & 63, gl = lane & 7, gshift = lane & ~7u;
  const uint64_t groups = ((uint64_t)gridDim.x * blockDim.x) >> 3;
  const uint64_t wave_first = ((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 3) - (lane >> 3);
  unsigned long long n_short = 0, n_iso = 0;
  uint32_t max_deg = 0;
  for (uint64_t base = wave_first; base < n; base += groups) {  // wave-uniform trip count
    const uint64_t x = base + (lane >> 3);
    Row r{0, 0, 0, 0};
    if (x < n) r = row_of((uint32_t)x, m, fwd, rev);
    const uint32_t kk = k < r.deg ? k : r.deg;
    if (x < n && gl == 0) {
      n_iso += r.deg == 0;
      n_short += r.deg != 0 && r.deg < k;
      max_deg = r.deg > max_deg ? r.deg : max_deg;
      if (r.deg == 0) core[x] = 0;
    }
    if (x < n && r.deg > MR_LANE_MAX) {
      if (r.deg < MR_BLOCK_MIN) {
        if (gl == 0) {
          const uint32_t pos = atomicAdd(&status[ST_NWAVE], 1u);
          if (pos < wave_cap)
            wave_list[pos] = (uint32_t)x;
          else
            status[ST_BAD] = 1;
        }
      } else if (r.deg < MR_GRID_MIN) {
        if (gl == 0) {
          const uint32_t pos = atomicAdd(&status[ST_NBLOCK], 1u);
          if (pos < block_cap)
            block_list[pos] = (uint32_t)x;
          else
            status[ST_BAD] = 1;
        }
      } else {
        uint32_t pos = 0;
        if (gl == 0) pos = atomicAdd(&status[ST_NGRID], 1u);
        pos = __shfl(pos, (int)gshift);  // the 8 lanes of the row clear its counters
        if (pos < grid_cap) {
          if (gl == 0) {
            grid_row[pos] = (uint32_t)x;
            grid_prefix[pos] = 0;
            grid_k[pos] = kk;
          }
          for (uint32_t i = gl; i < 256; i += 8) ghist[(size_t)pos * 256 + i] = 0;
        } else if (gl == 0) {
          status[ST_BAD] = 1;
        }
      }
    }
    const bool sel = x < n && r.deg >= 1 && r.deg <= MR_LANE_MAX;
    if (!__any(sel)) continue;
    uint32_t val[4];
    bool cand[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t i = gl + 8u * j;
      cand[j] = sel && i < r.deg;
      val[j] = cand[j] ? row_entry(r, i, w, wr) : 0u;
    }
    const uint32_t res = group_select<8>(val, cand, sel ? kk : 0u, gshift);
    if (sel && gl == 0) core[x] = res;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    n_short += __shfl_xor(n_short, s);
    n_iso += __shfl_xor(n_iso, s);
    const uint32_t o = __shfl_xor(max_deg, s);
    max_deg = o > max_deg ? o : max_deg;
  }
  if (lane == 0) {
    unsigned long long *s64 = reinterpret_cast<unsigned long long *>(status);
    if (n_short) atomicAdd(&s64[ST64_SHORT], n_short);
    if (n_iso) atomicAdd(&s64[ST64_ISO], n_iso);
    if (max_deg) atomicMax(&status[ST_MAXDEG], max_deg);
  }
}

// one wave per listed row of 33 .. 255 entries
__global__ __launch_bounds__(MR_BLOCK) void k_mr_wave_rows(uint32_t n, uint32_t m, uint32_t k, const uint32_t *__restrict__ fwd,
                                                           const uint32_t *__restrict__ rev, const uint32_t *__restrict__ w,
                                                           const uint32_t *__restrict__ wr, uint32_t *__restrict__ core,
                                                           const uint32_t *__restrict__ wave_list, uint32_t wave_cap,
                                                           uint32_t *__restrict__ status) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
  const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  uint32_t count = status[ST_NWAVE];
  if (count > wave_cap) count = wave_cap;
  for (uint64_t i = wave; i < count; i += waves) {
    const uint32_t x = wave_list[i];
    if (x >= n) {  // never: the list holds vertices
      if (lane == 0) status[ST_BAD] = 1;
      continue;
    }
    const Row r = row_of(x, m, fwd, rev);
    if (r.deg == 0 || r.deg >= MR_BLOCK_MIN) {  // never: listed by its degree
      if (lane == 0) status[ST_BAD] = 1;
      continue;
    }
    uint32_t val[4];
    bool cand[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t e = lane + 64u * j;
      cand[j] = e < r.deg;
      val[j] = cand[j] ? row_entry(r, e, w, wr) : 0u;
    }
    const uint32_t res = group_select<64>(val, cand, k < r.deg ? k : r.deg, 0u);
    if (lane == 0) core[x] = res;
  }
}

// the aligned quad of a[] that starts at entry q4 (a multiple of 4, < m); entries past m read as 0
__device__ __forceinline__ u32x4 load_quad(const uint32_t *__restrict__ a, uint64_t q4, uint64_t m) {
  if (q4 + 4 <= m) return *reinterpret_cast<const u32x4 *>(a + q4);
  u32x4 x = {0u, 0u, 0u, 0u};
  if (q4 < m) x.x = a[q4];
  if (q4 + 1 < m) x.y = a[q4 + 1];
  if (q4 + 2 < m) x.z = a[q4 + 2];
  return x;
}

// the entries of the quad inside [begin, end) that carry the prefix above the pass's digit: counted
__device__ __forceinline__ void hist_quad(u32x4 q, uint64_t q4, uint64_t begin, uint64_t end, uint32_t prefix, int pass,
                                          uint32_t *s_hist) {
  const int shift = 24 - 8 * pass;
  const uint32_t e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const uint64_t i = q4 + c;
    const bool match = pass == 0 || (e[c] >> (shift + 8)) == (prefix >> (shift + 8));
    if (i >= begin && i < end && match) atomicAdd(&s_hist[(e[c] >> shift) & 255u], 1u);
  }
}

// All 256 threads call it with their bin's count h: the digit d with (count below d) < kk <= (count up
// to d); *rest = kk - (count below d). No such digit (never: 1 <= kk <= the total): 255 and *bad set.
__device__ __forceinline__ uint32_t pick_digit(uint32_t h, uint32_t kk, uint32_t *s_scan, uint32_t *s_pick, uint32_t *rest,
                                               bool *bad) {
  const uint32_t t = threadIdx.x;
  s_scan[t] = h;
  if (t == 0) {
    s_pick[0] = 0xffffffffu;
    s_pick[1] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int d = 1; d < MR_BLOCK; d <<= 1) {
    const uint32_t o = t >= (unsigned)d ? s_scan[t - d] : 0u;
    __syncthreads();
    s_scan[t] += o;
    __syncthreads();
  }
  const uint32_t inc = s_scan[t], below = inc - h;
  if (below < kk && kk <= inc) {  // one bin at most
    s_pick[0] = t;
    s_pick[1] = kk - below;
  }
  __syncthreads();
  uint32_t d = s_pick[0];
  *rest = s_pick[1];
  *bad = d > 255u;
  if (d > 255u) {
    d = 255u;
    *rest = 1;
  }
  __syncthreads();
  return d;
}

// one workgroup per listed row of 256 .. 32767 entries: four passes over the two segments
__global__ __launch_bounds__(MR_BLOCK) void k_mr_block_rows(uint32_t n, uint32_t m, uint32_t k, const uint32_t *__restrict__ fwd,
                                                            const uint32_t *__restrict__ rev, const uint32_t *__restrict__ w,
                                                            const uint32_t *__restrict__ wr, uint32_t *__restrict__ core,
                                                            const uint32_t *__restrict__ block_list, uint32_t block_cap,
                                                            uint32_t *__restrict__ status) {
  __shared__ uint32_t s_hist[MR_BLOCK], s_scan[MR_BLOCK], s_pick[2];
  uint32_t count = status[ST_NBLOCK];
  if (count > block_cap) count = block_cap;
  for (uint32_t b = blockIdx.x; b < count; b += gridDim.x) {
    const uint32_t x = block_list[b];
    if (x >= n) {  // block-uniform; never
      if (threadIdx.x == 0) status[ST_BAD] = 1;
      continue;
    }
    const Row r = row_of(x, m, fwd, rev);
    if (r.deg == 0) {
      if (threadIdx.x == 0) status[ST_BAD] = 1;
      continue;
    }
    uint32_t kk = k < r.deg ? k : r.deg, prefix = 0;
    const uint64_t seg_b[2] = {r.fo, r.ro}, seg_e[2] = {(uint64_t)r.fo + r.fd, (uint64_t)r.ro + (r.deg - r.fd)};
    for (int pass = 0; pass < 4; ++pass) {
      s_hist[threadIdx.x] = 0;
      __syncthreads();
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const uint32_t *a = s ? wr : w;
        for (uint64_t q4 = (seg_b[s] & ~(uint64_t)3) + 4ull * threadIdx.x; q4 < seg_e[s]; q4 += 4ull * MR_BLOCK)
          hist_quad(load_quad(a, q4, m), q4, seg_b[s], seg_e[s], prefix, pass, s_hist);
      }
      __syncthreads();
      uint32_t rest;
      bool bad;
      const uint32_t d = pick_digit(s_hist[threadIdx.x], kk, s_scan, s_pick, &rest, &bad);
      if (bad && threadIdx.x == 0) status[ST_BAD] = 1;
      prefix |= d << (24 - 8 * pass);
      kk = rest;
    }
    if (threadIdx.x == 0) core[x] = prefix;
  }
}

// One digit pass over every grid row: workgroup g takes the tiles g, g + G, ... (rotated by the row's
// place in the list) of both segments of every row. Tiles are aligned to MR_TILE entries of the array.
__global__ __launch_bounds__(MR_BLOCK) void k_mr_grid_hist(int pass, uint32_t n, uint32_t m, const uint32_t *__restrict__ fwd,
                                                           const uint32_t *__restrict__ rev, const uint32_t *__restrict__ w,
                                                           const uint32_t *__restrict__ wr, const uint32_t *__restrict__ grid_row,
                                                           const uint32_t *__restrict__ grid_prefix, uint32_t *__restrict__ ghist,
                                                           uint32_t grid_cap, const uint32_t *__restrict__ status) {
  __shared__ uint32_t s_hist[MR_BLOCK];
  uint32_t count = status[ST_NGRID];
  if (count > grid_cap) count = grid_cap;
  for (uint32_t g = 0; g < count; ++g) {
    const uint32_t x = grid_row[g];
    if (x >= n) continue;  // never; reported by k_mr_grid_pick
    const Row r = row_of(x, m, fwd, rev);
    const uint32_t prefix = grid_prefix[g];
    const uint64_t seg_b[2] = {r.fo, r.ro}, seg_e[2] = {(uint64_t)r.fo + r.fd, (uint64_t)r.ro + (r.deg - r.fd)};
    const uint64_t rot = ((uint64_t)blockIdx.x + g) % gridDim.x;
    uint64_t first[2], last[2];
    bool mine = false;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      first[s] = seg_b[s] / MR_TILE + rot;
      last[s] = seg_e[s] > seg_b[s] ? (seg_e[s] - 1) / MR_TILE : 0;
      mine |= seg_e[s] > seg_b[s] && first[s] <= last[s];
    }
    if (!mine) continue;  // block-uniform
    s_hist[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (seg_e[s] <= seg_b[s]) continue;
      const uint32_t *a = s ? wr : w;
      for (uint64_t t = first[s]; t <= last[s]; t += gridDim.x) {
#pragma unroll
        for (int l = 0; l < 4; ++l) {
          const uint64_t q4 = t * MR_TILE + 4ull * (l * MR_BLOCK + threadIdx.x);
          if (q4 < seg_e[s] && q4 + 4 > seg_b[s]) hist_quad(load_quad(a, q4, m), q4, seg_b[s], seg_e[s], prefix, pass, s_hist);
        }
      }
    }
    __syncthreads();
    const uint32_t h = s_hist[threadIdx.x];
    if (h) atomicAdd(&ghist[(size_t)g * 256 + threadIdx.x], h);
    __syncthreads();
  }
}

// per grid row: the pass's digit out of the row's counters, which are cleared for the next pass
__global__ __launch_bounds__(MR_BLOCK) void k_mr_grid_pick(int pass, uint32_t n, const uint32_t *__restrict__ grid_row,
                                                           uint32_t *__restrict__ grid_prefix, uint32_t *__restrict__ grid_k,
                                                           uint32_t *__restrict__ ghist, uint32_t grid_cap,
                                                           uint32_t *__restrict__ core, uint32_t *__restrict__ status) {
  __shared__ uint32_t s_scan[MR_BLOCK], s_pick[2];
  uint32_t count = status[ST_NGRID];
  if (count > grid_cap) count = grid_cap;
  for (uint32_t g = blockIdx.x; g < count; g += gridDim.x) {
    const uint32_t x = grid_row[g];
    const uint32_t h = ghist[(size_t)g * 256 + threadIdx.x];
    ghist[(size_t)g * 256 + threadIdx.x] = 0;
    const uint32_t kk = grid_k[g], prefix = grid_prefix[g];
    uint32_t rest;
    bool bad;
    const uint32_t d = pick_digit(h, kk, s_scan, s_pick, &rest, &bad);  // its barriers order the reads above
    if (threadIdx.x == 0) {
      const uint32_t p = prefix | (d << (24 - 8 * pass));
      grid_prefix[g] = p;
      grid_k[g] = rest;
      if (bad || x >= n)
        status[ST_BAD] = 1;
      else if (pass == 3)
        core[x] = p;
    }
  }
}

// ---- stage 3: re-weight -----------------------------------------------------------------------------------
// w_out may be w: every lane reads its own four edges before it writes them
GHS_STREAM_KERNEL void k_mr_reweight(uint32_t n, uint64_t m, const uint32_t *__restrict__ u, const uint32_t *__restrict__ v,
                                     const uint32_t *w, const uint32_t *__restrict__ core, uint32_t *w_out,
                                     uint32_t *__restrict__ status) {
  unsigned long long raised = 0;
  for (uint64_t q4 = 4ull * (blockIdx.x * (uint64_t)BLOCK + threadIdx.x); q4 < m; q4 += 4ull * BLOCK * gridDim.x) {
    if (q4 + 4 <= m) {
      const u32x4 a = *reinterpret_cast<const u32x4 *>(u + q4), b = *reinterpret_cast<const u32x4 *>(v + q4);
      const u32x4 x = *reinterpret_cast<const u32x4 *>(w + q4);
      const uint32_t ea[4] = {a.x, a.y, a.z, a.w}, eb[4] = {b.x, b.y, b.z, b.w}, ew[4] = {x.x, x.y, x.z, x.w};
      uint32_t o[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t ca = ea[c] < n ? core[ea[c]] : 0u, cb = eb[c] < n ? core[eb[c]] : 0u;  // < n: validated
        const uint32_t hi = ca > cb ? ca : cb;
        o[c] = hi > ew[c] ? hi : ew[c];
        raised += o[c] > ew[c];
      }
      u32x4 y = {o[0], o[1], o[2], o[3]};
      *reinterpret_cast<u32x4 *>(w_out + q4) = y;
    } else {
      for (uint64_t e = q4; e < m; ++e) {
        const uint32_t a = u[e], b = v[e], x = w[e];
        const uint32_t ca = a < n ? core[a] : 0u, cb = b < n ? core[b] : 0u;
        const uint32_t hi = ca > cb ? ca : cb, o = hi > x ? hi : x;
        raised += o > x;
        w_out[e] = o;
      }
    }
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) raised += __shfl_xor(raised, s);
  if ((threadIdx.x & 63) == 0 && raised) atomicAdd(reinterpret_cast<unsigned long long *>(status) + ST64_RAISED, raised);
}

// ---- workspace ---------------------------------------------------------------------------------------------
//   per vertex 8 B: the forward and the reverse offsets (n + 1 entries each);
//   per edge   8 B: v sorted and w in that order;
//   the lists: a wave row has > 32 of the 2 m edge ends, a block row >= 256, a grid row >= 32768 (and
//   12 B of state + 1 KiB of counters each);
//   rocPRIM's sort storage, 1 KiB of status.
struct Layout {
  size_t fwd, rev, vs, wr, wave_list, block_list, grid_row, grid_prefix, grid_k, ghist;
  uint64_t wave_cap, block_cap, grid_cap;
  size_t prim, prim_bytes, status, total;
};

static size_t sort_bytes(uint64_t m) {
  size_t b = 0;
  if (m == 0) return 0;
  (void)rocprim::radix_sort_pairs(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr,
                                  (uint32_t *)nullptr, (size_t)m, 0u, 32u);
  return b;
}

static inline uint64_t rows_cap(uint32_t n, uint64_t m, uint64_t min_deg) {
  const uint64_t c = 2 * m / min_deg;
  return (c < n ? c : n) + 1;
}

static Layout layout(uint32_t n, uint64_t m) {
  Layout l{};
  size_t o = 0;
  auto take = [&o](size_t bytes) {
    const size_t at = o;
    o += align256(bytes);
    return at;
  };
  l.fwd = take(((size_t)n + 1) * 4);
  l.rev = take(((size_t)n + 1) * 4);
  l.vs = take((size_t)m * 4);
  l.wr = take((size_t)m * 4);
  l.wave_cap = rows_cap(n, m, MR_LANE_MAX + 1);
  l.block_cap = rows_cap(n, m, MR_BLOCK_MIN);
  l.grid_cap = rows_cap(n, m, MR_GRID_MIN);
  l.wave_list = take((size_t)l.wave_cap * 4);
  l.block_list = take((size_t)l.block_cap * 4);
  l.grid_row = take((size_t)l.grid_cap * 4);
  l.grid_prefix = take((size_t)l.grid_cap * 4);
  l.grid_k = take((size_t)l.grid_cap * 4);
  l.ghist = take((size_t)l.grid_cap * 1024);
  l.prim_bytes = align256(sort_bytes(m)) + 65536;
  l.prim = take(l.prim_bytes);
  l.status = take(1024);
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

// everything that needs no device, in the order the header lists it (ws: the device form's workspace)
static int check_args(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w, uint32_t k,
                      const uint32_t *core, const uint32_t *w_out, bool device_form, const void *ws, size_t ws_bytes) {
  if (k == 0) GHS_FAIL(GHS_E_ARG, "k (min_samples) must be >= 1");
  if (m >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "m must be < 2^31");
  if (n == 0) return GHS_OK;
  if (!core) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if ((uintptr_t)core & 3) GHS_FAIL(GHS_E_ARG, "core must be 4-byte aligned");
  if (m == 0) return GHS_OK;
  if (!u || !v || !w || (device_form && !ws)) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if (device_form && (((uintptr_t)u | (uintptr_t)v | (uintptr_t)w | (uintptr_t)w_out | (uintptr_t)ws) & 15))
    GHS_FAIL(GHS_E_ARG, "u, v, w, w_out and the workspace must be 16-byte aligned");
  const size_t mb = (size_t)m * 4, nb = (size_t)n * 4;
  if (w_out && w_out != w && overlap(w_out, mb, w, mb))
    GHS_FAIL(GHS_E_ARG, "w_out overlaps w without being equal to it");
  if (overlap(w_out, mb, u, mb) || overlap(w_out, mb, v, mb) || overlap(w_out, mb, core, nb))
    GHS_FAIL(GHS_E_ARG, "w_out overlaps u, v or core");
  if (overlap(core, nb, u, mb) || overlap(core, nb, v, mb) || overlap(core, nb, w, mb))
    GHS_FAIL(GHS_E_ARG, "core overlaps an input");
  if (device_form && ws_bytes < layout(n, m).total) GHS_FAIL(GHS_E_NOMEM, "workspace too small");
  return GHS_OK;
}

// opt-in HIP-event times of the last call's stages on this thread (ghs_mutual_reach_phases)
thread_local bool t_phases_on = false;
thread_local double t_phase_ms[3] = {0, 0, 0};  // rows, select, re-weight

struct PhaseEvents {
  hipEvent_t ev[4] = {};
  int made = 0;
  bool on = false;
  int start(bool enable) {
    on = enable;
    if (!on) return GHS_OK;
    for (; made < 4; ++made) GHS_HIP_CHECK(hipEventCreate(&ev[made]));
    return GHS_OK;
  }
  int mark(int k, hipStream_t st) {
    if (on) GHS_HIP_CHECK(hipEventRecord(ev[k], st));
    return GHS_OK;
  }
  int read(double *ms) {
    if (!on) return GHS_OK;
    for (int k = 0; k < 3; ++k) {
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

}  // namespace mreach
}  // namespace ghs

using namespace ghs;
using namespace ghs::mreach;

extern "C" {

size_t ghs_mutual_reach_workspace_bytes(uint32_t n, uint64_t m) {
  if (n == 0 || m == 0 || m >= (1ull << 31)) return 0;
  return layout(n, m).total;
}

int ghs_mutual_reach_phases(int enable, double *ms) {
  if (ms)
    for (int k = 0; k < 3; ++k) ms[k] = t_phase_ms[k];
  t_phases_on = enable != 0;
  return GHS_OK;
}

int ghs_mutual_reach_device(uint32_t n, uint64_t m64, const uint32_t *d_u, const uint32_t *d_v, const uint32_t *d_w, uint32_t k,
                            uint32_t *d_core, uint32_t *d_w_out, void *d_workspace, size_t workspace_bytes, void *stream,
                            ghs_mreach_result_t *result) {
  hipStream_t st = (hipStream_t)stream;
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_mreach_result_t{};
  if (int e = check_args(n, m64, d_u, d_v, d_w, k, d_core, d_w_out, true, d_workspace, workspace_bytes)) return e;
  if (n == 0) return GHS_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");

  const auto t0 = std::chrono::steady_clock::now();
  if (m64 == 0) {
    GHS_HIP_CHECK(hipMemsetAsync(d_core, 0, (size_t)n * 4, st));
    GHS_HIP_CHECK(hipStreamSynchronize(st));
    result->isolated = n;
    result->ms_total = ms_since(t0);
    return GHS_OK;
  }
  int canon = 0;
  const int rc = ghs_check_canonical(n, m64, d_u, d_v, stream, &canon);
  if (rc != GHS_OK) return rc;
  if (!canon) GHS_FAIL(GHS_E_NONCANON, "edge list is not canonical");

  const uint32_t m = (uint32_t)m64;  // < 2^31
  const Layout l = layout(n, m64);
  char *base = (char *)d_workspace;
  uint32_t *fwd = (uint32_t *)(base + l.fwd), *rev = (uint32_t *)(base + l.rev);
  uint32_t *vs = (uint32_t *)(base + l.vs), *wr = (uint32_t *)(base + l.wr);
  uint32_t *wave_list = (uint32_t *)(base + l.wave_list), *block_list = (uint32_t *)(base + l.block_list);
  uint32_t *grid_row = (uint32_t *)(base + l.grid_row), *grid_prefix = (uint32_t *)(base + l.grid_prefix);
  uint32_t *grid_k = (uint32_t *)(base + l.grid_k), *ghist = (uint32_t *)(base + l.ghist);
  uint32_t *status = (uint32_t *)(base + l.status);
  const uint32_t wave_cap = (uint32_t)l.wave_cap, block_cap = (uint32_t)l.block_cap, grid_cap = (uint32_t)l.grid_cap;
  PhaseEvents pe;
  if (int e = pe.start(t_phases_on)) return e;
  GHS_HIP_CHECK(hipMemsetAsync(status, 0, 1024, st));
  if (int e = pe.mark(0, st)) return e;

  // stage 1
  size_t need = 0;
  (void)rocprim::radix_sort_pairs(nullptr, need, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr,
                                  (uint32_t *)nullptr, (size_t)m, 0u, key_bits(n));
  if (need > l.prim_bytes) GHS_FAIL(GHS_E_STATE, "mreach: the sort needs more storage than the workspace holds");
  GHS_HIP_CHECK(rocprim::radix_sort_pairs(base + l.prim, need, d_v, vs, d_w, wr, (size_t)m, 0u, key_bits(n), st));
  k_mr_offsets<<<grid_for((uint64_t)n + 1), MR_BLOCK, 0, st>>>(n, m, d_u, vs, fwd, rev);
  GHS_HIP_CHECK(hipGetLastError());
  if (int e = pe.mark(1, st)) return e;

  // stage 2: the lists' lengths stay on the device; an empty class costs an empty launch
  k_mr_lane_rows<<<grid_for((uint64_t)n * 8), MR_BLOCK, 0, st>>>(n, m, k, fwd, rev, d_w, wr, d_core, wave_list, wave_cap,
                                                                 block_list, block_cap, grid_row, grid_prefix, grid_k, ghist,
                                                                 grid_cap, status);
  k_mr_wave_rows<<<grid_for((uint64_t)wave_cap * 64), MR_BLOCK, 0, st>>>(n, m, k, fwd, rev, d_w, wr, d_core, wave_list,
                                                                         wave_cap, status);
  k_mr_block_rows<<<grid_for(block_cap, 1), MR_BLOCK, 0, st>>>(n, m, k, fwd, rev, d_w, wr, d_core, block_list, block_cap,
                                                               status);
  GHS_HIP_CHECK(hipGetLastError());
  for (int pass = 0; pass < 4; ++pass) {
    k_mr_grid_hist<<<MR_GRID_BLOCKS, MR_BLOCK, 0, st>>>(pass, n, m, fwd, rev, d_w, wr, grid_row, grid_prefix, ghist, grid_cap,
                                                        status);
    k_mr_grid_pick<<<grid_for(grid_cap, 1, 1024), MR_BLOCK, 0, st>>>(pass, n, grid_row, grid_prefix, grid_k, ghist, grid_cap,
                                                                     d_core, status);
  }
  GHS_HIP_CHECK(hipGetLastError());
  if (int e = pe.mark(2, st)) return e;

  // stage 3
  if (d_w_out) {
    k_mr_reweight<<<grid_for((m64 + 3) / 4, BLOCK), BLOCK, 0, st>>>(n, m64, d_u, d_v, d_w, d_core, d_w_out, status);
    GHS_HIP_CHECK(hipGetLastError());
  }
  if (int e = pe.mark(3, st)) return e;
  uint32_t hst[16] = {0};
  GHS_HIP_CHECK(hipMemcpyAsync(hst, status, sizeof(hst), hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipStreamSynchronize(st));
  if (int e = pe.read(t_phase_ms)) return e;
  if (hst[ST_BAD]) GHS_FAIL(GHS_E_STATE, "mreach: a row left its class or a digit its range (internal error)");
  uint64_t h64[3];
  memcpy(h64, hst + 2 * ST64_SHORT, sizeof(h64));
  result->short_rows = h64[0];
  result->isolated = h64[1];
  result->raised_edges = h64[2];
  result->max_degree = hst[ST_MAXDEG];
  result->block_rows = hst[ST_NBLOCK];
  result->grid_rows = hst[ST_NGRID];
  result->ms_total = ms_since(t0);
  return GHS_OK;
}

// Host-buffer form: copy in, run, copy out on the default stream
int ghs_mutual_reach_host(uint32_t n, uint64_t m, const uint32_t *u, const uint32_t *v, const uint32_t *w, uint32_t k,
                          uint32_t *core, uint32_t *w_out, ghs_mreach_result_t *result) {
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_mreach_result_t{};
  if (int e = check_args(n, m, u, v, w, k, core, w_out, false, nullptr, 0)) return e;
  if (n == 0) return GHS_OK;
  if (int e = ghs::require_device()) return e;
  const size_t ws = ghs_mutual_reach_workspace_bytes(n, m);
  ghs::Staging s;
  const auto i_u = s.take<uint32_t>(m), i_v = s.take<uint32_t>(m), i_w = s.take<uint32_t>(m);
  const auto o_core = s.take<uint32_t>(n), o_w = s.take<uint32_t>(m);
  const auto d_ws = s.take<char>(ws);
  GHS_HIP_CHECK(s.alloc());
  hipStream_t st = nullptr;
  GHS_HIP_CHECK(s.up(i_u, u, st));
  GHS_HIP_CHECK(s.up(i_v, v, st));
  GHS_HIP_CHECK(s.up(i_w, w, st));
  const int rc = ghs_mutual_reach_device(n, m, s.at(i_u), s.at(i_v), s.at(i_w), k, s.at(o_core), s.at(o_w, w_out), s.at(d_ws),
                                         ws, st, result);
  if (rc) return rc;
  GHS_HIP_CHECK(s.down(core, o_core, n));
  GHS_HIP_CHECK(s.down(w_out, o_w, m));
  return GHS_OK;
}

}  // extern "C"
