// Ingest: the synthetic generators of BASELINE.json configs 3-5 (R-MAT s24/s26, 2D grid 16k^2)
// and the device-side canonicity check. A generator's output is the canonical edge list of
// include/ghs_mst.h (u < v, ascending (u, v), unique) — the device form of the reference's
// graph files (create_graph_files.py:43-89 writes every undirected edge once in
// graph_metadata.json). The reference's generator is networkx's seeded ER G(n, p)
// (create_graph_files.py:13-40); R-MAT and grids are the BASELINE scales it cannot reach. The
// canonical sort/dedupe is a rocPRIM radix sort of 64-bit (min << scale | max) keys, then a
// two-pass unique + decode (k_uniq_*). ghs_canonicalize_device is the general form of that stage for
// a caller's raw edge list (k_canon_*: the nx.Graph construction every reference entry point starts
// with, ghs_implementation.py:425-426, on the device). ghs_weight_ranks_device (k_weight_keys,
// k_rank_*) comes in front of it for float / 64-bit weights: nx.Graph takes any comparable weight,
// the engine uint32, and the dense rank among the distinct values is an order- and tie-preserving map.
// The CPU restatement of both generators (test infrastructure) is oracle/generators.c.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/device/device_reduce.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <mutex>
#include <unordered_map>

#include <string>

#include "common.h"

namespace ghs {

static inline unsigned grid_cap(uint64_t items, unsigned per_block, unsigned cap) {
  uint64_t g = (items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// canonical check: u < v < n and (u, v) strictly ascending
__global__ void k_check_canonical(uint32_t n, uint64_t m, const uint32_t *__restrict__ u, const uint32_t *__restrict__ v,
                                  unsigned int *__restrict__ bad) {
  for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t a = u[e], b = v[e];
    bool ok = a < b && b < n;
    if (ok && e > 0) {
      const uint32_t pa = u[e - 1], pb = v[e - 1];
      ok = (pa < a) || (pa == a && pb < b);
    }
    if (!ok) atomicOr(bad, 1u);
  }
}

// CSR row offsets of a canonical list (ABI 9, ghs_csr_offsets): off[r] = the first edge of row r.
// Edge e writes the offsets of the rows (u[e - 1], u[e]] (every row from 0 for e = 0, up to n for
// e = m): each row's entry is written exactly once, by the edge that starts it or by the first
// edge past it when it is empty. u ascending is required (the solve validates the offsets).
__global__ void k_csr_offsets(uint32_t n, uint64_t m, const uint32_t *__restrict__ u, uint32_t *__restrict__ off) {
  for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e <= m; e += (uint64_t)gridDim.x * blockDim.x) {
    const int64_t lo = e == 0 ? -1 : (int64_t)u[e - 1];
    const int64_t hi = e == m ? (int64_t)n : (int64_t)min(u[e], n);
    for (int64_t r = lo + 1; r <= hi; ++r) off[r] = (uint32_t)e;
  }
}

// ---- R-MAT ---------------------------------------------------------------------------------
// Graph500 quadrant probabilities as exact integer thresholds on a uniform 32-bit draw.
constexpr uint32_t RMAT_TA = (uint32_t)((57ull << 32) / 100);
constexpr uint32_t RMAT_TAB = (uint32_t)((76ull << 32) / 100);
constexpr uint32_t RMAT_TABC = (uint32_t)((95ull << 32) / 100);

__host__ __device__ __forceinline__ uint32_t rmat_perm(uint32_t x, uint32_t scale, uint64_t seed) {
  // bijection on [0, 2^scale): odd multiply, xorshift, odd multiply, xor constant (all mod 2^scale)
  const uint32_t mask = (scale >= 32) ? 0xffffffffu : ((1u << scale) - 1u);
  const uint32_t c1 = (uint32_t)splitmix64(seed ^ 0x1111) | 1u;
  const uint32_t c2 = (uint32_t)splitmix64(seed ^ 0x2222) | 1u;
  const uint32_t c3 = (uint32_t)splitmix64(seed ^ 0x3333);
  x = (x * c1) & mask;
  x ^= x >> ((scale + 1) / 2);
  x = (x * c2) & mask;
  x ^= x >> ((scale + 2) / 3);
  return (x ^ c3) & mask;
}

// tuple t -> packed canonical key (min << scale | max), or all-ones (2*scale bits) for a self-loop
__host__ __device__ __forceinline__ uint64_t rmat_tuple(uint64_t t, uint32_t scale, uint64_t seed) {
  uint64_t state = splitmix64(seed ^ splitmix64(t + 0x5bd1e995ull));
  uint32_t uu = 0, vv = 0;
  uint64_t bits = 0;
  for (uint32_t l = 0; l < scale; ++l) {
    if ((l & 1) == 0) {
      state += 0x9e3779b97f4a7c15ull;
      bits = splitmix64(state);
    }
    const uint32_t r = (l & 1) ? (uint32_t)(bits >> 32) : (uint32_t)bits;
    const uint32_t bu = r >= RMAT_TAB ? 1u : 0u;
    const uint32_t bv = (r >= RMAT_TA && r < RMAT_TAB) || r >= RMAT_TABC ? 1u : 0u;
    uu = (uu << 1) | bu;
    vv = (vv << 1) | bv;
  }
  uu = rmat_perm(uu, scale, seed);
  vv = rmat_perm(vv, scale, seed);
  if (uu == vv) return (scale >= 32) ? ~0ull : ((1ull << (2 * scale)) - 1ull);
  const uint32_t a = uu < vv ? uu : vv, b = uu < vv ? vv : uu;
  return ((uint64_t)a << scale) | b;
}

__global__ void k_rmat_tuples(uint64_t T, uint32_t scale, uint64_t seed, uint64_t *__restrict__ keys) {
  for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < T; t += (uint64_t)gridDim.x * blockDim.x)
    keys[t] = rmat_tuple(t, scale, seed);
}

// Unique + decode of the sorted keys in two passes over them (rocPRIM's unique, a partition
// over 2 GB of keys at s24, took 8 ms; these are streaming passes): a key is kept when it differs
// from its predecessor and is not the self-loop marker (which sorts last). Pass 1 counts the kept
// keys per tile, one block scans the tile counts, pass 2 writes each kept key's (u, v, w) at its
// rank — the weight hashes the output position, as the canonical list's edge id.
constexpr int UQ_BLOCK = 256;
constexpr int UQ_ROWS = 16;  // a tile is UQ_ROWS rows of UQ_BLOCK consecutive keys
constexpr uint64_t UQ_TILE = (uint64_t)UQ_BLOCK * UQ_ROWS;

__device__ __forceinline__ bool uq_keep(const uint64_t *__restrict__ keys, uint64_t i, uint64_t T, uint64_t marker,
                                        uint64_t *k_out) {
  if (i >= T) return false;
  const uint64_t k = keys[i];
  *k_out = k;
  return k != marker && (i == 0 || keys[i - 1] != k);
}

__global__ __launch_bounds__(UQ_BLOCK) void k_uniq_count(const uint64_t *__restrict__ keys, uint64_t T, uint64_t marker,
                                                         uint32_t *__restrict__ tile_cnt) {
  __shared__ uint32_t s_w[UQ_BLOCK / 64];
  const uint64_t base = blockIdx.x * UQ_TILE;
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < UQ_ROWS; ++j) {
    uint64_t k;
    c += uq_keep(keys, base + (uint64_t)j * UQ_BLOCK + threadIdx.x, T, marker, &k) ? 1u : 0u;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x / 64] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < UQ_BLOCK / 64; ++w) t += s_w[w];
    tile_cnt[blockIdx.x] = t;
  }
}

// exclusive scan of the tile counts in place (one block of 1024), total to *total
__global__ __launch_bounds__(1024) void k_uniq_scan(uint32_t *__restrict__ cnt, uint32_t ntiles,
                                                    uint64_t *__restrict__ total) {
  __shared__ uint32_t s_part[1024];
  const uint32_t per = (ntiles + 1023) / 1024;
  const uint32_t b = threadIdx.x * per;
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

__global__ __launch_bounds__(UQ_BLOCK) void k_uniq_write(const uint64_t *__restrict__ keys, uint64_t T, uint64_t marker,
                                                         const uint32_t *__restrict__ tile_off, uint32_t scale,
                                                         uint64_t wseed, uint32_t *__restrict__ u,
                                                         uint32_t *__restrict__ v, uint32_t *__restrict__ w) {
  __shared__ uint32_t s_cnt[UQ_ROWS][UQ_BLOCK / 64];
  const uint64_t base = blockIdx.x * UQ_TILE;
  const int lane = threadIdx.x & 63, wid = threadIdx.x / 64;
  const uint64_t lt = (1ull << lane) - 1ull;
  uint64_t kk[UQ_ROWS];
  uint64_t masks[UQ_ROWS];
#pragma unroll
  for (int j = 0; j < UQ_ROWS; ++j) {
    const bool keep = uq_keep(keys, base + (uint64_t)j * UQ_BLOCK + threadIdx.x, T, marker, &kk[j]);
    masks[j] = __ballot(keep);
    if (lane == 0) s_cnt[j][wid] = (uint32_t)__popcll(masks[j]);
  }
  __syncthreads();
  const uint64_t vmask = (1ull << scale) - 1ull;
  uint32_t row_base = tile_off[blockIdx.x];
#pragma unroll
  for (int j = 0; j < UQ_ROWS; ++j) {
    uint32_t before = 0, row = 0;
#pragma unroll
    for (int x = 0; x < UQ_BLOCK / 64; ++x) {
      const uint32_t c = s_cnt[j][x];
      before += x < wid ? c : 0u;
      row += c;
    }
    if ((masks[j] >> lane) & 1ull) {
      const uint32_t o = row_base + before + (uint32_t)__popcll(masks[j] & lt);
      u[o] = (uint32_t)(kk[j] >> scale);
      v[o] = (uint32_t)(kk[j] & vmask);
      w[o] = mix32(o ^ (uint32_t)wseed);
    }
    row_base += row;
  }
}

// ---- canonicalize (ABI 10 addition, ghs_canonicalize_device) ---------------------------------
// The general form of the stage above for a caller's raw edge list: any n, the caller's weights,
// nx.Graph "last write wins" for a repeated pair, range validation, and the raw index of the
// surviving occurrence. Pass 1 (k_canon_keys) packs (min << bits | max) keys with the raw index as
// the value; a self-loop and an edge with an endpoint >= n both become the marker (all ones over
// 2 * bits bits: the pair (2^bits - 1, 2^bits - 1), itself a self-loop, so no real edge has it), the
// latter also raising the error flag. rocPRIM's pairs sort is stable, so a run of equal keys keeps
// ascending raw index and its LAST entry is the occurrence nx.Graph would keep: the compaction
// (k_canon_count / k_uniq_scan / k_canon_write) keeps an entry that differs from its successor.
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint64_t canon_key(uint32_t a, uint32_t b, uint32_t n, uint32_t bits, uint64_t marker,
                                              bool *bad) {
  if (a >= n || b >= n) {
    *bad = true;
    return marker;
  }
  if (a == b) return marker;
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
  return ((uint64_t)lo << bits) | hi;
}

// Elements [head, head + 4 * nquads) are read as 16-byte vectors (the host picks head so that both
// ru + head and rv + head are 16-byte aligned, or nquads = 0 when no such head exists); the other
// nscalar elements — the first `head` and the tail past the quads — one by one. keys / vals are
// 256-byte aligned, so with head = 0 (the aligned caller) the stores are 16-byte vectors too.
__global__ __launch_bounds__(BLOCK) void k_canon_keys(uint32_t n, uint32_t bits, uint64_t marker, uint64_t head,
                                                      uint64_t nquads, uint64_t nscalar,
                                                      const uint32_t *__restrict__ ru, const uint32_t *__restrict__ rv,
                                                      uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                      unsigned int *__restrict__ err) {
  const uint64_t gid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (uint64_t q = gid; q < nquads; q += stride) {
    const uint64_t i = head + 4 * q;
    const u32x4 a = *reinterpret_cast<const u32x4 *>(ru + i);
    const u32x4 b = *reinterpret_cast<const u32x4 *>(rv + i);
    const uint64_t k0 = canon_key(a.x, b.x, n, bits, marker, &bad);
    const uint64_t k1 = canon_key(a.y, b.y, n, bits, marker, &bad);
    const uint64_t k2 = canon_key(a.z, b.z, n, bits, marker, &bad);
    const uint64_t k3 = canon_key(a.w, b.w, n, bits, marker, &bad);
    const uint32_t i0 = (uint32_t)i;
    if (head == 0) {
      u64x2 lo, hi;
      lo.x = k0; lo.y = k1; hi.x = k2; hi.y = k3;
      u32x4 iv;
      iv.x = i0; iv.y = i0 + 1; iv.z = i0 + 2; iv.w = i0 + 3;
      *reinterpret_cast<u64x2 *>(keys + i) = lo;
      *reinterpret_cast<u64x2 *>(keys + i + 2) = hi;
      *reinterpret_cast<u32x4 *>(vals + i) = iv;
    } else {
      keys[i] = k0; keys[i + 1] = k1; keys[i + 2] = k2; keys[i + 3] = k3;
      vals[i] = i0; vals[i + 1] = i0 + 1; vals[i + 2] = i0 + 2; vals[i + 3] = i0 + 3;
    }
  }
  for (uint64_t s = gid; s < nscalar; s += stride) {
    const uint64_t i = s < head ? s : 4 * nquads + s;
    keys[i] = canon_key(ru[i], rv[i], n, bits, marker, &bad);
    vals[i] = (uint32_t)i;
  }
  if (bad) atomicOr(err, 1u);
}

// a sorted entry survives when it is not the marker and its successor (read across lane, wave,
// block and tile boundaries alike: it is the next array element) has another key
__device__ __forceinline__ bool cn_keep(const uint64_t *__restrict__ keys, uint64_t i, uint64_t T, uint64_t marker,
                                        uint64_t *k_out) {
  if (i >= T) return false;
  const uint64_t k = keys[i];
  *k_out = k;
  return k != marker && (i + 1 == T || keys[i + 1] != k);
}

__global__ __launch_bounds__(UQ_BLOCK) void k_canon_count(const uint64_t *__restrict__ keys, uint64_t T,
                                                          uint64_t marker, uint32_t *__restrict__ tile_cnt) {
  __shared__ uint32_t s_w[UQ_BLOCK / 64];
  const uint64_t base = blockIdx.x * UQ_TILE;
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < UQ_ROWS; ++j) {
    uint64_t k;
    c += cn_keep(keys, base + (uint64_t)j * UQ_BLOCK + threadIdx.x, T, marker, &k) ? 1u : 0u;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x / 64] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < UQ_BLOCK / 64; ++w) t += s_w[w];
    tile_cnt[blockIdx.x] = t;
  }
}

// each survivor, at its rank: (u, v) decoded from the key, src = its raw index (the sorted value),
// w = rw[src] — a gather, for survivors only. src may be NULL.
__global__ __launch_bounds__(UQ_BLOCK) void k_canon_write(const uint64_t *__restrict__ keys,
                                                          const uint32_t *__restrict__ vals, uint64_t T,
                                                          uint64_t marker, const uint32_t *__restrict__ tile_off,
                                                          uint32_t bits, const uint32_t *__restrict__ rw,
                                                          uint32_t *__restrict__ u, uint32_t *__restrict__ v,
                                                          uint32_t *__restrict__ w, uint32_t *__restrict__ src) {
  __shared__ uint32_t s_cnt[UQ_ROWS][UQ_BLOCK / 64];
  const uint64_t base = blockIdx.x * UQ_TILE;
  const int lane = threadIdx.x & 63, wid = threadIdx.x / 64;
  const uint64_t lt = (1ull << lane) - 1ull;
  uint64_t kk[UQ_ROWS];
  uint64_t masks[UQ_ROWS];
#pragma unroll
  for (int j = 0; j < UQ_ROWS; ++j) {
    const bool keep = cn_keep(keys, base + (uint64_t)j * UQ_BLOCK + threadIdx.x, T, marker, &kk[j]);
    masks[j] = __ballot(keep);
    if (lane == 0) s_cnt[j][wid] = (uint32_t)__popcll(masks[j]);
  }
  __syncthreads();
  const uint64_t vmask = (1ull << bits) - 1ull;  // bits <= 32
  uint32_t row_base = tile_off[blockIdx.x];
#pragma unroll
  for (int j = 0; j < UQ_ROWS; ++j) {
    uint32_t before = 0, row = 0;
#pragma unroll
    for (int x = 0; x < UQ_BLOCK / 64; ++x) {
      const uint32_t c = s_cnt[j][x];
      before += x < wid ? c : 0u;
      row += c;
    }
    if ((masks[j] >> lane) & 1ull) {
      const uint32_t o = row_base + before + (uint32_t)__popcll(masks[j] & lt);
      const uint32_t r = vals[base + (uint64_t)j * UQ_BLOCK + threadIdx.x];
      u[o] = (uint32_t)(kk[j] >> bits);
      v[o] = (uint32_t)(kk[j] & vmask);
      w[o] = rw[r];
      if (src) src[o] = r;
    }
    row_base += row;
  }
}

static inline uint32_t canon_bits(uint32_t n) {
  uint32_t bits = 1;
  while (bits < 32 && (1ull << bits) < n) ++bits;
  return bits;
}

// ---- weight ranks (ABI 10 addition, ghs_weight_ranks_device) ---------------------------------
// The device form of graph._as_weight_array's np.searchsorted(np.unique(w), w): the solver's key is
// (w, eid), so any order-preserving map of the weights that keeps ties tied gives the same flags,
// and float / 64-bit weights reach the uint32 engine as their dense rank among the distinct values.
// Pass 1 (k_weight_keys) maps every weight to an unsigned key that orders as the value does, with the
// element's index as the sort's value; a pairs sort (no stability needed: equal keys get equal
// ranks); then head flags over the sorted keys (a key that differs from its predecessor opens a new
// rank) in the tile shape of the compaction above — but here EVERY element writes: its rank is the
// number of heads up to and including it, minus one, scattered to ranks[index].
template <uint32_t WT>
struct WeightKey;
template <>
struct WeightKey<GHS_W_FLOAT32> {
  typedef uint32_t key_t;
  static __device__ __forceinline__ key_t key(key_t b, bool *nan) {
    const key_t sign = 0x80000000u, mag = b & ~sign;
    if (mag > 0x7f800000u) *nan = true;
    if (mag == 0) b = 0;  // -0.0 == +0.0
    return (b & sign) ? ~b : (b | sign);
  }
};
template <>
struct WeightKey<GHS_W_FLOAT64> {
  typedef uint64_t key_t;
  static __device__ __forceinline__ key_t key(key_t b, bool *nan) {
    const key_t sign = 1ull << 63, mag = b & ~sign;
    if (mag > 0x7ff0000000000000ull) *nan = true;
    if (mag == 0) b = 0;
    return (b & sign) ? ~b : (b | sign);
  }
};
template <>
struct WeightKey<GHS_W_INT64> {
  typedef uint64_t key_t;
  static __device__ __forceinline__ key_t key(key_t b, bool *) { return b ^ (1ull << 63); }
};
template <>
struct WeightKey<GHS_W_UINT64> {
  typedef uint64_t key_t;
  static __device__ __forceinline__ key_t key(key_t b, bool *) { return b; }
};

// Elements [head, head + VEC * nvec) are read as 16-byte vectors (VEC = 4 or 2 elements; the host
// picks head so that w + head is 16-byte aligned), the other nscalar elements one by one. keys /
// vals are 256-byte aligned, so with head = 0 the key stores are 16-byte vectors too.
template <uint32_t WT>
__global__ __launch_bounds__(BLOCK) void k_weight_keys(uint64_t head, uint64_t nvec, uint64_t nscalar,
                                                       const typename WeightKey<WT>::key_t *__restrict__ w,
                                                       typename WeightKey<WT>::key_t *__restrict__ keys,
                                                       uint32_t *__restrict__ vals, unsigned int *__restrict__ err) {
  typedef typename WeightKey<WT>::key_t K;
  constexpr int VEC = 16 / sizeof(K);
  typedef K kvec __attribute__((ext_vector_type(VEC)));
  typedef uint32_t ivec __attribute__((ext_vector_type(VEC)));
  const uint64_t gid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool nan = false;
  for (uint64_t q = gid; q < nvec; q += stride) {
    const uint64_t i = head + VEC * q;
    const kvec b = *reinterpret_cast<const kvec *>(w + i);
    kvec k;
#pragma unroll
    for (int x = 0; x < VEC; ++x) k[x] = WeightKey<WT>::key(b[x], &nan);
    ivec iv;
#pragma unroll
    for (int x = 0; x < VEC; ++x) iv[x] = (uint32_t)(i + x);
    if (head == 0) {
      *reinterpret_cast<kvec *>(keys + i) = k;
      *reinterpret_cast<ivec *>(vals + i) = iv;
    } else {
#pragma unroll
      for (int x = 0; x < VEC; ++x) {
        keys[i + x] = k[x];
        vals[i + x] = iv[x];
      }
    }
  }
  for (uint64_t s = gid; s < nscalar; s += stride) {
    const uint64_t i = s < head ? s : VEC * nvec + s;
    keys[i] = WeightKey<WT>::key(w[i], &nan);
    vals[i] = (uint32_t)i;
  }
  if (nan) atomicOr(err, 1u);
}

// a sorted entry opens a new rank when it is the first or differs from its predecessor (read across
// lane, wave, block and tile boundaries alike: it is the previous array element)
template <typename K>
__device__ __forceinline__ bool wr_head(const K *__restrict__ keys, uint64_t i, uint64_t T) {
  if (i >= T) return false;
  return i == 0 || keys[i - 1] != keys[i];
}

template <typename K>
__global__ __launch_bounds__(UQ_BLOCK) void k_rank_count(const K *__restrict__ keys, uint64_t T,
                                                         uint32_t *__restrict__ tile_cnt) {
  __shared__ uint32_t s_w[UQ_BLOCK / 64];
  const uint64_t base = blockIdx.x * UQ_TILE;
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < UQ_ROWS; ++j) c += wr_head(keys, base + (uint64_t)j * UQ_BLOCK + threadIdx.x, T) ? 1u : 0u;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x / 64] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < UQ_BLOCK / 64; ++w) t += s_w[w];
    tile_cnt[blockIdx.x] = t;
  }
}

// every element, to ranks[its index]: (heads before the tile) + (heads of the tile up to and
// including it) - 1. The first element of the array is a head, so the sum is >= 1 everywhere; the
// in-tile prefix runs on across the tile's rows (row_base), unlike a compaction's per-survivor slot.
template <typename K>
__global__ __launch_bounds__(UQ_BLOCK) void k_rank_write(const K *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                         uint64_t T, const uint32_t *__restrict__ tile_off,
                                                         uint32_t *__restrict__ ranks) {
  __shared__ uint32_t s_cnt[UQ_ROWS][UQ_BLOCK / 64];
  const uint64_t base = blockIdx.x * UQ_TILE;
  const int lane = threadIdx.x & 63, wid = threadIdx.x / 64;
  const uint64_t le = ((1ull << lane) - 1ull) | (1ull << lane);
  uint64_t masks[UQ_ROWS];
#pragma unroll
  for (int j = 0; j < UQ_ROWS; ++j) {
    masks[j] = __ballot(wr_head(keys, base + (uint64_t)j * UQ_BLOCK + threadIdx.x, T));
    if (lane == 0) s_cnt[j][wid] = (uint32_t)__popcll(masks[j]);
  }
  __syncthreads();
  uint32_t row_base = tile_off[blockIdx.x];
#pragma unroll
  for (int j = 0; j < UQ_ROWS; ++j) {
    uint32_t before = 0, row = 0;
#pragma unroll
    for (int x = 0; x < UQ_BLOCK / 64; ++x) {
      const uint32_t c = s_cnt[j][x];
      before += x < wid ? c : 0u;
      row += c;
    }
    const uint64_t i = base + (uint64_t)j * UQ_BLOCK + threadIdx.x;
    if (i < T) ranks[vals[i]] = row_base + before + (uint32_t)__popcll(masks[j] & le) - 1u;
    row_base += row;
  }
}

static inline size_t weight_key_bytes(uint32_t wtype) { return wtype == GHS_W_FLOAT32 ? 4 : 8; }

static size_t weight_prim_bytes(uint32_t wtype, uint64_t m) {
  size_t sort_b = 0;
  if (wtype == GHS_W_FLOAT32)
    (void)rocprim::radix_sort_pairs(nullptr, sort_b, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                    (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)m, 0u, 32u);
  else
    (void)rocprim::radix_sort_pairs(nullptr, sort_b, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                    (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)m, 0u, 64u);
  const size_t tiles_b = ((m + UQ_TILE - 1) / UQ_TILE) * 4;
  return align256(sort_b > tiles_b ? sort_b : tiles_b);
}

// the enqueue of ghs_weight_ranks_device for one weight type: status[0] = distinct, [1] = NaN flag
template <uint32_t WT>
static int weight_ranks_enqueue(uint64_t T, const void *d_weights, uint32_t *d_ranks, char *base, uint64_t *status,
                                void *prim_temp, size_t prim_bytes, hipStream_t st) {
  typedef typename WeightKey<WT>::key_t K;
  constexpr uint64_t VEC = 16 / sizeof(K);
  const size_t ak = align256(T * sizeof(K)), a4 = align256(T * 4);
  K *ka = (K *)base;
  K *kb = (K *)(base + ak);
  uint32_t *va = (uint32_t *)(base + 2 * ak);
  uint32_t *vb = (uint32_t *)(base + 2 * ak + a4);
  const uint64_t ntiles = (T + UQ_TILE - 1) / UQ_TILE;
  uint32_t *tiles = (uint32_t *)prim_temp;  // reused after the sort
  uint64_t head = ((16 - ((uintptr_t)d_weights & 15)) & 15) / sizeof(K);
  if (head > T) head = T;
  const uint64_t nvec = (T - head) / VEC, nscalar = T - VEC * nvec;

  GHS_HIP_CHECK(hipMemsetAsync(status, 0, 16, st));
  k_weight_keys<WT><<<grid_cap(nvec > nscalar ? nvec : nscalar, BLOCK, 2048), BLOCK, 0, st>>>(
      head, nvec, nscalar, (const K *)d_weights, ka, va, (unsigned int *)(status + 1));
  GHS_HIP_CHECK(hipGetLastError());
  GHS_HIP_CHECK(rocprim::radix_sort_pairs(prim_temp, prim_bytes, ka, kb, va, vb, (size_t)T, 0u,
                                          (unsigned int)(8 * sizeof(K)), st));
  k_rank_count<K><<<(unsigned)ntiles, UQ_BLOCK, 0, st>>>(kb, T, tiles);
  k_uniq_scan<<<1, 1024, 0, st>>>(tiles, (uint32_t)ntiles, status);
  k_rank_write<K><<<(unsigned)ntiles, UQ_BLOCK, 0, st>>>(kb, vb, T, tiles, d_ranks);
  GHS_HIP_CHECK(hipGetLastError());
  return GHS_OK;
}

// ---- grid ----------------------------------------------------------------------------------
__global__ void k_grid(uint32_t k, uint32_t mode, uint64_t wseed, uint32_t *__restrict__ u, uint32_t *__restrict__ v,
                       uint32_t *__restrict__ w) {
  const uint64_t n = (uint64_t)k * k;
  for (uint64_t x = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; x < n; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = (uint32_t)(x / k), c = (uint32_t)(x % k);
    uint64_t e = (r < k - 1) ? (uint64_t)r * (2ull * k - 1) + 2ull * c
                             : (uint64_t)(k - 1) * (2ull * k - 1) + c;
    if (c < k - 1) {
      u[e] = (uint32_t)x; v[e] = (uint32_t)(x + 1);
      w[e] = mode ? (uint32_t)e : mix32((uint32_t)e ^ (uint32_t)wseed);
      ++e;
    }
    if (r < k - 1) {
      u[e] = (uint32_t)x; v[e] = (uint32_t)(x + k);
      w[e] = mode ? (uint32_t)e : mix32((uint32_t)e ^ (uint32_t)wseed);
    }
  }
}

}  // namespace ghs

using namespace ghs;

extern "C" {

int ghs_check_canonical(uint32_t n, uint64_t m, const uint32_t *d_u, const uint32_t *d_v, void *stream, int *ok) {
  hipStream_t st = (hipStream_t)stream;
  if (!ok) GHS_FAIL(GHS_E_ARG, "ok is NULL");
  *ok = 1;
  if (m == 0) return GHS_OK;
  if (!d_u || !d_v) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  unsigned int *bad = nullptr;
  GHS_HIP_CHECK(hipMallocAsync((void **)&bad, sizeof(unsigned int), st));
  GHS_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(unsigned int), st));
  k_check_canonical<<<grid_cap(m, 256, 16384), 256, 0, st>>>(n, m, d_u, d_v, bad);
  unsigned int h_bad = 0;
  hipError_t e = hipMemcpyAsync(&h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFreeAsync(bad, st);
  GHS_HIP_CHECK(e);
  *ok = h_bad ? 0 : 1;
  return GHS_OK;
}

int ghs_csr_offsets(uint32_t n, uint64_t m, const uint32_t *d_u, uint32_t *d_off, void *stream) {
  if (!d_off || (m && !d_u)) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if (m >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "m must be < 2^31");
  k_csr_offsets<<<grid_cap(m + 1, 256, 16384), 256, 0, (hipStream_t)stream>>>(n, m, d_u, d_off);
  GHS_HIP_CHECK(hipGetLastError());
  return GHS_OK;
}

size_t ghs_rmat_temp_bytes(uint32_t scale, uint32_t edgefactor) {
  const uint64_t T = (uint64_t)edgefactor << scale;
  size_t sort_b = 0;
  (void)rocprim::radix_sort_keys(nullptr, sort_b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)T, 0u,
                                 2u * scale);
  const size_t tiles_b = align256(((T + UQ_TILE - 1) / UQ_TILE) * 4);
  return 2 * align256(T * 8) + align256(sort_b > tiles_b ? sort_b : tiles_b) + 256;
}

int ghs_rmat_generate(uint32_t scale, uint32_t edgefactor, uint64_t seed, uint64_t wseed, uint32_t *d_u,
                      uint32_t *d_v, uint32_t *d_w, uint64_t *m_out, void *d_temp, size_t temp_bytes, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!m_out || !d_u || !d_v || !d_w || !d_temp) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if (scale < 1 || scale > 31) GHS_FAIL(GHS_E_ARG, "scale must be in [1, 31]");
  const uint64_t T = (uint64_t)edgefactor << scale;
  if (T == 0 || T >= (1ull << 32)) GHS_FAIL(GHS_E_ARG, "edgefactor * 2^scale must be in [1, 2^32)");
  if (temp_bytes < ghs_rmat_temp_bytes(scale, edgefactor)) GHS_FAIL(GHS_E_NOMEM, "temp too small");
  char *base = (char *)d_temp;
  uint64_t *ka = (uint64_t *)base;
  uint64_t *kb = (uint64_t *)(base + align256(T * 8));
  uint64_t *nsel = (uint64_t *)(base + 2 * align256(T * 8));
  void *prim_temp = base + 2 * align256(T * 8) + 256;
  size_t prim_bytes = temp_bytes - (2 * align256(T * 8) + 256);
  const uint64_t ntiles = (T + UQ_TILE - 1) / UQ_TILE;
  uint32_t *tiles = (uint32_t *)prim_temp;  // reused after the sort
  const uint64_t marker = (1ull << (2 * scale)) - 1ull;  // a self-loop's key (sorts last)

  k_rmat_tuples<<<grid_cap(T, 256, 16384), 256, 0, st>>>(T, scale, seed, ka);
  GHS_HIP_CHECK(hipGetLastError());
  GHS_HIP_CHECK(rocprim::radix_sort_keys(prim_temp, prim_bytes, ka, kb, (size_t)T, 0u, 2u * scale, st));
  k_uniq_count<<<(unsigned)ntiles, UQ_BLOCK, 0, st>>>(kb, T, marker, tiles);
  k_uniq_scan<<<1, 1024, 0, st>>>(tiles, (uint32_t)ntiles, nsel);
  k_uniq_write<<<(unsigned)ntiles, UQ_BLOCK, 0, st>>>(kb, T, marker, tiles, scale, wseed, d_u, d_v, d_w);
  GHS_HIP_CHECK(hipGetLastError());
  uint64_t cnt = 0;
  GHS_HIP_CHECK(hipMemcpyAsync(&cnt, nsel, 8, hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipStreamSynchronize(st));
  *m_out = cnt;
  return GHS_OK;
}

// temp layout: keys in / out (8 B per raw edge each), raw indices in / out (4 B each), a 256-byte
// status block (canonical count, error flag), then rocPRIM's sort storage, reused for the tile counts
static size_t canon_prim_bytes(uint32_t n, uint64_t m_raw) {
  size_t sort_b = 0;
  (void)rocprim::radix_sort_pairs(nullptr, sort_b, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                  (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)m_raw, 0u,
                                  2u * canon_bits(n));
  const size_t tiles_b = ((m_raw + UQ_TILE - 1) / UQ_TILE) * 4;
  return align256(sort_b > tiles_b ? sort_b : tiles_b);
}

size_t ghs_canonicalize_temp_bytes(uint32_t n, uint64_t m_raw) {
  if (m_raw == 0 || m_raw >= (1ull << 32)) return 0;
  return 2 * align256(m_raw * 8) + 2 * align256(m_raw * 4) + 256 + canon_prim_bytes(n, m_raw);
}

int ghs_canonicalize_device(uint32_t n, uint64_t m_raw, const uint32_t *d_ru, const uint32_t *d_rv,
                            const uint32_t *d_rw, uint32_t *d_u, uint32_t *d_v, uint32_t *d_w, uint32_t *d_src,
                            uint64_t *m_out, void *d_temp, size_t temp_bytes, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!m_out) GHS_FAIL(GHS_E_ARG, "m_out is NULL");
  *m_out = 0;
  if (m_raw == 0) return GHS_OK;
  if (m_raw >= (1ull << 32)) GHS_FAIL(GHS_E_ARG, "m_raw must be < 2^32");
  if (!d_ru || !d_rv || !d_rw || !d_u || !d_v || !d_w || !d_temp) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if (((uintptr_t)d_ru | (uintptr_t)d_rv | (uintptr_t)d_rw) & 3)
    GHS_FAIL(GHS_E_ARG, "raw u, v, w must be 4-byte aligned");
  if (((uintptr_t)d_u | (uintptr_t)d_v | (uintptr_t)d_w | (uintptr_t)d_src | (uintptr_t)d_temp) & 15)
    GHS_FAIL(GHS_E_ARG, "outputs and temp must be 16-byte aligned");
  if (temp_bytes < ghs_canonicalize_temp_bytes(n, m_raw)) GHS_FAIL(GHS_E_NOMEM, "temp too small");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");

  const uint64_t T = m_raw;
  const size_t a8 = align256(T * 8), a4 = align256(T * 4);
  char *base = (char *)d_temp;
  uint64_t *ka = (uint64_t *)base;
  uint64_t *kb = (uint64_t *)(base + a8);
  uint32_t *va = (uint32_t *)(base + 2 * a8);
  uint32_t *vb = (uint32_t *)(base + 2 * a8 + a4);
  uint64_t *status = (uint64_t *)(base + 2 * a8 + 2 * a4);  // [0] canonical count, [1] error flag
  void *prim_temp = base + 2 * a8 + 2 * a4 + 256;
  size_t prim_bytes = canon_prim_bytes(n, T);
  const uint64_t ntiles = (T + UQ_TILE - 1) / UQ_TILE;
  uint32_t *tiles = (uint32_t *)prim_temp;  // reused after the sort
  const uint32_t bits = canon_bits(n);
  const uint64_t marker = bits >= 32 ? ~0ull : ((1ull << (2 * bits)) - 1ull);

  // the 16-byte vector body of pass 1: from the first element at which ru is 16-byte aligned, when
  // rv is aligned there too (slices of separate allocations usually are; else all scalar)
  uint64_t head = ((16 - ((uintptr_t)d_ru & 15)) & 15) / 4, nquads = 0, nscalar = T;
  if (head > T) head = T;
  if ((((uintptr_t)d_rv + 4 * head) & 15) == 0) {
    nquads = (T - head) / 4;
    nscalar = T - 4 * nquads;
  } else {
    head = 0;
  }

  GHS_HIP_CHECK(hipMemsetAsync(status, 0, 16, st));
  k_canon_keys<<<grid_cap(nquads > nscalar ? nquads : nscalar, BLOCK, 2048), BLOCK, 0, st>>>(
      n, bits, marker, head, nquads, nscalar, d_ru, d_rv, ka, va, (unsigned int *)(status + 1));
  GHS_HIP_CHECK(hipGetLastError());
  GHS_HIP_CHECK(rocprim::radix_sort_pairs(prim_temp, prim_bytes, ka, kb, va, vb, (size_t)T, 0u, 2u * bits, st));
  k_canon_count<<<(unsigned)ntiles, UQ_BLOCK, 0, st>>>(kb, T, marker, tiles);
  k_uniq_scan<<<1, 1024, 0, st>>>(tiles, (uint32_t)ntiles, status);
  k_canon_write<<<(unsigned)ntiles, UQ_BLOCK, 0, st>>>(kb, vb, T, marker, tiles, bits, d_rw, d_u, d_v, d_w, d_src);
  GHS_HIP_CHECK(hipGetLastError());
  uint64_t h_status[2] = {0, 0};
  GHS_HIP_CHECK(hipMemcpyAsync(h_status, status, 16, hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipStreamSynchronize(st));
  if (h_status[1])
    GHS_FAIL(GHS_E_ARG, "vertex id out of range: a raw endpoint is >= n = " + std::to_string(n));
  if (h_status[0] >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "the canonical edge count must be < 2^31");
  *m_out = h_status[0];
  return GHS_OK;
}

// temp layout: keys in / out (4 or 8 B per weight each), indices in / out (4 B each), a 256-byte
// status block (distinct count, NaN flag), then rocPRIM's sort storage, reused for the tile counts
size_t ghs_weight_ranks_temp_bytes(uint32_t wtype, uint64_t m) {
  if (wtype > GHS_W_UINT64 || m == 0 || m >= (1ull << 32)) return 0;
  return 2 * align256(m * weight_key_bytes(wtype)) + 2 * align256(m * 4) + 256 + weight_prim_bytes(wtype, m);
}

int ghs_weight_ranks_device(uint32_t wtype, uint64_t m, const void *d_weights, uint32_t *d_ranks, uint64_t *distinct,
                            void *d_temp, size_t temp_bytes, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  if (wtype > GHS_W_UINT64) GHS_FAIL(GHS_E_ARG, "unknown weight type " + std::to_string(wtype));
  if (!distinct) GHS_FAIL(GHS_E_ARG, "distinct is NULL");
  *distinct = 0;
  if (m == 0) return GHS_OK;
  if (m >= (1ull << 32)) GHS_FAIL(GHS_E_ARG, "m must be < 2^32");
  if (!d_weights || !d_ranks || !d_temp) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  const size_t kb = weight_key_bytes(wtype);
  if ((uintptr_t)d_weights & (kb - 1))
    GHS_FAIL(GHS_E_ARG, "weights must be aligned to their element size (" + std::to_string(kb) + " bytes)");
  if ((uintptr_t)d_ranks & 3) GHS_FAIL(GHS_E_ARG, "ranks must be 4-byte aligned");
  if ((uintptr_t)d_temp & 15) GHS_FAIL(GHS_E_ARG, "temp must be 16-byte aligned");
  const size_t need = ghs_weight_ranks_temp_bytes(wtype, m);
  if (temp_bytes < need) GHS_FAIL(GHS_E_NOMEM, "temp too small");
  const uintptr_t r0 = (uintptr_t)d_ranks, r1 = r0 + m * 4;
  if ((r0 < (uintptr_t)d_weights + m * kb && (uintptr_t)d_weights < r1) ||
      (r0 < (uintptr_t)d_temp + need && (uintptr_t)d_temp < r1))
    GHS_FAIL(GHS_E_ARG, "ranks must not overlap the weights or temp");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");

  const size_t ak = align256(m * kb), a4 = align256(m * 4);
  char *base = (char *)d_temp;
  uint64_t *status = (uint64_t *)(base + 2 * ak + 2 * a4);  // [0] distinct count, [1] NaN flag
  void *prim_temp = base + 2 * ak + 2 * a4 + 256;
  const size_t prim_bytes = weight_prim_bytes(wtype, m);
  int rc = GHS_OK;
  switch (wtype) {
    case GHS_W_FLOAT32:
      rc = weight_ranks_enqueue<GHS_W_FLOAT32>(m, d_weights, d_ranks, base, status, prim_temp, prim_bytes, st);
      break;
    case GHS_W_FLOAT64:
      rc = weight_ranks_enqueue<GHS_W_FLOAT64>(m, d_weights, d_ranks, base, status, prim_temp, prim_bytes, st);
      break;
    case GHS_W_INT64:
      rc = weight_ranks_enqueue<GHS_W_INT64>(m, d_weights, d_ranks, base, status, prim_temp, prim_bytes, st);
      break;
    default:
      rc = weight_ranks_enqueue<GHS_W_UINT64>(m, d_weights, d_ranks, base, status, prim_temp, prim_bytes, st);
      break;
  }
  if (rc != GHS_OK) return rc;
  uint64_t h_status[2] = {0, 0};
  GHS_HIP_CHECK(hipMemcpyAsync(h_status, status, 16, hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipStreamSynchronize(st));
  if (h_status[1]) GHS_FAIL(GHS_E_ARG, "NaN weight: weights must be comparable numbers");
  *distinct = h_status[0];
  return GHS_OK;
}

struct FlagOne {
  __host__ __device__ uint32_t operator()(uint8_t f) const { return f ? 1u : 0u; }
};

}  // extern "C"

// ghs_flags_to_eids' per-device temporary storage (grown on demand), freed by ghs_release_cache
// (it used to be held until the process ended, outside torch's allocator's view)
namespace {
struct EidTemp {
  void *p = nullptr;
  size_t bytes = 0;
  uint32_t *h_cnt = nullptr;  // pinned: the selected count
  uint32_t *d_cnt = nullptr;
};
std::mutex g_eid_mu;
std::unordered_map<int, EidTemp> g_eid_temps;
}  // namespace

void ghs_release_eid_temps() {
  std::lock_guard<std::mutex> lock(g_eid_mu);
  int cur = 0;
  const bool have = hipGetDevice(&cur) == hipSuccess;
  for (auto &kv : g_eid_temps) {
    (void)hipSetDevice(kv.first);
    if (kv.second.p) (void)hipFree(kv.second.p);
    if (kv.second.d_cnt) (void)hipFree(kv.second.d_cnt);
    if (kv.second.h_cnt) (void)hipHostFree(kv.second.h_cnt);
  }
  g_eid_temps.clear();
  if (have) (void)hipSetDevice(cur);
}

extern "C" {

// The MSF edge ids of a flag range (a rank's own range for collect_results,
// ghs_implementation_mpi.py:760-779): rocPRIM's flagged select over a counting input. Its temporary
// storage is kept per device (grown on demand); the count comes back through pinned memory.
int ghs_flags_to_eids(const uint8_t *d_in_mst, uint64_t lo, uint64_t hi, uint32_t *d_eids, uint64_t capacity,
                      uint64_t *count, void *stream) {
  if (!count || (hi > lo && (!d_in_mst || !d_eids))) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if (hi < lo || hi >= (1ull << 32)) GHS_FAIL(GHS_E_ARG, "bad range (need lo <= hi < 2^32)");
  *count = 0;
  if (hi == lo) return GHS_OK;
  std::lock_guard<std::mutex> lock(g_eid_mu);
  int dev = 0;
  GHS_HIP_CHECK(hipGetDevice(&dev));
  EidTemp &t = g_eid_temps[dev];
  hipStream_t st = (hipStream_t)stream;
  const size_t N = (size_t)(hi - lo);
  rocprim::counting_iterator<uint32_t> in((uint32_t)lo);
  size_t need = 0;
  GHS_HIP_CHECK(rocprim::select(nullptr, need, in, d_in_mst + lo, d_eids, (uint32_t *)nullptr, N, st));
  if (!t.h_cnt) {
    GHS_HIP_CHECK(hipHostMalloc((void **)&t.h_cnt, sizeof(uint32_t), hipHostMallocDefault));
    GHS_HIP_CHECK(hipMalloc((void **)&t.d_cnt, sizeof(uint32_t)));
  }
  if (t.bytes < need) {
    if (t.p) (void)hipFree(t.p);
    t.p = nullptr;
    t.bytes = 0;
    GHS_HIP_CHECK(hipMalloc(&t.p, need));
    t.bytes = need;
  }
  // the output holds at most `capacity` ids: when the range is longer, count the flags first
  // (rocPRIM writes every selected id) and refuse the call instead of writing past it
  if (N > capacity) {
    auto ones = rocprim::make_transform_iterator(d_in_mst + lo, FlagOne());
    size_t rneed = 0;
    GHS_HIP_CHECK(rocprim::reduce(nullptr, rneed, ones, t.d_cnt, 0u, N, rocprim::plus<uint32_t>(), st));
    if (rneed > need) need = rneed;
    if (t.bytes < need) {
      if (t.p) (void)hipFree(t.p);
      t.p = nullptr;
      t.bytes = 0;
      GHS_HIP_CHECK(hipMalloc(&t.p, need));
      t.bytes = need;
    }
    GHS_HIP_CHECK(rocprim::reduce(t.p, rneed, ones, t.d_cnt, 0u, N, rocprim::plus<uint32_t>(), st));
    GHS_HIP_CHECK(hipMemcpyAsync(t.h_cnt, t.d_cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    GHS_HIP_CHECK(hipStreamSynchronize(st));
    if (*t.h_cnt > capacity) GHS_FAIL(GHS_E_NOMEM, "more flagged edges than the output's capacity");
  }
  GHS_HIP_CHECK(rocprim::select(t.p, need, in, d_in_mst + lo, d_eids, t.d_cnt, N, st));
  GHS_HIP_CHECK(hipMemcpyAsync(t.h_cnt, t.d_cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipStreamSynchronize(st));
  *count = *t.h_cnt;
  return GHS_OK;
}

int ghs_rmat_tuples(uint32_t scale, uint32_t edgefactor, uint64_t seed, uint64_t *d_keys, void *stream) {
  if (!d_keys) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if (scale < 1 || scale > 31) GHS_FAIL(GHS_E_ARG, "scale must be in [1, 31]");
  const uint64_t T = (uint64_t)edgefactor << scale;
  if (T == 0 || T >= (1ull << 32)) GHS_FAIL(GHS_E_ARG, "edgefactor * 2^scale must be in [1, 2^32)");
  k_rmat_tuples<<<grid_cap(T, 256, 16384), 256, 0, (hipStream_t)stream>>>(T, scale, seed, d_keys);
  GHS_HIP_CHECK(hipGetLastError());
  return GHS_OK;
}

int ghs_grid_generate(uint32_t k, uint32_t mode, uint64_t wseed, uint32_t *d_u, uint32_t *d_v, uint32_t *d_w,
                      void *stream) {
  if (k < 2) return GHS_OK;
  if ((uint64_t)k * k >= (1ull << 32)) GHS_FAIL(GHS_E_ARG, "k*k must be < 2^32");
  if (!d_u || !d_v || !d_w) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  const uint64_t n = (uint64_t)k * k;
  k_grid<<<grid_cap(n, 256, 16384), 256, 0, (hipStream_t)stream>>>(k, mode, wseed, d_u, d_v, d_w);
  GHS_HIP_CHECK(hipGetLastError());
  return GHS_OK;
}

}  // extern "C"
