// Exact brute-force k nearest neighbours of float32 points (ABI 10 addition, ghs_knn_device): the front
// of HDBSCAN on points. Semantics (the distance chain, the 64-bit keys, the tie-break): include/ghs_mst.h.
//
// k_knn_scan, grid = query tiles x slices, 256 threads. A workgroup owns TQ = 64 queries and sweeps the
// candidate tiles (TC = 64) of its slice. A step is one (candidate tile, dim chunk) pair: both sides' CH = 32
// dims go through LDS dim-major (row stride LD = TQ + 4 floats, so a lane's four queries or candidates are
// one 16-byte LDS read), fetched from global one step ahead into registers (16-byte loads when dim % 4 == 0,
// which with the 16-byte aligned base makes every row 16-byte aligned; scalar loads otherwise). Lane
// (tq, tc) = (tid / 16, tid % 16) keeps acc[4][4] for queries 4 tq + i and candidates 4 tc + j; every
// accumulator sees the dims in ascending order, s = a - b, acc = fmaf(s, s, acc), so the header's chain
// is reproduced bit for bit whatever the tiling. Rows and dims past the end are zeros in LDS
// (fmaf(0, 0, acc) == acc); candidates past n and the query itself are masked out of the selection.
//
// Selection, fused. Per query a sorted list of k keys in LDS, all UINT64_MAX to start; its last entry is
// the threshold. After a tile's last chunk every lane compares its 16 keys with its rows' thresholds; a tile
// where nothing passes costs four threshold reads, 16 compares and one barrier. Otherwise what passed goes
// to the query's LDS queue (QSLOTS entries; a full queue leaves the key with its lane for the next turn),
// each wave inserts the queues of a quarter of the queries, a whole wave per insertion (two reads and a
// write per list entry, whatever k is), and the turn repeats while any lane holds a key. A query's list
// takes about k ln(n / k) insertions over a sweep, a few per tile at n = 2^17 and fewer as n grows.
//
// slices == 1: the scan writes d_idx / d_dist itself. Otherwise every slice writes its lists to the
// workspace and k_knn_merge, one wave per query with one slice's list per lane, pops the smallest head k
// times. The finite check sits where rows are loaded: a non-finite coordinate is replaced by 0 before it
// reaches LDS (no key is formed from a NaN) and raises the status flag. No floating-point atomics; the
// only global atomic is the integer count of zero distances.
//
// This translation unit includes common.h only and launches only its own kernels.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>

#include "common.h"

namespace ghs {
namespace knn {

constexpr int KN_BLOCK = 256;
constexpr int TQ = GHS_KNN_TILE_Q, TC = GHS_KNN_TILE_C, CH = GHS_KNN_DIM_CHUNK;
constexpr int LD = TQ + 4;         // LDS row stride in floats: rows stay 16-byte aligned, staging stores 4-way at worst
constexpr int QSLOTS = 16;         // queue entries per query and turn
constexpr uint32_t TARGET_WGS = 1024;  // auto slices: 4 workgroups per CU
constexpr unsigned long long KEY_MAX = ~0ull;
static_assert(TQ == 64 && TC == 64 && KN_BLOCK == (TQ / 4) * (TC / 4), "4 x 4 accumulators per lane");
static_assert(CH % 4 == 0 && (TQ + TC) * (CH / 4) == 4 * KN_BLOCK, "four 16-byte staging loads per lane and step");
static_assert((LD * 4) % 16 == 0, "LDS rows are read 16 bytes at a time");

// status block (256 B): uint32 slots, one uint64 at byte 8
enum { ST_NONFINITE = 0, ST_BAD = 1, ST_SLOTS = 64 };
enum { ST64_ZEROS = 1 };

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// One staged piece: four consecutive dims of one row. Every load is unconditional, from the element itself or,
// past the row's or the array's end, from x[0]; bit e of the returned mask says that element e is real. The
// values are not looked at here, so the loads stay in flight until the piece is stored (clean).
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

// the finite check, where a piece goes to LDS: padding is 0; a non-finite coordinate becomes 0 and is reported
__device__ __forceinline__ float clean(float c, bool real, uint32_t &nonfinite) {
  const bool bad = real && (__float_as_uint(c) & 0x7f800000u) == 0x7f800000u;
  nonfinite |= bad;
  return real && !bad ? c : 0.f;
}

// The correctly rounded square root. sqrtf is that under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt; __fsqrt_rn is not: without OCML_BASIC_ROUNDED_OPERATIONS this
// toolchain maps it to the native instruction (1 ulp), and the exact tests tell the two apart.
__device__ __forceinline__ float rounded_sqrt(float d2) { return sqrtf(d2); }

template <int KCAP>
__global__ __launch_bounds__(KN_BLOCK) void k_knn_scan(uint32_t n, uint32_t dim, uint32_t k, uint32_t metric, uint32_t slices,
                                                       const float *__restrict__ x, uint32_t *__restrict__ idx,
                                                       float *__restrict__ dist, unsigned long long *__restrict__ parts,
                                                       uint32_t *__restrict__ status) {
  __shared__ __attribute__((aligned(16))) float s_q[CH * LD];
  __shared__ __attribute__((aligned(16))) float s_c[CH * LD];
  __shared__ unsigned long long s_list[KCAP * TQ];
  __shared__ unsigned long long s_queue[QSLOTS * TQ];
  __shared__ uint32_t s_qn[TQ];

  const uint32_t tid = threadIdx.x, tq = tid >> 4, tc = tid & 15;
  const uint64_t q0 = (uint64_t)blockIdx.x * TQ;
  const uint32_t slice = blockIdx.y;
  const uint32_t ctiles = (uint32_t)(((uint64_t)n + TC - 1) / TC), nchunks = (dim + CH - 1) / CH;
  const uint32_t t_lo = (uint32_t)((uint64_t)slice * ctiles / slices), t_hi = (uint32_t)((uint64_t)(slice + 1) * ctiles / slices);
  const bool vec = (dim & 3u) == 0;
  uint32_t nonfinite = 0;

  for (uint32_t e = tid; e < KCAP * TQ; e += KN_BLOCK) s_list[e] = KEY_MAX;
  if (tid < TQ) s_qn[tid] = 0;

  // a lane's staging pieces: r = 0, 1 of the query side, r = 2, 3 of the candidate side
  const uint32_t st_row[2] = {tid >> 3, (tid + KN_BLOCK) >> 3}, st_d = (tid & 7u) * 4;
  float4 pre[4];
  uint32_t real = 0;  // bit 4 r + e: element e of pre[r] is no padding
  auto fetch = [&](uint32_t ct, uint32_t dc) {
    real = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      real |= load_piece(x, n, dim, (r < 2 ? q0 : (uint64_t)ct * TC) + st_row[r & 1], dc * CH + st_d, vec, pre[r]) << (4 * r);
  };

  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

  uint32_t ct = t_lo, dc = 0;
  if (ct < t_hi) fetch(ct, dc);
  __syncthreads();  // the lists are set
  while (ct < t_hi) {  // block-uniform
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float *dst = (r < 2 ? s_q : s_c) + st_d * LD + st_row[r & 1];
      const uint32_t m = real >> (4 * r);
      dst[0] = clean(pre[r].x, m & 1u, nonfinite), dst[LD] = clean(pre[r].y, m & 2u, nonfinite);
      dst[2 * LD] = clean(pre[r].z, m & 4u, nonfinite), dst[3 * LD] = clean(pre[r].w, m & 8u, nonfinite);
    }
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
      // the tile's 16 keys of this lane are (bits of acc[i][j]) << 32 | c0 + j; bit 4 i + j of `pending`: the
      // key may still enter its query's list
      const uint64_t c0 = (uint64_t)ct_now * TC + tc * 4;
      uint32_t pending = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint64_t qi = q0 + tq * 4 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (qi < n && c0 + j < n && c0 + j != qi) pending |= 1u << (4 * i + j);  // padding and the query itself never compete
      }
      // what cannot enter: a key that does not beat its query's threshold, the list's last entry
      auto filter = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const unsigned long long thr = s_list[(tq * 4 + i) * KCAP + k - 1];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(acc[i][j]) << 32) | (uint32_t)(c0 + j);
            if (key >= thr) pending &= ~(1u << (4 * i + j));
          }
        }
      };
      filter();
      // Keys are distinct, so a list's final content is the k smallest keys of the candidate set, a pure
      // function of that set: neither the order in which lanes reach the queue nor the turn in which a key
      // gets its slot can change the result.
      while (__syncthreads_or(pending != 0)) {  // most tiles of a long sweep: no turn at all
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if ((pending >> (4 * i + j)) & 1u) {
              const uint32_t slot = atomicAdd(&s_qn[tq * 4 + i], 1u);
              if (slot < (uint32_t)QSLOTS) {  // a full queue leaves the key with its lane for the next turn
                s_queue[slot * TQ + tq * 4 + i] =
                    ((unsigned long long)__float_as_uint(acc[i][j]) << 32) | (uint32_t)(c0 + j);
                pending &= ~(1u << (4 * i + j));
              }
            }
        __syncthreads();
        // Wave w inserts for the queries w, w + 4, ...: lane j holds entries j and j + 64 of the list, and one
        // insertion is two reads and a write per entry, whatever k is: an entry below the key stays, the first
        // one above it becomes the key, every later one takes its predecessor.
        {
          const uint32_t wave = tid >> 6, lane = tid & 63;
          const uint32_t mine = lane < (uint32_t)(TQ / 4) ? s_qn[wave + 4 * lane] : 0u;
          unsigned long long has = __ballot(mine != 0);
          while (has) {  // wave-uniform
            const int l = __ffsll((long long)has) - 1;
            has &= has - 1;
            const uint32_t q = wave + 4 * (uint32_t)l;
            uint32_t cnt = __shfl(mine, l);
            cnt = cnt < (uint32_t)QSLOTS ? cnt : (uint32_t)QSLOTS;
            unsigned long long *list = s_list + q * KCAP;
            for (uint32_t e = 0; e < cnt; ++e) {
              const unsigned long long key = s_queue[e * TQ + q];
              if (key >= list[k - 1]) continue;
              unsigned long long nv[2];
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                const uint32_t j = lane + 64 * h;
                if (j < k) {
                  const unsigned long long cur = list[j], prev = j ? list[j - 1] : 0ull;
                  nv[h] = cur < key ? cur : ((j == 0 || prev < key) ? key : prev);
                }
              }
              // lanes read their neighbours' entries: every read of the wave comes before its writes, and the
              // writes before the next insertion's reads (the wave's LDS operations complete in order; the
              // fences keep the compiler from moving them)
              __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
              for (int h = 0; h < 2; ++h)
                if (lane + 64 * h < k) list[lane + 64 * h] = nv[h];
              __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
          }
          if (lane < (uint32_t)(TQ / 4)) s_qn[wave + 4 * lane] = 0;
        }
        __syncthreads();
        filter();
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    }
    if (!last_chunk) __syncthreads();  // every lane is done with the tiles before the next step overwrites them (the selection ends in a barrier of its own)
  }
  __syncthreads();

  unsigned long long zeros = 0;
  for (uint32_t e = tid; e < k * TQ; e += KN_BLOCK) {
    const uint32_t q = e / k, j = e - q * k;
    const uint64_t row = q0 + q;
    if (row >= n) continue;
    const unsigned long long kk = s_list[q * KCAP + j];
    if (slices == 1) {
      if (kk == KEY_MAX) {  // never: n - 1 >= k candidates compete
        status[ST_BAD] = 1;
        continue;
      }
      const float d2 = __uint_as_float((uint32_t)(kk >> 32));
      idx[row * k + j] = (uint32_t)kk;
      dist[row * k + j] = metric == GHS_KNN_EUCLIDEAN ? rounded_sqrt(d2) : d2;
      zeros += (kk >> 32) == 0;
    } else {
      parts[((size_t)slice * n + row) * k + j] = kk;
    }
  }
  if (slices == 1) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) zeros += __shfl_xor(zeros, s);
    if ((tid & 63) == 0 && zeros) atomicAdd(reinterpret_cast<unsigned long long *>(status) + ST64_ZEROS, zeros);
  }
  if (nonfinite) status[ST_NONFINITE] = 1;
}

// one wave per query, lane s holds the head of slice s's sorted list: k times the smallest head leaves
__global__ __launch_bounds__(KN_BLOCK) void k_knn_merge(uint32_t n, uint32_t k, uint32_t metric, uint32_t slices,
                                                        const unsigned long long *__restrict__ parts,
                                                        uint32_t *__restrict__ idx, float *__restrict__ dist,
                                                        uint32_t *__restrict__ status) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
  const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  unsigned long long zeros = 0;
  for (uint64_t i = wave; i < n; i += waves) {  // wave-uniform
    const unsigned long long *list = parts + ((size_t)lane * n + i) * k;
    uint32_t p = 0;
    unsigned long long head = lane < slices ? list[0] : KEY_MAX;
    for (uint32_t j = 0; j < k; ++j) {
      unsigned long long m = head;
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {
        const unsigned long long o = __shfl_xor(m, s);
        m = o < m ? o : m;
      }
      if (m == KEY_MAX) {  // never: the slices hold n - 1 >= k keys between them
        if (lane == 0) status[ST_BAD] = 1;
        break;
      }
      if (head == m) {  // one lane: keys are distinct
        ++p;
        head = p < k ? list[p] : KEY_MAX;
      }
      if (lane == 0) {
        const float d2 = __uint_as_float((uint32_t)(m >> 32));
        idx[i * k + j] = (uint32_t)m;
        dist[i * k + j] = metric == GHS_KNN_EUCLIDEAN ? rounded_sqrt(d2) : d2;
        zeros += (m >> 32) == 0;
      }
    }
  }
  if (lane == 0 && zeros) atomicAdd(reinterpret_cast<unsigned long long *>(status) + ST64_ZEROS, zeros);
}

// ---- host side ----------------------------------------------------------------------------------------------
static inline uint32_t query_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + TQ - 1) / TQ); }

// a function of n alone: enough slices for TARGET_WGS workgroups
static inline uint32_t auto_slices(uint32_t n) {
  const uint32_t tiles = query_tiles(n);
  if (tiles == 0) return 1;
  uint32_t s = (TARGET_WGS + tiles - 1) / tiles;
  if (s < 1) s = 1;
  if (s > GHS_KNN_MAX_SLICES) s = GHS_KNN_MAX_SLICES;
  return s;
}

struct Layout {
  size_t status, parts, total;
};

static Layout layout(uint32_t n, uint32_t k, uint32_t slices) {
  Layout l{};
  l.status = 0;
  l.parts = 256;
  l.total = 256 + (slices > 1 ? align256((size_t)slices * n * k * 8) : 0);
  return l;
}

static inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

static inline bool overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && abytes && bbytes && x < y + bbytes && y < x + abytes;
}

// everything that needs no device, in the order the header lists it; *slices becomes the count in use
static int check_args(uint32_t n, uint32_t dim, const float *x, uint32_t k, uint32_t metric, uint32_t *slices,
                      const uint32_t *idx, const float *dist, bool device_form, const void *ws, size_t ws_bytes) {
  if (k == 0 || k > GHS_KNN_MAX_K) GHS_FAIL(GHS_E_ARG, "k must be in [1, GHS_KNN_MAX_K]");
  if (dim == 0 || dim > GHS_KNN_MAX_DIM) GHS_FAIL(GHS_E_ARG, "dim must be in [1, GHS_KNN_MAX_DIM]");
  if (metric != GHS_KNN_SQEUCLIDEAN && metric != GHS_KNN_EUCLIDEAN) GHS_FAIL(GHS_E_ARG, "unknown metric");
  if (*slices > GHS_KNN_MAX_SLICES) GHS_FAIL(GHS_E_ARG, "slices must be <= GHS_KNN_MAX_SLICES");
  if (n == 0) return GHS_OK;
  if (k > n - 1) GHS_FAIL(GHS_E_ARG, "k must be <= n - 1 (a point is not its own neighbour)");
  if ((uint64_t)n * k >= (1ull << 32)) GHS_FAIL(GHS_E_ARG, "n * k must be < 2^32");
  if (*slices == 0) *slices = auto_slices(n);
  if (!x || !idx || !dist || (device_form && !ws)) GHS_FAIL(GHS_E_ARG, "NULL pointer");
  if (device_form && (((uintptr_t)x | (uintptr_t)ws) & 15)) GHS_FAIL(GHS_E_ARG, "d_x and the workspace must be 16-byte aligned");
  if (((uintptr_t)idx | (uintptr_t)dist) & 3) GHS_FAIL(GHS_E_ARG, "idx and dist must be 4-byte aligned");
  if (!device_form && ((uintptr_t)x & 3)) GHS_FAIL(GHS_E_ARG, "x must be 4-byte aligned");
  const size_t xb = (size_t)n * dim * 4, ob = (size_t)n * k * 4;
  if (overlap(idx, ob, dist, ob) || overlap(idx, ob, x, xb) || overlap(dist, ob, x, xb))
    GHS_FAIL(GHS_E_ARG, "idx, dist and x overlap");
  if (device_form) {
    const size_t need = layout(n, k, *slices).total;
    if (overlap(ws, need, x, xb) || overlap(ws, need, idx, ob) || overlap(ws, need, dist, ob))
      GHS_FAIL(GHS_E_ARG, "the workspace overlaps x, idx or dist");
    if (ws_bytes < need) GHS_FAIL(GHS_E_NOMEM, "workspace too small");
  }
  return GHS_OK;
}

template <int KCAP>
static void launch_scan(dim3 grid, hipStream_t st, uint32_t n, uint32_t dim, uint32_t k, uint32_t metric, uint32_t slices,
                        const float *x, uint32_t *idx, float *dist, unsigned long long *parts, uint32_t *status) {
  k_knn_scan<KCAP><<<grid, KN_BLOCK, 0, st>>>(n, dim, k, metric, slices, x, idx, dist, parts, status);
}

}  // namespace knn
}  // namespace ghs

using namespace ghs;
using namespace ghs::knn;

extern "C" {

size_t ghs_knn_workspace_bytes(uint32_t n, uint32_t dim, uint32_t k, uint32_t slices) {
  if (n == 0 || dim == 0 || dim > GHS_KNN_MAX_DIM || k == 0 || k > GHS_KNN_MAX_K || slices > GHS_KNN_MAX_SLICES) return 0;
  if ((uint64_t)n * k >= (1ull << 32)) return 0;
  return layout(n, k, slices ? slices : auto_slices(n)).total;
}

int ghs_knn_device(uint32_t n, uint32_t dim, const float *d_x, uint32_t k, uint32_t metric, uint32_t slices, uint32_t *d_idx,
                   float *d_dist, void *d_workspace, size_t workspace_bytes, void *stream, ghs_knn_result_t *result) {
  hipStream_t st = (hipStream_t)stream;
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_knn_result_t{};
  if (int e = check_args(n, dim, d_x, k, metric, &slices, d_idx, d_dist, true, d_workspace, workspace_bytes)) return e;
  if (n == 0) return GHS_OK;
  if (int e = ghs::require_device()) return e;

  const auto t0 = std::chrono::steady_clock::now();
  const Layout l = layout(n, k, slices);
  char *base = (char *)d_workspace;
  uint32_t *status = (uint32_t *)(base + l.status);
  unsigned long long *parts = (unsigned long long *)(base + l.parts);
  GHS_HIP_CHECK(hipMemsetAsync(status, 0, 256, st));
  const dim3 grid(query_tiles(n), slices);
  if (k <= 16)
    launch_scan<16>(grid, st, n, dim, k, metric, slices, d_x, d_idx, d_dist, parts, status);
  else if (k <= 32)
    launch_scan<32>(grid, st, n, dim, k, metric, slices, d_x, d_idx, d_dist, parts, status);
  else if (k <= 64)
    launch_scan<64>(grid, st, n, dim, k, metric, slices, d_x, d_idx, d_dist, parts, status);
  else
    launch_scan<128>(grid, st, n, dim, k, metric, slices, d_x, d_idx, d_dist, parts, status);
  GHS_HIP_CHECK(hipGetLastError());
  if (slices > 1) {
    uint64_t g = ((uint64_t)n + 3) / 4;  // four waves, four queries per workgroup
    if (g > 4096) g = 4096;
    k_knn_merge<<<(unsigned)g, KN_BLOCK, 0, st>>>(n, k, metric, slices, parts, d_idx, d_dist, status);
    GHS_HIP_CHECK(hipGetLastError());
  }
  uint32_t hst[4] = {0};
  GHS_HIP_CHECK(hipMemcpyAsync(hst, status, sizeof(hst), hipMemcpyDeviceToHost, st));
  GHS_HIP_CHECK(hipStreamSynchronize(st));
  if (hst[ST_NONFINITE]) GHS_FAIL(GHS_E_ARG, "knn: non-finite coordinate (NaN or +-inf) in the points");
  if (hst[ST_BAD]) GHS_FAIL(GHS_E_STATE, "knn: a neighbour list came back short (internal error)");
  uint64_t zeros;
  memcpy(&zeros, hst + 2 * ST64_ZEROS, sizeof(zeros));
  result->pairs = (uint64_t)n * (n - 1);
  result->zero_neighbours = zeros;
  result->slices = slices;
  result->query_tiles = query_tiles(n);
  result->ms_total = ms_since(t0);
  return GHS_OK;
}

// Host-buffer form: copy in, run, copy out on the default stream
int ghs_knn_host(uint32_t n, uint32_t dim, const float *x, uint32_t k, uint32_t metric, uint32_t *idx, float *dist,
                 ghs_knn_result_t *result) {
  if (!result) GHS_FAIL(GHS_E_ARG, "result is NULL");
  *result = ghs_knn_result_t{};
  uint32_t slices = 0;
  if (int e = check_args(n, dim, x, k, metric, &slices, idx, dist, false, nullptr, 0)) return e;
  if (n == 0) return GHS_OK;
  if (int e = ghs::require_device()) return e;
  const size_t ws = ghs_knn_workspace_bytes(n, dim, k, 0);
  ghs::Staging s;
  const auto i_x = s.take<float>((size_t)n * dim);
  const auto o_idx = s.take<uint32_t>((size_t)n * k);
  const auto o_dist = s.take<float>((size_t)n * k);
  const auto d_ws = s.take<char>(ws);
  GHS_HIP_CHECK(s.alloc());
  hipStream_t st = nullptr;
  GHS_HIP_CHECK(s.up(i_x, x, st));
  const int rc = ghs_knn_device(n, dim, s.at(i_x), k, metric, 0, s.at(o_idx), s.at(o_dist), s.at(d_ws), ws, st, result);
  if (rc) return rc;
  GHS_HIP_CHECK(s.down(idx, o_idx, (size_t)n * k));
  GHS_HIP_CHECK(s.down(dist, o_dist, (size_t)n * k));
  return GHS_OK;
}

}  // extern "C"
