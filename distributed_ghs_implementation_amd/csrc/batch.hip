// Batched MSF solve (ABI 10 addition): many small graphs in one launch, one workgroup per graph.
//
// The level engine of boruvka.hip is built for one huge graph; the reference's own workload is the
// opposite shape (ghs_implementation.py main(): six Erdos-Renyi graphs of a few dozen vertices one
// after another). Here B graphs are concatenated ("batch-canonical": nvert[B], eoff[B + 1], u / v / w
// with ids local to each graph, each slice canonical on its own) and every graph is solved by ONE
// workgroup that keeps the whole fragment state in LDS:
//   s_par[NMAX]   every vertex's root (fully compressed between rounds)
//   s_best[NMAX]  this round's minimum outgoing key per root, (uint64)w << 32 | local eid (ds_min_u64)
// A round clears the best keys, streams the slice's edges (a small slice stays in L2), takes the
// LDS atomicMin at both ends' roots, hooks every root along its minimum edge (a mutual pair keeps
// its smaller root: the edge's flag is written and counted once) and jumps pointers in LDS until
// every vertex points at a root. No n-sized global array, no global atomic on the hot path, no host
// involvement until the batch is done. Keys are strictly ordered, so each graph's flags equal
// canonical Kruskal's bit for bit.
//
// Size classes (DESIGN.md "Batched solve"): a graph of 6 vertices must not reserve the LDS of one
// with 4096, so the kernel is instantiated per class and k_batch_classify builds one list of graph
// ids per class (+ counts) in the workspace. Each class runs as a fixed persistent grid (resident
// blocks per CU x 256 CUs, clamped by the host-known B); blocks take graphs from their class's list
// through a ticket (one global atomicAdd by one thread, broadcast through LDS), so uneven graphs
// balance. Nothing the host would have to read back sizes a grid: the device entry only enqueues.
#include <hip/hip_runtime.h>

#include <string>

#include "common.h"

using namespace ghs;

namespace {

constexpr int NCLASS = 3;
//                                   n <=   threads  LDS per block          blocks per CU (grid)
constexpr uint32_t CLS_N[NCLASS] = {64,  // 64       12 B x 64   = 768 B    16  (one wave: barriers are free)
                                    512,  // 256      12 B x 512  = 6 KiB    8
                                    GHS_BATCH_MAX_VERTICES};  // 1024  48 KiB  2   (32 waves per CU)
constexpr uint32_t CLS_T[NCLASS] = {64, 256, 1024};
constexpr uint32_t CLS_PER_CU[NCLASS] = {16, 8, 2};
constexpr uint32_t NUM_CU = 256;
constexpr uint32_t MAX_ROUNDS = 32;  // generous over ceil(log2 4096) = 12: a hang guard, never expected
constexpr uint32_t MAX_JUMPS = 16;   // pointer-jump sweeps per round (a 4096-chain needs 12 + 1)

constexpr size_t HDR_BYTES = 256;  // counts[NCLASS], tickets[NCLASS]
size_t list_stride(uint32_t B) { return ((size_t)B * 4 + 255) & ~(size_t)255; }

struct BatchArgs {
  const uint32_t *nvert, *eoff, *u, *v, *w;
  uint8_t *flags;
  ghs_batch_result_t *res;
  const uint32_t *list;   // this class's graph ids
  const uint32_t *count;  // ... how many
  uint32_t *ticket;
  uint32_t B;
};

__device__ __forceinline__ uint32_t class_of(uint32_t n) { return n <= CLS_N[0] ? 0u : n <= CLS_N[1] ? 1u : 2u; }

// One list of graph ids per class (order within a list is whatever the atomics give: results do not
// depend on it). Wave-aggregated: one atomicAdd per wave and class. A graph over the caps goes to
// the last class, whose kernel reports it (status 3) before any id indexes LDS.
__global__ __launch_bounds__(BLOCK) void k_batch_classify(const uint32_t *__restrict__ nvert, uint32_t B,
                                                          uint32_t *__restrict__ counts, uint32_t *__restrict__ lists,
                                                          uint32_t stride) {
  const uint32_t g = blockIdx.x * BLOCK + threadIdx.x;
  const bool ok = g < B;
  const uint32_t c = ok ? class_of(nvert[g]) : NCLASS;
  const uint32_t lane = threadIdx.x & (WAVE - 1);
#pragma unroll
  for (uint32_t k = 0; k < NCLASS; ++k) {
    const unsigned long long mask = __ballot(c == k);
    if (!mask) continue;
    uint32_t base = 0;
    if (lane == (uint32_t)__ffsll(mask) - 1) base = atomicAdd(&counts[k], (uint32_t)__popcll(mask));
    base = __shfl(base, __ffsll(mask) - 1);
    if (c == k) lists[(size_t)k * stride + base + __popcll(mask & ((1ull << lane) - 1))] = g;
  }
}

template <int NMAX, int T>
__global__ __launch_bounds__(T) void k_batch(BatchArgs a) {
  constexpr int PER = NMAX / T;  // vertices per thread
  __shared__ unsigned long long s_best[NMAX];
  __shared__ uint32_t s_par[NMAX];
  __shared__ unsigned long long s_tw;
  __shared__ uint32_t s_tc, s_g;
  const uint32_t tid = threadIdx.x;
  const uint32_t cnt = *a.count;
  const uint32_t M = a.eoff[a.B];
  const bool nullp = !a.u || !a.v || !a.w || !a.flags;
  for (;;) {
    __syncthreads();  // the last graph's LDS is no longer read
    if (tid == 0) {
      s_g = atomicAdd(a.ticket, 1u);
      s_tc = 0;
      s_tw = 0;
    }
    __syncthreads();
    if (s_g >= cnt) return;
    const uint32_t g = a.list[s_g];
    const uint32_t n = a.nvert[g], e0 = a.eoff[g], e1 = a.eoff[g + 1];
    uint32_t status = 0, rounds = 0;
    // ---- validation, before any id indexes LDS ------------------------------------------------
    if (e1 < e0 || e1 > M || (e1 > e0 && nullp)) {
      status = 1;  // offsets not monotone: the slice is not defined, nothing of it is touched
    } else if (n > GHS_BATCH_MAX_VERTICES || e1 - e0 > GHS_BATCH_MAX_EDGES || n > (uint32_t)NMAX) {
      status = 3;
      for (uint32_t e = e0 + tid; e < e1; e += T) a.flags[e] = 0;
    } else {
      int bad = 0;
      for (uint32_t e = e0 + tid; e < e1; e += T) {
        const uint32_t x = a.u[e], y = a.v[e];
        a.flags[e] = 0;  // every byte of the slice is written
        if (x >= y || y >= n) bad = 1;
        if (e > e0) {
          const uint32_t px = a.u[e - 1], py = a.v[e - 1];
          if (px > x || (px == x && py >= y)) bad = 1;
        }
      }
      if (__syncthreads_or(bad)) status = 1;
    }
    unsigned long long tw = 0;
    if (status == 0) {
#pragma unroll
      for (int q = 0; q < PER; ++q) {
        const uint32_t i = tid + q * T;
        if (i < n) s_par[i] = i;
      }
      for (;;) {
        if (rounds == MAX_ROUNDS) {
          status = 2;
          break;
        }
#pragma unroll
        for (int q = 0; q < PER; ++q) {
          const uint32_t i = tid + q * T;
          if (i < n) s_best[i] = KEY_NONE;
        }
        __syncthreads();
        // min outgoing edge of every root (edge-centric: an edge is a candidate for both ends)
        for (uint32_t e = e0 + tid; e < e1; e += T) {
          const uint32_t ra = s_par[a.u[e]], rb = s_par[a.v[e]];
          if (ra == rb) continue;
          const unsigned long long k = (unsigned long long)a.w[e] << 32 | (e - e0);
          if (k < s_best[ra]) atomicMin(&s_best[ra], k);
          if (k < s_best[rb]) atomicMin(&s_best[rb], k);
        }
        __syncthreads();
        ++rounds;
        // CONNECT: every root with an outgoing edge picks the root at its other end ...
        uint32_t tgt[PER];
        unsigned long long key[PER];
#pragma unroll
        for (int q = 0; q < PER; ++q) {
          const uint32_t i = tid + q * T;
          tgt[q] = LABEL_NONE;
          key[q] = KEY_NONE;
          if (i < n && s_par[i] == i && s_best[i] != KEY_NONE) {
            key[q] = s_best[i];
            const uint32_t e = e0 + (uint32_t)key[q];
            const uint32_t ra = s_par[a.u[e]], rb = s_par[a.v[e]];
            tgt[q] = ra == i ? rb : ra;
          }
        }
        __syncthreads();
        // ... and hooks to it; a mutual pair (both picked the same edge) keeps its smaller root
        uint32_t hooks = 0;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
          const uint32_t i = tid + q * T, o = tgt[q];
          if (o != LABEL_NONE && !(s_best[o] == key[q] && i < o)) {
            s_par[i] = o;
            a.flags[e0 + (uint32_t)key[q]] = 1;
            tw += key[q] >> 32;
            ++hooks;
          }
        }
        const int any = hooks != 0;
        for (int dd = WAVE / 2; dd > 0; dd >>= 1) hooks += __shfl_xor(hooks, dd);
        if ((tid & (WAVE - 1)) == 0 && hooks) atomicAdd(&s_tc, hooks);
        if (!__syncthreads_or(any)) break;   // no root found an outgoing edge: the forest is complete
        if (s_tc + 1 == n) break;            // a spanning tree: no further scan needed
        // INITIATE: pointer jumping until every vertex points at a root
        uint32_t it = 0;
        for (; it < MAX_JUMPS; ++it) {
          int more = 0;
#pragma unroll
          for (int q = 0; q < PER; ++q) {
            const uint32_t i = tid + q * T;
            if (i < n) {
              const uint32_t p = s_par[i], pp = s_par[p];
              if (pp != p) {
                s_par[i] = pp;
                more = 1;
              }
            }
          }
          if (!__syncthreads_or(more)) break;
        }
        if (it == MAX_JUMPS) {
          status = 2;
          break;
        }
      }
    }
    for (int dd = WAVE / 2; dd > 0; dd >>= 1) tw += __shfl_xor(tw, dd);
    if ((tid & (WAVE - 1)) == 0 && tw) atomicAdd(&s_tw, tw);
    __syncthreads();
    if (tid == 0) {
      ghs_batch_result_t r;
      r.total_weight = s_tw;
      r.num_mst_edges = s_tc;
      r.rounds = rounds;
      r.status = status;
      r.reserved = 0;
      a.res[g] = r;
    }
  }
}

template <int C>
void launch_class(BatchArgs a, uint32_t B, hipStream_t st) {
  const uint32_t full = CLS_PER_CU[C] * NUM_CU;
  k_batch<(int)CLS_N[C], (int)CLS_T[C]><<<B < full ? B : full, CLS_T[C], 0, st>>>(a);
}

}  // namespace

extern "C" size_t ghs_batch_workspace_bytes(uint32_t num_graphs) {
  return HDR_BYTES + NCLASS * list_stride(num_graphs);
}

extern "C" int ghs_mst_batch_device(uint32_t num_graphs, const uint32_t *d_nvert, const uint32_t *d_eoff,
                                    const uint32_t *d_u, const uint32_t *d_v, const uint32_t *d_w, void *d_workspace,
                                    size_t workspace_bytes, uint8_t *d_in_mst, ghs_batch_result_t *d_results,
                                    void *stream) {
  if (num_graphs == 0) return GHS_OK;
  if (!d_nvert || !d_eoff || !d_results || !d_workspace) GHS_FAIL(GHS_E_ARG, "NULL device pointer");
  if (((uintptr_t)d_u | (uintptr_t)d_v | (uintptr_t)d_w) & 15) GHS_FAIL(GHS_E_ARG, "u, v, w must be 16-byte aligned");
  if (((uintptr_t)d_workspace & 15) || ((uintptr_t)d_results & 7)) GHS_FAIL(GHS_E_ARG, "misaligned workspace / results");
  if (workspace_bytes < ghs_batch_workspace_bytes(num_graphs)) GHS_FAIL(GHS_E_NOMEM, "batch workspace too small");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) GHS_FAIL(GHS_E_NODEVICE, "no HIP device");
  hipStream_t st = (hipStream_t)stream;
  const uint32_t B = num_graphs;
  const uint32_t stride = (uint32_t)(list_stride(B) / 4);
  uint32_t *counts = (uint32_t *)d_workspace, *tickets = counts + NCLASS;
  uint32_t *lists = (uint32_t *)((char *)d_workspace + HDR_BYTES);
  GHS_HIP_CHECK(hipMemsetAsync(d_workspace, 0, HDR_BYTES, st));
  k_batch_classify<<<(B + BLOCK - 1) / BLOCK, BLOCK, 0, st>>>(d_nvert, B, counts, lists, stride);
  BatchArgs a{d_nvert, d_eoff, d_u, d_v, d_w, d_in_mst, d_results, nullptr, nullptr, nullptr, B};
  auto cls = [&](uint32_t c) {
    BatchArgs x = a;
    x.list = lists + (size_t)c * stride;
    x.count = counts + c;
    x.ticket = tickets + c;
    return x;
  };
  // the largest class first: its few long blocks start while nothing else holds the CUs
  launch_class<2>(cls(2), B, st);
  launch_class<1>(cls(1), B, st);
  launch_class<0>(cls(0), B, st);
  GHS_HIP_CHECK(hipGetLastError());
  return GHS_OK;
}

extern "C" int ghs_mst_batch_host(uint32_t num_graphs, const uint32_t *nvert, const uint32_t *eoff, const uint32_t *u,
                                  const uint32_t *v, const uint32_t *w, uint8_t *in_mst, ghs_batch_result_t *results) {
  if (num_graphs == 0) return GHS_OK;
  if (!nvert || !eoff || !results) GHS_FAIL(GHS_E_ARG, "NULL host pointer");
  const uint32_t B = num_graphs;
  const size_t M = eoff[B];
  if (M >= (1ull << 31)) GHS_FAIL(GHS_E_ARG, "the batch's edge count must be < 2^31");
  if (M && (!u || !v || !w || !in_mst)) GHS_FAIL(GHS_E_ARG, "NULL host pointer");
  if (int e = ghs::require_device()) return e;
  const size_t ws = ghs_batch_workspace_bytes(B);
  ghs::Staging dev;
  const auto d_n = dev.take<uint32_t>(B), d_e = dev.take<uint32_t>((size_t)B + 1);
  const auto d_u = dev.take<uint32_t>(M), d_v = dev.take<uint32_t>(M), d_w = dev.take<uint32_t>(M);
  const auto d_f = dev.take<uint8_t>(M);
  const auto d_r = dev.take<ghs_batch_result_t>(B);
  const auto d_ws = dev.take<char>(ws);
  if (dev.alloc() != hipSuccess) {
    (void)hipGetLastError();
    GHS_FAIL(GHS_E_NOMEM, "hipMalloc of the batch buffers failed");
  }
  hipStream_t st = nullptr;
  GHS_HIP_CHECK(dev.up(d_n, nvert, st));
  GHS_HIP_CHECK(dev.up(d_e, eoff, st));
  GHS_HIP_CHECK(dev.up(d_u, u, st));
  GHS_HIP_CHECK(dev.up(d_v, v, st));
  GHS_HIP_CHECK(dev.up(d_w, w, st));
  // a slice behind non-monotone offsets is never written by the kernel: its flags read 0
  if (M) GHS_HIP_CHECK(hipMemsetAsync(dev.at(d_f), 0, M, st));
  int rc = ghs_mst_batch_device(B, dev.at(d_n), dev.at(d_e), dev.at(d_u), dev.at(d_v), dev.at(d_w), dev.at(d_ws), ws,
                                dev.at(d_f), dev.at(d_r), st);
  if (rc) return rc;
  GHS_HIP_CHECK(dev.down(in_mst, d_f, M));
  GHS_HIP_CHECK(dev.down(results, d_r, B));
  for (uint32_t g = 0; g < B; ++g) {
    const uint32_t s = results[g].status;
    if (s == 1) GHS_FAIL(GHS_E_NONCANON, "batch graph " + std::to_string(g) + ": edge slice is not canonical");
    if (s == 2) GHS_FAIL(GHS_E_ROUNDCAP, "batch graph " + std::to_string(g) + ": round cap exceeded");
    if (s != 0)
      GHS_FAIL(GHS_E_ARG, "batch graph " + std::to_string(g) + ": over GHS_BATCH_MAX_VERTICES / GHS_BATCH_MAX_EDGES");
  }
  return GHS_OK;
}
