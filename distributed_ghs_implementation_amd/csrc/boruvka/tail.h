// Part of boruvka.hip (included there once, inside namespace ghs; not a stand-alone header).
// The LDS tail of a level, device side: TailCtl / TailBufs / TailRun, k_tail_map, k_tail_labels,
// k_tail_open, k_tail_hook, k_tail_xhook, k_tail_round, k_tail_report. Relies on what precedes its
// include in boruvka.hip: the block offsets and LDS helpers, SegView, RoundSlot / write_report.

// ------------------------------------------------------------------------------------------
// The LDS tail of a level (one rank). Once a level's active fragments fit a workgroup's LDS
// (<= TAIL_MAX), its remaining rounds — the reference's last TEST / REPORT / CHANGEROOT /
// INITIATE exchanges of a level, ghs_implementation.py:235-387 — run without any global atomic and
// without n-sized arrays: the fragments get dense ids 0..F0-1 (their order in the active list),
// every edge is relabelled ONCE to the dense pair of its fragments, and each later round keeps
// every root's minimum in LDS per block.
//   k_tail_map    dmap[act[i]] = i; the tail's control block, R = identity, the root list
//   k_tail_open   (round 0 of the tail) every live edge: a, b -> dmap (its dense fragments);
//                 intra-fragment edges dropped, the rest compacted in order to the block's region of
//                 the tail buffer as one 12-byte record (da | db << 16, key); each end's candidate
//                 min'ed into the block's LDS minima; the block's row: each minimum's key and other end
//   k_tail_hook   one slot per active root: the minimum over the blocks' rows and its other end
//                 (the CONNECT target), the MSF flag of the edge
//   k_tail_round  every block applies the last round's hooks in LDS — over the ROOTS only: mutual
//                 pairs keep the smaller root, pointer jumping among the roots, then every dense id's
//                 root through one lookup (R[d] = P[R[d]]), the next root list — identically in every
//                 block (no grid barrier: the launch boundaries order open -> hook -> round -> hook,
//                 so ranks sharing a device cannot deadlock it), then streams its records (a
//                 candidate only where R[da] != R[db]) into its LDS minima and row. A round that
//                 starts with <= 1 active root finishes the level instead: lab of every fragment of
//                 the level = its final root, the round report.
// The LDS minima carry (w << 32 | the record's index in the block's region) instead of the key:
// a block's region holds its records in canonical (eid) order — a level's live edges keep the
// canonical order within and across their regions (k_select / k_filter / k_level_pass emit it,
// every compaction keeps it) and the open compacts in order — so within a block that order IS the
// (w, eid) order, and each minimum's record is one load away: its true key for the row and its
// other end. (Round 4's hook found the other end through the canonical list and the label chains,
// and its prologue jumped pointers over all F0 dense ids.)
// Per round: one stream of the 12-byte records + two launch boundaries, instead of the round
// kernels' relabel gathers, LDS-cache misses to best[], hook, jump and select over n-sized arrays.
// ------------------------------------------------------------------------------------------
constexpr uint32_t TAIL_MAX = 12288;        // dense fragments: LDS minima 96 KiB + 2 x 24 KiB of u16 tables
constexpr uint32_t TAIL_T = 1024;           // threads of the streaming tail kernels (16 waves, 1 block per CU)
constexpr uint32_t TAIL_G = 256;            // their blocks = rows of `partial`
constexpr uint32_t TAIL_ROUNDS_MAX = 32;    // a tail round at least halves the roots: <= 14 rounds
constexpr uint32_t TAIL_HS = 16;            // k_tail_hook: slots per 256-thread block (16 row groups)
constexpr uint16_t TAIL_NONE = 0xffffu;     // a row's other end where the block has no candidate
static_assert(TAIL_MAX <= 32768, "dense ids are packed as 16-bit pairs");

struct TailCtl {
  uint32_t F0;        // dense fragments (the active list at the tail's start)
  uint32_t done;      // the level is complete (lab written)
  uint32_t rounds;    // tail rounds streamed (set when done)
  uint32_t err;
  uint64_t Q;         // each block's region stride in the tail buffer
  uint64_t nroots[TAIL_ROUNDS_MAX + 1];  // active roots of round r (its list: droot[r & 1])
  uint64_t live[TAIL_ROUNDS_MAX];        // live (inter-fragment) edges round r scanned
  uint64_t edges[TAIL_ROUNDS_MAX];       // MSF edges (C_EDGES) once round r's hooks are counted
};

struct TailBufs {
  TailCtl *ctl;
  uint32_t *dmap;      // root label -> dense id (n entries; only the tail's roots are meaningful)
  uint64_t *partial;   // TAIL_G rows x TAIL_MAX block minima (root-list order)
  uint16_t *poth;      // ... and each minimum's other end (dense root id at the time of the stream)
  uint32_t *R[2];      // dense id -> dense root during round r: R[r & 1]
  uint32_t *droot[2];  // round r's active roots (ascending dense ids): droot[r & 1]
  uint32_t *ghook;     // per dense root: CONNECT target (dense root) of its minimum edge
  uint64_t *gkey;      // per dense root: its minimum key (KEY_NONE: no outgoing edge)
  uint64_t *gloc;      // several ranks: this rank's own minimum (gkey is then MIN-all-reduced)
  uint32_t *blive;     // per block: live edges of the round it streamed
  uint32_t *bcnt;      // per block: records in its region of the tail buffer
  uint32_t *rec;       // the tail buffer: da | db << 16
  uint64_t *rkey;      //   ... and the key
};

// A tail in progress (run_tail's batches, or the stepwise ghs_solver_tail_* calls of several ranks)
struct TailRun {
  TailBufs tb{};
  const uint32_t *act0 = nullptr;
  uint32_t F0 = 0, round0 = 0, lr0 = 0, r = 1;  // r: the next tail round to stream
  unsigned hook_g = 1;
  bool multi = false;
};

__global__ void k_tail_map(const uint32_t *__restrict__ act, const unsigned long long *__restrict__ d_nact, TailBufs tb) {
  const uint32_t F = (uint32_t)*d_nact;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < F; i += gridDim.x * blockDim.x) {
    tb.dmap[act[i]] = i;
    tb.R[0][i] = i;
    tb.droot[0][i] = i;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    TailCtl *c = tb.ctl;
    c->F0 = F;
    c->done = 0;
    c->rounds = 0;
    c->err = 0;
    c->nroots[0] = F;
  }
}

// The labels the live edges carry (the previous round's active list, or every vertex after a
// level's identity round) -> the dense id of their fragment now: dmap[x] = dmap[lab[x]] (one hop:
// lab of those labels is current; a root's own entry is k_tail_map's and is not rewritten here),
// so k_tail_open relabels an end with ONE gather.
__global__ void k_tail_labels(const uint32_t *__restrict__ prev, const unsigned long long *__restrict__ d_nprev,
                              const uint32_t *__restrict__ lab, TailBufs tb) {
  const uint64_t np = *d_nprev;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < np; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t x = prev ? prev[i] : (uint32_t)i;
    const uint32_t l = lab[x];
    if (l != x) tb.dmap[x] = tb.dmap[l];
  }
}

__device__ __forceinline__ void lds_min_u64(unsigned long long *s, uint32_t i, uint64_t k) {
  if (k < s[i]) atomicMin(&s[i], (unsigned long long)k);  // a plain read first: slots only decrease
}

// a wave's survivors staged in LDS for coalesced stores (12-byte records)
struct TailStage {
  uint32_t p[WAVE * 4];
  uint64_t k[WAVE * 4];
};

// a block-local candidate: the key's weight with the record's index in the block's region (the
// region is in eid order, so this orders the block's candidates exactly as (w, eid))
__device__ __forceinline__ uint64_t tail_local(uint64_t key, uint32_t idx) { return (key & ~0xffffffffull) | idx; }

// The block's row (root-list order: root i of the round = droots[i]): each root's minimum
// record (one load: its index is in the LDS minimum) gives the true key and the other end's dense
// root (through R: rmap == nullptr is the identity, the open). Every record load in flight first.
__device__ __forceinline__ void tail_row_out(const TailBufs tb, const unsigned long long *s_best, const uint16_t *droots,
                                             uint32_t nroot, const uint32_t *__restrict__ pr, const uint64_t *__restrict__ pk,
                                             const uint16_t *rmap) {
  constexpr uint32_t PER = TAIL_MAX / TAIL_T;
  uint64_t *row = tb.partial + (uint64_t)blockIdx.x * TAIL_MAX;
  uint16_t *orow = tb.poth + (uint64_t)blockIdx.x * TAIL_MAX;
  uint32_t p[PER], d[PER];
  uint64_t k[PER];
#pragma unroll
  for (uint32_t q = 0; q < PER; ++q) {
    const uint32_t i = threadIdx.x + q * TAIL_T;
    d[q] = i < nroot ? (droots ? droots[i] : i) : 0u;
    const uint64_t v = i < nroot ? s_best[d[q]] : KEY_NONE;
    const bool has = v != KEY_NONE;
    p[q] = has ? pr[(uint32_t)v] : 0u;
    k[q] = has ? pk[(uint32_t)v] : KEY_NONE;
  }
#pragma unroll
  for (uint32_t q = 0; q < PER; ++q) {
    const uint32_t i = threadIdx.x + q * TAIL_T;
    if (i >= nroot) break;
    uint16_t o = TAIL_NONE;
    if (k[q] != KEY_NONE) {
      const uint32_t da = p[q] & 0xffffu, db = p[q] >> 16;
      const uint32_t ra = rmap ? rmap[da] : da, rb = rmap ? rmap[db] : db;
      o = (uint16_t)(ra == d[q] ? rb : ra);
    }
    row[i] = k[q];
    orow[i] = o;
  }
}

// check (GHS_OPT_CHECK_TOTALS): verify the invariant the (w, index) minima rest on — the
// block's region holds its records in strictly increasing eid order — after writing it
__global__ __launch_bounds__(TAIL_T) void k_tail_open(const uint32_t *__restrict__ src, const uint32_t *__restrict__ dst,
                                                      const uint64_t *__restrict__ key, SegView in, TailBufs tb,
                                                      bool check) {
  __shared__ unsigned long long s_best[TAIL_MAX];
  __shared__ TailStage s_stage[TAIL_T / WAVE];
  __shared__ uint32_t s_wcnt[TAIL_T / WAVE];
  __shared__ uint32_t s_seg[2];
  __shared__ uint32_t s_live;
  const uint32_t F = tb.ctl->F0;
  for (uint32_t i = threadIdx.x; i < F; i += TAIL_T) s_best[i] = KEY_NONE;
  const uint64_t T = in.prefix[in.nseg];
  const uint64_t Q = ((T + gridDim.x - 1) / gridDim.x + 3) & ~3ull;
  const uint64_t vb = Q * blockIdx.x;
  const uint64_t ve = (vb + Q < T) ? vb + Q : T;
  if (threadIdx.x < WAVE) seg_range_wave(in.prefix, in.nseg, vb, ve, T, s_seg);
  if (threadIdx.x == 0) {
    s_live = 0;
    if (blockIdx.x == 0) tb.ctl->Q = Q;
  }
  __syncthreads();
  const uint32_t slo = s_seg[0], shi = s_seg[1];
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  uint32_t *orec = tb.rec + vb;
  uint64_t *okey = tb.rkey + vb;
  constexpr uint64_t STEP = (uint64_t)TAIL_T * 4;
  uint32_t out_n = 0, live_n = 0;
  for (uint64_t v0 = vb; v0 < ve; v0 += STEP) {
    const uint64_t v = v0 + (uint64_t)threadIdx.x * 4;
    const bool in_range = v < ve;
    const uint64_t ph = tile_phys(in, slo, shi, v, ve);
    const uint4 a4 = *reinterpret_cast<const uint4 *>(src + ph), b4 = *reinterpret_cast<const uint4 *>(dst + ph);
    const ulonglong2 k01 = *reinterpret_cast<const ulonglong2 *>(key + ph),
                     k23 = *reinterpret_cast<const ulonglong2 *>(key + ph + 2);
    const uint32_t A[4] = {a4.x, a4.y, a4.z, a4.w}, B[4] = {b4.x, b4.y, b4.z, b4.w};
    const uint64_t K[4] = {k01.x, k01.y, k23.x, k23.y};
    uint32_t da[4], db[4], mask = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // the dense fragments now (k_tail_labels: one gather per end)
      const bool valid = in_range & (A[j] != LABEL_NONE);
      da[j] = tb.dmap[valid ? A[j] : 0u];
      db[j] = tb.dmap[valid ? B[j] : 0u];
      mask |= (valid & (da[j] != db[j])) ? (1u << j) : 0u;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (((mask >> j) & 1u) && (da[j] >= F || db[j] >= F)) {  // a live edge must join two active fragments
        atomicOr(&tb.ctl->err, 1u);
        mask &= ~(1u << j);
      }
    live_n += __popc(mask);
    // survivors -> this block's region of the tail buffer, in order; their candidates carry their index
    uint32_t lane_excl, wave_before, wave_cnt, total;
    block_offsets_w<TAIL_T>((uint32_t)__popc(mask), s_wcnt, &lane_excl, &wave_before, &wave_cnt, &total);
    TailStage &ws = s_stage[wid];
    uint32_t o = lane_excl;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((mask >> j) & 1u) {
        ws.p[o] = da[j] | (db[j] << 16);
        ws.k[o] = K[j];
        const uint64_t c = tail_local(K[j], out_n + wave_before + o);
        lds_min_u64(s_best, da[j], c);
        lds_min_u64(s_best, db[j], c);
        ++o;
      }
    wave_sync_lds();  // the wave's records leave LDS as consecutive stores
    for (uint32_t i = lane; i < wave_cnt; i += WAVE) {
      orec[out_n + wave_before + i] = ws.p[i];
      okey[out_n + wave_before + i] = ws.k[i];
    }
    wave_sync_lds();
    out_n += total;
  }
  for (int d = WAVE / 2; d > 0; d >>= 1) live_n += __shfl_xor(live_n, d);
  if ((threadIdx.x & (WAVE - 1)) == 0) atomicAdd(&s_live, live_n);
  __syncthreads();  // every wave's record stores drained: the row reads them back through L2
  if (check)
    for (uint32_t i = threadIdx.x + 1; i < out_n; i += TAIL_T)
      if ((uint32_t)okey[i - 1] >= (uint32_t)okey[i]) atomicOr(&tb.ctl->err, 1u);
  // the block's minima of every dense fragment (round 0: the root list is the identity)
  tail_row_out(tb, s_best, nullptr, F, orec, okey, nullptr);
  if (threadIdx.x == 0) {
    tb.bcnt[blockIdx.x] = out_n;
    tb.blive[blockIdx.x] = s_live;
  }
}

// One active root per slot (root-list order): the blocks' minima reduced (16 row groups per slot)
// with their other ends, the root's CONNECT target, its MSF flag. Block 0 also totals the
// streamed round's live edges.
// several ranks (multi): the minimum is this rank's only — kept in gloc as well, no MSF flag yet
// (k_tail_xhook writes it once the ranks agree on the minimum)
__global__ __launch_bounds__(256) void k_tail_hook(TailBufs tb, uint32_t r, uint8_t *__restrict__ in_mst,
                                                   uint32_t nblocks, unsigned long long *__restrict__ err,
                                                   bool multi) {
  __shared__ unsigned long long s_part[256];
  __shared__ uint32_t s_prow[256];
  TailCtl *c = tb.ctl;
  if (c->done) return;  // r: the round just streamed
  const uint32_t nroot = (uint32_t)c->nroots[r];
  if (blockIdx.x == 0 && threadIdx.x < WAVE) {
    uint64_t t = 0;
    for (uint32_t b = threadIdx.x; b < nblocks; b += WAVE) t += tb.blive[b];
    for (int d = WAVE / 2; d > 0; d >>= 1) t += __shfl_xor(t, d);
    if (threadIdx.x == 0) c->live[r] = t;
  }
  const uint32_t s = threadIdx.x % TAIL_HS, g = threadIdx.x / TAIL_HS;  // slot, row group
  const uint32_t i = blockIdx.x * TAIL_HS + s;
  if (blockIdx.x * TAIL_HS >= nroot) return;  // block-uniform
  constexpr uint32_t GROUPS = 256 / TAIL_HS;
  uint64_t m = KEY_NONE;
  uint32_t w = 0;
  if (i < nroot) {
    uint64_t x[TAIL_G / GROUPS];
#pragma unroll
    for (uint32_t k = 0; k < TAIL_G / GROUPS; ++k) {
      const uint32_t b = g + k * GROUPS;
      x[k] = b < nblocks ? tb.partial[(uint64_t)b * TAIL_MAX + i] : KEY_NONE;
    }
#pragma unroll
    for (uint32_t k = 0; k < TAIL_G / GROUPS; ++k)
      if (x[k] < m) {
        m = x[k];
        w = g + k * GROUPS;
      }
  }
  s_part[threadIdx.x] = m;
  s_prow[threadIdx.x] = w;
  __syncthreads();
  if (g != 0 || i >= nroot) return;
  for (uint32_t k = 1; k < GROUPS; ++k) {
    const uint64_t x = s_part[k * TAIL_HS + s];
    if (x < m) {
      m = x;
      w = s_prow[k * TAIL_HS + s];
    }
  }
  const uint32_t d = tb.droot[r & 1][i];
  uint32_t o = LABEL_NONE;
  if (m != KEY_NONE) {
    o = tb.poth[(uint64_t)w * TAIL_MAX + i];
    if (o >= c->F0 || o == d) {  // the minimum edge must leave root d towards another root
      atomicOr(err, 2ull);
      o = LABEL_NONE;
      m = KEY_NONE;
    } else if (!multi) {
      in_mst[(uint32_t)m] = 1;  // both members of a mutual pair mark the same edge
    }
  }
  tb.gkey[d] = m;
  tb.ghook[d] = o;
  if (multi) tb.gloc[d] = m;
}

// Several ranks, between the MIN all-reduce of gkey and the MAX all-reduce of ghook: a root whose
// global minimum is this rank's own keeps its CONNECT target (and the owner writes the MSF flag of
// its own edge); every other root's target is withdrawn (LABEL_NONE = -1 under the int32 MAX), so
// the all-reduce leaves the owner's target on every rank. Keys are (w << 32 | global eid): unique.
__global__ __launch_bounds__(256) void k_tail_xhook(TailBufs tb, uint32_t r, uint8_t *__restrict__ in_mst,
                                                    uint32_t e_lo, uint32_t e_hi) {
  const TailCtl *c = tb.ctl;
  if (c->done) return;
  const uint32_t nroot = (uint32_t)c->nroots[r];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nroot; i += gridDim.x * blockDim.x) {
    const uint32_t d = tb.droot[r & 1][i];
    const uint64_t g = tb.gkey[d];
    if (g != KEY_NONE && g == tb.gloc[d]) {
      const uint32_t eid = (uint32_t)g;
      if (eid >= e_lo && eid < e_hi) in_mst[eid] = 1;
    } else {
      tb.ghook[d] = LABEL_NONE;
    }
  }
}

// Every block applies the last round's hooks (identical LDS computation in every block, over the
// roots only), then streams its records — or, when <= 1 root stays active, block 0 finishes the level.
__global__ __launch_bounds__(TAIL_T) void k_tail_round(TailBufs tb, uint32_t r, const uint32_t *__restrict__ act0,
                                                       uint32_t *__restrict__ lab, unsigned long long *__restrict__ cnt,
                                                       unsigned long long *__restrict__ err) {
  __shared__ unsigned long long s_best[TAIL_MAX];  // the prologue's pointer table first (u32 view)
  __shared__ uint16_t s_R[TAIL_MAX];
  __shared__ uint16_t s_root[TAIL_MAX];
  __shared__ uint32_t s_wsum[TAIL_T / WAVE];
  __shared__ unsigned long long s_tw, s_tc;
  __shared__ uint32_t s_live;
  TailCtl *c = tb.ctl;
  if (c->done) return;
  const uint32_t F = c->F0;  // r: the round about to stream (round r - 1 hooked last)
  const uint32_t nprev = (uint32_t)c->nroots[r - 1];
  const uint32_t *prev = tb.droot[(r - 1) & 1];
  uint32_t *P = reinterpret_cast<uint32_t *>(s_best);  // dense pointer forest over the roots (prologue only)
  constexpr uint32_t MARK = 0x80000000u;
  if (threadIdx.x == 0) {
    s_tw = 0;
    s_tc = 0;
    s_live = 0;
  }
  // every global load of the prologue first: the dense ids' roots, the roots' hooks and keys
  constexpr uint32_t PER = TAIL_MAX / TAIL_T;
  const uint32_t *Rp = tb.R[(r - 1) & 1];
  uint32_t rr[PER], pd[PER], ph[PER];
  uint64_t pk[PER];
#pragma unroll
  for (uint32_t q = 0; q < PER; ++q) {
    const uint32_t d = threadIdx.x + q * TAIL_T, i = d;
    rr[q] = d < F ? Rp[d] : 0u;
    pd[q] = i < nprev ? prev[i] : 0u;
  }
#pragma unroll
  for (uint32_t q = 0; q < PER; ++q) {
    const uint32_t i = threadIdx.x + q * TAIL_T;
    ph[q] = i < nprev ? tb.ghook[pd[q]] : LABEL_NONE;
    pk[q] = i < nprev ? tb.gkey[pd[q]] : KEY_NONE;
  }
  // every dense id a root of itself (an inactive root of round r - 1 stays one), then the hooks of
  // round r - 1's active roots
  for (uint32_t d = threadIdx.x; d < F; d += TAIL_T) P[d] = d;
  __syncthreads();
#pragma unroll
  for (uint32_t q = 0; q < PER; ++q) {
    const uint32_t i = threadIdx.x + q * TAIL_T;
    if (i < nprev && ph[q] != LABEL_NONE) P[pd[q]] = ph[q];
  }
  __syncthreads();
  // a mutual pair (d <-> o over their shared minimum) keeps its smaller member as the root
#pragma unroll
  for (uint32_t q = 0; q < PER; ++q) {
    const uint32_t i = threadIdx.x + q * TAIL_T;
    if (i < nprev) {
      const uint32_t d = pd[q], o = P[d] & ~MARK;
      if (o != d && (P[o] & ~MARK) == d && d < o) atomicOr(&P[d], MARK);
    }
  }
  __syncthreads();
  unsigned long long tw = 0, tc = 0;
#pragma unroll
  for (uint32_t q = 0; q < PER; ++q) {
    const uint32_t i = threadIdx.x + q * TAIL_T;
    if (i < nprev) {
      const uint32_t d = pd[q];
      if (P[d] & MARK) {
        P[d] = d;
      } else if (P[d] != d) {  // d hooked: one MSF edge
        tw += pk[q] >> 32;
        tc += 1;
      }
    }
  }
  __syncthreads();
  for (int it = 0; it < 32; ++it) {  // pointer jumping among the roots (a hook targets a root)
    int more = 0;
#pragma unroll
    for (uint32_t q = 0; q < PER; ++q) {
      const uint32_t i = threadIdx.x + q * TAIL_T;
      if (i < nprev) {
        const uint32_t d = pd[q], p = P[d], pp = P[p];
        if (pp != p) {
          P[d] = pp;
          more = 1;
        }
      }
    }
    if (!__syncthreads_or(more)) break;
  }
  // every dense id's root: its round r - 1 root's final root (a root that was not active keeps itself)
#pragma unroll
  for (uint32_t q = 0; q < PER; ++q) {
    const uint32_t d = threadIdx.x + q * TAIL_T;
    if (d < F) s_R[d] = (uint16_t)P[rr[q]];
  }
  // next roots: round r - 1's roots that had an edge and stayed roots (ascending: a block scan)
  uint32_t keep = 0;
#pragma unroll
  for (uint32_t q = 0; q < PER; ++q) {
    const uint32_t i = threadIdx.x + q * TAIL_T;
    if (i < nprev && pk[q] != KEY_NONE && P[pd[q]] == pd[q]) keep |= 1u << q;
  }
  uint32_t nroot = 0;
#pragma unroll
  for (uint32_t q = 0; q < PER; ++q) {  // root-list order = prev order (chunks of TAIL_T)
    if (q * TAIL_T < nprev) {  // block-uniform
      uint32_t tot;
      const uint32_t k = (keep >> q) & 1u;
      const uint32_t before = block_excl_scan<TAIL_T>(k, s_wsum, &tot);
      if (k) s_root[nroot + before] = (uint16_t)pd[q];
      nroot += tot;
    }
  }
  for (int dd = WAVE / 2; dd > 0; dd >>= 1) {
    tw += __shfl_xor(tw, dd);
    tc += __shfl_xor(tc, dd);
  }
  if ((threadIdx.x & (WAVE - 1)) == 0 && tc) {
    atomicAdd(&s_tw, tw);
    atomicAdd(&s_tc, tc);
  }
  __syncthreads();
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) {
      if (s_tc) {
        (void)atomicAdd(cnt + 2, s_tw);  // C_WEIGHT, C_EDGES (returning: complete before the report)
        (void)atomicAdd(cnt + 3, s_tc);
      }
      const unsigned long long edges = __hip_atomic_load(cnt + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      c->edges[r - 1] = edges;
    }
    if (nroot <= 1 || r >= TAIL_ROUNDS_MAX) {
      // the level is complete: every fragment of the level takes its final root's label
      uint32_t xs[PER], roots[PER];
#pragma unroll
      for (uint32_t q = 0; q < PER; ++q) {  // every gather in flight, then the stores
        const uint32_t d = threadIdx.x + q * TAIL_T;
        xs[q] = d < F ? act0[d] : 0u;
        roots[q] = d < F ? act0[s_R[d]] : 0u;
      }
#pragma unroll
      for (uint32_t q = 0; q < PER; ++q) {
        const uint32_t d = threadIdx.x + q * TAIL_T;
        if (d < F && roots[q] != xs[q]) lab[xs[q]] = roots[q];
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        if (r >= TAIL_ROUNDS_MAX && nroot > 1) atomicOr(err, 4ull);
        if (c->err) atomicOr(err, 2ull);
        c->done = 1;
        c->rounds = r;
        cnt[0] = 0;  // C_LIVE: no live edge left in the level
      }
      return;
    }
    for (uint32_t d = threadIdx.x; d < F; d += TAIL_T) tb.R[r & 1][d] = s_R[d];
    for (uint32_t i = threadIdx.x; i < nroot; i += TAIL_T) tb.droot[r & 1][i] = s_root[i];
    if (threadIdx.x == 0) c->nroots[r] = nroot;
  }
  if (nroot <= 1 || r >= TAIL_ROUNDS_MAX) return;  // block 0 finishes the level
  // stream this block's records into the LDS minima of the current roots
  for (uint32_t i = threadIdx.x; i < nroot; i += TAIL_T) s_best[s_root[i]] = KEY_NONE;
  __syncthreads();
  const uint64_t base = c->Q * blockIdx.x;
  const uint32_t n = tb.bcnt[blockIdx.x];
  const uint32_t *pr = tb.rec + base;
  const uint64_t *prk = tb.rkey + base;
  uint32_t live_n = 0;
  for (uint32_t e0 = threadIdx.x * 4; e0 < n; e0 += TAIL_T * 4) {
    uint32_t p[4];
    uint64_t k[4];
    if (e0 + 4 <= n) {  // a region starts at a multiple of 4: 16-B aligned
      const uint4 qv = *reinterpret_cast<const uint4 *>(pr + e0);
      const ulonglong2 k01 = *reinterpret_cast<const ulonglong2 *>(prk + e0), k23 = *reinterpret_cast<const ulonglong2 *>(prk + e0 + 2);
      p[0] = qv.x; p[1] = qv.y; p[2] = qv.z; p[3] = qv.w;
      k[0] = k01.x; k[1] = k01.y; k[2] = k23.x; k[3] = k23.y;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        p[j] = e0 + j < n ? pr[e0 + j] : 0u;
        k[j] = e0 + j < n ? prk[e0 + j] : KEY_NONE;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (e0 + j >= n) continue;
      const uint32_t ra = s_R[p[j] & 0xffffu], rb = s_R[p[j] >> 16];
      if (ra == rb) continue;
      ++live_n;
      const uint64_t cand = tail_local(k[j], e0 + j);
      lds_min_u64(s_best, ra, cand);
      lds_min_u64(s_best, rb, cand);
    }
  }
  for (int dd = WAVE / 2; dd > 0; dd >>= 1) live_n += __shfl_xor(live_n, dd);
  if ((threadIdx.x & (WAVE - 1)) == 0) atomicAdd(&s_live, live_n);
  __syncthreads();
  tail_row_out(tb, s_best, s_root, nroot, pr, prk, s_R);
  if (threadIdx.x == 0) tb.blive[blockIdx.x] = s_live;
}

// the report of a batch of tail rounds (enqueued after its copy of the control block): nact_out 0
// when the level is complete, else the active roots of the last round streamed (more rounds follow)
__global__ void k_tail_report(const TailBufs tb, uint32_t last, RoundSlot *slot, unsigned long long seq,
                              unsigned long long *cnt) {
  const TailCtl *c = tb.ctl;
  write_report(slot, seq, cnt, c->done ? 0ull : (unsigned long long)c->nroots[last], c->F0);
}
