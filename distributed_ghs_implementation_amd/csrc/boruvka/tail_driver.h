// Part of boruvka.hip (included there once, after `using namespace ghs`; not a stand-alone header).
// The LDS tail of a level, host side: the tail_* steps, run_tail (one rank), ghs_solver_tail_multi
// (the multi-rank loop's) and the stepwise ghs_solver_tail_* entry points. Relies on what precedes
// its include in boruvka.hip: struct ghs_solver, KT, the round helpers, and boruvka/tail.h.

// ---- the LDS tail: the rest of a level once its active fragments fit LDS (one rank) ---------
// Enters at a round >= 1 of a level whose exact active count is in [2, TAIL_MAX] (the host has
// read every earlier report); enqueues batches of tail rounds (k_tail_round + k_tail_hook, no-ops
// once the level is done) behind k_tail_map + k_tail_open, each batch ending with a copy of the
// control block and its report; reads the tail's per-round stats from that copy and closes the
// level. Rounds whose launches follow the finishing round exit at once.
// Tail rounds per batch: the first batch is sized from the level's last observed contraction.
// F0 fragments shrinking by `decay` per round leave <= 1 root after L = log_decay(F0) rounds of
// hooks (the open's included), so k_tail_round r = ceil(L) is the finishing one and the batch holds
// exactly the launches the level needs. The contraction slows inside a level (R-MAT s24 level 0:
// 26x, 19x, 10x, 10x), so half a round of margin — none when the open's hooks alone are expected to
// finish (F0 <= decay): R-MAT s24 levels 0 and 1 and both tails of the 16384^2 grid then launch no
// round past the finishing one (profiles/r06/rounds_*.txt). An underestimate costs one more batch.
constexpr uint32_t TAIL_BATCH_MIN = 1, TAIL_BATCH_MAX = 8;

static uint32_t tail_first_batch(uint64_t F0, uint64_t prev_in) {
  const double decay = std::max(2.0, prev_in > F0 ? (double)prev_in / (double)F0 : 2.0);
  const double L = std::log((double)F0) / std::log(decay);
  const double est = (double)F0 <= decay ? 1.0 : std::ceil(L + 0.5);
  return (uint32_t)std::min<double>(TAIL_BATCH_MAX, std::max<double>(TAIL_BATCH_MIN, est));
}
constexpr uint64_t TAIL_TRY = 32ull * TAIL_MAX;  // a bound below this: read the exact count first

static bool tail_usable(const ghs_solver *s) {
  return s->tail_on && s->tail.ctl && s->cfg.num_ranks <= 1 && !s->level_dense && s->level_round >= 1 &&
         !s->act_ident;
}

// map + labels + open (round 0's stream of the tail)
static void tail_start(ghs_solver *s, TailRun &t, bool multi) {
  hipStream_t st = s->stream;
  ensure_lab(s);
  t.tb = s->tail;
  const ArcBuf &I = s->buf[s->cur], &O = s->buf[s->cur ^ 1];
  t.tb.rec = O.src;  // the idle edge buffer holds the tail's records
  t.tb.rkey = O.key;
  if (s->scan_pending) flush_scan(s);
  t.act0 = s->act[s->act_cur];
  const unsigned long long *d_nact = cur_act_count(s);
  SegView in{I.seg_start, I.seg_prefix, s->cur_nseg};
  t.F0 = (uint32_t)s->nact;
  t.hook_g = (t.F0 + TAIL_HS - 1) / TAIL_HS;
  t.round0 = s->round;
  t.lr0 = s->level_round;
  t.r = 1;
  t.multi = multi;
  KT(GHS_K_TAIL_OPEN, s->arcs_known ? s->cur_arcs : 0);
  k_tail_map<<<grid_for(t.F0, 256, 64), 256, 0, st>>>(t.act0, d_nact, t.tb);
  // the labels the edges carry: the previous round's list (after the level's identity round 0:
  // every vertex; a dense level's: every dense label)
  const bool prev_ident = t.lr0 == 1;
  const uint32_t *prev = prev_ident ? nullptr : s->act[s->act_cur ^ 1];
  const unsigned long long *d_nprev =
      prev_ident ? s->cnt + (s->level_dense ? C_NDENSE : C_N) : act_count(s, s->act_cur ^ 1);
  const uint64_t nprev_bound = prev_ident ? (s->level_dense ? s->dense_n : s->n) : s->level_nact;
  k_tail_labels<<<grid_for(nprev_bound, 256, 8192), 256, 0, st>>>(prev, d_nprev, s->lab, t.tb);
  k_tail_open<<<TAIL_G, TAIL_T, 0, st>>>(I.src, I.dst, I.key, in, t.tb, s->check_totals);
}

// round rr's hooks: every root's minimum over the blocks' rows (several ranks: this rank's own,
// agreed by tail_agree between the caller's two all-reduces)
static int tail_hook_local(ghs_solver *s, const TailRun &t, uint32_t rr) {
  s->round = t.round0 + rr;  // the profile's round index: the round whose stream they reduce
  KT(GHS_K_TAIL_HOOK, rr ? 0 : t.F0);
  k_tail_hook<<<t.hook_g, 256, 0, s->stream>>>(t.tb, rr, s->in_mst, TAIL_G, s->cnt + C_ERR, t.multi);
  GHS_HIP_CHECK(hipGetLastError());
  return GHS_OK;
}

static int tail_agree(ghs_solver *s, const TailRun &t, uint32_t rr) {
  s->round = t.round0 + rr;
  KT(GHS_K_TAIL_HOOK, 0);
  k_tail_xhook<<<t.hook_g, 256, 0, s->stream>>>(t.tb, rr, s->in_mst, (uint32_t)s->e_lo, (uint32_t)s->e_hi);
  GHS_HIP_CHECK(hipGetLastError());
  return GHS_OK;
}

static int tail_round_launch(ghs_solver *s, const TailRun &t, uint32_t r) {
  s->round = t.round0 + r;
  KT(GHS_K_TAIL_ROUND, 0);
  k_tail_round<<<TAIL_G, TAIL_T, 0, s->stream>>>(t.tb, r, t.act0, s->lab, s->cnt, s->cnt + C_ERR);
  GHS_HIP_CHECK(hipGetLastError());
  return GHS_OK;
}

// the control block (and the report, checksummed) behind the tail's launches so far: *nact_out = 0
// once the level is done
static int tail_report(ghs_solver *s, const TailRun &t, uint32_t last, unsigned long long *nact_out) {
  hipStream_t st = s->stream;
  const unsigned long long seq = ++s->res->seq;
  RoundSlot *dslot = &s->d_slot[seq % SLOT_RING];
  GHS_HIP_CHECK(hipMemcpyAsync(s->res->h_tail, t.tb.ctl, sizeof(TailCtl), hipMemcpyDeviceToHost, st));
  k_tail_report<<<1, 1, 0, st>>>(t.tb, last, dslot, seq, s->cnt);
  GHS_HIP_CHECK(hipGetLastError());
  RoundSlot rep;
  if (int rc = wait_slot(s, s->h_slot + (seq % SLOT_RING), seq, &rep)) return rc;
  if (slot_err(rep.err)) return fail_counters(s, slot_err(rep.err), "in the LDS tail");
  s->rep_weight = rep.weight;
  s->rep_edges = rep.edges;
  s->report_final = true;
  if (s->debug)
    fprintf(stderr, "[ghs] level %u tail report: nact_out %llu edges %llu weight %llu\n", s->level, rep.nact_out,
            rep.edges, rep.weight);
  *nact_out = rep.nact_out;
  return GHS_OK;
}

// the level is done (the last report read): the tail rounds' stats, then the level's close
static int tail_finish(ghs_solver *s, const TailRun &t) {
  const TailCtl &c = *s->res->h_tail;
  const uint32_t rounds = std::min(c.rounds, TAIL_ROUNDS_MAX);
  for (uint32_t k = 0; k < rounds; ++k) push_stats(s, t.lr0 + k, c.live[k], c.nroots[k], c.edges[k]);
  s->round = t.round0 + rounds;
  s->level_round = t.lr0 + rounds;
  s->tail_ran = true;
  if (s->ev_rec.size() > s->round) s->ev_rec.resize(s->round);
  if (int rc = check_level_totals(s)) return rc;
  if (int rc = dense_close(s)) return rc;
  close_level(s);
  return GHS_OK;
}

// coll != nullptr: one rank of several (a dense level, ghs_solver_tail_multi) — each round's hooks
// agree across the ranks through two small all-reduces (MIN of the F0 keys, MAX of the targets)
static int run_tail(ghs_solver *s, uint64_t prev_in, const GhsTailColl *coll = nullptr) {
  hipStream_t st = s->stream;
  TailRun t;
  tail_start(s, t, coll != nullptr);
  auto hook = [&](uint32_t rr) -> int {
    if (int rc = tail_hook_local(s, t, rr)) return rc;
    if (coll) {
      if (int rc = coll->min_u64(coll->ctx, t.tb.gkey, t.F0, st)) return rc;
      if (int rc = tail_agree(s, t, rr)) return rc;
      if (int rc = coll->max_i32(coll->ctx, reinterpret_cast<int32_t *>(t.tb.ghook), t.F0, st)) return rc;
    }
    return GHS_OK;
  };
  if (int rc = hook(0)) return rc;
  uint32_t batch = tail_first_batch(t.F0, prev_in);
  for (;;) {
    const uint32_t last = std::min(t.r + batch - 1, TAIL_ROUNDS_MAX);  // the batch's last round
    for (; t.r <= last; ++t.r) {
      // round r - 1's hooks, unless the open's (launched above): a batch ends with a round, not with
      // its hook kernel, so the round that finishes the level is not followed by a no-op hook launch
      // when it closes its batch (the hook comes first in the next batch otherwise)
      if (t.r > 1)
        if (int rc = hook(t.r - 1)) return rc;
      if (int rc = tail_round_launch(s, t, t.r)) return rc;
    }
    unsigned long long nact_out = 0;
    if (int rc = tail_report(s, t, last, &nact_out)) return rc;
    if (nact_out <= 1) break;
    if (t.r > TAIL_ROUNDS_MAX) return fail_counters(s, 4, "in the LDS tail (round cap)");
    // the next batch from the batch's last contraction (the report's copy of the control block:
    // nroots[last] = nact_out roots entering round last's stream, nroots[last - 1] before them),
    // sized like the first — R-MAT s26 level 0 (1189 -> 106 -> 14 -> 3 roots) then finishes in a
    // batch of 1 instead of a fixed 3 with two no-op launch pairs
    const TailCtl &c = *s->res->h_tail;
    batch = tail_first_batch(nact_out, last >= 1 ? c.nroots[last - 1] : t.F0);
  }
  return tail_finish(s, t);
}

// The multi-rank loop's LDS tail (ghs_solver_run, multi.hip): at a round >= 1 of a dense level whose
// active count is at most TAIL_MAX, the rounds still in flight are drained (their reports give the
// exact count — every rank reads the same reports, so every rank takes the same branch), then the
// level finishes in run_tail with the ranks' hooks agreed per round. Returns 0 when not applicable,
// 1 when the level finished (in the drain or the tail), 2 when that ended the solve, or an error.
int ghs_solver_tail_multi(ghs_solver *s, const GhsTailColl *coll) {
  if (!s || !coll) return 0;
  if (s->phase != 0 || !s->level_open || s->cfg.num_ranks <= 1 || !s->level_dense || !s->tail_on || !s->tail.ctl ||
      s->act_ident || s->level_round < 1 || s->nact > TAIL_MAX)
    return 0;
  while (!s->pipe.empty()) {  // the rounds in flight (pipelined contract): their reports, in order
    const ghs_solver::PipeRound p = s->pipe.front();
    s->pipe.erase(s->pipe.begin());
    RoundSlot rep;
    if (int rc = wait_slot(s, s->h_slot + (p.seq % SLOT_RING), p.seq, &rep)) return rc;
    if (slot_err(rep.err)) return fail_counters(s, slot_err(rep.err), ("in round " + std::to_string(p.round + 1)).c_str());
    push_stats(s, p.level_round, s->pipe_live, rep.nact_in, rep.edges);
    s->pipe_live = rep.live_out;
    s->pipe_exact = rep.nact_out;
    s->pipe_exact_lr = p.level_round + 1;
    s->nact = rep.nact_out;
    if (rep.nact_out <= 1) {  // the level ended with round p: the rounds enqueued after it are no-ops
      s->pipe.clear();
      s->round = p.round + 1;
      s->level_round = p.level_round + 1;
      if (int rc = dense_close(s)) return rc;
      close_level(s);
      return s->phase == 2 ? 2 : 1;
    }
  }
  if (s->nact < 2) return 0;  // (the synchronous contract closes such a level itself)
  if (int rc = run_tail(s, s->last_nact_in, coll)) return rc;
  return s->phase == 2 ? 2 : 1;
}

static bool tail_step_usable(const ghs_solver *s) {
  return s->phase == 0 && s->level_open && s->cfg.num_ranks > 1 && s->level_dense && s->tail_on && s->tail.ctl &&
         !s->act_ident && s->level_round >= 1 && s->nact >= 2 && s->nact <= TAIL_MAX && s->pipe.empty();
}

extern "C" {

// ---- the stepwise LDS tail (ABI 10; include/ghs_mst.h): the caller's collectives between the calls ----
int ghs_solver_tail_begin(ghs_solver_t *s, uint64_t *num_fragments) {
  if (!s || !num_fragments) GHS_FAIL(GHS_E_ARG, "solver/num_fragments is NULL");
  *num_fragments = 0;
  if (s->tail_step) GHS_FAIL(GHS_E_STATE, "a tail is already in progress");
  if (!tail_step_usable(s)) return GHS_OK;
  s->trun = TailRun();
  tail_start(s, s->trun, true);
  if (int rc = tail_hook_local(s, s->trun, 0)) return rc;
  s->tail_step = true;
  s->phase = 3;  // (minedge / contract refuse until the tail ends)
  *num_fragments = s->trun.F0;
  return GHS_OK;
}

int ghs_solver_tail_buffers(ghs_solver_t *s, uint64_t **d_keys, int32_t **d_hooks) {
  if (!s || !d_keys || !d_hooks) GHS_FAIL(GHS_E_ARG, "solver/keys/hooks is NULL");
  if (!s->tail_step) GHS_FAIL(GHS_E_STATE, "no tail in progress (ghs_solver_tail_begin)");
  *d_keys = s->tail.gkey;
  *d_hooks = reinterpret_cast<int32_t *>(s->tail.ghook);
  return GHS_OK;
}

int ghs_solver_tail_agree(ghs_solver_t *s) {
  if (!s) GHS_FAIL(GHS_E_ARG, "solver is NULL");
  if (!s->tail_step) GHS_FAIL(GHS_E_STATE, "no tail in progress (ghs_solver_tail_begin)");
  return tail_agree(s, s->trun, s->trun.r - 1);
}

int ghs_solver_tail_round(ghs_solver_t *s, int *state) {
  if (!s || !state) GHS_FAIL(GHS_E_ARG, "solver/state is NULL");
  *state = 0;
  if (!s->tail_step) GHS_FAIL(GHS_E_STATE, "no tail in progress (ghs_solver_tail_begin)");
  TailRun &t = s->trun;
  if (t.r > TAIL_ROUNDS_MAX) {
    s->tail_step = false;
    return fail_counters(s, 4, "in the LDS tail (round cap)");
  }
  if (int rc = tail_round_launch(s, t, t.r)) return rc;
  unsigned long long nact_out = 0;
  if (int rc = tail_report(s, t, t.r, &nact_out)) {
    s->tail_step = false;
    return rc;
  }
  if (nact_out <= 1) {
    s->tail_step = false;
    s->phase = 0;
    if (int rc = tail_finish(s, t)) return rc;
    *state = s->phase == 2 ? 2 : 1;
    return GHS_OK;
  }
  if (int rc = tail_hook_local(s, t, t.r)) return rc;
  ++t.r;
  return GHS_OK;
}

}  // extern "C"
