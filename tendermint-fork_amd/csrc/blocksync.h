// blocksync.h — the blocksync replay window (f4): pipelined LIGHT batches.  Part of commit.hip's
// translation unit, after seam_host.h and kc_resolve.h.
//
// The context's batch stream: windows of requests whose sets share one key set (0 = generic keys)
// are cut into batches of up to bsz requests; batch b is planned, staged and queued while the
// device copies in and verifies the batches before it, which are then collected and replayed (f4).
// Same results as one run_seam over all requests.  The stream outlives a call: a replay that
// submits window w+1 before collecting window w (tmed_blocksync_submit) keeps the device busy
// across the windows' boundaries, where a call per window drains the pipeline at its end and
// refills it (the first batch's planning and copy-in) at the next start.
#pragma once

#include <chrono>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "c_guard.h"
#include "ctx.h"
#include "debug_zero.h"

// Defined in commit.hip, which includes this file and calls bs_drain and run_pipelined below (the
// one cycle between the two files): a batch is staged as a seam call's group is, and a batch whose
// templates do not fit the device assembler takes the seam's host-message route.
static int stage_group(tmed_ctx *ctx, const tmed_commit_request *reqs, size_t n, const Cands &cands, const Group &grp,
                       uint64_t keyset, const Templates &tp, int slot, tmed::VoteStage &st, int rule);
static int ctx_verify_host_msgs(tmed_ctx *ctx, const tmed_commit_request *reqs, size_t n, const Cands &cands,
                                uint8_t *valid, int rule);

namespace {
struct BsWindow {
  const tmed_commit_request *rq = nullptr;  // the window's requests (checked: check_request)
  tmed_commit_result *out = nullptr;
  size_t n = 0, bsz = 0, next = 0;          // requests; per batch; the next one to batch
  uint64_t keyset = 0;
  int rule = TMED_RULE_GO;  // the signature rule its call read at its entry: every batch of the window runs under it
  const KcCall *kc = nullptr;  // planning's cached address indexes (a call-scoped window only)
  // a submitted window owns its requests, its resolved set and its key-set cache pin (held until
  // its last batch is collected; released outside ctx->mu: ~KcCall takes it)
  std::vector<tmed_commit_request> own_reqs;
  std::vector<tmed_block_id> own_bids;
  std::vector<tmed_commit> own_commits;
  tmed_valset own_set{}, own_vals{};  // the caller's set; its resolved copy
  std::string own_chain;
  std::unique_ptr<KcCall> own_kc;
  size_t inflight = 0;
  bool done() const { return next >= n && inflight == 0; }
};
struct BsBatch {
  BsWindow *win = nullptr;
  size_t lo = 0, n = 0;
  Plans plans;
  Cands cands;
  Templates tmpl;
  std::vector<uint8_t> bits, valid;
  Group grp;  // the staged segments when candidates are aliased (else every run, in order)
  tmed::VoteStage st;
  bool device = false;  // queued on a vote slot (else verified synchronously / nothing to verify)
  std::chrono::steady_clock::time_point enq;  // when it was queued (TMED_TRACE timeline)
};
}  // namespace

// Pipeline depth.  With the signatures staged (pageable caller memory) two slots: a third
// overlaps the host staging of batch b with the copy engine reading batch b-1 out of pinned
// memory, and both slow down (C4 166-172 against 181-191 M verifies/s, profiles/r03/c4_pipe/).
// With the signatures DMA'd from pinned caller memory the host's share per batch is ~1.5 ms
// against ~2.2 ms of kernels, and a third slot keeps the kernel stream busy (C4 280-307 against
// 258-282 M/s, profiles/r03/c4_direct/).  So the depth follows the stream's first batch: three
// slots when its signatures went direct (VoteStage::sig_direct), else two.  (A ramp of small first
// batches did not pay, in round 3 nor again in round 4 with direct DMA: the host's planning and
// staging of each larger batch outlasted the device work of the small one before it, leaving the
// device idle 0.6-1.6 ms per ramp step — profiles/r04/c4_ramp_rejected.txt.)
constexpr int kPipeSlots = 3;
static_assert(kPipeSlots <= (int)(sizeof(((tmed_ctx *)nullptr)->vslot) / sizeof(tmed::VoteSlot)),
              "one context vote slot per pipeline slot");

struct BsStream {
  BsBatch slots[kPipeSlots];
  int ns = 2;
  size_t idx = 0;    // batches queued since the stream was last empty (slot idx % ns)
  int rc = TMED_OK;  // the first error of a submitted window, reported by tmed_blocksync_wait
  std::deque<std::unique_ptr<BsWindow>> wins;
  bool empty() const {
    for (const BsBatch &b : slots)
      if (b.n) return false;
    return true;
  }
};

namespace tmed {
void bs_destroy(tmed_ctx *c) {  // tmed_destroy: nothing may still read the windows' buffers
  if (!c->bs) return;
  (void)hipStreamSynchronize(c->copy_stream);
  (void)hipStreamSynchronize(c->stream);
  if (c->lane1.s) (void)hipStreamSynchronize(c->lane1.s);  // key-cached batches alternate lanes
  delete c->bs;  // the windows' cache pins go with them (the cache is destroyed after this)
  c->bs = nullptr;
}
}  // namespace tmed

using BsClock = std::chrono::steady_clock;
static double bs_us(BsClock::time_point a, BsClock::time_point b) {
  return std::chrono::duration<double, std::micro>(b - a).count();
}

// Collect batch b (ctx->mu held): its bits, then the host finish (seam_host.h finish_batch: the alias
// copies and the replay into its window's results).
// ph: tmed_seam_phase_us — host plan + templates + staging, host time blocked on the device
// (enqueueing the copies and kernels, votes_collect), host replay.
static int bs_finish(tmed_ctx *ctx, BsBatch &b, double ph[3]) {
  if (b.n == 0) return TMED_OK;
  BsWindow &w = *b.win;
  int r = TMED_OK;
  if (b.device) {
    b.bits.resize(b.grp.size(b.cands));
    const auto t0 = BsClock::now();
    r = tmed::votes_collect(ctx, b.st, b.bits.data());
    ph[1] += bs_us(t0, BsClock::now());
    if (r == TMED_OK && debug_zero_on()) debug_record_zeros(ctx, b.st, b.cands, b.grp, b.bits, b.lo);
  }
  const auto t1 = BsClock::now();
  if (r == TMED_OK)
    r = finish_batch(w.rq + b.lo, b.n, w.out + b.lo, b.plans, b.cands, b.grp, b.bits.data(), b.valid, b.device);
  ph[2] += bs_us(t1, BsClock::now());
  b.n = 0;
  b.device = false;
  b.win = nullptr;
  w.inflight--;
  return r;
}

// Collect every batch in flight, oldest first, except those of window `keep` (nullptr: all).
static int bs_collect(tmed_ctx *ctx, BsStream &S, const BsWindow *keep, double ph[3]) {
  int rc = TMED_OK;
  for (int k = 0; k < S.ns; k++) {
    BsBatch &b = S.slots[(S.idx + k) % S.ns];
    if (b.n && b.win != keep) {
      const int r = bs_finish(ctx, b, ph);
      if (rc == TMED_OK) rc = r;
    }
  }
  return rc;
}

// After an error: nothing queued may still read the callers' (pinned) buffers; the batches in
// flight are dropped (their windows' results are incomplete: the error is what the caller gets).
static void bs_abort(tmed_ctx *ctx, BsStream &S, int rc) {
  (void)hipStreamSynchronize(ctx->copy_stream);
  (void)hipStreamSynchronize(ctx->stream);
  // a dropped key-cached batch may run on the second lane: its slot (idx % ns) and its lane
  // (idx & 1) need not match the next batch's, so the lane must be idle before any slot is reused
  if (ctx->lane1.s) (void)hipStreamSynchronize(ctx->lane1.s);
  for (BsBatch &b : S.slots)
    if (b.n) {
      b.n = 0;
      b.device = false;
      if (b.win) b.win->inflight--;
      b.win = nullptr;
    }
  for (auto &w : S.wins) w->next = w->n;
  if (S.rc == TMED_OK) S.rc = rc;
}

// c_guard's recovery (ctx->mu held): a stream that still holds work is dropped, an idle one left alone.
static void bs_abort_pending(tmed_ctx *ctx, int rc) {
  if (ctx->bs && (!ctx->bs->empty() || !ctx->bs->wins.empty())) bs_abort(ctx, *ctx->bs, rc);
}

// Queue window w's batches (ctx->mu held through lk), collecting older batches as their slots are
// reused; returns with up to S.ns - 1 of them... in flight.
static int bs_pump(tmed_ctx *ctx, BsStream &S, BsWindow &w, double ph[3], std::unique_lock<std::mutex> &lk) {
  int rc = TMED_OK;
  if (S.empty()) {
    S.idx = 0;
    S.ns = 2;  // raised to 3 after the stream's first batch when its signatures went direct
  }
  if (trace_on()) {  // origin of the per-batch device timeline in the trace
    if (!ctx->trace_t0) (void)hipEventCreate(&ctx->trace_t0);
    if (ctx->trace_t0) (void)hipEventRecord(ctx->trace_t0, ctx->stream);
  }
  const auto t_origin = BsClock::now();
  while (w.next < w.n && rc == TMED_OK) {
    PhaseClock clk;
    const size_t idx = S.idx++;
    const int ns = S.ns;
    BsBatch &b = S.slots[idx % ns];
    BsBatch &mid = S.slots[(idx + ns - 1) % ns];  // batch idx-1 (in flight; with two slots the same as old)
    BsBatch &old = S.slots[(idx + 1) % ns];       // batch idx-ns+1: collected once batch idx is queued
    if (b.n) rc = bs_finish(ctx, b, ph);          // the slot's previous batch (the depth changed)
    if (rc != TMED_OK) break;
    b.win = &w;
    b.lo = w.next;
    b.n = std::min(w.bsz, w.n - w.next);
    w.next += b.n;
    w.inflight++;
    const tmed_commit_request *rq = w.rq + b.lo;
    const auto tp = BsClock::now();
    // b.grp: the staging segments; b.tmpl: the template rows (when several workers planned)
    rc = seam_plan(rq, b.n, w.out + b.lo, b.plans, b.cands, w.kc, &b.grp, &b.tmpl);
    clk.lap("plan");
    const size_t m = b.cands.size();
    bool fits = b.tmpl.fits;
    if (rc == TMED_OK && m && !b.tmpl.ready) rc = device_templates(rq, b.n, b.cands, b.tmpl, &fits);
    clk.lap("templates");
    if (rc == TMED_OK && m) {
      if (fits && m <= 0xffffffffu) {
        rc = stage_group(ctx, rq, b.n, b.cands, b.grp, w.keyset, b.tmpl, (int)(idx % ns), b.st, w.rule);
        // key-cached batches alternate between the two kernel lanes, so one batch's small kernels
        // (assembly, key order, prep, finish) run beside the other's main kernel
        b.st.lane = w.keyset && (idx & 1) && tmed::lanes_on() ? 1 : 0;
        clk.lap("stage");
        const auto te = BsClock::now();
        ph[0] += bs_us(tp, te);
        if (rc == TMED_OK) rc = tmed::votes_enqueue(ctx, b.st);
        b.enq = BsClock::now();
        if (idx == 0 && b.st.sig_direct) S.ns = 3;
        clk.lap("enqueue");
        ph[1] += bs_us(te, BsClock::now());  // queueing copies / launches can block behind a busy device
        b.device = rc == TMED_OK;
      } else {  // oversize template: host-assembled messages, synchronous (drain the pipeline first)
        if (old.n && &old != &b) rc = bs_finish(ctx, old, ph);
        if (rc == TMED_OK && mid.n && &mid != &b) rc = bs_finish(ctx, mid, ph);
        lk.unlock();
        b.valid.assign(m, 0);
        if (rc == TMED_OK) rc = ctx_verify_host_msgs(ctx, rq, b.n, b.cands, b.valid.data(), w.rule);
        lk.lock();
      }
    }
    const bool traced = trace_on() && old.n && old.st.m && &old != &b;
    if (rc == TMED_OK && &old != &b) rc = bs_finish(ctx, old, ph);  // overlaps the device work of batches idx-1 and idx
    clk.lap("finish_old");
    if (traced)
      fprintf(stderr,
              "[tmed] blocksync collected batch: kernels %.0fus copy-in %.0fus copy end -> kernels %.0fus"
              " | device us: copy %.0f-%.0f kernels %.0f-%.0f | host us: enqueued %.0f collected %.0f\n",
              1000.0 * ctx->last_ms, 1000.0 * ctx->last_copy_ms, 1000.0 * ctx->last_copy_gap_ms,
              1000.0 * ctx->last_at[0], 1000.0 * ctx->last_at[1], 1000.0 * ctx->last_at[2], 1000.0 * ctx->last_at[3],
              bs_us(t_origin, b.enq), bs_us(t_origin, BsClock::now()));
    clk.emit("pipelined batch", b.n, m);
  }
  return rc;
}

static BsStream &bs_stream(tmed_ctx *ctx) {
  if (!ctx->bs) ctx->bs = new BsStream();
  return *ctx->bs;
}

// Windows whose batches are all collected leave the stream (front first); they are destroyed by
// the caller after it released ctx->mu.
static void bs_pop_done(BsStream &S, std::vector<std::unique_ptr<BsWindow>> &gone) {
  while (!S.wins.empty() && S.wins.front()->done()) {
    gone.push_back(std::move(S.wins.front()));
    S.wins.pop_front();
  }
}

// The end of an entry point's hold of ctx->mu: its phase times for tmed_seam_phase_us, and the
// finished windows handed to the caller.
static void bs_call_end(BsStream &S, const double ph[3], std::vector<std::unique_ptr<BsWindow>> &gone) {
  for (int k = 0; k < 3; k++) g_seam_us[k] = ph[k];
  bs_pop_done(S, gone);
}

// Windows whose batches were collected by another seam call (bs_drain) are released here, outside
// ctx->mu (their key-set cache pins go with them: ~KcCall takes the lock).
static void bs_reap(tmed_ctx *ctx) {
  std::vector<std::unique_ptr<BsWindow>> gone;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->bs) bs_pop_done(*ctx->bs, gone);
  }
}

// Every batch of the stream collected (ctx->mu held): before a seam call uses the vote slots.
static int bs_drain(tmed_ctx *ctx) {
  if (!ctx->bs || ctx->bs->empty()) return TMED_OK;
  double ph[3] = {0, 0, 0};
  int rc = bs_collect(ctx, *ctx->bs, nullptr, ph);
  if (rc != TMED_OK) bs_abort(ctx, *ctx->bs, rc);
  return rc;
}

namespace tmed {
int bs_collect_submitted(tmed_ctx *c) { return bs_drain(c); }
void bs_release_collected(tmed_ctx *c) { bs_reap(c); }
}  // namespace tmed

// One window through the stream and back (every batch collected before returning).
static int run_pipelined(tmed_ctx *ctx, const tmed_commit_request *reqs, size_t nb, size_t bsz, uint64_t keyset,
                         tmed_commit_result *out, const KcCall *kc, int rule) {
  std::vector<std::unique_ptr<BsWindow>> gone;
  int rc;
  {
    std::unique_lock<std::mutex> lk(ctx->mu);
    BsStream &S = bs_stream(ctx);
    double ph[3] = {0, 0, 0};
    rc = bs_collect(ctx, S, nullptr, ph);  // earlier submitted windows finish first
    if (rc != TMED_OK) bs_abort(ctx, S, rc);  // theirs: reported here and by tmed_blocksync_wait
    const int prev = S.rc;
    auto w = std::make_unique<BsWindow>();
    w->rq = reqs;
    w->out = out;
    w->n = nb;
    w->bsz = std::max<size_t>(1, bsz);
    w->keyset = keyset;
    w->rule = rule;
    w->kc = kc;
    BsWindow *wp = w.get();
    S.wins.push_back(std::move(w));
    if (rc == TMED_OK) {
      rc = bs_pump(ctx, S, *wp, ph, lk);
      if (rc == TMED_OK) rc = bs_collect(ctx, S, nullptr, ph);
      if (rc != TMED_OK) {
        bs_abort(ctx, S, rc);
        S.rc = prev;  // only this call's window was in flight: its error is reported here
      }
    }
    wp->next = wp->n;
    bs_call_end(S, ph, gone);
    for (auto it = S.wins.begin(); it != S.wins.end(); ++it)  // this call's window (borrowed buffers) never stays
      if (it->get() == wp) {
        gone.push_back(std::move(*it));
        S.wins.erase(it);
        break;
      }
  }
  return rc;
}

// A blocksync window as LIGHT requests (blockchain/v0/reactor.go:366-367), resolved through the
// key-set cache, owned by the returned window.
static int bs_window(tmed_ctx *ctx, const tmed_blocksync_window *w, uint32_t batch_blocks, tmed_commit_result *out,
                     std::unique_ptr<BsWindow> &win) {
  if (!ctx || !w || (w->n_blocks && (!w->vals || !w->block_ids || !w->heights || !w->commits || !out)))
    return TMED_EINVAL;
  const size_t nb = w->n_blocks;
  win = std::make_unique<BsWindow>();
  BsWindow &W = *win;
  // the structs are copied (the caller may reuse them once submit returns); what they point to
  // (hashes, commit arrays, keys) is the caller's until the window's results are final
  W.own_reqs.resize(nb);
  W.own_bids.assign(w->block_ids, w->block_ids + nb);
  W.own_commits.assign(w->commits, w->commits + nb);
  if (nb) W.own_set = *w->vals;
  if (w->chain_id_len) W.own_chain.assign(w->chain_id, w->chain_id_len);
  for (size_t h = 0; h < nb; h++) {
    tmed_commit_request &r = W.own_reqs[h];
    memset(&r, 0, sizeof r);
    r.mode = TMED_MODE_LIGHT;
    r.chain_id = W.own_chain.data();
    r.chain_id_len = w->chain_id_len;
    r.vals = &W.own_set;
    r.block_id = &W.own_bids[h];
    r.height = w->heights[h];
    r.commit = &W.own_commits[h];
    if (check_request(r) != TMED_OK) return TMED_EINVAL;
  }
  W.own_kc = std::make_unique<KcCall>();  // one set for the whole window
  if (nb) {
    const tmed_commit_request *rq = keycache_resolve(ctx, W.own_reqs.data(), nb, *W.own_kc);
    if (rq != W.own_reqs.data()) {  // resolved onto the cache's pool: the window keeps its own copy
      W.own_vals = *rq[0].vals;
      for (tmed_commit_request &r : W.own_reqs) r.vals = &W.own_vals;
    }
  }
  W.rq = W.own_reqs.data();
  W.out = out;
  W.n = nb;
  W.bsz = batch_blocks ? batch_blocks : 128;
  W.keyset = nb ? W.own_reqs[0].vals->keyset : 0;
  W.rule = tmed::seam_rule(ctx);
  return TMED_OK;
}

extern "C" int tmed_blocksync_submit(tmed_ctx *ctx, const tmed_blocksync_window *w, uint32_t batch_blocks,
                                     tmed_commit_result *out) {
  return c_guard(ctx, [&] {
    std::unique_ptr<BsWindow> win;
    int rc = bs_window(ctx, w, batch_blocks, out, win);
    if (rc != TMED_OK) return rc;
    std::vector<std::unique_ptr<BsWindow>> gone;
    {
      std::unique_lock<std::mutex> lk(ctx->mu);
      BsStream &S = bs_stream(ctx);
      double ph[3] = {0, 0, 0};
      BsWindow *wp = win.get();
      S.wins.push_back(std::move(win));
      rc = bs_pump(ctx, S, *wp, ph, lk);
      // every EARLIER window's results final on return; this window's last batches stay in flight
      if (rc == TMED_OK) rc = bs_collect(ctx, S, wp, ph);
      if (rc != TMED_OK) bs_abort(ctx, S, rc);
      bs_call_end(S, ph, gone);
    }
    return rc;
  });
}

extern "C" int tmed_blocksync_wait(tmed_ctx *ctx) {
  if (!ctx) return TMED_EINVAL;
  return c_guard(ctx, [&] {
    std::vector<std::unique_ptr<BsWindow>> gone;
    int rc;
    {
      std::lock_guard<std::mutex> lk(ctx->mu);
      if (!ctx->bs) return TMED_OK;
      BsStream &S = *ctx->bs;
      double ph[3] = {0, 0, 0};
      rc = bs_collect(ctx, S, nullptr, ph);
      if (rc != TMED_OK) bs_abort(ctx, S, rc);
      rc = S.rc;
      S.rc = TMED_OK;
      bs_call_end(S, ph, gone);
    }
    return rc;
  });
}

extern "C" int tmed_blocksync_verify(tmed_ctx *ctx, const tmed_blocksync_window *w, uint32_t batch_blocks,
                                     tmed_commit_result *out) {
  return c_guard(ctx, [&] {
    std::unique_ptr<BsWindow> win;
    int rc = bs_window(ctx, w, batch_blocks, out, win);
    if (rc != TMED_OK || win->n == 0) return rc;
    return run_pipelined(ctx, win->rq, win->n, win->bsz, win->keyset, out, nullptr, win->rule);
  });
}

