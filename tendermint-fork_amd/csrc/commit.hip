// commit.hip — the drop-in seam: ValidatorSet.VerifyCommit* over one GPU batch (host C++).
//
// Reference loops restated (types/validator_set.go):
//   VerifyCommit               :667-714  verify EVERY non-absent signature, tally ForBlock power
//   VerifyCommitLight          :722-765  ForBlock only, return nil as soon as tally > 2/3
//   VerifyCommitLightTrusting  :775-826  ForBlock, GetByAddress (:270-278), double-vote check
//                                        before verifying, return nil once tally > trust level
// Per batch of requests:
//   1. the reference prechecks (set size, height, BlockID.Equals, zero denominator, safeMul)
//   2. candidate selection = exactly the signatures the loop can reach: for the early-exit
//      loops, the ForBlock prefix up to the crossing computed as if every signature were
//      valid (if one in that prefix is invalid the loop stops there anyway; if none is,
//      it stops at the crossing), and for Trusting also up to the first double vote
//   3. CanonicalVote sign-bytes (signbytes.hip over vote_wire.h), ONE device batch (tmed_verify_batch)
//   4. replay of the reference loop over the validity bits — first-error index, early
//      exit, Got/Needed and error kinds come out identical by construction.
#include <atomic>
#include <chrono>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/tmed25519.h"
#include "call_frame.h"
#include "host_pool.h"
#include "signbytes.h"
#include "votes_host.h"
#include "evidence_host.h"
#include "lca_host.h"
#include "median_host.h"
#include "validate_host.h"

// One translation unit, by role (each header is included here only, in this order):
//   seam_host.h   planning, aliasing, staging groups, scatter, replay: host C++ only
//   kc_resolve.h  the call's sets resolved through the key-set cache (set_index.h numbers them)
//   blocksync.h   the context's pipelined batch stream and the tmed_blocksync_* entry points
//                 (c_guard.h: the entry points' wrapper; debug_zero.h: diagnostics)
// This file: the verify path of one seam call, the light client's hashes, the tmed_verify_commits,
// tmed_light_verify, tmed_verify_light_client_attacks, tmed_validate_blocks and *_multi entry points.
#include "seam_host.h"
#include "kc_resolve.h"
#include "blocksync.h"

// Host fallback of the GPU verifier for templates the device assembler cannot hold.
static int ctx_verify_host_msgs(tmed_ctx *ctx, const tmed_commit_request *reqs, size_t n, const Cands &cands,
                                uint8_t *valid, int rule) {
  CandBatch cb;
  int rc = build_cand_batch(reqs, n, cands, cb);
  if (rc != TMED_OK) return rc;
  std::unordered_map<uint64_t, std::vector<uint32_t>> groups;
  for (size_t k = 0; k < cb.m; k++) groups[cb.keyset[k]].push_back((uint32_t)k);
  for (auto &g : groups) {
    const std::vector<uint32_t> &ix = g.second;
    const size_t m = ix.size();
    std::vector<uint8_t> pubs(m * 32), sigs(m * 64), msgs, out(m);
    std::vector<uint32_t> lens(m), offs(m + 1), vidx(m);
    size_t total = 0;
    for (size_t j = 0; j < m; j++) total += cb.offs[ix[j] + 1] - cb.offs[ix[j]];
    msgs.resize(total + 16);
    total = 0;
    for (size_t j = 0; j < m; j++) {
      const uint32_t k = ix[j];
      memcpy(&pubs[j * 32], &cb.pubs[k * 32], 32);
      memcpy(&sigs[j * 64], &cb.sigs[k * 64], 64);
      lens[j] = cb.lens[k];
      vidx[j] = cb.val_idx[k];
      const uint32_t len = cb.offs[k + 1] - cb.offs[k];
      offs[j] = (uint32_t)total;
      memcpy(&msgs[total], &cb.msgs[cb.offs[k]], len);
      total += len;
    }
    offs[m] = (uint32_t)total;
    rc = g.first == 0 ? tmed::verify_batch_rule(ctx, pubs.data(), sigs.data(), lens.data(), msgs.data(), offs.data(), m,
                                                out.data(), rule)
                      : tmed::verify_batch_keyset_rule(ctx, g.first, vidx.data(), sigs.data(), lens.data(), msgs.data(),
                                                       offs.data(), m, out.data(), rule);
    if (rc != TMED_OK) return rc;
    for (size_t j = 0; j < m; j++) valid[ix[j]] = out[j];
  }
  return TMED_OK;
}

// Device staging of one group's candidates into vote slot `slot`: sign-bytes are assembled on
// the device from per-commit templates, so only key references, signatures,
// flags and timestamps cross PCIe; they are written straight from the request arrays into the
// pinned staging area, run by run (multi-threaded for large batches).  The caller holds ctx->mu.
constexpr size_t kDmaMinRun = 256;  // signatures (16 KB)
static int stage_group(tmed_ctx *ctx, const tmed_commit_request *reqs, size_t n, const Cands &cands, const Group &grp,
                       uint64_t keyset, const Templates &tp, int slot, tmed::VoteStage &st, int rule) {
  const bool keyed = keyset != 0;
  const uint32_t m = (uint32_t)grp.size(cands);
  int rc = tmed::votes_stage(ctx, keyset, m, std::max<size_t>(tp.nrows, 1), st, slot);
  if (rc != TMED_OK) return rc;
  st.rule = rule;
  memcpy(st.tmpl, tp.rows.data(), std::max<size_t>(tp.nrows, 1) * tmed::kVoteTmplBytes);
  std::atomic<bool> key_ok{true};
  const uint32_t nkeys = keyed ? (uint32_t)st.ks->n : 0u;
  // Signature runs in pinned caller memory go to the device by their own DMA (votes_enqueue)
  // instead of through the staging area: only batches copied on the copy stream.
  bool direct = st.total >= tmed::kVoteCopyStreamMin;
  // pinned-memory lookups once per request (a registry lookup per run took a global lock per
  // vote where runs are single votes: Trusting candidates, C3)
  // (only requests with a run long enough for its own DMA: a light-client batch has none)
  std::vector<uint8_t> req_pinned;
  if (direct) {
    req_pinned.assign(n, 0);
    const size_t *pos = grp.positions(cands);
    const size_t nr = grp.nruns(cands);
    for (size_t j = 0; j < nr; j++)
      if (pos[j + 1] - pos[j] >= kDmaMinRun) req_pinned[cands.runs[grp.run(cands, j)].req] = 2;
    bool any = false;
    for (size_t q = 0; q < n; q++) {
      if (req_pinned[q] != 2) continue;
      const tmed_commit &c = *reqs[q].commit;
      req_pinned[q] = c.n_sigs && tmed::host_pinned(c.sigs, 64 * c.n_sigs) ? 1 : 0;
      any = any || req_pinned[q];
    }
    direct = any;
  }
  const unsigned nt = host_threads(m);
  std::vector<std::vector<tmed::VoteStage::Dma>> tdma(direct ? nt : 0u);
  std::atomic<bool> all_direct{direct};
  // per run segment: one memcpy per array; the key index, the template index and short
  // signatures stay per vote
  auto fill = [&](size_t lo, size_t hi, unsigned tid) {
    bool ok = true, staged_sig = false;
    std::vector<tmed::VoteStage::Dma> mine;  // (a header of its own: see PlanPart, seam_host.h)
    for_segments(cands, grp, lo, hi, [&](size_t j, uint32_t u0, uint32_t u1, size_t p) {
      const Run &run = cands.runs[grp.run(cands, j)];
      const tmed_commit_request &r = reqs[run.req];
      const tmed_commit &c = *r.commit;
      const size_t i = (size_t)(run.sig + (int32_t)u0);
      const int32_t v0 = run.val + (int32_t)u0;
      const size_t len = u1 - u0;
      if (keyed) {
        uint32_t *kd = reinterpret_cast<uint32_t *>(st.key) + p;
        const uint32_t *kix = r.vals->keyset_index;
        for (size_t u = 0; u < len; u++) {
          const uint32_t v = kix ? kix[v0 + (int32_t)u] : (uint32_t)(v0 + (int32_t)u);
          ok = ok && v < nkeys;
          kd[u] = v;
        }
      } else {
        memcpy(st.key + p * 32, r.vals->pubkeys + 32 * (size_t)v0, 32 * len);
      }
      // runs of at least kDmaMinRun signatures: a DMA command costs ~10 us of the copy engine
      bool dma = direct && len >= kDmaMinRun && tid < tdma.size() && req_pinned[run.req];
      if (dma && c.sig_lens)  // short signatures are zero-padded in staging
        for (size_t u = 0; u < len && dma; u++) dma = c.sig_lens[i + u] >= 64;
      if (dma) {
        mine.push_back({p * 64, c.sigs + 64 * i, 64 * len});
      } else {
        staged_sig = true;
        memcpy(st.sig + p * 64, c.sigs + 64 * i, 64 * len);
        if (c.sig_lens)
          for (size_t u = 0; u < len; u++) {
            const uint32_t sl = c.sig_lens[i + u];
            if (sl < 64) memset(st.sig + (p + u) * 64 + sl, 0, 64 - sl);
          }
      }
      std::fill(st.tidx + p, st.tidx + p + len, tp.row(cands, run.req));
      memcpy(st.flag + p, c.flags + i, len);
      memcpy(st.sec + p, c.ts_seconds + i, 8 * len);
      memcpy(st.nan + p, c.ts_nanos + i, 4 * len);
    });
    if (!ok) key_ok = false;
    if (staged_sig) all_direct = false;
    if (tid < tdma.size()) tdma[tid].swap(mine);
  };
  parallel_ranges(m, nt, fill);
  if (!key_ok) return TMED_EINVAL;  // a key-set index past the key set (votes_enqueue's check)
  for (auto &v : tdma)  // thread ranges in order; a run cut at a thread boundary is joined again
    for (const tmed::VoteStage::Dma &r : v) {
      tmed::VoteStage::Dma *b = st.dma.empty() ? nullptr : &st.dma.back();
      if (b && b->dst + b->bytes == r.dst && (const uint8_t *)b->src + b->bytes == (const uint8_t *)r.src)
        b->bytes += r.bytes;
      else
        st.dma.push_back(r);
    }
  st.sig_direct = all_direct && m > 0;
  st.keys_checked = keyed;
  return TMED_OK;
}

// GPU verifier of one seam call: candidates of validator sets with a key-set handle go
// through the key-cached kernels, one launch sequence per distinct key set.
static int ctx_verify(tmed_ctx *ctx, const tmed_commit_request *reqs, size_t n, const Cands &cands,
                      uint8_t *valid, int rule) {
  PhaseClock clk;
  thread_local Templates tmpl;
  bool fits = true;
  int rc = device_templates(reqs, n, cands, tmpl, &fits);
  if (rc != TMED_OK) return rc;
  if (!fits) return ctx_verify_host_msgs(ctx, reqs, n, cands, valid, rule);
  clk.lap("templates");
  // the runs by key set (usually a single group: then it is every run, in order)
  std::vector<uint64_t> gkeys;
  std::vector<Group> groups;
  group_by_keyset(reqs, cands, gkeys, groups);
  std::lock_guard<std::mutex> lk(ctx->mu);
  rc = bs_drain(ctx);  // batches of submitted blocksync windows hold the vote slots
  if (rc != TMED_OK) return rc;
  for (size_t g = 0; g < gkeys.size(); g++) {
    const Group &grp = groups[g];
    const uint32_t m = (uint32_t)grp.size(cands);
    if (m == 0) continue;
    tmed::VoteStage st;
    rc = stage_group(ctx, reqs, n, cands, grp, gkeys[g], tmpl, 0, st, rule);
    clk.lap("stage");
    std::vector<uint8_t> out(m);
    if (rc == TMED_OK) rc = tmed::votes_launch(ctx, st, out.data());
    if (rc != TMED_OK) return rc;
    clk.lap("device");
    if (trace_on()) fprintf(stderr, "[tmed] group %zu: %u votes, assemble+verify kernels %.0fus\n", g, m,
                            1000.0 * ctx->last_ms);
    scatter_bits(reqs, cands, grp, out.data(), valid);
    clk.lap("scatter");
  }
  copy_aliases(cands, valid);
  clk.emit("ctx_verify", n, cands.size());
  return TMED_OK;
}

// A large call whose sets share one key set (a light-client or evidence backlog) goes through
// the two-slot pipeline in batches of ~2^19 signatures (env TMED_PIPE_SIGS), so the host
// planning, staging and replay of one batch overlap the device work of the next.
static size_t pipe_batch_sigs() {
  const char *e = getenv("TMED_PIPE_SIGS");
  return e ? std::max<size_t>(1, strtoull(e, nullptr, 10)) : (size_t)1 << 19;
}

// rule: the context's rule as the entry point read it (tmed::seam_rule), once for the whole call.
static int verify_commits_impl(tmed_ctx *ctx, const tmed_commit_request *reqs, size_t n, tmed_commit_result *out,
                               int rule) {
  if (!ctx) return TMED_EINVAL;
  KcCall kc;
  reqs = keycache_resolve(ctx, reqs, n, kc);
  const size_t kPipeBatchSigs = pipe_batch_sigs();
  if (n > 1 && reqs && out) {
    // every request checked, one key set, the signature total (in parallel: a light-client call's
    // ~10k commit structs are cold in the cache)
    const uint64_t ks = reqs[0].vals ? reqs[0].vals->keyset : 0;
    std::atomic<bool> all_ok{true};
    std::atomic<size_t> sig_total{0};
    parallel_ranges(n, n >= 4096 ? host_threads(n * 64) : 1, [&](size_t lo, size_t hi, unsigned) {
      size_t sg = 0;
      bool good = true;
      for (size_t q = lo; q < hi && good; q++) {
        good = check_request(reqs[q]) == TMED_OK && reqs[q].vals->keyset == ks;
        if (good) sg += reqs[q].commit->n_sigs;
      }
      sig_total += sg;
      if (!good) all_ok = false;
    });
    const bool ok = all_ok.load();
    const size_t sigs = sig_total.load();
    if (ok && sigs >= 2 * kPipeBatchSigs) {
      const size_t bsz = std::max<size_t>(16, kPipeBatchSigs / std::max<size_t>(1, sigs / n));
      if (n > bsz) {
        const int rc = run_pipelined(ctx, reqs, n, bsz, ks, out, &kc, rule);
        bs_reap(ctx);
        return rc;
      }
    }
  }
  const int rc = run_seam(
      reqs, n, out,
      [&](const tmed_commit_request *rq, size_t nr, const Cands &cands, uint8_t *valid) {
        return ctx_verify(ctx, rq, nr, cands, valid, rule);
      },
      &kc);
  bs_reap(ctx);  // submitted windows this call collected (ctx_verify drained the stream) leave now
  return rc;
}

extern "C" int tmed_verify_commits(tmed_ctx *ctx, const tmed_commit_request *reqs, size_t n,
                                   tmed_commit_result *out) {
  if (!ctx) return TMED_EINVAL;
  return c_guard(ctx, [&] { return verify_commits_impl(ctx, reqs, n, out, tmed::seam_rule(ctx)); });
}

// ---- light.Verify (light/verifier.go:135-151; the replay is light_host.h) -------------------------
// Header.Hash of the requests need_hdr (header_hash_kernel, or the host-leaf route for a header
// outside the kernel's limits) and ValidatorSet.Hash of the untrusted sets of the requests
// need_vals, each distinct tmed_valset pointer once, under one hold of the context's lock;
// submitted blocksync windows are collected first.
static int light_hashes_device(tmed_ctx *ctx, const tmed_light_request *reqs, const std::vector<size_t> &need_hdr,
                               const std::vector<size_t> &need_vals, uint8_t *hdr_hash, uint8_t *hdr_ok,
                               uint8_t *vals_hash) {
  const size_t m = need_hdr.size();
  std::vector<tmed_header> hs;
  hs.reserve(m);
  for (const size_t i : need_hdr) {
    if (!tmed::header_pointers_ok(*reqs[i].header)) return TMED_EINVAL;
    hs.push_back(*reqs[i].header);
  }
  std::unordered_map<const tmed_valset *, size_t> set_of;
  std::vector<const tmed_valset *> sets;
  for (const size_t i : need_vals) {
    const tmed_valset *vs = reqs[i].vals;
    if (!set_of.emplace(vs, sets.size()).second) continue;
    if (vs->n && (!vs->pubkeys || !vs->powers)) return TMED_EINVAL;
    sets.push_back(vs);
  }
  std::vector<uint8_t> ho(32 * std::max<size_t>(m, 1)), ok(std::max<size_t>(m, 1));
  std::vector<uint8_t> so(32 * std::max<size_t>(sets.size(), 1));
  const int rc = tmed::locked(ctx, /*collect=*/true, [&] {
    int r = m ? tmed::header_hashes_locked(ctx, hs.data(), m, ho.data(), ok.data()) : TMED_OK;
    if (r == TMED_OK && !sets.empty()) r = tmed::valsets_hashes_locked(ctx, sets.data(), sets.size(), so.data());
    return r;
  });
  if (rc != TMED_OK) return rc;
  for (size_t j = 0; j < m; j++) {
    memcpy(hdr_hash + 32 * need_hdr[j], ho.data() + 32 * j, 32);
    hdr_ok[need_hdr[j]] = ok[j];
  }
  for (const size_t i : need_vals) memcpy(vals_hash + 32 * i, so.data() + 32 * set_of[reqs[i].vals], 32);
  return TMED_OK;
}

extern "C" int tmed_light_verify(tmed_ctx *ctx, const tmed_light_request *reqs, size_t n, uint32_t flags,
                                 tmed_light_result *out) {
  if (!ctx) return TMED_EINVAL;
  const int rule = tmed::seam_rule(ctx);  // one rule for both of the call's commit batches
  return c_guard(ctx, [&] {
    return tmed_light::light_run(
        reqs, n, flags, out,
        [&](const std::vector<size_t> &need_hdr, const std::vector<size_t> &need_vals, uint8_t *hh, uint8_t *hok,
            uint8_t *vh) { return light_hashes_device(ctx, reqs, need_hdr, need_vals, hh, hok, vh); },
        [&](const tmed_commit_request *rq, size_t m, tmed_commit_result *res) {
          return verify_commits_impl(ctx, rq, m, res, rule);
        });
  });
}

// ---- VerifyLightClientAttack (evidence/verify.go:113-154; the replay is lca_host.h) ----------------
// Header.Hash of both headers of the requests `live` under one hold of the context's lock (submitted
// blocksync windows are collected first), the commit checks as tmed_verify_commits runs them, then
// the byzantine lists and Hash() under another hold (lca.hip lca_tail_locked).
extern "C" int tmed_verify_light_client_attacks(tmed_ctx *ctx, const tmed_lca_request *reqs, size_t n, uint32_t flags,
                                                int32_t *byz, const uint64_t *byz_off, tmed_lca_result *out) {
  if (!ctx) return TMED_EINVAL;
  const int rule = tmed::seam_rule(ctx);
  return c_guard(ctx, [&] {
    return tmed_lca::lca_run(
        reqs, n, flags, byz, byz_off, out,
        [&](const std::vector<size_t> &live, uint8_t *ch, uint8_t *cok, uint8_t *th, uint8_t *tok) {
          const size_t m = live.size();
          std::vector<tmed_header> hs;
          hs.reserve(2 * m);
          for (const size_t i : live) {
            if (!tmed::header_pointers_ok(*reqs[i].conflicting_header) || !tmed::header_pointers_ok(*reqs[i].trusted_header))
              return (int)TMED_EINVAL;
            hs.push_back(*reqs[i].conflicting_header);
            hs.push_back(*reqs[i].trusted_header);
          }
          std::vector<uint8_t> ho(64 * m), ok(2 * m);
          const int rc = tmed::locked(ctx, /*collect=*/true, [&] {
            return tmed::header_hashes_locked(ctx, hs.data(), 2 * m, ho.data(), ok.data());
          });
          if (rc != TMED_OK) return rc;
          for (size_t j = 0; j < m; j++) {
            memcpy(ch + 32 * live[j], ho.data() + 64 * j, 32);
            memcpy(th + 32 * live[j], ho.data() + 64 * j + 32, 32);
            cok[live[j]] = ok[2 * j];
            tok[live[j]] = ok[2 * j + 1];
          }
          return (int)TMED_OK;
        },
        [&](const tmed_commit_request *rq, size_t m, tmed_commit_result *res) {
          return verify_commits_impl(ctx, rq, m, res, rule);
        },
        [&](const std::vector<size_t> &live, const uint8_t *ch, const uint8_t *cok, const std::vector<size_t> &need,
            const int *kinds, tmed_byz_result *bres, uint8_t *ev_hash) {
          return tmed::locked(ctx, /*collect=*/true, [&] {
            return tmed::lca_tail_locked(ctx, reqs, live, ch, cok, need, kinds, byz, byz_off, bres, ev_hash);
          });
        });
  });
}

// ---- validateBlock (state/validation.go:15-151; the replay is validate_host.h) ---------------------
// Three holds of the context's lock, one after the other, as tmed_light_verify takes its own: phase A
// (validate.hip validate_hashes_locked: the last commits staged once into the arena, the hashes, then
// block_check_kernel's masks and proposer indexes; submitted blocksync windows are collected first),
// VerifyCommit as tmed_verify_commits runs it (the seam takes and drops the lock itself, so the call
// cannot keep one hold across it), then MedianTime over the arena's arrays.  Another call on the
// context may run between the holds: a second tmed_validate_blocks would refill the arena, which the
// arena's generation shows, and the medians then stage their commits as tmed_median_times does; and the
// diagnostics (tmed_last_kernel_ms, tmed_validate_kernel_ms, tmed_validate_stats) are the context's
// last writer's, as for every call.
extern "C" int tmed_validate_blocks(tmed_ctx *ctx, const tmed_block_batch *batch, tmed_block_result *out) {
  if (!ctx) return TMED_EINVAL;
  const int rule = tmed::seam_rule(ctx);
  return c_guard(ctx, [&] {
    tmed::CommitArena arena;
    tmed::MedShared shared{nullptr, {}};
    uint64_t gen = 0;
    return tmed_validate::validate_run(
        batch, out,
        [&](const tmed_validate::Plan &plan, tmed_validate::Hashes &H) {
          return tmed::locked(ctx, /*collect=*/true,
                              [&] { return tmed::validate_hashes_locked(ctx, plan, H, &shared, &arena, &gen); });
        },
        [&](const tmed_median_request *mreqs, const std::vector<size_t> &m_of, tmed_median_result *mres,
            const std::vector<size_t> &, int32_t *) {  // the proposers came with phase A
          const size_t m = m_of.size();
          for (size_t j = 0; j < m; j++)
            if (tmed_median::check_request(mreqs[j]) != TMED_OK) return (int)TMED_EINVAL;
          if (m == 0) return (int)TMED_OK;
          return tmed::locked(ctx, /*collect=*/true, [&] {
            const bool mine = shared.arena && gen == ctx->vb_gen;  // the arena still holds this call's commits
            return tmed::median_times_locked(ctx, mreqs, m, mres, mine ? &shared : nullptr);
          });
        },
        [&](const tmed_commit_request *rq, size_t m, tmed_commit_result *res) {
          return verify_commits_impl(ctx, rq, m, res, rule);
        });
  });
}

// ---- free-standing votes: Vote.Verify and the checks of VoteSet.addVote (votes.hip) ---------------
// The requests' sets go through the key-set cache as a commit's do: each request stands in as a
// commit request of as many signatures as it has votes (the cache reads the set and that count only),
// and the device batch runs against the sets the cache resolved.
extern "C" int tmed_verify_votes(tmed_ctx *ctx, const tmed_vote_request *reqs, size_t n_reqs, uint8_t *codes) {
  if (!ctx || (n_reqs && !reqs)) return TMED_EINVAL;
  return c_guard(ctx, [&] {
    size_t total = 0;
    for (size_t q = 0; q < n_reqs; q++) {
      if (tmed_votes_host::check_request(reqs[q]) != TMED_OK) return (int)TMED_EINVAL;
      total += reqs[q].votes->n;
    }
    if (total && !codes) return (int)TMED_EINVAL;
    std::vector<tmed_commit> shadow_commits(n_reqs);
    std::vector<tmed_commit_request> shadow(n_reqs);
    for (size_t q = 0; q < n_reqs; q++) {
      memset(&shadow_commits[q], 0, sizeof(tmed_commit));
      memset(&shadow[q], 0, sizeof(tmed_commit_request));
      shadow_commits[q].n_sigs = reqs[q].votes->n;
      shadow[q].vals = reqs[q].vals;
      shadow[q].commit = &shadow_commits[q];
    }
    KcCall kc;  // pins the cache's pool until the batch below is collected
    const tmed_commit_request *resolved = keycache_resolve(ctx, shadow.data(), n_reqs, kc);
    std::vector<tmed_vote_request> rq(reqs, reqs + n_reqs);
    for (size_t q = 0; q < n_reqs; q++) rq[q].vals = resolved[q].vals;
    return tmed::locked(ctx, /*collect=*/true, [&] { return tmed::verify_votes_locked(ctx, rq.data(), n_reqs, codes); });
  });
}

// ---- evidence: VerifyDuplicateVote (evidence.hip) --------------------------------------------------
// The requests' sets go through the key-set cache as the votes' do: each request stands in as a commit
// request of two signatures per evidence.
extern "C" int tmed_verify_duplicate_votes(tmed_ctx *ctx, const tmed_dup_request *reqs, size_t n_reqs, uint8_t *codes) {
  if (!ctx || (n_reqs && !reqs)) return TMED_EINVAL;
  return c_guard(ctx, [&] {
    size_t total = 0;
    for (size_t q = 0; q < n_reqs; q++) {
      if (tmed_evidence_host::check_request(reqs[q]) != TMED_OK) return (int)TMED_EINVAL;
      total += reqs[q].ev->n;
    }
    if (total && !codes) return (int)TMED_EINVAL;
    std::vector<tmed_commit> shadow_commits(n_reqs);
    std::vector<tmed_commit_request> shadow(n_reqs);
    for (size_t q = 0; q < n_reqs; q++) {
      memset(&shadow_commits[q], 0, sizeof(tmed_commit));
      memset(&shadow[q], 0, sizeof(tmed_commit_request));
      shadow_commits[q].n_sigs = 2 * reqs[q].ev->n;
      shadow[q].vals = reqs[q].vals;
      shadow[q].commit = &shadow_commits[q];
    }
    KcCall kc;  // pins the cache's pool until the batch below is collected
    const tmed_commit_request *resolved = keycache_resolve(ctx, shadow.data(), n_reqs, kc);
    std::vector<tmed_dup_request> rq(reqs, reqs + n_reqs);
    for (size_t q = 0; q < n_reqs; q++) rq[q].vals = resolved[q].vals;
    return tmed::locked(ctx, /*collect=*/true,
                        [&] { return tmed::verify_dup_votes_locked(ctx, rq.data(), n_reqs, codes); });
  });
}

// ---- several GPUs in one process (§8e): contiguous shards balanced by signature count ----

// Shard boundaries over n items whose weights are w(i): shard t = [cut[t], cut[t+1]).
template <class W>
static std::vector<size_t> weighted_cuts(size_t n, size_t parts, W &&w) {
  size_t total = 0;
  for (size_t i = 0; i < n; i++) total += w(i);
  std::vector<size_t> cut(parts + 1, n);
  cut[0] = 0;
  size_t acc = 0, t = 1;
  for (size_t i = 0; i < n && t < parts; i++) {
    acc += w(i);
    while (t < parts && acc * parts >= total * t) cut[t++] = i + 1;
  }
  return cut;
}

template <class F>
static int run_shards(size_t n_ctx, const std::vector<size_t> &cut, F &&f) {
  std::vector<int> rcs(n_ctx, TMED_OK);
  std::vector<std::thread> th;
  for (size_t t = 0; t < n_ctx; t++)
    if (cut[t + 1] > cut[t]) th.emplace_back([&, t] { rcs[t] = f(t, cut[t], cut[t + 1]); });
  for (auto &x : th) x.join();
  for (int rc : rcs)
    if (rc != TMED_OK) return rc;
  return TMED_OK;
}

// Every context present and under one signature rule (a call sharded over contexts of different
// rules would decide its shards differently: TMED_EINVAL).
static bool ctxs_ok(tmed_ctx *const *ctxs, size_t n_ctx) {
  if (!ctxs || n_ctx == 0) return false;
  for (size_t t = 0; t < n_ctx; t++)
    if (!ctxs[t]) return false;
  for (size_t t = 1; t < n_ctx; t++)
    if (tmed::seam_rule(ctxs[t]) != tmed::seam_rule(ctxs[0])) return false;
  return true;
}

extern "C" int tmed_verify_commits_multi(tmed_ctx *const *ctxs, size_t n_ctx, const tmed_commit_request *reqs,
                                         size_t n, tmed_commit_result *out) {
  if (!ctxs_ok(ctxs, n_ctx) || (n && (!reqs || !out))) return TMED_EINVAL;
  for (size_t q = 0; q < n; q++)
    if (check_request(reqs[q]) != TMED_OK) return TMED_EINVAL;
  const auto cut = weighted_cuts(n, n_ctx, [&](size_t q) { return (size_t)reqs[q].commit->n_sigs + 1; });
  return run_shards(n_ctx, cut, [&](size_t t, size_t lo, size_t hi) {
    return tmed_verify_commits(ctxs[t], reqs + lo, hi - lo, out + lo);
  });
}

extern "C" int tmed_blocksync_verify_multi(tmed_ctx *const *ctxs, size_t n_ctx, const tmed_blocksync_window *w,
                                           uint32_t batch_blocks, tmed_commit_result *out) {
  if (!ctxs_ok(ctxs, n_ctx) || !w) return TMED_EINVAL;
  const size_t nb = w->n_blocks;
  if (nb && (!w->vals || !w->block_ids || !w->heights || !w->commits || !out)) return TMED_EINVAL;
  const auto cut = weighted_cuts(nb, n_ctx, [&](size_t h) { return (size_t)w->commits[h].n_sigs + 1; });
  return run_shards(n_ctx, cut, [&](size_t t, size_t lo, size_t hi) {
    tmed_blocksync_window s = *w;
    s.n_blocks = hi - lo;
    s.block_ids = w->block_ids + lo;
    s.heights = w->heights + lo;
    s.commits = w->commits + lo;
    return tmed_blocksync_verify(ctxs[t], &s, batch_blocks, out + lo);
  });
}
