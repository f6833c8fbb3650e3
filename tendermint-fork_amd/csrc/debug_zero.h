// debug_zero.h — the seam's diagnostics-only entry points: the TMED_DEBUG_ZERO recorder of the
// blocksync stream (blocksync.h bs_finish) and the host pool's test jitter.  Part of commit.hip's
// translation unit, after seam_host.h.
#pragma once

#include <mutex>
#include <vector>

#include "ctx.h"

// TMED_DEBUG_ZERO=1 (diagnostics only): every staged candidate of a pipelined generic batch whose
// device bit is 0 is recorded with what the host staged (key, signature), what the device held
// (its copy of both, the assembled sign-bytes) and which request / signature it was, for
// tmed_debug_zero_bits.  It tells a false reject from the verification kernels apart from one
// in the staging, the copy or the assembly.
namespace {
struct ZeroRec {
  uint64_t req;  // request index in the call's window
  int32_t sig;   // signature index in its commit
  uint32_t pos, msg_len, batch_m;
  uint8_t key_host[32], sig_host[64], key_dev[32], sig_dev[64], msg[256];
};
std::mutex g_zero_mu;
std::vector<ZeroRec> g_zero;
bool debug_zero_on() {
  static const bool on = getenv("TMED_DEBUG_ZERO") != nullptr;
  return on;
}
}  // namespace

// The zero bits of one collected batch: its staging, candidates and staged segments, the collected
// bits in staging order, and the batch's first request in its window.
static void debug_record_zeros(tmed_ctx *ctx, const tmed::VoteStage &st, const Cands &cands, const Group &grp,
                               const std::vector<uint8_t> &bits, size_t lo) {
  if (st.ks || st.zc || st.sig_direct) return;  // generic staged batches only
  const tmed::VoteSlot &vs = ctx->vslot[st.slot];
  const size_t m = bits.size();
  std::vector<ZeroRec> recs;
  for_segments(cands, grp, 0, m, [&](size_t j, uint32_t u0, uint32_t u1, size_t p0) {
    const Run &run = cands.runs[grp.run(cands, j)];
    for (uint32_t u = u0; u < u1; u++) {
      const size_t p = p0 + (u - u0);
      if (bits[p]) continue;
      ZeroRec z{};
      z.req = lo + run.req;
      z.sig = run.sig + (int32_t)u;
      z.pos = (uint32_t)p;
      z.batch_m = (uint32_t)m;
      memcpy(z.key_host, st.key + 32 * p, 32);
      memcpy(z.sig_host, st.sig + 64 * p, 64);
      const uint8_t *d = (const uint8_t *)vs.d_votes.p;
      (void)hipMemcpy(z.key_dev, d + st.o_key + 32 * p, 32, hipMemcpyDeviceToHost);
      (void)hipMemcpy(z.sig_dev, d + st.o_sig + 64 * p, 64, hipMemcpyDeviceToHost);
      (void)hipMemcpy(z.msg, (const uint8_t *)vs.d_vmsg.p + (size_t)tmed::kVoteSlot * p, 256, hipMemcpyDeviceToHost);
      (void)hipMemcpy(&z.msg_len, (const uint32_t *)vs.d_off.p + p, 4, hipMemcpyDeviceToHost);
      recs.push_back(z);
    }
  });
  std::lock_guard<std::mutex> g(g_zero_mu);
  g_zero.insert(g_zero.end(), recs.begin(), recs.end());
}

// The recorded zero bits (TMED_DEBUG_ZERO), oldest first: copies up to cap records of
// sizeof(ZeroRec) bytes into out and removes them; *n = records copied.
extern "C" int tmed_debug_zero_bits(void *out, size_t cap, size_t *n) {
  std::lock_guard<std::mutex> g(g_zero_mu);
  const size_t k = std::min(cap, g_zero.size());
  if (k && out) memcpy(out, g_zero.data(), k * sizeof(ZeroRec));
  g_zero.erase(g_zero.begin(), g_zero.begin() + (ptrdiff_t)k);
  if (n) *n = k;
  return (int)sizeof(ZeroRec);
}

// Tests: every host-pool part starts up to max_us microseconds late (0: off), see host_pool.h.
extern "C" void tmed_test_pool_jitter(int max_us) { g_pool_jitter_us.store(max_us < 0 ? 0 : max_us); }
