// call_frame.h — the frame the host entry points share (host side of the HIP units): check the
// arguments, take ctx->mu (locked), stage into the context's pinned buffers, queue copies and launches
// on the context stream, wait for the stream whatever happened (finish_call), map the error.  The raw
// host batch (keys, signatures, messages in; one byte per signature out) is raw_stage / raw_run, for
// its three public entries and, through slot_batch.h, the host routes of the votes and the evidence.
// slot_batch.h builds the frame of those two calls on this one (grouping by route and key set, the
// device-route envelope around finish_call, verify_sigs).  api_guard.h, included here, is the frame's
// outermost part (guarded); a HIP unit includes this header and has the frame and ctx.h.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#include <mutex>

#include "api_guard.h"
#include "ctx.h"

namespace tmed {

// The regions of a staging buffer (a layout struct per call kind) start at multiples of 256 bytes.
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The device part of a call under ctx->mu.  collect: the call follows the seam's rule (ctx.h
// bs_collect_submitted) and first collects the submitted blocksync windows, then releases the
// completed ones once the lock is dropped (their key-set cache pins take the lock).
template <class F>
int locked(tmed_ctx *c, bool collect, F &&run) {
  int rc;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    rc = collect ? bs_collect_submitted(c) : TMED_OK;
    if (rc == TMED_OK) rc = run();
  }
  if (collect) bs_release_collected(c);
  return rc;
}

// The one exit of every host-side call that has queued a copy or a launch on stream s, taken on a
// failure (rc, the first error) as on success: the queued copies read or write host memory of the
// call's own (plans, offsets, results on its stack), the context's pinned staging or the caller's
// arrays, so the call waits for the stream before any of them goes away or is reused.  ms: on success,
// the time between ev0 and ev1, which the call recorded around its kernels of record.
inline int finish_call(tmed_ctx *c, hipStream_t s, int rc, float *ms = nullptr) {
  const int rs = map_err(hipStreamSynchronize(s));
  if (rc == TMED_OK) rc = rs;
  if (rc == TMED_OK && ms) (void)hipEventElapsedTime(ms, c->ev0, c->ev1);
  return rc;
}
inline int finish_call(tmed_ctx *c, hipStream_t s, hipError_t e, float *ms = nullptr) {
  return finish_call(c, s, map_err(e), ms);
}

// ---- the raw host batch ------------------------------------------------------------------------------
// n messages [off[i], off[i+1]) of msgs, in order, and an array for them unless all are empty.
inline int check_offsets(const uint32_t *off, size_t n, const void *msgs) {
  for (size_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) return TMED_EINVAL;
  return off[n] && !msgs ? TMED_EINVAL : TMED_OK;
}

// The arguments of a raw host batch; an empty batch is TMED_OK and the caller returns it.
inline int check_raw_batch(const tmed_ctx *c, const void *keys, const void *sigs, const void *msgs, const uint32_t *off,
                           size_t n, const void *out) {
  if (!c || !out) return TMED_EINVAL;
  if (n == 0) return TMED_OK;
  if (!keys || !sigs || !off || n > 0xffffffffu) return TMED_EINVAL;
  return check_offsets(off, n, msgs);
}

// A batch of n signatures with key_bytes a key (32: encodings, 4: key-set indexes) and mbytes of
// messages, staged in the context's pinned buffers: the caller's arrays may be pageable, or memory a
// garbage collector owns (Go), so no queued copy reads them (the ZIP-215 entry alone keeps its copies
// from the caller's arrays, for its measured speed).  ctx->mu held from raw_stage to raw_run's end.
struct RawStage {
  size_t n = 0, key_bytes = 0, mbytes = 0;
  uint8_t *keys = nullptr, *sigs = nullptr, *msgs = nullptr;  // the sources of the copies in: pinned, the caller fills them
  uint32_t *off = nullptr;                                    // n + 1 message offsets
  float ms = 0.f;  // raw_run: the kernels' time when it was asked to time them, else 0
};

// Grows the device buffers and their pinned mirrors; nothing is queued.  pinned = false: only the
// pinned h_out grows, and the caller points the four sources at arrays that outlive the call (raw_run
// waits for the stream before it returns).  (static: no out-of-line copy joins the library's dynamic symbols.)
static int raw_stage(tmed_ctx *c, size_t key_bytes, size_t n, size_t mbytes, RawStage &st, bool pinned = true) {
  const size_t bytes[5] = {n * key_bytes, n * 64, mbytes + 16, (n + 1) * 4, n};
  DevBuf *const d[5] = {&c->d_a, &c->d_b, &c->d_msg, &c->d_off, &c->d_out};
  HostBuf *const h[5] = {&c->h_a, &c->h_b, &c->h_msg, &c->h_off, &c->h_out};
  hipError_t e = hipSuccess;
  for (int i = 0; i < 5 && e == hipSuccess; i++) e = d[i]->ensure(bytes[i]);
  for (int i = pinned ? 0 : 4; i < 5 && e == hipSuccess; i++) e = h[i]->ensure(bytes[i]);
  if (e != hipSuccess) return map_err(e);
  st = RawStage{n, key_bytes, mbytes};
  if (pinned) {
    st.keys = (uint8_t *)c->h_a.p, st.sigs = (uint8_t *)c->h_b.p, st.msgs = (uint8_t *)c->h_msg.p;
    st.off = (uint32_t *)c->h_off.p;
  }
  return TMED_OK;
}

// The staged batch through the device: the four copies in, run(d_keys, d_sigs, d_msgs, d_off, n, d_out,
// stream) -> TMED_* inside a scratch_acquire / scratch_release pair (timed: ev0 / ev1 around it, a
// small batch skips them: they add ~8 us to the call), the bits back through the pinned h_out into
// out, and the reference's length rule: a signature whose length is not 64 is rejected
// (crypto/ed25519/ed25519.go:150-152).
template <class Run>
int raw_run(tmed_ctx *c, RawStage &st, bool timed, Run &&run, uint8_t *out, const uint32_t *sig_lens) {
  const size_t n = st.n, moff = (n + 1) * 4;
  hipStream_t s = c->stream;
  hipError_t e = hipMemcpyAsync(c->d_a.p, st.keys, n * st.key_bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(c->d_b.p, st.sigs, n * 64, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && st.mbytes) e = hipMemcpyAsync(c->d_msg.p, st.msgs, st.mbytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(c->d_off.p, st.off, moff, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = scratch_acquire(c, s);
  const bool acquired = e == hipSuccess;
  if (e == hipSuccess && timed) e = hipEventRecord(c->ev0, s);
  int rc = map_err(e);
  if (rc == TMED_OK)
    rc = run((const uint8_t *)c->d_a.p, (const uint8_t *)c->d_b.p, (const uint8_t *)c->d_msg.p,
             (const uint32_t *)c->d_off.p, (uint32_t)n, (uint8_t *)c->d_out.p, s);
  if (rc == TMED_OK && timed) rc = map_err(hipEventRecord(c->ev1, s));
  if (acquired) {
    const int rr = map_err(scratch_release(c, s));
    if (rc == TMED_OK) rc = rr;
  }
  if (rc == TMED_OK) rc = map_err(hipMemcpyAsync(c->h_out.p, c->d_out.p, n, hipMemcpyDeviceToHost, s));
  rc = finish_call(c, s, rc, timed ? &st.ms : nullptr);
  if (rc != TMED_OK) return rc;
  memcpy(out, c->h_out.p, n);
  if (sig_lens)
    for (size_t i = 0; i < n; i++)
      if (sig_lens[i] != 64) out[i] = 0;
  return TMED_OK;
}

}  // namespace tmed
