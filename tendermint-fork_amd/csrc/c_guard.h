// c_guard.h — the wrapper of the seam's C entry points (commit.hip, blocksync.h).
#pragma once

#include <mutex>
#include <new>

#include "ctx.h"

// Defined in blocksync.h, whose own entry points run under c_guard (the one cycle between the two
// files): with ctx->mu held, drops the context's blocksync stream if it still holds work.
static void bs_abort_pending(tmed_ctx *ctx, int rc);

// The seam's C entry points: no C++ exception may cross into the caller (a cgo caller would abort).
// A host allocation that fails inside a call (the per-part plan vectors, a window's copies) returns
// TMED_ENOMEM, any other exception TMED_EINTERNAL (never TMED_EHIP: the device is fine).  When the
// context's blocksync stream still holds work (batches in flight, windows not collected), it is
// dropped (bs_abort_pending), so no queued batch still reads the caller's buffers, and its windows' callers
// get the error from tmed_blocksync_wait; an idle stream is left alone, so the failure of one
// synchronous call is not reported to a later, unrelated window.
// The calling thread is bound to the context's device for the call and given its own device back
// on return: a cgo call may run on any OS thread (goroutines migrate), and the _multi entry points
// call in from fresh threads (device 0).
struct DeviceScope {
  int prev = -1;
  explicit DeviceScope(const tmed_ctx *ctx) {
    if (ctx && hipGetDevice(&prev) == hipSuccess && prev != ctx->device) (void)hipSetDevice(ctx->device);
    else prev = -1;
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

template <class F>
static int c_guard(tmed_ctx *ctx, F &&f) {
  int rc;
  DeviceScope dev(ctx);
  try {
    return f();
  } catch (const std::bad_alloc &) {
    rc = TMED_ENOMEM;
  } catch (...) {
    rc = TMED_EINTERNAL;
  }
  if (ctx) {
    try {
      std::lock_guard<std::mutex> lk(ctx->mu);
      bs_abort_pending(ctx, rc);
    } catch (...) {
    }
  }
  return rc;
}
