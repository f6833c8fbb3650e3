// c_guard.h — the wrapper of the seam's C entry points (commit.hip, blocksync.h): guarded
// (api_guard.h) plus the device scope and the recovery of the context's blocksync stream.
#pragma once

#include <mutex>

#include "api_guard.h"
#include "ctx.h"

// Defined in blocksync.h, whose own entry points run under c_guard (the one cycle between the two
// files): with ctx->mu held, drops the context's blocksync stream if it still holds work.
static void bs_abort_pending(tmed_ctx *ctx, int rc);

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

// What c_guard adds over guarded, whose mapping of an exception to TMED_ENOMEM / TMED_EINTERNAL it
// keeps: the DeviceScope, and, after an exception only (never after an error f returned), the
// recovery of the context's blocksync stream.  When that stream still holds work (batches in flight,
// windows not collected), it is dropped (bs_abort_pending), so no queued batch still reads the
// caller's buffers, and its windows' callers get the error from tmed_blocksync_wait; an idle stream
// is left alone, so the failure of one synchronous call is not reported to a later, unrelated window.
template <class F>
static int c_guard(tmed_ctx *ctx, F &&f) {
  DeviceScope dev(ctx);
  bool threw = true;
  const int rc = guarded([&] {
    const int r = f();
    threw = false;
    return r;
  });
  if (threw && ctx) {
    (void)guarded([&] {
      std::lock_guard<std::mutex> lk(ctx->mu);
      bs_abort_pending(ctx, rc);
      return rc;
    });
  }
  return rc;
}
