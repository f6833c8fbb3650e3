// api_guard.h — no C++ exception crosses the C ABI (a cgo caller would abort).  Host C++ only, no HIP
// include: seam_host.h uses it in the host-only test builds too.
#pragma once

#include <new>

#include "../../include/tmed25519.h"

// body checks the arguments, builds the call's host vectors and runs it.  A host allocation that
// fails returns TMED_ENOMEM, any other exception TMED_EINTERNAL (never TMED_EHIP: the device is fine).
template <class F>
static int guarded(F &&body) {
  try {
    return body();
  } catch (const std::bad_alloc &) {
    return TMED_ENOMEM;
  } catch (...) {
    return TMED_EINTERNAL;
  }
}
