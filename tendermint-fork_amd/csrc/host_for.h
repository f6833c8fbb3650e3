// host_for.h — a short-lived fork-join over host threads for the calls that pack many commits or
// sets into pinned staging (merkle.hip, median.hip): host_for runs the loop, pack_threads sizes it.
#pragma once
#include <stdlib.h>

#include <algorithm>
#include <thread>
#include <vector>

namespace tmed {

// f(i) for i in [0, n) on up to `threads` host threads (contiguous shares).
template <class F>
void host_for(size_t n, unsigned threads, F &&f) {
  if (threads <= 1 || n < 2) {
    for (size_t i = 0; i < n; i++) f(i);
    return;
  }
  threads = (unsigned)std::min<size_t>(threads, n);
  std::vector<std::thread> ts;
  ts.reserve(threads);
  auto share = [&](unsigned t) {
    for (size_t i = n * t / threads; i < n * (t + 1) / threads; i++) f(i);
  };
  for (unsigned t = 1; t < threads; t++) {
    try {
      ts.emplace_back(share, t);
    } catch (...) {  // no thread to be had: the caller runs that share
      share(t);
    }
  }
  share(0);
  for (auto &t : ts) t.join();
}

inline unsigned pack_threads(size_t sigs) {
  if (sigs < (1u << 16)) return 1;
  const char *v = getenv("TMED_HOST_THREADS");  // as the seam's host pool: 16 by default
  const unsigned want = v ? (unsigned)std::max(1, atoi(v)) : 16u;
  return std::min(want, std::max(1u, std::thread::hardware_concurrency()));
}

}  // namespace tmed
