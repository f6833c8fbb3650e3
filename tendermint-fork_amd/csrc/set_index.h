// set_index.h — the distinct tmed_valset structs of one seam call, numbered in the order of their
// first request (kc_resolve.h keycache_resolve; requests on one struct share its resolution).
// Host C++ only (no HIP, no tmed_ctx): tests/native/set_index_race.cpp compiles the same code under
// ThreadSanitizer with the pool jitter on.
//
// A flat open-addressing table of pointers filled by the host pool without locks (a light-client
// batch: 20k requests on 10k sets; serially the table's cache misses cost ~0.2 ms a call).  Each slot
// keeps the smallest request index that names it, so the set order — and the order keys are appended
// to the cache's pool — does not depend on addresses or on timing.
//
// Parallel regions (parallel_ranges) and what each part reads from outside its own range:
//   fill      reqs (caller, read-only); tkey / tval of any slot, through atomics only (acquire load
//             and pointer CAS on tkey, relaxed load and min-CAS on tval); writes slot[lo, hi)
//   is_first  tval[slot[q]], plainly: final since the fill region ended; writes is_first[lo, hi)
//   (serial)  first[] and tval[slot] = -1 - k (the set index), in request order
//   set_of    tval[slot[q]] (the serial pass above); writes set_of[lo, hi), adds to sigs[k] of any
//             set by a relaxed atomic add (read by the caller after the region)
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/tmed25519.h"
#include "host_pool.h"

namespace {
// Scratch kept across calls by the caller (fresh pages cost a fault per 4 KB on every call).
struct SetIndex {
  std::vector<const tmed_valset *> tkey;  // the table: slot -> set
  std::vector<int32_t> tval;              // slot -> its smallest request index, then -1 - set index
  std::vector<int32_t> set_of;            // request -> set (-1: no vals or no commit)
  std::vector<uint32_t> slot, first;      // request -> slot; set -> the smallest request index naming it
  std::vector<uint8_t> is_first;
  std::vector<size_t> sigs;               // set -> commit->n_sigs summed over its requests
};
}  // namespace

// Workers of the pass (and of the caller's other loops over the call's requests and sets).
static unsigned set_index_threads(size_t n) { return host_threads(n >= 1024 ? ~(size_t)0 : n * 128); }

// The distinct reqs[q].vals pointers, numbered in the order of their first request; returns the
// number of sets.  numbered() runs once first[] is complete, before the per-set sums (not at all
// when there is no set).
template <class Numbered>
static size_t number_sets(const tmed_commit_request *reqs, size_t n, SetIndex &S, Numbered &&numbered) {
  S.set_of.resize(n);
  size_t cap = 16;
  while (cap < 2 * n) cap <<= 1;
  S.tkey.assign(cap, nullptr);
  S.tval.assign(cap, INT32_MAX);
  S.slot.resize(n);
  S.is_first.resize(n);
  const tmed_valset **tkey = S.tkey.data();
  int32_t *tval = S.tval.data();
  uint32_t *slot = S.slot.data();
  const unsigned nt = set_index_threads(n);
  constexpr uint32_t kNoSet = 0xffffffffu;
  parallel_ranges(n, nt, [&](size_t lo, size_t hi, unsigned) {
    for (size_t q = lo; q < hi; q++) {
      const tmed_valset *v = reqs[q].vals;
      if (!v || !reqs[q].commit) {
        slot[q] = kNoSet;
        continue;
      }
      size_t h = (size_t)(((uintptr_t)v >> 4) * 0x9E3779B97F4A7C15ull >> 20) & (cap - 1);
      for (;;) {
        const tmed_valset *cur = __atomic_load_n(&tkey[h], __ATOMIC_ACQUIRE);
        if (cur == v) break;
        if (!cur) {
          const tmed_valset *expect = nullptr;
          if (__atomic_compare_exchange_n(&tkey[h], &expect, v, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) break;
          if (expect == v) break;
        }
        h = (h + 1) & (cap - 1);
      }
      slot[q] = (uint32_t)h;
      int32_t f = __atomic_load_n(&tval[h], __ATOMIC_RELAXED);  // the slot's smallest request index
      while ((int32_t)q < f && !__atomic_compare_exchange_n(&tval[h], &f, (int32_t)q, true, __ATOMIC_RELAXED,
                                                            __ATOMIC_RELAXED)) {
      }
    }
  });
  // a request opens a set when it is its slot's smallest index (read after the region: final)
  uint8_t *is_first = S.is_first.data();
  parallel_ranges(n, nt, [&](size_t lo, size_t hi, unsigned) {
    for (size_t q = lo; q < hi; q++) is_first[q] = slot[q] != kNoSet && tval[slot[q]] == (int32_t)q;
  });
  size_t nsets = 0;
  for (size_t q = 0; q < n; q++) nsets += is_first[q];
  S.first.resize(nsets);
  S.sigs.resize(nsets);
  std::fill(S.sigs.begin(), S.sigs.end(), (size_t)0);
  if (nsets == 0) {
    for (size_t q = 0; q < n; q++) S.set_of[q] = -1;
    return 0;
  }
  for (size_t q = 0, k = 0; q < n; q++)
    if (is_first[q]) {
      S.first[k] = (uint32_t)q;
      tval[slot[q]] = -1 - (int32_t)k;  // slot -> set index (encoded negative: no request index collides)
      k++;
    }
  numbered();
  // request -> set and signatures per set (the policy's amortisation and the counters)
  size_t *sigs = S.sigs.data();
  parallel_ranges(n, nt, [&](size_t lo, size_t hi, unsigned) {
    for (size_t q = lo; q < hi; q++) {
      const int32_t s_ = slot[q] == kNoSet ? -1 : -1 - tval[slot[q]];
      S.set_of[q] = s_;
      if (s_ >= 0) __atomic_fetch_add(&sigs[s_], reqs[q].commit->n_sigs, __ATOMIC_RELAXED);
    }
  });
  return nsets;
}
static size_t number_sets(const tmed_commit_request *reqs, size_t n, SetIndex &S) {
  return number_sets(reqs, n, S, [] {});
}
