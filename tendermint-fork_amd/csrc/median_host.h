// median_host.h — state.MedianTime (state/state.go:268-285) over tmtime.WeightedMedian
// (types/time/time.go:35-58) without a device: tmed_median_times_host, and the route
// tmed_median_times gives every pair its kernels do not take (csrc/median.hip).  include/tmed25519.h
// states the rule and its outcome codes; DESIGN.md §4.6 derives why the reference's sort-and-walk
// equals "the smallest entering key t with W(<= t) >= median" for non-negative weights.  The pieces
// both the kernels and the host use (the sort key, the weight sum) are TMED_HD.  Otherwise host C++
// only (no HIP): tests/native/median_host.cpp compiles this file under AddressSanitizer and
// UndefinedBehaviorSanitizer.
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <unordered_map>
#include <vector>

#include "../../include/tmed25519.h"
#include "keycache.h"  // AddrIndex: GetByAddress as a hash lookup, first match in set order

#include "vote_wire.h"  // TMED_HD; the zero time

namespace tmed_median {

constexpr int64_t kNanos = 1000000000ll;
constexpr int64_t kZeroTimeSeconds = tmed::kMinSeconds;  // time.Time{}.Unix(): 0001-01-01T00:00:00Z

// Time.UnixNano() = seconds * 1e9 + nanos (the sort key, time.go:46) when that is an int64 and nanos
// is a Time's nanosecond field; false otherwise (Go's UnixNano is then undefined: GO_PATH).
// int64 holds [-9223372036.854775808 s, 9223372036.854775807 s].
TMED_HD bool unix_nano(int64_t sec, int32_t nanos, int64_t *key) {
  constexpr int64_t kLoSec = -9223372037ll, kHiSec = 9223372036ll;
  if (nanos < 0 || nanos >= kNanos || sec < kLoSec || sec > kHiSec) return false;
  if ((sec == kLoSec && nanos < 145224192) || (sec == kHiSec && nanos > 854775807)) return false;
  *key = (int64_t)((uint64_t)sec * (uint64_t)kNanos + (uint64_t)(int64_t)nanos);  // exact: the true value fits
  return true;
}

// The Time of a key: floor division, nanos in [0, 1e9).
TMED_HD void key_time(int64_t key, int64_t *sec, int32_t *nanos) {
  int64_t s = key / kNanos, n = key % kNanos;
  if (n < 0) {
    s--;
    n += kNanos;
  }
  *sec = s;
  *nanos = (int32_t)n;
}

// acc += w for acc, w in [0, 2^63); false (acc unchanged) when the sum is not an int64.
TMED_HD bool add_weight(int64_t *acc, int64_t w) {
  const uint64_t s = (uint64_t)*acc + (uint64_t)w;
  if (s >> 63) return false;
  *acc = (int64_t)s;
  return true;
}

struct Entry {
  int64_t key, w;
};

// The smallest key t of e with W(<= t) >= median, for 0 <= median <= the sum of the weights, all
// weights >= 0 and e not empty: a three-way quickselect on the key that carries the weight below
// the range along (expected O(n); after 64 rounds the rest is sorted and walked, so chosen
// timestamps cannot make it quadratic).  Reorders e.
inline int64_t weighted_select(std::vector<Entry> &e, int64_t median) {
  size_t lo = 0, hi = e.size();
  int64_t below = 0;  // the weight of every key smaller than those in [lo, hi)
  for (int round = 0; round < 64; round++) {
    const int64_t a = e[lo].key, b = e[lo + (hi - lo) / 2].key, c = e[hi - 1].key;
    const int64_t pivot = std::max(std::min(a, b), std::min(std::max(a, b), c));
    size_t lt = lo, i = lo, gt = hi;  // [lo, lt) < pivot, [lt, i) == pivot, [gt, hi) > pivot
    int64_t wl = 0, we = 0;
    while (i < gt) {
      if (e[i].key < pivot) {
        wl += e[i].w;
        std::swap(e[lt++], e[i++]);
      } else if (e[i].key > pivot) {
        std::swap(e[i], e[--gt]);
      } else {
        we += e[i++].w;
      }
    }
    if (lt > lo && below + wl >= median) {
      hi = lt;
    } else if (below + wl + we >= median) {
      return pivot;
    } else {
      below += wl + we;
      lo = gt;
    }
  }
  std::sort(e.begin() + lo, e.begin() + hi, [](const Entry &x, const Entry &y) { return x.key < y.key; });
  for (size_t i = lo; i < hi; i++) {
    below += e[i].w;
    if (below >= median) return e[i].key;
  }
  return e[hi - 1].key;  // not reached: the weights of [lo, hi) reach median
}

// TMED_EINVAL: a NULL array that a non-empty commit or set needs.
inline int check_request(const tmed_median_request &r) {
  if (!r.commit || !r.vals) return TMED_EINVAL;
  const tmed_commit &c = *r.commit;
  if (c.n_sigs && (!c.flags || !c.addresses || !c.ts_seconds || !c.ts_nanos)) return TMED_EINVAL;
  if (r.vals->n && (!r.vals->addresses || !r.vals->powers)) return TMED_EINVAL;
  return TMED_OK;
}

inline void set_zero_time(tmed_median_result &o) {
  o.code = TMED_MEDIAN_ZERO_TIME;
  o.seconds = kZeroTimeSeconds;
  o.nanos = 0;
}

// MedianTime(commit, vals) of one checked pair.  ix: vals' address index; e: scratch.
inline void median_pair(const tmed_commit &c, const tmed_valset &v, const tmed::AddrIndex &ix, std::vector<Entry> &e,
                        tmed_median_result &o) {
  memset(&o, 0, sizeof(o));
  e.clear();
  int64_t total = 0;
  for (size_t i = 0; i < c.n_sigs; i++) {
    if (c.flags[i] == 1) continue;                            // commitSig.Absent(), state.go:273
    if (c.address_lens && c.address_lens[i] != 20) continue;  // bytes.Equal with a 20-byte address
    const uint8_t *a = c.addresses + 20 * i;
    int32_t vi = ix.at(a, i);
    if (vi == -2) vi = ix.find(a);
    if (vi < 0) continue;  // validator == nil, state.go:278
    Entry x;
    x.w = v.powers[vi];
    if (!unix_nano(c.ts_seconds[i], c.ts_nanos[i], &x.key) || x.w < 0 || !add_weight(&total, x.w)) {
      o.code = TMED_MEDIAN_GO_PATH;
      return;
    }
    e.push_back(x);
  }
  o.entered = (uint32_t)e.size();
  if (e.empty()) return set_zero_time(o);
  o.code = TMED_MEDIAN_OK;
  key_time(weighted_select(e, total / 2), &o.seconds, &o.nanos);
}

// The address index of each distinct tmed_valset pointer of a call, built at its first use.
struct SetIndexes {
  std::unordered_map<const tmed_valset *, tmed::AddrIndex> by_set;
  const tmed::AddrIndex &get(const tmed_valset &v) {
    auto it = by_set.find(&v);
    if (it == by_set.end()) {
      it = by_set.emplace(&v, tmed::AddrIndex()).first;
      it->second.build(v.addresses, v.n);
    }
    return it->second;
  }
};

// Checked requests which[0 .. m) -> out[which[j]].
inline void median_run(const tmed_median_request *reqs, const size_t *which, size_t m, SetIndexes &sets,
                       tmed_median_result *out) {
  std::vector<Entry> e;
  for (size_t j = 0; j < m; j++) {
    const tmed_median_request &r = reqs[which[j]];
    median_pair(*r.commit, *r.vals, sets.get(*r.vals), e, out[which[j]]);
  }
}

inline int median_times_host(const tmed_median_request *reqs, size_t n, tmed_median_result *out) {
  if (n == 0) return TMED_OK;
  if (!reqs || !out) return TMED_EINVAL;
  std::vector<size_t> all(n);
  for (size_t i = 0; i < n; i++) {
    if (check_request(reqs[i]) != TMED_OK) return TMED_EINVAL;
    all[i] = i;
  }
  SetIndexes sets;
  median_run(reqs, all.data(), n, sets, out);
  return TMED_OK;
}

}  // namespace tmed_median
