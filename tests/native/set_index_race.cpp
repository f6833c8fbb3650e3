// set_index_race.cpp — TEST-ONLY: the set numbering of the key-set cache's resolution
// (csrc/set_index.h number_sets, the code kc_resolve.h keycache_resolve runs) with the product's own
// parallelism, built with ThreadSanitizer by tests/test_native_sanitizers.py and run with the pool
// jitter on.  Three calls of 2,048 requests (the pass is serial below 512): a few shared sets in a
// scrambled order with some requests lacking their set or commit, one set per request (the table at
// its 2n capacity rule: probing), and no set at all.
//
// Checks the numbering against a serial restatement and exits non-zero on a miss; prints a digest of
// set_of, first and sigs, which the test compares with a run on one host thread.
//
// usage: set_index_race JITTER_US SEED
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <unordered_map>
#include <vector>

#include "set_index.h"

namespace {

constexpr size_t kRequests = 2048;

uint64_t g_digest = 1469598103934665603ull;
void mix(uint64_t x) { g_digest = (g_digest ^ x) * 1099511628211ull; }

// One call: number the sets, check every property, fold the arrays into the digest.
bool run_case(const char *name, const std::vector<tmed_commit_request> &reqs, SetIndex &S, size_t want_sets) {
  const size_t n = reqs.size();
  const size_t nsets = number_sets(reqs.data(), n, S);
  size_t bad = 0;
  auto miss = [&](const char *what, size_t at) {
    if (bad++ < 5) printf("%s: %s at %zu\n", name, what, at);
  };
  if (nsets != want_sets || S.first.size() != nsets || S.sigs.size() != nsets) miss("set count", nsets);
  for (size_t k = 0; k < nsets && !bad; k++) {
    if (k && S.first[k] <= S.first[k - 1]) miss("first[] not strictly increasing", k);
    if (S.first[k] >= n || S.set_of[S.first[k]] != (int32_t)k) miss("set_of[first[k]] != k", k);
  }
  // every request's set is that of the first request with its pointer; the serial sums
  std::unordered_map<const tmed_valset *, size_t> first_of;
  std::vector<size_t> sums(nsets, 0);
  for (size_t q = 0; q < n && !bad; q++) {
    const int32_t s = S.set_of[q];
    if (!reqs[q].vals || !reqs[q].commit) {
      if (s != -1) miss("a request without set or commit has a set", q);
      continue;
    }
    const size_t f = first_of.emplace(reqs[q].vals, q).first->second;
    if (s < 0 || (size_t)s >= nsets || s != S.set_of[f] || S.first[s] != f) miss("set_of differs from its first request's", q);
    else sums[s] += reqs[q].commit->n_sigs;
  }
  for (size_t k = 0; k < nsets && !bad; k++)
    if (S.sigs[k] != sums[k]) miss("sigs[k] != serial sum", k);
  for (size_t q = 0; q < n; q++) mix((uint64_t)(int64_t)S.set_of[q]);
  for (size_t k = 0; k < nsets; k++) {
    mix(S.first[k]);
    mix(S.sigs[k]);
  }
  printf("%s: requests %zu sets %zu misses %zu\n", name, n, nsets, bad);
  return bad == 0;
}

}  // namespace

int main(int argc, char **argv) {
  const int jitter = argc > 1 ? atoi(argv[1]) : 0;
  const uint64_t seed = argc > 2 ? (uint64_t)atoll(argv[2]) : 7;
  g_pool_jitter_us.store(jitter);
  std::mt19937_64 rng(seed);
  std::vector<tmed_valset> vals(kRequests);
  std::vector<tmed_commit> commits(kRequests);
  for (size_t q = 0; q < kRequests; q++) commits[q].n_sigs = 1 + (size_t)(rng() % 997);  // sums tell the sets apart
  SetIndex S;  // kept across the calls, as the product keeps it
  bool ok = true;

  // a few shared sets, scrambled; every 97th request without its set, every 101st without its commit
  std::vector<tmed_commit_request> reqs(kRequests);
  size_t shared = 0;
  {
    std::vector<uint8_t> used(5, 0);
    for (size_t q = 0; q < kRequests; q++) {
      const size_t s = (size_t)(rng() % 5);
      reqs[q] = tmed_commit_request{};
      reqs[q].vals = q % 97 == 0 ? nullptr : &vals[s];
      reqs[q].commit = q % 101 == 0 ? nullptr : &commits[q];
      if (reqs[q].vals && reqs[q].commit) used[s] = 1;
    }
    for (uint8_t u : used) shared += u;
  }
  ok = run_case("shared", reqs, S, shared) && ok;

  // one set per request
  for (size_t q = 0; q < kRequests; q++) {
    reqs[q].vals = &vals[q];
    reqs[q].commit = &commits[q];
  }
  ok = run_case("distinct", reqs, S, kRequests) && ok;

  // no set at all
  for (size_t q = 0; q < kRequests; q++) {
    reqs[q].vals = nullptr;
    reqs[q].commit = q & 1 ? &commits[q] : nullptr;
  }
  ok = run_case("none", reqs, S, 0) && ok;

  printf("digest %016llx\n", (unsigned long long)g_digest);
  return ok ? 0 : 1;
}
