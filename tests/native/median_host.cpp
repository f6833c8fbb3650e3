// median_host.cpp — TEST-ONLY stand-alone host program: state.MedianTime as csrc/median_host.h
// computes it (tmed_median_times_host and the host route of tmed_median_times), over pairs read
// from a text file, one outcome per line on stdout; then self-checks of the key's range, of the
// weighted quickselect against a sort-and-walk (its sorted fallback included) and of the malformed
// calls.  tests/test_median_host.py builds it with -fsanitize=address,undefined and runs it as a
// plain executable:
//   g++ -std=c++17 -fsanitize=address,undefined -I tendermint-fork_amd/csrc median_host.cpp
// Input, blank-separated:
//   pair <n_sigs> <n_vals>            n_vals = -1: the previous pair's set (the same tmed_valset)
//   s <flag> <address_len> <address hex or -> <seconds> <nanos>      n_sigs lines
//   v <address hex> <power>                                         n_vals lines
// Output per pair: code seconds nanos entered.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "median_host.h"

#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      fprintf(stderr, "median_host.cpp:%d: %s\n", __LINE__, #c); \
      return 1;                                                  \
    }                                                            \
  } while (0)

// Arrays of exactly the sizes the structs promise: the sanitizer sees any byte read past them.
struct Set {
  std::vector<uint8_t> addr;
  std::vector<int64_t> power;
  tmed_valset c;
  void finish() {
    memset(&c, 0, sizeof(c));
    c.n = power.size();
    c.addresses = addr.data();
    c.powers = power.data();
  }
};
struct Commit {
  std::vector<uint8_t> flags, addr;
  std::vector<uint32_t> alen;
  std::vector<int64_t> sec;
  std::vector<int32_t> nanos;
  tmed_commit c;
  void finish() {
    memset(&c, 0, sizeof(c));
    c.n_sigs = flags.size();
    c.flags = flags.data();
    c.addresses = addr.data();
    c.address_lens = alen.data();
    c.ts_seconds = sec.data();
    c.ts_nanos = nanos.data();
  }
};

static void unhex(const std::string &s, uint8_t *out, size_t cap) {
  if (s == "-") return;
  for (size_t i = 0; 2 * i + 1 < s.size() && i < cap; i++) out[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
}

static int run_file(const char *path) {
  std::ifstream in(path);
  std::vector<std::unique_ptr<Commit>> commits;
  std::vector<std::unique_ptr<Set>> sets;
  std::vector<tmed_median_request> reqs;
  std::string tok;
  while (in >> tok) {
    if (tok != "pair") return 2;
    long long ns, nv;
    if (!(in >> ns >> nv)) return 2;
    commits.emplace_back(new Commit);
    Commit &cm = *commits.back();
    for (long long i = 0; i < ns; i++) {
      std::string tag, hex;
      unsigned flag, alen;
      long long sec, nanos;
      if (!(in >> tag >> flag >> alen >> hex >> sec >> nanos) || tag != "s") return 2;
      cm.flags.push_back((uint8_t)flag);
      cm.alen.push_back(alen);
      cm.addr.resize(cm.addr.size() + 20, 0);
      unhex(hex, cm.addr.data() + 20 * i, 20);
      cm.sec.push_back(sec);
      cm.nanos.push_back((int32_t)nanos);
    }
    cm.finish();
    if (nv >= 0) {
      sets.emplace_back(new Set);
      Set &vs = *sets.back();
      for (long long i = 0; i < nv; i++) {
        std::string tag, hex;
        long long power;
        if (!(in >> tag >> hex >> power) || tag != "v") return 2;
        vs.addr.resize(vs.addr.size() + 20, 0);
        unhex(hex, vs.addr.data() + 20 * i, 20);
        vs.power.push_back(power);
      }
      vs.finish();
    }
    if (sets.empty()) return 2;
    reqs.push_back(tmed_median_request{&cm.c, &sets.back()->c});
  }
  std::vector<tmed_median_result> out(reqs.size());
  if (tmed_median::median_times_host(reqs.data(), reqs.size(), out.data()) != TMED_OK) return 3;
  for (const tmed_median_result &o : out)
    printf("%d %" PRId64 " %d %u\n", o.code, o.seconds, o.nanos, o.entered);
  // each pair alone gives the same outcome as inside the batch
  for (size_t i = 0; i < reqs.size(); i++) {
    tmed_median_result one;
    if (tmed_median::median_times_host(&reqs[i], 1, &one) != TMED_OK) return 3;
    if (one.code != out[i].code || one.seconds != out[i].seconds || one.nanos != out[i].nanos || one.entered != out[i].entered)
      return 4;
  }
  return 0;
}

static int64_t sort_and_walk(std::vector<tmed_median::Entry> e, int64_t median) {
  std::stable_sort(e.begin(), e.end(), [](const tmed_median::Entry &a, const tmed_median::Entry &b) { return a.key < b.key; });
  for (const tmed_median::Entry &x : e) {  // time.go:48-56
    if (median <= x.w) return x.key;
    median -= x.w;
  }
  return e.back().key;
}

static int self_checks() {
  using namespace tmed_median;
  int64_t k, s;
  int32_t ns;
  CHECK(unix_nano(-9223372037ll, 145224192, &k) && k == INT64_MIN);
  CHECK(!unix_nano(-9223372037ll, 145224191, &k) && !unix_nano(-9223372038ll, 999999999, &k));
  CHECK(unix_nano(9223372036ll, 854775807, &k) && k == INT64_MAX);
  CHECK(!unix_nano(9223372036ll, 854775808, &k) && !unix_nano(9223372037ll, 0, &k));
  CHECK(!unix_nano(INT64_MIN, 0, &k) && !unix_nano(INT64_MAX, 0, &k) && !unix_nano(18446744074ll, 0, &k));
  CHECK(!unix_nano(5, -1, &k) && !unix_nano(5, 1000000000, &k) && !unix_nano(5, INT32_MIN, &k));
  CHECK(unix_nano(-1, 999999999, &k) && k == -1 && unix_nano(0, 0, &k) && k == 0);
  key_time(INT64_MIN, &s, &ns);
  CHECK(s == -9223372037ll && ns == 145224192);
  key_time(INT64_MAX, &s, &ns);
  CHECK(s == 9223372036ll && ns == 854775807);
  key_time(-1, &s, &ns);
  CHECK(s == -1 && ns == 999999999);
  int64_t acc = INT64_MAX - 1;
  CHECK(add_weight(&acc, 1) && acc == INT64_MAX && !add_weight(&acc, 1) && acc == INT64_MAX && add_weight(&acc, 0));

  // the quickselect against the reference's sort and walk
  uint64_t x = 88172645463325252ull;
  auto next = [&] {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    return x;
  };
  for (int round = 0; round < 400; round++) {
    const size_t n = 1 + next() % 300;
    std::vector<Entry> e(n);
    int64_t total = 0;
    for (Entry &y : e) {
      y.key = round % 3 == 0 ? (int64_t)(next() % 5) - 2 : (int64_t)next();
      y.w = round % 5 == 0 ? (int64_t)(next() % 2) : (int64_t)(next() % 1000);
      total += y.w;
    }
    for (const int64_t median : {total / 2, (int64_t)0, total}) {
      std::vector<Entry> copy = e;
      CHECK(weighted_select(copy, median) == sort_and_walk(e, median));
    }
  }
  {  // a key order on which the median-of-three pivot peels few elements a round: the sorted fallback
    const size_t n = 4096;
    std::vector<Entry> e(n);
    for (size_t i = 0; i < n; i++) e[i] = Entry{(int64_t)(i % 2 ? n - i : i), 1};
    for (const int64_t median : {(int64_t)1, (int64_t)n / 2, (int64_t)n}) {
      std::vector<Entry> copy = e;
      CHECK(weighted_select(copy, median) == sort_and_walk(e, median));
    }
    std::vector<Entry> sorted(n), copy;
    for (size_t i = 0; i < n; i++) sorted[i] = Entry{(int64_t)i, (int64_t)(i % 3)};
    copy = sorted;
    CHECK(weighted_select(copy, 1365) == sort_and_walk(sorted, 1365));
  }

  // malformed calls
  Commit cm;
  Set vs;
  cm.flags = {2};
  cm.addr.assign(20, 7);
  cm.alen = {20};
  cm.sec = {5};
  cm.nanos = {6};
  cm.finish();
  vs.addr.assign(20, 7);
  vs.power = {9};
  vs.finish();
  tmed_median_request r{&cm.c, &vs.c};
  tmed_median_result o;
  CHECK(median_times_host(&r, 1, &o) == TMED_OK && o.code == TMED_MEDIAN_OK && o.seconds == 5 && o.nanos == 6 &&
        o.entered == 1 && o.on_device == 0);
  CHECK(median_times_host(nullptr, 0, nullptr) == TMED_OK);
  CHECK(median_times_host(nullptr, 1, &o) == TMED_EINVAL && median_times_host(&r, 1, nullptr) == TMED_EINVAL);
  for (int field = 0; field < 8; field++) {
    tmed_commit c2 = cm.c;
    tmed_valset v2 = vs.c;
    tmed_median_request r2{&c2, &v2};
    switch (field) {
      case 0: c2.flags = nullptr; break;
      case 1: c2.addresses = nullptr; break;
      case 2: c2.ts_seconds = nullptr; break;
      case 3: c2.ts_nanos = nullptr; break;
      case 4: v2.addresses = nullptr; break;
      case 5: v2.powers = nullptr; break;
      case 6: r2.commit = nullptr; break;
      case 7: r2.vals = nullptr; break;
    }
    CHECK(median_times_host(&r2, 1, &o) == TMED_EINVAL);
  }
  tmed_commit c0 = cm.c;  // an empty commit and an empty set need no arrays
  tmed_valset v0 = vs.c;
  c0.n_sigs = 0;
  c0.flags = c0.addresses = nullptr;
  c0.ts_seconds = nullptr;
  c0.ts_nanos = nullptr;
  c0.address_lens = nullptr;
  v0.n = 0;
  v0.addresses = nullptr;
  v0.powers = nullptr;
  tmed_median_request r0{&c0, &vs.c}, r1{&cm.c, &v0};
  CHECK(median_times_host(&r0, 1, &o) == TMED_OK && o.code == TMED_MEDIAN_ZERO_TIME && o.seconds == kZeroTimeSeconds);
  CHECK(median_times_host(&r1, 1, &o) == TMED_OK && o.code == TMED_MEDIAN_ZERO_TIME && o.entered == 0);
  cm.c.address_lens = nullptr;  // NULL = all 20
  CHECK(median_times_host(&r, 1, &o) == TMED_OK && o.code == TMED_MEDIAN_OK);
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 2) return 64;
  int rc = run_file(argv[1]);
  if (rc) return rc;
  rc = self_checks();
  if (rc) return rc;
  printf("select-ok\n");
  return 0;
}
