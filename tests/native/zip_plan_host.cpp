// zip_plan_host.cpp — TEST-ONLY stand-alone host program: the bisection plan of the ZIP-215 batch
// mode (csrc/zip_plan.h, the bookkeeping of zip215_verify_device) driven by a callback that knows
// which signatures fail.  tests/test_zip_plan_host.py builds it with -fsanitize=address,undefined
// and runs it as a plain executable:
//   g++ -std=c++17 -fsanitize=address,undefined -I tendermint-fork_amd/csrc zip_plan_host.cpp
//
//   zip_plan_host trace <file>     cases from a text file, one per line: N min_group k f_1 .. f_k
//       per case on stdout:  case <N> <equations> <groups decided singly>
//                            e <level> <lo> <cnt> <ok>      one per equation, in call order
//                            s <lo> <cnt>                   one per singly decided group
//   zip_plan_host all <max_n> <max_k> <min_group>
//       every N in 1..max_n with every set of at most max_k failing indices, sizes ascending, sets in
//       lexicographic order; per case one line:  <equations> <lo>:<cnt> ...  (the groups decided singly)
// Both modes check every case's trace (check_trace below) and exit 1 at the first violation.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "zip_plan.h"

struct Eq {
  uint32_t level, lo, cnt;
  bool ok;
};

struct Trace {
  std::vector<Eq> eqs;
  std::vector<tmed::ZipGroup> single;
  uint32_t equations = 0;
};

static bool holds(const std::vector<uint32_t> &fails, uint32_t lo, uint32_t cnt) {
  for (uint32_t f : fails)
    if (f >= lo && f - lo < cnt) return false;
  return true;
}

static int run_plan(uint32_t N, uint32_t min_group, const std::vector<uint32_t> &fails, Trace &t) {
  t.eqs.clear();
  return tmed::zip_plan_run(
      N, min_group,
      [&](uint32_t level, uint32_t lo, uint32_t cnt, bool *ok) {
        *ok = holds(fails, lo, cnt);
        t.eqs.push_back(Eq{level, lo, cnt, *ok});
        return 0;
      },
      t.single, t.equations);
}

#define CHECK(c)                                                                      \
  do {                                                                                \
    if (!(c)) {                                                                       \
      fprintf(stderr, "zip_plan_host.cpp:%d: %s (N = %u, %zu failing)\n", __LINE__, #c, N, fails.size()); \
      return false;                                                                   \
    }                                                                                 \
  } while (0)

static bool check_trace(uint32_t N, uint32_t min_group, const std::vector<uint32_t> &fails, const Trace &t) {
  CHECK(t.equations == t.eqs.size() && !t.eqs.empty());
  CHECK(t.eqs[0].level == 0 && t.eqs[0].lo == 0 && t.eqs[0].cnt == N);
  if (fails.empty()) CHECK(t.equations == 1 && t.single.empty());
  std::vector<int> cover(N, 0);
  uint32_t level = 0;
  size_t i = 0;
  while (i < t.eqs.size()) {
    size_t j = i;
    std::fill(cover.begin(), cover.end(), 0);
    while (j < t.eqs.size() && t.eqs[j].level == level) {  // one level: disjoint sub-ranges of the chunk
      const Eq &e = t.eqs[j];
      CHECK(e.cnt >= 1 && e.lo <= N && e.cnt <= N - e.lo);
      CHECK(e.ok == holds(fails, e.lo, e.cnt));
      for (uint32_t x = e.lo; x < e.lo + e.cnt; x++) CHECK(cover[x]++ == 0);
      j++;
    }
    CHECK(j > i);
    if (level > 0) {  // consecutive pairs are the halves of a failed group of the level above
      CHECK((j - i) % 2 == 0);
      for (size_t p = i; p < j; p += 2) {
        const Eq &a = t.eqs[p], &b = t.eqs[p + 1];
        CHECK(a.lo + a.cnt == b.lo && a.cnt == (a.cnt + b.cnt) / 2 && a.cnt >= min_group && b.cnt >= min_group);
        bool found = false;
        for (const Eq &q : t.eqs)
          found |= q.level + 1 == level && !q.ok && q.lo == a.lo && q.cnt == a.cnt + b.cnt;
        CHECK(found);
      }
    }
    i = j;
    level++;
  }
  // every failed equation was either split (its first half starts a pair of the next level) or decided singly
  for (const Eq &e : t.eqs) {
    if (e.ok) continue;
    int split = 0, single = 0;
    for (const Eq &q : t.eqs) split += q.level == e.level + 1 && q.lo == e.lo && q.cnt == e.cnt / 2;
    for (auto &g : t.single) single += g.first == e.lo && g.second == e.cnt;
    CHECK(split + single == 1);
  }
  std::fill(cover.begin(), cover.end(), 0);
  for (auto &g : t.single) {  // singly decided groups: failed equations, no index twice
    bool found = false;
    for (const Eq &e : t.eqs) found |= !e.ok && e.lo == g.first && e.cnt == g.second;
    CHECK(found);
    for (uint32_t x = g.first; x < g.first + g.second; x++) CHECK(cover[x]++ == 0);
  }
  for (uint32_t f : fails) CHECK(cover[f] == 1);
  return true;
}

static int mode_trace(const char *path) {
  std::ifstream in(path);
  if (!in) return 2;
  std::string line;
  Trace t;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    uint32_t N, min_group, k;
    if (!(ls >> N >> min_group >> k)) continue;
    std::vector<uint32_t> fails(k);
    for (auto &f : fails)
      if (!(ls >> f) || f >= N) return 2;
    if (run_plan(N, min_group, fails, t) != 0 || !check_trace(N, min_group, fails, t)) return 1;
    printf("case %u %u %zu\n", N, t.equations, t.single.size());
    for (const Eq &e : t.eqs) printf("e %u %u %u %d\n", e.level, e.lo, e.cnt, e.ok ? 1 : 0);
    for (auto &g : t.single) printf("s %u %u\n", g.first, g.second);
  }
  return 0;
}

static int mode_all(uint32_t max_n, uint32_t max_k, uint32_t min_group) {
  Trace t;
  for (uint32_t N = 1; N <= max_n; N++)
    for (uint32_t k = 0; k <= max_k && k <= N; k++) {
      std::vector<uint32_t> fails(k);
      for (uint32_t q = 0; q < k; q++) fails[q] = q;
      for (;;) {
        if (run_plan(N, min_group, fails, t) != 0 || !check_trace(N, min_group, fails, t)) return 1;
        printf("%u", t.equations);
        for (auto &g : t.single) printf(" %u:%u", g.first, g.second);
        putchar('\n');
        int q = (int)k - 1;  // the next set in lexicographic order
        while (q >= 0 && fails[q] == N - k + (uint32_t)q) q--;
        if (q < 0) break;
        fails[q]++;
        for (uint32_t r = (uint32_t)q + 1; r < k; r++) fails[r] = fails[r - 1] + 1;
      }
    }
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && std::string(argv[1]) == "trace") return mode_trace(argv[2]);
  if (argc == 5 && std::string(argv[1]) == "all")
    return mode_all((uint32_t)atoi(argv[2]), (uint32_t)atoi(argv[3]), (uint32_t)atoi(argv[4]));
  fprintf(stderr, "usage: zip_plan_host trace <file> | all <max_n> <max_k> <min_group>\n");
  return 2;
}
