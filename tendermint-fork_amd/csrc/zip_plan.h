// zip_plan.h — host-only: which groups of a ZIP-215 chunk get a batch equation and which are decided
// signature by signature (the bisection bookkeeping of zip215_verify_device, csrc/zip215.hip).  No
// device code and no HIP types, so tests/native/zip_plan_host.cpp builds it stand-alone.
//
// Groups [lo, lo + cnt) of a chunk of N signatures, level by level, starting from the whole chunk:
// every group of a level runs one equation.  A failing group is split in halves (h = cnt / 2 and
// cnt - h) while the failures look sparse — at most half of the level's groups fail; a level of one
// group is never dense — and both halves stay >= min_group, i.e. cnt >= 2 min_group; every other
// failing group is decided signature by signature.  Groups whose equation holds are finished: every
// signature of them keeps the verdict the prep wrote.
#pragma once
#include <stdint.h>

#include <utility>
#include <vector>

namespace tmed {

typedef std::pair<uint32_t, uint32_t> ZipGroup;  // (lo, cnt)

// eq(level, lo, cnt, &ok) answers "does the equation over [lo, lo + cnt) hold?" and returns 0, or an
// error code that ends the plan and is returned.  single: the groups to decide singly, in the order
// the levels found them; equations: the calls of eq made.
template <class Eq>
int zip_plan_run(uint32_t N, uint32_t min_group, Eq &&eq, std::vector<ZipGroup> &single, uint32_t &equations) {
  single.clear();
  equations = 0;
  std::vector<ZipGroup> level{{0u, N}};
  for (uint32_t depth = 0; !level.empty(); depth++) {
    std::vector<ZipGroup> failed;
    for (auto &g : level) {
      bool ok = false;
      const int rc = eq(depth, g.first, g.second, &ok);
      if (rc != 0) return rc;
      equations++;
      if (!ok) failed.push_back(g);
    }
    const bool dense = level.size() >= 2 && failed.size() * 2 > level.size();
    std::vector<ZipGroup> next;
    for (auto &g : failed) {
      if (!dense && g.second >= 2 * (uint64_t)min_group) {
        const uint32_t h = g.second / 2;
        next.push_back({g.first, h});
        next.push_back({g.first + h, g.second - h});
      } else {
        single.push_back(g);
      }
    }
    level.swap(next);
  }
  return 0;
}

}  // namespace tmed
