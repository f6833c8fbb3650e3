// merkle_levels.h — the level plan of one Merkle call: where every node of every level of every tree
// lies in the call's node buffer.  Host only (no HIP header): merkle.hip builds it once per call from
// the trees' leaf counts and uploads it before the first level launch, and a host-compiled test
// (tests/native/proofpath_host.cpp) walks it as merkle_level_kernel and merkle_aunts_kernel do.
//
// Level 0 holds the leaves, level l + 1 pairs the adjacent nodes of level l and promotes an odd last
// node (crypto/merkle/tree.go:57-101 HashFromByteSlicesIterative).  Every level lies tree-contiguous
// at nodes + lvl_off[l], tree t's nodes from tab[l * (T + 1) + t].  A tree that is down to one node
// carries it through the remaining levels, so the last level holds every root; an empty tree stays
// empty (0 -> 0).  A tree of n >= 1 leaves has at most 2 n - 1 + nlevels nodes over all levels and
// nlevels <= 33 below 2^32 leaves, so nodes <= 2 L + 32 T for L leaves in T trees.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace tmed {

struct MerkleLevels {
  size_t T = 0;                   // trees
  size_t nlevels = 0;             // >= 1
  uint64_t leaves = 0;            // of all trees; the tables hold only below 2^32
  uint64_t nodes = 0;             // of all levels
  std::vector<uint32_t> tab;      // nlevels x (T + 1) prefix tables
  std::vector<uint64_t> lvl_off;  // nlevels level starts, in nodes

  explicit MerkleLevels(const std::vector<uint32_t> &counts) : T(counts.size()) {
    std::vector<uint32_t> cnt(counts);
    for (const uint32_t n : counts) leaves += n;
    for (;;) {
      const size_t at = tab.size();
      tab.resize(at + T + 1);
      lvl_off.push_back(nodes);
      tab[at] = 0;
      bool more = false;
      for (size_t t = 0; t < T; t++) {
        tab[at + t + 1] = tab[at + t] + cnt[t];
        if (cnt[t] > 1) more = true;
        cnt[t] -= cnt[t] / 2;  // ceil(c / 2) without the carry: 0 -> 0, 1 -> 1
      }
      nodes += tab[at + T];
      if (!more) break;
    }
    nlevels = lvl_off.size();
  }
  const uint32_t *level(size_t l) const { return tab.data() + l * (T + 1); }
  uint32_t level_nodes(size_t l) const { return level(l)[T]; }
};

}  // namespace tmed
