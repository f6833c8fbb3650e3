// proofpath_host.cpp — TEST-ONLY host build of the Merkle proofs' path arithmetic and of the level
// plan: the exact sources the host sizing, the tree builder and the device kernels compile
// (csrc/merkle_path.h, csrc/merkle_levels.h), run on the CPU so the suite can sweep them without a
// GPU.  tests/test_proofs_host.py compiles this file itself:
//   g++ -O2 -shared -fPIC -I tendermint-fork_amd/csrc proofpath_host.cpp
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "merkle_levels.h"
#include "merkle_path.h"

extern "C" {

uint64_t pp_split_point(uint64_t n) { return tmed::merkle_split_point(n); }

// aunt counts of every leaf of an n-leaf tree (what sizes aunt_off and bounds merkle_aunts_kernel)
void pp_aunt_counts(uint64_t n, uint32_t *out) {
  for (uint64_t p = 0; p < n; p++) out[p] = tmed::merkle_aunt_count(p, n);
}

// merkle_verify_kernel's walk: 1 with (*d, *mask), or 0 where computeHashFromAunts returns nil
int pp_path(int64_t index, int64_t total, uint32_t *d, uint64_t *mask) {
  return tmed::merkle_path(index, total, d, mask) ? 1 : 0;
}

// The level plan merkle.hip builds and uploads for trees of counts[0 .. n_trees) leaves
// (csrc/merkle_levels.h): returns nlevels, *nodes = the total node count, and the first
// min(nlevels, cap_levels) entries of lvl_off and rows (n_trees + 1 entries each) of tab.
uint32_t pp_level_plan(const uint32_t *counts, size_t n_trees, uint32_t cap_levels, uint64_t *lvl_off, uint32_t *tab,
                       uint64_t *nodes) {
  const tmed::MerkleLevels p(std::vector<uint32_t>(counts, counts + n_trees));
  *nodes = p.nodes;
  for (size_t l = 0; l < p.nlevels && l < cap_levels; l++) {
    lvl_off[l] = p.lvl_off[l];
    for (size_t t = 0; t <= n_trees; t++) tab[l * (n_trees + 1) + t] = p.level(l)[t];
  }
  return (uint32_t)p.nlevels;
}

}  // extern "C"
