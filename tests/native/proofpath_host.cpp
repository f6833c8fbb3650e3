// proofpath_host.cpp — TEST-ONLY host build of the Merkle proofs' path arithmetic: the exact source
// the host sizing and the device kernels compile (csrc/merkle_path.h), run on the CPU so the suite
// can sweep it without a GPU.  tests/test_proofs_host.py compiles this file itself:
//   g++ -O2 -shared -fPIC -I tendermint-fork_amd/csrc proofpath_host.cpp
#include <stddef.h>
#include <stdint.h>

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

}  // extern "C"
