// merkle_path.h — path arithmetic of the reference's Merkle proofs, shared by the host's aunt_off
// sizing, merkle_aunts_kernel, merkle_verify_kernel (merkle.hip) and a host-compiled test
// (tests/native/proofpath_host.cpp).  No hashing here.
//
// Reference: crypto/merkle/tree.go:103-117 getSplitPoint; crypto/merkle/proof.go:151-181
// computeHashFromAunts (top-down over (index, total), one aunt consumed per step, the LAST aunt at
// the root); :197-212 FlattenAunts (a leaf's aunts bottom-up); :216-237 trailsFromByteSlices.
#pragma once
#include <stdint.h>

#include "fe25519.h"  // TMED_HD

namespace tmed {

// getSplitPoint: the largest power of two strictly less than n (n >= 2), in 64 bits.
TMED_HD uint64_t merkle_split_point(uint64_t n) {
  const uint64_t k = 1ull << (63 - __builtin_clzll(n));
  return k == n ? k >> 1 : k;
}

// Aunts of the leaf at position p of an n-leaf tree, counted on the level-wise shape the kernels
// build (adjacent nodes paired, an odd last node promoted): at a level of c nodes the node has a
// sibling iff p ^ 1 < c.  Equal to the depth of leaf p in the split-point recursion.  n <= 1: 0.
TMED_HD uint32_t merkle_aunt_count(uint64_t p, uint64_t n) {
  uint32_t d = 0;
  for (uint64_t c = n; c > 1; c = (c + 1) >> 1) {
    if ((p ^ 1) < c) d++;
    p >>= 1;
  }
  return d;
}

// The walk of computeHashFromAunts over (index, total) without the hashes: false where it returns
// nil whatever the aunts are (index < 0, total <= 0, index >= total).  Else *d = the number of aunts
// it consumes (it returns nil for any other count; at most 63) and bit k of *mask tells on which
// side aunt k (bottom-up, Proof.Aunts order) stands: 1 = the aunt is the LEFT input of innerHash
// (the path went right), 0 = the aunt is the right input.
TMED_HD bool merkle_path(int64_t index, int64_t total, uint32_t *d, uint64_t *mask) {
  if (index < 0 || total <= 0 || index >= total) return false;
  uint64_t i = (uint64_t)index, n = (uint64_t)total, m = 0;
  uint32_t depth = 0;
  while (n > 1) {
    const uint64_t k = merkle_split_point(n);
    m <<= 1;
    if (i < k) {
      n = k;
    } else {
      m |= 1;
      i -= k;
      n -= k;
    }
    depth++;
  }
  *d = depth;
  *mask = m;
  return true;
}

}  // namespace tmed
