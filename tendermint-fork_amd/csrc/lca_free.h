// lca_free.h — one LightClientAttackEvidence: the rule of GetByzantineValidators
// (types/evidence.go:233-279) and of LightClientAttackEvidence.Hash() (:302-309), stated once.
//
// Host and device compile this same source: lca_lookup_kernel, lca_rank_kernel and lca_hash_kernel
// (lca.hip) run it on the device, tmed_byzantine_validators_host and
// tmed_verify_light_client_attacks_with (lca_host.h) and tests/native/lca_host.cpp on the CPU.
//
// The attack kind:
//   LUNATIC       ConflictingHeaderIsInvalid(trusted.Header) (:285-292): one of ValidatorsHash,
//                 NextValidatorsHash, ConsensusHash, AppHash, LastResultsHash differs under bytes.Equal
//                 (lengths count, nil equals empty);
//   EQUIVOCATION  otherwise, and the two commits' rounds are equal (:253);
//   AMNESIA       otherwise: no validators, a nil list.
// The candidates (the signatures whose address is looked up, in commit order):
//   LUNATIC       every ForBlock signature of the conflicting commit, looked up in common_vals; those
//                 that find nobody are dropped;
//   EQUIVOCATION  every i with conflicting sig i not absent and trusted sig i not absent, looked up in
//                 conflicting_vals; a non-absent conflicting sig at i >= the trusted commit's size is an
//                 index out of range (panic); so is, through the sort, a candidate that finds nobody in a
//                 list of two or more; a list of one that finds nobody is returned as one nil entry.
// The order: ValidatorsByVotingPower (types/validator_set.go:906-911): power descending as int64, then
// address ascending under bytes.Compare.  It is held as an ordering KEY of eight dwords compared most
// significant first as unsigned numbers:
//   [0] 0 found / 1 nobody (nobody orders behind every validator; the host then reads the found count)
//   [1..2] ~(power ^ 2^63), high dword first: ascending in it is descending in the signed power
//   [3..7] the address's five dwords BYTE-SWAPPED: an address sits in memory as bytes, a dword read on a
//          little-endian machine puts byte 0 in the LOW bits, and bytes.Compare is lexicographic on bytes,
//          so the dwords are compared big-endian
// and ties (one validator found by two signatures) by commit position, so that the ranks of a request's
// candidates are a permutation.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/tmed25519.h"
#include "evidence_free.h"  // ev_addr_match, kEvNone; over vote_wire.h (TMED_HD, uvarint_len) and sha256.h

namespace tmed {

constexpr uint8_t kFlagAbsent = 1, kFlagCommit = 2;  // BlockIDFlagAbsent, BlockIDFlagCommit (types/block.go:585-590)
constexpr uint32_t kLcaKeyDw = 8;

// ---- the attack kind (host: it reads the caller's structs) ---------------------------------------
inline bool lca_bytes_equal(const uint8_t *a, uint32_t na, const uint8_t *b, uint32_t nb) {  // bytes.Equal
  return na == nb && (na == 0 || memcmp(a, b, na) == 0);
}
// ConflictingHeaderIsInvalid: tmed_header::hashes[2..6] are ValidatorsHash, NextValidatorsHash,
// ConsensusHash, AppHash, LastResultsHash.
inline bool lca_header_invalid(const tmed_header &trusted, const tmed_header &conflicting) {
  for (int k = 2; k <= 6; k++)
    if (!lca_bytes_equal(trusted.hashes[k], trusted.hash_lens[k], conflicting.hashes[k], conflicting.hash_lens[k])) return true;
  return false;
}
inline int lca_kind(const tmed_lca_request &r) {
  if (lca_header_invalid(*r.trusted_header, *r.conflicting_header)) return TMED_LCA_LUNATIC;
  return r.trusted_commit->round == r.conflicting_commit->round ? TMED_LCA_EQUIVOCATION : TMED_LCA_AMNESIA;
}

// ---- the ordering key ----------------------------------------------------------------------------
TMED_HD uint32_t lca_bswap(uint32_t x) {
  return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24);
}
// addr: the found validator's address as five dwords as they lie in memory (read only when found).
TMED_HD void lca_key(bool found, int64_t power, const uint32_t *addr, uint32_t w[kLcaKeyDw]) {
#pragma unroll
  for (uint32_t k = 0; k < kLcaKeyDw; k++) w[k] = 0;
  w[0] = found ? 0u : 1u;
  if (!found) return;
  const uint64_t inv = ~((uint64_t)power ^ 0x8000000000000000ull);
  w[1] = (uint32_t)(inv >> 32);
  w[2] = (uint32_t)inv;
#pragma unroll
  for (int k = 0; k < 5; k++) w[3 + k] = lca_bswap(addr[k]);
}
// Does candidate a (key, commit position) order before candidate b?
TMED_HD bool lca_before(const uint32_t a[kLcaKeyDw], uint32_t pos_a, const uint32_t b[kLcaKeyDw], uint32_t pos_b) {
  bool lt = pos_a < pos_b;
#pragma unroll
  for (int k = (int)kLcaKeyDw - 1; k >= 0; k--) lt = a[k] < b[k] || (a[k] == b[k] && lt);
  return lt;
}

// ---- Hash() --------------------------------------------------------------------------------------
// tmhash.Sum(bz), bz = make([]byte, 32 + n): copy(bz[:31], ConflictingBlock.Hash()) (a nil hash copies
// nothing), bz[31] = 0, bz[32:] = the n bytes of binary.PutVarint(CommonHeight), the ZIGZAG varint
// (ux = uint64(x) << 1, complemented for x < 0; then 7 bits a byte, low first).  At most 42 bytes: one
// SHA-256 block.  hdr: the header hash as eight dwords as they lie in memory (read only when ok);
// st: the digest as eight big-endian word values.  Every index into w is a constant: no scratch.
TMED_HD void lca_evidence_hash(const uint32_t hdr[8], bool ok, int64_t common_height, uint32_t st[8]) {
  uint32_t w[16];
#pragma unroll
  for (int k = 0; k < 16; k++) w[k] = 0;
  if (ok) {
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = lca_bswap(hdr[k]);
    w[7] &= 0xffffff00u;  // only tmhash.Size - 1 bytes are copied
  }
  uint64_t ux = (uint64_t)common_height << 1;
  if (common_height < 0) ux = ~ux;
  const uint32_t n = uvarint_len(ux);
#pragma unroll
  for (uint32_t i = 0; i <= 10; i++) {  // the varint's bytes, then SHA-256's 0x80
    uint32_t b = 0;
    if (i < n) b = (uint32_t)((ux >> (7 * (i < 10 ? i : 9))) & 0x7f) | (i + 1 < n ? 0x80u : 0u);
    else if (i == n) b = 0x80u;
    w[8 + i / 4] |= b << (24 - 8 * (i % 4));
  }
  w[15] = (32 + n) * 8;
  sha256_init(st);
  sha256_compress(st, w);
}

}  // namespace tmed
