// vote_free.h — one free-standing vote: VoteSignBytes(chainID, vote) from the vote's own fields (no
// per-commit template) and the checks VoteSet.addVote and Vote.Verify run in front of the signature.
//
// Host and device compile this same source: vote_prepare_kernel (votes.hip) runs it one lane per
// vote, tmed_votes_sign_bytes / tmed_verify_votes_host (votes_host.h) and tests/native/votes_host.cpp
// run it lane by lane on the CPU.
//
// The bytes are vote_wire.h's, field for field: the head from the vote's type, height and round, the
// BlockID field from its hash, total and part-set hash, the timestamp, the chain ID.  A hash or
// part-set hash whose length is neither 0 nor 32 makes CanonicalizeBlockID panic (BlockIDFromProto ->
// ValidateBasic -> ValidateHash): vote_bid_malformed, nothing is encoded.
#pragma once
#include <stdint.h>
#include <string.h>

#include "sha256.h"
#include "signbytes.h"
#include "vote_wire.h"

namespace tmed {

// Outcome codes of tmed_verify_votes (include/tmed25519.h TMED_VOTE_*; votes_host.h asserts them equal).
constexpr uint8_t kVoteOk = 0, kVoteIndexNegative = 1, kVoteAddressEmpty = 2, kVoteUnexpectedStep = 3,
                  kVoteIndexNotInSet = 4, kVoteAddressNotInSet = 5, kVoteAddressNotOfKey = 6, kVotePanic = 7,
                  kVoteInvalidSignature = 8, kVoteGoPath = 9;
constexpr uint32_t kVoteFlagAddVote = 1;  // TMED_VOTES_ADDVOTE

// The longest message of a vote whose chain ID has at most kVoteChainMax bytes (MaxChainIDLen,
// types/genesis.go): every field at vote_wire.h's longest (head 29, BlockID 78, timestamp 24) and
// chain ID 2 + 50: a body of 183 bytes behind a two-byte length.  Such votes are assembled on the
// device, each into its kVoteSlot-byte slot; a request with a longer chain ID is assembled on the
// host by the same source (votes.hip), as VoteEncoder::device_template rules for commits.
constexpr uint32_t kVoteChainMax = 50;
constexpr uint32_t kVoteFreeFixedMax = kVoteHeadMax + kBlockIdFieldMax + kTimestampFieldMax;
constexpr uint32_t kVoteFreeBodyMax = kVoteFreeFixedMax + 2 + kVoteChainMax;
constexpr uint32_t kVoteFreeMsgMax = 2 + kVoteFreeBodyMax;
static_assert(kVoteChainMax < 128 && kVoteFreeBodyMax >= 128 && kVoteFreeBodyMax < (1u << 14),
              "one-byte chain-ID length, two-byte body length");
static_assert(kVoteFreeMsgMax == 185 && kVoteFreeMsgMax <= kVoteSlot, "the worst-case vote fits its slot");

// One staged vote (nine 16-byte rows).  hash_len / psh_len / addr_len hold min(length, 255): every
// length that matters (0, 20, 32) is exact, and a longer hash or address is malformed / a mismatch
// whatever its bytes are, so only the first 32 / 20 bytes are staged.
struct VoteRec {
  int64_t height;
  int64_t sec;
  int32_t type;
  int32_t round;
  int32_t nanos;
  int32_t val_index;
  uint32_t psh_total;
  uint8_t hash_len, psh_len, addr_len, sig_full;  // sig_full: len(Signature) == 64
  uint32_t key;  // keyed route: the validator's index in the key set
  uint32_t req;  // the vote's request (VoteStep) in the call
  uint8_t hash[32];
  uint8_t psh[32];
  uint8_t addr[20];
  uint8_t pad[12];
};
constexpr uint32_t kVoteRecBytes = 144;
static_assert(sizeof(VoteRec) == kVoteRecBytes && kVoteRecBytes % 16 == 0, "VoteRec is nine int4 rows");

// One request's side of the checks: the VoteSet's step (ADDVOTE), the set's size, where its
// addresses start in the call's packed address array, and the chain ID (device route: <= kVoteChainMax).
struct VoteStep {
  int64_t height;
  int32_t round;
  int32_t type;
  uint32_t flags;
  uint32_t cid_len;
  uint32_t n_vals;
  uint32_t pad;
  uint64_t addr_base;  // validators before this set's in the packed addresses (ADDVOTE)
  uint8_t chain[kVoteChainMax + 6];
};
static_assert(sizeof(VoteStep) == 96, "VoteStep layout");

TMED_HD bool vote_bid_malformed(const VoteRec &r) {
  return (r.hash_len != 0 && r.hash_len != 32) || (r.psh_len != 0 && r.psh_len != 32);
}

// The body and the length of the sign-bytes of a vote whose BlockID is not malformed.
TMED_HD uint32_t vote_free_body(const VoteRec &r, uint32_t cid_len) {
  return vote_body_len(vote_head_len(r.type, r.height, r.round), block_id_field_len(r.hash_len, r.psh_total, r.psh_len),
                       timestamp_field_len(r.sec, r.nanos), chain_id_field_len(cid_len));
}
TMED_HD uint32_t vote_free_size(const VoteRec &r, uint32_t cid_len) { return vote_msg_len(vote_free_body(r, cid_len)); }

// The vote's sign-bytes into o (vote_free_size bytes; the BlockID is not malformed); returns the length.
// vote_splice's message with the three ranges written in place instead of copied: a lane of
// vote_prepare_kernel has nowhere to stage them.
TMED_HD uint32_t vote_free_write(const VoteRec &r, const uint8_t *chain, uint32_t cid_len, uint8_t *o) {
  uint32_t p = put_uvarint(o, 0, vote_free_body(r, cid_len));
  p = put_vote_head(o, p, r.type, r.height, r.round);
  p = put_block_id_field(o, p, r.hash_len ? r.hash : nullptr, r.psh_total, r.psh_len ? r.psh : nullptr);
  p = put_timestamp_field(o, p, r.sec, r.nanos);
  return put_chain_id_field(o, p, chain, cid_len);
}

// PubKey.Address() = SHA-256(key)[:20] (crypto/ed25519/ed25519.go:136-141, crypto/tmhash
// SumTruncated) against the vote's 20-byte address: one sha256_compress.  pubw: the key's eight
// little-endian words.
TMED_HD bool vote_address_of_key(const VoteRec &r, const uint32_t pubw[8]) {
  uint32_t st[8], w[16];
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = bswap32(pubw[k]);
  w[8] = 0x80000000u;
#pragma unroll
  for (int k = 9; k < 15; k++) w[k] = 0;
  w[15] = 256;
  sha256_init(st);
  sha256_compress(st, w);
  uint32_t diff = 0;
#pragma unroll
  for (int k = 0; k < 5; k++) {
    const uint8_t *a = r.addr + 4 * k;
    diff |= st[k] ^ (((uint32_t)a[0] << 24) | ((uint32_t)a[1] << 16) | ((uint32_t)a[2] << 8) | a[3]);
  }
  return diff == 0;
}

// The checks in front of the signature, in the reference's order; 0 = the signature decides.
//   1 valIndex < 0                                             types/vote_set.go:165
//   2 len(valAddr) == 0                          (ADDVOTE)     :167
//   3 height / round / type differ from the step (ADDVOTE)     :172-178
//   4 GetByIndex(valIndex) finds nobody                        :181-186
//   5 !bytes.Equal(valAddr, lookupAddr)          (ADDVOTE)     :189-194
//     (the duplicate lookup of :197-202 sits here in the reference: it reads the VoteSet's state and
//     stays in Go)
//   6 !bytes.Equal(pubKey.Address(), vote.ValidatorAddress)    types/vote.go:148
//   7 CanonicalizeBlockID panics on a malformed hash           types/canonical.go:19-22
//   then the Timestamp's range (vote_wire.h timestamp_encodable: VoteSignBytes panics outside it,
//   types/vote.go:95-98, and a Go time.Time holds no such nanos): kVoteGoPath
// set_addr: the request's set addresses (n_vals x 20; read only under ADDVOTE); key(w): loads the
// eight words of the key at val_index (called only when checks 1-5 passed).
template <class KeyFn>
TMED_HD uint8_t vote_prechecks(const VoteRec &r, const VoteStep &s, const uint8_t *set_addr, KeyFn &&key) {
  const bool add = (s.flags & kVoteFlagAddVote) != 0;
  if (r.val_index < 0) return kVoteIndexNegative;
  if (add && r.addr_len == 0) return kVoteAddressEmpty;
  if (add && (r.height != s.height || r.round != s.round || r.type != s.type)) return kVoteUnexpectedStep;
  if ((uint32_t)r.val_index >= s.n_vals) return kVoteIndexNotInSet;
  if (add) {
    const uint8_t *a = set_addr + 20 * (size_t)r.val_index;
    uint32_t diff = r.addr_len ^ 20u;
    for (int k = 0; k < 20; k++) diff |= (uint32_t)(a[k] ^ r.addr[k]);
    if (diff) return kVoteAddressNotInSet;
  }
  if (r.addr_len != 20) return kVoteAddressNotOfKey;
  uint32_t pubw[8];
  key(pubw);
  if (!vote_address_of_key(r, pubw)) return kVoteAddressNotOfKey;
  if (vote_bid_malformed(r)) return kVotePanic;
  if (!timestamp_encodable(r.sec, r.nanos)) return kVoteGoPath;
  return 0;
}

}  // namespace tmed
