// evidence_free.h — one DuplicateVoteEvidence: the checks of VerifyDuplicateVote in front of the two
// signatures (evidence/verify.go:162-209) and DuplicateVoteEvidence.Bytes() (types/evidence.go:90-98).
//
// Host and device compile this same source, over vote_free.h (the staged vote, VoteSignBytes) and
// vote_wire.h (the put_* writers): evidence_prepare_kernel and evidence_hash_kernel (evidence.hip) run
// it one lane per evidence, tmed_verify_duplicate_votes_host / tmed_evidence_bytes (evidence_host.h)
// and tests/native/evidence_host.cpp run it lane by lane on the CPU.
//
// Bytes() is the generated marshaller's output (fields ascending, gogoproto StdTime as in vote_wire.h):
//   DuplicateVoteEvidence (proto/tendermint/types/evidence.pb.go:449-497):
//     0a len VoteA | 12 len VoteB | 18 uvarint(total_voting_power) if != 0
//     | 20 uvarint(validator_power) if != 0 | 2a len ts ALWAYS
//   Vote (proto/tendermint/types/types.pb.go:1431-1489):
//     08 uvarint(uint64(int64(type))) if != 0 | 10 uvarint(uint64(height)) if != 0
//     | 18 uvarint(uint64(int64(round))) if != 0
//     | 22 len BlockID ALWAYS { 0a len hash if len > 0 | 12 len PartSetHeader ALWAYS
//                               { 08 uvarint(total) if != 0 | 12 len hash if len > 0 } }  (:1153-1171, :1233-1256)
//     | 2a len ts ALWAYS | 32 len addr if len > 0 | 38 uvarint(uint64(int64(index))) if != 0
//     | 42 len sig if len > 0
// A negative int32 or int64 takes ten bytes; the zero Vote's BlockID field is 22 02 12 00.
// DERIVED, NOT REFERENCE-PINNED: the reference holds no known answer for these bytes and no size bound
// either (types/evidence_test.go only round-trips), so the rule above stands on the reading of the two
// generated marshallers alone, as the CommitSig rule of tmed_commit_hashes does on its one.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "vote_free.h"

namespace tmed {

// Outcome codes of tmed_verify_duplicate_votes (include/tmed25519.h TMED_DUPVOTE_*; evidence_host.h
// asserts them equal).
constexpr uint8_t kEvOk = 0, kEvNotAValidator = 1, kEvHrsMismatch = 2, kEvAddressMismatch = 3, kEvSameBlockId = 4,
                  kEvAddressNotOfKey = 5, kEvValidatorPower = 6, kEvTotalPower = 7, kEvPanic = 8, kEvVoteASignature = 9,
                  kEvVoteBSignature = 10, kEvGoPath = 11;
constexpr uint32_t kEvNone = 0xffffffffu;  // GetByAddress found nobody

// The evidence's own fields beside its two staged votes (VoteRec 2i and 2i + 1 of the call; four
// 16-byte rows).  The lengths are the true ones: VoteRec clips its own at 255, which decides
// "malformed" but not whether two long hashes have the same length.
struct EvRec {
  int64_t total_power;  // DuplicateVoteEvidence.TotalVotingPower
  int64_t val_power;    // .ValidatorPower
  int64_t sec;          // .Timestamp
  int32_t nanos;
  uint32_t req;         // the evidence's request (EvStep) in the call
  uint32_t hash_len[2], psh_len[2], addr_len[2], sig_len[2];  // [0] VoteA, [1] VoteB
};
constexpr uint32_t kEvRecBytes = 64;
static_assert(sizeof(EvRec) == kEvRecBytes && kEvRecBytes % 16 == 0, "EvRec is four int4 rows");
static_assert(offsetof(VoteRec, addr) == 112, "the lookup kernel reads VoteA's address as dwords 28-32 of its record");

// One request's side: the set (its size, where its validators start in the call's packed address,
// power and key arrays, its total power) and the chain ID (device route: <= kVoteChainMax).
struct EvStep {
  int64_t total_power;  // vals->total_power
  uint64_t addr_base;
  uint32_t n_vals;
  uint32_t cid_len;
  uint8_t chain[kVoteChainMax + 6];
};
static_assert(sizeof(EvStep) == 80, "EvStep layout");

// ---- the lookup ------------------------------------------------------------------------------
// bytes.Equal of two 20-byte addresses held as five dwords (types/validator_set.go:270-278).
TMED_HD bool ev_addr_match(const uint32_t want[5], const uint32_t *cand) {
  uint32_t diff = 0;
#pragma unroll
  for (int k = 0; k < 5; k++) diff |= want[k] ^ cand[k];
  return diff == 0;
}

// ---- the checks ------------------------------------------------------------------------------
// bytes.Equal of a carried pair (at most `cap` bytes are staged; an empty slice equals a nil one):
// 0 differ, 1 equal, 2 the structs do not say (the same length above cap on both sides).
TMED_HD uint32_t ev_bytes_equal(const uint8_t *a, uint32_t la, const uint8_t *b, uint32_t lb, uint32_t cap) {
  if (la != lb) return 0;
  if (la > cap) return 2;
  uint32_t diff = 0;
  for (uint32_t k = 0; k < la; k++) diff |= (uint32_t)(a[k] ^ b[k]);
  return diff ? 0 : 1;
}
// BlockID.Equals (types/block.go:1170-1173 over types/part_set.go:111-113): false as soon as one of
// the three comparisons is false, else unknown if one of them is, else true.
TMED_HD uint32_t ev_block_ids_equal(const VoteRec &a, const VoteRec &b, const EvRec &e) {
  const uint32_t h = ev_bytes_equal(a.hash, e.hash_len[0], b.hash, e.hash_len[1], 32);
  const uint32_t p = ev_bytes_equal(a.psh, e.psh_len[0], b.psh, e.psh_len[1], 32);
  if (h == 0 || p == 0 || a.psh_total != b.psh_total) return 0;
  return (h == 2 || p == 2) ? 2 : 1;
}

// The checks in front of the signatures, in the reference's order; 0 = the signatures decide.
//   1 GetByAddress(VoteA.ValidatorAddress) finds nobody          evidence/verify.go:163-166
//   2 height, round or type differ between the votes             :170-176
//   3 !bytes.Equal(VoteA.ValidatorAddress, VoteB.ValidatorAddress) :179-184
//   4 VoteA.BlockID.Equals(VoteB.BlockID)                        :187-192 (kEvGoPath where unknown)
//   5 !bytes.Equal(pubKey.Address(), VoteA.ValidatorAddress)     :195-199
//   6 val.VotingPower != e.ValidatorPower                        :202-205
//   7 valSet.TotalVotingPower() != e.TotalVotingPower            :206-209
// found: the first validator of the set with VoteA's address (kEvNone: nobody; a found validator means
// VoteA's address has 20 bytes); found_power: its power; key(w): loads the eight words of its key
// (called only when checks 1-4 passed).
template <class KeyFn>
TMED_HD uint8_t ev_prechecks(const VoteRec &a, const VoteRec &b, const EvRec &e, const EvStep &s, uint32_t found,
                             int64_t found_power, KeyFn &&key) {
  if (found == kEvNone) return kEvNotAValidator;
  if (a.height != b.height || a.round != b.round || a.type != b.type) return kEvHrsMismatch;
  if (ev_bytes_equal(a.addr, 20, b.addr, e.addr_len[1], 20) != 1) return kEvAddressMismatch;
  const uint32_t same = ev_block_ids_equal(a, b, e);
  if (same == 1) return kEvSameBlockId;
  if (same == 2) return kEvGoPath;
  uint32_t pubw[8];
  key(pubw);
  if (!vote_address_of_key(a, pubw)) return kEvAddressNotOfKey;
  if (found_power != e.val_power) return kEvValidatorPower;
  if (s.total_power != e.total_power) return kEvTotalPower;
  return 0;
}

// What VoteSignBytes does with one vote: 0 = it returns the bytes vote_free_write writes.
TMED_HD uint8_t ev_vote_state(const VoteRec &r) {
  if (vote_bid_malformed(r)) return kEvPanic;
  if (!timestamp_encodable(r.sec, r.nanos)) return kEvGoPath;
  return 0;
}

// The call's outcome from the pre-code, the votes' states and the two validity bits, in the order
// the reference computes them (:211-219): VoteA's sign-bytes, VoteA's signature, VoteB's, VoteB's.
TMED_HD uint8_t ev_outcome(uint8_t pre, uint8_t state_a, bool valid_a, uint8_t state_b, bool valid_b) {
  if (pre) return pre;
  if (state_a) return state_a;
  if (!valid_a) return kEvVoteASignature;
  if (state_b) return state_b;
  if (!valid_b) return kEvVoteBSignature;
  return kEvOk;
}

// ---- Bytes() ---------------------------------------------------------------------------------
TMED_HD uint32_t pb_varint_field_len(uint64_t v) { return v ? 1 + uvarint_len(v) : 0; }
TMED_HD uint32_t pb_bytes_field_len(uint32_t n) { return n ? 1 + uvarint_len(n) + n : 0; }
TMED_HD uint32_t put_varint_field(uint8_t *o, uint32_t p, uint8_t tag, uint64_t v) {
  if (!v) return p;
  o[p++] = tag;
  return put_uvarint(o, p, v);
}
TMED_HD uint32_t put_bytes_field(uint8_t *o, uint32_t p, uint8_t tag, const uint8_t *b, uint32_t n) {
  if (!n) return p;
  o[p++] = tag;
  p = put_uvarint(o, p, n);
  return put_bytes(o, p, b, n);
}

// The longest Vote: type, height and round 1 + 10 each; BlockID 2 + {hash 2 + 32, part-set header
// 2 + {total 1 + 5, hash 2 + 32}}; timestamp 24; address 2 + 20; index 1 + 10; signature 2 + 64.
constexpr uint32_t kEvVoteBodyMax = 11 + 11 + 11 + kBlockIdFieldMax + kTimestampFieldMax + 22 + 11 + 66;
// The longest evidence: two Votes behind a tag and a two-byte length, two powers 1 + 10 each, the timestamp.
constexpr uint32_t kEvBytesMax = 2 * (1 + 2 + kEvVoteBodyMax) + 11 + 11 + kTimestampFieldMax;
static_assert(kEvVoteBodyMax == 234 && kEvVoteBodyMax >= 128 && kEvVoteBodyMax < (1u << 14),
              "the longest Vote is 234 bytes behind a two-byte length");
static_assert(kEvBytesMax == 520, "the longest DuplicateVoteEvidence is 520 bytes");

// What the struct can reproduce: a hash of at most 32 bytes, an address of at most 20 and a signature
// of at most 64 (longer ones are not carried), and three timestamps StdTimeMarshal accepts (Bytes()
// panics otherwise).
TMED_HD bool evidence_encodable(const VoteRec &a, const VoteRec &b, const EvRec &e) {
  bool ok = timestamp_encodable(e.sec, e.nanos) && timestamp_encodable(a.sec, a.nanos) && timestamp_encodable(b.sec, b.nanos);
  for (int k = 0; k < 2; k++) ok = ok && e.hash_len[k] <= 32 && e.psh_len[k] <= 32 && e.addr_len[k] <= 20 && e.sig_len[k] <= 64;
  return ok;
}

// Vote k (0: VoteA, 1: VoteB) of an encodable evidence.
TMED_HD uint32_t ev_psh_body(const VoteRec &r, const EvRec &e, int k) {
  return pb_varint_field_len(r.psh_total) + pb_bytes_field_len(e.psh_len[k]);
}
TMED_HD uint32_t ev_vote_body(const VoteRec &r, const EvRec &e, int k) {
  return pb_varint_field_len((uint64_t)(int64_t)r.type) + pb_varint_field_len((uint64_t)r.height) +
         pb_varint_field_len((uint64_t)(int64_t)r.round) + 2 + pb_bytes_field_len(e.hash_len[k]) + 2 + ev_psh_body(r, e, k) +
         timestamp_field_len(r.sec, r.nanos) + pb_bytes_field_len(e.addr_len[k]) +
         pb_varint_field_len((uint64_t)(int64_t)r.val_index) + pb_bytes_field_len(e.sig_len[k]);
}
TMED_HD uint32_t put_ev_vote(uint8_t *o, uint32_t p, const VoteRec &r, const EvRec &e, int k, const uint8_t *sig) {
  p = put_varint_field(o, p, 0x08, (uint64_t)(int64_t)r.type);
  p = put_varint_field(o, p, 0x10, (uint64_t)r.height);
  p = put_varint_field(o, p, 0x18, (uint64_t)(int64_t)r.round);
  const uint32_t psh = ev_psh_body(r, e, k);
  o[p++] = 0x22;
  o[p++] = (uint8_t)(pb_bytes_field_len(e.hash_len[k]) + 2 + psh);
  p = put_bytes_field(o, p, 0x0a, r.hash, e.hash_len[k]);
  o[p++] = 0x12;
  o[p++] = (uint8_t)psh;
  p = put_varint_field(o, p, 0x08, r.psh_total);
  p = put_bytes_field(o, p, 0x12, r.psh, e.psh_len[k]);
  p = put_timestamp_field(o, p, r.sec, r.nanos);
  p = put_bytes_field(o, p, 0x32, r.addr, e.addr_len[k]);
  p = put_varint_field(o, p, 0x38, (uint64_t)(int64_t)r.val_index);
  return put_bytes_field(o, p, 0x42, sig, e.sig_len[k]);
}

// Bytes() of an encodable evidence: its length, and the bytes into o (sig_a / sig_b: the votes'
// signatures); returns the length.
TMED_HD uint32_t evidence_size(const VoteRec &a, const VoteRec &b, const EvRec &e) {
  const uint32_t la = ev_vote_body(a, e, 0), lb = ev_vote_body(b, e, 1);
  return 1 + uvarint_len(la) + la + 1 + uvarint_len(lb) + lb + pb_varint_field_len((uint64_t)e.total_power) +
         pb_varint_field_len((uint64_t)e.val_power) + timestamp_field_len(e.sec, e.nanos);
}
TMED_HD uint32_t evidence_write(const VoteRec &a, const VoteRec &b, const EvRec &e, const uint8_t *sig_a,
                                const uint8_t *sig_b, uint8_t *o) {
  uint32_t p = 0;
  o[p++] = 0x0a;
  p = put_uvarint(o, p, ev_vote_body(a, e, 0));
  p = put_ev_vote(o, p, a, e, 0, sig_a);
  o[p++] = 0x12;
  p = put_uvarint(o, p, ev_vote_body(b, e, 1));
  p = put_ev_vote(o, p, b, e, 1, sig_b);
  p = put_varint_field(o, p, 0x18, (uint64_t)e.total_power);
  p = put_varint_field(o, p, 0x20, (uint64_t)e.val_power);
  return put_timestamp_field(o, p, e.sec, e.nanos);
}

// ---- hashing the bytes where they were written ---------------------------------------------------
// A lane's slot: kEvBytesMax bytes rounded up to dwords, plus one so that the stride (131 dwords) is
// odd: lane l's slot then starts at bank 131 l mod 32 = 3 l mod 32, so the 32 lanes of a half-wave
// (the group LDS writes conflict in) sit on 32 different banks, where a stride of 2^k dwords (k >= 5)
// would put every lane on the same one.
constexpr uint32_t kEvSlotDw = (kEvBytesMax + 3) / 4 + 1;
static_assert(kEvSlotDw == 131 && (kEvSlotDw & 1) == 1, "an odd dword stride spreads the lanes' slots over the banks");

// SHA-256(M) (npre = 0: tmhash.Sum) or SHA-256(0x00 || M) (npre = 1: leafHash, crypto/merkle/hash.go:
// 19-22) of the len bytes at the start of the slot dw, whose bytes past len are zero.  Up to nine
// blocks, so a loop.  The stream word at position pos holds M[pos - npre .. pos - npre + 4): with the
// dword before the slot read as zero the leaf's 0x00 prefix needs no case of its own.
TMED_HD void sha256_of_slot(uint32_t st[8], int npre, const uint32_t *dw, uint32_t len) {
  const uint32_t total = (uint32_t)npre + len;
  const uint32_t nblocks = (total + 9 + 63) >> 6;
  sha256_init(st);
#pragma unroll 1
  for (uint32_t b = 0; b < nblocks; b++) {
    uint32_t w[16];
#pragma unroll
    for (int t = 0; t < 16; t++) {
      const uint32_t q = b * 16 + (uint32_t)t;  // the slot dword the word starts in
      const uint32_t cur = q < kEvSlotDw ? bswap32(dw[q]) : 0u;
      uint32_t v = cur;
      if (npre) {
        const uint32_t prev = (q >= 1 && q - 1 < kEvSlotDw) ? bswap32(dw[q - 1]) : 0u;
        v = (prev << 24) | (cur >> 8);
      }
      const int32_t nv = (int32_t)total - (int32_t)(4 * q);  // stream bytes in this word
      if (nv >= 0 && nv < 4) v |= 0x80u << (24 - 8 * nv);
      if (b == nblocks - 1 && t == 14) v = 0;
      if (b == nblocks - 1 && t == 15) v = total << 3;
      w[t] = v;
    }
    sha256_compress(st, w);
  }
}

}  // namespace tmed
