// signbytes.h — per-commit CanonicalVote encoder (vote_wire.h has the layout + citations).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/tmed25519.h"
#include "vote_wire.h"

namespace tmed {

// f1: on-device CanonicalVote assembly (kernels.h launch_assemble_votes): templates are
// kVoteTmplBytes records, message i is written at i * kVoteSlot.
constexpr uint32_t kVoteTmplBytes = 256;
constexpr uint32_t kVoteSlot = 256;

// Everything but the per-vote flag/timestamp is encoded once per commit: the three ranges of
// vote_wire.h's vote_splice.
struct VoteEncoder {
  uint8_t pre[kVoteHeadMax];  // 08 02 [11 height] [19 round]
  uint32_t pre_len = 0;
  uint8_t bid[kBlockIdFieldMax];  // the commit BlockID's field; empty for the zero BlockID and under !bid_ok
  uint32_t bid_len = 0;
  bool bid_ok = true;  // block/part-set hashes pass ValidateHash (else only Absent/Nil votes encode)
  std::vector<uint8_t> cid;  // the chain-ID field

  int init(const tmed_vote_template *t);
  // BlockIDFlagCommit -> the commit BlockID; Absent/Nil -> the zero BlockID (CommitSig.BlockID)
  uint32_t bid_len_of(int flag) const { return flag == 2 ? bid_len : 0; }
  size_t size(int flag, int64_t sec, int32_t nanos) const {
    return vote_msg_len(vote_body_len(pre_len, bid_len_of(flag), timestamp_field_len(sec, nanos), (uint32_t)cid.size()));
  }
  uint8_t *write(uint8_t *out, int flag, int64_t sec, int32_t nanos) const {
    return out + vote_splice(out, pre, pre_len, bid, bid_len_of(flag), sec, nanos, cid.data(), (uint32_t)cid.size());
  }
  // Device template record for the on-device assembler (votes_dev.h):
  // [pre_len, bid_len, cid_len, 0] + pre + BlockID field + chain-id field.
  // Returns false if it does not fit in `cap` bytes, or if a vote's message could exceed `slot`
  // bytes (the device writes vote i at i * slot): long chain IDs take the host path.
  bool device_template(uint8_t *out, size_t cap, size_t slot) const;
};

// Vote (flag, sec, nanos) of the commit whose device_template record is rec, into o (at most the
// record's `slot` bytes); returns its length.  What the device assemblers run on the staged record.
TMED_HD uint32_t vote_from_template(uint8_t *__restrict__ o, const uint8_t *rec, int flag, int64_t sec, int32_t nanos) {
  const uint8_t *pre = rec + 4, *bid = pre + rec[0], *cid = bid + rec[1];
  return vote_splice(o, pre, rec[0], bid, flag == 2 ? rec[1] : 0, sec, nanos, cid, rec[2]);
}

}  // namespace tmed
