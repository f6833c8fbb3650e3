// signbytes.hip — CanonicalVote sign-bytes for the commit seam (host C++).
//
// The votes of a commit, over the byte layout of vote_wire.h:
//   Commit.VoteSignBytes          types/block.go:807-810 (GetVote :784-796)
//   CommitSig.BlockID             types/block.go:652-665 (Commit -> commit BlockID; Absent/Nil -> zero)
// Only the timestamp (and the flag) differ between the votes of one commit, so the encoder writes
// the ranges in front of and behind the timestamp once per commit, and vote_splice puts each
// validator's timestamp between them, here and on the device (votes_dev.h).
#include <string.h>

#include "../../include/tmed25519.h"
#include "signbytes.h"

namespace tmed {

int VoteEncoder::init(const tmed_vote_template *t) {
  if (!t) return TMED_EINVAL;
  if (t->chain_id_len && !t->chain_id) return TMED_EINVAL;
  // ValidateHash: CanonicalizeBlockID panics on a malformed hash (types/canonical.go:18-22), which
  // only a Commit-flag vote reaches (Absent / Nil votes sign the zero BlockID): such a template
  // can still encode those, and write()/size() must never be asked for a Commit vote.
  bid_ok = (t->block_hash_len == 0 || t->block_hash_len == 32) && (t->psh_hash_len == 0 || t->psh_hash_len == 32);
  pre_len = put_vote_head(pre, 0, /*SignedMsgType Precommit (Commit.GetVote, types/block.go:787)*/ 2, t->height, t->round);
  bid_len = bid_ok ? put_block_id_field(bid, 0, t->block_hash_len ? t->block_hash : nullptr, t->psh_total,
                                        t->psh_hash_len ? t->psh_hash : nullptr)
                   : 0;
  cid.resize(chain_id_field_len(t->chain_id_len));
  put_chain_id_field(cid.data(), 0, (const uint8_t *)t->chain_id, t->chain_id_len);
  return TMED_OK;
}

bool VoteEncoder::device_template(uint8_t *out, size_t cap, size_t slot) const {
  const size_t cid_len = cid.size();
  if (4 + (size_t)pre_len + bid_len + cid_len > cap || cid_len > 255) return false;
  // the longest message of this template: a Commit-flag vote whose timestamp has a 10-byte seconds
  // varint and a 10-byte nanos varint (any int32 nanos crosses the ABI; negative ones are 10 bytes)
  if (vote_msg_len(vote_body_len(pre_len, bid_len, kTimestampFieldMax, (uint32_t)cid_len)) > slot) return false;
  out[0] = (uint8_t)pre_len;
  out[1] = (uint8_t)bid_len;
  out[2] = (uint8_t)cid_len;
  out[3] = 0;
  uint32_t p = put_bytes(out, 4, pre, pre_len);
  p = put_bytes(out, p, bid, bid_len);
  put_bytes(out, p, cid.data(), (uint32_t)cid_len);
  return true;
}

}  // namespace tmed

extern "C" int tmed_vote_sign_bytes(const tmed_vote_template *t, size_t n, const uint8_t *flags,
                                    const int64_t *ts_seconds, const int32_t *ts_nanos, uint8_t *out,
                                    size_t out_cap, uint32_t *out_off, size_t *out_len) {
  if (!t || (n && (!ts_seconds || !ts_nanos || !out_off))) return TMED_EINVAL;
  tmed::VoteEncoder enc;
  int rc = enc.init(t);
  if (rc != TMED_OK) return rc;
  size_t pos = 0;
  for (size_t i = 0; i < n; i++) {
    const int f = flags ? flags[i] : 2;
    if (f < 1 || f > 3) return TMED_EINVAL;  // CommitSig.BlockID panics on unknown flags (types/block.go:663)
    if (f == 2 && !enc.bid_ok) return TMED_EINVAL;  // CanonicalizeBlockID panics (types/canonical.go:18-22)
    const size_t total = enc.size(f, ts_seconds[i], ts_nanos[i]);
    out_off[i] = (uint32_t)pos;
    if (out && pos + total <= out_cap) enc.write(out + pos, f, ts_seconds[i], ts_nanos[i]);
    pos += total;
    if (pos > 0xffffffffu) return TMED_EINVAL;
  }
  if (n) out_off[n] = (uint32_t)pos;
  if (out_len) *out_len = pos;
  return (out && pos > out_cap) ? TMED_ENOMEM : TMED_OK;
}
