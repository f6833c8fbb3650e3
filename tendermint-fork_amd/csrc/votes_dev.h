// votes_dev.h — CanonicalVote sign-bytes assembly on the device, shared by
// assemble_votes_kernel (kernels.hip) and the hash lanes of the generic latency kernel
// (latency.hip), which assemble their own message instead of waiting for a separate launch.
//
// Per commit a template (signbytes.hip VoteEncoder::device_template): [pre_len, bid_len, cid_len, 0]
// then the pre bytes (type/height/round), the complete BlockID field and the complete chain-id
// field.  Per vote only the flag and the timestamp vary (types/block.go:784-810): the message is
// vote_wire.h's vote_splice of the three ranges, the BlockID field only under flag == Commit
// (signbytes.h vote_from_template, which the host tests run on the same records).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace tmed {

// Vote i into o (at most kVoteSlot bytes); returns its length.  tl: this lane's kVoteTmplBytes of
// LDS — the template is staged there with sixteen independent 16-B loads, so a template in pinned
// host memory (small batches, keyset.hip votes_enqueue) costs one bus round trip instead of one
// per byte of the copy loops.
__device__ __forceinline__ uint32_t assemble_vote_into(const VoteAsm &va, uint32_t i, uint8_t *__restrict__ o,
                                                       int4 *tl) {
  {
    const int4 *src = reinterpret_cast<const int4 *>(va.tmpl + (size_t)va.tmpl_idx[i] * kVoteTmplBytes);
    int4 v[kVoteTmplBytes / 16];
#pragma unroll
    for (int q = 0; q < (int)(kVoteTmplBytes / 16); q++) v[q] = src[q];
#pragma unroll
    for (int q = 0; q < (int)(kVoteTmplBytes / 16); q++) tl[q] = v[q];
  }
  return vote_from_template(o, reinterpret_cast<const uint8_t *>(tl), va.flags[i], va.ts_sec[i], va.ts_nanos[i]);
}

// Vote i into its kVoteSlot-byte slot of out, its length into out_len[i] (the latency kernels'
// hash lanes, which assemble their own message in place).
__device__ __forceinline__ void assemble_vote(const VoteAsm &va, uint32_t i, uint8_t *__restrict__ out,
                                              uint32_t *__restrict__ out_len, int4 *tl) {
  out_len[i] = assemble_vote_into(va, i, out + (size_t)i * kVoteSlot, tl);
}

}  // namespace tmed
