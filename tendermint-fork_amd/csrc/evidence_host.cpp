// evidence_host.cpp — the host entries of DuplicateVoteEvidence: tmed_evidence_bytes and
// tmed_verify_duplicate_votes_host (include/tmed25519.h), and the per-request lanes the device batch's
// host route uses (evidence.hip run_group_host).  Plain C++ (no HIP): see evidence_host.h.
#include "evidence_host.h"

#include "api_guard.h"

namespace tmed_evidence_host {

void request_lanes_host(const tmed_dup_request &q, HostLane *lanes) { request_lanes(q, lanes); }

}  // namespace tmed_evidence_host

extern "C" {

int tmed_evidence_bytes(const tmed_dup_evidence *ev, uint8_t *out, size_t out_cap, uint32_t *out_off, size_t *out_len,
                        uint8_t *ok) {
  return tmed_evidence_host::evidence_bytes(ev, out, out_cap, out_off, out_len, ok);
}

int tmed_verify_duplicate_votes_host(const tmed_dup_request *reqs, size_t n_reqs, uint8_t *pre_codes, uint8_t *vote_states,
                                     int32_t *found, uint32_t *msg_lens, uint8_t *device_route) {
  return guarded([&] {
    return tmed_evidence_host::verify_duplicate_votes_host(reqs, n_reqs, pre_codes, vote_states, found, msg_lens,
                                                           device_route);
  });
}

}  // extern "C"
