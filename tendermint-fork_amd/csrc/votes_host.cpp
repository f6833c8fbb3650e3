// votes_host.cpp — the host entries of the free-standing votes: tmed_votes_sign_bytes and
// tmed_verify_votes_host (include/tmed25519.h), and the per-request prechecks the device batch's
// host route uses (votes.hip run_group_host).  Plain C++ (no HIP): see votes_host.h.
#include "votes_host.h"

namespace tmed_votes_host {

void request_prechecks_host(const tmed_vote_request &q, uint8_t *codes) { request_prechecks(q, codes); }

}  // namespace tmed_votes_host

extern "C" {

int tmed_votes_sign_bytes(const char *chain_id, uint32_t chain_id_len, const tmed_votes *votes, uint8_t *out,
                          size_t out_cap, uint32_t *out_off, size_t *out_len, uint8_t *malformed) {
  return tmed_votes_host::votes_sign_bytes(chain_id, chain_id_len, votes, out, out_cap, out_off, out_len, malformed);
}

int tmed_verify_votes_host(const tmed_vote_request *reqs, size_t n_reqs, uint8_t *codes, uint32_t *msg_lens,
                           uint8_t *device_route) {
  return tmed_votes_host::verify_votes_host(reqs, n_reqs, codes, msg_lens, device_route);
}

}  // extern "C"
