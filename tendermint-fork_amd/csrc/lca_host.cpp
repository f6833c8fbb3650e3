// lca_host.cpp — the host entries of LightClientAttackEvidence: tmed_byzantine_validators_host and
// tmed_verify_light_client_attacks_with (include/tmed25519.h).  Plain C++ (no HIP): see lca_host.h.
#include "lca_host.h"

#include "api_guard.h"

extern "C" {

int tmed_byzantine_validators_host(const tmed_lca_request *reqs, size_t n, int32_t *byz, const uint64_t *byz_off,
                                   tmed_byz_result *out) {
  return guarded([&] { return tmed_lca::byzantine_validators_host(reqs, n, byz, byz_off, out); });
}

int tmed_verify_light_client_attacks_with(const tmed_lca_request *reqs, size_t n, uint32_t flags, int32_t *byz,
                                          const uint64_t *byz_off, tmed_lca_result *out,
                                          const uint8_t *conflicting_hashes, const uint8_t *conflicting_ok,
                                          const uint8_t *trusted_hashes, const uint8_t *trusted_ok,
                                          tmed_batch_verify_fn verify, void *user) {
  if (!verify || (n && (!conflicting_hashes || !conflicting_ok || !trusted_hashes || !trusted_ok))) return TMED_EINVAL;
  return guarded([&] {
    return tmed_lca::lca_run(
        reqs, n, flags, byz, byz_off, out,
        [&](const std::vector<size_t> &live, uint8_t *ch, uint8_t *cok, uint8_t *th, uint8_t *tok) {
          for (const size_t i : live) {
            memcpy(ch + 32 * i, conflicting_hashes + 32 * i, 32);
            memcpy(th + 32 * i, trusted_hashes + 32 * i, 32);
            cok[i] = conflicting_ok[i];
            tok[i] = trusted_ok[i];
          }
          return (int)TMED_OK;
        },
        [&](const tmed_commit_request *rq, size_t m, tmed_commit_result *res) {
          return tmed_verify_commits_with(rq, m, res, verify, user);
        },
        [&](const std::vector<size_t> &live, const uint8_t *ch, const uint8_t *cok, const std::vector<size_t> &need,
            const int *kinds, tmed_byz_result *bres, uint8_t *ev_hash) {
          return tmed_lca::tail_host(reqs, live, ch, cok, need, kinds, byz, byz_off, bres, ev_hash);
        });
  });
}

}  // extern "C"
