// validate_host.cpp — the host entry of block validation: tmed_validate_blocks_with
// (include/tmed25519.h).  Plain C++ (no HIP): see validate_host.h.
#include "validate_host.h"

#include "api_guard.h"

extern "C" int tmed_validate_blocks_with(const tmed_block_batch *batch, tmed_block_result *out,
                                         const uint8_t *commit_hashes, const uint8_t *commit_ok,
                                         const uint8_t *data_hashes, const uint8_t *evidence_hashes,
                                         const uint8_t *evidence_ok, const uint8_t *header_hashes,
                                         const uint8_t *header_ok, const uint8_t *validators_hashes,
                                         const uint8_t *next_validators_hashes, const tmed_median_result *medians,
                                         const int32_t *proposer_idx, tmed_batch_verify_fn verify, void *user) {
  namespace V = tmed_validate;
  if (!verify || !batch) return TMED_EINVAL;
  if (batch->n && (!commit_hashes || !commit_ok || !data_hashes || !evidence_hashes || !evidence_ok || !header_hashes ||
                   !header_ok || !validators_hashes || !next_validators_hashes || !medians || !proposer_idx))
    return TMED_EINVAL;
  return guarded([&] {
    return V::validate_run(
        batch, out,
        [&](const V::Plan &p, V::Hashes &H) {
          for (const size_t i : p.need) {
            memcpy(&H.commit[32 * i], commit_hashes + 32 * i, 32);
            memcpy(&H.data[32 * i], data_hashes + 32 * i, 32);
            memcpy(&H.evidence[32 * i], evidence_hashes + 32 * i, 32);
            memcpy(&H.vals[32 * i], validators_hashes + 32 * i, 32);
            memcpy(&H.next[32 * i], next_validators_hashes + 32 * i, 32);
            H.commit_ok[i] = commit_ok[i];
            H.evidence_ok[i] = evidence_ok[i];
          }
          for (const size_t i : p.need_hdr) {
            memcpy(&H.header[32 * i], header_hashes + 32 * i, 32);
            H.header_ok[i] = header_ok[i];
          }
          V::host_masks(p, H);
          return (int)TMED_OK;
        },
        [&](const tmed_median_request *, const std::vector<size_t> &m_of, tmed_median_result *mres,
            const std::vector<size_t> &need_prop, int32_t *proposer) {
          for (size_t j = 0; j < m_of.size(); j++) mres[j] = medians[m_of[j]];
          for (const size_t i : need_prop) proposer[i] = proposer_idx[i];
          return (int)TMED_OK;
        },
        [&](const tmed_commit_request *rq, size_t m, tmed_commit_result *res) {
          return tmed_verify_commits_with(rq, m, res, verify, user);
        });
  });
}
