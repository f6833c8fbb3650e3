// votes.hip — free-standing votes on gfx950: vote_prepare_kernel and the device batch of
// tmed_verify_votes (include/tmed25519.h states the call; vote_free.h is the encoder, over the field
// writers of vote_wire.h, and the checks, shared with the host; votes_host.h the host entries, the
// signature helpers and the host's key words).  What the call shares with tmed_verify_duplicate_votes
// lives in two headers: slot_rows.h (device: record staging, slot zeroing, the coalesced slot
// write-out, the key words) and slot_batch.h (host: the grouping by route and key set, the distinct
// sets, the device-route envelope, the host route's second half, the choice of verifier).  This
// file keeps what is the votes' own: the kernel's checks, the staging layout, the records and the
// mapping of the results to codes.
//
// vote_prepare_kernel: one lane per vote, one wavefront per workgroup of 64 votes, laid out like
// assemble_votes_kernel (kernels.hip).  A lane stages its 144-byte record (VoteRec, nine 16-byte
// loads) into LDS, zeroes its 256-byte message slot in LDS, runs the checks 1-7 of vote_free.h (one
// sha256_compress for the key's address; the key comes from the key set's table on the keyed route,
// from the staged keys on the generic one) and, when every check passes, writes VoteSignBytes into
// the slot.  The wavefront then writes its 64 slots out as sixteen coalesced 1-KB rows: no per-byte
// global store (wave_store_slots' comment records what those cost).  LDS per workgroup:
// 64 x 144 B of records + 64 x 256 B of slots = 25,600 B; __launch_bounds__(64).
// Outputs per vote: the slot, the message length (0 where a check fails: the verify kernels then
// hash an empty message and their bit is ignored), the precheck code.
//
// The signatures are decided by the commit seam's launchers in their msg_slots mode (verify_sigs:
// the latency kernels up to lat_max / glat_max votes, the throughput kernels above), none of which
// changes.
#include <hip/hip_runtime.h>
#include <string.h>

#include <utility>
#include <vector>

#include "../../include/tmed25519.h"
#include "host_for.h"
#include "slot_batch.h"
#include "slot_rows.h"
#include "votes_host.h"

namespace tmed {

constexpr uint32_t kVprepLanes = kSlotLanes;
constexpr uint32_t kVoteRecInt4 = kVoteRecBytes / 16;

__global__ __launch_bounds__(kVprepLanes) void vote_prepare_kernel(VotePrep p, uint32_t n) {
  __shared__ int4 rl[kVprepLanes][kVoteRecInt4];
  __shared__ int4 ob[kVprepLanes][kVoteSlot / 16];
  const uint32_t lane = threadIdx.x, i0 = blockIdx.x * kVprepLanes, i = i0 + lane;
  if (i < n) {
    lds_stage<kVoteRecInt4>(rl[lane], p.recs + (size_t)i * kVoteRecInt4);
    lds_zero<kSlotInt4>(ob[lane]);
    const VoteRec &r = *reinterpret_cast<const VoteRec *>(rl[lane]);
    const VoteStep &s = p.steps[r.req];
    uint8_t code = vote_prechecks(r, s, p.set_addr + 20 * s.addr_base, [&](uint32_t w[8]) {
      const int4 *k = reinterpret_cast<const int4 *>(p.pubs ? p.pubs + 32 * (size_t)i : p.key_pub + 32 * (size_t)r.key);
      key_words(k[0], k[1], w);
    });
    // the host sends only requests whose chain ID fits (votes_host.h device_route); never write past the slot
    if (code == 0 && s.cid_len > kVoteChainMax) code = kVoteGoPath;
    uint32_t len = 0;
    if (code == 0) len = vote_free_write(r, s.chain, s.cid_len, reinterpret_cast<uint8_t *>(ob[lane]));
    p.lens[i] = len;
    p.codes[i] = code;
  }
  __syncthreads();
  wave_store_slots<1>(&ob[0][0], p.slots, i0, n);
}

hipError_t launch_vote_prepare(const VotePrep &p, uint32_t n, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vote_prepare_kernel, dim3((n + kVprepLanes - 1) / kVprepLanes), dim3(kVprepLanes), 0, stream, p, n);
  return hipGetLastError();
}

namespace {

namespace VH = tmed_votes_host;

// The key of vote i of request q: its index in the key set (keyed; 0 when the validator index is
// outside the set: check 4 fails before the key is read) or its 32 bytes (generic; zeros then).
bool vote_key_index(const tmed_valset &vs, int32_t vi, size_t nkeys, uint32_t *out) {
  *out = 0;
  if (vi < 0 || (size_t)vi >= vs.n) return true;
  const uint32_t k = vs.keyset_index ? vs.keyset_index[vi] : (uint32_t)vi;
  *out = k;
  return k < nkeys;
}
void vote_key_bytes(const tmed_valset &vs, int32_t vi, uint8_t *out) {
  if (vi < 0 || (size_t)vi >= vs.n) memset(out, 0, 32);
  else memcpy(out, vs.pubkeys + 32 * (size_t)vi, 32);
}
uint8_t vote_outcome(uint8_t pre, bool valid, const tmed_votes &v, size_t i) {
  return pre ? pre : (valid && VH::sig_full(v, i)) ? TMED_VOTE_OK : TMED_VOTE_INVALID_SIGNATURE;
}

// Device route (slot_batch.h slot_batch_device): records, steps and set addresses in, one prepare
// launch, codes and validity bits out.
int run_group_device(tmed_ctx *c, const tmed_vote_request *reqs, const size_t *base, const SlotGroup &g, Keyset *ks,
                     uint8_t *codes) {
  const int rule = seam_rule(c);  // ctx->mu is held from the call's entry: one value for all its groups
  const size_t m = g.m, G = g.reqs.size();
  SetTable sets;  // the addresses of the ADDVOTE requests' sets
  for (const size_t q : g.reqs)
    if (reqs[q].flags & TMED_VOTES_ADDVOTE) sets.add(reqs[q].vals);
  const size_t o_rec = 0, o_step = align256(o_rec + m * kVoteRecBytes), o_addr = align256(o_step + G * sizeof(VoteStep)),
               o_key = align256(o_addr + 20 * sets.n_vals), o_sig = align256(o_key + m * (ks ? 4 : 32)),
               o_code = align256(o_sig + m * 64), o_valid = align256(o_code + m), o_slot = align256(o_valid + m),
               o_len = align256(o_slot + m * kVoteSlot), total = align256(o_len + m * 4);
  hipError_t e = c->stage.ensure(o_slot, total);  // the slots and lengths stay on the device
  if (e == hipSuccess && !c->vote_ev) e = hipEventCreate(&c->vote_ev);
  if (e != hipSuccess) return map_err(e);
  uint8_t *h = c->stage.host(), *d = c->stage.dev();
  VoteStep *steps = reinterpret_cast<VoteStep *>(h + o_step);
  bool keys_ok = true;
  size_t at = 0;
  std::vector<size_t> start(G);
  for (size_t j = 0; j < G; j++) {
    const tmed_vote_request &rq = reqs[g.reqs[j]];
    VH::fill_step(rq, (rq.flags & TMED_VOTES_ADDVOTE) ? sets.at(rq.vals) : 0, steps[j]);
    start[j] = at;
    at += rq.votes->n;
  }
  for (const tmed_valset *vs : sets.sets)
    if (vs->n) memcpy(h + o_addr + 20 * sets.at(vs), vs->addresses, 20 * vs->n);
  host_for(G, pack_threads(m), [&](size_t j) {
    const tmed_vote_request &rq = reqs[g.reqs[j]];
    const tmed_votes &v = *rq.votes;
    bool ok = true;
    for (size_t i = 0; i < v.n; i++) {
      const size_t k = start[j] + i;
      uint32_t key = 0;
      if (ks) {
        ok = vote_key_index(*rq.vals, v.validator_indexes[i], ks->n, &key) && ok;
        reinterpret_cast<uint32_t *>(h + o_key)[k] = key;
      } else {
        vote_key_bytes(*rq.vals, v.validator_indexes[i], h + o_key + 32 * k);
      }
      VH::fill_rec(v, i, (uint32_t)j, key, *reinterpret_cast<VoteRec *>(h + o_rec + k * kVoteRecBytes));
      VH::vote_sig(v, i, h + o_sig + 64 * k);
    }
    if (!ok) __atomic_store_n(&keys_ok, false, __ATOMIC_RELAXED);
  });
  if (!keys_ok) return TMED_EINVAL;  // a keyset_index past the key set
  const VotePrep p{reinterpret_cast<const int4 *>(d + o_rec), reinterpret_cast<const VoteStep *>(d + o_step), d + o_addr,
                   ks ? nullptr : d + o_key, ks ? ks->d_pub : nullptr, d + o_slot, reinterpret_cast<uint32_t *>(d + o_len),
                   d + o_code};
  const int rc = slot_batch_device(
      c, o_code, o_code, o_slot,
      [&](hipStream_t s) {
        const hipError_t el = launch_vote_prepare(p, (uint32_t)m, s);
        return el == hipSuccess ? hipEventRecord(c->vote_ev, s) : el;
      },
      SlotSigs{ks, d + o_key, d + o_sig, d + o_slot, p.lens, (uint32_t)m, d + o_valid, rule});
  if (rc != TMED_OK) return rc;
  float pms = 0.f;
  (void)hipEventElapsedTime(&pms, c->ev0, c->vote_ev);
  c->last_vote_prep_ms += pms;
  for (size_t j = 0; j < G; j++) {
    const tmed_votes &v = *reqs[g.reqs[j]].votes;
    uint8_t *out = codes + base[g.reqs[j]];
    for (size_t i = 0; i < v.n; i++) out[i] = vote_outcome(h[o_code + start[j] + i], h[o_valid + start[j] + i], v, i);
  }
  return TMED_OK;
}

// Host route (a chain ID past kVoteChainMax; slot_batch.h slot_batch_host): checks and messages by
// the same source on the host, the messages packed behind each other.
int run_group_host(tmed_ctx *c, const tmed_vote_request *reqs, const size_t *base, const SlotGroup &g, Keyset *ks,
                   uint8_t *codes) {
  const size_t m = g.m;
  std::vector<uint8_t> pre(m), valid(m);
  std::vector<std::pair<size_t, size_t>> src(m);  // vote k: its request and its index there
  MsgPack mp;
  size_t k = 0;
  for (const size_t q : g.reqs) {
    const tmed_votes &v = *reqs[q].votes;
    VH::request_prechecks_host(reqs[q], pre.data() + k);
    for (size_t i = 0; i < v.n; i++, k++) {
      src[k] = {q, i};
      if (pre[k]) {
        mp.skip();
        continue;
      }
      VoteRec r;
      VH::fill_rec(v, i, 0, 0, r);
      uint8_t *msg = mp.next(vote_free_size(r, reqs[q].chain_id_len));
      if (!msg) return TMED_EINVAL;
      vote_free_write(r, (const uint8_t *)reqs[q].chain_id, reqs[q].chain_id_len, msg);
    }
  }
  const int rc = slot_batch_host(
      c, ks, seam_rule(c), mp,
      [&](size_t j, uint8_t *out) {
        const tmed_vote_request &rq = reqs[src[j].first];
        const int32_t vi = rq.votes->validator_indexes[src[j].second];
        if (ks) return vote_key_index(*rq.vals, vi, ks->n, reinterpret_cast<uint32_t *>(out));
        vote_key_bytes(*rq.vals, vi, out);
        return true;
      },
      [&](size_t j, uint8_t *out) { VH::vote_sig(*reqs[src[j].first].votes, src[j].second, out); }, valid.data());
  if (rc != TMED_OK) return rc;
  for (k = 0; k < m; k++) {
    const size_t q = src[k].first, i = src[k].second;
    codes[base[q] + i] = vote_outcome(pre[k], valid[k], *reqs[q].votes, i);
  }
  return TMED_OK;
}

}  // namespace

int verify_votes_locked(tmed_ctx *c, const tmed_vote_request *reqs, size_t n, uint8_t *codes) {
  c->last_ms = 0.f;
  c->last_vote_prep_ms = 0.f;
  (void)hipSetDevice(c->device);
  return run_slot_groups(
      c, n, 0x7fffffffu, [&](size_t q) { return (size_t)reqs[q].votes->n; }, [&](size_t q) { return VH::device_route(reqs[q]); },
      [&](size_t q) { return reqs[q].vals->keyset; },
      [&](const SlotGroup &g, Keyset *ks, const size_t *base) {
        return g.device ? run_group_device(c, reqs, base, g, ks, codes) : run_group_host(c, reqs, base, g, ks, codes);
      });
}

}  // namespace tmed

extern "C" {

float tmed_votes_last_prepare_ms(tmed_ctx *c) { return c ? c->last_vote_prep_ms : 0.f; }

}  // extern "C"
