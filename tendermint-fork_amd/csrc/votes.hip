// votes.hip — free-standing votes on gfx950: vote_prepare_kernel and the device batch of
// tmed_verify_votes (include/tmed25519.h states the call; vote_free.h is the encoder, over the field
// writers of vote_wire.h, and the checks, shared with the host; votes_host.h the host entries).
//
// vote_prepare_kernel: one lane per vote, one wavefront per workgroup of 64 votes, laid out like
// assemble_votes_kernel (kernels.hip).  A lane stages its 144-byte record (VoteRec, nine 16-byte
// loads) into LDS, zeroes its 256-byte message slot in LDS, runs the checks 1-7 of vote_free.h (one
// sha256_compress for the key's address; the key comes from the key set's table on the keyed route,
// from the staged keys on the generic one) and, when every check passes, writes VoteSignBytes into
// the slot.  The wavefront then writes its 64 slots out as sixteen coalesced 1-KB rows: no per-byte
// global store (assemble_votes_kernel's comment records what those cost).  LDS per workgroup:
// 64 x 144 B of records + 64 x 256 B of slots = 25,600 B; __launch_bounds__(64).
// Outputs per vote: the slot, the message length (0 where a check fails: the verify kernels then
// hash an empty message and their bit is ignored), the precheck code.
//
// The signatures are decided by the commit seam's launchers in their msg_slots mode
// (keyset_verify / generic_verify: the latency kernels up to lat_max / glat_max votes, the
// throughput kernels above), none of which changes.
#include <hip/hip_runtime.h>
#include <string.h>

#include <map>
#include <unordered_map>
#include <vector>

#include "../../include/tmed25519.h"
#include "call_frame.h"
#include "host_for.h"
#include "votes_host.h"

namespace tmed {

constexpr uint32_t kVprepLanes = 64;
constexpr uint32_t kVoteRecInt4 = kVoteRecBytes / 16;

__global__ __launch_bounds__(kVprepLanes) void vote_prepare_kernel(VotePrep p, uint32_t n) {
  __shared__ int4 rl[kVprepLanes][kVoteRecInt4];
  __shared__ int4 ob[kVprepLanes][kVoteSlot / 16];
  const uint32_t lane = threadIdx.x, i0 = blockIdx.x * kVprepLanes, i = i0 + lane;
  if (i < n) {
    {
      const int4 *src = p.recs + (size_t)i * kVoteRecInt4;
      int4 v[kVoteRecInt4];
#pragma unroll
      for (int q = 0; q < (int)kVoteRecInt4; q++) v[q] = src[q];
#pragma unroll
      for (int q = 0; q < (int)kVoteRecInt4; q++) rl[lane][q] = v[q];
    }
#pragma unroll
    for (int q = 0; q < (int)(kVoteSlot / 16); q++) ob[lane][q] = make_int4(0, 0, 0, 0);
    const VoteRec &r = *reinterpret_cast<const VoteRec *>(rl[lane]);
    const VoteStep &s = p.steps[r.req];
    uint8_t code = vote_prechecks(r, s, p.set_addr + 20 * s.addr_base, [&](uint32_t w[8]) {
      const int4 *k = reinterpret_cast<const int4 *>(p.pubs ? p.pubs + 32 * (size_t)i : p.key_pub + 32 * (size_t)r.key);
      const int4 a = k[0], b = k[1];
      w[0] = (uint32_t)a.x; w[1] = (uint32_t)a.y; w[2] = (uint32_t)a.z; w[3] = (uint32_t)a.w;
      w[4] = (uint32_t)b.x; w[5] = (uint32_t)b.y; w[6] = (uint32_t)b.z; w[7] = (uint32_t)b.w;
    });
    // the host sends only requests whose chain ID fits (votes_host.h device_route); never write past the slot
    if (code == 0 && s.cid_len > kVoteChainMax) code = kVoteGoPath;
    uint32_t len = 0;
    if (code == 0) len = vote_free_write(r, s.chain, s.cid_len, reinterpret_cast<uint8_t *>(ob[lane]));
    p.lens[i] = len;
    p.codes[i] = code;
  }
  __syncthreads();
  const uint32_t nslots = n - i0 < kVprepLanes ? n - i0 : kVprepLanes;
  int4 *dst = reinterpret_cast<int4 *>(p.slots + (size_t)i0 * kVoteSlot);
  const int4 *src = &ob[0][0];
#pragma unroll
  for (uint32_t q = 0; q < kVoteSlot / 16; q++) {
    const uint32_t c = q * kVprepLanes + lane;  // int4 index in the wave's 16-KB run of slots
    if (c / (kVoteSlot / 16) < nslots) dst[c] = src[c];
  }
}

hipError_t launch_vote_prepare(const VotePrep &p, uint32_t n, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vote_prepare_kernel, dim3((n + kVprepLanes - 1) / kVprepLanes), dim3(kVprepLanes), 0, stream, p, n);
  return hipGetLastError();
}

namespace {

namespace VH = tmed_votes_host;

// One group of the call: the requests that share a route and a key set.
struct VoteGroup {
  bool device;
  uint64_t keyset;
  std::vector<size_t> reqs;
  size_t m = 0;
};

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
void vote_sig(const tmed_votes &v, size_t i, uint8_t *out) {
  const uint32_t sl = v.sig_lens ? v.sig_lens[i] : 64;
  memcpy(out, v.sigs + 64 * i, sl < 64 ? sl : 64);
  if (sl < 64) memset(out + sl, 0, 64 - sl);
}

// Device route: records, steps and set addresses in, one prepare launch, the verify launchers in
// msg_slots mode, codes and validity bits out.
int run_group_device(tmed_ctx *c, const tmed_vote_request *reqs, const size_t *base, const VoteGroup &g, Keyset *ks,
                     uint8_t *codes) {
  const int rule = seam_rule(c);  // ctx->mu is held from the call's entry: one value for all its groups
  const size_t m = g.m, G = g.reqs.size();
  // each distinct set's addresses once (ADDVOTE requests only)
  std::unordered_map<const tmed_valset *, uint64_t> abase;
  std::vector<const tmed_valset *> asets;
  size_t n_addr = 0;
  for (const size_t q : g.reqs) {
    if (!(reqs[q].flags & TMED_VOTES_ADDVOTE)) continue;
    if (abase.emplace(reqs[q].vals, n_addr).second) {
      asets.push_back(reqs[q].vals);
      n_addr += reqs[q].vals->n;
    }
  }
  const size_t o_rec = 0, o_step = align256(o_rec + m * kVoteRecBytes), o_addr = align256(o_step + G * sizeof(VoteStep)),
               o_key = align256(o_addr + 20 * n_addr), o_sig = align256(o_key + m * (ks ? 4 : 32)),
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
    const auto it = abase.find(rq.vals);
    VH::fill_step(rq, (rq.flags & TMED_VOTES_ADDVOTE) ? it->second : 0, steps[j]);
    start[j] = at;
    at += rq.votes->n;
  }
  for (const tmed_valset *vs : asets)
    if (vs->n) memcpy(h + o_addr + 20 * abase[vs], vs->addresses, 20 * vs->n);
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
      vote_sig(v, i, h + o_sig + 64 * k);
    }
    if (!ok) __atomic_store_n(&keys_ok, false, __ATOMIC_RELAXED);
  });
  if (!keys_ok) return TMED_EINVAL;  // a keyset_index past the key set
  hipStream_t s = c->stream;
  e = hipMemcpyAsync(d, h, o_code, hipMemcpyHostToDevice, s);  // one copy in
  if (e == hipSuccess) e = scratch_acquire(c, s);
  const bool acquired = e == hipSuccess;
  if (e == hipSuccess) e = hipEventRecord(c->ev0, s);
  if (e == hipSuccess)
    e = launch_vote_prepare(VotePrep{reinterpret_cast<const int4 *>(d + o_rec), reinterpret_cast<const VoteStep *>(d + o_step),
                                     d + o_addr, ks ? nullptr : d + o_key, ks ? ks->d_pub : nullptr, d + o_slot,
                                     reinterpret_cast<uint32_t *>(d + o_len), d + o_code},
                            (uint32_t)m, s);
  if (e == hipSuccess) e = hipEventRecord(c->vote_ev, s);
  if (e == hipSuccess) {
    const uint32_t *lens = reinterpret_cast<const uint32_t *>(d + o_len);
    e = ks ? keyset_verify_batch(c, *ks, reinterpret_cast<const uint32_t *>(d + o_key), d + o_sig, d + o_slot, lens,
                                 (uint32_t)m, d + o_valid, s, /*msg_slots=*/true, rule)
           : generic_verify(c, d + o_key, d + o_sig, d + o_slot, lens, (uint32_t)m, d + o_valid, s, /*msg_slots=*/true,
                            nullptr, nullptr, rule);
  }
  if (e == hipSuccess) e = hipEventRecord(c->ev1, s);
  if (acquired) {
    const hipError_t er = scratch_release(c, s);
    if (e == hipSuccess) e = er;
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h + o_code, d + o_code, o_slot - o_code, hipMemcpyDeviceToHost, s);
  float ms = 0.f, pms = 0.f;
  const int rc = finish_call(c, s, e, &ms);
  if (rc != TMED_OK) return rc;
  (void)hipEventElapsedTime(&pms, c->ev0, c->vote_ev);
  c->last_ms += ms;
  c->last_vote_prep_ms += pms;
  for (size_t j = 0; j < G; j++) {
    const tmed_votes &v = *reqs[g.reqs[j]].votes;
    uint8_t *out = codes + base[g.reqs[j]];
    for (size_t i = 0; i < v.n; i++) {
      const size_t k = start[j] + i;
      const uint8_t pre = h[o_code + k];
      const bool sig_full = !v.sig_lens || v.sig_lens[i] == 64;  // crypto/ed25519/ed25519.go:150-152
      out[i] = pre ? pre : (h[o_valid + k] && sig_full) ? TMED_VOTE_OK : TMED_VOTE_INVALID_SIGNATURE;
    }
  }
  return TMED_OK;
}

// Host route (a chain ID past kVoteChainMax): checks and messages by the same source on the host,
// the messages packed behind each other, the verify launchers in their offset mode.
int run_group_host(tmed_ctx *c, const tmed_vote_request *reqs, const size_t *base, const VoteGroup &g, Keyset *ks,
                   uint8_t *codes) {
  const int rule = seam_rule(c);  // ctx->mu is held from the call's entry: one value for all its groups
  const size_t m = g.m;
  std::vector<uint8_t> pre(m), valid(m), msgs;
  std::vector<uint32_t> off(m + 1);
  size_t k = 0, pos = 0;
  for (const size_t q : g.reqs) {
    const tmed_votes &v = *reqs[q].votes;
    VH::request_prechecks_host(reqs[q], pre.data() + k);
    for (size_t i = 0; i < v.n; i++, k++) {
      off[k] = (uint32_t)pos;
      if (pre[k]) continue;
      VoteRec r;
      VH::fill_rec(v, i, 0, 0, r);
      const size_t len = vote_free_size(r, reqs[q].chain_id_len);
      if (pos + len > 0xffffffffu) return TMED_EINVAL;
      msgs.resize(pos + len);
      vote_free_write(r, (const uint8_t *)reqs[q].chain_id, reqs[q].chain_id_len, msgs.data() + pos);
      pos += len;
    }
  }
  off[m] = (uint32_t)pos;
  RawStage st;
  int rc = raw_stage(c, ks ? 4 : 32, m, pos, st);
  if (rc != TMED_OK) return rc;
  k = 0;
  for (const size_t q : g.reqs) {
    const tmed_votes &v = *reqs[q].votes;
    for (size_t i = 0; i < v.n; i++, k++) {
      if (ks) {
        if (!vote_key_index(*reqs[q].vals, v.validator_indexes[i], ks->n, (uint32_t *)st.keys + k)) return TMED_EINVAL;
      } else {
        vote_key_bytes(*reqs[q].vals, v.validator_indexes[i], st.keys + 32 * k);
      }
      vote_sig(v, i, st.sigs + 64 * k);
    }
  }
  if (pos) memcpy(st.msgs, msgs.data(), pos);
  memcpy(st.off, off.data(), (m + 1) * 4);
  rc = raw_run(c, st, /*timed=*/true,
               [&](const uint8_t *d_key, const uint8_t *d_sig, const uint8_t *d_msg, const uint32_t *d_off, uint32_t n,
                   uint8_t *d_out, hipStream_t s) {
                 return map_err(ks ? keyset_verify_batch(c, *ks, (const uint32_t *)d_key, d_sig, d_msg, d_off, n, d_out, s,
                                                         /*msg_slots=*/false, rule)
                                   : generic_verify(c, d_key, d_sig, d_msg, d_off, n, d_out, s, /*msg_slots=*/false, nullptr,
                                                    nullptr, rule));
               },
               valid.data(), nullptr);
  if (rc != TMED_OK) return rc;
  c->last_ms += st.ms;
  k = 0;
  for (const size_t q : g.reqs) {
    const tmed_votes &v = *reqs[q].votes;
    uint8_t *out = codes + base[q];
    for (size_t i = 0; i < v.n; i++, k++) {
      const bool sig_full = !v.sig_lens || v.sig_lens[i] == 64;
      out[i] = pre[k] ? pre[k] : (valid[k] && sig_full) ? TMED_VOTE_OK : TMED_VOTE_INVALID_SIGNATURE;
    }
  }
  return TMED_OK;
}

}  // namespace

int verify_votes_locked(tmed_ctx *c, const tmed_vote_request *reqs, size_t n, uint8_t *codes) {
  std::vector<size_t> base(n + 1, 0);
  std::map<std::pair<bool, uint64_t>, VoteGroup> groups;
  for (size_t q = 0; q < n; q++) {
    base[q + 1] = base[q] + reqs[q].votes->n;
    if (reqs[q].votes->n == 0) continue;
    const bool dev = VH::device_route(reqs[q]);
    VoteGroup &g = groups[{!dev, reqs[q].vals->keyset}];
    g.device = dev;
    g.keyset = reqs[q].vals->keyset;
    g.reqs.push_back(q);
    g.m += reqs[q].votes->n;
  }
  c->last_ms = 0.f;
  c->last_vote_prep_ms = 0.f;
  (void)hipSetDevice(c->device);
  for (auto &kv : groups) {
    const VoteGroup &g = kv.second;
    if (g.m > 0x7fffffffu) return TMED_EINVAL;
    Keyset *ks = nullptr;
    if (g.keyset) {
      auto it = c->keysets.find(g.keyset);
      if (it == c->keysets.end()) return TMED_ENOKEYSET;
      ks = &it->second;
    }
    const int rc = g.device ? run_group_device(c, reqs, base.data(), g, ks, codes)
                            : run_group_host(c, reqs, base.data(), g, ks, codes);
    if (rc != TMED_OK) return rc;
  }
  return TMED_OK;
}

}  // namespace tmed

extern "C" {

float tmed_votes_last_prepare_ms(tmed_ctx *c) { return c ? c->last_vote_prep_ms : 0.f; }

}  // extern "C"
