// evidence.hip — DuplicateVoteEvidence on gfx950: the device batches of tmed_verify_duplicate_votes
// (VerifyDuplicateVote, evidence/verify.go:162-222) and tmed_evidence_hashes
// (DuplicateVoteEvidence.Hash and EvidenceList.Hash, types/evidence.go:90-103, :431-442).
// include/tmed25519.h states the calls; evidence_free.h holds the checks and the Bytes() encoder,
// shared with the host; evidence_host.h the host entries.  What tmed_verify_duplicate_votes shares
// with tmed_verify_votes lives in slot_rows.h (device: record staging, slot zeroing, the coalesced
// slot write-out, the key words) and slot_batch.h (host: the grouping by route and key set, the
// distinct sets, the device-route envelope, the host route's second half, the choice of verifier);
// the signature helpers are votes_host.h's.
//
// evidence_lookup_kernel: GetByAddress, one wavefront per evidence.  The lanes stride over the set's
// 20-byte addresses, each read as five dwords from the call's packed, 4-byte-aligned address array;
// the first stride in which a lane matches ends the scan, and the lowest matching lane of that stride
// (the wave-wide minimum of the matching index, taken from the ballot) is the first match in index
// order (addr_scan.h wave_first_address, shared with lca.hip).  No sort and no host map.
//
// evidence_prepare_kernel: one lane per evidence, one wavefront per workgroup of 64, laid out like
// vote_prepare_kernel (votes.hip).  A lane stages its two 144-byte VoteRecs and its 64-byte EvRec
// into LDS, zeroes its two 256-byte message slots, runs checks 2-7 of evidence_free.h against the
// validator the lookup found (one sha256_compress for the key's address) and the two votes' states,
// and writes both votes' sign-bytes with vote_free_write.  The wavefront then writes its 128 slots out
// as coalesced 1-KB rows.  LDS per workgroup: 64 x (288 + 64 + 512) B = 55,296 B.
// Outputs per evidence: the pre-code; per vote: the state, the slot, the message length (0 where no
// signature is to be checked: the verify kernels then hash an empty message and their bit is
// ignored) and the found validator's key (its key-set index, or its 32 bytes on the generic route).
//
// The lookup and the prepare are TWO kernels, not one: the lookup wants a wavefront per evidence
// (64 addresses compared per step), the prepare a lane per evidence (its checks and two encoders are
// serial per evidence).  Fused, either a wavefront would run 64 scans one after the other with one
// lane encoding at the end, or every lane would scan a whole set alone.
//
// The signatures are decided by the commit seam's launchers in their msg_slots mode over the 2n
// slots (verify_sigs), none of which changes.
//
// evidence_hash_kernel: one lane per evidence, 64 lanes per workgroup.  A lane stages the two VoteRecs
// and the EvRec, writes Bytes() into its LDS slot (kEvSlotDw = 131 dwords: the 520-byte bound, on an
// odd dword stride) and hashes the slot twice with sha256_of_slot (a loop: up to nine blocks):
// SHA-256(bytes) to ev_hashes, SHA-256(0x00 || bytes) as the evidence's Merkle leaf.  LDS per
// workgroup: 64 x (288 + 64 + 524) B = 56,064 B.  Opaque items are hashed by merkle_leaf_kernel;
// evidence_gather_kernel then copies each list item's leaf into level 0 (an evidence may be named by
// several lists), and merkle.hip's level builder makes the roots.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/tmed25519.h"
#include "addr_scan.h"
#include "evidence_host.h"
#include "host_for.h"
#include "merkle_levels.h"
#include "slot_batch.h"
#include "slot_rows.h"

namespace tmed {

constexpr uint32_t kEvLanes = kSlotLanes;
constexpr uint32_t kEvVoteInt4 = kVoteRecBytes / 16;  // 9
constexpr uint32_t kEvRecInt4 = kEvRecBytes / 16;     // 4
constexpr uint32_t kEvSlotInt4 = kSlotInt4;           // 16

// The inputs and outputs of the lookup and prepare kernels (device pointers).
struct EvPrep {
  const int4 *recs;          // 2n VoteRec: VoteA of evidence i at 2i, VoteB at 2i + 1
  const int4 *evs;           // n EvRec
  const EvStep *steps;       // one per request
  const uint8_t *set_addr;   // the requests' sets, packed: 20 B a validator
  const int64_t *set_pow;    //   8 B a validator
  const uint32_t *set_kidx;  //   keyed route: the validator's index in the key set
  const uint8_t *set_pub;    //   generic route: 32 B a validator
  const uint8_t *key_pub;    // keyed route: the key set's encodings
  uint32_t *found;           // n: the first validator with VoteA's address, kEvNone for nobody
  uint8_t *keys;             // 2n x 4 (keyed: key-set index) or 2n x 32 (generic: key bytes)
  uint8_t *slots;            // 2n x kVoteSlot
  uint32_t *lens;            // 2n
  uint8_t *pre;              // n
  uint8_t *state;            // 2n
};

__global__ __launch_bounds__(kEvLanes) void evidence_lookup_kernel(EvPrep p, uint32_t n) {
  const uint32_t i = blockIdx.x, lane = threadIdx.x;
  if (i >= n) return;
  const EvRec &e = *reinterpret_cast<const EvRec *>(p.evs + (size_t)i * kEvRecInt4);
  const EvStep &s = p.steps[e.req];
  uint32_t found = kEvNone;
  if (e.addr_len[0] == 20) {
    const uint32_t *rec = reinterpret_cast<const uint32_t *>(p.recs + (size_t)2 * i * kEvVoteInt4);
    uint32_t want[5];
#pragma unroll
    for (int k = 0; k < 5; k++) want[k] = rec[28 + k];  // VoteRec::addr
    found = wave_first_address(want, reinterpret_cast<const uint32_t *>(p.set_addr) + 5 * s.addr_base, s.n_vals, lane);
  }
  if (lane == 0) p.found[i] = found;
}

__global__ __launch_bounds__(kEvLanes) void evidence_prepare_kernel(EvPrep p, uint32_t n) {
  __shared__ int4 rl[kEvLanes][2 * kEvVoteInt4];
  __shared__ int4 el[kEvLanes][kEvRecInt4];
  __shared__ int4 ob[kEvLanes][2 * kEvSlotInt4];
  const uint32_t lane = threadIdx.x, i0 = blockIdx.x * kEvLanes, i = i0 + lane;
  if (i < n) {
    lds_stage<2 * kEvVoteInt4>(rl[lane], p.recs + (size_t)i * 2 * kEvVoteInt4);
    lds_stage<kEvRecInt4>(el[lane], p.evs + (size_t)i * kEvRecInt4);
    lds_zero<2 * kEvSlotInt4>(ob[lane]);
    const VoteRec *vr[2] = {reinterpret_cast<const VoteRec *>(rl[lane]),
                            reinterpret_cast<const VoteRec *>(rl[lane] + kEvVoteInt4)};
    const EvRec &e = *reinterpret_cast<const EvRec *>(el[lane]);
    const EvStep &s = p.steps[e.req];
    const uint32_t found = p.found[i];
    const bool has = found != kEvNone && found < s.n_vals;
    const size_t v = has ? (size_t)s.addr_base + found : 0;
    const uint32_t kidx = (has && p.set_kidx) ? p.set_kidx[v] : 0;
    const int4 *kp = reinterpret_cast<const int4 *>(p.set_pub ? p.set_pub + 32 * v : p.key_pub + 32 * (size_t)kidx);
    int4 k0 = make_int4(0, 0, 0, 0), k1 = k0;
    if (has) { k0 = kp[0]; k1 = kp[1]; }
    uint8_t pre = ev_prechecks(*vr[0], *vr[1], e, s, has ? found : kEvNone, has ? p.set_pow[v] : 0,
                               [&](uint32_t w[8]) { key_words(k0, k1, w); });
    // the host sends only requests whose chain ID fits (evidence_host.h device_route); never write past the slot
    if (pre == 0 && s.cid_len > kVoteChainMax) pre = kEvGoPath;
#pragma unroll 1
    for (int k = 0; k < 2; k++) {
      const uint8_t st = ev_vote_state(*vr[k]);
      uint32_t len = 0;
      if (pre == 0 && st == 0)
        len = vote_free_write(*vr[k], s.chain, s.cid_len, reinterpret_cast<uint8_t *>(ob[lane] + k * kEvSlotInt4));
      p.lens[2 * (size_t)i + k] = len;
      p.state[2 * (size_t)i + k] = st;
      if (p.set_pub) {
        int4 *ko = reinterpret_cast<int4 *>(p.keys + 32 * (2 * (size_t)i + k));
        ko[0] = k0;
        ko[1] = k1;
      } else {
        reinterpret_cast<uint32_t *>(p.keys)[2 * (size_t)i + k] = kidx;
      }
    }
    p.pre[i] = pre;
  }
  __syncthreads();
  wave_store_slots<2>(&ob[0][0], p.slots, i0, n);
}

// The inputs and outputs of the hash kernel.
struct EvHash {
  const int4 *recs;     // 2n VoteRec
  const int4 *evs;      // n EvRec
  const uint8_t *sigs;  // 2n x 64
  uint32_t *hashes;     // n x 32 B: DuplicateVoteEvidence.Hash(), bytes (zero where not encodable)
  uint32_t *leaves;     // n x 8 state words: leafHash(Bytes())
};

__global__ __launch_bounds__(kEvLanes) void evidence_hash_kernel(EvHash p, uint32_t n) {
  __shared__ int4 rl[kEvLanes][2 * kEvVoteInt4];
  __shared__ int4 el[kEvLanes][kEvRecInt4];
  __shared__ uint32_t sl[kEvLanes][kEvSlotDw];
  const uint32_t lane = threadIdx.x, i = blockIdx.x * kEvLanes + lane;
  if (i >= n) return;  // a lane touches its own rows of LDS only: no barrier in this kernel
  lds_stage<2 * kEvVoteInt4>(rl[lane], p.recs + (size_t)i * 2 * kEvVoteInt4);
  lds_stage<kEvRecInt4>(el[lane], p.evs + (size_t)i * kEvRecInt4);
  for (uint32_t q = 0; q < kEvSlotDw; q++) sl[lane][q] = 0;
  const VoteRec &a = *reinterpret_cast<const VoteRec *>(rl[lane]);
  const VoteRec &b = *reinterpret_cast<const VoteRec *>(rl[lane] + kEvVoteInt4);
  const EvRec &e = *reinterpret_cast<const EvRec *>(el[lane]);
  uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0}, leaf[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (evidence_encodable(a, b, e)) {
    const uint32_t len = evidence_write(a, b, e, p.sigs + 64 * (2 * (size_t)i), p.sigs + 64 * (2 * (size_t)i + 1),
                                        reinterpret_cast<uint8_t *>(sl[lane]));
    sha256_of_slot(h, 0, sl[lane], len);
    sha256_of_slot(leaf, 1, sl[lane], len);
#pragma unroll
    for (int k = 0; k < 8; k++) h[k] = bswap32(h[k]);
  }
  uint4 *ho = reinterpret_cast<uint4 *>(p.hashes + 8 * (size_t)i), *lo = reinterpret_cast<uint4 *>(p.leaves + 8 * (size_t)i);
  ho[0] = make_uint4(h[0], h[1], h[2], h[3]);
  ho[1] = make_uint4(h[4], h[5], h[6], h[7]);
  lo[0] = make_uint4(leaf[0], leaf[1], leaf[2], leaf[3]);
  lo[1] = make_uint4(leaf[4], leaf[5], leaf[6], leaf[7]);
}

// Level 0 of the lists' trees: item k's leaf, an evidence's (items[k] >= 0) or an opaque string's.
__global__ __launch_bounds__(256) void evidence_gather_kernel(const int64_t *__restrict__ items,
                                                              const uint4 *__restrict__ ev_leaves,
                                                              const uint4 *__restrict__ op_leaves, uint32_t n_items,
                                                              uint4 *__restrict__ out) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_items) return;
  const int64_t it = items[k];
  const uint4 *src = it >= 0 ? ev_leaves + 2 * (size_t)it : op_leaves + 2 * (size_t)(-1 - it);
  out[2 * (size_t)k] = src[0];
  out[2 * (size_t)k + 1] = src[1];
}

namespace {

namespace EH = tmed_evidence_host;

using tmed_votes_host::sig_full;
using tmed_votes_host::vote_sig;

// Every validator's key-set index of set vs into out; false for one past the key set.
bool set_key_indexes(const tmed_valset &vs, size_t nkeys, uint32_t *out) {
  bool ok = true;
  for (size_t v = 0; v < vs.n; v++) {
    out[v] = vs.keyset_index ? vs.keyset_index[v] : (uint32_t)v;
    ok = ok && out[v] < nkeys;
  }
  return ok;
}

// Device route (slot_batch.h slot_batch_device): records, steps and the sets' arrays in, the lookup
// and the prepare launch, pre-codes, states and validity bits out.
int run_group_device(tmed_ctx *c, const tmed_dup_request *reqs, const size_t *base, const SlotGroup &g, Keyset *ks,
                     uint8_t *codes) {
  const int rule = seam_rule(c);  // ctx->mu is held from the call's entry: one value for all its groups
  const size_t m = g.m, G = g.reqs.size();
  SetTable sets;
  for (const size_t q : g.reqs) sets.add(reqs[q].vals);
  const size_t kb = ks ? 4 : 32, n_addr = sets.n_vals;
  const size_t o_rec = 0, o_ev = align256(o_rec + 2 * m * kVoteRecBytes), o_step = align256(o_ev + m * kEvRecBytes),
               o_addr = align256(o_step + G * sizeof(EvStep)), o_pow = align256(o_addr + 20 * n_addr),
               o_setkey = align256(o_pow + 8 * n_addr), o_sig = align256(o_setkey + kb * n_addr),
               o_found = align256(o_sig + 2 * m * 64), o_pre = align256(o_found + 4 * m), o_state = align256(o_pre + m),
               o_valid = align256(o_state + 2 * m), o_key = align256(o_valid + 2 * m), o_slot = align256(o_key + 2 * m * kb),
               o_len = align256(o_slot + 2 * m * kVoteSlot), total = align256(o_len + 2 * m * 4);
  hipError_t e = c->stage.ensure(o_key, total);  // the keys, slots and lengths stay on the device
  if (e == hipSuccess && !c->vote_ev) e = hipEventCreate(&c->vote_ev);
  if (e == hipSuccess && !c->ev_lookup) e = hipEventCreate(&c->ev_lookup);
  if (e != hipSuccess) return map_err(e);
  uint8_t *h = c->stage.host(), *d = c->stage.dev();
  EvStep *steps = reinterpret_cast<EvStep *>(h + o_step);
  size_t at = 0;
  std::vector<size_t> start(G);
  for (size_t j = 0; j < G; j++) {
    const tmed_dup_request &rq = reqs[g.reqs[j]];
    EH::fill_step(rq, sets.at(rq.vals), steps[j]);
    start[j] = at;
    at += rq.ev->n;
  }
  bool keys_ok = true;
  for (const tmed_valset *vs : sets.sets) {
    if (!vs->n) continue;
    const uint64_t b = sets.at(vs);
    memcpy(h + o_addr + 20 * b, vs->addresses, 20 * vs->n);
    memcpy(h + o_pow + 8 * b, vs->powers, 8 * vs->n);
    if (ks) keys_ok = set_key_indexes(*vs, ks->n, reinterpret_cast<uint32_t *>(h + o_setkey) + b) && keys_ok;
    else memcpy(h + o_setkey + 32 * b, vs->pubkeys, 32 * vs->n);
  }
  if (!keys_ok) return TMED_EINVAL;  // a keyset_index past the key set
  host_for(G, pack_threads(2 * m), [&](size_t j) {
    const tmed_dup_request &rq = reqs[g.reqs[j]];
    const tmed_dup_evidence &ev = *rq.ev;
    for (size_t i = 0; i < ev.n; i++) {
      const size_t k = start[j] + i;
      VoteRec *vr = reinterpret_cast<VoteRec *>(h + o_rec + 2 * k * kVoteRecBytes);
      EH::fill_evidence(ev, i, (uint32_t)j, vr[0], vr[1], *reinterpret_cast<EvRec *>(h + o_ev + k * kEvRecBytes));
      vote_sig(ev.votes, 2 * i, h + o_sig + 64 * (2 * k));
      vote_sig(ev.votes, 2 * i + 1, h + o_sig + 64 * (2 * k + 1));
    }
  });
  const EvPrep p{reinterpret_cast<const int4 *>(d + o_rec), reinterpret_cast<const int4 *>(d + o_ev),
                 reinterpret_cast<const EvStep *>(d + o_step), d + o_addr, reinterpret_cast<const int64_t *>(d + o_pow),
                 ks ? reinterpret_cast<const uint32_t *>(d + o_setkey) : nullptr, ks ? nullptr : d + o_setkey,
                 ks ? ks->d_pub : nullptr, reinterpret_cast<uint32_t *>(d + o_found), d + o_key, d + o_slot,
                 reinterpret_cast<uint32_t *>(d + o_len), d + o_pre, d + o_state};
  const int rc = slot_batch_device(
      c, o_found, o_found, o_key,
      [&](hipStream_t s) {
        hipLaunchKernelGGL(evidence_lookup_kernel, dim3((uint32_t)m), dim3(kEvLanes), 0, s, p, (uint32_t)m);
        hipError_t el = hipGetLastError();
        if (el == hipSuccess) el = hipEventRecord(c->ev_lookup, s);
        if (el != hipSuccess) return el;
        hipLaunchKernelGGL(evidence_prepare_kernel, dim3((uint32_t)((m + kEvLanes - 1) / kEvLanes)), dim3(kEvLanes), 0, s, p,
                           (uint32_t)m);
        el = hipGetLastError();
        return el == hipSuccess ? hipEventRecord(c->vote_ev, s) : el;
      },
      SlotSigs{ks, d + o_key, d + o_sig, d + o_slot, p.lens, (uint32_t)(2 * m), d + o_valid, rule});
  if (rc != TMED_OK) return rc;
  float lms = 0.f, pms = 0.f;
  (void)hipEventElapsedTime(&lms, c->ev0, c->ev_lookup);
  (void)hipEventElapsedTime(&pms, c->ev_lookup, c->vote_ev);
  c->last_ev_ms[0] += lms;
  c->last_ev_ms[1] += pms;
  for (size_t j = 0; j < G; j++) {
    const tmed_votes &v = reqs[g.reqs[j]].ev->votes;
    uint8_t *out = codes + base[g.reqs[j]];
    for (size_t i = 0; i < reqs[g.reqs[j]].ev->n; i++) {
      const size_t k = start[j] + i;
      out[i] = ev_outcome(h[o_pre + k], h[o_state + 2 * k], h[o_valid + 2 * k] && sig_full(v, 2 * i), h[o_state + 2 * k + 1],
                          h[o_valid + 2 * k + 1] && sig_full(v, 2 * i + 1));
    }
  }
  return TMED_OK;
}

// Host route (a chain ID past kVoteChainMax; slot_batch.h slot_batch_host): lookup, checks and
// messages by the same source on the host, the messages packed behind each other.
int run_group_host(tmed_ctx *c, const tmed_dup_request *reqs, const size_t *base, const SlotGroup &g, Keyset *ks,
                   uint8_t *codes) {
  const size_t m = g.m;
  std::vector<EH::HostLane> lanes(m);
  std::vector<uint8_t> valid(2 * m);
  std::vector<std::pair<size_t, size_t>> src(m);  // evidence k: its request and its index there
  MsgPack mp;
  size_t k = 0;
  for (const size_t q : g.reqs) {
    const tmed_dup_evidence &ev = *reqs[q].ev;
    EH::request_lanes_host(reqs[q], lanes.data() + k);
    for (size_t i = 0; i < ev.n; i++, k++) {
      src[k] = {q, i};
      for (size_t w = 0; w < 2; w++) {
        if (!lanes[k].len[w]) {
          mp.skip();
          continue;
        }
        VoteRec r;
        tmed_votes_host::fill_rec(ev.votes, 2 * i + w, 0, 0, r);
        uint8_t *msg = mp.next(lanes[k].len[w]);
        if (!msg) return TMED_EINVAL;
        vote_free_write(r, (const uint8_t *)reqs[q].chain_id, reqs[q].chain_id_len, msg);
      }
    }
  }
  const int rc = slot_batch_host(
      c, ks, seam_rule(c), mp,
      [&](size_t j, uint8_t *out) {  // both votes' key: the found validator's (key 0, or zeros, for nobody)
        const tmed_valset &vs = *reqs[src[j / 2].first].vals;
        const uint32_t f = lanes[j / 2].found;
        if (ks) {
          const uint32_t key = f == kEvNone ? 0 : vs.keyset_index ? vs.keyset_index[f] : f;
          *reinterpret_cast<uint32_t *>(out) = key;
          return key < ks->n;
        }
        if (f == kEvNone) memset(out, 0, 32);
        else memcpy(out, vs.pubkeys + 32 * (size_t)f, 32);
        return true;
      },
      [&](size_t j, uint8_t *out) { vote_sig(reqs[src[j / 2].first].ev->votes, 2 * src[j / 2].second + j % 2, out); },
      valid.data());
  if (rc != TMED_OK) return rc;
  for (k = 0; k < m; k++) {
    const size_t q = src[k].first, i = src[k].second;
    const tmed_votes &v = reqs[q].ev->votes;
    codes[base[q] + i] = ev_outcome(lanes[k].pre, lanes[k].state[0], valid[2 * k] && sig_full(v, 2 * i), lanes[k].state[1],
                                    valid[2 * k + 1] && sig_full(v, 2 * i + 1));
  }
  return TMED_OK;
}

}  // namespace

int verify_dup_votes_locked(tmed_ctx *c, const tmed_dup_request *reqs, size_t n, uint8_t *codes) {
  c->last_ms = 0.f;
  c->last_ev_ms[0] = c->last_ev_ms[1] = 0.f;
  (void)hipSetDevice(c->device);
  return run_slot_groups(
      c, n, 0x3fffffffu, [&](size_t q) { return (size_t)reqs[q].ev->n; }, [&](size_t q) { return EH::device_route(reqs[q]); },
      [&](size_t q) { return reqs[q].vals->keyset; },
      [&](const SlotGroup &g, Keyset *ks, const size_t *base) {
        return g.device ? run_group_device(c, reqs, base, g, ks, codes) : run_group_host(c, reqs, base, g, ks, codes);
      });
}

namespace {

// The arguments of tmed_evidence_hashes once checked: K items in T lists, n_op opaque strings.
struct EvHashCall {
  const tmed_dup_evidence *ev;
  const int64_t *items;
  size_t K, T, n_op;
  const uint8_t *opaque;
  const uint64_t *opaque_off;
  std::vector<uint32_t> counts;  // items per list
  uint8_t *d_keep = nullptr;     // device memory that also receives the T roots (validate.hip)
};

// Evidences (host) -> hashes and roots (host; not yet zeroed where ev_ok / list_ok is 0).  ctx->mu held.
int evidence_hashes_locked(tmed_ctx *c, const EvHashCall &a, uint8_t *ev_hashes, uint8_t *roots) {
  const size_t n = a.ev->n, K = a.K, T = a.T;
  const MerkleLevels plan(a.counts);
  (void)hipSetDevice(c->device);
  hipStream_t s = c->stream;
  int rc = merkle_ensure_nodes(c, plan);
  if (rc != TMED_OK) return rc;
  const size_t o_rec = 0, o_ev = align256(o_rec + 2 * n * kVoteRecBytes), o_sig = align256(o_ev + n * kEvRecBytes),
               o_items = align256(o_sig + 2 * n * 64), o_hash = align256(o_items + 8 * K), o_roots = align256(o_hash + 32 * n),
               o_evleaf = align256(o_roots + 32 * T), o_opleaf = align256(o_evleaf + 32 * n),
               total = align256(o_opleaf + 32 * a.n_op);
  const size_t op_bytes = a.n_op ? a.opaque_off[a.n_op] - a.opaque_off[0] : 0;
  hipError_t e = c->stage.ensure(o_evleaf, total);  // the leaves stay on the device
  if (e == hipSuccess) e = c->d_msg.ensure(op_bytes + 16);
  if (e == hipSuccess) e = c->d_off.ensure((a.n_op + 1) * 8);
  if (e != hipSuccess) return map_err(e);
  uint8_t *h = c->stage.host(), *d = c->stage.dev();
  host_for(n, pack_threads(2 * n), [&](size_t i) {
    VoteRec *vr = reinterpret_cast<VoteRec *>(h + o_rec + 2 * i * kVoteRecBytes);
    EH::fill_evidence(*a.ev, i, 0, vr[0], vr[1], *reinterpret_cast<EvRec *>(h + o_ev + i * kEvRecBytes));
    vote_sig(a.ev->votes, 2 * i, h + o_sig + 64 * (2 * i));
    vote_sig(a.ev->votes, 2 * i + 1, h + o_sig + 64 * (2 * i + 1));
  });
  if (K) memcpy(h + o_items, a.items, 8 * K);
  std::vector<uint64_t> &off = c->merkle_off;  // the opaque strings' offsets from 0: a copy's source until the wait
  off.resize(a.n_op + 1);
  for (size_t j = 0; j <= a.n_op; j++) off[j] = a.n_op ? a.opaque_off[j] - a.opaque_off[0] : 0;
  e = hipMemcpyAsync(d, h, o_hash, hipMemcpyHostToDevice, s);  // one copy in, then the opaque strings
  if (e == hipSuccess && op_bytes)
    e = hipMemcpyAsync(c->d_msg.p, a.opaque + a.opaque_off[0], op_bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && a.n_op) e = hipMemcpyAsync(c->d_off.p, off.data(), (a.n_op + 1) * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipEventRecord(c->ev0, s);
  if (e == hipSuccess && n) {
    const EvHash p{reinterpret_cast<const int4 *>(d + o_rec), reinterpret_cast<const int4 *>(d + o_ev), d + o_sig,
                   reinterpret_cast<uint32_t *>(d + o_hash), reinterpret_cast<uint32_t *>(d + o_evleaf)};
    hipLaunchKernelGGL(evidence_hash_kernel, dim3((uint32_t)((n + kEvLanes - 1) / kEvLanes)), dim3(kEvLanes), 0, s, p,
                       (uint32_t)n);
    e = hipGetLastError();
  }
  if (e == hipSuccess && a.n_op)
    e = merkle_leaf_hashes((const uint8_t *)c->d_msg.p, (const uint64_t *)c->d_off.p, (uint32_t)a.n_op, d + o_opleaf, s);
  if (e == hipSuccess && K) {
    hipLaunchKernelGGL(evidence_gather_kernel, dim3((uint32_t)((K + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const int64_t *>(d + o_items), reinterpret_cast<const uint4 *>(d + o_evleaf),
                       reinterpret_cast<const uint4 *>(d + o_opleaf), (uint32_t)K, reinterpret_cast<uint4 *>(merkle_level0(c)));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(c->ev1, s);
  if (e == hipSuccess && T) e = merkle_build_levels(c, plan, s);
  if (e == hipSuccess && T) e = merkle_emit_roots(c, plan, d + o_roots, s);
  if (e == hipSuccess && T && a.d_keep) e = hipMemcpyAsync(a.d_keep, d + o_roots, 32 * T, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && n + T) e = hipMemcpyAsync(h + o_hash, d + o_hash, o_evleaf - o_hash, hipMemcpyDeviceToHost, s);
  rc = finish_call(c, s, e, &c->last_ms);
  if (rc != TMED_OK) return rc;
  if (ev_hashes && n) memcpy(ev_hashes, h + o_hash, 32 * n);
  if (T) memcpy(roots, h + o_roots, 32 * T);
  return TMED_OK;
}

}  // namespace

// tmed_evidence_hashes inside the guard.  held: the caller holds ctx->mu already and has collected the
// submitted windows (validate.hip).
int evidence_hashes_body(tmed_ctx *c, const tmed_dup_evidence *ev, const int64_t *items, const uint32_t *list_off,
                         size_t n_lists, const uint8_t *opaque, const uint64_t *opaque_off, uint8_t *ev_hashes,
                         uint8_t *roots, uint8_t *ev_ok, uint8_t *list_ok, bool held, uint8_t *d_keep) {
  if (!c || !ev || !tmed_evidence_host::evidence_arrays_ok(*ev)) return TMED_EINVAL;
  if (n_lists && (!list_off || !roots || list_off[0] != 0)) return TMED_EINVAL;
  if (n_lists > 0x7fffffffu) return TMED_EINVAL;
  {
    EvHashCall a{ev, items, n_lists ? list_off[n_lists] : 0, n_lists, 0, opaque, opaque_off, {}, d_keep};
    if (a.K && !items) return (int)TMED_EINVAL;
    a.counts.resize(n_lists);
    for (size_t l = 0; l < n_lists; l++) {
      if (list_off[l + 1] < list_off[l]) return (int)TMED_EINVAL;
      a.counts[l] = list_off[l + 1] - list_off[l];
    }
    for (size_t k = 0; k < a.K; k++) {
      if (items[k] >= 0 && (uint64_t)items[k] >= ev->n) return (int)TMED_EINVAL;
      if (items[k] < 0) {
        const uint64_t j = (uint64_t)(-1 - items[k]);
        if (j >= 0x7fffffffu) return (int)TMED_EINVAL;
        a.n_op = std::max<size_t>(a.n_op, (size_t)j + 1);
      }
    }
    if (a.n_op) {
      if (!opaque_off) return (int)TMED_EINVAL;
      for (size_t j = 0; j < a.n_op; j++)
        if (opaque_off[j + 1] < opaque_off[j] || opaque_off[j + 1] - opaque_off[j] > 0xffffffffu - 64) return (int)TMED_EINVAL;
      if (opaque_off[a.n_op] > opaque_off[0] && !opaque) return (int)TMED_EINVAL;
    }
    // what the struct can reproduce is a matter of lengths and timestamps: decided here, by the
    // function the kernel guards its encoder with
    std::vector<uint8_t> ok(ev->n);
    for (size_t i = 0; i < ev->n; i++) {
      VoteRec va, vb;
      EvRec r;
      tmed_evidence_host::fill_evidence(*ev, i, 0, va, vb, r);
      ok[i] = evidence_encodable(va, vb, r);
    }
    if (ev->n + n_lists == 0) return (int)TMED_OK;
    const int rc = held ? evidence_hashes_locked(c, a, ev_hashes, roots)
                        : locked(c, /*collect=*/true, [&] { return evidence_hashes_locked(c, a, ev_hashes, roots); });
    if (rc != TMED_OK) return rc;
    for (size_t i = 0; i < ev->n; i++) {
      if (ev_ok) ev_ok[i] = ok[i];
      if (ev_hashes && !ok[i]) memset(ev_hashes + 32 * i, 0, 32);
    }
    for (size_t l = 0; l < n_lists; l++) {
      bool good = true;
      for (uint32_t k = list_off[l]; k < list_off[l + 1]; k++) good = good && (items[k] < 0 || ok[(size_t)items[k]]);
      if (list_ok) list_ok[l] = good;
      if (!good) memset(roots + 32 * l, 0, 32);
    }
    return (int)TMED_OK;
  }
}

}  // namespace tmed

extern "C" {

int tmed_evidence_kernel_times(tmed_ctx *c, float ms[2]) {
  if (!c || !ms) return TMED_EINVAL;
  ms[0] = c->last_ev_ms[0];
  ms[1] = c->last_ev_ms[1];
  return TMED_OK;
}

int tmed_evidence_hashes(tmed_ctx *c, const tmed_dup_evidence *ev, const int64_t *items, const uint32_t *list_off,
                         size_t n_lists, const uint8_t *opaque, const uint64_t *opaque_off, uint8_t *ev_hashes,
                         uint8_t *roots, uint8_t *ev_ok, uint8_t *list_ok) {
  if (!c) return TMED_EINVAL;
  return guarded([&] {
    return tmed::evidence_hashes_body(c, ev, items, list_off, n_lists, opaque, opaque_off, ev_hashes, roots, ev_ok, list_ok,
                                      /*held=*/false, nullptr);
  });
}

}  // extern "C"
