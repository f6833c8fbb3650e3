// slot_batch.h — the frame of the free-standing checks that verify signatures over message slots
// (host side of the HIP units, on top of call_frame.h): tmed_verify_votes (votes.hip) and
// tmed_verify_duplicate_votes (evidence.hip).  Such a call groups its requests by (route, key set)
// (run_slot_groups).  A device-route group stages records and the sets' arrays (SetTable: each
// distinct set once) into tmed_ctx::stage, has a prepare kernel write sign-bytes into kVoteSlot-byte
// slots and hands the slots to the unchanged verify launchers in msg_slots mode (slot_batch_device).
// A host-route group (a chain ID the slots cannot hold) packs its messages on the host (MsgPack) and
// goes through the raw host batch in offset mode (slot_batch_host).  verify_sigs is the one place
// that picks the keyed or the generic launchers.  The layouts, the records and the mapping of the
// results to codes are each call's own.
#pragma once
#include <map>
#include <unordered_map>
#include <utility>
#include <vector>

#include "call_frame.h"

namespace tmed {

// n signatures over device-resident tuples on stream s, inside a scratch pair: ks's cached keys (keys:
// n key-set indexes) or the generic route (keys: n x 32 bytes).  lens_or_off: the slots' message
// lengths (msg_slots) or the n + 1 offsets of packed messages.
inline hipError_t verify_sigs(tmed_ctx *c, Keyset *ks, const uint8_t *keys, const uint8_t *sigs, const uint8_t *msgs,
                              const uint32_t *lens_or_off, uint32_t n, uint8_t *out, hipStream_t s, bool msg_slots,
                              int rule) {
  return ks ? keyset_verify_batch(c, *ks, reinterpret_cast<const uint32_t *>(keys), sigs, msgs, lens_or_off, n, out, s,
                                  msg_slots, rule)
            : generic_verify(c, keys, sigs, msgs, lens_or_off, n, out, s, msg_slots, nullptr, nullptr, rule);
}

// One group of a call: the requests that share a route and a key set, m items in all.
struct SlotGroup {
  bool device;
  std::vector<size_t> reqs;
  size_t m = 0;
};

// The n requests of a call by group, device groups first, each in key-set order: run(group, its key
// set or null, base) -> TMED_*, base[q] the items before request q.  count(q), device(q), keyset(q):
// request q's items, route and key-set handle; a request without items joins no group.  limit: the
// most items a group may hold.  ctx->mu held.
template <class Count, class Route, class Handle, class Run>
int run_slot_groups(tmed_ctx *c, size_t n, size_t limit, Count &&count, Route &&device, Handle &&keyset, Run &&run) {
  std::vector<size_t> base(n + 1, 0);
  std::map<std::pair<bool, uint64_t>, SlotGroup> groups;
  for (size_t q = 0; q < n; q++) {
    base[q + 1] = base[q] + count(q);
    if (count(q) == 0) continue;
    const bool dev = device(q);
    SlotGroup &g = groups[{!dev, keyset(q)}];
    g.device = dev;
    g.reqs.push_back(q);
    g.m += count(q);
  }
  for (const auto &kv : groups) {
    if (kv.second.m > limit) return TMED_EINVAL;
    Keyset *ks = nullptr;
    if (kv.first.second) {
      auto it = c->keysets.find(kv.first.second);
      if (it == c->keysets.end()) return TMED_ENOKEYSET;
      ks = &it->second;
    }
    const int rc = run(kv.second, ks, base.data());
    if (rc != TMED_OK) return rc;
  }
  return TMED_OK;
}

// Each distinct validator set of a group once: its base in the group's packed per-validator arrays.
struct SetTable {
  std::unordered_map<const tmed_valset *, uint64_t> base;
  std::vector<const tmed_valset *> sets;  // in order of their bases
  size_t n_vals = 0;                      // validators in all
  void add(const tmed_valset *vs) {
    if (base.emplace(vs, n_vals).second) {
      sets.push_back(vs);
      n_vals += vs->n;
    }
  }
  uint64_t at(const tmed_valset *vs) const { return base.find(vs)->second; }
};

// The signatures of a device-route group as verify_sigs takes them (device pointers, msg_slots mode).
struct SlotSigs {
  Keyset *ks;
  const uint8_t *keys, *sigs, *slots;
  const uint32_t *lens;
  uint32_t n;
  uint8_t *valid;
  int rule;
};

// The device route of a group whose inputs are packed in the staging arena: one copy in ([0, in_bytes)
// of tmed_ctx::stage), scratch_acquire, ev0, prepare(stream) -> hipError_t (the prepare launches and
// the events between them), the verify launchers over the slots, ev1, scratch_release (on a failure
// too), one copy out ([out_lo, out_hi)), finish_call.  The time between ev0 and ev1 joins c->last_ms.
template <class Prepare>
int slot_batch_device(tmed_ctx *c, size_t in_bytes, size_t out_lo, size_t out_hi, Prepare &&prepare, const SlotSigs &v) {
  uint8_t *h = c->stage.host(), *d = c->stage.dev();
  hipStream_t s = c->stream;
  hipError_t e = hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = scratch_acquire(c, s);
  const bool acquired = e == hipSuccess;
  if (e == hipSuccess) e = hipEventRecord(c->ev0, s);
  if (e == hipSuccess) e = prepare(s);
  if (e == hipSuccess) e = verify_sigs(c, v.ks, v.keys, v.sigs, v.slots, v.lens, v.n, v.valid, s, /*msg_slots=*/true, v.rule);
  if (e == hipSuccess) e = hipEventRecord(c->ev1, s);
  if (acquired) {
    const hipError_t er = scratch_release(c, s);
    if (e == hipSuccess) e = er;
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h + out_lo, d + out_lo, out_hi - out_lo, hipMemcpyDeviceToHost, s);
  float ms = 0.f;
  const int rc = finish_call(c, s, e, &ms);
  if (rc == TMED_OK) c->last_ms += ms;
  return rc;
}

// The messages of a host-route group, packed behind each other: off[k] .. off[k + 1] is message k.
struct MsgPack {
  std::vector<uint8_t> msgs;
  std::vector<uint32_t> off{0};
  void skip() { off.push_back(off.back()); }  // an empty message: no signature is to be checked
  // Room for the next message (len > 0); null when the offsets would pass 32 bits.
  uint8_t *next(size_t len) {
    const size_t pos = msgs.size();
    if (pos + len > 0xffffffffu) return nullptr;
    msgs.resize(pos + len);
    off.push_back((uint32_t)(pos + len));
    return msgs.data() + pos;
  }
  size_t n() const { return off.size() - 1; }
};

// The host route of a group once its messages are packed: the raw host batch (raw_stage, raw_run)
// with the verify launchers in offset mode.  key(k, out) writes signature k's key (4 bytes of key-set
// index with ks, else 32) and returns false for an index past the key set (TMED_EINVAL); sig(k, out)
// its 64 bytes.  valid: one byte a signature.  The kernels' time joins c->last_ms.
template <class KeyFill, class SigFill>
int slot_batch_host(tmed_ctx *c, Keyset *ks, int rule, const MsgPack &mp, KeyFill &&key, SigFill &&sig, uint8_t *valid) {
  const size_t n = mp.n(), kb = ks ? 4 : 32, bytes = mp.msgs.size();
  RawStage st;
  int rc = raw_stage(c, kb, n, bytes, st);
  if (rc != TMED_OK) return rc;
  for (size_t k = 0; k < n; k++) {
    if (!key(k, st.keys + kb * k)) return TMED_EINVAL;
    sig(k, st.sigs + 64 * k);
  }
  if (bytes) memcpy(st.msgs, mp.msgs.data(), bytes);
  memcpy(st.off, mp.off.data(), (n + 1) * 4);
  rc = raw_run(c, st, /*timed=*/true,
               [&](const uint8_t *d_key, const uint8_t *d_sig, const uint8_t *d_msg, const uint32_t *d_off, uint32_t m,
                   uint8_t *d_out, hipStream_t s) {
                 return map_err(verify_sigs(c, ks, d_key, d_sig, d_msg, d_off, m, d_out, s, /*msg_slots=*/false, rule));
               },
               valid, nullptr);
  if (rc == TMED_OK) c->last_ms += st.ms;
  return rc;
}

}  // namespace tmed
