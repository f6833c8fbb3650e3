// vote_wire.h — the bytes a validator signs, every rule once: VoteSignBytes(chainID, vote) =
// protoio.MarshalDelimited(CanonicalizeVote(chainID, vote)) (types/vote.go:93-101).  Plain C++ that
// host and device compile alike (TMED_HD; g++ needs no HIP header for it): the commit encoder
// (signbytes.h), the device splice (votes_dev.h) and the free-standing votes (vote_free.h) are
// composed from it.
//
//   uvarint(len(body))                      libs/protoio/writer.go:54-100
//   08 uvarint(uint64(int64(type)))         only if type != 0 (canonical.pb.go:517-579; an int32: a
//                                           negative type is ten bytes)
//   11 le64(height)                         sfixed64, only if height != 0
//   19 le64(int64(round))                   sfixed64, only if round != 0 (canonical.go:56-65)
//   22 len {[0a 20 hash] 12 len {[08 uvarint(total)] [12 20 psh_hash]}}
//                                           only if the BlockID is not zero: hash, total and part-set
//                                           hash not all empty / 0 (canonical.go:18-34; :370-428).  The
//                                           inner PartSetHeader field is always there (non-nullable);
//                                           an incomplete BlockID encodes as Go encodes it
//   2a len {[08 uvarint(seconds)] [10 uvarint(int64(nanos))]}   ALWAYS (gogoproto StdTimeMarshalTo;
//                                           zero seconds / nanos omitted)
//   32 len chain_id                         only if len(chain_id) > 0
// A hash is 32 bytes or absent: any other length makes CanonicalizeBlockID panic (ValidateHash), and
// the callers encode nothing then.
#pragma once
#include <stdint.h>

#ifndef TMED_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TMED_HD __host__ __device__ __forceinline__
#else
#define TMED_HD static inline
#endif
#endif

namespace tmed {

// ---- primitives ------------------------------------------------------------------------------
TMED_HD uint32_t uvarint_len(uint64_t v) {
  uint32_t n = 1;
  while (v >= 0x80) { v >>= 7; n++; }
  return n;
}
// Every writer: bytes into o from position p on, the new position back.
TMED_HD uint32_t put_uvarint(uint8_t *o, uint32_t p, uint64_t v) {
  while (v >= 0x80) { o[p++] = (uint8_t)(v | 0x80); v >>= 7; }
  o[p++] = (uint8_t)v;
  return p;
}
TMED_HD uint32_t put_le64(uint8_t *o, uint32_t p, uint64_t v) {
  for (int i = 0; i < 8; i++) o[p++] = (uint8_t)(v >> (8 * i));
  return p;
}
TMED_HD uint32_t put_bytes(uint8_t *o, uint32_t p, const uint8_t *b, uint32_t n) {
  for (uint32_t j = 0; j < n; j++) o[p++] = b[j];
  return p;
}

// google.protobuf.Timestamp's range (gogoproto validateTimestamp, which StdTimeMarshal runs): outside
// it the reference's marshalling fails (VoteSignBytes and Commit.Hash panic), and it is the range in
// which Time.Add of an int64-nanosecond duration cannot overflow.  A Go time.Time holds no nanos
// outside [0, 1e9).
constexpr int64_t kMinSeconds = -62135596800ll;  // 0001-01-01T00:00:00Z, Go's zero time.Time{}.Unix()
constexpr int64_t kMaxSeconds = 253402300800ll;  // 10000-01-01T00:00:00Z (exclusive)
TMED_HD bool timestamp_encodable(int64_t sec, int32_t nanos) {
  return sec >= kMinSeconds && sec < kMaxSeconds && nanos >= 0 && nanos < 1000000000;
}

// ---- fields ----------------------------------------------------------------------------------
// The longest of each: type 1 + 10, height 1 + 8, round 1 + 8; BlockID 2 + {hash 2 + 32, part-set
// header 2 + {total 1 + 5 (a uint32), hash 2 + 32}}; timestamp 2 + {1 + 10, 1 + 10} (any int64 seconds
// and any int32 nanos: a negative one is ten bytes).
constexpr uint32_t kVoteHeadMax = 11 + 9 + 9;
constexpr uint32_t kBlockIdFieldMax = 2 + 34 + 2 + 6 + 34;
constexpr uint32_t kTimestampFieldMax = 2 + 11 + 11;
static_assert(kBlockIdFieldMax == 78 && kTimestampFieldMax == 24, "bodies below 128 bytes: one length byte each");

// 08 type, 11 height, 19 round.
TMED_HD uint32_t vote_head_len(int32_t type, int64_t height, int32_t round) {
  return (type ? 1 + uvarint_len((uint64_t)(int64_t)type) : 0) + (height ? 9 : 0) + (round ? 9 : 0);
}
TMED_HD uint32_t put_vote_head(uint8_t *o, uint32_t p, int32_t type, int64_t height, int32_t round) {
  if (type) { o[p++] = 0x08; p = put_uvarint(o, p, (uint64_t)(int64_t)type); }
  if (height) { o[p++] = 0x11; p = put_le64(o, p, (uint64_t)height); }
  if (round) { o[p++] = 0x19; p = put_le64(o, p, (uint64_t)(int64_t)round); }
  return p;
}

// The complete 22 field; nothing for the zero BlockID.  hash / psh: 32 bytes, or nullptr for an empty
// one.  Each of the two length bytes is set once its body stands.
TMED_HD uint32_t block_id_field_len(bool hash, uint32_t psh_total, bool psh) {
  if (!hash && !psh_total && !psh) return 0;
  return 2 + (hash ? 34 : 0) + 2 + (psh_total ? 1 + uvarint_len(psh_total) : 0) + (psh ? 34 : 0);
}
TMED_HD uint32_t put_block_id_field(uint8_t *o, uint32_t p, const uint8_t *hash, uint32_t psh_total,
                                    const uint8_t *psh) {
  if (!hash && !psh_total && !psh) return p;
  const uint32_t bid = p;
  o[p++] = 0x22; p++;
  if (hash) { o[p++] = 0x0a; o[p++] = 32; p = put_bytes(o, p, hash, 32); }
  const uint32_t part = p;
  o[p++] = 0x12; p++;
  if (psh_total) { o[p++] = 0x08; p = put_uvarint(o, p, psh_total); }
  if (psh) { o[p++] = 0x12; o[p++] = 32; p = put_bytes(o, p, psh, 32); }
  o[part + 1] = (uint8_t)(p - part - 2);
  o[bid + 1] = (uint8_t)(p - bid - 2);
  return p;
}

// The complete 32 field; nothing for an empty chain ID.
TMED_HD uint32_t chain_id_field_len(uint32_t n) { return n ? 1 + uvarint_len(n) + n : 0; }
TMED_HD uint32_t put_chain_id_field(uint8_t *o, uint32_t p, const uint8_t *chain, uint32_t n) {
  if (!n) return p;
  o[p++] = 0x32;
  p = put_uvarint(o, p, n);
  return put_bytes(o, p, chain, n);
}

// The 2a field, always there.
TMED_HD uint32_t timestamp_field_len(int64_t sec, int32_t nanos) {
  const uint64_t s = (uint64_t)sec, ns = (uint64_t)(int64_t)nanos;
  return 2 + (s ? 1 + uvarint_len(s) : 0) + (ns ? 1 + uvarint_len(ns) : 0);
}
TMED_HD uint32_t put_timestamp_field(uint8_t *o, uint32_t p, int64_t sec, int32_t nanos) {
  const uint64_t s = (uint64_t)sec, ns = (uint64_t)(int64_t)nanos;
  const uint32_t at = p;
  o[p++] = 0x2a; p++;
  if (s) { o[p++] = 0x08; p = put_uvarint(o, p, s); }
  if (ns) { o[p++] = 0x10; p = put_uvarint(o, p, ns); }
  o[at + 1] = (uint8_t)(p - at - 2);
  return p;
}

// ---- the message -----------------------------------------------------------------------------
// uvarint(body) || pre || [BlockID field] || timestamp field || chain-ID field: the body and the
// message from the lengths of the four parts (bid_len 0: a vote for the zero BlockID; ts_len:
// timestamp_field_len, or kTimestampFieldMax for the longest vote of a template).
TMED_HD uint32_t vote_body_len(uint32_t pre_len, uint32_t bid_len, uint32_t ts_len, uint32_t cid_len) {
  return pre_len + bid_len + ts_len + cid_len;
}
TMED_HD uint32_t vote_msg_len(uint32_t body) { return uvarint_len(body) + body; }
// The message into o from three encoded ranges (the head, the BlockID field, the chain-ID field) and
// the vote's time; returns its length (vote_msg_len of the body with timestamp_field_len(sec, nanos)).
TMED_HD uint32_t vote_splice(uint8_t *__restrict__ o, const uint8_t *pre, uint32_t pre_len, const uint8_t *bid,
                             uint32_t bid_len, int64_t sec, int32_t nanos, const uint8_t *cid, uint32_t cid_len) {
  uint32_t p = put_uvarint(o, 0, vote_body_len(pre_len, bid_len, timestamp_field_len(sec, nanos), cid_len));
  p = put_bytes(o, p, pre, pre_len);
  p = put_bytes(o, p, bid, bid_len);
  p = put_timestamp_field(o, p, sec, nanos);
  return put_bytes(o, p, cid, cid_len);
}

}  // namespace tmed
