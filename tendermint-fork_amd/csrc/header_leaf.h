// header_leaf.h — the 14 Merkle leaves of Header.Hash (types/block.go:440-475), one per lane, as
// SHA-256 message words; the packed header record the lanes read; the fold of the fixed tree.
//
// The leaves (cdcEncode wrappers, types/encoding_helper.go; oracle/merkle.py header_leaves is the
// checker), zero fields omitted as gogoproto does:
//    0 Version      tmversion.Consensus {1: block, 2: app}
//    1 ChainID      StringValue {1: value}
//    2 Height       Int64Value {1: value}
//    3 Time         Timestamp {1: seconds, 2: nanos}               (StdTimeMarshal)
//    4 LastBlockID  BlockID {1: hash, 2: PartSetHeader {1: total, 2: hash}}; the PartSetHeader is a
//                   non-nullable message: its tag and length are always there
//    5..13          BytesValue {1: value}: LastCommitHash .. ProposerAddress
//
// The packed record (kHdrRecBytes, written by header_pack): 14 slots of 128 bytes, slot l the two
// SHA-256 blocks of leaf l's stream 0x00 || leaf with the field's raw bytes already at their stream
// offsets and zeros everywhere else, then one 16-byte descriptor per slot:
//   Version   (block u64, app u64)          ChainID and the nine hash fields  (length, 0, 0, 0)
//   Height    (height u64, 0)               LastBlockID  (hash length, psh_total, psh hash length, 0)
//   Time      (seconds u64, nanos as int64)
// so a lane's leaf is nine 16-byte loads.  The lane writes the protobuf around the raw bytes (tags,
// lengths, varints), the 0x80 terminator and the bit length into the 32 message words it holds.
//
// Host and device compile this same source (tests/native/light_host.cpp runs it on the CPU).  Every
// array index is a compile-time constant after unrolling, so on the device the words stay in
// registers.
#pragma once
#include <string.h>

#include "../../include/tmed25519.h"
#include "sha256.h"

namespace tmed {

constexpr uint32_t kHdrLeaves = 14, kHdrSlotBytes = 128, kHdrMetaOff = kHdrLeaves * kHdrSlotBytes;
constexpr uint32_t kHdrRecBytes = 2048;
constexpr uint32_t kHdrBytesAt = 3;      // stream offset of a bytes field's value: 00 | tag | length
constexpr uint32_t kHdrMaxStream = 119;  // 0x00 || leaf: with 0x80 and the bit length, two blocks
constexpr uint32_t kHdrMaxChainID = 50;  // MaxChainIDLen, types/genesis.go:21
constexpr uint32_t kHdrMaxHash = 64;     // the kernel's limit on every hash field (3 + 64 <= 119)
static_assert(kHdrMetaOff + 16 * kHdrLeaves <= kHdrRecBytes, "descriptors inside the record");
static_assert(kHdrBytesAt + kHdrMaxHash <= kHdrMaxStream && kHdrBytesAt + kHdrMaxChainID <= kHdrMaxStream,
              "a bytes leaf fits two SHA-256 blocks");

// Stream byte `pos` of the message words w[0 .. N): a compare per word, static register indexes.
template <int N>
TMED_HD void hdr_put(uint32_t *w, uint32_t &pos, uint32_t byte) {
  const uint32_t t = pos >> 2, v = byte << (24 - 8 * (pos & 3u));
#pragma unroll
  for (int k = 0; k < N; k++) w[k] |= ((uint32_t)k == t) ? v : 0u;
  pos++;
}
template <int N>
TMED_HD void hdr_put_varint(uint32_t *w, uint32_t &pos, uint64_t v) {
#pragma unroll 1
  for (;;) {
    const uint32_t b = (uint32_t)v & 0x7fu;
    v >>= 7;
    hdr_put<N>(w, pos, b | (v ? 0x80u : 0u));
    if (!v) break;
  }
}

TMED_HD uint32_t hdr_varint_len(uint32_t v) {
  uint32_t n = 0;
  for (; v; v >>= 7) n++;
  return n;
}

// Leaf `slot` (< 14): w holds the slot's 128 bytes as 32 big-endian words on entry and the padded
// SHA-256 message of 0x00 || leaf on return (one block when the returned stream length is <= 55,
// else two); (m0 .. m3) is the slot's descriptor.
TMED_HD uint32_t header_leaf_words(uint32_t w[32], uint32_t slot, uint32_t m0, uint32_t m1, uint32_t m2, uint32_t m3) {
  uint32_t pos = 1;  // stream byte 0 is the leaf prefix 0x00
  if (slot == 0 || slot == 2 || slot == 3) {
    // {1: a, 2: b}: at most 1 + 11 + 11 bytes, then the terminator: words 0 .. 5
    const uint64_t a = (uint64_t)m0 | ((uint64_t)m1 << 32), b = (uint64_t)m2 | ((uint64_t)m3 << 32);
    if (a) { hdr_put<6>(w, pos, 0x08); hdr_put_varint<6>(w, pos, a); }
    if (b) { hdr_put<6>(w, pos, 0x10); hdr_put_varint<6>(w, pos, b); }
  } else if (slot == 4) {
    // the bytes written here end before 1 + 2 + 64 + 2 + 6 + 2 = 77: words 0 .. 19
    const uint32_t hl = m0, tot = m1, pl = m2;
    if (hl) { hdr_put<20>(w, pos, 0x0a); hdr_put<20>(w, pos, hl); pos += hl; }
    hdr_put<20>(w, pos, 0x12);
    hdr_put<20>(w, pos, (tot ? 1 + hdr_varint_len(tot) : 0) + (pl ? 2 + pl : 0));
    if (tot) { hdr_put<20>(w, pos, 0x08); hdr_put_varint<20>(w, pos, tot); }
    if (pl) { hdr_put<20>(w, pos, 0x12); hdr_put<20>(w, pos, pl); pos += pl; }
  } else if (m0) {
    w[0] |= 0x000a0000u | (m0 << 8);
    pos = kHdrBytesAt + m0;
  }
  const uint32_t len = pos;  // <= kHdrMaxStream (header_fused_ok)
  hdr_put<30>(w, pos, 0x80);
  if (len > 55) w[31] = len * 8;
  else w[15] = len * 8;
  return len;
}

// The fixed tree 14 -> 7 -> 4 -> 2 -> 1 folded over 16 lanes: at step s = 1, 2, 4, 8 the node at
// lane l takes the node at lane l + s as its right child iff this holds; a node without one (lane
// 12 at s = 2) is the odd last node of its level and is promoted unchanged, as merkle_level_kernel
// and HashFromByteSlicesIterative (crypto/merkle/tree.go:57-101) do.
TMED_HD bool header_fold_takes(uint32_t l, uint32_t s) { return (l & (2 * s - 1)) == 0 && l + s < kHdrLeaves; }

// Stream length (0x00 prefix included) of the LastBlockID leaf; *psh_at: where the PartSetHeader
// hash's bytes lie in it.
inline uint32_t lbid_stream_len(const tmed_block_id &b, uint32_t *psh_at) {
  const uint32_t at = 1 + (b.hash_len ? 2 + b.hash_len : 0) + 2 + (b.psh_total ? 1 + hdr_varint_len(b.psh_total) : 0) + 2;
  if (psh_at) *psh_at = at;
  return b.psh_hash_len ? at + b.psh_hash_len : at - 2;
}

// Every leaf of h fits two SHA-256 blocks and every length one varint byte: the kernel's limits
// (include/tmed25519.h, tmed_header_hashes).
inline bool header_fused_ok(const tmed_header &h) {
  if (h.chain_id_len > kHdrMaxChainID) return false;
  for (int k = 0; k < 9; k++)
    if (h.hash_lens[k] > kHdrMaxHash) return false;
  const tmed_block_id &b = h.last_block_id;
  return b.hash_len <= kHdrMaxHash && b.psh_hash_len <= kHdrMaxHash && lbid_stream_len(b, nullptr) <= kHdrMaxStream;
}

// The packed record of header h (header_fused_ok).
inline void header_pack(const tmed_header &h, uint8_t *rec) {
  memset(rec, 0, kHdrRecBytes);
  uint8_t *meta = rec + kHdrMetaOff;
  auto set64 = [&](int slot, int at, uint64_t v) { memcpy(meta + 16 * slot + 8 * at, &v, 8); };
  auto set32 = [&](int slot, int at, uint32_t v) { memcpy(meta + 16 * slot + 4 * at, &v, 4); };
  auto bytes = [&](int slot, const void *p, uint32_t n) {
    set32(slot, 0, n);
    if (n) memcpy(rec + slot * kHdrSlotBytes + kHdrBytesAt, p, n);
  };
  set64(0, 0, h.version_block);
  set64(0, 1, h.version_app);
  bytes(1, h.chain_id, h.chain_id_len);
  set64(2, 0, (uint64_t)h.height);
  set64(3, 0, (uint64_t)h.time_seconds);
  set64(3, 1, (uint64_t)(int64_t)h.time_nanos);
  const tmed_block_id &b = h.last_block_id;
  uint32_t psh_at;
  (void)lbid_stream_len(b, &psh_at);
  bytes(4, b.hash, b.hash_len);
  set32(4, 1, b.psh_total);
  set32(4, 2, b.psh_hash_len);
  if (b.psh_hash_len) memcpy(rec + 4 * kHdrSlotBytes + psh_at, b.psh_hash, b.psh_hash_len);
  for (int k = 0; k < 9; k++) bytes(5 + k, h.hashes[k], h.hash_lens[k]);
}

}  // namespace tmed
