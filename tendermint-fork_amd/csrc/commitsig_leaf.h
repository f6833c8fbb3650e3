// commitsig_leaf.h — the Merkle leaf of one CommitSig, assembled as SHA-256 message words.
//
// Commit.Hash (types/block.go:894-912) hashes cs.ToProto().Marshal() of every CommitSig.  The
// encoding below is the reference's rule as read from the generated marshaller
// (proto/tendermint/types/types.pb.go:1563-1596, gogoproto StdTime), fields in ascending order:
//   08 varint(flag)          only if flag != 0 (a byte: values >= 128 take a two-byte varint)
//   12 len addr              only if len(addr) > 0
//   1a len ts                ALWAYS (a non-nullable message), ts = [08 varint(uint64(seconds))]
//                            if seconds != 0, then [10 varint(nanos)] if nanos != 0
//   22 len sig               only if len(sig) > 0
// The reference holds no Commit.Hash known answer; the rule is pinned by its size bound only:
// the longest leaf is MaxCommitSigBytes = 109 (types/block.go:591, types/block_test.go:260-274).
//
// Host and device compile this same source (tests/native/blockhash_host.cpp runs it on the CPU).
// Fields are appended into the word stream with shifts: every array index below is a
// compile-time constant after unrolling, so on the device the stream stays in registers.
#pragma once
#include <string.h>

#include "sha256.h"

namespace tmed {

constexpr uint32_t kCommitSigMaxLeaf = 109;  // MaxCommitSigBytes
constexpr int kCommitSigWords = 28;          // 0x00 || leaf || 0x80 is at most 111 bytes
// The kernel runs one or two sha256_compress calls and no loop: prefix + leaf + 0x80 + the 8-byte
// bit length never exceed two 64-byte blocks (one block up to a 54-byte leaf, two from 55).
static_assert(1 + kCommitSigMaxLeaf + 1 + 8 <= 128, "a CommitSig leaf must fit two SHA-256 blocks");
static_assert(1 + kCommitSigMaxLeaf + 1 <= 4 * kCommitSigWords, "stream words hold prefix, leaf and pad byte");

// d |= src placed at byte offset off.  src: NS big-endian words, left-aligned, zero past its last
// byte.  The caller guarantees off / 4 < 2^QBITS and that the piece ends inside d.
template <int ND, int NS, int QBITS>
TMED_HD void words_or_at(uint32_t (&d)[ND], const uint32_t (&src)[NS], uint32_t off) {
  const uint32_t r = 8 * (off & 3), q = off >> 2;
  uint32_t t[ND];
#pragma unroll
  for (int k = 0; k < ND; k++) {  // byte part of the shift: one funnel shift per word
    const uint32_t hi = (k >= 1 && k - 1 < NS) ? src[k - 1] : 0u;
    const uint32_t lo = k < NS ? src[k] : 0u;
    t[k] = (uint32_t)((((uint64_t)hi << 32) | lo) >> r);
  }
#pragma unroll
  for (int b = QBITS - 1; b >= 0; b--) {  // word part: a barrel shifter of selects
    const int step = 1 << b;
    const bool on = (q & (uint32_t)step) != 0;
#pragma unroll
    for (int k = ND - 1; k >= 0; k--) {
      const uint32_t moved = k >= step ? t[k - step] : 0u;
      t[k] = on ? moved : t[k];
    }
  }
#pragma unroll
  for (int k = 0; k < ND; k++) d[k] |= t[k];
}

// o = tag byte, then varint(v) (at most 10 bytes); returns the byte count.
TMED_HD uint32_t tagged_varint(uint32_t (&o)[3], uint32_t tag, uint64_t v) {
  uint32_t n = 1;
#pragma unroll
  for (int k = 1; k < 10; k++)
    if (v >> (7 * k)) n = (uint32_t)k + 1;
  o[0] = tag << 24;
  o[1] = o[2] = 0;
#pragma unroll
  for (int k = 0; k < 10; k++) {
    uint32_t byte = (uint32_t)(v >> (7 * k)) & 0x7fu;
    if ((uint32_t)k + 1 < n) byte |= 0x80u;
    if ((uint32_t)k >= n) byte = 0;
    const int pos = k + 1;
    o[pos >> 2] |= byte << (24 - 8 * (pos & 3));
  }
  return 1 + n;
}

// The SHA-256 input of leafHash(CommitSig): w[0..15] is the first block and w[16..31] the second
// (used only when the returned leaf length is >= 55), as big-endian words with the 0x00 leaf
// prefix, the 0x80 pad byte and the bit length in place.  Returns the leaf length (2..109).
//   flag      BlockIDFlag byte
//   addr_len  0 or 20; addr_row (20 bytes, dword-aligned on the device) is read only when 20
//   seconds   in [-62135596800, 253402300800), nanos in [0, 10^9) (else the reference's Marshal
//             fails: such signatures never reach this function)
//   sig_len   0..64; sig_row (64 bytes, 16-byte aligned on the device) is read when > 0 and only
//             its first sig_len bytes are used
TMED_HD uint32_t commitsig_leaf_words(uint32_t w[32], uint32_t flag, uint32_t addr_len, int64_t seconds,
                                      int32_t nanos, uint32_t sig_len, const uint8_t *addr_row,
                                      const uint8_t *sig_row) {
  uint32_t s[kCommitSigWords];
#pragma unroll
  for (int k = 0; k < kCommitSigWords; k++) s[k] = 0;
  uint32_t pos = 1;  // stream byte 0 is the leaf prefix 0x00
  flag &= 0xffu;
  if (flag != 0) {   // 08 varint(flag): for flag >= 128 the low group already carries bit 7
    s[0] = (0x08u << 16) | (flag << 8) | (flag >> 7);
    pos = flag < 0x80u ? 3 : 4;
  }
  if (addr_len == 20) {  // 12 14 addr
    uint32_t a[5], b[6];
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t *ap = reinterpret_cast<const uint32_t *>(addr_row);
#pragma unroll
    for (int k = 0; k < 5; k++) a[k] = bswap32(ap[k]);
#else
    for (int k = 0; k < 5; k++) {
      uint32_t v;
      memcpy(&v, addr_row + 4 * k, 4);
      a[k] = bswap32(v);
    }
#endif
    b[0] = 0x12140000u | (a[0] >> 16);
#pragma unroll
    for (int k = 1; k < 5; k++) b[k] = (a[k - 1] << 16) | (a[k] >> 16);
    b[5] = a[4] << 16;
    words_or_at<kCommitSigWords, 6, 1>(s, b, pos);  // pos <= 4
    pos += 22;
  }
  {  // 1a len [08 varint(seconds)] [10 varint(nanos)]
    uint32_t p1[3] = {0, 0, 0}, p2[3] = {0, 0, 0}, c[5];
    const uint32_t n1 = seconds != 0 ? tagged_varint(p1, 0x08, (uint64_t)seconds) : 0;  // <= 11
    const uint32_t n2 = nanos != 0 ? tagged_varint(p2, 0x10, (uint64_t)(uint32_t)nanos) : 0;  // <= 6
    c[0] = 0x1a000000u | ((n1 + n2) << 16) | (p1[0] >> 16);
    c[1] = (p1[0] << 16) | (p1[1] >> 16);
    c[2] = (p1[1] << 16) | (p1[2] >> 16);
    c[3] = p1[2] << 16;
    c[4] = 0;
    const uint32_t p2w[2] = {p2[0], p2[1]};
    words_or_at<5, 2, 2>(c, p2w, 2 + n1);           // offset <= 13
    words_or_at<kCommitSigWords, 5, 3>(s, c, pos);  // pos <= 26
    pos += 2 + n1 + n2;
  }
  if (sig_len != 0) {  // 22 len sig
    uint32_t g[16], d[17];
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 *sp = reinterpret_cast<const uint4 *>(sig_row);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint4 v = sp[k];
      g[4 * k] = bswap32(v.x); g[4 * k + 1] = bswap32(v.y); g[4 * k + 2] = bswap32(v.z); g[4 * k + 3] = bswap32(v.w);
    }
#else
    for (int k = 0; k < 16; k++) {
      uint32_t v;
      memcpy(&v, sig_row + 4 * k, 4);
      g[k] = bswap32(v);
    }
#endif
#pragma unroll
    for (int k = 0; k < 16; k++) {  // bytes of the slot past sig_len are not part of the signature
      const int32_t nv = (int32_t)sig_len - 4 * k;
      if (nv <= 0) g[k] = 0;
      else if (nv < 4) g[k] &= ~(0xffffffffu >> (8 * nv));
    }
    d[0] = 0x22000000u | (sig_len << 16) | (g[0] >> 16);
#pragma unroll
    for (int k = 1; k < 16; k++) d[k] = (g[k - 1] << 16) | (g[k] >> 16);
    d[16] = g[15] << 16;
    words_or_at<kCommitSigWords, 17, 4>(s, d, pos);  // pos <= 45
    pos += 2 + sig_len;
  }
#pragma unroll
  for (int k = 0; k < kCommitSigWords; k++)  // the pad byte, at stream byte pos <= 110
    if ((uint32_t)k == (pos >> 2)) s[k] |= 0x80000000u >> (8 * (pos & 3));
#pragma unroll
  for (int k = 0; k < kCommitSigWords; k++) w[k] = s[k];
  w[28] = w[29] = w[30] = w[31] = 0;
  if (pos <= 55) w[15] = pos * 8;  // one block: bytes 56..63 hold the bit length
  else w[31] = pos * 8;
  return pos - 1;
}

}  // namespace tmed
