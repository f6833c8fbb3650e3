// vote_wire_host.cpp — TEST-ONLY stand-alone host program: the device splice on the CPU.  For each
// case it builds the commit's template record (csrc/signbytes.hip VoteEncoder::device_template), runs
// what the device assemblers run on that record (csrc/signbytes.h vote_from_template: vote_wire.h's
// vote_splice), and requires byte equality with VoteEncoder::write and with vote_free_write of the
// equivalent precommit (csrc/vote_free.h).  tests/test_votes_host.py builds it plain and with
// -fsanitize=address,undefined, runs it as a plain executable and compares the printed messages with
// oracle.signbytes:
//   g++ -std=c++17 -fsanitize=address,undefined -I tendermint-fork_amd/csrc vote_wire_host.cpp \
//       -x c++ tendermint-fork_amd/csrc/signbytes.hip
//   vote_wire_host            one line of hex per case, then "wire-ok <cases> <longest>"
// Every buffer has exactly the size its writer is promised, so the sanitizer sees a byte past it.
// The cases, in the order of the loops of run() (tests/test_votes_host.py wire_cases restates it):
// the product of BlockIDs, heights, rounds, chain-ID lengths, seconds, nanos and flags; bodies of 127
// and 128 bytes; the template-fit boundary.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "signbytes.h"
#include "vote_free.h"

#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      fprintf(stderr, "vote_wire_host.cpp:%d: %s\n", __LINE__, #c); \
      return 1;                                                     \
    }                                                               \
  } while (0)

struct Bid {
  bool hash;
  uint32_t total;
  bool psh;
};

static size_t g_cases = 0, g_longest = 0;

// One commit's vote (flag, sec, nanos) through the three encoders; fits: whether device_template must
// accept the commit.  Prints the message.
static int one(const std::string &chain, int64_t height, int32_t round, const Bid &b, int flag, int64_t sec,
               int32_t nanos, bool fits) {
  uint8_t h[32], p[32];
  for (int i = 0; i < 32; i++) { h[i] = (uint8_t)(0xa0 + i); p[i] = (uint8_t)(0x10 + i); }
  tmed_vote_template t;
  t.chain_id = chain.data();
  t.chain_id_len = (uint32_t)chain.size();
  t.height = height;
  t.round = round;
  t.block_hash = h;
  t.block_hash_len = b.hash ? 32 : 0;
  t.psh_total = b.total;
  t.psh_hash = p;
  t.psh_hash_len = b.psh ? 32 : 0;
  tmed::VoteEncoder enc;
  CHECK(enc.init(&t) == TMED_OK && enc.bid_ok);

  // the host encoder, into a buffer of exactly size() bytes
  const size_t len = enc.size(flag, sec, nanos);
  std::unique_ptr<uint8_t[]> host(new uint8_t[len]);
  CHECK(enc.write(host.get(), flag, sec, nanos) == host.get() + len);

  // the device route: the record, then the splice into one slot
  std::unique_ptr<uint8_t[]> rec(new uint8_t[tmed::kVoteTmplBytes]);
  memset(rec.get(), 0, tmed::kVoteTmplBytes);
  const bool fit = enc.device_template(rec.get(), tmed::kVoteTmplBytes, tmed::kVoteSlot);
  CHECK(fit == fits);
  const size_t longest = enc.size(2, -1, -1);  // ten-byte seconds and nanos
  CHECK(fit == (longest <= tmed::kVoteSlot));
  if (fit) {
    std::unique_ptr<uint8_t[]> slot(new uint8_t[tmed::kVoteSlot]);
    CHECK(tmed::vote_from_template(slot.get(), rec.get(), flag, sec, nanos) == len);
    CHECK(memcmp(slot.get(), host.get(), len) == 0);
  }

  // the free-standing precommit: Commit -> the commit's BlockID, Absent / Nil -> the zero BlockID
  tmed::VoteRec r;
  memset(&r, 0, sizeof(r));
  r.type = 2;
  r.height = height;
  r.round = round;
  r.sec = sec;
  r.nanos = nanos;
  if (flag == 2) {
    r.psh_total = b.total;
    r.hash_len = b.hash ? 32 : 0;
    r.psh_len = b.psh ? 32 : 0;
    memcpy(r.hash, h, 32);
    memcpy(r.psh, p, 32);
  }
  CHECK(tmed::vote_free_size(r, (uint32_t)chain.size()) == len);
  std::unique_ptr<uint8_t[]> fr(new uint8_t[len]);
  CHECK(tmed::vote_free_write(r, (const uint8_t *)chain.data(), (uint32_t)chain.size(), fr.get()) == len);
  CHECK(memcmp(fr.get(), host.get(), len) == 0);

  for (size_t i = 0; i < len; i++) printf("%02x", host[i]);
  printf("\n");
  g_cases++;
  g_longest = len > g_longest ? len : g_longest;
  return 0;
}

static int run() {
  // zero, hash only, part-set hash only, full, and a total of one and of five varint bytes
  const Bid bids[] = {{false, 0, false}, {true, 0, false}, {false, 0, true}, {true, 123, true}, {false, 1, false},
                      {true, 0xffffffffu, true}};
  const int64_t heights[] = {0, 1, INT64_MAX};
  const int32_t rounds[] = {0, 1, INT32_MAX};
  const size_t chains[] = {0, 13, 50, 127, 128};
  const int64_t secs[] = {0, 1, -62135596800ll, 253402300799ll};
  const int32_t nanos[] = {0, 1, 999999999, -1};
  for (const Bid &b : bids) for (int64_t h : heights) for (int32_t r : rounds) for (size_t cl : chains)
    for (int64_t s : secs) for (int32_t ns : nanos) for (int flag = 1; flag <= 3; flag++)
      if (one(std::string(cl, 'c'), h, r, b, flag, s, ns, true)) return 1;
  // a body of 127 bytes behind a one-byte length, of 128 behind two: 08 02, 2a 00 and the chain-ID field
  for (size_t cl : {121, 122}) {
    tmed::VoteEncoder e;
    const std::string chain(cl, 'c');
    tmed_vote_template t = {chain.data(), (uint32_t)cl, 0, 0, nullptr, 0, 0, nullptr, 0};
    CHECK(e.init(&t) == TMED_OK && e.size(1, 0, 0) == (cl == 121 ? 1 + 127 : 2 + 128));
    if (one(chain, 0, 0, bids[0], 1, 0, 0, true)) return 1;
  }
  // the template-fit boundary with every field at its longest: pre 20, BlockID field 78, timestamp 24
  // and a chain-ID field of 3 + 129 make a body of 254 behind two bytes, the 256 of a slot; 130 do not fit
  for (int flag = 1; flag <= 3; flag++) {
    if (one(std::string(129, 'c'), INT64_MAX, INT32_MAX, bids[5], flag, -1, -1, true)) return 1;
    if (one(std::string(130, 'c'), INT64_MAX, INT32_MAX, bids[5], flag, -1, -1, false)) return 1;
  }
  CHECK(g_longest == 257);
  printf("wire-ok %zu %zu\n", g_cases, g_longest);
  return 0;
}

int main() { return run(); }
