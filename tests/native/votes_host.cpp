// votes_host.cpp — TEST-ONLY stand-alone host program: the free-standing votes' encoder and checks
// (csrc/vote_free.h through csrc/votes_host.h, the source vote_prepare_kernel compiles) on the CPU.
// tests/test_votes_host.py builds it with -fsanitize=address,undefined and runs it as a plain
// executable:
//   g++ -std=c++17 -fsanitize=address,undefined -I tendermint-fork_amd/csrc votes_host.cpp
//   votes_host sweep <out.bin>   VoteSignBytes over the product of field values below (the order of
//                                Python's itertools.product), each message as u16 length + bytes
//   votes_host cases <in.txt>    requests read from a text file, "code msg_len" per vote on stdout
// Input of `cases`, blank-separated ("-" = empty bytes):
//   req <flags> <height> <round> <type> <chain hex> <n_vals> <n_votes>
//   val <key hex> <address hex>                                                      n_vals lines
//   vote <type> <height> <round> <hash hex> <total> <psh hex> <seconds> <nanos> <address hex> <index> <sig_len>
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "votes_host.h"

#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      fprintf(stderr, "votes_host.cpp:%d: %s\n", __LINE__, #c); \
      return 1;                                                 \
    }                                                           \
  } while (0)

// Arrays of exactly the sizes the structs promise: the sanitizer sees any byte read past them.
struct Votes {
  std::vector<int32_t> type, round, nanos, index;
  std::vector<int64_t> height, sec;
  std::vector<uint8_t> hash, psh, addr, sig;
  std::vector<uint32_t> hash_len, psh_len, addr_len, sig_len, total;
  tmed_votes c;
  static void put(std::vector<uint8_t> &dst, std::vector<uint32_t> &lens, const std::vector<uint8_t> &b, size_t w) {
    const size_t at = dst.size();
    dst.resize(at + w, 0);
    if (!b.empty()) memcpy(dst.data() + at, b.data(), b.size() < w ? b.size() : w);
    lens.push_back((uint32_t)b.size());
  }
  void add(int32_t t, int64_t h, int32_t r, const std::vector<uint8_t> &bh, uint32_t tot, const std::vector<uint8_t> &ph,
           int64_t s, int32_t ns, const std::vector<uint8_t> &a, int32_t idx, uint32_t slen) {
    type.push_back(t); height.push_back(h); round.push_back(r); total.push_back(tot);
    sec.push_back(s); nanos.push_back(ns); index.push_back(idx);
    put(hash, hash_len, bh, 32);
    put(psh, psh_len, ph, 32);
    put(addr, addr_len, a, 20);
    sig.resize(sig.size() + 64, 0);
    sig_len.push_back(slen);
  }
  void finish() {
    memset(&c, 0, sizeof(c));
    c.n = type.size();
    c.types = type.data(); c.heights = height.data(); c.rounds = round.data();
    c.block_hashes = hash.data(); c.block_hash_lens = hash_len.data();
    c.psh_totals = total.data(); c.psh_hashes = psh.data(); c.psh_hash_lens = psh_len.data();
    c.ts_seconds = sec.data(); c.ts_nanos = nanos.data();
    c.addresses = addr.data(); c.address_lens = addr_len.data();
    c.validator_indexes = index.data(); c.sigs = sig.data(); c.sig_lens = sig_len.data();
  }
};

static std::vector<uint8_t> unhex(const std::string &s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return out;
}

static int run_sweep(const char *path) {
  const int32_t types[] = {0, 1, 2, 32, -1, INT32_MAX};
  const int64_t heights[] = {0, 1, -1, INT64_MAX};
  const int32_t rounds[] = {0, 1, -1, INT32_MAX};
  const int64_t secs[] = {0, 1, -62135596800ll, INT64_MAX};
  const int32_t nanos[] = {0, 1, 999999999};
  const std::string chains[] = {"", "test_chain_id", std::string(50, 'c')};
  std::vector<uint8_t> h(32), p(32), none;
  for (int i = 0; i < 32; i++) { h[i] = (uint8_t)(0xa0 + i); p[i] = (uint8_t)(0x10 + i); }
  struct Bid { const std::vector<uint8_t> *h; uint32_t t; const std::vector<uint8_t> *p; };
  const Bid bids[] = {{&none, 0, &none}, {&h, 123, &p}, {&h, 0, &none}, {&none, 0, &p}, {&none, 7, &none},
                      {&h, 0xffffffffu, &p}};
  FILE *f = fopen(path, "wb");
  CHECK(f);
  size_t count = 0, longest = 0;
  // product order: type, height, round, BlockID, seconds, nanos, chain (the last varies fastest)
  for (int32_t t : types) for (int64_t ht : heights) for (int32_t r : rounds) for (const Bid &b : bids)
    for (int64_t s : secs) for (int32_t ns : nanos) for (const std::string &chain : chains) {
      Votes v;
      v.add(t, ht, r, *b.h, b.t, *b.p, s, ns, none, 0, 64);
      v.finish();
      // exact-size output buffer: sized by a first call, as a caller would
      uint32_t off[2];
      size_t len = 0;
      uint8_t bad = 9;
      CHECK(tmed_votes_host::votes_sign_bytes(chain.data(), (uint32_t)chain.size(), &v.c, nullptr, 0, off, &len, &bad) == TMED_OK);
      CHECK(bad == 0 && len > 0 && len <= tmed::kVoteFreeMsgMax);
      std::unique_ptr<uint8_t[]> out(new uint8_t[len]);
      CHECK(tmed_votes_host::votes_sign_bytes(chain.data(), (uint32_t)chain.size(), &v.c, out.get(), len, off, &len, &bad) == TMED_OK);
      CHECK(off[0] == 0 && off[1] == len);
      const uint8_t l2[2] = {(uint8_t)len, (uint8_t)(len >> 8)};
      CHECK(fwrite(l2, 1, 2, f) == 2 && fwrite(out.get(), 1, len, f) == len);
      longest = len > longest ? len : longest;
      count++;
    }
  fclose(f);
  // the worst case of the bound beside kVoteSlot: every field at its longest, a 50-byte chain ID
  {
    Votes v;
    v.add(-1, 1, 1, h, 0xffffffffu, p, -1, -1, none, 0, 64);
    v.finish();
    uint32_t off[2];
    size_t len = 0;
    uint8_t bad = 0;
    const std::string chain(50, 'c');
    CHECK(tmed_votes_host::votes_sign_bytes(chain.data(), 50, &v.c, nullptr, 0, off, &len, &bad) == TMED_OK);
    CHECK(len == tmed::kVoteFreeMsgMax && len == 185);
  }
  // a malformed BlockID encodes nothing; without the malformed array it is a malformed call
  {
    Votes v;
    v.add(1, 1, 0, std::vector<uint8_t>(31, 1), 1, p, 1, 1, none, 0, 64);
    v.add(1, 1, 0, h, 1, std::vector<uint8_t>(33, 1), 1, 1, none, 0, 64);
    v.add(1, 1, 0, h, 1, p, 1, 1, none, 0, 64);
    v.finish();
    uint32_t off[4];
    size_t len = 0;
    uint8_t bad[3] = {9, 9, 9};
    CHECK(tmed_votes_host::votes_sign_bytes("x", 1, &v.c, nullptr, 0, off, &len, bad) == TMED_OK);
    CHECK(bad[0] == 1 && bad[1] == 1 && bad[2] == 0 && off[0] == 0 && off[1] == 0 && off[2] == 0 && off[3] == len);
    CHECK(tmed_votes_host::votes_sign_bytes("x", 1, &v.c, nullptr, 0, off, &len, nullptr) == TMED_EINVAL);
    CHECK(tmed_votes_host::votes_sign_bytes(nullptr, 1, &v.c, nullptr, 0, off, &len, bad) == TMED_EINVAL);
    CHECK(tmed_votes_host::votes_sign_bytes("x", 1, nullptr, nullptr, 0, off, &len, bad) == TMED_EINVAL);
  }
  printf("sweep-ok %zu %zu\n", count, longest);
  return 0;
}

static int run_cases(const char *path) {
  std::ifstream in(path);
  CHECK(in.good());
  std::string tok;
  while (in >> tok) {
    CHECK(tok == "req");
    uint32_t flags;
    int64_t height;
    int32_t round, type;
    std::string chain_hex;
    size_t n_vals, n_votes;
    in >> flags >> height >> round >> type >> chain_hex >> n_vals >> n_votes;
    const std::vector<uint8_t> chain = unhex(chain_hex);
    std::vector<uint8_t> pubs, addrs;
    for (size_t i = 0; i < n_vals; i++) {
      std::string k, a;
      in >> tok >> k >> a;
      CHECK(tok == "val");
      const std::vector<uint8_t> kb = unhex(k), ab = unhex(a);
      CHECK(kb.size() == 32 && ab.size() == 20);
      pubs.insert(pubs.end(), kb.begin(), kb.end());
      addrs.insert(addrs.end(), ab.begin(), ab.end());
    }
    Votes v;
    for (size_t i = 0; i < n_votes; i++) {
      int32_t t, r, ns, idx;
      int64_t ht, s;
      uint32_t total, slen;
      std::string hh, ph, ah;
      in >> tok >> t >> ht >> r >> hh >> total >> ph >> s >> ns >> ah >> idx >> slen;
      CHECK(tok == "vote" && !in.fail());
      v.add(t, ht, r, unhex(hh), total, unhex(ph), s, ns, unhex(ah), idx, slen);
    }
    v.finish();
    tmed_valset vs;
    memset(&vs, 0, sizeof(vs));
    vs.n = n_vals;
    vs.pubkeys = pubs.data();
    vs.addresses = addrs.data();
    tmed_vote_request q;
    memset(&q, 0, sizeof(q));
    q.chain_id = (const char *)chain.data();
    q.chain_id_len = (uint32_t)chain.size();
    q.vals = &vs;
    q.votes = &v.c;
    q.flags = flags;
    q.height = height;
    q.round = round;
    q.msg_type = type;
    std::vector<uint8_t> codes(n_votes), again(n_votes);
    std::vector<uint32_t> lens(n_votes);
    uint8_t route = 9;
    CHECK(tmed_votes_host::verify_votes_host(&q, 1, codes.data(), lens.data(), &route) == TMED_OK);
    CHECK(route == (chain.size() <= 50));
    tmed_votes_host::request_prechecks(q, again.data());  // the device batch's host route
    CHECK(again == codes);
    for (size_t i = 0; i < n_votes; i++) printf("%u %u\n", codes[i], lens[i]);
  }
  // malformed calls
  {
    tmed_vote_request q;
    memset(&q, 0, sizeof(q));
    uint8_t code;
    CHECK(tmed_votes_host::verify_votes_host(&q, 1, &code, nullptr, nullptr) == TMED_EINVAL);
    CHECK(tmed_votes_host::verify_votes_host(nullptr, 1, &code, nullptr, nullptr) == TMED_EINVAL);
    CHECK(tmed_votes_host::verify_votes_host(nullptr, 0, nullptr, nullptr, nullptr) == TMED_OK);
  }
  printf("cases-ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && std::string(argv[1]) == "sweep") return run_sweep(argv[2]);
  if (argc == 3 && std::string(argv[1]) == "cases") return run_cases(argv[2]);
  fprintf(stderr, "usage: votes_host sweep <out.bin> | cases <in.txt>\n");
  return 2;
}
