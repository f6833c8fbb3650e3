// zip_finish_host.cpp — TEST ONLY: the ZIP-215 finish (csrc/zip_finish.h zip_finish_one, the source
// keyset_finish_zip_kernel compiles) as a stand-alone host program, built by
// tests/test_zip_finish_host.py under AddressSanitizer and UndefinedBehaviorSanitizer.
//
//   zip_finish_host <rows> <out>
// rows: m records of 153 bytes: 30 little-endian int32 limbs (X, Y, Z), the 32 bytes of R, the bit
// already in `out`.  out: m bytes, each record's decision.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "zip_finish.h"

static constexpr size_t kRow = 30 * 4 + 32 + 1;

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s <rows> <out>\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  std::vector<uint8_t> in;
  uint8_t buf[4096];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) in.insert(in.end(), buf, buf + k);
  fclose(f);
  if (in.empty() || in.size() % kRow != 0) {
    fprintf(stderr, "%s: %zu bytes is not a whole number of %zu-byte rows\n", argv[1], in.size(), kRow);
    return 2;
  }
  const size_t m = in.size() / kRow;
  std::vector<uint8_t> out(m);
  for (size_t p = 0; p < m; p++) {
    const uint8_t *row = in.data() + p * kRow;
    int32_t limbs[30];
    memcpy(limbs, row, sizeof limbs);
    tmed::fe X, Y, Z;
    for (int i = 0; i < 10; i++) {
      X.v[i] = limbs[i];
      Y.v[i] = limbs[10 + i];
      Z.v[i] = limbs[20 + i];
    }
    uint32_t Rw[8];
    memcpy(Rw, row + 120, 32);  // little-endian words, as load_row_words reads a signature row
    out[p] = tmed::zip_finish_one(X, Y, Z, Rw, row[152] != 0) ? 1 : 0;
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 1, m, f) != m || fclose(f) != 0) {
    perror(argv[2]);
    return 2;
  }
  return 0;
}
