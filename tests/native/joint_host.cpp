// joint_host.cpp — TEST-ONLY host build of the half-size path's joint radix-4 table
// (verify_core.h build_table_joint, verify_hs.h hs_straus_joint) beside the two-table form it
// replaced in the kernels (build_table_affine, hs_straus), for tests/test_joint_table_host.py and
// as the host twin of tmed_test_joint_rows (tests/test_gpu_joint_table.py).  Never part of the
// product.
#include <stdint.h>
#include <string.h>

#include "verify_core.h"
#include "verify_hs.h"

using namespace tmed;

namespace {

// The device's SlabTabN<12> on a host array: rows in fe_pack256 form, Y+X and Y-X exchanged by
// the take of a negated entry.
struct JointTab {
  uint32_t rows[kJointRows + 1][32];
  int pf = 0;
  bool sw = false;
  void store(int j, const ge_cached &c) {
    const fe *fs[4] = {&c.YpX, &c.YmX, &c.Z, &c.T2d};
    for (int f = 0; f < 4; f++) fe_pack256(rows[j] + 8 * f, *fs[f]);
  }
  void prefetch(int j, bool swap = false) { pf = j; sw = swap; }
  void take(ge_cached &c) const {
    fe *fs[4] = {sw ? &c.YmX : &c.YpX, sw ? &c.YpX : &c.YmX, &c.Z, &c.T2d};
    for (int f = 0; f < 4; f++) fe_unpack256(*fs[f], rows[pf] + 8 * f);
  }
};

// The two-table form's accessor (hostsim.cpp's HostTab).
struct Tab8 {
  ge_cached e[9];
  int pf = 0;
  bool sw = false;
  void store(int j, const ge_cached &c) { e[j] = c; }
  void prefetch(int j, bool swap = false) { pf = j; sw = swap; }
  void take(ge_cached &c) const {
    c = e[pf];
    if (sw) { const fe t = c.YpX; c.YpX = c.YmX; c.YmX = t; }
  }
};

// B rows computed on demand (hostsim.cpp's HostB26Ref, for either radix).
template <int BITS>
struct BRef {
  static constexpr int kBits = BITS;
  const ge_p3 *base;
  int pf = 0;
  void prefetch(int j) { pf = j; }
  void take(ge_niels &n) const {
    if (pf == 0) ge_niels_0(n);
    else comb_entry(n, *base, (uint32_t)pf, BITS);
  }
};

const ge_p3 *b_bases() {
  static ge_p3 b[2];
  static bool init = false;
  if (!init) {
    ge_base_point(b[0]);
    b[1] = b[0];
    for (int i = 0; i < 16; i++) ge_mul256(b[1]);  // 2^128 B
    init = true;
  }
  return b;
}

void to_bytes(uint8_t *o, const uint32_t w[8]) {
  for (int i = 0; i < 32; i++) o[i] = (uint8_t)(w[i / 4] >> (8 * (i % 4)));
}

// A and R from their encodings (Point.SetBytes; the identity when one does not decode), then
// P = -A and Q = -sign(d) R as the main kernel forms them.
void points(ge_p3 &P, ge_p3 &Q, const uint8_t *a32, const uint8_t *r32, int dneg) {
  uint32_t aw[8], rw[8];
  load_words8(aw, a32);
  load_words8(rw, r32);
  ge_p3 A, R;
  ge_frombytes_go(A, aw);
  ge_frombytes_go(R, rw);
  hs_points(P, Q, dneg != 0, A, R.X, R.Y);
}

void enc_cached(uint8_t *o, const ge_cached &c) {
  ge_p3 p;
  ge_cached_to_p3(p, c);
  uint32_t w[8];
  ge_tobytes(w, p.X, p.Y, p.Z);
  to_bytes(o, w);
}

}  // namespace

extern "C" {

void jointhost_split4(int D, int *h, int *l) { hs_split4(D, *h, *l); }

int jointhost_index(int i, int j) { return joint_index(i, j); }

// The twelve rows as the device stores them: rows[12][128].
void jointhost_rows(const uint8_t *a32, const uint8_t *r32, int dneg, uint8_t *rows) {
  ge_p3 P, Q;
  points(P, Q, a32, r32, dneg);
  JointTab tj;
  build_table_joint(tj, P, Q);
  for (int j = 1; j <= kJointRows; j++)
    for (int w = 0; w < 32; w++)
      for (int b = 0; b < 4; b++) rows[128 * (j - 1) + 4 * w + b] = (uint8_t)(tj.rows[j][w] >> (8 * b));
}

// got[13][32]: the encoding of every row of the joint table (row 0: the identity), taken as the
// Straus loop takes it.  exp[13][32]: i P + j Q for the row's (i, j) from the two-table form's
// code — build_table_affine's entries i P and |j| Q and one ge_add_cached.
void jointhost_rows_enc(const uint8_t *a32, const uint8_t *r32, int dneg, uint8_t *got, uint8_t *exp) {
  ge_p3 P, Q;
  points(P, Q, a32, r32, dneg);
  JointTab tj;
  build_table_joint(tj, P, Q);
  Tab8 ta, tr;
  build_table_affine(ta, P);
  build_table_affine(tr, Q);
  for (int i = 0; i <= 2; i++)
    for (int j = -2; j <= 2; j++) {
      const int idx = joint_index(i, j);
      if (idx < 0) continue;
      ge_cached c;
      tj.prefetch(idx, false);
      tj.take(c);
      enc_cached(got + 32 * idx, c);
      ge_p3 p;
      ge_p1p1 t;
      ge_cached_to_p3(p, ta.e[i]);
      ge_add_cached(t, p, tr.e[j < 0 ? -j : j], j < 0);
      ge_p1p1_to_p3(p, t);
      uint32_t w[8];
      ge_tobytes(w, p.X, p.Y, p.Z);
      to_bytes(exp + 32 * idx, w);
    }
}

// [e]B + [c]P + [|d|]Q over W windows by the joint table (enc_joint) and by the two tables
// (enc_two); c, |d|, e: 32-byte LE scalars (c, |d| < 2^(4W), e < L), b16: the radix-2^16 B windows.
void jointhost_straus(const uint8_t *c32, const uint8_t *d32, const uint8_t *e32, int W, const uint8_t *a32,
                      const uint8_t *r32, int dneg, int b16, uint8_t *enc_joint, uint8_t *enc_two) {
  ge_p3 P, Q;
  points(P, Q, a32, r32, dneg);
  uint32_t c[8], d[8], e[8], er[8];
  load_words8(c, c32);
  load_words8(d, d32);
  load_words8(e, e32);
  HsDigits dg;
  sc_recode16(dg.cr, c);
  sc_recode16(dg.dr, d);
  if (b16) sc_recode_b<16>(er, e);
  else memcpy(er, e, sizeof er);
  const ge_p3 *bb = b_bases();
  JointTab tj;
  Tab8 ta, tr;
  build_table_joint(tj, P, Q);
  build_table_affine(ta, P);
  build_table_affine(tr, Q);
  ge_p2 qj, qt;
  if (b16) {
    BRef<16> bl{&bb[0]}, bh{&bb[1]};
    hs_straus_joint(qj, dg, er, W, tj, bl, bh);
    hs_straus(qt, dg, er, W, ta, tr, bl, bh);
  } else {
    BRef<26> bl{&bb[0]}, bh{&bb[1]};
    hs_straus_joint(qj, dg, er, W, tj, bl, bh);
    hs_straus(qt, dg, er, W, ta, tr, bl, bh);
  }
  uint32_t w[8];
  ge_tobytes(w, qj.X, qj.Y, qj.Z);
  to_bytes(enc_joint, w);
  ge_tobytes(w, qt.X, qt.Y, qt.Z);
  to_bytes(enc_two, w);
}

}  // extern "C"
