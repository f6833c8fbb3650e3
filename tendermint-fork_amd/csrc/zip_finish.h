// zip_finish.h — the ZIP-215 finish of the key-cached routes: one signature's decision from the
// projective P = [S]B + [k](-A) a main kernel left in its fin slot and the 32 bytes of R.
//
// The Go rule's finish (verify_core.h finish_group / projective_matches) asks whether P encodes to
// the bytes of R.  ZIP-215 decodes R permissively instead (ge_frombytes_go: y >= p reduced, x = 0
// with the sign bit set accepted, which is also how the keys were decoded) and asks whether
// [8](P - R) is the identity, so P may differ from R by any of the eight small-order points.
// Host and device compile this source (tests/native/zip_finish_host.cpp; kernels.hip
// keyset_finish_zip_kernel).
#pragma once
#include "ge25519.h"

namespace tmed {

// bit && Z != 0 && R decodes && [8](P - R) == identity, for P = (X : Y : Z) with X, Y, Z carried
// values (what ge_p1p1_to_p2 / ge_p1p1_to_p3 store through fin_store).
//   * P has no T: (X Z : Y Z : Z^2 : X Y) is the same point in extended form (3 M + 1 S).
//   * P - R is the unified a = -1 addition (ge_add_cached, complete since d is a non-square): P = R,
//     the ordinary valid signature, needs no doubling case, and a difference of order 2, 4 or 8 comes
//     out as that exact point, which the three doublings (complete as well) take to the identity.
//   * the identity test is on fully reduced values (fe_iszero / fe_equal go through fe_to_words):
//     x = 0 and y = 1, that is X == 0 and Y == Z with Z != 0.
//   * Z == 0 never comes out of the complete formulas for points on the curve; it is rejected all
//     the same, as verify_finish_kernel does: with Z = 0 every coordinate of the extended form is 0
//     and "X == 0 and Y == Z" would hold by accident.
// A rejected R leaves the identity in its place (ge_frombytes_go), so the arithmetic stays defined
// and the decision is masked at the end: no branch on the data.
// (two steps so that the kernel can decode R, the long chain, before it loads P: the thirty limbs of
// P are then not live across the decompression)
TMED_HD bool zip_finish_check(const fe &X, const fe &Y, const fe &Z, const ge_p3 &R, bool r_ok, bool bit) {
  ge_p3 P;
  fe_mul_x2(P.X, X, Z, P.Y, Y, Z);
  fe_sqc(P.Z, Z);
  fe_mul(P.T, X, Y);
  ge_cached rc;
  ge_p3_to_cached(rc, R);
  ge_p1p1 t;
  ge_p2 q;
  ge_add_cached(t, P, rc, /*neg=*/true);  // P - R
#pragma unroll 1
  for (int i = 0; i < 3; i++) {  // [8]
    ge_p1p1_to_p2(q, t);
    ge_p2_dbl(t, q);
  }
  ge_p1p1_to_p2(q, t);
  const bool identity = fe_iszero(q.X) && fe_equal(q.Y, q.Z) && !fe_iszero(q.Z);
  return bit && r_ok && !fe_iszero(Z) && identity;
}

TMED_HD bool zip_finish_one(const fe &X, const fe &Y, const fe &Z, const uint32_t Rw[8], bool bit) {
  ge_p3 R;
  const bool r_ok = ge_frombytes_go(R, Rw);
  return zip_finish_check(X, Y, Z, R, r_ok, bit);
}

}  // namespace tmed
