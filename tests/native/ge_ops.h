// ge_ops.h — TEST-ONLY: the group-layer functions of ge25519.h and verify_core.h by number, one
// call each, shared by the host build (hostsim.cpp, hostsim_ge) and the device harness
// (devprim.hip, devprim_ge) so that both run the identical cases (tests/group_cases.py).
//
// in: up to eight field elements (raw limbs, meaning per op); out: four (unused ones zero).
//   0 ge_p2_dbl           in 0..2 = X, Y, Z                          out = p1p1 X, Y, Z, T
//   1 ge_add_cached       in 0..3 = p3 X, Y, Z, T; 4..7 = cached YpX, YmX, Z, T2d   out = p1p1
//   2 ge_add_cached_pre   as 1; the operand is passed as given (the caller has exchanged
//                         YpX / YmX when neg, as the callers' load addresses do)
//   3 ge_madd_niels       in 0..3 = p3; 4..6 = niels YpX, YmX, XY2d  out = p1p1
//   4 ge_p1p1_to_p2       in 0..3 = p1p1                             out = X, Y, Z
//   5 ge_p1p1_to_p3       in 0..3 = p1p1                             out = X, Y, Z, T
//   6 ge_p3_to_cached     in 0..3 = p3                               out = YpX, YmX, Z, T2d
//   7 ge_cached_to_p3     in 0..3 = cached                           out = X, Y, Z, T
//   8 ge_p3_add           in 0..3 = acc; 4..7 = o                    out = acc + o
//   9 ge_p3_to_niels      in 0..3 = p3                               out = YpX, YmX, XY2d
#pragma once
#include "verify_core.h"

namespace tmed {

constexpr int kGeOps = 10;

template <int OP>
TMED_HD void ge_op_run(bool neg, const fe in[8], fe out[4]) {
#pragma unroll
  for (int k = 0; k < 4; k++) fe_0(out[k]);
  if constexpr (OP == 0) {
    const ge_p2 p{in[0], in[1], in[2]};
    ge_p1p1 r;
    ge_p2_dbl(r, p);
    out[0] = r.X; out[1] = r.Y; out[2] = r.Z; out[3] = r.T;
  } else if constexpr (OP == 1 || OP == 2) {
    const ge_p3 p{in[0], in[1], in[2], in[3]};
    const ge_cached q{in[4], in[5], in[6], in[7]};
    ge_p1p1 r;
    if constexpr (OP == 1) ge_add_cached(r, p, q, neg);
    else ge_add_cached_pre(r, p, q, neg);
    out[0] = r.X; out[1] = r.Y; out[2] = r.Z; out[3] = r.T;
  } else if constexpr (OP == 3) {
    const ge_p3 p{in[0], in[1], in[2], in[3]};
    const ge_niels q{in[4], in[5], in[6]};
    ge_p1p1 r;
    ge_madd_niels(r, p, q, neg);
    out[0] = r.X; out[1] = r.Y; out[2] = r.Z; out[3] = r.T;
  } else if constexpr (OP == 4) {
    const ge_p1p1 p{in[0], in[1], in[2], in[3]};
    ge_p2 r;
    ge_p1p1_to_p2(r, p);
    out[0] = r.X; out[1] = r.Y; out[2] = r.Z;
  } else if constexpr (OP == 5) {
    const ge_p1p1 p{in[0], in[1], in[2], in[3]};
    ge_p3 r;
    ge_p1p1_to_p3(r, p);
    out[0] = r.X; out[1] = r.Y; out[2] = r.Z; out[3] = r.T;
  } else if constexpr (OP == 6) {
    const ge_p3 p{in[0], in[1], in[2], in[3]};
    ge_cached r;
    ge_p3_to_cached(r, p);
    out[0] = r.YpX; out[1] = r.YmX; out[2] = r.Z; out[3] = r.T2d;
  } else if constexpr (OP == 7) {
    const ge_cached c{in[0], in[1], in[2], in[3]};
    ge_p3 r;
    ge_cached_to_p3(r, c);
    out[0] = r.X; out[1] = r.Y; out[2] = r.Z; out[3] = r.T;
  } else if constexpr (OP == 8) {
    ge_p3 acc{in[0], in[1], in[2], in[3]};
    const ge_p3 o{in[4], in[5], in[6], in[7]};
    ge_p3_add(acc, o);
    out[0] = acc.X; out[1] = acc.Y; out[2] = acc.Z; out[3] = acc.T;
  } else {
    const ge_p3 p{in[0], in[1], in[2], in[3]};
    ge_niels r;
    ge_p3_to_niels(r, p);
    out[0] = r.YpX; out[1] = r.YmX; out[2] = r.XY2d;
  }
}

}  // namespace tmed
