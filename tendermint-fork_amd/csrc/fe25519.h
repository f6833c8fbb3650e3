// fe25519.h — GF(2^255-19) arithmetic for the CDNA4 verify kernels.
//
// Replaces the field layer of Go 1.18 crypto/internal/edwards25519/field
// (third-party to the reference; reached from crypto/ed25519/ed25519.go:154).
//
// Representation: 10 signed 32-bit limbs, radix 2^25.5 (limb i weighs
// 2^ceil(25.5 i); 26 bits for even i, 25 for odd i).  Every limb product is a
// single v_mad_i64_i32 into a 64-bit accumulator: the radix leaves enough
// head-room that a column of 10 products (including the x19 wrap and the x2
// odd-odd factor) never overflows int64, so no carry handling is needed inside
// a multiplication — only one carry pass per result.
//
// Magnitude discipline (checked by tools/gen_fe_asm.py check_bounds and by
// tests/test_kernel_host.py on the host build):
//   "carried" value — every mul/sq output: even limbs in [-2^25, 2^25) (rounded carries),
//     odd limbs in [0, 2^25) (floored carries; limb 1 in [-2^16, 2^25 + 2^16)); fe_carry /
//     fe_from_words give odd limbs in [-2^24, 2^24], inside the same bound
//   mul/sq inputs may be sums/differences of up to THREE carried values
//   (19 * 3 * (2^25 + 2^16) < 2^31 keeps the pre-multiplied operand in int32; the
//   column sum stays below 2^61.3).
//   fe_mul's FIRST operand f (and fe_mul_x2's f0, f1) may be a sum/difference of up to FOUR
//   carried values while g stays within three: f is only ever doubled (2 * 4 * (2^25 + 2^16)
//   < 2^31) and the worst column is below 2^61.7, inside check_bounds' 2^62.5.  The allowance is
//   one-sided — a 4-sum g would leave int32 in its x19 copy — and quad.h's doubling relies on it
//   (F = B - A - 2C is the f of quad_round2); tests/test_group_host.py and
//   tests/test_gpu_group.py hold it in place (check_bounds with nsum 4 x 3, and the products at
//   the limb extremes on both builds).
//
// All functions are __host__ __device__ so that the identical code can be
// exercised on the CPU by the test-only host build (tests/, never the product).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TMED_HD __host__ __device__ __forceinline__
#define TMED_HDM __host__ __device__ __forceinline__  // member functions
#else
#define TMED_HD static inline
#define TMED_HDM inline
#endif

namespace tmed {

struct fe { int32_t v[10]; };

// x*19, x*38: one v_mul_lo_u32 each.  (Measured on gfx950, tools/probe_valu.py:
// v_mul_lo_u32 issues at the same rate as one v_lshl_add_u32, so the two-shift-add
// form would cost twice as much.)
TMED_HD int32_t mul19(int32_t x) { return (int32_t)(19u * (uint32_t)x); }
TMED_HD int32_t mul38(int32_t x) { return (int32_t)(38u * (uint32_t)x); }
// 2x as one v_add_u32 (LLVM selects v_lshlrev_b32 for x << 1, which issues at half the rate of
// v_add_u32 on gfx950: profiles/r02/micro/issue_probe.jsonl).
TMED_HD int32_t dbl32(int32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  int32_t r;
  asm("v_add_u32 %0, %1, %1" : "=v"(r) : "v"(x));
  return r;
#else
  return (int32_t)(2u * (uint32_t)x);
#endif
}

TMED_HD void fe_0(fe &h) {
#pragma unroll
  for (int i = 0; i < 10; i++) h.v[i] = 0;
}
TMED_HD void fe_1(fe &h) { fe_0(h); h.v[0] = 1; }
TMED_HD void fe_copy(fe &h, const fe &f) {
#pragma unroll
  for (int i = 0; i < 10; i++) h.v[i] = f.v[i];
}
TMED_HD void fe_add(fe &h, const fe &f, const fe &g) {
#pragma unroll
  for (int i = 0; i < 10; i++) h.v[i] = f.v[i] + g.v[i];
}
TMED_HD void fe_sub(fe &h, const fe &f, const fe &g) {
#pragma unroll
  for (int i = 0; i < 10; i++) h.v[i] = f.v[i] - g.v[i];
}
TMED_HD void fe_neg(fe &h, const fe &f) {
#pragma unroll
  for (int i = 0; i < 10; i++) h.v[i] = -f.v[i];
}
// h = b ? g : f   (lane-local select, no branch)
TMED_HD void fe_select(fe &h, const fe &f, const fe &g, bool b) {
#pragma unroll
  for (int i = 0; i < 10; i++) h.v[i] = b ? g.v[i] : f.v[i];
}

// Column biases: the accumulators start at B_k = 2^25 (even k) / 2^24 (odd k), so the
// rounding carry c = (h + B) >> s needs no separate bias add.  Carried columns are kept
// biased (L_k = (h_k + B_k) mod 2^s, 32-bit) until the end, where limb_k = L_k - B_k in
// [-2^25, 2^25) / [-2^24, 2^24): the same centered result as the unbiased chain, with
// one 64-bit shift, one 32-bit and, one 64-bit add per carry (+ one 32-bit sub per limb).
TMED_HD int64_t fe_bias(int k) { return (k & 1) ? ((int64_t)1 << 24) : ((int64_t)1 << 25); }

// The products of fe_mul / fe_sq / fe_sq2 as explicit v_mad_i64_i32 schedules with the carry
// chain fused in (generated: tools/gen_fe_asm.py).  Column sums with a separate carry pass cost
// ~8 % more instructions and were slower even for a lone wave (C1 keyed 0.0840 against 0.0801 ms,
// profiles/r04/s20/).
#include "fe_cols.h"

// Carry pass over BIASED 64-bit column sums H_k = h_k + B_k -> carried limbs.  Two
// interleaved chains (0..4 and 4..9) give the scheduler independent work.
TMED_HD void fe_carry64(fe &out, int64_t H[10]) {
  uint32_t L[10];
  int64_t c;
#define TMED_CARRY(k, s)              \
  c = H[k] >> (s);                    \
  L[k] = (uint32_t)H[k] & ((1u << (s)) - 1u);
  TMED_CARRY(0, 26); H[1] += c;
  TMED_CARRY(4, 26); H[5] += c;
  TMED_CARRY(1, 25); H[2] += c;
  TMED_CARRY(5, 25); H[6] += c;
  TMED_CARRY(2, 26); H[3] += c;
  TMED_CARRY(6, 26); H[7] += c;
  TMED_CARRY(3, 25); H[4] = (int64_t)L[4] + c;   // column 4 again (biased L4 + carry)
  TMED_CARRY(7, 25); H[8] += c;
  TMED_CARRY(4, 26); L[5] += (uint32_t)c;           // column 5 already carried
  TMED_CARRY(8, 26); H[9] += c;
  TMED_CARRY(9, 25); H[0] = (int64_t)L[0] + c * 19;  // 2^255 = 19 (mod p)
  TMED_CARRY(0, 26); L[1] += (uint32_t)c;           // column 1 already carried
#undef TMED_CARRY
#pragma unroll
  for (int i = 0; i < 10; i++) out.v[i] = (int32_t)(L[i] - (uint32_t)fe_bias(i));
}

// Re-carry a 32-bit-limb value (e.g. a 2- or 3-sum) into carried form.
TMED_HD void fe_carry(fe &h, const fe &f) {
  int64_t t[10];
#pragma unroll
  for (int i = 0; i < 10; i++) t[i] = (int64_t)f.v[i] + fe_bias(i);
  fe_carry64(h, t);
}

// Fused carry (fe_mul_fused / fe_sq1_fused / fe_sq2_fused, tools/gen_fe_asm.py): the carry
// chain runs inside the column schedule.  Even columns round (their bias 2^25 arrives with the
// carry from below), odd columns floor: column 0 starts from 2^25, columns 1, 3, 5, 7 from 2^50
// (the bias of the next even column, pre-shifted by 25 — a multiple of 2^25, so the odd limb is
// unchanged and the odd carry brings exactly +2^25), column 9 from 0; even columns 2..8 start
// FROM the odd carry below (the first mad's addend: no add), odd columns take the even carry
// below with one 64-bit add.  Against fe_carry64: 5 instead of 10 64-bit adds, 9 instead of 11
// 64-bit shifts before the wrap, and only the even limbs lose a bias.  Here: the x19 wrap of
// column 9 into the biased column 0, its small carry into limb 1, and the limbs.
TMED_HD void fe_fused_fin(fe &h, const int64_t H[10]) {
  const int64_t c9 = H[9] >> 25;
  const int64_t h0 = (int64_t)((uint32_t)H[0] & 0x3ffffffu) + c9 * 19;
  const int32_t c0 = (int32_t)(h0 >> 26);  // |c0| < 2^16
  h.v[0] = (int32_t)((uint32_t)h0 & 0x3ffffffu) - (1 << 25);
  h.v[1] = (int32_t)((uint32_t)H[1] & 0x1ffffffu) + c0;
#pragma unroll
  for (int k = 2; k < 10; k++)
    h.v[k] = (k & 1) ? (int32_t)((uint32_t)H[k] & 0x1ffffffu) : (int32_t)((uint32_t)H[k] & 0x3ffffffu) - (1 << 25);
}

// h = f * g  (100 v_mad_i64_i32; operand pairs (i, j) carry x2 when both are odd and x19 on g_j
// when i + j >= 10 — fe_mul_fused)
TMED_HD void fe_mul(fe &h, const fe &f, const fe &g) {
  int32_t g19[10], f2[10];
#pragma unroll
  for (int j = 0; j < 10; j++) g19[j] = mul19(g.v[j]);
#pragma unroll
  for (int i = 0; i < 10; i++) f2[i] = dbl32(f.v[i]);
  int64_t acc[10];
  fe_mul_fused(acc, f.v, f2, g.v, g19);
  fe_fused_fin(h, acc);
}

// Column sums of D f^2, D = 1 (square) or 2 (the doubling's 2 Z^2): 55 products.  Pair (i, j),
// i <= j, carries the coefficient D * (i<j ? 2 : 1) * (i,j odd ? 2 : 1) * (i+j>=10 ? 19 : 1),
// spread over the two operands as pre-multiplied copies x2, x4, x19, x38 = 2 * x19 (the split:
// tools/gen_fe_asm.py sq_products): the 19 on the odd-index operand where there is one, with a
// factor 2 only on an odd (25-bit) limb, so every operand stays inside int32 for inputs up to
// three carried values (D = 1) or one (D = 2).
// (The fused squarings put the 19 on the higher index of a wrapped pair and never x38 on a
// 3-sum: fe_sq1_fused needs x2 of every limb, x4 of limbs 1, 3, 5, 7 and x19 of 5..9.)
struct fe_premul {
  int32_t x[10], x2[10], x4[10], x19[10], x38[10];
  TMED_HDM explicit fe_premul(const fe &f) {
#pragma unroll
    for (int i = 0; i < 10; i++) {
      x[i] = f.v[i];
      x2[i] = dbl32(f.v[i]);
      x4[i] = dbl32(x2[i]);
      x19[i] = mul19(f.v[i]);
      x38[i] = mul38(f.v[i]);
    }
  }
};

TMED_HD void fe_sq(fe &h, const fe &f) {
  const fe_premul p(f);
  int64_t acc[10];
  fe_sq1_fused(acc, p.x, p.x2, p.x4, p.x19, p.x38);
  fe_fused_fin(h, acc);
}

// h = f^2 for a CARRIED f (one carried value, e.g. any mul / sq output, not a sum):
// fe_sq1c_fused's 13 premultiplied copies (x2 of limbs 0, 1, 2, 3, 5, 7, x19 of 6, 8, x38 of
// 5..9; x38 of 6, 8 as 2 * x19) instead of fe_sq's 19.
struct fe_premul_c {
  int32_t x[10], x2[10], x19[10], x38[10];
  TMED_HDM explicit fe_premul_c(const fe &f) {
#pragma unroll
    for (int i = 0; i < 10; i++) {
      x[i] = f.v[i];
      x2[i] = dbl32(f.v[i]);
      x19[i] = mul19(f.v[i]);
      x38[i] = (i == 6 || i == 8) ? dbl32(x19[i]) : mul38(f.v[i]);
    }
  }
};

TMED_HD void fe_sqc(fe &h, const fe &f) {
  const fe_premul_c p(f);
  int64_t acc[10];
  fe_sq1c_fused(acc, p.x, p.x2, p.x19, p.x38);
  fe_fused_fin(h, acc);
}

// h = 2 f^2 (f carried)
TMED_HD void fe_sq2(fe &h, const fe &f) {
  const fe_premul p(f);
  int64_t acc[10];
  fe_sq2_fused(acc, p.x, p.x2, p.x4, p.x19, p.x38);
  fe_fused_fin(h, acc);
}

// Two independent products / squares in one schedule (fe_mul_fused_x2, fe_sq1_fused_x2,
// fe_sq2_sq1_fused): each chain's dependent instructions are >= 3 slots apart, where one product at
// a time leaves them 2 apart (~5 % per mad: profiles/r02/micro/mad_dep_probe.jsonl).  Outputs may
// alias inputs (everything is read before anything is written).
TMED_HD void fe_mul_x2(fe &h0, const fe &f0, const fe &g0, fe &h1, const fe &f1, const fe &g1) {
  int32_t a19[10], a2[10], b19[10], b2[10];
#pragma unroll
  for (int j = 0; j < 10; j++) { a19[j] = mul19(g0.v[j]); b19[j] = mul19(g1.v[j]); }
#pragma unroll
  for (int i = 0; i < 10; i++) { a2[i] = dbl32(f0.v[i]); b2[i] = dbl32(f1.v[i]); }
  int64_t H0[10], H1[10];
  fe_mul_fused_x2(H0, H1, f0.v, a2, g0.v, a19, f1.v, b2, g1.v, b19);
  fe_fused_fin(h0, H0);
  fe_fused_fin(h1, H1);
}

TMED_HD void fe_sq_x2(fe &h0, const fe &f0, fe &h1, const fe &f1) {
  const fe_premul a(f0), b(f1);
  int64_t H0[10], H1[10];
  fe_sq1_fused_x2(H0, H1, a.x, a.x2, a.x4, a.x19, a.x38, b.x, b.x2, b.x4, b.x19, b.x38);
  fe_fused_fin(h0, H0);
  fe_fused_fin(h1, H1);
}

// h0 = f0^2, h1 = f1^2 for carried f0, f1 (fe_sqc)
TMED_HD void fe_sqc_x2(fe &h0, const fe &f0, fe &h1, const fe &f1) {
  const fe_premul_c a(f0), b(f1);
  int64_t H0[10], H1[10];
  fe_sq1c_fused_x2(H0, H1, a.x, a.x2, a.x19, a.x38, b.x, b.x2, b.x19, b.x38);
  fe_fused_fin(h0, H0);
  fe_fused_fin(h1, H1);
}

// h0 = 2 f0^2 (f0 carried), h1 = f1^2
TMED_HD void fe_sq2_sq(fe &h0, const fe &f0, fe &h1, const fe &f1) {
  const fe_premul a(f0), b(f1);
  int64_t H0[10], H1[10];
  fe_sq2_sq1_fused(H0, H1, a.x, a.x2, a.x4, a.x19, a.x38, b.x, b.x2, b.x4, b.x19, b.x38);
  fe_fused_fin(h0, H0);
  fe_fused_fin(h1, H1);
}

// f carried (every caller squares a product output)
TMED_HD void fe_sqn(fe &h, const fe &f, int n) {
  fe_sqc(h, f);
#pragma unroll 1
  for (int i = 1; i < n; i++) fe_sqc(h, h);
}

// z^(2^250 - 1) and z^11 (shared prefix of the inversion / (p-5)/8 chains)
TMED_HD void fe_pow250(fe &z250, fe &z11, const fe &z) {
  fe z2, z9, t, a, b, c;
  fe_sqc(z2, z);                            // z carried (a product output at every call site)
  fe_sqn(t, z2, 2); fe_mul(z9, t, z);
  fe_mul(z11, z9, z2);
  fe_sqc(t, z11); fe_mul(a, t, z9);         // a = z^(2^5-1)
  fe_sqn(t, a, 5); fe_mul(b, t, a);         // b = 2^10-1
  fe_sqn(t, b, 10); fe_mul(c, t, b);        // c = 2^20-1
  fe_sqn(t, c, 20); fe_mul(t, t, c);        // 2^40-1
  fe_sqn(t, t, 10); fe_mul(a, t, b);        // a = 2^50-1
  fe_sqn(t, a, 50); fe_mul(b, t, a);        // b = 2^100-1
  fe_sqn(t, b, 100); fe_mul(t, t, b);       // 2^200-1
  fe_sqn(t, t, 50); fe_mul(z250, t, a);     // 2^250-1
}

TMED_HD void fe_invert(fe &out, const fe &z) {   // z^(p-2)
  fe z250, z11, t;
  fe_pow250(z250, z11, z);
  fe_sqn(t, z250, 5); fe_mul(out, t, z11);
}

TMED_HD void fe_pow22523(fe &out, const fe &z) { // z^((p-5)/8)
  fe z250, z11, t;
  fe_pow250(z250, z11, z);
  fe_sqn(t, z250, 2); fe_mul(out, t, z);
}

// 32 little-endian bytes, held as 8 LE 32-bit words.  Bit 255 is ignored and
// values >= p are accepted (reduced by the arithmetic), as Go's
// field.Element.SetBytes.
TMED_HD void fe_from_words(fe &h, const uint32_t w[8]) {
  const int off[10] = {0, 26, 51, 77, 102, 128, 153, 179, 204, 230};
  int64_t t[10];
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const int o = off[i], q = o >> 5, r = o & 31;
    const uint64_t lo = w[q];
    const uint64_t hi = (q + 1 < 8) ? (uint64_t)w[q + 1] : 0;
    const uint64_t x = ((hi << 32) | lo) >> r;
    const uint32_t mask = (i & 1) ? 0x1ffffffu : 0x3ffffffu;
    t[i] = (int64_t)(uint32_t)(x & mask) + fe_bias(i);
  }
  fe_carry64(h, t);
}

// Canonical encoding (fully reduced, 0 <= value < p) as 8 LE words.
TMED_HD void fe_to_words(uint32_t w[8], const fe &f) {
  int32_t h[10];
#pragma unroll
  for (int i = 0; i < 10; i++) h[i] = f.v[i];
  int32_t q = (19 * h[9] + (1 << 24)) >> 25;
#pragma unroll
  for (int i = 0; i < 10; i++) q = (h[i] + q) >> ((i & 1) ? 25 : 26);
  h[0] += 19 * q;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const int s = (i & 1) ? 25 : 26;
    const int32_t c = h[i] >> s;
    h[i + 1] += c;
    h[i] -= (int32_t)((uint32_t)c << s);
  }
  h[9] -= (int32_t)((uint32_t)(h[9] >> 25) << 25);
  const int off[10] = {0, 26, 51, 77, 102, 128, 153, 179, 204, 230};
  uint64_t acc[8];
#pragma unroll
  for (int i = 0; i < 8; i++) acc[i] = 0;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const int o = off[i], q2 = o >> 5, r = o & 31;
    const uint64_t x = (uint64_t)(uint32_t)h[i] << r;
    acc[q2] |= x & 0xffffffffu;
    if (q2 + 1 < 8) acc[q2 + 1] |= x >> 32;
  }
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = (uint32_t)acc[i];
}

// 256-bit storage form (the main kernel's per-lane tables: one 128-B line per cached point).
// Input: at most a 2-sum of carried values.  Limb 9 is first floor-carried with the
// 2^255 = 19 wrap (limb 9 in [0, 2^25), limb 0 grows by 19 * {-2..0}), then one floor-carry pass
// over limbs 0..8 without a wrap: limbs 0..8 end in [0, 2^26) / [0, 2^25) and limb 9 keeps that
// pass's carry (limb 9 in [-2, 2^25], 26 bits signed): 5*26 + 4*25 + 26 = 256 bits, at the same
// bit offsets as fe_from_words.  The value changes by a multiple of p only.
TMED_HD void fe_pack256(uint32_t w[8], const fe &f) {
  int32_t h[10];
#pragma unroll
  for (int i = 0; i < 10; i++) h[i] = f.v[i];
  {
    const int32_t c = h[9] >> 25;
    h[9] -= (int32_t)((uint32_t)c << 25);
    h[0] += mul19(c);
  }
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const int s = (i & 1) ? 25 : 26;
    const int32_t c = h[i] >> s;
    h[i] -= (int32_t)((uint32_t)c << s);
    h[i + 1] += c;
  }
  const uint32_t *u = reinterpret_cast<const uint32_t *>(h);
  w[0] = u[0] | (u[1] << 26);
  w[1] = (u[1] >> 6) | (u[2] << 19);
  w[2] = (u[2] >> 13) | (u[3] << 13);
  w[3] = (u[3] >> 19) | (u[4] << 6);
  w[4] = u[5] | (u[6] << 25);
  w[5] = (u[6] >> 7) | (u[7] << 19);
  w[6] = (u[7] >> 13) | (u[8] << 12);
  w[7] = (u[8] >> 20) | (u[9] << 6);
}

// Inverse of fe_pack256 (field extraction only, no carry): limbs at most twice a carried limb,
// inside the mul / sq operand bound of a 2-sum.
TMED_HD void fe_unpack256(fe &h, const uint32_t w[8]) {
  h.v[0] = (int32_t)(w[0] & 0x3ffffffu);
  h.v[1] = (int32_t)(((w[0] >> 26) | (w[1] << 6)) & 0x1ffffffu);
  h.v[2] = (int32_t)(((w[1] >> 19) | (w[2] << 13)) & 0x3ffffffu);
  h.v[3] = (int32_t)(((w[2] >> 13) | (w[3] << 19)) & 0x1ffffffu);
  h.v[4] = (int32_t)(w[3] >> 6);
  h.v[5] = (int32_t)(w[4] & 0x1ffffffu);
  h.v[6] = (int32_t)(((w[4] >> 25) | (w[5] << 7)) & 0x3ffffffu);
  h.v[7] = (int32_t)(((w[5] >> 19) | (w[6] << 13)) & 0x1ffffffu);
  h.v[8] = (int32_t)(((w[6] >> 12) | (w[7] << 20)) & 0x3ffffffu);
  h.v[9] = (int32_t)w[7] >> 6;
}

TMED_HD bool fe_isnegative(const fe &f) {
  uint32_t w[8];
  fe_to_words(w, f);
  return w[0] & 1;
}

TMED_HD bool fe_iszero(const fe &f) {
  uint32_t w[8];
  fe_to_words(w, f);
  uint32_t a = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) a |= w[i];
  return a == 0;
}

TMED_HD bool fe_equal(const fe &f, const fe &g) {
  fe d;
  fe_sub(d, f, g);
  fe_carry(d, d);
  return fe_iszero(d);
}

// Constants in carried form.
TMED_HD void fe_const_d(fe &h) {
  const int32_t c[10] = {-10913610, 13857413, -15372611, 6949391, 114729, -8787816, -6275908, -3247719, -18696448, -12055116};
#pragma unroll
  for (int i = 0; i < 10; i++) h.v[i] = c[i];
}
TMED_HD void fe_const_d2(fe &h) {
  const int32_t c[10] = {-21827239, -5839606, -30745221, 13898782, 229458, 15978800, -12551817, -6495438, 29715968, 9444199};
#pragma unroll
  for (int i = 0; i < 10; i++) h.v[i] = c[i];
}
TMED_HD void fe_const_sqrtm1(fe &h) {
  const int32_t c[10] = {-32595792, -7943725, 9377950, 3500415, 12389472, -272473, -25146209, -2005654, 326686, 11406482};
#pragma unroll
  for (int i = 0; i < 10; i++) h.v[i] = c[i];
}

// ---- inversion by binary GCD (Pornin's optimized binary GCD, IACR ePrint 2020/972) ----------
// z^-1 mod p from the binary extended GCD on (a, b) = (z, p): each inner iteration, if a is odd,
// subtracts the smaller of a, b from the larger (keeping b odd) and halves a; 30 iterations run on
// 64-bit approximations of a and b (their exact low 30 bits and the top 34 bits of the longer
// one), recording the transition matrix (f0 g0; f1 g1) (|entries| <= 2^30), which is then applied
// to the full a, b (9 limbs of 30 bits, two v_mad_i64_i32 per limb and output) and to the
// cofactors u, v (field elements: 2 mads per limb).  The cofactors are never halved: after the
// 18 x 30 = 540 iterations (>= 2 * 255 - 1, the bound for 255-bit operands), b = gcd = 1 and
// v = 2^540 / z, so one multiplication by 2^-540 finishes.  z = 0 gives 0, like z^(p-2).  About
// 15k VALU instructions, a third of them mads, against ~24k (15k mads) for the exponentiation;
// the branch-free inner loop keeps every lane of a wave on one instruction stream.
// (Replaces fe_invert in the batched finish: verify_core.h finish_group.)
constexpr uint32_t kM30 = 0x3fffffffu;
constexpr int kBgcdOuter = 18;

TMED_HD void w8_to_l30(uint32_t l[9], const uint32_t w[8]) {
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const int o = 30 * i, q = o >> 5, r = o & 31;
    const uint64_t x = (uint64_t)w[q] | ((q + 1 < 8) ? (uint64_t)w[q + 1] << 32 : 0ull);
    l[i] = (uint32_t)(x >> r) & kM30;
  }
}

// x = a >> s for a runtime s in [30, 240] (a < 2^(s + 34)): bits [30q, 30q + 64) of a, shifted
TMED_HD uint64_t l30_shr(const uint32_t a[9], int q, int r) {
  uint32_t s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
  for (int i = 1; i < 8; i++) {
    if (q == i) { s0 = a[i]; s1 = a[i + 1]; s2 = i + 2 < 9 ? a[i + 2] : 0u; }
  }
  const uint64_t t = (uint64_t)s0 | ((uint64_t)s1 << 30) | ((uint64_t)(s2 & 15u) << 60);
  return t >> r;
}

// (f a + g b) / 2^30 (exact: the low 30 bits cancel), with the sign folded out: returns the
// magnitude in r and negates (f, g) when the value was negative.
TMED_HD void l30_lincomb(uint32_t r[9], int32_t &f, int32_t &g, const uint32_t a[9], const uint32_t b[9]) {
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const int64_t t = (int64_t)f * (int32_t)a[i] + (int64_t)g * (int32_t)b[i] + c;
    if (i) r[i - 1] = (uint32_t)t & kM30;
    c = t >> 30;
  }
  const uint32_t m = c < 0 ? 0xffffffffu : 0u;  // negative: r = -r (two's complement over 30-bit limbs)
  r[8] = (uint32_t)c;
  uint32_t cy = m & 1u;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint32_t t = (r[i] ^ (m & kM30)) + cy;
    r[i] = t & kM30;
    cy = t >> 30;
  }
  r[8] = (r[8] ^ m) + cy;
  f = (int32_t)(((uint32_t)f ^ m) - m);
  g = (int32_t)(((uint32_t)g ^ m) - m);
}

// h = f0 x + g0 y (field elements, |f0|, |g0| <= 2^30; x, y carried)
TMED_HD void fe_lincomb(fe &h, int32_t f0, const fe &x, int32_t g0, const fe &y) {
  int64_t H[10];
#pragma unroll
  for (int k = 0; k < 10; k++) H[k] = fe_bias(k) + (int64_t)f0 * x.v[k] + (int64_t)g0 * y.v[k];
  fe_carry64(h, H);
}

TMED_HD void fe_invert_bgcd(fe &out, const fe &z) {
  uint32_t w[8], a[9], b[9];
  fe_to_words(w, z);
  w8_to_l30(a, w);
  const uint32_t pw[8] = {0xffffffedu, 0xffffffffu, 0xffffffffu, 0xffffffffu,
                          0xffffffffu, 0xffffffffu, 0xffffffffu, 0x7fffffffu};
  w8_to_l30(b, pw);
  fe u, v;
  fe_1(u);
  fe_0(v);
#pragma unroll 1
  for (int it = 0; it < kBgcdOuter; it++) {
    // n = max(len a, len b, 64); the approximations: exact low 30 bits, then a >> (n - 34)
    int top = 0;
#pragma unroll
    for (int i = 0; i < 9; i++)
      if (a[i] | b[i]) top = i;
    const uint32_t tl = a[top] | b[top];
    int n = 30 * top + 32 - __builtin_clz(tl | 1u);
    if (n < 64) n = 64;
    const int s = n - 34, q = s / 30, r = s - 30 * q;
    uint64_t xa = (uint64_t)a[0] | (l30_shr(a, q, r) << 30);
    uint64_t xb = (uint64_t)b[0] | (l30_shr(b, q, r) << 30);
    int32_t f0 = 1, g0 = 0, f1 = 0, g1 = 1;
#pragma unroll 1
    for (int j = 0; j < 30; j++) {
      const bool odd = (xa & 1u) != 0;
      const bool sw = odd && xa < xb;
      const uint64_t ta = sw ? xb : xa, tb = sw ? xa : xb;
      const int32_t tf0 = sw ? f1 : f0, tg0 = sw ? g1 : g0, tf1 = sw ? f0 : f1, tg1 = sw ? g0 : g1;
      xa = odd ? ta - tb : ta;
      xb = tb;
      f0 = odd ? tf0 - tf1 : tf0;
      g0 = odd ? tg0 - tg1 : tg0;
      f1 = tf1 * 2;
      g1 = tg1 * 2;
      xa >>= 1;
    }
    uint32_t na[9], nb[9];
    l30_lincomb(na, f0, g0, a, b);
    l30_lincomb(nb, f1, g1, a, b);
#pragma unroll
    for (int i = 0; i < 9; i++) { a[i] = na[i]; b[i] = nb[i]; }
    fe nu, nv;
    fe_lincomb(nu, f0, u, g0, v);
    fe_lincomb(nv, f1, u, g1, v);
    fe_copy(u, nu);
    fe_copy(v, nv);
  }
  // b = 1: v = 2^540 / z (the invariant b 2^540 = v z holds whatever the approximations decided:
  // every update is exact), times 2^-540 mod p.  b != 1 (z = 0, or an input the iteration count
  // did not bring down — none in 12M random and edge-case inputs, tests/test_kernel_host.py):
  // the exponentiation, on that lane only.
  uint32_t one = b[0] ^ 1u;
#pragma unroll
  for (int i = 1; i < 9; i++) one |= b[i];
  if (one != 0) {
    fe_invert(out, z);
    return;
  }
  const uint32_t kw[8] = {0x29d6dea8u, 0x827b63fdu, 0x788dd408u, 0x965683e6u,
                          0x3cfc744cu, 0x490aa31au, 0x24e016b1u, 0x1855b1b2u};
  fe k;
  fe_from_words(k, kw);
  fe_mul(out, v, k);
}

}  // namespace tmed
