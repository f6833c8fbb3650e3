// rows.h — the row forms the kernels exchange through global memory and LDS.
//
// A 128-B row is eight int4: 30 field words (three field elements of ten limbs) and two words of
// padding.  Comb and B-table entries keep affine niels points that way, the comb fill parks
// projective (X, Y, Z) in the row it is about to finish.  Next to them: the 40-word p3 form of the
// comb bases, the comb readers (GlobalComb, GlobalComb16) both kernel units use, and the
// [chunk q][slot] hand-offs between the prep, main and finish kernels.
// Everything here is __forceinline__: the callers' instruction streams do not depend on which
// helper spelled the loop.
#pragma once
#include "ge25519.h"
#include "kernels.h"

namespace tmed {

// Three field elements <- the row's eight int4, int4 q read at src[q * stride]: a table row
// (stride 1), a row already in registers (an int4[8], stride 1), or a wave's LDS region with lane
// l's piece q at q * 64 + l (src = region + l, stride 64).
__device__ __forceinline__ void row30_load(fe &a, fe &b, fe &c, const int4 *src, int stride = 1) {
  fe *fs[3] = {&a, &b, &c};
#pragma unroll
  for (int q = 0; q < kCombEntryInt4; q++) {
    const int4 v = src[q * stride];
    const int32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int f = 4 * q + i;
      if (f < 30) fs[f / 10]->v[f % 10] = w[i];
    }
  }
}
__device__ __forceinline__ void row30_store(int4 *dst, const fe &a, const fe &b, const fe &c) {
  const fe *fs[3] = {&a, &b, &c};
#pragma unroll
  for (int q = 0; q < kCombEntryInt4; q++) {
    int32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int f = 4 * q + i;
      w[i] = f < 30 ? fs[f / 10]->v[f % 10] : 0;
    }
    dst[q] = make_int4(w[0], w[1], w[2], w[3]);
  }
}

// affine niels row (Y+X, Y-X, 2dXY)
__device__ __forceinline__ void niels_load(ge_niels &e, const int4 *src, int stride = 1) {
  row30_load(e.YpX, e.YmX, e.XY2d, src, stride);
}
__device__ __forceinline__ void niels_store(int4 *dst, const ge_niels &e) { row30_store(dst, e.YpX, e.YmX, e.XY2d); }
// projective (X, Y, Z) parked in a comb row (comb_fill_run)
__device__ __forceinline__ void row_load_xyz(const int4 *row, fe &X, fe &Y, fe &Z) { row30_load(X, Y, Z, row); }
__device__ __forceinline__ void row_store_xyz(int4 *row, const ge_p3 &P) { row30_store(row, P.X, P.Y, P.Z); }

// A radix-256 comb (kernels.h kComb*) as comb_base_mult (verify_core.h) reads it.
struct GlobalComb {
  static constexpr int kBits = 8;
  const int4 *base;  // 32 windows x 129 entries x 8 int4
  __device__ __forceinline__ void load(int w, int j, ge_niels &e) const {
    niels_load(e, base + ((size_t)w * kCombEntries + j) * kCombEntryInt4);
  }
};

// Radix-2^16 comb of +B (the key-cached throughput kernel, the radix-2^24 / 2^26 builders):
// 16 windows x 32769 entries (j * 2^(16w) * B) x 8 int4 = 67 MB in HBM, built once per context.
struct GlobalComb16 {
  static constexpr int kBits = 16;
  const int4 *base;
  __device__ __forceinline__ void load(int w, int j, ge_niels &e) const {
    niels_load(e, base + ((size_t)w * kB16Entries + j) * kCombEntryInt4);
  }
};

// p3 as 40 words (X, Y, Z, T): the comb bases
TMED_HD void p3_store(int32_t *dst, const ge_p3 &p) {
  const fe *fs[4] = {&p.X, &p.Y, &p.Z, &p.T};
#pragma unroll
  for (int f = 0; f < 40; f++) dst[f] = fs[f / 10]->v[f % 10];
}
TMED_HD void p3_load(ge_p3 &p, const int32_t *src) {
  fe *fs[4] = {&p.X, &p.Y, &p.Z, &p.T};
#pragma unroll
  for (int f = 0; f < 40; f++) fs[f / 10]->v[f % 10] = src[f];
}

// Per-signature hand-off from the prep to the main kernel: k (words 0-7), s (8-15), A.x (16-25),
// A.y (26-35), ok (36): 37 words padded to 10 x int4, stored [chunk q][slot] for coalescing.
// (verify_prep_kernel writes it in two parts, k and s as soon as the hash is reduced.)
constexpr int kPrepInt4 = 10;

// The key-cached hand-off: only what verify_keyset_main_kernel reads (k, s in int4 0..3, ok at
// word 36 = int4 9): 80 B per signature instead of the generic prep's 160 B.
__device__ __forceinline__ void prep_store_ks(int4 *prep, uint32_t stride, uint32_t slot, const uint32_t k[8],
                                              const uint32_t s[8], bool ok) {
  prep[slot] = make_int4((int)k[0], (int)k[1], (int)k[2], (int)k[3]);
  prep[(size_t)stride + slot] = make_int4((int)k[4], (int)k[5], (int)k[6], (int)k[7]);
  prep[(size_t)2 * stride + slot] = make_int4((int)s[0], (int)s[1], (int)s[2], (int)s[3]);
  prep[(size_t)3 * stride + slot] = make_int4((int)s[4], (int)s[5], (int)s[6], (int)s[7]);
  prep[(size_t)9 * stride + slot] = make_int4(ok ? 1 : 0, 0, 0, 0);
}

__device__ __forceinline__ bool prep_load(const int4 *prep, uint32_t stride, uint32_t slot, uint32_t k[8],
                                          uint32_t s[8], ge_p3 &A) {
  int32_t w[40];
#pragma unroll
  for (int q = 0; q < kPrepInt4; q++) {
    const int4 v = prep[(size_t)q * stride + slot];
    w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
  }
#pragma unroll
  for (int i = 0; i < 8; i++) { k[i] = (uint32_t)w[i]; s[i] = (uint32_t)w[8 + i]; }
#pragma unroll
  for (int i = 0; i < 10; i++) { A.X.v[i] = w[16 + i]; A.Y.v[i] = w[26 + i]; }
  fe_1(A.Z);
  fe_mul(A.T, A.X, A.Y);
  return w[36] != 0;
}

// Projective R' of signature slot (X, Y, Z: 30 limbs + 2 pad = 8 int4), stored [q][slot].
__device__ __forceinline__ void fin_store(int4 *fin, uint32_t stride, uint32_t slot, const fe &X, const fe &Y,
                                          const fe &Z) {
  int32_t w[32];
#pragma unroll
  for (int i = 0; i < 10; i++) { w[i] = X.v[i]; w[10 + i] = Y.v[i]; w[20 + i] = Z.v[i]; }
  w[30] = w[31] = 0;
#pragma unroll
  for (int q = 0; q < kFinInt4; q++)
    fin[(size_t)q * stride + slot] = make_int4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
}

}  // namespace tmed
