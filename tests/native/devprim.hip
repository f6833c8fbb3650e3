// devprim.hip — TEST-ONLY device harness for the kernels' building blocks.
//
// Runs the __host__ __device__ primitives of tendermint-fork_amd/csrc (fe25519.h / fe_cols.h,
// sc25519.h, sha512.h, verify_hs.h, ge25519.h) on the GPU, one case per lane, so that the
// branches under `#if defined(__HIP_DEVICE_COMPILE__)` (the inline-asm mad schedules, the
// carry-chain builtins, the reciprocal quotient estimate, the SHA-512 bit operations and message
// reader) see the same edge inputs as the host build of tests/native/hostsim.cpp.  Never part of
// the product: nothing in libtmed25519_hip.so links or loads this file.
//
// The group layer one step above them: devprim_ge runs each point formula of ge25519.h and the
// group helpers of verify_core.h (ge_ops.h numbers them; hostsim_ge is the host twin) on raw
// limbs, one case per lane; devprim_quad runs quad.h (the DPP quad-lane formulas of the latency
// kernels and the ZIP-215 Horner chain, device-only code) one case per quad of lanes, single
// operations and chains of doublings and additions.  Both call the product's functions only.
//
// Every entry point copies its input arrays to the device, launches one kernel (blocks of 64,
// every lane guarded by i < n; devprim_quad guards whole quads), synchronises, copies the results
// back and returns the HIP error code (0 = hipSuccess).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "verify_core.h"
#include "verify_hs.h"
#include "quad.h"
#include "ge_ops.h"

using namespace tmed;

namespace {

constexpr int kBlock = 64;

// A device allocation freed on every path.
struct DevBuf {
  void *p = nullptr;
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
  hipError_t put(const void *src, size_t bytes) {
    hipError_t e = alloc(bytes);
    if (e == hipSuccess && bytes) e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
    return e;
  }
  hipError_t get(void *dst, size_t bytes) const {
    return bytes ? hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost) : hipSuccess;
  }
  template <class T>
  T *as() const { return (T *)p; }
  ~DevBuf() { if (p) (void)hipFree(p); }
};

inline unsigned grid_of(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

hipError_t finish_launch() {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return e;
}

#define DP_TRY(x)                       \
  do {                                  \
    const hipError_t e_ = (x);          \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)

__device__ void load_fe(fe &f, const int32_t *p) {
#pragma unroll
  for (int i = 0; i < 10; i++) f.v[i] = p[i];
}
__device__ void store_fe(int32_t *p, uint8_t *enc, const fe &f) {
#pragma unroll
  for (int i = 0; i < 10; i++) p[i] = f.v[i];
  uint32_t w[8];
  fe_to_words(w, f);
#pragma unroll
  for (int i = 0; i < 32; i++) enc[i] = (uint8_t)(w[i / 4] >> (8 * (i % 4)));
}
__device__ void store_words8(uint8_t *o, const uint32_t w[8]) {
#pragma unroll
  for (int i = 0; i < 32; i++) o[i] = (uint8_t)(w[i / 4] >> (8 * (i % 4)));
}

// op: 0 fe_mul, 1 fe_sq, 2 fe_sq2, 3 fe_sqc (first operand set only), 4 fe_mul_x2, 5 fe_sq_x2,
// 6 fe_sqc_x2, 7 fe_sq2_sq (both sets).  alias (pair forms): 0 = separate outputs, 1 = each output
// is its own first input, 2 = each output is its own last input, 3 = each output is the OTHER
// product's first input.
__global__ void fe_raw_kernel(int op, int alias, size_t n, const int32_t *a0, const int32_t *b0, const int32_t *a1,
                              const int32_t *b1, int32_t *o0, uint8_t *e0, int32_t *o1, uint8_t *e1) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  fe f0, g0, f1, g1, h0, h1;
  load_fe(f0, a0 + 10 * i);
  load_fe(g0, b0 + 10 * i);
  load_fe(f1, a1 + 10 * i);
  load_fe(g1, b1 + 10 * i);
  fe_0(h0);
  fe_0(h1);
  if (op < 4) {
    switch (op) {
      case 0: fe_mul(h0, f0, g0); break;
      case 1: fe_sq(h0, f0); break;
      case 2: fe_sq2(h0, f0); break;
      default: fe_sqc(h0, f0); break;
    }
    store_fe(o0 + 10 * i, e0 + 32 * i, h0);
    return;
  }
  const bool mul = op == 4;
  // the aliased calls write into the operand objects themselves
  fe *r0 = &h0, *r1 = &h1;
  if (alias == 1) { r0 = &f0; r1 = &f1; }
  if (alias == 2) { r0 = mul ? &g0 : &f0; r1 = mul ? &g1 : &f1; }
  if (alias == 3) { r0 = &f1; r1 = &f0; }
  switch (op) {
    case 4: fe_mul_x2(*r0, f0, g0, *r1, f1, g1); break;
    case 5: fe_sq_x2(*r0, f0, *r1, f1); break;
    case 6: fe_sqc_x2(*r0, f0, *r1, f1); break;
    default: fe_sq2_sq(*r0, f0, *r1, f1); break;
  }
  store_fe(o0 + 10 * i, e0 + 32 * i, *r0);
  store_fe(o1 + 10 * i, e1 + 32 * i, *r1);
}

// The ops of hostsim_fe_op, on 32-byte encodings.
__global__ void fe_bytes_kernel(int op, size_t n, const uint8_t *a, const uint8_t *b, uint8_t *out) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t wa[8], wb[8], wo[8];
  load_words8(wa, a + 32 * i);
  load_words8(wb, b + 32 * i);
  fe fa, fb, fo;
  fe_from_words(fa, wa);
  fe_from_words(fb, wb);
  switch (op) {
    case 0: fe_mul(fo, fa, fb); break;
    case 1: fe_sq(fo, fa); break;
    case 2: fe_invert(fo, fa); break;
    case 3: fe_pow22523(fo, fa); break;
    case 4: fe_add(fo, fa, fb); fe_carry(fo, fo); break;
    case 5: fe_sub(fo, fa, fb); fe_carry(fo, fo); break;
    case 6: fe_sq2(fo, fa); break;
    case 7: { fe t; fe_add(t, fa, fb); fe_add(t, t, fa); fe_mul(fo, t, t); break; }  // 3-sum input
    case 8: { fe t; fe_add(t, fa, fb); fe_add(t, t, fa); fe_sq(fo, t); break; }
    case 9: fe_invert_bgcd(fo, fa); break;
    default: fe_copy(fo, fa);
  }
  fe_to_words(wo, fo);
  store_words8(out + 32 * i, wo);
}

__global__ void pack256_kernel(size_t n, const int32_t *limbs, const uint8_t *g, int32_t *out_limbs, uint8_t *prod) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  fe f, u, gf, o;
  load_fe(f, limbs + 10 * i);
  uint32_t w[8], wg[8], wo[8];
  fe_pack256(w, f);
  fe_unpack256(u, w);
#pragma unroll
  for (int k = 0; k < 10; k++) out_limbs[10 * i + k] = u.v[k];
  load_words8(wg, g + 32 * i);
  fe_from_words(gf, wg);
  fe_mul(o, u, gf);
  fe_to_words(wo, o);
  store_words8(prod + 32 * i, wo);
}

__global__ void sc_reduce_kernel(size_t n, const uint8_t *x64, uint8_t *out) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t x[16], r[8];
  load_words8(x, x64 + 64 * i);
  load_words8(x + 8, x64 + 64 * i + 32);
  sc_reduce512(r, x);
  store_words8(out + 32 * i, r);
}

__global__ void sc_canonical_kernel(size_t n, const uint8_t *s32, uint8_t *out) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t s[8];
  load_words8(s, s32 + 32 * i);
  out[i] = sc_is_canonical(s) ? 1 : 0;
}

__global__ void sc_muladd_kernel(size_t n, const uint8_t *a32, const uint8_t *b32, const uint8_t *c32, uint8_t *out) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t a[8], b[8], c[8], r[8];
  load_words8(a, a32 + 32 * i);
  load_words8(b, b32 + 32 * i);
  load_words8(c, c32 + 32 * i);
  sc_muladd(r, a, b, c);
  store_words8(out + 32 * i, r);
}

__global__ void halfsize_kernel(size_t n, const uint8_t *k32, uint8_t *c32, uint8_t *d32, int32_t *dneg, int32_t *W,
                                int32_t *tight) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t k[8], c[8], dm[8];
  load_words8(k, k32 + 32 * i);
  bool neg;
  int wt = 0;
  const int w = sc_halfsize<true>(c, dm, neg, k, &wt);
  store_words8(c32 + 32 * i, c);
  store_words8(d32 + 32 * i, dm);
  dneg[i] = neg ? 1 : 0;
  W[i] = w;
  tight[i] = wt;
}

// SHA-512(p0 || p1 || M) with npre = 0, 32 or 64 prefix bytes; M = buf[off .. off + len).
__global__ void sha512_kernel(size_t n, int npre, const uint8_t *p0, const uint8_t *p1, const uint8_t *buf,
                              const uint32_t *off, const uint32_t *len, uint8_t *out) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t w0[8], w1[8], h[16];
  load_words8(w0, p0 + 32 * i);
  load_words8(w1, p1 + 32 * i);
  sha512_stream(h, w0, w1, npre, buf + off[i], len[i]);
  store_words8(out + 64 * i, h);
  store_words8(out + 64 * i + 32, h + 8);
}

// SHA-512(p0 || p1 || M) for M at the start of lane i's 256-byte, 16-byte aligned slot.
__global__ void sha512_slot_kernel(size_t n, const uint8_t *p0, const uint8_t *p1, const uint8_t *slots,
                                   const uint32_t *len, uint8_t *out) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t w0[8], w1[8], h[16];
  load_words8(w0, p0 + 32 * i);
  load_words8(w1, p1 + 32 * i);
  sha512_stream_slot(h, w0, w1, slots + 256 * i, len[i]);
  store_words8(out + 64 * i, h);
  store_words8(out + 64 * i + 32, h + 8);
}

__global__ void decode_kernel(size_t n, const uint8_t *p, uint8_t *ok, uint8_t *enc) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8], e[8];
  load_words8(w, p + 32 * i);
  ge_p3 A;
  const bool good = ge_frombytes_go(A, w);
  ge_tobytes(e, A.X, A.Y, A.Z);
  store_words8(enc + 32 * i, e);
  ok[i] = good ? 1 : 0;
}

// One group-layer call (ge_ops.h) per lane: in [n][8][10], out [n][4][10], enc [n][4][32].
template <int OP>
__global__ void ge_kernel(int neg, size_t n, const int32_t *in, int32_t *out, uint8_t *enc) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  fe fi[8], fo[4];
#pragma unroll
  for (int k = 0; k < 8; k++) load_fe(fi[k], in + 80 * i + 10 * k);
  ge_op_run<OP>(neg != 0, fi, fo);
#pragma unroll
  for (int k = 0; k < 4; k++) store_fe(out + 40 * i + 10 * k, enc + 128 * i + 32 * k, fo[k]);
}

constexpr int kQuadOps = 7;
constexpr int kChainSteps = 16;    // steps of a chain program
constexpr uint32_t kChainMaxDbl = 16;  // doublings per step

// quad.h, one case per quad: lane 4c + r holds field element r of case c.  in [n][2][4][10] (the
// point v, the cached operand q), out [n][4][10].  op: 0 quad_dbl(v), 1 quad_add(v, q),
// 2 quad_to_cached(v), 3 quad_identity, 4 quad_identity_cached, 5 comb_take(window, dg[c]),
// 6 chain: from quad_identity, step s of prog[c][0..16) = ndbl | sel << 8 runs ndbl x quad_dbl,
// then quad_add of v (sel 1), of q (sel 2) or nothing (sel 0); v and q are both cached operands.
__global__ void quad_kernel(int op, size_t n, const int32_t *in, const int4 *window, const int32_t *dg,
                            const uint32_t *prog, int32_t *out) {
  const size_t c = ((size_t)blockIdx.x * kBlock + threadIdx.x) >> 2;
  if (c >= n) return;  // the four lanes of a quad share c: a quad is wholly active or wholly idle
  const QuadK K((int)threadIdx.x);
  fe v, q, o;
  load_fe(v, in + 80 * c + 10 * K.r);
  load_fe(q, in + 80 * c + 40 + 10 * K.r);
  fe_0(o);
  switch (op) {
    case 0: quad_dbl(v, K); o = v; break;
    case 1: quad_add(v, q, K); o = v; break;
    case 2: quad_to_cached(o, v, K); break;
    case 3: quad_identity(o, K.r); break;
    case 4: quad_identity_cached(o, K.r); break;
    case 5: comb_take(o, window, dg[c], K); break;
    default: {
      quad_identity(o, K.r);
#pragma unroll 1
      for (int s = 0; s < kChainSteps; s++) {
        const uint32_t st = prog[kChainSteps * c + s];
        const uint32_t nd = st & 0xffu, sel = st >> 8;
#pragma unroll 1
        for (uint32_t k = 0; k < nd; k++) quad_dbl(o, K);
        if (sel == 1) quad_add(o, v, K);
        else if (sel == 2) quad_add(o, q, K);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 10; i++) out[40 * c + 10 * K.r + i] = o.v[i];
}

}  // namespace

extern "C" {

// The group-layer functions (ge_ops.h: op 0..9; neg 0 / 1 where the function takes it), one case
// per lane: in n x 8 x 10 raw limbs, out n x 4 x 10 raw output limbs, enc n x 4 x 32 their
// canonical encodings.
int devprim_ge(int op, int neg, size_t n, const int32_t *in, int32_t *out, uint8_t *enc) {
  if (n == 0) return 0;
  if (op < 0 || op >= kGeOps || neg < 0 || neg > 1) return (int)hipErrorInvalidValue;
  DevBuf din, dout, denc;
  DP_TRY(din.put(in, 320 * n));
  DP_TRY(dout.alloc(160 * n));
  DP_TRY(denc.alloc(128 * n));
  const unsigned g = grid_of(n);
  int32_t *o = dout.as<int32_t>();
  uint8_t *e = denc.as<uint8_t>();
  const int32_t *i = din.as<int32_t>();
  switch (op) {
    case 0: ge_kernel<0><<<g, kBlock>>>(neg, n, i, o, e); break;
    case 1: ge_kernel<1><<<g, kBlock>>>(neg, n, i, o, e); break;
    case 2: ge_kernel<2><<<g, kBlock>>>(neg, n, i, o, e); break;
    case 3: ge_kernel<3><<<g, kBlock>>>(neg, n, i, o, e); break;
    case 4: ge_kernel<4><<<g, kBlock>>>(neg, n, i, o, e); break;
    case 5: ge_kernel<5><<<g, kBlock>>>(neg, n, i, o, e); break;
    case 6: ge_kernel<6><<<g, kBlock>>>(neg, n, i, o, e); break;
    case 7: ge_kernel<7><<<g, kBlock>>>(neg, n, i, o, e); break;
    case 8: ge_kernel<8><<<g, kBlock>>>(neg, n, i, o, e); break;
    default: ge_kernel<9><<<g, kBlock>>>(neg, n, i, o, e); break;
  }
  DP_TRY(finish_launch());
  DP_TRY(dout.get(out, 160 * n));
  DP_TRY(denc.get(enc, 128 * n));
  return 0;
}

// quad.h, one case per quad of lanes (see quad_kernel): in n x 2 x 4 x 10, out n x 4 x 10.
// window: nrows synthetic 128-byte comb rows (32 int32 each: YpX, YmX, XY2d, two unused) and
// dg[n] the per-case digit, |dg| < nrows, read by op 5 only; prog n x 16 chain steps, read by
// op 6 only (at most 16 doublings a step, sel 0..2).  Unused arrays may be null.
int devprim_quad(int op, size_t n, const int32_t *in, const int32_t *window, size_t nrows, const int32_t *dg,
                 const uint32_t *prog, int32_t *out) {
  if (n == 0) return 0;
  if (op < 0 || op >= kQuadOps) return (int)hipErrorInvalidValue;
  if (op == 5) {
    if (!window || !dg || nrows == 0) return (int)hipErrorInvalidValue;
    for (size_t c = 0; c < n; c++) {
      const int64_t d = dg[c];
      if ((d < 0 ? -d : d) >= (int64_t)nrows) return (int)hipErrorInvalidValue;
    }
  }
  if (op == 6) {
    if (!prog) return (int)hipErrorInvalidValue;
    for (size_t k = 0; k < (size_t)kChainSteps * n; k++)
      if ((prog[k] & 0xffu) > kChainMaxDbl || (prog[k] >> 8) > 2) return (int)hipErrorInvalidValue;
  }
  DevBuf din, dwin, ddg, dprog, dout;
  DP_TRY(din.put(in, 320 * n));
  DP_TRY(dwin.put(window, op == 5 ? 128 * nrows : 0));
  DP_TRY(ddg.put(dg, op == 5 ? 4 * n : 0));
  DP_TRY(dprog.put(prog, op == 6 ? 4 * (size_t)kChainSteps * n : 0));
  DP_TRY(dout.alloc(160 * n));
  quad_kernel<<<grid_of(4 * n), kBlock>>>(op, n, din.as<int32_t>(), dwin.as<int4>(), ddg.as<int32_t>(),
                                          dprog.as<uint32_t>(), dout.as<int32_t>());
  DP_TRY(finish_launch());
  DP_TRY(dout.get(out, 160 * n));
  return 0;
}

// Raw signed limbs (10 per operand, n cases): result limbs and canonical encodings out.  The
// single-operand ops (op < 4) read a0 / b0 and write out0 / enc0 only; the second set's arrays
// must still be valid (n x 10 / n x 32).
int devprim_fe_raw(int op, int alias, size_t n, const int32_t *a0, const int32_t *b0, const int32_t *a1,
                   const int32_t *b1, int32_t *out0, uint8_t *enc0, int32_t *out1, uint8_t *enc1) {
  if (n == 0) return 0;
  if (op < 0 || op > 7 || alias < 0 || alias > 3) return (int)hipErrorInvalidValue;
  DevBuf da0, db0, da1, db1, do0, de0, do1, de1;
  const size_t lb = 40 * n, eb = 32 * n;
  DP_TRY(da0.put(a0, lb));
  DP_TRY(db0.put(b0, lb));
  DP_TRY(da1.put(a1, lb));
  DP_TRY(db1.put(b1, lb));
  DP_TRY(do0.alloc(lb));
  DP_TRY(de0.alloc(eb));
  DP_TRY(do1.alloc(lb));
  DP_TRY(de1.alloc(eb));
  DP_TRY(hipMemset(do1.p, 0, lb));
  DP_TRY(hipMemset(de1.p, 0, eb));
  fe_raw_kernel<<<grid_of(n), kBlock>>>(op, alias, n, da0.as<int32_t>(), db0.as<int32_t>(), da1.as<int32_t>(),
                                        db1.as<int32_t>(), do0.as<int32_t>(), de0.as<uint8_t>(), do1.as<int32_t>(),
                                        de1.as<uint8_t>());
  DP_TRY(finish_launch());
  DP_TRY(do0.get(out0, lb));
  DP_TRY(de0.get(enc0, eb));
  DP_TRY(do1.get(out1, lb));
  DP_TRY(de1.get(enc1, eb));
  return 0;
}

int devprim_fe_bytes(int op, size_t n, const uint8_t *a, const uint8_t *b, uint8_t *out) {
  if (n == 0) return 0;
  DevBuf da, db, dout;
  DP_TRY(da.put(a, 32 * n));
  DP_TRY(db.put(b, 32 * n));
  DP_TRY(dout.alloc(32 * n));
  fe_bytes_kernel<<<grid_of(n), kBlock>>>(op, n, da.as<uint8_t>(), db.as<uint8_t>(), dout.as<uint8_t>());
  DP_TRY(finish_launch());
  DP_TRY(dout.get(out, 32 * n));
  return 0;
}

// hostsim_pack256 over n cases: limbs n x 10, g n x 32 -> unpacked limbs n x 10, product n x 32.
int devprim_pack256(size_t n, const int32_t *limbs, const uint8_t *g, int32_t *out_limbs, uint8_t *prod) {
  if (n == 0) return 0;
  DevBuf dl, dg, dol, dp;
  DP_TRY(dl.put(limbs, 40 * n));
  DP_TRY(dg.put(g, 32 * n));
  DP_TRY(dol.alloc(40 * n));
  DP_TRY(dp.alloc(32 * n));
  pack256_kernel<<<grid_of(n), kBlock>>>(n, dl.as<int32_t>(), dg.as<uint8_t>(), dol.as<int32_t>(), dp.as<uint8_t>());
  DP_TRY(finish_launch());
  DP_TRY(dol.get(out_limbs, 40 * n));
  DP_TRY(dp.get(prod, 32 * n));
  return 0;
}

int devprim_sc_reduce(size_t n, const uint8_t *x64, uint8_t *out) {
  if (n == 0) return 0;
  DevBuf dx, dout;
  DP_TRY(dx.put(x64, 64 * n));
  DP_TRY(dout.alloc(32 * n));
  sc_reduce_kernel<<<grid_of(n), kBlock>>>(n, dx.as<uint8_t>(), dout.as<uint8_t>());
  DP_TRY(finish_launch());
  DP_TRY(dout.get(out, 32 * n));
  return 0;
}

int devprim_sc_is_canonical(size_t n, const uint8_t *s32, uint8_t *out) {
  if (n == 0) return 0;
  DevBuf ds, dout;
  DP_TRY(ds.put(s32, 32 * n));
  DP_TRY(dout.alloc(n));
  sc_canonical_kernel<<<grid_of(n), kBlock>>>(n, ds.as<uint8_t>(), dout.as<uint8_t>());
  DP_TRY(finish_launch());
  DP_TRY(dout.get(out, n));
  return 0;
}

int devprim_sc_muladd(size_t n, const uint8_t *a, const uint8_t *b, const uint8_t *c, uint8_t *out) {
  if (n == 0) return 0;
  DevBuf da, db, dc, dout;
  DP_TRY(da.put(a, 32 * n));
  DP_TRY(db.put(b, 32 * n));
  DP_TRY(dc.put(c, 32 * n));
  DP_TRY(dout.alloc(32 * n));
  sc_muladd_kernel<<<grid_of(n), kBlock>>>(n, da.as<uint8_t>(), db.as<uint8_t>(), dc.as<uint8_t>(), dout.as<uint8_t>());
  DP_TRY(finish_launch());
  DP_TRY(dout.get(out, 32 * n));
  return 0;
}

// sc_halfsize<true> over n scalars k (n x 32): c, |d| (n x 32 each), dneg, W, tight (n each).
int devprim_halfsize(size_t n, const uint8_t *k32, uint8_t *c32, uint8_t *d32, int32_t *dneg, int32_t *W,
                     int32_t *tight) {
  if (n == 0) return 0;
  DevBuf dk, dc, dd, dn, dw, dt;
  DP_TRY(dk.put(k32, 32 * n));
  DP_TRY(dc.alloc(32 * n));
  DP_TRY(dd.alloc(32 * n));
  DP_TRY(dn.alloc(4 * n));
  DP_TRY(dw.alloc(4 * n));
  DP_TRY(dt.alloc(4 * n));
  halfsize_kernel<<<grid_of(n), kBlock>>>(n, dk.as<uint8_t>(), dc.as<uint8_t>(), dd.as<uint8_t>(), dn.as<int32_t>(),
                                          dw.as<int32_t>(), dt.as<int32_t>());
  DP_TRY(finish_launch());
  DP_TRY(dc.get(c32, 32 * n));
  DP_TRY(dd.get(d32, 32 * n));
  DP_TRY(dn.get(dneg, 4 * n));
  DP_TRY(dw.get(W, 4 * n));
  DP_TRY(dt.get(tight, 4 * n));
  return 0;
}

// Messages M_i = buf[off[i] .. off[i] + len[i]) of one device copy of buf (buflen bytes, padded on
// the device to the dword the reader's last aligned load ends at), so off[i] % 4 is the lane's
// misalignment.  npre = 0, 32 or 64 bytes of prefix (p0, then p1; n x 32 each).
int devprim_sha512(size_t n, int npre, const uint8_t *p0, const uint8_t *p1, const uint8_t *buf, size_t buflen,
                   const uint32_t *off, const uint32_t *len, uint8_t *out) {
  if (n == 0) return 0;
  if (npre != 0 && npre != 32 && npre != 64) return (int)hipErrorInvalidValue;
  for (size_t i = 0; i < n; i++)
    if ((size_t)off[i] + len[i] > buflen) return (int)hipErrorInvalidValue;
  DevBuf d0, d1, dbuf, doff, dlen, dout;
  DP_TRY(d0.put(p0, 32 * n));
  DP_TRY(d1.put(p1, 32 * n));
  DP_TRY(dbuf.alloc(buflen + 8));
  DP_TRY(hipMemset(dbuf.p, 0, buflen + 8));
  if (buflen) DP_TRY(hipMemcpy(dbuf.p, buf, buflen, hipMemcpyHostToDevice));
  DP_TRY(doff.put(off, 4 * n));
  DP_TRY(dlen.put(len, 4 * n));
  DP_TRY(dout.alloc(64 * n));
  sha512_kernel<<<grid_of(n), kBlock>>>(n, npre, d0.as<uint8_t>(), d1.as<uint8_t>(), dbuf.as<uint8_t>(),
                                        doff.as<uint32_t>(), dlen.as<uint32_t>(), dout.as<uint8_t>());
  DP_TRY(finish_launch());
  DP_TRY(dout.get(out, 64 * n));
  return 0;
}

// sha512_stream_slot: message i is the first len[i] (<= 256) bytes of slots[256 i .. 256 i + 256).
int devprim_sha512_slot(size_t n, const uint8_t *p0, const uint8_t *p1, const uint8_t *slots, const uint32_t *len,
                        uint8_t *out) {
  if (n == 0) return 0;
  for (size_t i = 0; i < n; i++)
    if (len[i] > 256) return (int)hipErrorInvalidValue;
  DevBuf d0, d1, ds, dlen, dout;
  DP_TRY(d0.put(p0, 32 * n));
  DP_TRY(d1.put(p1, 32 * n));
  DP_TRY(ds.put(slots, 256 * n));
  DP_TRY(dlen.put(len, 4 * n));
  DP_TRY(dout.alloc(64 * n));
  sha512_slot_kernel<<<grid_of(n), kBlock>>>(n, d0.as<uint8_t>(), d1.as<uint8_t>(), ds.as<uint8_t>(),
                                             dlen.as<uint32_t>(), dout.as<uint8_t>());
  DP_TRY(finish_launch());
  DP_TRY(dout.get(out, 64 * n));
  return 0;
}

// ge_frombytes_go + ge_tobytes (hostsim_decode) over n encodings.
int devprim_decode(size_t n, const uint8_t *p, uint8_t *ok, uint8_t *enc) {
  if (n == 0) return 0;
  DevBuf dp, dok, denc;
  DP_TRY(dp.put(p, 32 * n));
  DP_TRY(dok.alloc(n));
  DP_TRY(denc.alloc(32 * n));
  decode_kernel<<<grid_of(n), kBlock>>>(n, dp.as<uint8_t>(), dok.as<uint8_t>(), denc.as<uint8_t>());
  DP_TRY(finish_launch());
  DP_TRY(dok.get(ok, n));
  DP_TRY(denc.get(enc, 32 * n));
  return 0;
}

}  // extern "C"
