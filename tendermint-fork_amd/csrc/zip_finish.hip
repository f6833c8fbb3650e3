// zip_finish.hip — the finishes of the key-cached routes under the ZIP-215 rule (zip_finish.h): one
// lane per signature, after the unchanged prep and main kernels of the throughput route
// (launch_finish_zip) and after the unchanged latency kernel (launch_lat_finish_zip).  A unit of
// its own: nothing here hashes, and the default rule's kernels in kernels.hip compile exactly as
// without it.
#include "kernels.h"
#include "kernel_util.h"
#include "zip_finish.h"

namespace tmed {

// Position p < m: P from fin slot p ([q][slot], fin_store's layout), R from the signature row of
// index fin_base + p (perm[fin_base + p] in the key-grouped order), out[index] &= the decision.
// No inversion and nothing shared between lanes: the cost is R's decompression (one pow22523 chain
// of ~254 dependent squarings), so the lanes are latency-bound chains that want other waves to issue
// from.  R is decoded before P is loaded, which keeps P's thirty limbs out of the chain's live set:
// 161 VGPRs, no scratch, three waves a SIMD.  Four waves (128 VGPRs) spill 47 registers into the
// squaring chain; P loaded first needs 185 VGPRs (two waves).
constexpr int kZipFinWaves = 3;
__global__ __launch_bounds__(kThreadsPerBlock, kZipFinWaves) void keyset_finish_zip_kernel(
    const int4 *__restrict__ fin, const uint8_t *__restrict__ sig, uint8_t *__restrict__ out, uint32_t fin_base,
    uint32_t m, const uint32_t *__restrict__ perm) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const uint32_t i = perm ? perm[fin_base + p] : fin_base + p;
  uint32_t Rw[8];
  load_row_words(Rw, sig + 64 * (size_t)i, 2);
  ge_p3 R;
  const bool r_ok = ge_frombytes_go(R, Rw);
  int32_t w[32];
#pragma unroll
  for (int q = 0; q < kFinInt4; q++) {
    const int4 t = fin[(size_t)q * kFinCap + p];
    w[4 * q] = t.x; w[4 * q + 1] = t.y; w[4 * q + 2] = t.z; w[4 * q + 3] = t.w;
  }
  fe X, Y, Z;
#pragma unroll
  for (int j = 0; j < 10; j++) { X.v[j] = w[j]; Y.v[j] = w[10 + j]; Z.v[j] = w[20 + j]; }
  const bool ok = zip_finish_check(X, Y, Z, R, r_ok, out[i] != 0);
  out[i] = ok ? 1 : 0;
}

hipError_t launch_finish_zip(const int4 *fin, const uint8_t *sig, uint8_t *out, uint32_t fin_base, uint32_t m,
                             hipStream_t stream, const uint32_t *perm) {
  if (m == 0) return hipSuccess;
  if (m > kFinCap) return hipErrorInvalidValue;  // fin holds kFinCap slots
  hipLaunchKernelGGL(keyset_finish_zip_kernel, dim3((m + kThreadsPerBlock - 1) / kThreadsPerBlock),
                     dim3(kThreadsPerBlock), 0, stream, fin, sig, out, fin_base, m, perm);
  return hipGetLastError();
}

// The latency route's finish under the rule.  verify_keyset_lat_kernel's R blocks run as they do
// under the Go rule, beside the comb sum: they decode R (Point.SetBytes, the permissive decoding)
// and store (x, y) with a flag that also asks for a canonical encoding.  Where the flag is set, R is
// that point and the finish is the short part alone (P - R, three doublings: no decompression chain
// behind the comb sum).  Where it is not, the bytes either do not decode (rejected here, no chain)
// or are a non-canonical encoding, which ZIP-215 accepts: only then does the lane decode R itself.
// Such encodings appear in adversarial input alone, and only their waves pay the chain.
__global__ __launch_bounds__(kThreadsPerBlock) void keyset_lat_finish_zip_kernel(
    const int4 *__restrict__ fin, const int4 *__restrict__ dec, const uint8_t *__restrict__ sig, uint32_t m,
    uint8_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  int32_t w[32];
#pragma unroll
  for (int q = 0; q < kLatDecRows; q++) {
    const int4 t = dec[(size_t)q * m + i];
    w[4 * q] = t.x; w[4 * q + 1] = t.y; w[4 * q + 2] = t.z; w[4 * q + 3] = t.w;
  }
  ge_p3 R;
  bool r_ok = w[20] != 0;
  if (r_ok) {
#pragma unroll
    for (int j = 0; j < 10; j++) { R.X.v[j] = w[j]; R.Y.v[j] = w[10 + j]; }
    fe_1(R.Z);
    fe_mul(R.T, R.X, R.Y);
  } else {
    // The flag is clear for bytes that do not decode and for non-canonical encodings of a point:
    // y >= p, or x = 0 (y = 1 or y = p - 1) with the sign bit set (verify_core.h r_strict_extra).
    // Only the latter can still be accepted, so only those bytes are decoded here; a flipped R,
    // the common invalid signature, is rejected without the chain.
    uint32_t Rw[8];
    load_row_words(Rw, sig + 64 * (size_t)i, 2);
    const uint32_t top = Rw[7] & 0x7fffffffu;
    bool mid_ones = true, mid_zero = true;
#pragma unroll
    for (int j = 1; j < 7; j++) {
      mid_ones = mid_ones && Rw[j] == 0xffffffffu;
      mid_zero = mid_zero && Rw[j] == 0u;
    }
    const bool y_ge_p = mid_ones && top == 0x7fffffffu && Rw[0] >= 0xffffffedu;
    const bool y_is_1 = mid_zero && top == 0u && Rw[0] == 1u;
    const bool y_is_m1 = mid_ones && top == 0x7fffffffu && Rw[0] == 0xffffffecu;
    const bool noncanonical = y_ge_p || ((Rw[7] >> 31) != 0 && (y_is_1 || y_is_m1));
    if (noncanonical) {
      r_ok = ge_frombytes_go(R, Rw);
    } else {
      ge_p3_0(R);  // r_ok stays false: the arithmetic below stays defined, the decision is masked
    }
  }
#pragma unroll
  for (int q = 0; q < kFinInt4; q++) {
    const int4 t = fin[(size_t)q * kFinCap + i];
    w[4 * q] = t.x; w[4 * q + 1] = t.y; w[4 * q + 2] = t.z; w[4 * q + 3] = t.w;
  }
  fe X, Y, Z;
#pragma unroll
  for (int j = 0; j < 10; j++) { X.v[j] = w[j]; Y.v[j] = w[10 + j]; Z.v[j] = w[20 + j]; }
  const bool ok = zip_finish_check(X, Y, Z, R, r_ok, out[i] != 0);
  out[i] = ok ? 1 : 0;
}

hipError_t launch_lat_finish_zip(const int4 *fin, const int4 *dec, const uint8_t *sig, uint8_t *out, uint32_t m,
                                 hipStream_t stream) {
  if (m == 0) return hipSuccess;
  if (m > kFinCap) return hipErrorInvalidValue;
  hipLaunchKernelGGL(keyset_lat_finish_zip_kernel, dim3((m + kThreadsPerBlock - 1) / kThreadsPerBlock),
                     dim3(kThreadsPerBlock), 0, stream, fin, dec, sig, m, out);
  return hipGetLastError();
}

}  // namespace tmed
