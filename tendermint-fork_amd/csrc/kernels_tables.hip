// kernels_tables.hip — gfx950 kernels that run once per context or per key set: the shared
// tables of B and the key sets' combs of -A.  Rows are 128-B affine niels entries (rows.h).
#include "kernels.h"
#include "verify_core.h"
#include "kernel_util.h"
#include "rows.h"

namespace tmed {

// j*B for j = 0..kB16Entries-1 into 128-B rows (one lane per entry; once per context).
__global__ __launch_bounds__(256) void b16_fill_kernel(int4 *__restrict__ tab) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= kB16Entries) return;
  ge_niels e;
  if (j == 0) {
    ge_niels_0(e);
  } else {
    ge_p3 B;
    ge_base_point(B);
    comb_entry(e, B, j, 16);
  }
  niels_store(tab + (size_t)j * kCombEntryInt4, e);
}

hipError_t launch_build_b16(int4 *tab, hipStream_t stream) {
  hipLaunchKernelGGL(b16_fill_kernel, dim3((kB16Entries + 255) / 256), dim3(256), 0, stream, tab);
  return hipGetLastError();
}

// ============================================================ fixed-base combs

__global__ __launch_bounds__(64) void comb_bases_kernel(const uint8_t *__restrict__ pubs, uint32_t n, int negate,
                                                       uint8_t *__restrict__ ok_out, int32_t *__restrict__ bases) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t pw[8];
  load_row_words(pw, pubs + 32 * (size_t)i, 2);
  ge_p3 P;
  const bool ok = ge_frombytes_go(P, pw);
  ok_out[i] = ok ? 1 : 0;
  if (negate) { fe_neg(P.X, P.X); fe_neg(P.T, P.T); }
#pragma unroll 1
  for (int w = 0; w < kCombWindows; w++) {
    p3_store(bases + ((size_t)i * kCombWindows + w) * 40, P);
    ge_mul256(P);
  }
}

// Comb entries in runs of kCombARun consecutive j per lane: the run's first entry j0 * base by
// double-and-add over nbits bits of j0, the next ones by one cached addition each (8 M), the run's
// projective points parked in their own comb rows (X, Y, Z: 30 of the row's 32 words) and their
// prefix products of Z in LDS, ONE inversion per run (Montgomery's trick: 3 M per entry), then
// each row rewritten in affine niels form.  ~6k mads per entry against ~34k for a double-and-add
// and an inversion per entry (the round-5 radix-2^12 comb of 10k keys: 1.6 s of device time that
// way, 98 ms like this — profiles/r05/final/ and s14/ kernel_stats.csv).
constexpr uint32_t kCombARun = 8;
// rows[j] = j * base for j = j0 .. j0 + kCombARun - 1 (rows: the window's entry 0; base: p3 words;
// pre: this block's LDS, 64 lanes)
__device__ __forceinline__ void comb_fill_run(int4 *rows, const int32_t *base, uint32_t j0, int nbits,
                              fe (*pre)[64], uint32_t lane) {
  ge_p3 B, P;
  p3_load(B, base);
  ge_cached cB;
  ge_p3_to_cached(cB, B);
  {  // P = j0 * B, double-and-add over j0's bits
    ge_p3 sum;
    ge_p1p1 t;
    ge_p2 q;
    ge_p3_0(P);
#pragma unroll 1
    for (int b = nbits - 1; b >= 0; b--) {
      ge_p3_to_p2(q, P);
      ge_p2_dbl(t, q);
      ge_p1p1_to_p3(P, t);
      ge_add_cached(t, P, cB, false);
      ge_p1p1_to_p3(sum, t);
      const bool bit = (j0 >> b) & 1u;
      fe_select(P.X, P.X, sum.X, bit);
      fe_select(P.Y, P.Y, sum.Y, bit);
      fe_select(P.Z, P.Z, sum.Z, bit);
      fe_select(P.T, P.T, sum.T, bit);
    }
  }
  fe acc;
#pragma unroll 1
  for (uint32_t t = 0; t < kCombARun; t++) {
    if (t) {
      ge_p1p1 s;
      ge_add_cached(s, P, cB, false);
      ge_p1p1_to_p3(P, s);
      fe_mul(acc, acc, P.Z);
    } else {
      fe_copy(acc, P.Z);
    }
    row_store_xyz(rows + (size_t)(j0 + t) * kCombEntryInt4, P);
    pre[t][lane] = acc;
  }
  fe inv, d2;
  fe_invert_bgcd(inv, acc);
  fe_const_d2(d2);
#pragma unroll 1
  for (int t = (int)kCombARun - 1; t >= 0; t--) {
    int4 *r = rows + (size_t)(j0 + t) * kCombEntryInt4;
    fe X, Y, Z, zi, x, y, xy;
    row_load_xyz(r, X, Y, Z);
    if (t) {
      fe_mul(zi, inv, pre[t - 1][lane]);
      fe_mul(inv, inv, Z);
    } else {
      fe_copy(zi, inv);
    }
    fe_mul_x2(x, X, zi, y, Y, zi);
    ge_niels e;
    fe_add(e.YpX, y, x); fe_carry(e.YpX, e.YpX);
    fe_sub(e.YmX, y, x); fe_carry(e.YmX, e.YmX);
    fe_mul(xy, x, y);
    fe_mul(e.XY2d, xy, d2);
    niels_store(r, e);
  }
}
// the bit length of a run's largest start 1 + kCombARun (runs - 1)
constexpr int comb_start_bits(uint32_t runs) {
  int b = 0;
  for (uint32_t v = 1 + kCombARun * (runs - 1); v; v >>= 1) b++;
  return b;
}

// The radix-256 comb: 16 runs of 8 per (key, window) (j = 1..128), four windows per 64-lane block.
constexpr uint32_t kCombRuns = (kCombEntries - 1) / kCombARun;  // 16
static_assert((kCombEntries - 1) % kCombARun == 0 && 64 % kCombRuns == 0, "radix-256 comb runs");
__global__ __launch_bounds__(64) void comb_fill_kernel(const int32_t *__restrict__ bases, uint32_t n,
                                                       int4 *__restrict__ comb) {
  __shared__ fe pre[kCombARun][64];
  const uint32_t kw = blockIdx.x * (64 / kCombRuns) + threadIdx.x / kCombRuns;  // key * 32 + window
  const uint32_t run = threadIdx.x % kCombRuns;
  if (kw >= n * kCombWindows) return;
  int4 *rows = comb + (size_t)kw * kCombEntries * kCombEntryInt4;
  if (run == 0) {
    ge_niels id;
    ge_niels_0(id);
    niels_store(rows, id);
  }
  comb_fill_run(rows, bases + (size_t)kw * 40, 1u + kCombARun * run, comb_start_bits(kCombRuns), pre, threadIdx.x);
}

// Lane (w, j) of the radix-2^16 B comb: j * bases[w] (bases[w] = 2^(16w) B, p3 words).
__global__ __launch_bounds__(256) void bcomb16_fill_kernel(const int32_t *__restrict__ bases, int4 *__restrict__ comb) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= 16u * kB16Entries) return;
  const uint32_t w = g / kB16Entries, j = g % kB16Entries;
  ge_niels e;
  if (j == 0) {
    ge_niels_0(e);
  } else {
    ge_p3 P;
    p3_load(P, bases + (size_t)w * 40);
    comb_entry(e, P, j, 16);
  }
  niels_store(comb + (size_t)g * kCombEntryInt4, e);
}

void host_bcomb16_bases(int32_t out[16 * 40]) {
  ge_p3 P;
  ge_base_point(P);
  for (int w = 0; w < 16; w++) {
    p3_store(out + w * 40, P);
    ge_mul256(P);
    ge_mul256(P);
  }
}

hipError_t launch_build_bcomb16(const int32_t *d_bases, int4 *comb, hipStream_t stream) {
  hipLaunchKernelGGL(bcomb16_fill_kernel, dim3((16u * kB16Entries + 255) / 256), dim3(256), 0, stream, d_bases, comb);
  return hipGetLastError();
}

// Entry (t, j) of the radix-2^26 B tables: j * 2^(128 t) B for j = 0..2^25 (t = 0, 1), from
// windows 8t and 8t + 1 of the radix-2^16 comb (j = d0 + 2^16 d1, d0 signed: two mixed
// additions), then affine niels with one inversion (per entry: ~15k mads, 2^26 entries, once
// per device).
__global__ __launch_bounds__(256) void b26_fill_kernel(const int4 *__restrict__ comb16, int4 *__restrict__ tab) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= 2u * kB26Entries) return;
  const uint32_t t = g / kB26Entries, j = g % kB26Entries;
  ge_niels e;
  if (j == 0) {
    ge_niels_0(e);
  } else {
    int d0 = (int)(j & 0xffffu);
    uint32_t d1 = j >> 16;
    if (d0 >= 32768) { d0 -= 65536; d1++; }
    const GlobalComb16 bc{comb16};
    ge_p3 P;
    ge_p1p1 q;
    ge_niels n;
    ge_p3_0(P);
    bc.load(8 * (int)t, d0 < 0 ? -d0 : d0, n);
    niels_apply_sign(n, d0 < 0);
    ge_madd_niels(q, P, n, false);
    ge_p1p1_to_p3(P, q);
    bc.load(8 * (int)t + 1, (int)d1, n);
    ge_madd_niels(q, P, n, false);
    ge_p1p1_to_p3(P, q);
    ge_p3_to_niels(e, P);
  }
  niels_store(tab + (size_t)g * kCombEntryInt4, e);
}

hipError_t launch_build_b26(const int4 *comb16, int4 *tab, hipStream_t stream) {
  hipLaunchKernelGGL(b26_fill_kernel, dim3((2u * kB26Entries + 255) / 256), dim3(256), 0, stream, comb16, tab);
  return hipGetLastError();
}

// Entry (w, j) of the radix-2^24 comb: j * 2^(24w) B for j = 0..2^23.  24w = 16v + r (r = 0 or 8):
// J = j 2^r < 2^31 as two signed 16-bit digits at windows v, v + 1 of the radix-2^16 comb (two mixed
// additions), then affine niels with one inversion.  Window 10 (bits 240..263) only ever needs
// j <= 4097 (S < L < 2^252 + 2^125, plus the bit below); it sits on the comb's last window (v = 15),
// so an entry with a second digit has nowhere to take it from and is left as the identity: that is
// every j >= 2^15, where d0 >= 32768 carries into d1 (tests/test_gpu_table_rows.py pins both the
// chain up to 32767 and the identity beyond).
__global__ __launch_bounds__(256) void b24_fill_kernel(const int4 *__restrict__ comb16, int4 *__restrict__ tab) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (uint32_t)kB24Windows * kB24Entries) return;
  const uint32_t w = g / kB24Entries, j = g % kB24Entries;
  const uint32_t v = (24u * w) >> 4, r = (24u * w) & 15u;
  const uint32_t J = j << r;
  int d0 = (int)(J & 0xffffu);
  uint32_t d1 = J >> 16;
  if (d0 >= 32768) { d0 -= 65536; d1++; }
  ge_niels e;
  if (j == 0 || (v + 1 >= 16 && d1 != 0)) {
    ge_niels_0(e);
  } else {
    const GlobalComb16 bc{comb16};
    ge_p3 P;
    ge_p1p1 q;
    ge_niels n;
    ge_p3_0(P);
    bc.load((int)v, d0 < 0 ? -d0 : d0, n);
    niels_apply_sign(n, d0 < 0);
    ge_madd_niels(q, P, n, false);
    ge_p1p1_to_p3(P, q);
    if (d1) {
      bc.load((int)v + 1, (int)d1, n);
      ge_madd_niels(q, P, n, false);
      ge_p1p1_to_p3(P, q);
    }
    ge_p3_to_niels(e, P);
  }
  niels_store(tab + (size_t)g * kCombEntryInt4, e);
}

hipError_t launch_build_b24(const int4 *comb16, int4 *tab, hipStream_t stream) {
  const uint32_t n = (uint32_t)kB24Windows * kB24Entries;
  hipLaunchKernelGGL(b24_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, comb16, tab);
  return hipGetLastError();
}

hipError_t launch_comb_bases(const uint8_t *pubs, uint32_t n, int negate, uint8_t *ok, int32_t *bases,
                             hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(comb_bases_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, pubs, n, negate, ok, bases);
  return hipGetLastError();
}

hipError_t launch_comb_fill(const int32_t *bases, uint32_t n, int4 *comb, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(comb_fill_kernel, dim3((n * kCombWindows + 64 / kCombRuns - 1) / (64 / kCombRuns)), dim3(64), 0,
                     stream, bases, n, comb);
  return hipGetLastError();
}

// ---- radix-2^B comb of -A (kernels.h kCombA*) -------------------------------------------
__global__ __launch_bounds__(64) void comba_bases_kernel(const uint8_t *__restrict__ pubs, uint32_t n,
                                                        int32_t *__restrict__ bases) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t pw[8];
  load_row_words(pw, pubs + 32 * (size_t)i, 2);
  ge_p3 P;
  (void)ge_frombytes_go(P, pw);  // the identity when the key does not decode (key_ok rejects it)
  fe_neg(P.X, P.X);
  fe_neg(P.T, P.T);
#pragma unroll 1
  for (int w = 0; w < kCombAWindows; w++) {
    p3_store(bases + ((size_t)i * kCombAWindows + w) * 40, P);
    ge_mul256(P);  // x 2^B: B - 8 more doublings
    ge_p1p1 t;
    ge_p2 q;
    ge_p3_to_p2(q, P);
#pragma unroll 1
    for (int d = 0; d < kCombABits - 8; d++) {
      ge_p2_dbl(t, q);
      if (d + 1 < kCombABits - 8) ge_p1p1_to_p2(q, t);
    }
    ge_p1p1_to_p3(P, t);
  }
}

// The radix-2^B comb of -A: runs of 8 (comb_fill_run), 64 runs per block, each block within one
// (key, window).
constexpr uint32_t kCombARunsReg = (kCombAEntries - 1) / kCombARun;     // 256: j = 1..2048
constexpr uint32_t kCombARunsTop = (kCombATopEntries - 1) / kCombARun;  // 528: j = 1..4224
static_assert((kCombAEntries - 1) % kCombARun == 0 && (kCombATopEntries - 1) % kCombARun == 0, "runs");
constexpr uint32_t kCombABlocksReg = (kCombARunsReg + 63) / 64, kCombABlocksTop = (kCombARunsTop + 63) / 64;
constexpr uint32_t kCombABlocksPerKey = (kCombAWindows - 1) * kCombABlocksReg + kCombABlocksTop;
__global__ __launch_bounds__(64) void comba_fill_kernel(const int32_t *__restrict__ bases, int4 *__restrict__ comb) {
  __shared__ fe pre[kCombARun][64];
  const uint32_t key = blockIdx.x / kCombABlocksPerKey, g = blockIdx.x % kCombABlocksPerKey;
  const bool top = g >= (kCombAWindows - 1) * kCombABlocksReg;
  const uint32_t w = top ? kCombAWindows - 1 : g / kCombABlocksReg;
  const uint32_t run = (g - w * kCombABlocksReg) * 64u + threadIdx.x;
  int4 *rows = comb + ((size_t)key * kCombARowsPerKey + comba_row((int)w, 0)) * kCombEntryInt4;
  if (run == 0) {
    ge_niels id;
    ge_niels_0(id);
    niels_store(rows, id);
  }
  if (run >= (top ? kCombARunsTop : kCombARunsReg)) return;
  comb_fill_run(rows, bases + ((size_t)key * kCombAWindows + w) * 40, 1u + kCombARun * run,
                top ? comb_start_bits(kCombARunsTop) : comb_start_bits(kCombARunsReg), pre, threadIdx.x);
}

hipError_t launch_build_comba(const uint8_t *pubs, uint32_t n, int32_t *bases, int4 *comba, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(comba_bases_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, pubs, n, bases);
  hipLaunchKernelGGL(comba_fill_kernel, dim3(n * kCombABlocksPerKey), dim3(64), 0, stream, bases, comba);
  return hipGetLastError();
}

// ---- tests: the chain check of a whole table (kernels.h ChainPlan) ------------------------
__device__ __forceinline__ bool niels_is_identity(const ge_niels &e) {
  fe one;
  fe_1(one);
  return fe_equal(e.YpX, one) && fe_equal(e.YmX, one) && fe_iszero(e.XY2d);
}
// the affine niels row e is the projective point P: e (Y+X, Y-X, 2dXY / Z^2) against P's
// (Y + X) / Z, (Y - X) / Z, 2d T / Z, cross-multiplied and compared fully reduced
__device__ __forceinline__ bool niels_equals_p3(const ge_niels &e, const ge_p3 &P) {
  fe l, r, d2;
  fe_mul(l, e.YpX, P.Z);
  fe_add(r, P.Y, P.X);
  bool same = fe_equal(l, r);
  fe_mul(l, e.YmX, P.Z);
  fe_sub(r, P.Y, P.X);
  same = fe_equal(l, r) && same;
  fe_const_d2(d2);
  fe_mul(l, e.XY2d, P.Z);
  fe_mul(r, d2, P.T);
  same = fe_equal(l, r) && same;
  return same && !fe_iszero(P.Z);
}

// One lane per row (unit u, window w, entry j).  Reads the table only; writes out[0] (rows
// checked), out[1] (rows that fail) and out[2..17] (the first failing rows, window << 32 | j).
__global__ __launch_bounds__(256) void table_chain_kernel(ChainPlan p, unsigned long long *__restrict__ out) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = g < p.rows_per_unit * p.units;
  bool bad = false;
  uint32_t w = 0, j = 0;
  if (live) {
    const uint64_t u = g / p.rows_per_unit;
    const uint32_t rr = (uint32_t)(g % p.rows_per_unit);
    w = rr / p.entries;
    if (w >= p.windows) w = p.windows - 1;
    j = rr - w * p.entries;
    const int4 *unit = p.chunks ? p.chunks[u >> kKeyChunkBits] + (u & (kKeyChunkKeys - 1)) * p.rows_per_unit * kCombEntryInt4
                                : p.base;
    const int4 *win = unit + (size_t)w * p.entries * kCombEntryInt4;
    const bool top = w + 1 == p.windows;
    ge_niels e;
    niels_load(e, win + (size_t)j * kCombEntryInt4);
    if (j == 0 || (p.ok && !p.ok[u]) || (top && j > p.top_chain_last)) {
      bad = !niels_is_identity(e);
    } else if (j == 1) {
      if (!top) {  // the next window's base: step_bits doublings of this one
        ge_p3 P;
        ge_p2 q;
        ge_p1p1 t;
        ge_niels_to_p3(P, e);
        ge_p3_to_p2(q, P);
#pragma unroll 1
        for (uint32_t d = 0; d + 1 < p.step_bits; d++) { ge_p2_dbl(t, q); ge_p1p1_to_p2(q, t); }
        ge_p2_dbl(t, q);
        ge_p1p1_to_p3(P, t);
        niels_load(e, win + (size_t)(p.entries + 1) * kCombEntryInt4);
        bad = !niels_equals_p3(e, P);
      }
    } else {  // row j = row (j - 1) + row 1
      ge_niels prev, one;
      ge_p3 P;
      ge_p1p1 t;
      niels_load(prev, win + (size_t)(j - 1) * kCombEntryInt4);
      niels_load(one, win + kCombEntryInt4);
      ge_niels_to_p3(P, prev);
      ge_madd_niels(t, P, one, false);
      ge_p1p1_to_p3(P, t);
      bad = !niels_equals_p3(e, P);
    }
  }
  const unsigned long long lanes = __ballot(live);
  if (live && (threadIdx.x & 63u) == (uint32_t)(__ffsll(lanes) - 1))
    atomicAdd(out, (unsigned long long)__popcll(lanes));
  if (bad) {
    const unsigned long long slot = atomicAdd(out + 1, 1ull);
    if (slot < 16) out[2 + slot] = (unsigned long long)w << 32 | j;
  }
}

__global__ void table_corrupt_kernel(int4 *row) { row->x += 1; }

hipError_t launch_table_chain(const ChainPlan &p, uint64_t *d_out, hipStream_t stream) {
  const uint64_t blocks = (p.rows_per_unit * p.units + 255) / 256;
  if (blocks == 0 || blocks > 0x7fffffffu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(table_chain_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, p,
                     reinterpret_cast<unsigned long long *>(d_out));
  return hipGetLastError();
}
hipError_t launch_table_corrupt(int4 *row, hipStream_t stream) {
  hipLaunchKernelGGL(table_corrupt_kernel, dim3(1), dim3(1), 0, stream, row);
  return hipGetLastError();
}

}  // namespace tmed
