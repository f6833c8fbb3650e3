// kernels.hip — gfx950 kernels: batch ed25519 verify (the generic throughput path, then the
// key-cached path) and RFC 8032 sign.  The kernels that build the tables these read, once per
// context or per key set, are in kernels_tables.hip.
// Every kernel that hashes stays in this one unit: sha512_stream is compiled once per unit, and
// how the compiler shapes its block loop depends on the set of prefix lengths the unit's callers
// pass (the verify kernels 64, the signer 32).  Apart, the verify kernels' code changes.
//
// One signature per lane (64 per wave) on the throughput paths.  The work per signature
// is ~2.2e5 32x32->64 integer multiply-adds, entirely VALU; the
// algorithmic HBM traffic is ~214 B per verify, so the kernels are bound by integer-VALU
// issue, not by memory and not by MFMA (which has no 32x32->64 integer path).
//
// Memory layout
//   pub   n x 32 B, sig n x 64 B (16-B aligned rows -> dwordx4 loads)
//   msgs  concatenated bytes, off[n+1] u32 (or fixed 256-B vote slots)
//   slab  per-lane variable-base tables: 12 (joint table of -A and R) or 8 cached points x 128 B (fe_pack256),
//         lane-major [slot][entry][chunk]; the default main kernel keeps entries 1 and 5 in LDS instead
//   b16   32769 niels multiples of B in 128-B rows in HBM (4.2 MB; the full-length fallback, variant 5)
//   combs key-set combs [key][window][entry] and the shared combs of B (radix 256, radix 2^16)
#include "kernels.h"
#include "verify_core.h"
#include "verify_hs.h"
#include "kernel_util.h"
#include "rows.h"
#include "slot_rows.h"
#include "votes_dev.h"

namespace tmed {

// Per-lane table in the HBM slab, lane-major [slot][entry 1..ROWS][chunk]: each lane's entry is one
// aligned 128-B line (the four coordinates in fe_pack256 form), so a divergent lookup reads
// exactly one line.  The slab does not fit L2/MALL at full occupancy; the 160-B int32 form
// read 2.25 lines per lookup, and its traffic cost ~10 % of the clock (profiles/r02/s4).
// Entry 0 (the identity, cached form (1, 1, 1, 0)) is not stored per lane: every lane reads this
// one row (an L2 hit), so the slab holds entries 1..ROWS.
// (a plain __device__ variable: global address space like the slab, so the row select below stays a
// global pointer and the table loads are global_load — a select against a constant-address-space
// row made them flat_load, which also count in lgkmcnt: every s_waitcnt lgkmcnt(0) of the B-row
// prefetch then waited for the table rows in flight as well)
__device__ int4 kIdentityRow[8] = {{1, 0, 0, 0}, {0, 0, 0, 0}, {1, 0, 0, 0}, {0, 0, 0, 0},
                                          {1, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};

// Per-lane table rows go through the default cache policy: a non-temporal policy for the slab
// stores, the slab loads or the B rows was measured at -12 / -6 / -0.5 % on C2 (all three -26 %,
// profiles/r05/s2/): a lane re-reads its rows ~4 times and nt sends every re-read to HBM.
__device__ __forceinline__ void slab_st(int4 *p, int4 v) { *p = v; }
__device__ __forceinline__ int4 slab_ld(const int4 *p) { return *p; }

// ROWS: 8 (j * (-A), the full-length fallback) or kJointRows (the joint table of the half-size path).
template <int ROWS>
struct SlabTabN {
  int4 *base;
  uint32_t slot;

  __device__ __forceinline__ const int4 *row(int j) const {
    return j == 0 ? kIdentityRow : base + ((size_t)slot * ROWS + (j - 1)) * 8;
  }

  __device__ __forceinline__ void store(int j, const ge_cached &c) const {
    if (j == 0) return;
    int4 *r = base + ((size_t)slot * ROWS + (j - 1)) * 8;
    const fe *fs[4] = {&c.YpX, &c.YmX, &c.Z, &c.T2d};
#pragma unroll
    for (int f = 0; f < 4; f++) {
      uint32_t w[8];
      fe_pack256(w, *fs[f]);
      slab_st(r + 2 * f, make_int4((int)w[0], (int)w[1], (int)w[2], (int)w[3]));
      slab_st(r + 2 * f + 1, make_int4((int)w[4], (int)w[5], (int)w[6], (int)w[7]));
    }
  }
  // prefetch issues the row's eight 16-B loads into registers (swap: Y+X and Y-X exchanged by
  // the load addresses — a negative digit's entry, ge_add_cached_pre); take unpacks them.
  // hs_straus_joint (verify_hs.h) prefetches every row two doublings before its take.
  int4 pv[8];
  __device__ __forceinline__ void prefetch(int j, bool swap = false) {
    const int4 *r = row(j);
    const int sx = swap ? 2 : 0;
#pragma unroll
    for (int q = 0; q < 8; q++) pv[q] = slab_ld(r + (q < 4 ? (q ^ sx) : q));
  }
  __device__ __forceinline__ void take(ge_cached &c) const {
    fe *fs[4] = {&c.YpX, &c.YmX, &c.Z, &c.T2d};
#pragma unroll
    for (int f = 0; f < 4; f++) {
      const uint32_t w[8] = {(uint32_t)pv[2 * f].x, (uint32_t)pv[2 * f].y, (uint32_t)pv[2 * f].z,
                             (uint32_t)pv[2 * f].w, (uint32_t)pv[2 * f + 1].x, (uint32_t)pv[2 * f + 1].y,
                             (uint32_t)pv[2 * f + 1].z, (uint32_t)pv[2 * f + 1].w};
      fe_unpack256(*fs[f], w);
    }
  }
};
using SlabTab = SlabTabN<8>;
using SlabTabJ = SlabTabN<kJointRows>;
static_assert(kSlabSlotBytes == 8 * 128 && kSlabJointSlotBytes == kJointRows * 128, "slab rows are 128 B");

// The joint table of verify_main_hs_kernel<26>: SlabTabJ with rows 1 (Q) and 5 (P) in LDS.  One
// sub-step lookup in four reads P or Q alone (a radix-4 digit pair (+-1, 0) or (0, +-1)), the two
// rows that are affine and that build_table_joint reads back, so they stay on the CU: lds is the
// block's [2][kLdsRowInt4][kHsBlock] array (row, piece, lane — lane l's piece q of P at
// lds[(kLdsRowInt4 + q) * kHsBlock + l], as the B rows are staged), Y+X, Y-X and 2dT in
// fe_pack256 form; Z = 1 is not stored.  Their slab lines are never written or read (the slot
// stride stays kSlabJointSlotBytes).  prefetch issues the slab loads (the lanes whose row is in LDS
// read the shared identity row with them); take reads LDS into the same registers for those lanes.
// The slab loads stay global_load and the LDS reads ds_read (see kIdentityRow: no select between
// the two pointers).
constexpr int kLdsRowInt4 = 6;
constexpr uint32_t kLdsRowsInt4 = 2 * kLdsRowInt4 * kThreadsPerBlock;  // int4 per block: 48 KB
// (the two kinds of load through pointers of their own address spaces: through generic pointers the
// compiler merged a prefetch and the take after it into one flat load from a selected pointer)
typedef int v4i __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) v4i glb_v4i;
typedef __attribute__((address_space(3))) v4i lds_v4i;
struct SlabLdsTabJ {
  int4 *blk;     // the slab slot of the block's lane 0 (uniform) and the lane's index in the block:
  uint32_t tid;  // a row's address is made from the two where it is loaded, no 64-bit one is kept per lane
  int4 *lds;     // the block's array + the lane's index in the block
  __device__ __forceinline__ int4 *slab_row(int j) const { return blk + (tid * kJointRows + (uint32_t)(j - 1)) * 8u; }

  __device__ __forceinline__ static bool in_lds(int j) { return j == 1 || j == 5; }

  __device__ __forceinline__ void store(int j, const ge_cached &c) const {
    if (j == 0) return;
    if (in_lds(j)) {
      lds_v4i *r = (lds_v4i *)lds + (j == 5 ? kLdsRowInt4 : 0) * kThreadsPerBlock;
      const fe *fs[3] = {&c.YpX, &c.YmX, &c.T2d};
#pragma unroll
      for (int f = 0; f < 3; f++) {
        uint32_t w[8];
        fe_pack256(w, *fs[f]);
        r[(2 * f) * kThreadsPerBlock] = v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
        r[(2 * f + 1) * kThreadsPerBlock] = v4i{(int)w[4], (int)w[5], (int)w[6], (int)w[7]};
      }
      return;
    }
    glb_v4i *r = (glb_v4i *)slab_row(j);
    const fe *fs[4] = {&c.YpX, &c.YmX, &c.Z, &c.T2d};
#pragma unroll
    for (int f = 0; f < 4; f++) {
      uint32_t w[8];
      fe_pack256(w, *fs[f]);
      r[2 * f] = v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
      r[2 * f + 1] = v4i{(int)w[4], (int)w[5], (int)w[6], (int)w[7]};
    }
  }
  v4i pv[8];
  bool inl, isp, swp;  // the prefetched row is in LDS; it is P; Y+X and Y-X exchanged (lane masks in
                       // scalar registers: the kernel has no vector register to spare)
  // The lanes whose row is in LDS load the shared identity row, an L2 hit as for digit 0: with the
  // slab loads under a branch of their own the compiler's wait counts at the join were vmcnt(0),
  // the whole prefetch distance.
  __device__ __forceinline__ void prefetch(int j, bool swap = false) {
    inl = in_lds(j);
    isp = j == 5;
    swp = swap;
    const glb_v4i *r = (const glb_v4i *)(j == 0 || inl ? kIdentityRow : slab_row(j));
    const int sx = swap ? 2 : 0;
#pragma unroll
    for (int q = 0; q < 8; q++) pv[q] = r[q < 4 ? (q ^ sx) : q];
  }
  __device__ __forceinline__ void take(ge_cached &c) {
    if (inl) {
      const lds_v4i *r = (const lds_v4i *)lds + (isp ? kLdsRowInt4 : 0) * (int)kThreadsPerBlock;
      const int sx = swp ? 2 * (int)kThreadsPerBlock : 0;  // swap, through the read addresses
      const lds_v4i *a = r + sx, *b = r + (2 * (int)kThreadsPerBlock - sx);
      pv[0] = a[0];
      pv[1] = a[kThreadsPerBlock];
      pv[2] = b[0];
      pv[3] = b[kThreadsPerBlock];
      pv[4] = v4i{1, 0, 0, 0};  // Z = 1: fe_unpack256 gives exactly fe_1
      pv[5] = v4i{0, 0, 0, 0};
      pv[6] = r[4 * kThreadsPerBlock];
      pv[7] = r[5 * kThreadsPerBlock];
    }
    fe *fs[4] = {&c.YpX, &c.YmX, &c.Z, &c.T2d};
#pragma unroll
    for (int f = 0; f < 4; f++) {
      const uint32_t w[8] = {(uint32_t)pv[2 * f].x, (uint32_t)pv[2 * f].y, (uint32_t)pv[2 * f].z,
                             (uint32_t)pv[2 * f].w, (uint32_t)pv[2 * f + 1].x, (uint32_t)pv[2 * f + 1].y,
                             (uint32_t)pv[2 * f + 1].z, (uint32_t)pv[2 * f + 1].w};
      fe_unpack256(*fs[f], w);
    }
  }
};

typedef __attribute__((address_space(1))) void global_void;
typedef __attribute__((address_space(3))) void lds_void;

// Radix-2^16 / 2^26 B table (double_scalarmult<16>, hs_straus): j*B, j = 0..32768 / 2^25, affine niels in 128-B rows
// (kCombEntryInt4 int4, 4.2 MB, L2/MALL-resident).  The entry of the next B window is fetched
// into LDS with global_load_lds_dwordx4 right after the current B addition, 16 doublings
// before it is needed; buf is this wave's [8][64] int4 region (lane l's piece q at q*64+l).
template <int BITS>
struct BPf {
  static constexpr int kBits = BITS;
  const int4 *tab;
  int4 *buf;
  uint32_t lane;
  __device__ __forceinline__ void prefetch(int j) const {
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the previous take's LDS reads are done
#pragma unroll
    for (int q = 0; q < 8; q++)
      __builtin_amdgcn_global_load_lds((global_void *)(tab + (size_t)j * 8 + q), (lds_void *)(buf + q * 64), 16, 0, 0);
  }
  __device__ __forceinline__ void take(ge_niels &e) const { niels_load(e, buf + lane, 64); }
};

// Phase 1: SHA-512(R||A||M) mod L, S < L, A = Point.SetBytes(pub)  (one lane per signature
// of the chunk [base, base + count)).
// Threads per block of the generic throughput kernels (prep, prep_r, the half-size main): 256.
// (Blocks of 64 / 128 threads, whose wave slots come back sooner at a launch's end, were level /
// 4 % slower per C2 step: profiles/r05/s32/.)
constexpr uint32_t kHsBlock = kThreadsPerBlock;

constexpr int kPrepWaves = 3;  // 152 VGPRs, no spills (4 waves with a leaner decode: no faster, profiles/r03/prep_joint)
__global__ __launch_bounds__(kHsBlock, kPrepWaves) void verify_prep_kernel(
    const uint8_t *__restrict__ pub, const uint8_t *__restrict__ sig, MsgSrc ms, uint32_t base, uint32_t count,
    int4 *__restrict__ prep, uint32_t stride, uint32_t *__restrict__ place) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (place && slot == 0) place[0] = place[1] = 0;  // the half-size placement counters (verify_prep_r_kernel)
  if (slot >= count) return;
  const uint32_t i = base + slot;
  // verify_prep's steps with the hash first and k, s handed over at once, so the decode of A
  // runs with only the key's words live (s keeps S when only A fails to decode: the verdict
  // is false either way and S < L after the S checks).
  uint32_t pw[8];
  bool sok;
  {
    uint32_t sw[16], k[8], h[16];
    load_row_words(pw, pub + 32 * (size_t)i, 2);
    load_row_words(sw, sig + 64 * (size_t)i, 4);
    const uint8_t *m;
    uint32_t mlen;
    ms.get(i, m, mlen);
    sok = (sw[15] & 0xE0000000u) == 0 && sc_is_canonical(sw + 8);
    sha512_stream(h, sw, pw, 64, m, mlen);
    sc_reduce512(k, h);
#pragma unroll
    for (int q = 0; q < 2; q++)
      prep[(size_t)q * stride + slot] = make_int4((int)k[4 * q], (int)k[4 * q + 1], (int)k[4 * q + 2], (int)k[4 * q + 3]);
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const uint32_t *S = sw + 8 + 4 * q;
      prep[(size_t)(2 + q) * stride + slot] = sok ? make_int4((int)S[0], (int)S[1], (int)S[2], (int)S[3])
                                                  : make_int4(0, 0, 0, 0);
    }
  }
  ge_p3 A;
  const bool ok = ge_frombytes_go(A, pw) && sok;  // Point.SetBytes (identity on failure)
  int32_t w[24];
#pragma unroll
  for (int j = 0; j < 10; j++) { w[j] = A.X.v[j]; w[10 + j] = A.Y.v[j]; }
  w[20] = ok ? 1 : 0;
  w[21] = w[22] = w[23] = 0;
#pragma unroll
  for (int q = 0; q < 6; q++)  // words 16..39: A.x, A.y, ok
    prep[(size_t)(4 + q) * stride + slot] = make_int4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
}

// ---- f1: CanonicalVote sign-bytes assembled on the device ----------
// (votes_dev.h assemble_vote_into: vote_wire.h's vote_splice on the staged template; this kernel
// serves the throughput and key-cached paths, the latency kernels assemble in their hash lanes.)  One wave per block: every lane assembles its
// vote in LDS (byte stores to LDS, beside its staged template), then the wave writes its 64
// consecutive 256-B slots as sixteen coalesced 1-KB rows (slot_rows.h wave_store_slots, which
// records what stores straight into the global slots cost).
constexpr uint32_t kAsmLanes = kSlotLanes;
__global__ __launch_bounds__(kAsmLanes) void assemble_votes_kernel(VoteAsm va, uint32_t n, uint8_t *__restrict__ out,
                                                                  uint32_t *__restrict__ out_len) {
  __shared__ int4 tl[kAsmLanes][kVoteTmplBytes / 16];
  __shared__ int4 ob[kAsmLanes][kVoteSlot / 16];
  const uint32_t lane = threadIdx.x, i0 = blockIdx.x * kAsmLanes, i = i0 + lane;
  if (i < n) {
    lds_zero<kSlotInt4>(ob[lane]);
    out_len[i] = assemble_vote_into(va, i, reinterpret_cast<uint8_t *>(ob[lane]), tl[lane]);
  }
  __syncthreads();
  wave_store_slots<1>(&ob[0][0], out, i0, n);
}

// Phase 2 of the full-length fallback (TMED_MAIN_WAVES=5): table of -A, Straus [k](-A) + [s]B
// (radix-2^16 B windows from the HBM table, each entry fetched into LDS 16 doublings ahead)
// -> projective R' (hand-off to the batched finish).
__global__ __launch_bounds__(kThreadsPerBlock, 2) void verify_main_kernel(
    uint32_t base, uint32_t count, const int4 *__restrict__ prep, uint32_t stride, int4 *__restrict__ slab,
    const int4 *__restrict__ b16, int4 *__restrict__ fin, uint32_t fin_base, uint8_t *__restrict__ out) {
  __shared__ int4 sb16[kThreadsPerBlock / 64][8 * 64];
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= count) return;
  const uint32_t i = base + slot;
  uint32_t k[8], s[8];
  ge_p3 A;
  const bool ok = prep_load(prep, stride, slot, k, s, A);
  ge_p2 R;
  BPf<16> bt{b16, sb16[threadIdx.x >> 6], threadIdx.x & 63u};
  SlabTab tab{slab, slot};
  verify_main_point(R, k, s, A, tab, bt);
  fin_store(fin, kFinCap, i - fin_base, R.X, R.Y, R.Z);
  out[i] = ok ? 1 : 0;
}

// ---- half-size path (verify_hs.h; main variant 6, the default) -----------------------
// verify_prep_kernel writes k, s, A, ok to the first prep region (10 int4 per slot); the
// R kernel writes the second region (kPrepHsInt4 int4 per position, [q][position]): recoded c
// (words 0-7), recoded |d| (8-12), recoded e (13-20), R.x (21-30), R.y (31-40), flags (41:
// bit 0 ok, bit 1 d < 0, bits 8.. window count W), the signature's slot (42), A.x (44-53),
// A.y (54-63) — everything the main kernel reads.
//
// Placement by window count: the main kernel runs every lane of a wave over the wave's largest
// W, and W is 32 or 33 for almost every signature (a few lanes 34+).  The R kernel therefore
// writes signatures with W > 32 from the front of the region and the others (W <= 32) from the back
// (one atomic per wave and group on place[0] / place[1], the lanes of a group at consecutive
// positions, so the stores stay coalesced): the waves of the W <= 32 part run 32 windows instead
// of the unsorted wave maximum (~33.3 on average, tmed_window_stats), ~2 % of the main kernel.
// The longer waves go first, so the launch's last round holds short ones (-0.3 % per C2 step
// against short first, 9 of 11 alternating rounds, profiles/r05/s33/).
constexpr int kPrepHsInt4 = 16;
constexpr int kHsWSmall = 32;
static_assert((kPrepInt4 + kPrepHsInt4) * 16 <= kPrepSlotBytes, "prep slot too small for the half-size hand-off");

constexpr int kPrepRWaves = 3;  // 168 VGPRs, 6 spilled: -0.06 ms per 2^20 against 2 waves (the Euclid loop hides its memory waits)
__global__ __launch_bounds__(kHsBlock, kPrepRWaves) void verify_prep_r_kernel(
    const uint8_t *__restrict__ sig, uint32_t base, uint32_t count, const int4 *__restrict__ prep,
    int4 *__restrict__ prep2, uint32_t stride, uint32_t *__restrict__ place, int zip215) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= count) return;
  // R's decode first (the sqrt-ratio chain), then k and s from the hand-off for the lattice step:
  // nothing of the hand-off is live across the chain, so the kernel fits 3 waves/SIMD unspilled
  uint32_t Rw[8];
  load_row_words(Rw, sig + 64 * (size_t)(base + slot), 2);
  fe Rx, Ry;
  bool rok;
  if (zip215) {
    ge_p3 P;
    rok = ge_frombytes_go(P, Rw);
    fe_copy(Rx, P.X);
    fe_copy(Ry, P.Y);
  } else {
    rok = r_decode_strict(Rx, Ry, Rw);
  }
  if (!rok) { fe_0(Rx); fe_1(Ry); }
  int32_t w[64];
#pragma unroll
  for (int q = 0; q < 4; q++) {  // k (words 0-7), s (8-15)
    const int4 v = prep[(size_t)q * stride + slot];
    w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
  }
  uint32_t k[8], s[8], cr[8], dr[8], er[8];
#pragma unroll
  for (int j = 0; j < 8; j++) { k[j] = (uint32_t)w[j]; s[j] = (uint32_t)w[8 + j]; }
  bool dneg;
  int W, Wl;  // W: the tight window count (top digits 0..16, hs_straus), Wl the latency kernels' count
  hs_scalars(k, s, cr, dr, er, dneg, Wl, /*raw_e=*/true, &W);  // (hs_prep_r's two phases, in this order)
  const bool ok = prep[(size_t)9 * stride + slot].x != 0;  // word 36
#pragma unroll
  for (int j = 0; j < 8; j++) { w[j] = (int32_t)cr[j]; w[13 + j] = (int32_t)er[j]; }
#pragma unroll
  for (int j = 0; j < 5; j++) w[8 + j] = (int32_t)dr[j];
#pragma unroll
  for (int j = 0; j < 10; j++) { w[21 + j] = Rx.v[j]; w[31 + j] = Ry.v[j]; }
  w[41] = ((ok && rok) ? 1 : 0) | (dneg ? 2 : 0) | (W << 8);
  w[42] = (int32_t)slot;
  w[43] = 0;
#pragma unroll
  for (int q = 4; q < 9; q++) {  // A.x, A.y: words 16..35 of the first region
    const int4 v = prep[(size_t)q * stride + slot];
    w[28 + 4 * q] = v.x; w[29 + 4 * q] = v.y; w[30 + 4 * q] = v.z; w[31 + 4 * q] = v.w;
  }
  // position: W > kHsWSmall from the front, the rest from the back (count - 1 downwards), so the
  // main kernel's longest waves are dispatched first
  const bool front = W > kHsWSmall;
  const uint64_t act = __ballot(1), sm = __ballot(front);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  uint32_t fs = 0, fl = 0;
  if (lane == (uint32_t)__builtin_ctzll(act)) {  // the wave's first active lane takes both ranges
    const uint32_t ns = (uint32_t)__builtin_popcountll(sm), nl = (uint32_t)__builtin_popcountll(act & ~sm);
    if (ns) fs = atomicAdd(&place[0], ns);
    if (nl) fl = atomicAdd(&place[1], nl);
  }
  const int leader = __builtin_ctzll(act);
  fs = (uint32_t)__shfl((int)fs, leader);
  fl = (uint32_t)__shfl((int)fl, leader);
  const uint32_t pos = front ? fs + (uint32_t)__builtin_popcountll(sm & below)
                             : count - 1u - (fl + (uint32_t)__builtin_popcountll(act & ~sm & below));
#pragma unroll
  for (int q = 0; q < kPrepHsInt4; q++)
    prep2[(size_t)q * stride + pos] = make_int4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
}

// The lane's index in its wave, computed afresh where it is used (two v_mbcnt on an operand the
// compiler cannot see through, so the value is neither hoisted out of a loop nor kept): the main
// kernel has no register for a lane index that a read per eight windows needs.
__device__ __forceinline__ uint32_t lane_fresh() {
  uint32_t z = 0;
  asm volatile("" : "+v"(z));
  return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z));
}

// Digits of the recoded c / |d| straight from the hand-off (one dword per eight windows).
// Lanes past count read all-zero digits (0x88888888): their hand-off positions hold a previous
// batch's recodings, whose top digit (hs_top_digit) could leave [-8, 8] at this wave's W and
// index past the lane's table rows.
struct HsDigitsDev {
  const int4 *p2;
  uint32_t stride, slot0;  // slot0: the position of the wave's lane 0 (wave-uniform)
  bool active;
  __device__ __forceinline__ uint32_t word(int w) const {
    // a 32-bit word index, its uniform part apart, beside the uniform base: no address of the lane's
    // own live through the loop.  (The digits are words 0..12, below 4 * stride int4, and a
    // context's hand-off and slab, ~2.5 KB per slot, bound stride far below 2^28.)
    const uint32_t u = ((uint32_t)(w >> 2) * stride + slot0) * 4u + (uint32_t)(w & 3);
    return active ? reinterpret_cast<const uint32_t *>(p2)[u + lane_fresh() * 4u] : 0x88888888u;
  }
  __device__ __forceinline__ uint32_t cword(int w) const { return word(w); }
  __device__ __forceinline__ uint32_t dword(int w) const { return w < 5 ? word(8 + w) : 0x88888888u; }
};

// Phase 2: the joint radix-4 table of -A and -sign(d) R (twelve rows per lane: ten in the slab and
// the two points themselves in LDS, SlabLdsTabJ; radix 16: all twelve in the slab), the 3-point
// Straus sum over the wave's largest window count, B digits from the two radix-2^26 tables (radix
// 16: windows 0 and 8 of the radix-2^16 comb), each row fetched into LDS ahead of its addition,
// identity test.  Every
// lane of the grid stays to the end (the wave maximum of W is a shuffle reduction); lanes
// past count run on the identity and store nothing.
constexpr int kHsWaves = 2;  // waves per SIMD of the half-size main kernel (all 256 VGPRs at 2, no scratch)
// BB: radix of the B windows — 26 (the default: btab, two 2^25-entry tables, ten B additions) or
// 16 (windows 0 and 8 of the 2^16 comb, sixteen; when the 8.6-GB tables are unavailable).  The
// hand-off carries e unrecoded (hs_prep_r raw_e); radix 16 recodes it here.
// LDS per block.  Radix 26: one B-row buffer per wave — BH's row is fetched into it right after
// BL's take (hs_b26_add), a cached addition (~3k issue cycles) before its own — and the P and Q
// table rows (SlabLdsTabJ): 32 + 48 = 80 KB, two blocks fill a CU's 160 KB.  Radix 16 (sixteen B
// steps, each row fetched a whole step ahead): a buffer each for BL and BH, the table in the slab.
static_assert(kHsBlock == kThreadsPerBlock, "SlabLdsTabJ's lane stride");
template <int BB>
struct HsLds;
template <>
struct HsLds<26> {
  int4 bl[kHsBlock / 64][8 * 64];
  int4 pq[kLdsRowsInt4];
  __device__ __forceinline__ int4 *bh(uint32_t wv) { return bl[wv]; }
};
template <>
struct HsLds<16> {
  int4 bl[kHsBlock / 64][8 * 64];
  int4 bhs[kHsBlock / 64][8 * 64];
  __device__ __forceinline__ int4 *bh(uint32_t wv) { return bhs[wv]; }
};
template <int BB>
__global__ __launch_bounds__(kHsBlock, kHsWaves) void verify_main_hs_kernel(
    uint32_t base, uint32_t count, const int4 *__restrict__ prep, const int4 *__restrict__ prep2, uint32_t stride,
    int4 *__restrict__ slab, const int4 *__restrict__ btab, uint8_t *__restrict__ out, int zip215) {
  __shared__ HsLds<BB> sm;
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;  // position in the placed hand-off
  const bool active = slot < count;
  int32_t w[64];
  // e, R, flags, the signature's slot, A (words 12..63); radix 26 reads e (words 13..20) after the
  // table build, the kernel's register peak
#pragma unroll
  for (int q = BB == 26 ? 5 : 3; q < kPrepHsInt4; q++) {
    const int4 v = active ? prep2[(size_t)q * stride + slot] : make_int4(0, 0, 0, 0);
    w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
  }
  uint32_t er[8];
  if constexpr (BB == 16) {
    uint32_t e[8];
#pragma unroll
    for (int j = 0; j < 8; j++) e[j] = (uint32_t)w[13 + j];
    sc_recode_b<16>(er, e);
  }
  fe Rx, Ry;
#pragma unroll
  for (int j = 0; j < 10; j++) { Rx.v[j] = w[21 + j]; Ry.v[j] = w[31 + j]; }
  ge_p3 A;
#pragma unroll
  for (int j = 0; j < 10; j++) { A.X.v[j] = w[44 + j]; A.Y.v[j] = w[54 + j]; }
  if (!active) { fe_1(A.Y); fe_1(Ry); }
  fe_1(A.Z);
  fe_mul(A.T, A.X, A.Y);
  const int flags = w[41];
  int W = active ? (flags >> 8) : 29;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int x = __shfl_xor(W, o);
    W = x > W ? x : W;
  }
  W = __builtin_amdgcn_readfirstlane(W);
  if (W < 29) W = 29;
  if (W > 64) W = 64;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t slot0 = blockIdx.x * blockDim.x + ((uint32_t)__builtin_amdgcn_readfirstlane((int)threadIdx.x) & ~63u);
  const HsDigitsDev ds{prep2, stride, slot0, active};
  // the high table: the second radix-2^26 table, or window 8 (j * 2^128 B) of the 2^16 comb
  const size_t hi = BB == 26 ? (size_t)kB26Entries * kCombEntryInt4 : (size_t)8 * kB16Entries * kCombEntryInt4;
  BPf<BB> bl{btab, sm.bl[wv], lane};
  BPf<BB> bh{btab + hi, sm.bh(wv), lane};
  bool id;
  if constexpr (BB == 26) {
    SlabLdsTabJ tj{slab + (size_t)blockIdx.x * blockDim.x * (kJointRows * 8), threadIdx.x, sm.pq + threadIdx.x};
    ge_p3 P, Q;  // verify_main_hsj's steps
    hs_points(P, Q, (flags & 2) != 0, A, Rx, Ry);
    build_table_joint(tj, P, Q);
#pragma unroll
    for (int q = 3; q < 6; q++) {
      const int4 v = active ? prep2[(size_t)q * stride + slot0 + lane_fresh()] : make_int4(0, 0, 0, 0);
      w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) er[j] = (uint32_t)w[13 + j];
    ge_p2 q;
    hs_straus_joint(q, ds, er, W, tj, bl, bh);
    if (zip215) p2_mul8(q);
    id = p2_is_identity(q);
  } else {
    SlabTabJ tj{slab, slot};
    id = verify_main_hsj(ds, (flags & 2) != 0, er, W, A, Rx, Ry, tj, bl, bh, zip215 != 0);
  }
  if (active) {
    // the verdict bit and the signature's slot once more from the hand-off (word 41, 42), at an
    // index the compiler cannot match with the first read's: kept from there they cost registers
    // (spilled ones, with the P and Q rows in LDS) through the whole sum
    const int4 v = prep2[(size_t)10 * stride + slot0 + lane_fresh()];
    out[base + (uint32_t)v.z] = ((v.y & 1) && id) ? 1 : 0;
  }
}

// Diagnostics (tmed_window_stats): the lattice step's window count W of every lane of the last
// half-size chunk (hand-off flags, bits 8..), as a per-lane histogram and a histogram of the
// wave maxima — the loop length each wave of verify_main_hs_kernel actually ran (W = 64: the
// (k, 1) fallback).  Same 64-slot waves as the main kernel.
__global__ __launch_bounds__(kThreadsPerBlock) void window_stats_kernel(const int4 *__restrict__ prep2, uint32_t stride,
                                                                       uint32_t count, uint32_t *__restrict__ lane_hist,
                                                                       uint32_t *__restrict__ wave_hist) {
  __shared__ uint32_t lh[65], wh[65];  // block-local histograms, one global atomic per bin per block
  for (uint32_t b = threadIdx.x; b < 65; b += blockDim.x) lh[b] = wh[b] = 0;
  __syncthreads();
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = slot < count;
  int W = active ? (prep2[(size_t)10 * stride + slot].y >> 8) : 0;  // word 41
  if (W < 0 || W > 64) W = 64;
  if (active) atomicAdd(&lh[W], 1u);
  int m = W;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int x = __shfl_xor(m, o);
    m = x > m ? x : m;
  }
  if ((threadIdx.x & 63u) == 0 && slot < count) atomicAdd(&wh[m], 1u);
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < 65; b += blockDim.x) {
    if (lh[b]) atomicAdd(&lane_hist[b], lh[b]);
    if (wh[b]) atomicAdd(&wave_hist[b], wh[b]);
  }
}

// Tests (tmed_test_joint_rows): lane i builds the joint table of the points encoded in a[i] and
// r[i] (Point.SetBytes; the identity when one does not decode) with dneg[i] as d's sign, as
// verify_main_hs_kernel does, into rows ([i][kJointRows][128 B]).
__global__ __launch_bounds__(kHsBlock) void test_joint_rows_kernel(const uint8_t *__restrict__ a,
                                                                   const uint8_t *__restrict__ r,
                                                                   const uint8_t *__restrict__ dneg, uint32_t n,
                                                                   int4 *__restrict__ rows) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t aw[8], rw[8];
  load_row_words(aw, a + 32 * (size_t)i, 2);
  load_row_words(rw, r + 32 * (size_t)i, 2);
  ge_p3 A, R, P, Q;
  ge_frombytes_go(A, aw);
  ge_frombytes_go(R, rw);
  hs_points(P, Q, dneg[i] != 0, A, R.X, R.Y);
  SlabTabJ tj{rows, i};
  build_table_joint(tj, P, Q);
}

hipError_t launch_test_joint_rows(const uint8_t *a, const uint8_t *r, const uint8_t *dneg, uint32_t n, int4 *rows,
                                  hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(test_joint_rows_kernel, dim3((n + kHsBlock - 1) / kHsBlock), dim3(kHsBlock), 0, stream, a, r,
                     dneg, n, rows);
  return hipGetLastError();
}

// Tests (tmed_test_lds_rows): the same table through the main kernel's accessor (SlabLdsTabJ: rows 1
// and 5 in the block's LDS array, the others in rows, whose lines 1 and 5 stay as the caller filled
// them), then every row 0..kJointRows read back through prefetch / take, swap false and true, into
// out ([i][row][swap][40 int32]: the limbs of Y+X, Y-X, Z, 2dT).
__global__ __launch_bounds__(kHsBlock) void test_lds_rows_kernel(const uint8_t *__restrict__ a,
                                                                 const uint8_t *__restrict__ r,
                                                                 const uint8_t *__restrict__ dneg, uint32_t n,
                                                                 int4 *__restrict__ rows, int32_t *__restrict__ out) {
  __shared__ int4 pq[kLdsRowsInt4];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t aw[8], rw[8];
  load_row_words(aw, a + 32 * (size_t)i, 2);
  load_row_words(rw, r + 32 * (size_t)i, 2);
  ge_p3 A, R, P, Q;
  ge_frombytes_go(A, aw);
  ge_frombytes_go(R, rw);
  hs_points(P, Q, dneg[i] != 0, A, R.X, R.Y);
  SlabLdsTabJ tj{rows + (size_t)blockIdx.x * blockDim.x * (kJointRows * 8), threadIdx.x, pq + threadIdx.x};
  build_table_joint(tj, P, Q);
  int32_t *o = out + (size_t)i * (kJointRows + 1) * 2 * 40;
#pragma unroll 1
  for (int j = 0; j <= kJointRows; j++) {
#pragma unroll 1
    for (int s = 0; s < 2; s++) {
      ge_cached c;
      tj.prefetch(j, s != 0);
      tj.take(c);
#pragma unroll
      for (int l = 0; l < 10; l++) {
        o[l] = c.YpX.v[l];
        o[10 + l] = c.YmX.v[l];
        o[20 + l] = c.Z.v[l];
        o[30 + l] = c.T2d.v[l];
      }
      o += 40;
    }
  }
}

hipError_t launch_test_lds_rows(const uint8_t *a, const uint8_t *r, const uint8_t *dneg, uint32_t n, int4 *rows,
                                int32_t *out, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(test_lds_rows_kernel, dim3((n + kHsBlock - 1) / kHsBlock), dim3(kHsBlock), 0, stream, a, r, dneg,
                     n, rows, out);
  return hipGetLastError();
}

// Tests (tmed_test_verify_k): words 0..7 of the first prep region (int4 rows 0 and 1 at slot, where
// verify_prep_kernel left k = H(R || A || M) mod L) overwritten with the caller's k of signature
// base + slot (k32: 32 little-endian bytes a signature, the whole batch's).  Launched between
// verify_prep_kernel and the chunk's next kernel, which reads k from there.
__global__ __launch_bounds__(kHsBlock) void test_set_k_kernel(const uint8_t *__restrict__ k32, uint32_t base,
                                                              uint32_t count, int4 *__restrict__ prep, uint32_t stride) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= count) return;
  uint32_t k[8];
  load_row_words(k, k32 + 32 * (size_t)(base + slot), 2);
#pragma unroll
  for (int q = 0; q < 2; q++)
    prep[(size_t)q * stride + slot] = make_int4((int)k[4 * q], (int)k[4 * q + 1], (int)k[4 * q + 2], (int)k[4 * q + 3]);
}

// (s_sleep 127 is ~8k clocks, ~3.4 us at 2.4 GHz; a bounded loop, no memory access)
__global__ __launch_bounds__(64) void test_delay_kernel(uint32_t iters) {
  for (uint32_t i = 0; i < iters; i++) __builtin_amdgcn_s_sleep(127);
}

hipError_t launch_test_delay(hipStream_t stream, uint32_t us) {
  if (us == 0) return hipSuccess;
  hipLaunchKernelGGL(test_delay_kernel, dim3(1), dim3(64), 0, stream, (us < 100000u ? us : 100000u) / 3u + 1u);
  return hipGetLastError();
}

hipError_t launch_window_stats(const int4 *prep, uint32_t stride, uint32_t count, uint32_t *d_hist,
                               hipStream_t stream) {
  if (count == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(d_hist, 0, 2 * 65 * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(window_stats_kernel, dim3((count + kThreadsPerBlock - 1) / kThreadsPerBlock),
                     dim3(kThreadsPerBlock), 0, stream, prep + (size_t)kPrepInt4 * stride, stride, count, d_hist,
                     d_hist + 65);
  return hipGetLastError();
}

// Phase 3: batched finish.  Lane l owns slots l, l + L, l + 2L, ... (< m) of the block of m
// signatures starting at fin_base (coalesced [q][slot] loads); finish_group inverts their
// Z with one inversion and compares each canonical encoding with R.
struct FinDev {
  const int4 *fin;
  int4 *pre;
  const uint8_t *sig;
  uint8_t *out;
  uint32_t fin_base, lane, L, m;
  const uint32_t *perm;  // position -> signature index (key-grouped order), or null
  __device__ __forceinline__ int count() const { return lane < m ? (int)((m - lane + L - 1) / L) : 0; }
  __device__ __forceinline__ uint32_t slot(int j) const { return lane + (uint32_t)j * L; }
  __device__ __forceinline__ void load_z(int j, fe &z) const {
    int32_t w[12];  // words 20..31
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const int4 v = fin[(size_t)(5 + q) * kFinCap + slot(j)];
      w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int i = 0; i < 10; i++) z.v[i] = w[i];
  }
  __device__ __forceinline__ void load_xy(int j, fe &X, fe &Y) const {
    int32_t w[20];  // words 0..19
#pragma unroll
    for (int q = 0; q < 5; q++) {
      const int4 v = fin[(size_t)q * kFinCap + slot(j)];
      w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int i = 0; i < 10; i++) { X.v[i] = w[i]; Y.v[i] = w[10 + i]; }
  }
  __device__ __forceinline__ void store_pre(int j, const fe &p) const {
    const size_t idx = (size_t)j * L + lane;
    pre[idx] = make_int4(p.v[0], p.v[1], p.v[2], p.v[3]);
    pre[kFinPreStride + idx] = make_int4(p.v[4], p.v[5], p.v[6], p.v[7]);
    pre[2 * (size_t)kFinPreStride + idx] = make_int4(p.v[8], p.v[9], 0, 0);
  }
  __device__ __forceinline__ void load_pre(int j, fe &p) const {
    const size_t idx = (size_t)j * L + lane;
    const int4 a = pre[idx], b = pre[kFinPreStride + idx], c = pre[2 * (size_t)kFinPreStride + idx];
    p.v[0] = a.x; p.v[1] = a.y; p.v[2] = a.z; p.v[3] = a.w;
    p.v[4] = b.x; p.v[5] = b.y; p.v[6] = b.z; p.v[7] = b.w;
    p.v[8] = c.x; p.v[9] = c.y;
  }
  __device__ __forceinline__ uint32_t sig_index(int j) const {
    const uint32_t p = fin_base + slot(j);
    return perm ? perm[p] : p;
  }
  __device__ __forceinline__ void load_r(int j, uint32_t Rw[8]) const {
    load_row_words(Rw, sig + 64 * (size_t)sig_index(j), 2);
  }
  __device__ __forceinline__ void result(int j, bool ok) const {
    uint8_t *o = out + sig_index(j);
    *o = (*o && ok) ? 1 : 0;
  }
};

__global__ __launch_bounds__(kThreadsPerBlock) void verify_finish_kernel(
    const int4 *__restrict__ fin, int4 *__restrict__ pre, const uint8_t *__restrict__ sig, uint8_t *__restrict__ out,
    uint32_t fin_base, uint32_t L, uint32_t m, const uint32_t *__restrict__ perm) {
  const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= L) return;
  FinDev a{fin, pre, sig, out, fin_base, lane, L, m, perm};
  finish_group(a);
}

// Finish launch for the m signatures at fin_base: group size G = ceil(m / 65536) clamped to
// [1, 16], so at most 65,536 lanes = one wave per SIMD: each lane pays one inversion per group,
// a latency-bound chain, and a SIMD holding two such waves runs them ~twice as long (a C4 batch of
// ~853k votes took 13 per group = 1,025 waves with the floor: C4 585 -> 591 M/s, profiles/r05/s17/).
hipError_t launch_finish(const int4 *fin, int4 *pre, const uint8_t *sig, uint8_t *out, uint32_t fin_base, uint32_t m,
                         hipStream_t stream, const uint32_t *perm) {
  if (m == 0) return hipSuccess;
  constexpr uint32_t kLanes = 65536;  // one inversion per lane and group; 65,536 lanes fill every SIMD
  uint32_t G = (m + kLanes - 1) / kLanes;
  if (G < 1) G = 1;
  if (G > kFinGroupMax) G = kFinGroupMax;
  const uint32_t L = (m + G - 1) / G;
  hipLaunchKernelGGL(verify_finish_kernel, dim3((L + kThreadsPerBlock - 1) / kThreadsPerBlock),
                     dim3(kThreadsPerBlock), 0, stream, fin, pre, sig, out, fin_base, L, m, perm);
  return hipGetLastError();
}

// Tests (tmed_test_finish): position p's X, Y, Z (30 limbs) into fin slot p as fin_store writes
// them, its R into the first half of signature row fin_base + p (perm[fin_base + p] with perm), and
// its bit into out at the same index.
__global__ __launch_bounds__(kThreadsPerBlock) void test_fin_fill_kernel(
    const int32_t *__restrict__ xyz, const uint8_t *__restrict__ r, const uint8_t *__restrict__ bits,
    const uint32_t *__restrict__ perm, uint32_t fin_base, uint32_t m, int4 *__restrict__ fin, uint8_t *__restrict__ sig,
    uint8_t *__restrict__ out) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= m) return;
  fe X, Y, Z;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    X.v[i] = xyz[30 * (size_t)p + i];
    Y.v[i] = xyz[30 * (size_t)p + 10 + i];
    Z.v[i] = xyz[30 * (size_t)p + 20 + i];
  }
  fin_store(fin, kFinCap, p, X, Y, Z);
  const uint32_t i = perm ? perm[fin_base + p] : fin_base + p;
  const uint4 *src = reinterpret_cast<const uint4 *>(r + 32 * (size_t)p);
  uint4 *dst = reinterpret_cast<uint4 *>(sig + 64 * (size_t)i);
  dst[0] = src[0];
  dst[1] = src[1];
  out[i] = bits[p];
}

hipError_t launch_test_fin_fill(const int32_t *xyz, const uint8_t *r, const uint8_t *bits, const uint32_t *perm,
                                uint32_t fin_base, uint32_t m, int4 *fin, uint8_t *sig, uint8_t *out,
                                hipStream_t stream) {
  if (m == 0 || m > kFinCap) return hipErrorInvalidValue;
  hipLaunchKernelGGL(test_fin_fill_kernel, dim3((m + kThreadsPerBlock - 1) / kThreadsPerBlock), dim3(kThreadsPerBlock),
                     0, stream, xyz, r, bits, perm, fin_base, m, fin, sig, out);
  return hipGetLastError();
}

hipError_t launch_verify(const uint8_t *pub, const uint8_t *sig, const uint8_t *msgs, const uint32_t *off,
                         uint32_t n, uint8_t *out, int4 *slab, uint32_t slab_stride, BTabs btab,
                         int4 *prep, int4 *fin, int4 *fin_pre, hipStream_t stream, uint32_t chunk, int main_waves,
                         bool msg_slots, KernelTimer *timer, bool zip215, const uint8_t *test_k) {
  const MsgSrc ms{msgs, off, msg_slots};
  // Chunks of at most slab_stride signatures (the per-lane tables and the prep hand-off are
  // sized for one chunk; tmed_init keeps both multiples of kThreadsPerBlock, so every lane of
  // every launched block owns a slot below slab_stride).  The finish (variant 5 only) runs
  // once per kFinCap block.
  if (chunk == 0 || chunk > slab_stride) chunk = slab_stride;
  if (chunk % kThreadsPerBlock != 0 || slab_stride % kThreadsPerBlock != 0) return hipErrorInvalidValue;
  const bool hs = main_waves != 5 || zip215;  // the ZIP-215 rule runs on the half-size path only
  // placement counters of the half-size hand-off: the tail of the prep allocation (kPrepTailBytes)
  uint32_t *place = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(prep) + (size_t)slab_stride * kPrepSlotBytes);
  if (timer) timer->mark(stream, -1);
  for (uint32_t fbase = 0; fbase < n; fbase += kFinCap) {
    const uint32_t m = (n - fbase) < kFinCap ? (n - fbase) : kFinCap;
    for (uint32_t base = fbase; base < fbase + m; base += chunk) {
      const uint32_t count = (fbase + m - base) < chunk ? (fbase + m - base) : chunk;
      const uint32_t blocks = (count + kThreadsPerBlock - 1) / kThreadsPerBlock;
      const uint32_t hblocks = (count + kHsBlock - 1) / kHsBlock;

      hipLaunchKernelGGL(verify_prep_kernel, dim3(hblocks), dim3(kHsBlock), 0, stream, pub, sig, ms, base,
                         count, prep, slab_stride, hs ? place : nullptr);
      if (test_k)  // tests only (tmed_test_verify_k): a chosen k in place of the hash
        hipLaunchKernelGGL(test_set_k_kernel, dim3(hblocks), dim3(kHsBlock), 0, stream, test_k, base, count, prep,
                           slab_stride);
      if (timer) timer->mark(stream, 0);
      if (hs) {  // default: half-size scalars (verify_hs.h): R decode + lattice, main; no finish
        int4 *prep2 = prep + (size_t)kPrepInt4 * slab_stride;
        hipLaunchKernelGGL(verify_prep_r_kernel, dim3(hblocks), dim3(kHsBlock), 0, stream, sig, base, count,
                           prep, prep2, slab_stride, place, zip215 ? 1 : 0);
        if (timer) timer->mark(stream, 0);
        if (btab.b26)
          hipLaunchKernelGGL(verify_main_hs_kernel<26>, dim3(hblocks), dim3(kHsBlock), 0, stream, base, count,
                             prep, prep2, slab_stride, slab, btab.b26, out, zip215 ? 1 : 0);
        else
          hipLaunchKernelGGL(verify_main_hs_kernel<16>, dim3(hblocks), dim3(kHsBlock), 0, stream, base, count,
                             prep, prep2, slab_stride, slab, btab.comb16, out, zip215 ? 1 : 0);
      } else {  // fallback 5: full-length Straus + batched finish
        hipLaunchKernelGGL(verify_main_kernel, dim3(blocks), dim3(kThreadsPerBlock), 0, stream, base, count, prep,
                           slab_stride, slab, btab.b16, fin, fbase, out);
      }
      if (timer) timer->mark(stream, 1);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
    hipError_t e = hs ? hipSuccess : launch_finish(fin, fin_pre, sig, out, fbase, m, stream);
    if (timer) timer->mark(stream, 2);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_verify_prep(const uint8_t *pub, const uint8_t *sig, const uint8_t *msgs, const uint32_t *off,
                              bool msg_slots, uint32_t base, uint32_t count, int4 *prep, uint32_t stride,
                              hipStream_t stream) {
  if (count == 0) return hipSuccess;
  if (count > stride) return hipErrorInvalidValue;
  const MsgSrc ms{msgs, off, msg_slots};
  hipLaunchKernelGGL(verify_prep_kernel, dim3((count + kHsBlock - 1) / kHsBlock),
                     dim3(kHsBlock), 0, stream, pub, sig, ms, base, count, prep, stride, nullptr);
  return hipGetLastError();
}

hipError_t launch_assemble_votes(const uint8_t *tmpl, const uint32_t *tmpl_idx, const uint8_t *flags,
                                 const int64_t *ts_sec, const int32_t *ts_nanos, uint32_t n, uint8_t *out,
                                 uint32_t *out_len, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(assemble_votes_kernel, dim3((n + kAsmLanes - 1) / kAsmLanes), dim3(kAsmLanes), 0, stream,
                     VoteAsm{tmpl, tmpl_idx, flags, ts_sec, ts_nanos}, n, out, out_len);
  return hipGetLastError();
}

// ============================================================ key-cached path
// The keyed prep and main kernels (throughput), the key-grouped visiting order, and the latency
// mode for small batches.  The signatures' keys are indices into a key set whose combs
// kernels_tables.hip built; the batched finish is launch_finish above.

constexpr int kKsPrepWaves = 4;  // 128 VGPRs, 4 spilled: keyed prep 0.347 -> 0.337 ms per 2^20 against 3 waves
                                 // (130 VGPRs), three alternating runs each (profiles/r04/s22)
__global__ __launch_bounds__(kThreadsPerBlock, kKsPrepWaves) void verify_keyset_prep_kernel(
    const uint32_t *__restrict__ val_idx, uint32_t nkeys, const uint8_t *__restrict__ key_pub,
    const uint8_t *__restrict__ key_ok, const uint8_t *__restrict__ sig, MsgSrc ms, uint32_t base, uint32_t count,
    int4 *__restrict__ prep, uint32_t stride) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= count) return;
  const uint32_t i = base + slot;
  const uint32_t vi = val_idx[i];
  const bool vin = vi < nkeys;  // an index past the key set rejects the signature (row 0 is read)
  const uint32_t v = vin ? vi : 0u;
  uint32_t pw[8], sw[16], k[8], s[8];
  load_row_words(pw, key_pub + 32 * (size_t)v, 2);
  load_row_words(sw, sig + 64 * (size_t)i, 4);
  const uint8_t *m;
  uint32_t mlen;
  ms.get(i, m, mlen);
  const bool ok = verify_prep_comb(pw, vin && key_ok[v] != 0, sw, m, mlen, k, s, ms.slots);  // slots: hashed from dwordx4 loads (sha512_stream_slot)
  prep_store_ks(prep, stride, slot, k, s, ok);
}

// Key-cached Straus with the next comb row in flight: the 48 rows a signature
// reads (32 from its key's radix-256 comb, 16 from the shared radix-2^16 comb of B) are random
// 128-B lines of a multi-GB table, so a row loaded right before its addition leaves the wave
// parked on HBM latency for most of it (rocprof: 0.35 of the mad peak, round 2).  Here the row
// of addition t+1 is loaded into registers before addition t runs.  Schedule per 32-bit word q
// of the recodings: A(4q), A(4q+1), B(2q), A(4q+2), A(4q+3), B(2q+1) — the same sum as
// verify_main_comb_point<16>.  The first addition starts from the identity, so it is replaced
// by the niels -> extended conversion (1 M instead of 7 M), and the last one stops at
// projective (X, Y, Z) (3 M instead of 4 M for p1p1 -> p3).  The six additions of a word stay
// unrolled: each step's role is then fixed at compile time.
struct CombRowPf {
  int4 pv[8];
  bool neg;
  __device__ __forceinline__ void fetch(const int4 *row, bool n) {
#pragma unroll
    for (int q = 0; q < 8; q++) pv[q] = row[q];
    neg = n;
  }
  __device__ __forceinline__ void take(ge_niels &e) const {
    niels_load(e, pv);
    niels_apply_sign(e, neg);
  }
};

__device__ __forceinline__ const int4 *ks_arow(const int4 *ak, int w, uint32_t byte, bool &neg) {
  const int d = (int)byte - 128;
  neg = d < 0;
  return ak + ((size_t)w * kCombEntries + (uint32_t)(neg ? -d : d)) * kCombEntryInt4;
}
__device__ __forceinline__ const int4 *ks_brow(const int4 *bc, int wb, uint32_t half, bool &neg) {
  const int d = (int)half - 32768;
  neg = d < 0;
  return bc + ((size_t)wb * kB16Entries + (uint32_t)(neg ? -d : d)) * kCombEntryInt4;
}

// out (X : Y : Z) = [k](-A) + [s]B from the key's comb (ak) and the radix-2^16 comb of B (bc).
__device__ __forceinline__ void keyset_straus_pf(ge_p2 &out, const uint32_t k[8], const uint32_t s[8],
                                                 const int4 *ak, const int4 *bc) {
  uint32_t kr[8], sr[8];
  sc_recode256(kr, k);
  sc_recode_b<16>(sr, s);
  CombRowPf pf;
  bool ng;
  pf.fetch(ks_arow(ak, 0, kr[0] & 0xffu, ng), ng);
  ge_p3 acc;
  ge_p1p1 t;
  ge_niels e;
#pragma unroll 1
  for (int q = 0; q < 8; q++) {
    const uint32_t kc = kr[0], sc = sr[0];
#pragma unroll
    for (int m = 0; m < 7; m++) { kr[m] = kr[m + 1]; sr[m] = sr[m + 1]; }
#pragma unroll
    for (int st = 0; st < 6; st++) {
      pf.take(e);
      // the row of the next addition: A byte, A byte, B half, A, A, B, then the next word's A byte 0
      const int nx = st + 1;
      const int4 *row;
      if (nx == 6) {
        row = ks_arow(ak, 4 * q + 4 < 32 ? 4 * q + 4 : 0, kr[0] & 0xffu, ng);  // past the end: any row
      } else if (nx == 2 || nx == 5) {
        row = ks_brow(bc, 2 * q + (nx == 5), (sc >> (nx == 5 ? 16 : 0)) & 0xffffu, ng);
      } else {
        const int b = nx < 2 ? nx : nx - 1;  // byte of kc
        row = ks_arow(ak, 4 * q + b, (kc >> (8 * b)) & 0xffu, ng);
      }
      if (q < 7 || st < 5) pf.fetch(row, ng);
      if (st == 0 && q == 0) {
        ge_niels_to_p3(acc, e);
      } else {
        ge_madd_niels(t, acc, e, false);
        if (q == 7 && st == 5) {
          ge_p1p1_to_p2(out, t);
        } else {
          ge_p1p1_to_p3(acc, t);
        }
      }
    }
  }
}

// out (X : Y : Z) = [k](-A) + [s]B with the radix-2^24 comb of B: the key's 32 radix-256 rows, then
// eleven B rows, d_m = bits [24m, 24m + 24) of s + bit (24m - 1) - 2^24 bit (24m + 23), read off a
// copy of s shifted right by 24 bits per row (no carry chain); 43 mixed additions, the row of
// addition t + 1 loaded while addition t runs.
__device__ __forceinline__ const int4 *ks_b24row(const int4 *bc, int w, int d, bool &neg) {
  neg = d < 0;
  return bc + ((size_t)w * kB24Entries + (uint32_t)(neg ? -d : d)) * kCombEntryInt4;
}
__device__ __forceinline__ void keyset_straus_b24(ge_p2 &out, const uint32_t k[8], const uint32_t s[8],
                                                  const int4 *ak, const int4 *bc) {
  uint32_t kr[8], sw[8];
  sc_recode256(kr, k);
#pragma unroll
  for (int i = 0; i < 8; i++) sw[i] = s[i];
  CombRowPf pf;
  bool ng;
  pf.fetch(ks_arow(ak, 0, kr[0] & 0xffu, ng), ng);
  ge_p3 acc;
  ge_p1p1 t;
  ge_niels e;
  // the key's 32 rows, four per word of the recoding
#pragma unroll 1
  for (int q = 0; q < 8; q++) {
    const uint32_t kc = kr[0];
#pragma unroll
    for (int m = 0; m < 7; m++) kr[m] = kr[m + 1];
#pragma unroll
    for (int b = 0; b < 4; b++) {
      pf.take(e);
      if (b < 3) {
        pf.fetch(ks_arow(ak, 4 * q + b + 1, (kc >> (8 * (b + 1))) & 0xffu, ng), ng);
      } else if (q < 7) {
        pf.fetch(ks_arow(ak, 4 * q + 4, kr[0] & 0xffu, ng), ng);
      } else {  // the first B row: digit 0
        const uint32_t u = sw[0] & 0xffffffu;
        pf.fetch(ks_b24row(bc, 0, (int)u - (int)((u >> 23) << 24), ng), ng);
      }
      if (q == 0 && b == 0) {
        ge_niels_to_p3(acc, e);
      } else {
        ge_madd_niels(t, acc, e, false);
        ge_p1p1_to_p3(acc, t);
      }
    }
  }
  // the eleven B rows; row m + 1's digit is read off s shifted right by 24 (m + 1) bits
#pragma unroll 1
  for (int m = 0; m < kB24Windows; m++) {
    pf.take(e);
    if (m + 1 < kB24Windows) {
      const uint32_t below = (sw[0] >> 23) & 1u;  // bit 24(m + 1) - 1
#pragma unroll
      for (int i = 0; i < 7; i++) sw[i] = __builtin_amdgcn_alignbit(sw[i + 1], sw[i], 24);
      sw[7] >>= 24;
      const uint32_t u = sw[0] & 0xffffffu;
      pf.fetch(ks_b24row(bc, m + 1, (int)(u + below) - (int)((u >> 23) << 24), ng), ng);
    }
    ge_madd_niels(t, acc, e, false);
    if (m + 1 == kB24Windows) ge_p1p1_to_p2(out, t);
    else ge_p1p1_to_p3(acc, t);
  }
}

// The same sum with -A from its radix-2^B comb (kernels.h kCombA*, B = 12: 21 A rows), then the
// eleven B rows.  Digit m of k is read off k shifted right by Bm bits (bits [Bm, Bm + B) plus the
// bit below, minus 2^B times the top bit of the field; the top digit is every bit left, unsigned).
__device__ __forceinline__ const int4 *ks_arow(const int4 *ak, int w, int d, bool &neg) {
  neg = d < 0;
  return ak + comba_row(w, (uint32_t)(neg ? -d : d)) * kCombEntryInt4;
}
__device__ __forceinline__ void keyset_straus_ab24(ge_p2 &out, const uint32_t k[8], const uint32_t s[8],
                                                   const int4 *ak, const int4 *bc) {
  uint32_t kw[8], sw[8];
#pragma unroll
  for (int i = 0; i < 8; i++) { kw[i] = k[i]; sw[i] = s[i]; }
  CombRowPf pf;
  bool ng;
  constexpr uint32_t kMask = (1u << kCombABits) - 1u;
  {
    const uint32_t u = kw[0] & kMask;
    pf.fetch(ks_arow(ak, 0, (int)u - (int)((u >> (kCombABits - 1)) << kCombABits), ng), ng);
  }
  ge_p3 acc;
  ge_p1p1 t;
  ge_niels e;
#pragma unroll 1
  for (int m = 0; m < kCombAWindows; m++) {
    pf.take(e);
    if (m + 1 < kCombAWindows) {
      const uint32_t below = (kw[0] >> (kCombABits - 1)) & 1u;  // bit B(m + 1) - 1
#pragma unroll
      for (int i = 0; i < 7; i++) kw[i] = __builtin_amdgcn_alignbit(kw[i + 1], kw[i], kCombABits);
      kw[7] >>= kCombABits;
      // the top window's digit: every bit left (k < L: bits B(W-1)..252) + the bit below, unsigned
      const bool last = m + 2 == kCombAWindows;
      const uint32_t u = last ? kw[0] : kw[0] & kMask;
      const int top = last ? 0 : (int)((u >> (kCombABits - 1)) << kCombABits);
      pf.fetch(ks_arow(ak, m + 1, (int)(u + below) - top, ng), ng);
    } else {  // the first B row: digit 0
      const uint32_t u = sw[0] & 0xffffffu;
      pf.fetch(ks_b24row(bc, 0, (int)u - (int)((u >> 23) << 24), ng), ng);
    }
    if (m == 0) {
      ge_niels_to_p3(acc, e);
    } else {
      ge_madd_niels(t, acc, e, false);
      ge_p1p1_to_p3(acc, t);
    }
  }
#pragma unroll 1
  for (int m = 0; m < kB24Windows; m++) {
    pf.take(e);
    if (m + 1 < kB24Windows) {
      const uint32_t below = (sw[0] >> 23) & 1u;
#pragma unroll
      for (int i = 0; i < 7; i++) sw[i] = __builtin_amdgcn_alignbit(sw[i + 1], sw[i], 24);
      sw[7] >>= 24;
      const uint32_t u = sw[0] & 0xffffffu;
      pf.fetch(ks_b24row(bc, m + 1, (int)(u + below) - (int)((u >> 23) << 24), ng), ng);
    }
    ge_madd_niels(t, acc, e, false);
    if (m + 1 == kB24Windows) ge_p1p1_to_p2(out, t);
    else ge_p1p1_to_p3(acc, t);
  }
}

// First row of key v's comb in a chunked key set (kernels.h kKeyChunk*): one 8-B table load per
// signature in front of its first comb row.
__device__ __forceinline__ const int4 *key_rows(const int4 *const *__restrict__ tab, uint32_t v, size_t int4_per_key) {
  return tab[v >> kKeyChunkBits] + (size_t)(v & (kKeyChunkKeys - 1)) * int4_per_key;
}

template <int WAVES, bool B24 = false, bool ACOMB = false>
__global__ __launch_bounds__(kThreadsPerBlock, WAVES) void verify_keyset_main_kernel(
    const uint32_t *__restrict__ val_idx, uint32_t nkeys, const int4 *const *__restrict__ acomb,
    const int4 *__restrict__ bcomb, uint32_t base, uint32_t count, const int4 *__restrict__ prep, uint32_t stride,
    int4 *__restrict__ fin, uint32_t fin_base, uint8_t *__restrict__ out, const uint32_t *__restrict__ perm) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= count) return;
  // visiting position pos (key-grouped when perm is set: perm holds this chunk's signature
  // indices, so the prep hand-off of signature i is at slot i - base)
  const uint32_t pos = base + slot;
  const uint32_t i = perm ? perm[pos] : pos;
  const uint32_t ps = i - base;
  const uint32_t vi = val_idx[i];
  const uint32_t v = vi < nkeys ? vi : 0u;  // the prep kernel rejected an index past the key set
  uint32_t k[8], s[8];
  int32_t w[16];
#pragma unroll
  for (int q = 0; q < 4; q++) {  // k, s; ok at word 36
    const int4 x = prep[(size_t)q * stride + ps];
    w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w;
  }
  const bool ok = prep[(size_t)9 * stride + ps].x != 0;
#pragma unroll
  for (int j = 0; j < 8; j++) { k[j] = (uint32_t)w[j]; s[j] = (uint32_t)w[8 + j]; }
  ge_p2 R;
  if (ACOMB) keyset_straus_ab24(R, k, s, key_rows(acomb, v, kCombARowsPerKey * kCombEntryInt4), bcomb);
  else if (B24) keyset_straus_b24(R, k, s, key_rows(acomb, v, (size_t)kCombWindows * kCombEntries * kCombEntryInt4), bcomb);
  else keyset_straus_pf(R, k, s, key_rows(acomb, v, (size_t)kCombWindows * kCombEntries * kCombEntryInt4), bcomb);
  fin_store(fin, kFinCap, pos - fin_base, R.X, R.Y, R.Z);
  out[i] = ok ? 1 : 0;
}

// ---- key-grouped visiting order (launch_key_order) -------------------------------------
// A counting sort of one chunk's signatures by key group (G consecutive keys per bin, G a power
// of two chosen so that at most kKeyBins bins exist; indices past the key set form the last
// bin).  Random-address global atomics run far below the streaming rate on this part, so every
// tile of kKeyTile signatures counts in LDS and touches the global counters once per non-empty
// bin, 64 consecutive bins per wave instruction: (1) per-bin totals, (2) one block turns them
// into bin starts, (3) each tile reserves its range of every bin and places its signatures at
// LDS-atomic ranks inside it (the order inside a bin is irrelevant).
constexpr uint32_t kKeyBins = 4096, kKeyTile = 4096;

__device__ __forceinline__ uint32_t key_bin(uint32_t v, uint32_t nkeys, uint32_t shift) {
  return v < nkeys ? (v >> shift) : ((nkeys - 1) >> shift) + 1;
}

__global__ __launch_bounds__(256) void key_hist_kernel(const uint32_t *__restrict__ val_idx, uint32_t n,
                                                       uint32_t nkeys, uint32_t shift, uint32_t nbins,
                                                       uint32_t *__restrict__ total) {
  __shared__ uint32_t h[kKeyBins];
  for (uint32_t b = threadIdx.x; b < nbins; b += blockDim.x) h[b] = 0;
  __syncthreads();
  const uint32_t t0 = blockIdx.x * kKeyTile;
  for (uint32_t j = threadIdx.x; j < kKeyTile; j += blockDim.x) {
    const uint32_t i = t0 + j;
    if (i < n) atomicAdd(&h[key_bin(val_idx[i], nkeys, shift)], 1u);
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nbins; b += blockDim.x)
    if (h[b]) atomicAdd(&total[b], h[b]);
}

// Exclusive prefix sum of cnt[0..m) in place, one 1024-lane block (m <= kKeyBins): lane t scans
// a contiguous run, the run totals are scanned in LDS, then the runs are rebased.
__global__ __launch_bounds__(1024) void key_scan_kernel(uint32_t *__restrict__ cnt, uint32_t m) {
  __shared__ uint32_t tot[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (m + 1023) / 1024, lo = t * per, hi = lo + per < m ? lo + per : m;
  uint32_t s = 0;
  for (uint32_t j = lo; j < hi; j++) s += cnt[j];
  tot[t] = s;
  __syncthreads();
  for (uint32_t o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan of the run totals
    const uint32_t x = t >= o ? tot[t - o] : 0u;
    __syncthreads();
    tot[t] += x;
    __syncthreads();
  }
  uint32_t acc = t ? tot[t - 1] : 0u;
  for (uint32_t j = lo; j < hi; j++) {
    const uint32_t c = cnt[j];
    cnt[j] = acc;
    acc += c;
  }
}

__global__ __launch_bounds__(256) void key_scatter_kernel(const uint32_t *__restrict__ val_idx, uint32_t n,
                                                          uint32_t nkeys, uint32_t shift, uint32_t nbins,
                                                          uint32_t *__restrict__ cursor, uint32_t index_base,
                                                          uint32_t *__restrict__ perm) {
  __shared__ uint32_t h[kKeyBins];
  for (uint32_t b = threadIdx.x; b < nbins; b += blockDim.x) h[b] = 0;
  __syncthreads();
  const uint32_t t0 = blockIdx.x * kKeyTile;
  for (uint32_t j = threadIdx.x; j < kKeyTile; j += blockDim.x) {
    const uint32_t i = t0 + j;
    if (i < n) atomicAdd(&h[key_bin(val_idx[i], nkeys, shift)], 1u);
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nbins; b += blockDim.x)
    h[b] = h[b] ? atomicAdd(&cursor[b], h[b]) : 0u;  // this tile's range of bin b
  __syncthreads();
  for (uint32_t j = threadIdx.x; j < kKeyTile; j += blockDim.x) {
    const uint32_t i = t0 + j;
    if (i < n) perm[atomicAdd(&h[key_bin(val_idx[i], nkeys, shift)], 1u)] = index_base + i;
  }
}

uint32_t key_order_shift(uint32_t nkeys) {
  uint32_t shift = 0;
  while (((nkeys - 1) >> shift) + 2 > kKeyBins) shift++;
  return shift;
}

uint32_t key_order_scratch_words(uint32_t n, uint32_t nkeys) {
  (void)n;
  return ((nkeys - 1) >> key_order_shift(nkeys)) + 2;
}

hipError_t launch_key_order(const uint32_t *val_idx, uint32_t n, uint32_t nkeys, uint32_t *scratch, uint32_t *perm,
                            uint32_t index_base, hipStream_t stream) {
  if (nkeys == 0 || nkeys > kKeyOrderMaxKeys) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const uint32_t shift = key_order_shift(nkeys), nbins = ((nkeys - 1) >> shift) + 2;
  const uint32_t ntiles = (n + kKeyTile - 1) / kKeyTile;
  hipError_t e = hipMemsetAsync(scratch, 0, (size_t)nbins * 4, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(key_hist_kernel, dim3(ntiles), dim3(256), 0, stream, val_idx, n, nkeys, shift, nbins, scratch);
  hipLaunchKernelGGL(key_scan_kernel, dim3(1), dim3(1024), 0, stream, scratch, nbins);
  hipLaunchKernelGGL(key_scatter_kernel, dim3(ntiles), dim3(256), 0, stream, val_idx, n, nkeys, shift, nbins, scratch,
                     index_base, perm);
  return hipGetLastError();
}

// ---- latency mode (verify_core.h): small key-cached batches ------------------------------
// One launch, two roles by block (64-lane blocks; the R blocks come first so the longest
// chain is dispatched first):
//  * blocks [0, nR): lane i strictly decodes R of signature i -> (x_R, y_R, ok) in dec;
//  * blocks [nR, nR + nC): 8 lanes per signature; every lane of the group hashes (the same
//    SHA-512, so no divergence), lane r sums its 8 comb entries, three __shfl_down steps
//    add the partial sums, lane 0 writes R' (fin) and the prep verdict (out).
// verify_lat_finish_kernel then compares projectively.  dec layout: [q][i], q < 6 int4.
constexpr int kLatDecInt4 = 6;

__device__ __forceinline__ void shfl_down_fe(fe &o, const fe &f, int L) {
#pragma unroll
  for (int i = 0; i < 10; i++) o.v[i] = __shfl_down(f.v[i], (unsigned)L, kLatLanes);
}

// comb_partial (verify_core.h) with the next comb row in flight and the first row converted
// instead of added to the identity: lane rr's 8 rows are A(w), B(w) for w = rr, rr+8, rr+16, rr+24.
__device__ __forceinline__ const int4 *lat_row(const int4 *comb, int w, uint32_t byte, bool &neg) {
  const int d = (int)byte - 128;
  neg = d < 0;
  return comb + ((size_t)w * kCombEntries + (uint32_t)(neg ? -d : d)) * kCombEntryInt4;
}
__device__ __forceinline__ void comb_partial_pf(ge_p3 &acc, const uint32_t kr[8], const uint32_t sr[8], int rr,
                                                const int4 *ac, const int4 *bc) {
  const int sh = 8 * (rr & 3);
  CombRowPf pf;
  bool ng;
  pf.fetch(lat_row(ac, rr, ((rr & 4) ? kr[1] : kr[0]) >> sh & 0xffu, ng), ng);
  ge_p1p1 t;
  ge_niels e;
#pragma unroll
  for (int st = 0; st < 8; st++) {
    const int q = st >> 1;
    pf.take(e);
    if (st < 7) {  // the row of step st + 1
      const int nq = (st + 1) >> 1, w = rr + 8 * nq;
      const uint32_t word = (st + 1) & 1 ? ((rr & 4) ? sr[2 * nq + 1] : sr[2 * nq])
                                         : ((rr & 4) ? kr[2 * nq + 1] : kr[2 * nq]);
      pf.fetch(lat_row((st + 1) & 1 ? bc : ac, w, (word >> sh) & 0xffu, ng), ng);
    }
    (void)q;
    if (st == 0) {
      ge_niels_to_p3(acc, e);
    } else {
      ge_madd_niels(t, acc, e, false);
      ge_p1p1_to_p3(acc, t);
    }
  }
}

__global__ __launch_bounds__(64) void verify_keyset_lat_kernel(
    const uint32_t *__restrict__ val_idx, uint32_t nkeys, const uint8_t *__restrict__ key_pub,
    const uint8_t *__restrict__ key_ok,
    const int4 *const *__restrict__ acomb, const int4 *__restrict__ bcomb, const uint8_t *__restrict__ sig, MsgSrc ms,
    uint32_t m, uint32_t nR, int4 *__restrict__ fin, int4 *__restrict__ dec, uint8_t *__restrict__ out, VoteAsm va,
    int assemble) {
  __shared__ int4 tl[64][kVoteTmplBytes / 16];  // the comb lanes' vote templates (assemble_vote)
  if (blockIdx.x < nR) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= m) return;
    uint32_t Rw[8];
    load_row_words(Rw, sig + 64 * (size_t)i, 2);
    fe x, y;
    const bool ok = r_decode_strict(x, y, Rw);
    int32_t w[24];
#pragma unroll
    for (int j = 0; j < 10; j++) { w[j] = x.v[j]; w[10 + j] = y.v[j]; }
    w[20] = ok ? 1 : 0;
    w[21] = w[22] = w[23] = 0;
#pragma unroll
    for (int q = 0; q < kLatDecInt4; q++) dec[(size_t)q * m + i] = make_int4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    return;
  }
  const uint32_t g = (blockIdx.x - nR) * (64 / kLatLanes) + (threadIdx.x / kLatLanes);
  const int r = (int)(threadIdx.x % kLatLanes);
  if (g >= m) return;  // whole 8-lane groups leave together: the shuffles stay inside live groups
  if (assemble) assemble_vote(va, g, const_cast<uint8_t *>(ms.msgs), const_cast<uint32_t *>(ms.off), tl[threadIdx.x]);
  const uint32_t vi = val_idx[g];
  const bool vin = vi < nkeys;  // an index past the key set rejects the signature (row 0 is read)
  const uint32_t v = vin ? vi : 0u;
  uint32_t pw[8], sw[16], k[8], s[8], kr[8], sr[8];
  load_row_words(pw, key_pub + 32 * (size_t)v, 2);
  load_row_words(sw, sig + 64 * (size_t)g, 4);
  const uint8_t *msg;
  uint32_t mlen;
  ms.get(g, msg, mlen);
  const bool ok = verify_prep_comb(pw, vin && key_ok[v] != 0, sw, msg, mlen, k, s);
  sc_recode256(kr, k);
  sc_recode256(sr, s);
  ge_p3 acc, o;
  comb_partial_pf(acc, kr, sr, r, key_rows(acomb, v, (size_t)kCombWindows * kCombEntries * kCombEntryInt4), bcomb);
#pragma unroll 1
  for (int L = 1; L < kLatLanes; L <<= 1) {
    shfl_down_fe(o.X, acc.X, L);
    shfl_down_fe(o.Y, acc.Y, L);
    shfl_down_fe(o.Z, acc.Z, L);
    shfl_down_fe(o.T, acc.T, L);
    ge_p3_add(acc, o);
  }
  if (r == 0) {
    fin_store(fin, kFinCap, g, acc.X, acc.Y, acc.Z);
    out[g] = ok ? 1 : 0;
  }
}

__global__ __launch_bounds__(kThreadsPerBlock) void verify_lat_finish_kernel(const int4 *__restrict__ fin,
                                                                            const int4 *__restrict__ dec, uint32_t m,
                                                                            uint8_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  int32_t w[32];
#pragma unroll
  for (int q = 0; q < kFinInt4; q++) {
    const int4 t = fin[(size_t)q * kFinCap + i];
    w[4 * q] = t.x; w[4 * q + 1] = t.y; w[4 * q + 2] = t.z; w[4 * q + 3] = t.w;
  }
  fe X, Y, Z, x, y;
#pragma unroll
  for (int j = 0; j < 10; j++) { X.v[j] = w[j]; Y.v[j] = w[10 + j]; Z.v[j] = w[20 + j]; }
#pragma unroll
  for (int q = 0; q < kLatDecInt4; q++) {
    const int4 t = dec[(size_t)q * m + i];
    w[4 * q] = t.x; w[4 * q + 1] = t.y; w[4 * q + 2] = t.z; w[4 * q + 3] = t.w;
  }
#pragma unroll
  for (int j = 0; j < 10; j++) { x.v[j] = w[j]; y.v[j] = w[10 + j]; }
  const bool ok = out[i] && w[20] && projective_matches(X, Y, Z, x, y);
  out[i] = ok ? 1 : 0;
}

hipError_t launch_verify_keyset_lat(const uint32_t *val_idx, uint32_t nkeys, const uint8_t *key_pub, const uint8_t *key_ok,
                                    const int4 *const *acomb, const int4 *bcomb, const uint8_t *sig, const uint8_t *msgs,
                                    const uint32_t *off, uint32_t n, uint8_t *out, int4 *fin, int4 *dec,
                                    hipStream_t stream, bool msg_slots, const VoteAsm *va, int rule) {
  if (n == 0) return hipSuccess;
  if (n > kLatMax) return hipErrorInvalidValue;  // fin / dec are sized for kLatMax signatures
  if (va && !msg_slots) return hipErrorInvalidValue;
  const MsgSrc ms{msgs, off, msg_slots};
  static_assert(kLatDecInt4 == kLatDecRows, "dec layout shared with zip_finish.hip");
  const uint32_t nR = (n + 63) / 64, nC = (n + 64 / kLatLanes - 1) / (64 / kLatLanes);
  hipLaunchKernelGGL(verify_keyset_lat_kernel, dim3(nR + nC), dim3(64), 0, stream, val_idx, nkeys, key_pub, key_ok, acomb,
                     bcomb, sig, ms, n, nR, fin, dec, out, va ? *va : VoteAsm{}, va ? 1 : 0);
  if (rule == kRuleZip215) {  // R from the R blocks' decode where it is canonical: zip_finish.hip
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : launch_lat_finish_zip(fin, dec, sig, out, n, stream);
  }
  hipLaunchKernelGGL(verify_lat_finish_kernel, dim3((n + kThreadsPerBlock - 1) / kThreadsPerBlock),
                     dim3(kThreadsPerBlock), 0, stream, fin, dec, n, out);
  return hipGetLastError();
}

hipError_t launch_verify_keyset(const uint32_t *val_idx, uint32_t nkeys, const uint8_t *key_pub, const uint8_t *key_ok,
                                const int4 *const *acomb, const int4 *bcomb, const uint8_t *sig, const uint8_t *msgs,
                                const uint32_t *off, uint32_t n, uint8_t *out, int4 *prep, uint32_t stride,
                                int4 *fin, int4 *fin_pre, hipStream_t stream, bool msg_slots, KernelTimer *timer,
                                uint32_t *perm, uint32_t *order_scratch, const int4 *bcomb24,
                                const int4 *const *acomba, int rule) {
  const MsgSrc ms{msgs, off, msg_slots};
  if (stride > kFinCap) stride = kFinCap;
  if (timer) timer->mark(stream, -1);
  for (uint32_t fbase = 0; fbase < n; fbase += kFinCap) {
    const uint32_t m = (n - fbase) < kFinCap ? (n - fbase) : kFinCap;
    for (uint32_t base = fbase; base < fbase + m; base += stride) {
      const uint32_t count = (fbase + m - base) < stride ? (fbase + m - base) : stride;
      const uint32_t blocks = (count + kThreadsPerBlock - 1) / kThreadsPerBlock;
      if (perm) {  // key-grouped visiting order of this chunk (main + finish)
        hipError_t e = launch_key_order(val_idx + base, count, nkeys, order_scratch, perm + base, base, stream);
        if (e != hipSuccess) return e;
      }
      hipLaunchKernelGGL(verify_keyset_prep_kernel, dim3(blocks), dim3(kThreadsPerBlock), 0, stream, val_idx,
                         nkeys, key_pub, key_ok, sig, ms, base, count, prep, stride);
      if (timer) timer->mark(stream, 0);
      if (bcomb24 && acomba)
        hipLaunchKernelGGL((verify_keyset_main_kernel<2, true, true>), dim3(blocks), dim3(kThreadsPerBlock), 0, stream,
                           val_idx, nkeys, acomba, bcomb24, base, count, prep, stride, fin, fbase, out, perm);
      else if (bcomb24)
        hipLaunchKernelGGL((verify_keyset_main_kernel<2, true>), dim3(blocks), dim3(kThreadsPerBlock), 0, stream,
                           val_idx, nkeys, acomb, bcomb24, base, count, prep, stride, fin, fbase, out, perm);
      else
        hipLaunchKernelGGL(verify_keyset_main_kernel<2>, dim3(blocks), dim3(kThreadsPerBlock), 0, stream, val_idx,
                           nkeys, acomb, bcomb, base, count, prep, stride, fin, fbase, out, perm);
      if (timer) timer->mark(stream, 1);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
    hipError_t e = rule == kRuleZip215 ? launch_finish_zip(fin, sig, out, fbase, m, stream, perm)
                                       : launch_finish(fin, fin_pre, sig, out, fbase, m, stream, perm);
    if (timer) timer->mark(stream, 2);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ============================================================ signer
__device__ void comb_sign_one(uint32_t sg[16], uint32_t pb[8], const uint32_t seed[8], const uint8_t *m,
                              uint32_t mlen, const int4 *bcomb) {
  const GlobalComb bc{bcomb};
  sign_one_bm(sg, pb, seed, m, mlen, [&](uint32_t enc[8], const uint32_t s[8]) { comb_base_mult(enc, s, bc); });
}

// RFC 8032 signer for synthetic commits: [a]B and [r]B from the shared comb of B.
__global__ __launch_bounds__(kThreadsPerBlock) void sign_kernel(
    const uint8_t *__restrict__ seeds, const uint8_t *__restrict__ msgs, const uint32_t *__restrict__ off,
    uint32_t n, uint8_t *__restrict__ sig_out, uint8_t *__restrict__ pub_out, const int4 *__restrict__ bcomb) {
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  for (uint32_t i = gtid; i < n; i += gridDim.x * blockDim.x) {
    uint32_t seed[8], sg[16], pb[8];
    load_row_words(seed, seeds + 32 * (size_t)i, 2);
    const uint32_t o0 = off[i], o1 = off[i + 1];
    comb_sign_one(sg, pb, seed, msgs + o0, o1 - o0, bcomb);
    uint4 *so = reinterpret_cast<uint4 *>(sig_out + 64 * (size_t)i);
#pragma unroll
    for (int q = 0; q < 4; q++) so[q] = make_uint4(sg[4 * q], sg[4 * q + 1], sg[4 * q + 2], sg[4 * q + 3]);
    uint4 *po = reinterpret_cast<uint4 *>(pub_out + 32 * (size_t)i);
#pragma unroll
    for (int q = 0; q < 2; q++) po[q] = make_uint4(pb[4 * q], pb[4 * q + 1], pb[4 * q + 2], pb[4 * q + 3]);
  }
}

static uint32_t grid_for(size_t n, uint32_t max_blocks) {
  size_t b = (n + kThreadsPerBlock - 1) / kThreadsPerBlock;
  if (b > max_blocks) b = max_blocks;
  if (b == 0) b = 1;
  return (uint32_t)b;
}

hipError_t launch_sign(const uint8_t *seeds, const uint8_t *msgs, const uint32_t *off, uint32_t n, uint8_t *sig_out,
                       uint8_t *pub_out, const int4 *bcomb, hipStream_t stream) {
  const uint32_t grid = grid_for(n, 4096);
  hipLaunchKernelGGL(sign_kernel, dim3(grid), dim3(kThreadsPerBlock), 0, stream, seeds, msgs, off, n, sig_out,
                     pub_out, bcomb);
  return hipGetLastError();
}

}  // namespace tmed
