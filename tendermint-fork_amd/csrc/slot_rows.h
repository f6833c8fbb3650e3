// slot_rows.h — what the one-wavefront slot kernels share on the device: assemble_votes_kernel
// (kernels.hip), vote_prepare_kernel (votes.hip), evidence_prepare_kernel and evidence_hash_kernel
// (evidence.hip).  Each runs one lane per item in workgroups of kSlotLanes, stages the item's records
// into the lane's own LDS row, builds its message in the lane's LDS slots and, in the first three,
// has the wavefront write the slots out together.  The __shared__ arrays stay in the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "signbytes.h"

namespace tmed {

constexpr uint32_t kSlotLanes = 64;           // one wavefront per workgroup
constexpr uint32_t kSlotInt4 = kVoteSlot / 16;  // 16 int4 a slot

// N int4 rows of src into this lane's LDS row: every load first, then the stores, so the loads are
// issued together.
template <int N>
__device__ __forceinline__ void lds_stage(int4 *lds_row, const int4 *src) {
  int4 v[N];
#pragma unroll
  for (int q = 0; q < N; q++) v[q] = src[q];
#pragma unroll
  for (int q = 0; q < N; q++) lds_row[q] = v[q];
}

template <int N>
__device__ __forceinline__ void lds_zero(int4 *lds_row) {
#pragma unroll
  for (int q = 0; q < N; q++) lds_row[q] = make_int4(0, 0, 0, 0);
}

// The wavefront's slots, kSlotsPerLane of kVoteSlot bytes a lane and consecutive in ob (LDS) as in
// slots (global, item i's first slot at kSlotsPerLane * i), written out as coalesced 1-KB rows: lane l
// stores int4 l of each row.  The caller's __syncthreads() comes first; i0 is the workgroup's first
// item, n the launch's item count (the last workgroup writes the slots of its n - i0 items only).
// Written straight into the global slots, each lane's ~114 byte stores went to 64 different lines per
// instruction: 0.29 ms per 853k-vote blocksync batch (profiles/r03/fin2/kernel_stats.csv).
template <uint32_t kSlotsPerLane>
__device__ __forceinline__ void wave_store_slots(const int4 *ob, uint8_t *slots, uint32_t i0, uint32_t n) {
  const uint32_t lane = threadIdx.x;
  const uint32_t nslots = kSlotsPerLane * (n - i0 < kSlotLanes ? n - i0 : kSlotLanes);
  int4 *dst = reinterpret_cast<int4 *>(slots + (size_t)kSlotsPerLane * i0 * kVoteSlot);
#pragma unroll
  for (uint32_t q = 0; q < kSlotsPerLane * kSlotInt4; q++) {
    const uint32_t c = q * kSlotLanes + lane;  // int4 index in the wavefront's run of slots
    if (c / kSlotInt4 < nslots) dst[c] = ob[c];
  }
}

// A key's 32 bytes, read as two int4 rows, as the eight little-endian words the address check hashes
// (the host twin: votes_host.h key_words).
__device__ __forceinline__ void key_words(int4 a, int4 b, uint32_t w[8]) {
  w[0] = (uint32_t)a.x; w[1] = (uint32_t)a.y; w[2] = (uint32_t)a.z; w[3] = (uint32_t)a.w;
  w[4] = (uint32_t)b.x; w[5] = (uint32_t)b.y; w[6] = (uint32_t)b.z; w[7] = (uint32_t)b.w;
}

}  // namespace tmed
