// validate.hip — block validation on gfx950: the device half of tmed_validate_blocks
// (include/tmed25519.h states the call; validate_host.h is the replay of validateBlock,
// state/validation.go:15-151, and commit.hip holds the entry point beside tmed_light_verify).
//
// validate_hashes_locked is phase A under one hold of the context's lock: Commit.Hash, Data.Hash,
// EvidenceList.Hash, Header.Hash and ValidatorSet.Hash by the routines of their own entry points
// (merkle.hip, evidence.hip), each distinct tmed_valset pointer hashed once, then block_check_kernel.
// The last commits' flags, addresses, timestamps and signatures are staged ONCE, into the arena
// tmed_ctx::vb_commit (commit_hashes_held with a CommitArena): the CommitSig leaf kernel reads them
// there, and so do the median kernels of phase B (median_times_locked with a MedShared).  Every hash
// routine leaves its roots on the device too, as rows of 32 bytes in tmed_ctx::d_vb (a copy on the
// stream beside the copy to the host, which the error values need).
//
// block_check_kernel: one wavefront per block, kCheckWaves = 4 blocks per 256-thread workgroup, no LDS
// and no barrier.  A block's 256-byte record holds the header's six 32-byte fields (LastCommitHash,
// DataHash, EvidenceHash, ValidatorsHash, NextValidatorsHash, LastBlockID.Hash) and, per field, the row
// of d_vb that holds the computed value: lanes 0..47 compare one dword each against the device-resident
// hashes, one ballot gives the 48 results, and lane 0 folds them into the block's mask of mismatches
// under its enable word (a compare the host decides alone, a field of another length or a skipped
// check, is not enabled and its row is not read).  The same wave then runs GetByAddress for
// ProposerAddress over the set's staged addresses (addr_scan.h wave_first_address, the scan of
// evidence_lookup_kernel: a 10,000-address set is 157 strides of one wavefront) and lane 0 writes the
// found index or kEvNone.  Every branch is wave-uniform: the block index, the enable word and the
// set's size are the same in all 64 lanes, so each ballot sees the whole wavefront.
#include <hip/hip_runtime.h>
#include <string.h>

#include <unordered_map>
#include <vector>

#include "../../include/tmed25519.h"
#include "addr_scan.h"
#include "call_frame.h"
#include "slot_batch.h"
#include "validate_host.h"

namespace tmed {

namespace V = tmed_validate;

constexpr uint32_t kCheckWaves = 4;  // blocks per workgroup

// One block: `want` the header's fields (slot s at dwords [8 s, 8 s + 8)), row[s] the row of the hash
// table that holds slot s's computed value, the proposer's address, the enable word (validate_host.h
// kCmp*), its set's size and first address.
struct BlockCheckRec {
  uint32_t want[48];
  uint32_t row[6];
  uint32_t addr[5];
  uint32_t enable, n_vals, pad;
  uint64_t set_base;
};
static_assert(sizeof(BlockCheckRec) == 256, "BlockCheckRec layout");

__global__ __launch_bounds__(64 * kCheckWaves) void block_check_kernel(const BlockCheckRec *__restrict__ recs, uint32_t n,
                                                                      const uint32_t *__restrict__ hashes, uint32_t n_rows,
                                                                      const uint32_t *__restrict__ set_addr,
                                                                      uint2 *__restrict__ out) {
  const uint32_t g = blockIdx.x * kCheckWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (g >= n) return;  // a whole wavefront; the kernel has no barrier
  const BlockCheckRec &r = recs[g];
  const uint32_t enable = r.enable;
  bool differ = false;
  if (lane < 48) {
    const uint32_t slot = lane >> 3, row = r.row[slot];
    if ((enable >> slot & 1) && row < n_rows) differ = r.want[lane] != hashes[8 * (size_t)row + (lane & 7)];
  }
  const unsigned long long d = __ballot(differ);  // all 64 lanes are here
  uint32_t mask = 0;
#pragma unroll
  for (int s = 0; s < V::kCompares; s++) mask |= ((d >> (8 * s)) & 0xffull) ? 1u << s : 0u;
  uint32_t found = kEvNone;
  if (enable & V::kCmpLookup) {  // wave-uniform
    uint32_t want[5];
#pragma unroll
    for (int q = 0; q < 5; q++) want[q] = r.addr[q];
    found = wave_first_address(want, set_addr + 5 * r.set_base, r.n_vals, lane);
  }
  if (lane == 0) out[g] = make_uint2(mask, found);
}

int validate_hashes_locked(tmed_ctx *c, const V::Plan &plan, V::Hashes &H, MedShared *shared, CommitArena *arena,
                           uint64_t *gen) {
  const tmed_block_batch &b = *plan.b;
  const size_t n = b.n, m = plan.need.size(), k = plan.need_hdr.size();
  c->last_vb_ms = 0.f;
  c->vb_stats[0] = c->vb_stats[1] = c->vb_stats[2] = 0;
  // the distinct known sets
  std::unordered_map<const tmed_valset *, size_t> set_of;
  std::vector<const tmed_valset *> hsets;
  for (const size_t i : plan.need) {
    const tmed_block_request &r = b.blocks[i];
    for (const tmed_valset *vs : {V::knows(r, TMED_VB_KNOW_VALIDATORS) ? r.state->validators : nullptr,
                                  V::knows(r, TMED_VB_KNOW_NEXT_VALIDATORS) ? r.state->next_validators : nullptr})
      if (vs && set_of.emplace(vs, hsets.size()).second) hsets.push_back(vs);
  }
  // the hash table on the device: rows of 32 bytes
  const size_t r_commit = 0, r_data = r_commit + m, r_ev = r_data + n, r_hdr = r_ev + n, r_set = r_hdr + k,
               n_rows = r_set + hsets.size();
  if (n_rows > 0x7fffffffu) return TMED_EINVAL;
  (void)hipSetDevice(c->device);
  hipStream_t s = c->stream;
  hipError_t e = c->d_vb.ensure(32 * n_rows);
  if (e != hipSuccess) return map_err(e);
  uint8_t *tab = (uint8_t *)c->d_vb.p;
  // Commit.Hash of the plan's commits; their arrays stay in the arena
  {
    std::vector<const tmed_commit *> cs(m);  // pointers: no struct is copied
    for (size_t j = 0; j < m; j++) cs[j] = b.blocks[plan.need[j]].last_commit;
    std::vector<uint8_t> out(32 * m), ok(m);
    *gen = ++c->vb_gen;
    const int rc = commit_hashes_held(c, cs.data(), m, out.data(), ok.data(), arena);
    if (rc != TMED_OK) return rc;
    e = hipMemcpyAsync(tab + 32 * r_commit, arena->roots, 32 * m, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return finish_call(c, s, e);
    shared->arena = arena;
    shared->base.clear();
    for (size_t j = 0; j < m; j++) {
      memcpy(&H.commit[32 * plan.need[j]], &out[32 * j], 32);
      H.commit_ok[plan.need[j]] = ok[j];
      if (arena->base[j] != (size_t)-1) shared->base.emplace(b.blocks[plan.need[j]].last_commit, arena->base[j]);
    }
  }
  // Data.Hash of every block (block_off == NULL: none has transactions)
  if (b.block_off) {
    const int rc = txs_hashes_held(c, b.txs, b.tx_off, b.block_off, n, H.data.data(), tab + 32 * r_data);
    if (rc != TMED_OK) return rc;
  } else {
    for (size_t i = 0; i < n; i++) memcpy(&H.data[32 * i], V::kEmptyHash, 32);
  }
  // EvidenceList.Hash of every block's list (list_off == NULL: none has evidence)
  if (b.list_off) {
    const int rc = evidence_hashes_body(c, b.ev, b.items, b.list_off, n, b.opaque, b.opaque_off, nullptr, H.evidence.data(),
                                        nullptr, H.evidence_ok.data(), /*held=*/true, tab + 32 * r_ev);
    if (rc != TMED_OK) return rc;
  } else {
    for (size_t i = 0; i < n; i++) {
      memcpy(&H.evidence[32 * i], V::kEmptyHash, 32);
      H.evidence_ok[i] = 1;
    }
  }
  // Header.Hash of the blocks linked requests read
  std::vector<uint32_t> hdr_row(n, 0);
  if (k) {
    std::vector<const tmed_header *> hs(k);
    for (size_t j = 0; j < k; j++) hs[j] = b.blocks[plan.need_hdr[j]].header;
    std::vector<uint8_t> out(32 * k), ok(k);
    std::vector<uint32_t> row_of(k);
    const int rc = header_hashes_locked(c, hs.data(), k, out.data(), ok.data(), tab + 32 * r_hdr, row_of.data());
    if (rc != TMED_OK) return rc;
    for (size_t j = 0; j < k; j++) {
      memcpy(&H.header[32 * plan.need_hdr[j]], &out[32 * j], 32);
      H.header_ok[plan.need_hdr[j]] = ok[j];
      hdr_row[plan.need_hdr[j]] = (uint32_t)r_hdr + row_of[j];
    }
  }
  // ValidatorSet.Hash of each distinct known set, once
  if (!hsets.empty()) {
    std::vector<uint8_t> out(32 * hsets.size());
    const int rc = valsets_hashes_locked(c, hsets.data(), hsets.size(), out.data(), tab + 32 * r_set);
    if (rc != TMED_OK) return rc;
    c->vb_stats[0] = hsets.size();
    for (const size_t i : plan.need) {
      const tmed_block_request &r = b.blocks[i];
      if (V::knows(r, TMED_VB_KNOW_VALIDATORS)) memcpy(&H.vals[32 * i], &out[32 * set_of[r.state->validators]], 32);
      if (V::knows(r, TMED_VB_KNOW_NEXT_VALIDATORS)) memcpy(&H.next[32 * i], &out[32 * set_of[r.state->next_validators]], 32);
    }
  }
  V::fill_enable(plan, H);
  // block_check_kernel over the plan's requests: records and each distinct set's addresses in, one
  // (mask, proposer) pair a block out
  SetTable sets;
  for (const size_t i : plan.need)
    if (H.enable[i] & V::kCmpLookup) sets.add(b.blocks[i].state->validators);
  const size_t nv = sets.n_vals;
  if (m > 0x7fffffffu || nv > 0x7fffffffu) return TMED_EINVAL;
  const size_t o_rec = 0, o_addr = align256(o_rec + m * sizeof(BlockCheckRec)), o_out = align256(o_addr + 20 * nv),
               total = align256(o_out + 8 * m);
  e = c->stage.ensure(total, total);
  if (e != hipSuccess) return map_err(e);
  uint8_t *h = c->stage.host(), *d = c->stage.dev();
  BlockCheckRec *recs = reinterpret_cast<BlockCheckRec *>(h + o_rec);
  std::vector<uint32_t> host_mask(m, 0);
  for (size_t j = 0; j < m; j++) {
    const size_t i = plan.need[j];
    const tmed_block_request &r = b.blocks[i];
    BlockCheckRec &rec = recs[j];
    memset(&rec, 0, sizeof(rec));
    rec.enable = H.enable[i];
    // a slot whose computed value the table does not hold (no transactions or no evidence in the whole
    // call: the empty hash, a host constant) is compared here and leaves the kernel's enable word
    const uint32_t rows[6] = {(uint32_t)(r_commit + j), (uint32_t)(r_data + i), (uint32_t)(r_ev + i),
                              V::knows(r, TMED_VB_KNOW_VALIDATORS) ? (uint32_t)(r_set + set_of[r.state->validators]) : 0u,
                              V::knows(r, TMED_VB_KNOW_NEXT_VALIDATORS) ? (uint32_t)(r_set + set_of[r.state->next_validators]) : 0u,
                              hdr_row[V::linked(r) ? i - 1 : i]};
    for (int q = 0; q < V::kCompares; q++) {
      if (!(rec.enable >> q & 1)) continue;
      uint32_t len;
      const uint8_t *want = V::want_of(*r.header, q, &len);
      if ((q == 1 && !b.block_off) || (q == 2 && !b.list_off)) {
        if (memcmp(want, V::kEmptyHash, 32) != 0) host_mask[j] |= 1u << q;
        rec.enable &= ~(1u << q);
        continue;
      }
      memcpy(rec.want + 8 * q, want, 32);
      rec.row[q] = rows[q];
    }
    if (rec.enable & V::kCmpLookup) {
      const tmed_valset *vs = r.state->validators;
      memcpy(rec.addr, r.header->hashes[V::kHProposer], 20);
      rec.n_vals = (uint32_t)vs->n;
      rec.set_base = sets.at(vs);
    }
  }
  for (const tmed_valset *vs : sets.sets)
    if (vs->n) memcpy(h + o_addr + 20 * sets.at(vs), vs->addresses, 20 * vs->n);
  e = hipMemcpyAsync(d, h, o_out, hipMemcpyHostToDevice, s);  // one copy in
  if (e == hipSuccess) e = hipEventRecord(c->ev0, s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(block_check_kernel, dim3((uint32_t)((m + kCheckWaves - 1) / kCheckWaves)), dim3(64 * kCheckWaves), 0, s,
                       reinterpret_cast<const BlockCheckRec *>(d + o_rec), (uint32_t)m,
                       reinterpret_cast<const uint32_t *>(tab), (uint32_t)n_rows,
                       reinterpret_cast<const uint32_t *>(d + o_addr), reinterpret_cast<uint2 *>(d + o_out));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(c->ev1, s);
  if (e == hipSuccess) e = hipMemcpyAsync(h + o_out, d + o_out, 8 * m, hipMemcpyDeviceToHost, s);
  const int rc = finish_call(c, s, e, &c->last_vb_ms);
  if (rc != TMED_OK) return rc;
  const uint32_t *res = reinterpret_cast<const uint32_t *>(h + o_out);
  for (size_t j = 0; j < m; j++) {
    H.mask[plan.need[j]] = res[2 * j] | host_mask[j];
    H.proposer[plan.need[j]] = (int32_t)res[2 * j + 1];  // kEvNone is -1
  }
  H.have_proposer = true;
  c->vb_stats[1] = sets.sets.size();
  c->vb_stats[2] = m;
  return TMED_OK;
}

}  // namespace tmed

extern "C" {

float tmed_validate_kernel_ms(tmed_ctx *c) { return c ? c->last_vb_ms : 0.f; }

int tmed_validate_stats(tmed_ctx *c, uint64_t out[3]) {
  if (!c || !out) return TMED_EINVAL;
  for (int k = 0; k < 3; k++) out[k] = c->vb_stats[k];
  return TMED_OK;
}

}  // extern "C"
