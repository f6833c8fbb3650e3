// lca.hip — LightClientAttackEvidence on gfx950: GetByzantineValidators (types/evidence.go:233-279)
// without a host map and without a host sort, and LightClientAttackEvidence.Hash() (:302-309).
// include/tmed25519.h states the calls (tmed_byzantine_validators, tmed_verify_light_client_attacks);
// lca_free.h holds the rule, shared with the host; lca_host.h the replay of VerifyLightClientAttack,
// whose device tail is lca_tail_locked below (commit.hip holds the entry point beside light.Verify's).
//
// The host plans each request's candidates (the signatures whose address is looked up: lca_host.h
// plan_candidates) and numbers them flat over the call, with a per-request offset table (LcaStep), so
// requests of any size mix in one launch.
//
// lca_lookup_kernel: GetByAddress, one wavefront per candidate, by the scan of evidence_lookup_kernel
// (addr_scan.h wave_first_address).  Lane 0 then writes the candidate's ordering key (lca_free.h: eight
// dwords from the found validator's power and address) and the found index.
//
// lca_rank_kernel: nothing is sorted.  One lane per candidate counts the candidates of its request that
// order before it; the ranks are a permutation (ties by commit position), so the lane writes its
// validator index at its rank with no atomic and every entry of the request's range is written by
// exactly one lane (a call leaves nothing of an earlier one behind).  A workgroup of kLcaTile = 128
// lanes serves 128 candidates of ONE request (the host's block table names the request and the first
// candidate) and walks all of that request's keys in tiles of 128 staged in LDS (4 KB: 128 x 32 B);
// every lane reads the same tile entry at the same time, which the LDS broadcasts, as two 16-byte
// reads.  O(m^2) compares per request: at m = 10,000 that is 79 workgroups x 79 tiles.
//
// The lookup and the rank are TWO kernels for the reason evidence.hip gives: the lookup wants a
// wavefront per candidate, the rank a lane per candidate.
//
// lca_hash_kernel: Hash(), one lane per request: one SHA-256 block (lca_free.h lca_evidence_hash).
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "../../include/tmed25519.h"
#include "addr_scan.h"
#include "call_frame.h"
#include "lca_host.h"
#include "slot_batch.h"

namespace tmed {

constexpr uint32_t kLcaTile = 128;

// One request's side: where its set starts in the call's packed address and power arrays, its size,
// and where its candidates start in the call's flat candidate arrays.
struct LcaStep {
  uint64_t addr_base;
  uint32_t n_vals, cand_off, n_cand, pad;
};
static_assert(sizeof(LcaStep) == 24, "LcaStep layout");
// One candidate: its address as five dwords, then its request (bit 31: the address's length is not
// 20, it matches nobody).
constexpr uint32_t kLcaCandDw = 6;
// One workgroup of the rank kernel: the request and the first of its 128 candidates there.
struct LcaBlock {
  uint32_t req, first;
};
// One Hash(): the conflicting header's hash (ok = 0: nil) and CommonHeight.
struct LcaHashIn {
  uint32_t hdr[8];
  int64_t common_height;
  uint32_t ok, pad;
};
static_assert(sizeof(LcaHashIn) == 48, "LcaHashIn layout");

// Device pointers of one call.
struct LcaDev {
  const LcaStep *steps;
  const uint32_t *cands;    // m x kLcaCandDw
  const LcaBlock *blocks;
  const uint8_t *set_addr;  // the requests' sets, packed: 20 B a validator
  const int64_t *set_pow;   //   8 B a validator
  uint4 *keys;              // m x 2: the ordering keys
  uint32_t *found;          // m: the found validator's index, kEvNone for nobody
  int32_t *ranked;          // m: request r's found indices in order at [cand_off, cand_off + n_cand), -1 behind them
};

__global__ __launch_bounds__(kScanLanes) void lca_lookup_kernel(LcaDev p, uint32_t m) {
  const uint32_t k = blockIdx.x, lane = threadIdx.x;
  if (k >= m) return;
  const uint32_t *cd = p.cands + (size_t)kLcaCandDw * k;
  const uint32_t meta = cd[5];
  const LcaStep &s = p.steps[meta & 0x7fffffffu];
  const uint32_t *set = reinterpret_cast<const uint32_t *>(p.set_addr) + 5 * s.addr_base;
  uint32_t found = kEvNone;
  if (!(meta >> 31)) {
    uint32_t want[5];
#pragma unroll
    for (int q = 0; q < 5; q++) want[q] = cd[q];
    found = wave_first_address(want, set, s.n_vals, lane);
  }
  if (lane == 0) {
    const bool has = found != kEvNone;
    uint32_t addr[5] = {0, 0, 0, 0, 0}, w[kLcaKeyDw];
    if (has) {
#pragma unroll
      for (int q = 0; q < 5; q++) addr[q] = set[5 * (size_t)found + q];
    }
    lca_key(has, has ? p.set_pow[s.addr_base + found] : 0, addr, w);
    p.keys[2 * (size_t)k] = make_uint4(w[0], w[1], w[2], w[3]);
    p.keys[2 * (size_t)k + 1] = make_uint4(w[4], w[5], w[6], w[7]);
    p.found[k] = found;
  }
}

__global__ __launch_bounds__(kLcaTile) void lca_rank_kernel(LcaDev p, uint32_t n_blocks) {
  __shared__ uint4 tile[kLcaTile][2];
  const uint32_t t = threadIdx.x;
  if (blockIdx.x >= n_blocks) return;  // the whole workgroup
  const LcaBlock blk = p.blocks[blockIdx.x];
  const LcaStep s = p.steps[blk.req];
  const uint4 *keys = p.keys + 2 * (size_t)s.cand_off;
  const uint32_t me = blk.first + t;
  const bool live = me < s.n_cand;
  uint32_t mine[kLcaKeyDw] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (live) {
    const uint4 a = keys[2 * (size_t)me], b = keys[2 * (size_t)me + 1];
    mine[0] = a.x, mine[1] = a.y, mine[2] = a.z, mine[3] = a.w, mine[4] = b.x, mine[5] = b.y, mine[6] = b.z, mine[7] = b.w;
  }
  uint32_t rank = 0;
  for (uint32_t base = 0; base < s.n_cand; base += kLcaTile) {  // uniform over the workgroup: s is its request's
    __syncthreads();  // the tile before this one has been read
    const uint32_t j = base + t;
    if (j < s.n_cand) {
      tile[t][0] = keys[2 * (size_t)j];
      tile[t][1] = keys[2 * (size_t)j + 1];
    }
    __syncthreads();
    const uint32_t lim = s.n_cand - base < kLcaTile ? s.n_cand - base : kLcaTile;
    if (live) {
      for (uint32_t q = 0; q < lim; q++) {
        const uint4 a = tile[q][0], b = tile[q][1];
        const uint32_t other[kLcaKeyDw] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        rank += lca_before(other, base + q, mine, me) ? 1u : 0u;
      }
    }
  }
  // rank < n_cand: it counts candidates of the request other than this one
  if (live) p.ranked[s.cand_off + rank] = (int32_t)p.found[s.cand_off + me];  // kEvNone is -1
}

__global__ __launch_bounds__(64) void lca_hash_kernel(const LcaHashIn *__restrict__ in, uint32_t n, uint32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 *src = reinterpret_cast<const uint4 *>(in + i);
  const uint4 a = src[0], b = src[1], c = src[2];
  const uint32_t hdr[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t st[8];
  lca_evidence_hash(hdr, c.z != 0, (int64_t)(((uint64_t)c.y << 32) | c.x), st);
  uint4 *o = reinterpret_cast<uint4 *>(out + 8 * (size_t)i);
  o[0] = make_uint4(lca_bswap(st[0]), lca_bswap(st[1]), lca_bswap(st[2]), lca_bswap(st[3]));
  o[1] = make_uint4(lca_bswap(st[4]), lca_bswap(st[5]), lca_bswap(st[6]), lca_bswap(st[7]));
}

int lca_tail_locked(tmed_ctx *c, const tmed_lca_request *reqs, const std::vector<size_t> &live, const uint8_t *ch,
                    const uint8_t *cok, const std::vector<size_t> &need, const int *kinds, int32_t *byz,
                    const uint64_t *byz_off, tmed_byz_result *bres, uint8_t *ev_hash) {
  namespace LH = tmed_lca;
  c->last_ms = 0.f;
  c->last_lca_ms[0] = c->last_lca_ms[1] = 0.f;
  // the plan: each request's candidates, the distinct sets they are looked up in, the rank workgroups
  const size_t G = need.size(), H = live.size();
  std::vector<std::vector<uint32_t>> pos(G);
  std::vector<uint8_t> panicked(G, 0);
  std::vector<LcaStep> steps(G);
  std::vector<LcaBlock> blocks;
  SetTable sets;
  size_t m = 0;
  for (size_t j = 0; j < G; j++) {
    const tmed_lca_request &r = reqs[need[j]];
    panicked[j] = !LH::plan_candidates(r, kinds[need[j]], pos[j]);
    if (panicked[j]) pos[j].clear();
    if (!pos[j].empty()) sets.add(LH::lookup_set(r, kinds[need[j]]));
    if (m + pos[j].size() > 0x7fffffffu) return TMED_EINVAL;
    steps[j] = LcaStep{0, 0, (uint32_t)m, (uint32_t)pos[j].size(), 0};
    for (size_t f = 0; f < pos[j].size(); f += kLcaTile) blocks.push_back(LcaBlock{(uint32_t)j, (uint32_t)f});
    m += pos[j].size();
  }
  const size_t B = blocks.size(), nv = sets.n_vals;
  if (nv > 0x7fffffffu) return TMED_EINVAL;
  const size_t o_step = 0, o_cand = align256(o_step + G * sizeof(LcaStep)), o_blk = align256(o_cand + m * kLcaCandDw * 4),
               o_addr = align256(o_blk + B * sizeof(LcaBlock)), o_pow = align256(o_addr + 20 * nv),
               o_hin = align256(o_pow + 8 * nv), o_rank = align256(o_hin + H * sizeof(LcaHashIn)),
               o_hout = align256(o_rank + 4 * m), o_key = align256(o_hout + 32 * H), o_found = align256(o_key + 32 * m),
               total = align256(o_found + 4 * m);
  if (m + H) {
    (void)hipSetDevice(c->device);
    hipStream_t s = c->stream;
    hipError_t e = c->stage.ensure(o_key, total);  // the keys and the found indices stay on the device
    if (e == hipSuccess && !c->ev_lookup) e = hipEventCreate(&c->ev_lookup);
    if (e != hipSuccess) return map_err(e);
    uint8_t *h = c->stage.host(), *d = c->stage.dev();
    for (size_t j = 0; j < G; j++) {
      const tmed_lca_request &r = reqs[need[j]];
      if (pos[j].empty()) continue;
      const tmed_valset *vs = LH::lookup_set(r, kinds[need[j]]);
      steps[j].addr_base = sets.at(vs);
      steps[j].n_vals = (uint32_t)vs->n;
      const tmed_commit &cm = *r.conflicting_commit;
      uint32_t *cd = reinterpret_cast<uint32_t *>(h + o_cand) + (size_t)kLcaCandDw * steps[j].cand_off;
      for (size_t k = 0; k < pos[j].size(); k++, cd += kLcaCandDw) {
        memcpy(cd, cm.addresses + 20 * (size_t)pos[j][k], 20);
        cd[5] = (uint32_t)j | (LH::cand_len_ok(cm, pos[j][k]) ? 0u : 0x80000000u);
      }
    }
    if (G) memcpy(h + o_step, steps.data(), G * sizeof(LcaStep));
    if (B) memcpy(h + o_blk, blocks.data(), B * sizeof(LcaBlock));
    for (const tmed_valset *vs : sets.sets) {
      if (!vs->n) continue;
      const uint64_t b = sets.at(vs);
      memcpy(h + o_addr + 20 * b, vs->addresses, 20 * vs->n);
      memcpy(h + o_pow + 8 * b, vs->powers, 8 * vs->n);
    }
    LcaHashIn *hin = reinterpret_cast<LcaHashIn *>(h + o_hin);
    for (size_t q = 0; q < H; q++) {
      const size_t i = live[q];
      memset(&hin[q], 0, sizeof(LcaHashIn));
      if (cok[i]) memcpy(hin[q].hdr, ch + 32 * i, 32);
      hin[q].common_height = reqs[i].common_height;
      hin[q].ok = cok[i] ? 1u : 0u;
    }
    const LcaDev p{reinterpret_cast<const LcaStep *>(d + o_step), reinterpret_cast<const uint32_t *>(d + o_cand),
                   reinterpret_cast<const LcaBlock *>(d + o_blk), d + o_addr, reinterpret_cast<const int64_t *>(d + o_pow),
                   reinterpret_cast<uint4 *>(d + o_key), reinterpret_cast<uint32_t *>(d + o_found),
                   reinterpret_cast<int32_t *>(d + o_rank)};
    e = hipMemcpyAsync(d, h, o_rank, hipMemcpyHostToDevice, s);  // one copy in
    if (e == hipSuccess) e = hipEventRecord(c->ev0, s);
    if (e == hipSuccess && m) {
      hipLaunchKernelGGL(lca_lookup_kernel, dim3((uint32_t)m), dim3(kScanLanes), 0, s, p, (uint32_t)m);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(c->ev_lookup, s);
    if (e == hipSuccess && B) {
      hipLaunchKernelGGL(lca_rank_kernel, dim3((uint32_t)B), dim3(kLcaTile), 0, s, p, (uint32_t)B);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(c->ev1, s);
    if (e == hipSuccess && H) {
      hipLaunchKernelGGL(lca_hash_kernel, dim3((uint32_t)((H + 63) / 64)), dim3(64), 0, s,
                         reinterpret_cast<const LcaHashIn *>(d + o_hin), (uint32_t)H, reinterpret_cast<uint32_t *>(d + o_hout));
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h + o_rank, d + o_rank, o_key - o_rank, hipMemcpyDeviceToHost, s);
    const int rc = finish_call(c, s, e, &c->last_ms);
    if (rc != TMED_OK) return rc;
    (void)hipEventElapsedTime(&c->last_lca_ms[0], c->ev0, c->ev_lookup);
    (void)hipEventElapsedTime(&c->last_lca_ms[1], c->ev_lookup, c->ev1);
    for (size_t q = 0; q < H; q++) memcpy(ev_hash + 32 * live[q], h + o_hout + 32 * q, 32);
  }
  const int32_t *ranked = m ? reinterpret_cast<const int32_t *>(c->stage.host() + o_rank) : nullptr;
  for (size_t j = 0; j < G; j++) {
    const size_t i = need[j];
    if (panicked[j]) {
      bres[i] = tmed_byz_result{kinds[i], TMED_BYZ_PANIC, 0};
      continue;
    }
    LH::finish_list(kinds[i], ranked ? ranked + steps[j].cand_off : nullptr, pos[j].size(), byz + byz_off[i], bres[i]);
  }
  return TMED_OK;
}

}  // namespace tmed

extern "C" {

int tmed_lca_kernel_times(tmed_ctx *c, float ms[2]) {
  if (!c || !ms) return TMED_EINVAL;
  ms[0] = c->last_lca_ms[0];
  ms[1] = c->last_lca_ms[1];
  return TMED_OK;
}

int tmed_byzantine_validators(tmed_ctx *c, const tmed_lca_request *reqs, size_t n, int32_t *byz, const uint64_t *byz_off,
                              tmed_byz_result *out) {
  using namespace tmed;
  if (!c) return TMED_EINVAL;
  return guarded([&] {
    const int rc = tmed_lca::check_lca_call(reqs, n, byz, byz_off, out);
    if (rc != TMED_OK || n == 0) return rc;
    std::vector<size_t> need(n);
    std::vector<int> kinds(n);
    for (size_t i = 0; i < n; i++) {
      need[i] = i;
      kinds[i] = lca_kind(reqs[i]);
    }
    return locked(c, /*collect=*/true, [&] {
      return lca_tail_locked(c, reqs, {}, nullptr, nullptr, need, kinds.data(), byz, byz_off, out, nullptr);
    });
  });
}

}  // extern "C"
