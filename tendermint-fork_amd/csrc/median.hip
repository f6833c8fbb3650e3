// median.hip — state.MedianTime (state/state.go:268-285) for many (commit, validator set) pairs per
// call on gfx950: the device half of tmed_median_times (include/tmed25519.h states the rule;
// median_host.h is the same rule on the host and the route of every pair the kernels do not take).
//
// The reference looks every non-absent signature's address up in the set (a linear scan), sorts
// the weighted times by UnixNano and walks them until half the total power is passed
// (types/time/time.go:35-58).  For non-negative weights that walk returns the smallest entering key
// t with W(<= t) >= median, W(<= t) = the entering weight with key <= t, so nothing
// is sorted here:
//   pass 1  each lane loads its elements (a few per lane, kept in registers): the flag, the 20-byte
//           address compare against the set's address at the same index (the fast-path test: any
//           mismatch ends the pair with kMedMisaligned and the library computes it on the host),
//           the key seconds * 1e9 + nanos with its range checks, the power; one reduction gives the
//           total (int64, overflow detected), the entering count, the status bits, and the smallest
//           and largest key;
//   search  median == 0: the smallest key.  Otherwise the bits of the sign-biased key from the
//           highest bit in which the smallest and the largest key differ down to bit 0: one
//           weighted count W(<= candidate) per bit, int64 and exact, reduced across the group.
// Two shapes of one kernel template, chosen by n_sigs (median_times_locked):
//   wave    one wavefront per commit, kMedWaveGroups commits per 256-lane workgroup, kMedWavePerLane
//           elements per lane: n_sigs <= kMedWaveMax = 512 (C3's 175 validators: 3 per lane).  No LDS
//           and no barrier: every reduction is an xor butterfly of __shfl_xor across the 64 lanes;
//   block   one workgroup of kMedBlockWaves = 16 wavefronts per commit, kMedBlockPerLane elements per
//           lane: C4's 10,000 signatures sit in registers (capacity kMedBlockCap = 12,288); a longer
//           commit's elements past the capacity are re-read through a strided loop at every step.
//           Reductions: the butterfly inside each wavefront, then 16 partials through LDS (two
//           buffers of 16 x 8 B, one barrier per reduction), summed by a 16-lane butterfly.
// Neither shape stages anything else through LDS; no floating point anywhere.
#include <hip/hip_runtime.h>
#include <string.h>

#include <unordered_map>
#include <vector>

#include "../../include/tmed25519.h"
#include "call_frame.h"
#include "host_for.h"
#include "median_host.h"

namespace tmed {

constexpr uint32_t kMedWaveGroups = 4;     // commits per workgroup of the wave shape
constexpr uint32_t kMedWavePerLane = 8;    // elements a lane of the wave shape holds
constexpr uint32_t kMedWaveMax = 512;      // = 64 * kMedWavePerLane: larger commits take the block shape
constexpr uint32_t kMedBlockWaves = 16;    // wavefronts per commit of the block shape
constexpr uint32_t kMedBlockPerLane = 12;  // elements a lane of the block shape holds
constexpr uint32_t kMedBlockCap = 12288;   // = 64 * kMedBlockWaves * kMedBlockPerLane: past it, the strided loop
constexpr size_t kMedMaxSigs = (size_t)1 << 24;  // longer commits are computed on the host
static_assert(kMedWaveMax == 64 * kMedWavePerLane && kMedBlockCap == 64 * kMedBlockWaves * kMedBlockPerLane, "shape");

// One staged pair: its commit's and its set's first element in the packed arrays.
struct MedPair {
  uint64_t cbase, sbase;
  uint32_t n, pad;
};
// status: TMED_MEDIAN_OK / _ZERO_TIME / _GO_PATH, or kMedMisaligned (not a fast-path pair)
constexpr uint32_t kMedMisaligned = 3;
struct MedOut {
  int64_t key;  // OK: the median's UnixNano
  uint32_t entered, status;
};

// element status bits
constexpr uint32_t kElEntered = 1, kElGoPath = 2, kElMisaligned = 4;
constexpr uint64_t kKeyBias = 1ull << 63;  // int64 order as uint64 order

struct MedArrays {
  const uint8_t *flags, *caddr;
  const int64_t *sec;
  const int32_t *nanos;
  const uint8_t *saddr;
  const int64_t *power;
};

// Element i of pair p: its biased key and weight when it enters (else ~0 and 0, which no weighted
// count sees), and its status bits.
__device__ __forceinline__ uint32_t med_load(const MedArrays &a, const MedPair &p, uint32_t i, uint64_t &key, int64_t &w) {
  key = ~0ull;
  w = 0;
  const uint64_t ci = p.cbase + i, si = p.sbase + i;
  if (a.flags[ci] == 1) return 0;
  const uint32_t *x = reinterpret_cast<const uint32_t *>(a.caddr + 20 * ci);
  const uint32_t *y = reinterpret_cast<const uint32_t *>(a.saddr + 20 * si);
  uint32_t diff = 0;
#pragma unroll
  for (int k = 0; k < 5; k++) diff |= x[k] ^ y[k];
  if (diff) return kElMisaligned;
  int64_t k64;
  const int64_t pw = a.power[si];
  if (!tmed_median::unix_nano(a.sec[ci], a.nanos[ci], &k64) || pw < 0) return kElGoPath;
  key = (uint64_t)k64 ^ kKeyBias;
  w = pw;
  return kElEntered;
}

// ---- reductions: every lane of the group receives the result -------------------------------------
struct OpMin {
  __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a < b ? a : b; }
};
struct OpMax {
  __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a > b ? a : b; }
};
struct OpAdd {
  __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; }
};
struct OpOr {
  __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a | b; }
};
// sums of values in [0, 2^63): bit 63 set = the sum passed int64 (it stays set)
struct OpAddSat {
  __device__ uint64_t operator()(uint64_t a, uint64_t b) const {
    const uint64_t s = (a & ~kKeyBias) + (b & ~kKeyBias);
    return s | ((a | b) & kKeyBias);
  }
};

template <uint32_t kWaves>
struct Group {
  unsigned long long (*red)[kWaves];  // LDS: two buffers of kWaves partials (kWaves > 1)
  uint32_t turn;
  template <class Op>
  __device__ __forceinline__ uint64_t all(uint64_t v, Op op) {
#pragma unroll
    for (int s = 32; s; s >>= 1) v = op(v, (uint64_t)__shfl_xor((unsigned long long)v, s));
    if constexpr (kWaves > 1) {
      // A buffer is rewritten two reductions later: every wavefront has passed the barrier between,
      // which it reaches only after reading this one.
      unsigned long long *buf = red[turn & 1];
      turn++;
      if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
      __syncthreads();
      v = buf[threadIdx.x & (kWaves - 1)];
#pragma unroll
      for (int s = kWaves / 2; s; s >>= 1) v = op(v, (uint64_t)__shfl_xor((unsigned long long)v, s));
    }
    return v;
  }
};

template <uint32_t kWaves, uint32_t kPerLane>
__global__ __launch_bounds__(kWaves == 1 ? 64 * kMedWaveGroups : 64 * kWaves) void median_kernel(
    const MedPair *pairs, uint32_t m, MedArrays a, MedOut *out) {
  constexpr uint32_t T = 64 * kWaves;  // lanes per commit
  __shared__ unsigned long long red[kWaves > 1 ? 2 : 1][kWaves];
  Group<kWaves> grp{red, 0};
  uint32_t g, tid;
  if constexpr (kWaves == 1) {
    g = blockIdx.x * kMedWaveGroups + (threadIdx.x >> 6);
    tid = threadIdx.x & 63;
    if (g >= m) return;  // a whole wavefront; this shape has no barrier
  } else {
    g = blockIdx.x;
    tid = threadIdx.x;
  }
  const MedPair p = pairs[g];

  // pass 1: load, classify, total
  uint64_t key[kPerLane];
  int64_t w[kPerLane];
  uint32_t st = 0, cnt = 0;
  uint64_t tot = 0, mn = ~0ull, mx = 0;
  auto account = [&](uint32_t s, uint64_t k, int64_t wt) {
    st |= s;
    if (s & kElEntered) {
      cnt++;
      tot = OpAddSat()(tot, (uint64_t)wt);
      mn = k < mn ? k : mn;
      mx = k > mx ? k : mx;
    }
  };
#pragma unroll
  for (uint32_t e = 0; e < kPerLane; e++) {
    const uint32_t i = tid + e * T;
    key[e] = ~0ull;
    w[e] = 0;
    if (i < p.n) account(med_load(a, p, i, key[e], w[e]), key[e], w[e]);
  }
  for (uint64_t i = (uint64_t)kPerLane * T + tid; i < p.n; i += T) {  // past the registers' capacity
    uint64_t k;
    int64_t wt;
    const uint32_t s = med_load(a, p, (uint32_t)i, k, wt);
    account(s, k, wt);
  }
  st = (uint32_t)grp.all(st, OpOr());
  tot = grp.all(tot, OpAddSat());
  cnt = (uint32_t)grp.all(cnt, OpAdd());

  MedOut o{0, 0, TMED_MEDIAN_OK};
  if (st & kElMisaligned) {
    o.status = kMedMisaligned;
  } else if ((st & kElGoPath) || (tot & kKeyBias)) {
    o.status = TMED_MEDIAN_GO_PATH;
  } else if (cnt == 0) {
    o.status = TMED_MEDIAN_ZERO_TIME;
  } else {  // every branch above and below is uniform across the group: st, tot, cnt are reduced values
    o.entered = cnt;
    mn = grp.all(mn, OpMin());
    const uint64_t median = tot >> 1;  // total / 2, total >= 0
    uint64_t ans = mn;                 // median == 0: the smallest entering key
    if (median != 0) {
      mx = grp.all(mx, OpMax());
      // the answer lies in [mn, mx]: the bits above their highest differing bit are settled
      const uint64_t d = mn ^ mx;
      const int nbits = d ? 64 - __clzll((long long)d) : 0;
      ans = nbits == 64 ? 0 : (mn >> nbits) << nbits;
      for (int b = nbits - 1; b >= 0; b--) {
        const uint64_t cand = ans | ((1ull << b) - 1);  // bit b clear, every lower bit set
        uint64_t acc = 0;
#pragma unroll
        for (uint32_t e = 0; e < kPerLane; e++) acc += key[e] <= cand ? (uint64_t)w[e] : 0;
        for (uint64_t i = (uint64_t)kPerLane * T + tid; i < p.n; i += T) {
          uint64_t k;
          int64_t wt;
          (void)med_load(a, p, (uint32_t)i, k, wt);
          acc += k <= cand ? (uint64_t)wt : 0;
        }
        if (grp.all(acc, OpAdd()) < median) ans |= 1ull << b;  // W(<= cand) < median: the key has bit b
      }
    }
    o.key = (int64_t)(ans ^ kKeyBias);
  }
  if (tid == 0) out[g] = o;
}

// ---- staging ---------------------------------------------------------------------------------------
// The call's regions for P pairs, Nc commit elements and Ns set elements; [0, out) is copied in.
struct MedLayout {
  size_t pairs, sec, power, nanos, caddr, saddr, flags, out, total;
  MedLayout(size_t P, size_t Nc, size_t Ns) {
    pairs = 0;
    sec = align256(pairs + sizeof(MedPair) * P);
    power = align256(sec + 8 * Nc);
    nanos = align256(power + 8 * Ns);
    caddr = align256(nanos + 4 * Nc);
    saddr = align256(caddr + 20 * Nc);
    flags = align256(saddr + 20 * Ns);
    out = align256(flags + Nc);
    total = out + sizeof(MedOut) * P;
  }
};

// A fast-path candidate by what the host sees without reading an address: equal sizes, within the
// kernels' range, and no non-absent signature whose address length is not 20 (the kernels compare
// 20-byte slots).
static bool med_candidate(const tmed_commit &cm, const tmed_valset &vs) {
  if (cm.n_sigs != vs.n || cm.n_sigs > kMedMaxSigs) return false;
  if (cm.address_lens)
    for (size_t i = 0; i < cm.n_sigs; i++)
      if (cm.flags[i] != 1 && cm.address_lens[i] != 20) return false;
  return true;
}

int median_times_locked(tmed_ctx *c, const tmed_median_request *reqs, size_t n, tmed_median_result *out,
                        const MedShared *shared) {
  if (shared)  // every commit of the call must lie in the arena, else the call stages as usual
    for (size_t i = 0; i < n && shared; i++)
      if (!shared->base.count(reqs[i].commit)) shared = nullptr;
  std::vector<size_t> dev, big, host;  // request indexes: wave shape (then the block shape appended) / host route
  for (size_t i = 0; i < n; i++) {
    const tmed_commit &cm = *reqs[i].commit;
    (!med_candidate(cm, *reqs[i].vals) ? host : cm.n_sigs <= kMedWaveMax ? dev : big).push_back(i);
  }
  const size_t n_wave = dev.size(), n_block = big.size(), P = n_wave + n_block;
  dev.insert(dev.end(), big.begin(), big.end());
  tmed_median::SetIndexes sets;
  c->last_ms = 0.f;
  if (P) {
    if (P > 0x7fffffffu) return TMED_EINVAL;
    // each distinct commit and each distinct set of the device pairs is staged once
    std::unordered_map<const tmed_commit *, size_t> cbase;
    std::unordered_map<const tmed_valset *, size_t> sbase;
    std::vector<const tmed_commit *> commits;
    std::vector<const tmed_valset *> vsets;
    std::vector<size_t> coff, soff;
    size_t Nc = 0, Ns = 0;
    for (const size_t i : dev) {
      if (shared) {
        cbase.emplace(reqs[i].commit, shared->base.find(reqs[i].commit)->second);
      } else if (cbase.emplace(reqs[i].commit, Nc).second) {
        commits.push_back(reqs[i].commit);
        coff.push_back(Nc);
        Nc += reqs[i].commit->n_sigs;
      }
      if (sbase.emplace(reqs[i].vals, Ns).second) {
        vsets.push_back(reqs[i].vals);
        soff.push_back(Ns);
        Ns += reqs[i].vals->n;
      }
    }
    const MedLayout lay(P, Nc, Ns);
    (void)hipSetDevice(c->device);
    hipStream_t s = c->stream;
    hipError_t e = c->stage.ensure(lay.total, lay.total);
    if (e != hipSuccess) return map_err(e);
    uint8_t *h = c->stage.host(), *d = c->stage.dev();
    MedPair *hp = reinterpret_cast<MedPair *>(h + lay.pairs);
    for (size_t j = 0; j < P; j++)
      hp[j] = MedPair{cbase[reqs[dev[j]].commit], sbase[reqs[dev[j]].vals], (uint32_t)reqs[dev[j]].commit->n_sigs, 0};
    host_for(commits.size(), pack_threads(Nc), [&](size_t k) {
      const tmed_commit &cm = *commits[k];
      const size_t b = coff[k], m = cm.n_sigs;
      if (!m) return;
      memcpy(h + lay.sec + 8 * b, cm.ts_seconds, 8 * m);
      memcpy(h + lay.nanos + 4 * b, cm.ts_nanos, 4 * m);
      memcpy(h + lay.caddr + 20 * b, cm.addresses, 20 * m);
      memcpy(h + lay.flags + b, cm.flags, m);
    });
    host_for(vsets.size(), pack_threads(Ns), [&](size_t k) {
      const tmed_valset &vs = *vsets[k];
      if (!vs.n) return;
      memcpy(h + lay.power + 8 * soff[k], vs.powers, 8 * vs.n);
      memcpy(h + lay.saddr + 20 * soff[k], vs.addresses, 20 * vs.n);
    });
    const MedArrays arr = shared ? MedArrays{shared->arena->flags, shared->arena->addr, shared->arena->sec,
                                             shared->arena->nanos, d + lay.saddr, (const int64_t *)(d + lay.power)}
                                 : MedArrays{d + lay.flags, d + lay.caddr, (const int64_t *)(d + lay.sec),
                                             (const int32_t *)(d + lay.nanos), d + lay.saddr, (const int64_t *)(d + lay.power)};
    const MedPair *dp = reinterpret_cast<const MedPair *>(d + lay.pairs);
    MedOut *dout = reinterpret_cast<MedOut *>(d + lay.out);
    e = hipMemcpyAsync(d, h, lay.out, hipMemcpyHostToDevice, s);  // one copy in
    if (e == hipSuccess) e = hipEventRecord(c->ev0, s);
    if (e == hipSuccess && n_wave) {
      hipLaunchKernelGGL((median_kernel<1, kMedWavePerLane>), dim3((uint32_t)((n_wave + kMedWaveGroups - 1) / kMedWaveGroups)),
                         dim3(64 * kMedWaveGroups), 0, s, dp, (uint32_t)n_wave, arr, dout);
      e = hipGetLastError();
    }
    if (e == hipSuccess && n_block) {
      hipLaunchKernelGGL((median_kernel<kMedBlockWaves, kMedBlockPerLane>), dim3((uint32_t)n_block),
                         dim3(64 * kMedBlockWaves), 0, s, dp + n_wave, (uint32_t)n_block, arr, dout + n_wave);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(c->ev1, s);
    if (e == hipSuccess) e = hipMemcpyAsync(h + lay.out, d + lay.out, sizeof(MedOut) * P, hipMemcpyDeviceToHost, s);
    // While the device works: GetByAddress returns the FIRST validator with an address, so the
    // validator at the same index is the match only in a set whose addresses are distinct.
    if (e == hipSuccess) {
      try {
        for (const tmed_valset *vs : vsets) (void)sets.get(*vs);
      } catch (...) {  // nothing leaves before the stream has been waited for
        e = hipErrorOutOfMemory;
      }
    }
    const int rc = finish_call(c, s, e, &c->last_ms);
    if (rc != TMED_OK) return rc;
    const MedOut *ho = reinterpret_cast<const MedOut *>(h + lay.out);
    for (size_t j = 0; j < P; j++) {
      if (ho[j].status == kMedMisaligned || !sets.get(*reqs[dev[j]].vals).unique) {
        host.push_back(dev[j]);
        continue;
      }
      tmed_median_result &o = out[dev[j]];
      memset(&o, 0, sizeof(o));
      o.code = (int)ho[j].status;
      o.on_device = 1;
      if (o.code == TMED_MEDIAN_OK) {
        o.entered = ho[j].entered;
        tmed_median::key_time(ho[j].key, &o.seconds, &o.nanos);
      } else if (o.code == TMED_MEDIAN_ZERO_TIME) {
        tmed_median::set_zero_time(o);
      }
    }
  }
  tmed_median::median_run(reqs, host.data(), host.size(), sets, out);
  return TMED_OK;
}

}  // namespace tmed
