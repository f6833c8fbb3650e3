// merkle.hip — batched RFC-6962 Merkle roots on gfx950.
//
// Reference (all Go, restated here; oracle/merkle.py is the checker):
//   crypto/merkle/tree.go:9-22   HashFromByteSlices: 0 items -> emptyHash, 1 -> leafHash,
//                                else split at the largest power of two < n, recurse
//   crypto/merkle/hash.go:19-27  leafHash = SHA-256(0x00||x), innerHash = SHA-256(0x01||l||r)
//   types/validator_set.go:347-353  ValidatorSet.Hash = HashFromByteSlices(val.Bytes() ...)
//   types/validator.go:117-133      Validator.Bytes = SimpleValidator{PubKey, VotingPower} proto
//   types/block.go:440-475          Header.Hash = HashFromByteSlices(14 encoded fields)
//   types/part_set.go:166-194       PartSet root = ProofsFromByteSlices(part_size chunks) root
//   types/block.go:894-912          Commit.Hash = HashFromByteSlices(CommitSig proto ...)
//   types/block.go:1004-1012        Data.Hash = Txs.Hash (types/tx.go:47-55): leaves are SHA-256(tx)
// Callers: light/verifier.go:183 (untrustedVals.Hash() per header), :237 (Header.Hash),
// blockchain/v0/reactor.go:359-361 (MakePartSet + first.Hash() per block),
// types/block.go:55-106 (Block.ValidateBasic recomputes LastCommit.Hash and Data.Hash per block).
//
// Device shape: one lane per leaf (SHA-256 of 0x00 || leaf), then one launch per tree level
// over ALL trees of the call (one lane per output node).  The split-point recursion of
// tree.go equals pairing adjacent nodes level by level and promoting an odd last node
// (HashFromByteSlicesIterative, tree.go:57-101, is asserted equal by tree_test.go:104-116),
// which is what the level kernel does.  Work per inner node: 2 SHA-256 blocks.
//
// Host shape, the same for every root and proof call: the level plan (merkle_levels.h) from the
// trees' leaf counts, a leaf stage that writes level 0 into the node buffer, build_levels (the plan
// uploaded once, then every level launch back to back into the one buffer that keeps every level),
// emit_roots on the last level, and one wait before the call returns (finish_call).  The call frame
// (guard, lock, that exit) is call_frame.h; Commit.Hash and the fused Header.Hash stage in tmed_ctx::stage.
//
// Proofs (crypto/merkle/proof.go:35-68, 151-181, 216-237; types/part_set.go:166-194 keeps every
// part's proof, types/tx.go:80-93 builds one per transaction): after the levels are built,
// merkle_aunts_kernel copies each leaf's siblings out of them (no hashing); merkle_verify_kernel is
// Proof.Verify, one lane per proof.  The path arithmetic both share with the host sizing is
// merkle_path.h.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "../../include/tmed25519.h"
#include "call_frame.h"
#include "commitsig_leaf.h"
#include "header_leaf.h"
#include "host_for.h"
#include "merkle_levels.h"
#include "merkle_path.h"
#include "sha256.h"
#include "vote_wire.h"

namespace tmed {

struct Digest { uint32_t w[8]; };

__device__ __forceinline__ void store_digest(Digest *d, const uint32_t st[8]) {
  uint4 *p = reinterpret_cast<uint4 *>(d);
  p[0] = make_uint4(st[0], st[1], st[2], st[3]);
  p[1] = make_uint4(st[4], st[5], st[6], st[7]);
}
__device__ __forceinline__ void load_digest(uint32_t st[8], const Digest *d) {
  const uint4 *p = reinterpret_cast<const uint4 *>(d);
  const uint4 a = p[0], b = p[1];
  st[0] = a.x; st[1] = a.y; st[2] = a.z; st[3] = a.w;
  st[4] = b.x; st[5] = b.y; st[6] = b.z; st[7] = b.w;
}

// leafHash of every leaf: leaf i = leaves[off[i] .. off[i+1]).
__global__ __launch_bounds__(256) void merkle_leaf_kernel(const uint8_t *__restrict__ leaves,
                                                          const uint64_t *__restrict__ off, uint32_t n,
                                                          Digest *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t o0 = off[i], o1 = off[i + 1];
  uint32_t st[8];
  sha256_prefixed(st, 1, 0x00, leaves + o0, (uint32_t)(o1 - o0));
  store_digest(out + i, st);
}

// leafHash(Validator.Bytes()) for ed25519 validators: the SimpleValidator encoding
//   0a 22 | 0a 20 <pubkey 32> | [10 varint(power) if power != 0]
// (types/validator.go:117-133; PublicKey oneof ed25519 = field 1) is built in registers:
// 1 + 36 + <= 11 bytes always fits one SHA-256 block.
__global__ __launch_bounds__(256) void valset_leaf_kernel(const uint8_t *__restrict__ pubkeys,
                                                          const int64_t *__restrict__ powers, uint32_t n,
                                                          Digest *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint8_t b[64];
#pragma unroll
  for (int k = 0; k < 64; k++) b[k] = 0;
  b[0] = 0x00;  // leaf prefix
  b[1] = 0x0a; b[2] = 0x22; b[3] = 0x0a; b[4] = 0x20;
  const uint4 *pk = reinterpret_cast<const uint4 *>(pubkeys + 32 * (size_t)i);
  const uint4 p0 = pk[0], p1 = pk[1];
  const uint32_t pw[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
#pragma unroll
  for (int k = 0; k < 32; k++) b[5 + k] = (uint8_t)(pw[k >> 2] >> (8 * (k & 3)));
  uint32_t len = 37;
  uint64_t v = (uint64_t)powers[i];
  if (v != 0) {
    b[len++] = 0x10;
#pragma unroll
    for (int k = 0; k < 10; k++) {
      b[len++] = (uint8_t)((v & 0x7f) | (v >= 0x80 ? 0x80 : 0));
      v >>= 7;
      if (v == 0) break;
    }
  }
  b[len] = 0x80;
  uint32_t w[16];
#pragma unroll
  for (int t = 0; t < 14; t++)
    w[t] = ((uint32_t)b[4 * t] << 24) | ((uint32_t)b[4 * t + 1] << 16) | ((uint32_t)b[4 * t + 2] << 8) | b[4 * t + 3];
  w[14] = 0;
  w[15] = len * 8;
  uint32_t st[8];
  sha256_init(st);
  sha256_compress(st, w);
  store_digest(out + i, st);
}

// leafHash(CommitSig proto) for Commit.Hash: one lane per CommitSig of the call, read from the
// commits' flat arrays (meta = flag | address length << 8 | signature length << 16; 16-byte loads
// of the 64-byte signature row, dword loads of the 20-byte address row).  The encoding
// (commitsig_leaf.h) is assembled directly as big-endian message words in registers.
__global__ __launch_bounds__(256) void commit_leaf_kernel(const uint32_t *__restrict__ meta,
                                                          const int64_t *__restrict__ seconds,
                                                          const int32_t *__restrict__ nanos,
                                                          const uint8_t *__restrict__ addrs,
                                                          const uint8_t *__restrict__ sigs, uint32_t n,
                                                          Digest *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t m = meta[i];
  uint32_t w[32], st[8];
  const uint32_t len = commitsig_leaf_words(w, m & 0xffu, (m >> 8) & 0xffu, seconds[i], nanos[i], (m >> 16) & 0xffu,
                                            addrs + 20 * (size_t)i, sigs + 64 * (size_t)i);
  sha256_init(st);
  sha256_compress(st, w);
  if (len + 1 > 55) sha256_compress(st, w + 16);  // at most two blocks (static_assert in commitsig_leaf.h)
  store_digest(out + i, st);
}

// leafHash(SHA-256(tx)) for Data.Hash (types/tx.go:47-55): one lane per transaction, the
// transaction streamed as a part-set leaf is, then one block over its digest's state words.
__global__ __launch_bounds__(256) void txs_leaf_kernel(const uint8_t *__restrict__ txs,
                                                       const uint64_t *__restrict__ off, uint32_t n,
                                                       Digest *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t o0 = off[i], o1 = off[i + 1];
  uint32_t h[8], st[8];
  sha256_prefixed(h, 0, 0, txs + o0, (uint32_t)(o1 - o0));
  sha256_leaf32(st, h);
  store_digest(out + i, st);
}

// One tree level for every tree: tree t has c_t = in_base[t+1] - in_base[t] nodes at
// in[in_base[t] ..); output node k of tree t (k < ceil(c_t / 2)) goes to out[out_base[t] + k].
__global__ __launch_bounds__(256) void merkle_level_kernel(const Digest *__restrict__ in,
                                                           const uint32_t *__restrict__ in_base,
                                                           const uint32_t *__restrict__ out_base, uint32_t ntrees,
                                                           uint32_t nout, Digest *__restrict__ out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nout) return;
  uint32_t lo = 0, hi = ntrees;  // last t with out_base[t] <= j (trees with no output are skipped)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (out_base[mid] <= j) lo = mid; else hi = mid;
  }
  const uint32_t t = lo;
  const uint32_t k = j - out_base[t];
  const uint32_t c = in_base[t + 1] - in_base[t];
  const uint32_t src = in_base[t] + 2 * k;
  uint32_t l[8];
  load_digest(l, in + src);
  if (2 * k + 1 < c) {
    uint32_t r[8], st[8];
    load_digest(r, in + src + 1);
    sha256_inner(st, l, r);
    store_digest(out + j, st);
  } else {
    store_digest(out + j, l);  // odd node promoted
  }
}

// roots[t] = digest bytes of tree t's single node, or emptyHash for an empty tree.
__global__ __launch_bounds__(256) void merkle_emit_kernel(const Digest *__restrict__ in,
                                                          const uint32_t *__restrict__ base, uint32_t ntrees,
                                                          uint8_t *__restrict__ roots) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntrees) return;
  uint32_t st[8];
  if (base[t + 1] == base[t]) sha256_prefixed(st, 0, 0, nullptr, 0);  // emptyHash
  else load_digest(st, in + base[t]);
  uint32_t *o = reinterpret_cast<uint32_t *>(roots + 32 * (size_t)t);
#pragma unroll
  for (int k = 0; k < 8; k++) o[k] = bswap32(st[k]);
}

// ---- Merkle proofs (crypto/merkle/proof.go) ------------------------------------------------------
// Every level is kept (merkle_levels.h): level l of all trees lies tree-contiguous at nodes +
// lvl_off[l] (tree t's nodes at tab[l * (ntrees + 1) + t] ..), built by merkle_level_kernel from
// level l - 1.  A tree that is down to one node carries it through the remaining levels, so the last
// level holds every root.

// Proof.Aunts and Proof.LeafHash of every leaf, no hashing: eight lanes per leaf, lane w of a leaf
// copies digest word w.  The leaf at position p of its tree walks the kept levels: at a level of c
// nodes its node's sibling p ^ 1 is the next aunt if it exists (p ^ 1 < c; an odd last node is
// promoted and contributes nothing), then p >>= 1, until c = 1 (merkle_path.h merkle_aunt_count is
// the same walk and sized aunt_off).  Each group of eight lanes reads one whole 32-byte digest and
// writes one whole 32-byte hash per step, so every store instruction fills 32-byte sectors.
__global__ __launch_bounds__(256) void merkle_aunts_kernel(const Digest *__restrict__ nodes,
                                                           const uint64_t *__restrict__ lvl_off,
                                                           const uint32_t *__restrict__ tab, uint32_t ntrees,
                                                           uint32_t nlevels, uint32_t nleaves,
                                                           const uint64_t *__restrict__ aunt_off,
                                                           uint32_t *__restrict__ aunts,
                                                           uint32_t *__restrict__ leaf_hashes) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t i = (uint32_t)(j >> 3), w = (uint32_t)j & 7u;
  if ((j >> 3) >= nleaves) return;
  uint32_t lo = 0, hi = ntrees;  // last t with tab[t] <= i (empty trees are skipped)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (tab[mid] <= i) lo = mid; else hi = mid;
  }
  const uint32_t t = lo;
  uint32_t p = i - tab[t];
  leaf_hashes[8 * (size_t)i + w] = bswap32(nodes[i].w[w]);
  const uint64_t a0 = aunt_off[i], a1 = aunt_off[i + 1];
  uint64_t a = a0;
  for (uint32_t l = 0; l < nlevels && a < a1; l++) {
    const uint32_t *tb = tab + (size_t)l * (ntrees + 1);
    const uint32_t base = tb[t], c = tb[t + 1] - base;
    if (c <= 1) break;
    const uint32_t sib = p ^ 1u;
    if (sib < c) {
      aunts[8 * a + w] = bswap32(nodes[lvl_off[l] + base + sib].w[w]);
      a++;
    }
    p >>= 1;
  }
}

__device__ __forceinline__ void load_hash_be(uint32_t st[8], const uint8_t *h) {
  const uint4 *p = reinterpret_cast<const uint4 *>(h);  // hashes lie at multiples of 32 bytes
  const uint4 a = p[0], b = p[1];
  st[0] = bswap32(a.x); st[1] = bswap32(a.y); st[2] = bswap32(a.z); st[3] = bswap32(a.w);
  st[4] = bswap32(b.x); st[5] = bswap32(b.y); st[6] = bswap32(b.z); st[7] = bswap32(b.w);
}

// Proof.Verify (proof.go:52-68), one lane per proof; code[i] = TMED_PROOF_*.  The checks in the
// reference's order; computeHashFromAunts (:151-181) as merkle_path's top-down walk (path length
// and side mask, no aunt read unless the count fits) and a bottom-up fold of the aunts.
__global__ __launch_bounds__(256) void merkle_verify_kernel(const uint8_t *__restrict__ leaves,
                                                            const uint64_t *__restrict__ leaf_off,
                                                            const uint8_t *__restrict__ leaf_hashes,
                                                            const int64_t *__restrict__ totals,
                                                            const int64_t *__restrict__ indexes,
                                                            const uint64_t *__restrict__ aunt_off,
                                                            const uint8_t *__restrict__ aunts,
                                                            const uint8_t *__restrict__ roots,
                                                            const uint32_t *__restrict__ root_of, uint32_t n,
                                                            uint8_t *__restrict__ code) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t total = totals[i], index = indexes[i];
  if (total < 0) { code[i] = TMED_PROOF_NEGATIVE_TOTAL; return; }
  if (index < 0) { code[i] = TMED_PROOF_NEGATIVE_INDEX; return; }
  const uint64_t o0 = leaf_off[i], o1 = leaf_off[i + 1];
  uint32_t h[8], x[8];
  sha256_prefixed(h, 1, 0x00, leaves + o0, (uint32_t)(o1 - o0));
  load_hash_be(x, leaf_hashes + 32 * (size_t)i);
  bool same = true;
#pragma unroll
  for (int k = 0; k < 8; k++) same &= h[k] == x[k];
  if (!same) { code[i] = TMED_PROOF_LEAF_HASH; return; }
  uint32_t d;
  uint64_t mask;
  const uint64_t a0 = aunt_off[i];
  if (!merkle_path(index, total, &d, &mask) || aunt_off[i + 1] - a0 != d) {
    code[i] = TMED_PROOF_ROOT_HASH;
    return;
  }
#pragma unroll 1
  for (uint32_t k = 0; k < d; k++) {
    uint32_t st[8];
    load_hash_be(x, aunts + 32 * (a0 + k));
    if ((mask >> k) & 1) sha256_inner(st, x, h);
    else sha256_inner(st, h, x);
#pragma unroll
    for (int q = 0; q < 8; q++) h[q] = st[q];
  }
  load_hash_be(x, roots + 32 * (size_t)(root_of ? root_of[i] : i));
#pragma unroll
  for (int k = 0; k < 8; k++) same &= h[k] == x[k];
  code[i] = same ? TMED_PROOF_OK : TMED_PROOF_ROOT_HASH;
}

// ---- Header.Hash in one launch (types/block.go:440-475; leaves, record and fold: header_leaf.h) ----
// A 16-lane group per header, four headers per wave: lane l < 14 encodes leaf l and takes its
// leafHash, then the fixed tree 14 -> 7 -> 4 -> 2 -> 1 is folded inside the group: at step s = 1, 2,
// 4, 8 the node at lane l (a multiple of 2 s) takes the node at lane l + s as its right child when
// that lane holds one (l + s < 14), else it is the odd last node and is promoted as it is: the same
// pairing as merkle_level_kernel.  Every lane of the wave runs every shuffle: lanes 14 and 15 of a
// group redo leaf 13 and the groups past n redo header n - 1; neither is ever taken or stored.
__global__ __launch_bounds__(256) void header_hash_kernel(const uint8_t *__restrict__ recs, uint32_t n,
                                                          uint8_t *__restrict__ out) {
  const uint32_t l = threadIdx.x & 15u, g = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const uint32_t hi = g < n ? g : n - 1, sl = l < kHdrLeaves ? l : kHdrLeaves - 1;
  const uint8_t *rec = recs + (size_t)hi * kHdrRecBytes;
  const uint4 m = reinterpret_cast<const uint4 *>(rec + kHdrMetaOff)[sl];
  const uint4 *img = reinterpret_cast<const uint4 *>(rec + sl * kHdrSlotBytes);
  uint32_t w[32];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const uint4 q = img[k];
    w[4 * k] = bswap32(q.x); w[4 * k + 1] = bswap32(q.y); w[4 * k + 2] = bswap32(q.z); w[4 * k + 3] = bswap32(q.w);
  }
  const uint32_t len = header_leaf_words(w, sl, m.x, m.y, m.z, m.w);
  uint32_t d[8];
  sha256_init(d);
  sha256_compress(d, w);
  if (len > 55) sha256_compress(d, w + 16);
#pragma unroll
  for (uint32_t s = 1; s < 16; s <<= 1) {
    uint32_t r[8], st[8];
#pragma unroll
    for (int k = 0; k < 8; k++) r[k] = __shfl_down(d[k], s, 16);
    sha256_inner(st, d, r);
    const bool take = header_fold_takes(l, s);
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = take ? st[k] : d[k];
  }
  if (l == 0 && g < n) {
    uint4 *o = reinterpret_cast<uint4 *>(out + 32 * (size_t)g);
    o[0] = make_uint4(bswap32(d[0]), bswap32(d[1]), bswap32(d[2]), bswap32(d[3]));
    o[1] = make_uint4(bswap32(d[4]), bswap32(d[5]), bswap32(d[6]), bswap32(d[7]));
  }
}

// One step of a call's chain of stream operations: after a failure (e) or for no lanes nothing is
// launched; else kernel k over `lanes` lanes in blocks of 256.
template <class K, class... A>
static hipError_t launch(hipError_t e, K k, size_t lanes, hipStream_t s, A... args) {
  if (e != hipSuccess || lanes == 0) return e;
  hipLaunchKernelGGL(k, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, s, args...);
  return hipGetLastError();
}

// ---- the one tree builder ---------------------------------------------------------------------
// d_merkle_lv holds every level of the call's plan (merkle_levels.h), d_merkle_tab the plan itself:
// the level starts, then (from the next multiple of 256 bytes) the per-level base tables.  Every
// function below takes ctx->mu held and queues on the context stream without waiting.
static Digest *dev_nodes(tmed_ctx *c) { return (Digest *)c->d_merkle_lv.p; }
static const uint64_t *dev_lvl_off(tmed_ctx *c) { return (const uint64_t *)c->d_merkle_tab.p; }
static const uint32_t *dev_tab(tmed_ctx *c, const MerkleLevels &p) {
  return (const uint32_t *)((const uint8_t *)c->d_merkle_tab.p + align256(p.nlevels * 8));
}

// Room for every node of the plan, before the leaf stage writes level 0 at the buffer's start
// (and before the call queues anything).  TMED_EINVAL past 2^32 - 1 leaves: the tables are 32-bit.
static int ensure_nodes(tmed_ctx *c, const MerkleLevels &p) {
  if (p.leaves > 0xffffffffu) return TMED_EINVAL;
  return map_err(c->d_merkle_lv.ensure(std::max<uint64_t>(p.nodes, 1) * sizeof(Digest)));
}

// Level 0 (written by a leaf stage queued before) -> every level: the plan uploaded once, then one
// merkle_level_kernel launch per level, back to back.
static hipError_t build_levels(tmed_ctx *c, const MerkleLevels &p, hipStream_t s) {
  const size_t o_tab = align256(p.nlevels * 8);
  hipError_t e = c->d_merkle_tab.ensure(o_tab + p.tab.size() * 4);
  if (e != hipSuccess) return e;
  uint8_t *d = (uint8_t *)c->d_merkle_tab.p;
  e = hipMemcpyAsync(d, p.lvl_off.data(), p.nlevels * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d + o_tab, p.tab.data(), p.tab.size() * 4, hipMemcpyHostToDevice, s);
  Digest *lv = dev_nodes(c);
  const uint32_t *tab = dev_tab(c, p);
  for (size_t l = 0; l + 1 < p.nlevels; l++)
    e = launch(e, merkle_level_kernel, p.level_nodes(l + 1), s, lv + p.lvl_off[l], tab + l * (p.T + 1),
               tab + (l + 1) * (p.T + 1), (uint32_t)p.T, p.level_nodes(l + 1), lv + p.lvl_off[l + 1]);
  return e;
}

// The last level -> d_roots (32 B a tree, emptyHash for an empty tree).
static hipError_t emit_roots(tmed_ctx *c, const MerkleLevels &p, uint8_t *d_roots, hipStream_t s) {
  const size_t last = p.nlevels - 1;
  return launch(hipSuccess, merkle_emit_kernel, p.T, s, dev_nodes(c) + p.lvl_off[last],
                dev_tab(c, p) + last * (p.T + 1), (uint32_t)p.T, d_roots);
}

}  // namespace tmed

using namespace tmed;

namespace {

// Every extern "C" function of this file runs in the shared call frame: guarded(body) (api_guard.h),
// in which body checks the arguments and builds the call's host vectors, then locked(c, collect, run)
// for the device part, which leaves through finish_call (call_frame.h; timed calls pass &c->last_ms
// for the kernel of record between ev0 and ev1, tmed_last_kernel_ms).

// ---- argument checks ------------------------------------------------------------------------
// The forest of a byte-slice call (n_trees >= 1): tree t holds leaves [tree_off[t], tree_off[t+1]),
// leaf i the bytes [leaf_off[i], leaf_off[i+1]) of `leaves`.  counts: leaves per tree.
int forest_counts(const uint32_t *tree_off, size_t n_trees, const uint64_t *leaf_off, const uint8_t *leaves,
                  std::vector<uint32_t> &counts) {
  const size_t L = tree_off[n_trees];
  if (tree_off[0] != 0) return TMED_EINVAL;
  counts.resize(n_trees);
  for (size_t t = 0; t < n_trees; t++) {
    if (tree_off[t + 1] < tree_off[t]) return TMED_EINVAL;
    counts[t] = tree_off[t + 1] - tree_off[t];
  }
  for (size_t i = 0; i < L; i++)
    if (leaf_off[i + 1] < leaf_off[i] || leaf_off[i + 1] - leaf_off[i] > 0xffffffffu - 64) return TMED_EINVAL;
  if (L && leaf_off[L] > leaf_off[0] && !leaves) return TMED_EINVAL;
  return TMED_OK;
}

// The part sets of a part-set call (n_blocks >= 1): block b's bytes [data_off[b], data_off[b+1]) cut
// into parts of part_size (types/part_set.go:166-194).  off: the parts' offsets (from data_off[0]),
// counts: parts per block, part_off (n_blocks + 1 entries, or NULL): each block's first part.  The
// running part count is checked per block, so no offsets are pushed past 2^32 - 1 parts.
int split_parts(const uint8_t *data, const uint64_t *data_off, size_t n_blocks, uint32_t part_size,
                std::vector<uint64_t> &off, std::vector<uint32_t> &counts, uint32_t *part_off) {
  counts.resize(n_blocks);
  off.assign(1, data_off[0]);
  for (size_t b = 0; b < n_blocks; b++) {
    if (data_off[b + 1] < data_off[b]) return TMED_EINVAL;
    const uint64_t len = data_off[b + 1] - data_off[b];
    const uint64_t parts = (len + part_size - 1) / part_size;  // types/part_set.go:168
    if (parts > 0xffffffffu || off.size() - 1 + parts > 0xffffffffu) return TMED_EINVAL;
    counts[b] = (uint32_t)parts;
    if (part_off) part_off[b] = (uint32_t)(off.size() - 1);
    for (uint64_t p = 0; p < parts; p++) off.push_back(std::min(data_off[b] + (p + 1) * part_size, data_off[b + 1]));
  }
  if (part_off) part_off[n_blocks] = (uint32_t)(off.size() - 1);
  return off.size() > 1 && !data ? TMED_EINVAL : TMED_OK;
}

// gogoproto varint / field helpers for the header leaves (types/block.go:440-475)
void put_varint(std::vector<uint8_t> &o, uint64_t v) {
  uint8_t b[10];
  o.insert(o.end(), b, b + put_uvarint(b, 0, v));
}
void put_bytes_field(std::vector<uint8_t> &o, uint8_t tag, const uint8_t *p, size_t n) {
  o.push_back(tag);
  put_varint(o, n);
  o.insert(o.end(), p, p + n);
}

// The 14 leaves of Header.Hash, appended to `leaves` with their offsets.
void header_leaves(const tmed_header &h, std::vector<uint8_t> &leaves, std::vector<uint64_t> &off) {
  std::vector<uint8_t> f;
  auto push = [&]() { leaves.insert(leaves.end(), f.begin(), f.end()); off.push_back(leaves.size()); f.clear(); };
  // 1. Version (tendermint.version.Consensus): block = 1, app = 2, zero fields omitted
  if (h.version_block) { f.push_back(0x08); put_varint(f, h.version_block); }
  if (h.version_app) { f.push_back(0x10); put_varint(f, h.version_app); }
  push();
  // 2. cdcEncode(ChainID): gogotypes.StringValue{1: value}
  if (h.chain_id_len) put_bytes_field(f, 0x0a, (const uint8_t *)h.chain_id, h.chain_id_len);
  push();
  // 3. cdcEncode(Height): gogotypes.Int64Value{1: value}
  if (h.height) { f.push_back(0x08); put_varint(f, (uint64_t)h.height); }
  push();
  // 4. gogotypes.StdTimeMarshal(Time): Timestamp{1: seconds, 2: nanos}
  if (h.time_seconds) { f.push_back(0x08); put_varint(f, (uint64_t)h.time_seconds); }
  if (h.time_nanos) { f.push_back(0x10); put_varint(f, (uint64_t)(int64_t)h.time_nanos); }
  push();
  // 5. LastBlockID.ToProto().Marshal(): BlockID{1: hash, 2: PartSetHeader (always present)}
  {
    std::vector<uint8_t> psh;
    if (h.last_block_id.psh_total) { psh.push_back(0x08); put_varint(psh, h.last_block_id.psh_total); }
    if (h.last_block_id.psh_hash_len)
      put_bytes_field(psh, 0x12, h.last_block_id.psh_hash, h.last_block_id.psh_hash_len);
    if (h.last_block_id.hash_len) put_bytes_field(f, 0x0a, h.last_block_id.hash, h.last_block_id.hash_len);
    put_bytes_field(f, 0x12, psh.data(), psh.size());
  }
  push();
  // 6..14. cdcEncode(HexBytes): gogotypes.BytesValue{1: value}
  for (int k = 0; k < 9; k++) {
    if (h.hash_lens[k]) put_bytes_field(f, 0x0a, h.hashes[k], h.hash_lens[k]);
    push();
  }
}

// The leaf stage of the byte-slice calls: L leaves on the host -> level 0 (ensure_nodes has run).
// txs: the byte slices are transactions (leaf = leafHash(SHA-256(tx)), txs_leaf_kernel); else they
// are the leaves themselves.  timed: ev0 / ev1 around the leaf kernel.
hipError_t hash_host_leaves(tmed_ctx *c, const uint8_t *leaves, const uint64_t *leaf_off, size_t L, bool txs,
                            bool timed, hipStream_t s) {
  const size_t bytes = leaf_off[L] - leaf_off[0];
  hipError_t e = c->d_msg.ensure(bytes + 16);
  if (e == hipSuccess) e = c->d_off.ensure((L + 1) * 8);
  if (e != hipSuccess) return e;
  std::vector<uint64_t> &off = c->merkle_off;
  off.resize(L + 1);
  for (size_t i = 0; i <= L; i++) off[i] = leaf_off[i] - leaf_off[0];
  if (bytes) e = hipMemcpyAsync(c->d_msg.p, leaves + leaf_off[0], bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(c->d_off.p, off.data(), (L + 1) * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && timed) e = hipEventRecord(c->ev0, s);
  e = launch(e, txs ? txs_leaf_kernel : merkle_leaf_kernel, L, s, (const uint8_t *)c->d_msg.p,
             (const uint64_t *)c->d_off.p, (uint32_t)L, dev_nodes(c));
  if (e == hipSuccess && timed) e = hipEventRecord(c->ev1, s);
  return e;
}

// Leaves on the host -> roots on the host: the common driver of the byte-slice root calls (the
// transactions' leaf kernel is timed for tmed_last_kernel_ms).  ctx->mu held.
// d_keep: device memory that also receives the T roots (a copy on the stream, for a caller that reads
// them there: validate.hip).
int roots_from_host_leaves_locked(tmed_ctx *c, const uint8_t *leaves, const uint64_t *leaf_off, size_t L,
                                  const std::vector<uint32_t> &counts, uint8_t *roots, bool txs = false,
                                  uint8_t *d_keep = nullptr) {
  const MerkleLevels plan(counts);
  const size_t T = counts.size();
  (void)hipSetDevice(c->device);
  hipStream_t s = c->stream;
  const int rc = ensure_nodes(c, plan);
  if (rc != TMED_OK) return rc;
  hipError_t e = c->d_out.ensure(T * 32);
  if (e == hipSuccess) e = hash_host_leaves(c, leaves, leaf_off, L, txs, /*timed=*/txs, s);
  if (e == hipSuccess) e = build_levels(c, plan, s);
  if (e == hipSuccess) e = emit_roots(c, plan, (uint8_t *)c->d_out.p, s);
  if (e == hipSuccess && d_keep) e = hipMemcpyAsync(d_keep, c->d_out.p, T * 32, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(roots, c->d_out.p, T * 32, hipMemcpyDeviceToHost, s);
  return finish_call(c, s, e, txs ? &c->last_ms : nullptr);
}

// ---- Commit.Hash (types/block.go:894-912) ---------------------------------------------------
// The commits' arrays of one call, packed per kind: region offsets for N signatures.
struct CsigLayout {
  size_t sig, sec, meta, nanos, addr, roots, flags, total;  // flags: the raw BlockIDFlag bytes, for a shared arena only
  bool with_flags;
  CsigLayout(size_t N, size_t n_commits, bool with_flags_ = false) : with_flags(with_flags_) {
    sig = 0;
    sec = align256(sig + 64 * N);
    meta = align256(sec + 8 * N);
    nanos = align256(meta + 4 * N);
    addr = align256(nanos + 4 * N);
    roots = align256(addr + 20 * N);
    flags = total = roots + 32 * n_commits;
    if (with_flags) {
      flags = align256(total);
      total = flags + N;
    }
  }
};

// 0: this struct cannot reproduce the commit's hash (ok = 0); 1: it can; TMED_EINVAL: a missing array.
int commit_scan(const tmed_commit &cm) {
  const size_t n = cm.n_sigs;
  if (n == 0) return 1;
  if (!cm.flags || !cm.ts_seconds || !cm.ts_nanos) return TMED_EINVAL;
  bool ok = true, any_addr = false, any_sig = false;
  for (size_t j = 0; j < n; j++) {
    const uint32_t sl = cm.sig_lens ? cm.sig_lens[j] : 64u;
    const uint32_t al = cm.address_lens ? cm.address_lens[j] : 20u;
    any_sig |= sl != 0;
    any_addr |= al == 20;
    ok &= sl <= 64 && (al == 0 || al == 20);
    // outside StdTimeMarshal's range the reference's Marshal fails and Commit.Hash panics
    ok &= timestamp_encodable(cm.ts_seconds[j], cm.ts_nanos[j]);
  }
  if ((any_addr && !cm.addresses) || (ok && any_sig && !cm.sigs)) return TMED_EINVAL;
  return ok ? 1 : 0;
}

// Commit cm's arrays into the staging regions at signature index base.
void commit_pack(const tmed_commit &cm, uint8_t *h, const CsigLayout &lay, size_t base) {
  const size_t n = cm.n_sigs;
  if (n == 0) return;
  if (lay.with_flags) memcpy(h + lay.flags + base, cm.flags, n);
  if (cm.sigs) memcpy(h + lay.sig + 64 * base, cm.sigs, 64 * n);
  memcpy(h + lay.sec + 8 * base, cm.ts_seconds, 8 * n);
  memcpy(h + lay.nanos + 4 * base, cm.ts_nanos, 4 * n);
  if (cm.addresses) memcpy(h + lay.addr + 20 * base, cm.addresses, 20 * n);
  uint32_t *meta = reinterpret_cast<uint32_t *>(h + lay.meta) + base;
  for (size_t j = 0; j < n; j++) {
    const uint32_t sl = cm.sig_lens ? cm.sig_lens[j] : 64u;
    const uint32_t al = cm.address_lens ? cm.address_lens[j] : 20u;
    meta[j] = (uint32_t)cm.flags[j] | (al << 8) | (sl << 16);
  }
}

// Element i of an array of structs or of an array of pointers to them: the hash bodies below take
// either (a caller whose structs lie apart passes the pointers and copies nothing).
template <class T>
inline const T &item(const T *a, size_t i) { return a[i]; }
template <class T>
inline const T &item(const T *const *a, size_t i) { return *a[i]; }

// Header.Hash of the headers idx[0 .. m) (all header_fused_ok) into out + 32 * idx[j].  ctx->mu held.
template <class HA>
int header_hashes_fused(tmed_ctx *c, HA headers, const std::vector<size_t> &idx, uint8_t *out,
                        uint8_t *d_keep = nullptr) {
  const size_t m = idx.size();
  if (m > 0x0fffffffu) return TMED_EINVAL;
  const size_t o_roots = m * (size_t)kHdrRecBytes;  // a multiple of 256
  (void)hipSetDevice(c->device);
  hipStream_t s = c->stream;
  hipError_t e = c->stage.ensure(o_roots + 32 * m, o_roots + 32 * m);
  if (e != hipSuccess) return map_err(e);
  uint8_t *h = c->stage.host(), *d = c->stage.dev();
  host_for(m, pack_threads(m * 32), [&](size_t j) { header_pack(item(headers, idx[j]), h + j * kHdrRecBytes); });
  e = hipMemcpyAsync(d, h, o_roots, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipEventRecord(c->ev0, s);
  e = launch(e, header_hash_kernel, 16 * m, s, (const uint8_t *)d, (uint32_t)m, d + o_roots);
  if (e == hipSuccess) e = hipEventRecord(c->ev1, s);
  if (e == hipSuccess && d_keep) e = hipMemcpyAsync(d_keep, d + o_roots, 32 * m, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(h + o_roots, d + o_roots, 32 * m, hipMemcpyDeviceToHost, s);
  const int rc = finish_call(c, s, e, &c->last_ms);
  if (rc != TMED_OK) return rc;
  for (size_t j = 0; j < m; j++) memcpy(out + 32 * idx[j], h + o_roots + 32 * j, 32);
  return TMED_OK;
}

// shared: stage into the arena tmed_ctx::vb_commit instead of tmed_ctx::stage, with the raw flags beside
// the other arrays, and report where they and the roots lie on the device: they stay there after the
// call (no other routine uses that arena), for the median kernels and block_check_kernel of the same
// tmed_validate_blocks call.
template <class CA>
int commit_hashes_locked(tmed_ctx *c, CA commits, size_t n, const std::vector<uint32_t> &counts,
                         const std::vector<size_t> &base, size_t N, uint8_t *out, CommitArena *shared = nullptr) {
  const MerkleLevels plan(counts);
  (void)hipSetDevice(c->device);
  hipStream_t s = c->stream;
  const CsigLayout lay(N, n, shared != nullptr);
  int rc = ensure_nodes(c, plan);
  if (rc != TMED_OK) return rc;
  Staged &arena = shared ? c->vb_commit : c->stage;
  hipError_t e = arena.ensure(lay.total, lay.total);
  if (e != hipSuccess) return map_err(e);
  uint8_t *h = arena.host(), *d = arena.dev();
  if (shared) {
    shared->flags = d + lay.flags, shared->addr = d + lay.addr, shared->roots = d + lay.roots;
    shared->sec = (const int64_t *)(d + lay.sec), shared->nanos = (const int32_t *)(d + lay.nanos);
  }
  host_for(n, pack_threads(N), [&](size_t i) {
    if (counts[i]) commit_pack(item(commits, i), h, lay, base[i]);
  });
  if (N) {  // one copy per array kind
    e = hipMemcpyAsync(d + lay.sig, h + lay.sig, 64 * N, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + lay.sec, h + lay.sec, 8 * N, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + lay.meta, h + lay.meta, 4 * N, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + lay.nanos, h + lay.nanos, 4 * N, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + lay.addr, h + lay.addr, 20 * N, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && shared) e = hipMemcpyAsync(d + lay.flags, h + lay.flags, N, hipMemcpyHostToDevice, s);
  }
  if (e == hipSuccess) e = hipEventRecord(c->ev0, s);
  e = launch(e, commit_leaf_kernel, N, s, (const uint32_t *)(d + lay.meta), (const int64_t *)(d + lay.sec),
             (const int32_t *)(d + lay.nanos), d + lay.addr, d + lay.sig, (uint32_t)N, dev_nodes(c));
  if (e == hipSuccess) e = hipEventRecord(c->ev1, s);
  if (e == hipSuccess) e = build_levels(c, plan, s);
  if (e == hipSuccess) e = emit_roots(c, plan, d + lay.roots, s);
  if (e == hipSuccess) e = hipMemcpyAsync(h + lay.roots, d + lay.roots, n * 32, hipMemcpyDeviceToHost, s);
  rc = finish_call(c, s, e, &c->last_ms);
  if (rc != TMED_OK) return rc;
  memcpy(out, h + lay.roots, n * 32);
  return TMED_OK;
}

// tmed_commit_hashes once its pointers are checked: the scan of every commit, the device part under
// the context's lock (held: the caller holds it already and has collected the submitted windows),
// the hashes of the commits with ok = 0 zeroed.
template <class CA>
int commit_hashes_body(tmed_ctx *c, CA commits, size_t n, uint8_t *out, uint8_t *ok, bool held,
                       CommitArena *shared = nullptr) {
  std::vector<uint32_t> counts(n);
  std::vector<size_t> base(n);
  size_t N = 0, all = 0;
  for (size_t i = 0; i < n; i++) all += item(commits, i).n_sigs;
  std::vector<int> scan(n);
  host_for(n, pack_threads(all), [&](size_t i) { scan[i] = commit_scan(item(commits, i)); });
  for (size_t i = 0; i < n; i++) {
    const int r = scan[i];
    if (r < 0) return r;
    ok[i] = (uint8_t)r;
    base[i] = N;
    if (item(commits, i).n_sigs > 0xffffffffu) return TMED_EINVAL;
    counts[i] = r ? (uint32_t)item(commits, i).n_sigs : 0;  // a commit with ok = 0 contributes no leaves
    N += counts[i];
    if (N > 0xffffffffu) return TMED_EINVAL;
  }
  if (shared) {  // each commit's first signature in the arena's arrays (a commit with ok = 0 is not staged)
    shared->base.assign(n, (size_t)-1);
    for (size_t i = 0; i < n; i++)
      if (counts[i] || item(commits, i).n_sigs == 0) shared->base[i] = base[i];
  }
  const int rc = held ? commit_hashes_locked(c, commits, n, counts, base, N, out, shared)
                      : locked(c, /*collect=*/true, [&] { return commit_hashes_locked(c, commits, n, counts, base, N, out); });
  if (rc != TMED_OK) return rc;
  for (size_t i = 0; i < n; i++)
    if (!ok[i]) memset(out + 32 * i, 0, 32);
  return TMED_OK;
}

// ---- Merkle proofs --------------------------------------------------------------------------
// The caller's output arrays of a generator (include/tmed25519.h).
struct ProofOut {
  uint8_t *roots, *leaf_hashes;
  uint64_t *aunt_off;
  uint8_t *aunts;
  size_t aunts_cap;
  size_t *aunts_len;
};

// Every level of every tree on the device, then the aunts: leaves (host) -> o (host).  ao: the
// leaves' aunt offsets (sized by the caller).  ctx->mu held.
int proofs_locked(tmed_ctx *c, const uint8_t *leaves, const uint64_t *leaf_off, size_t L,
                  const std::vector<uint32_t> &counts, bool txs, const std::vector<uint64_t> &ao, const ProofOut &o) {
  const MerkleLevels plan(counts);
  const size_t T = counts.size();
  const size_t need = 32 * (size_t)ao[L];
  const size_t o_leaf = align256(need), o_root = align256(o_leaf + 32 * L);  // d_proof_out: aunts | leaf hashes | roots
  (void)hipSetDevice(c->device);
  hipStream_t s = c->stream;
  const int rc = ensure_nodes(c, plan);
  if (rc != TMED_OK) return rc;
  hipError_t e = c->d_proof_off.ensure((L + 1) * 8);
  if (e == hipSuccess) e = c->d_proof_out.ensure(o_root + 32 * T);
  uint8_t *d_res = (uint8_t *)c->d_proof_out.p;
  if (e == hipSuccess) e = hash_host_leaves(c, leaves, leaf_off, L, txs, /*timed=*/false, s);
  if (e == hipSuccess) e = build_levels(c, plan, s);
  if (e == hipSuccess) e = emit_roots(c, plan, d_res + o_root, s);
  if (e == hipSuccess) e = hipMemcpyAsync(c->d_proof_off.p, ao.data(), (L + 1) * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipEventRecord(c->ev0, s);
  if (e == hipSuccess)  // (the device tables are there once build_levels has run)
    e = launch(e, merkle_aunts_kernel, 8 * L, s, dev_nodes(c), dev_lvl_off(c), dev_tab(c, plan), (uint32_t)T,
               (uint32_t)plan.nlevels, (uint32_t)L, (const uint64_t *)c->d_proof_off.p, (uint32_t *)d_res,
               (uint32_t *)(d_res + o_leaf));
  if (e == hipSuccess) e = hipEventRecord(c->ev1, s);
  if (e == hipSuccess && need) e = hipMemcpyAsync(o.aunts, d_res, need, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && L) e = hipMemcpyAsync(o.leaf_hashes, d_res + o_leaf, 32 * L, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(o.roots, d_res + o_root, 32 * T, hipMemcpyDeviceToHost, s);
  return finish_call(c, s, e, &c->last_ms);
}

// The common tail of the three generators: size the aunts on the host (merkle_path.h), answer a
// sizing call or a too small buffer there, else run the device route.
int proofs_from_host_leaves(tmed_ctx *c, const uint8_t *leaves, const uint64_t *leaf_off, size_t L,
                            const std::vector<uint32_t> &counts, bool txs, const ProofOut &o) {
  std::vector<uint64_t> ao(L + 1);
  size_t i = 0;
  ao[0] = 0;
  for (const uint32_t n : counts)
    for (uint32_t p = 0; p < n; p++, i++) ao[i + 1] = ao[i] + merkle_aunt_count(p, n);
  const size_t need = 32 * (size_t)ao[L];
  if (o.aunts && o.aunts_cap < need) return TMED_ENOMEM;
  if (o.aunts) {
    if (!o.roots || (L && !o.leaf_hashes)) return TMED_EINVAL;
    const int rc =
        locked(c, /*collect=*/true, [&] { return proofs_locked(c, leaves, leaf_off, L, counts, txs, ao, o); });
    if (rc != TMED_OK) return rc;
  }
  memcpy(o.aunt_off, ao.data(), (L + 1) * 8);
  *o.aunts_len = need;
  return TMED_OK;
}

// The caller's arrays of tmed_merkle_proofs_verify: leaves and aunts from their first used byte.
struct ProofIn {
  size_t n;
  const uint8_t *roots;
  size_t n_roots;
  const uint32_t *root_of;
  const uint8_t *leaves;
  size_t leaf_bytes;
  const uint8_t *leaf_hashes;
  const int64_t *totals, *indexes;
  const uint8_t *aunts;
  size_t n_aunts;
};

// Proofs (host) -> codes (host).  off: the n + 1 leaf offsets, then the n + 1 aunt offsets, both
// from 0.  The aunts lie in d_merkle_lv (the generators' digest buffer).  ctx->mu held.
int verify_proofs_locked(tmed_ctx *c, const ProofIn &in, const std::vector<uint64_t> &off, uint8_t *out_code) {
  const size_t n = in.n;
  // d_proof_in: leaf hashes | roots | totals | indexes | root indexes
  const size_t o_root = align256(32 * n), o_tot = align256(o_root + 32 * in.n_roots),
               o_idx = align256(o_tot + 8 * n), o_rof = align256(o_idx + 8 * n);
  (void)hipSetDevice(c->device);
  hipStream_t s = c->stream;
  hipError_t e = c->d_msg.ensure(in.leaf_bytes + 16);
  if (e == hipSuccess) e = c->d_off.ensure((n + 1) * 8);
  if (e == hipSuccess) e = c->d_proof_off.ensure((n + 1) * 8);
  if (e == hipSuccess) e = c->d_merkle_lv.ensure(std::max<size_t>(in.n_aunts, 1) * sizeof(Digest));
  if (e == hipSuccess) e = c->d_proof_in.ensure(o_rof + (in.root_of ? 4 * n : 0));
  if (e == hipSuccess) e = c->d_proof_out.ensure(n);
  if (e != hipSuccess) return map_err(e);
  uint8_t *d_in = (uint8_t *)c->d_proof_in.p;
  if (in.leaf_bytes) e = hipMemcpyAsync(c->d_msg.p, in.leaves, in.leaf_bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(c->d_off.p, off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(c->d_proof_off.p, off.data() + n + 1, (n + 1) * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && in.n_aunts)
    e = hipMemcpyAsync(c->d_merkle_lv.p, in.aunts, 32 * in.n_aunts, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_in, in.leaf_hashes, 32 * n, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_in + o_root, in.roots, 32 * in.n_roots, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_in + o_tot, in.totals, 8 * n, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_in + o_idx, in.indexes, 8 * n, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && in.root_of) e = hipMemcpyAsync(d_in + o_rof, in.root_of, 4 * n, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipEventRecord(c->ev0, s);
  e = launch(e, merkle_verify_kernel, n, s, (const uint8_t *)c->d_msg.p, (const uint64_t *)c->d_off.p,
             (const uint8_t *)d_in, (const int64_t *)(d_in + o_tot), (const int64_t *)(d_in + o_idx),
             (const uint64_t *)c->d_proof_off.p, (const uint8_t *)c->d_merkle_lv.p, (const uint8_t *)(d_in + o_root),
             in.root_of ? (const uint32_t *)(d_in + o_rof) : nullptr, (uint32_t)n, (uint8_t *)c->d_proof_out.p);
  if (e == hipSuccess) e = hipEventRecord(c->ev1, s);
  if (e == hipSuccess) e = hipMemcpyAsync(out_code, c->d_proof_out.p, n, hipMemcpyDeviceToHost, s);
  return finish_call(c, s, e, &c->last_ms);
}

// tmed_merkle_roots, and tmed_txs_hashes (txs) over blocks of transactions
int forest_roots(tmed_ctx *c, const uint8_t *leaves, const uint64_t *leaf_off, const uint32_t *tree_off,
                 size_t n_trees, uint8_t *roots, bool txs) {
  if (!c || (n_trees && (!tree_off || !roots || !leaf_off))) return TMED_EINVAL;
  if (n_trees == 0) return TMED_OK;
  return guarded([&] {
    std::vector<uint32_t> counts;
    const int rc = forest_counts(tree_off, n_trees, leaf_off, leaves, counts);
    if (rc != TMED_OK) return rc;
    return locked(c, /*collect=*/false, [&] {
      return roots_from_host_leaves_locked(c, leaves, leaf_off, tree_off[n_trees], counts, roots, txs);
    });
  });
}

// tmed_merkle_proofs, and tmed_txs_proofs (txs) over blocks of transactions
int forest_proofs(tmed_ctx *c, const uint8_t *leaves, const uint64_t *leaf_off, const uint32_t *tree_off,
                  size_t n_trees, bool txs, const ProofOut &o) {
  if (!c || !o.aunt_off || !o.aunts_len || (n_trees && (!tree_off || !leaf_off))) return TMED_EINVAL;
  if (n_trees == 0) {
    o.aunt_off[0] = 0;
    *o.aunts_len = 0;
    return TMED_OK;
  }
  return guarded([&] {
    std::vector<uint32_t> counts;
    const int rc = forest_counts(tree_off, n_trees, leaf_off, leaves, counts);
    if (rc != TMED_OK) return rc;
    return proofs_from_host_leaves(c, leaves, leaf_off, tree_off[n_trees], counts, txs, o);
  });
}

}  // namespace

namespace tmed {

// The tree builder as evidence.hip uses it (ctx.h).
int merkle_ensure_nodes(tmed_ctx *c, const MerkleLevels &plan) { return ensure_nodes(c, plan); }
void *merkle_level0(tmed_ctx *c) { return dev_nodes(c); }
hipError_t merkle_leaf_hashes(const uint8_t *d_leaves, const uint64_t *d_off, uint32_t n, void *d_out, hipStream_t s) {
  return launch(hipSuccess, merkle_leaf_kernel, n, s, d_leaves, d_off, n, (Digest *)d_out);
}
hipError_t merkle_build_levels(tmed_ctx *c, const MerkleLevels &plan, hipStream_t s) { return build_levels(c, plan, s); }
hipError_t merkle_emit_roots(tmed_ctx *c, const MerkleLevels &plan, uint8_t *d_roots, hipStream_t s) {
  return emit_roots(c, plan, d_roots, s);
}

bool header_pointers_ok(const tmed_header &h) {
  for (int k = 0; k < 9; k++)
    if (h.hash_lens[k] && !h.hashes[k]) return false;
  return !((h.chain_id_len && !h.chain_id) || (h.last_block_id.hash_len && !h.last_block_id.hash) ||
           (h.last_block_id.psh_hash_len && !h.last_block_id.psh_hash));
}

int valset_hashes_locked(tmed_ctx *c, const uint8_t *pubkeys, const int64_t *powers, const uint32_t *set_off,
                         size_t n_sets, uint8_t *out, uint8_t *d_keep) {
  const size_t N = set_off[n_sets];
  std::vector<uint32_t> counts(n_sets);
  for (size_t t = 0; t < n_sets; t++) counts[t] = set_off[t + 1] - set_off[t];
  const MerkleLevels plan(counts);
  (void)hipSetDevice(c->device);
  hipStream_t s = c->stream;
  const int rc = ensure_nodes(c, plan);
  if (rc != TMED_OK) return rc;
  hipError_t e = c->d_a.ensure(std::max<size_t>(N, 1) * 32);
  if (e == hipSuccess) e = c->d_b.ensure(std::max<size_t>(N, 1) * 8);
  if (e == hipSuccess) e = c->d_out.ensure(n_sets * 32);
  if (e == hipSuccess && N) e = hipMemcpyAsync(c->d_a.p, pubkeys, N * 32, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && N) e = hipMemcpyAsync(c->d_b.p, powers, N * 8, hipMemcpyHostToDevice, s);
  e = launch(e, valset_leaf_kernel, N, s, (const uint8_t *)c->d_a.p, (const int64_t *)c->d_b.p, (uint32_t)N,
             dev_nodes(c));
  if (e == hipSuccess) e = build_levels(c, plan, s);
  if (e == hipSuccess) e = emit_roots(c, plan, (uint8_t *)c->d_out.p, s);
  if (e == hipSuccess && d_keep) e = hipMemcpyAsync(d_keep, c->d_out.p, n_sets * 32, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(out, c->d_out.p, n_sets * 32, hipMemcpyDeviceToHost, s);
  return finish_call(c, s, e);
}

// ValidatorSet.Hash of n_sets validator sets given as structs: their keys and powers are packed
// straight into the context's pinned staging (h_a / h_b: one pass over the callers' arrays, and the
// copies to the device run from page-locked memory), then hashed as above.
int valsets_hashes_locked(tmed_ctx *c, const tmed_valset *const *sets, size_t n_sets, uint8_t *out, uint8_t *d_keep) {
  std::vector<uint32_t> set_off(n_sets + 1, 0);
  for (size_t s = 0; s < n_sets; s++) {
    if (sets[s]->n > 0xffffffffu - set_off[s]) return TMED_EINVAL;
    set_off[s + 1] = set_off[s] + (uint32_t)sets[s]->n;
  }
  const size_t N = set_off[n_sets];
  (void)hipSetDevice(c->device);
  hipError_t e = c->h_a.ensure(std::max<size_t>(N, 1) * 32);
  if (e == hipSuccess) e = c->h_b.ensure(std::max<size_t>(N, 1) * 8);
  if (e != hipSuccess) return map_err(e);
  uint8_t *pubs = (uint8_t *)c->h_a.p;
  int64_t *pows = (int64_t *)c->h_b.p;
  host_for(n_sets, pack_threads(N), [&](size_t s) {
    if (!sets[s]->n) return;
    memcpy(pubs + 32 * (size_t)set_off[s], sets[s]->pubkeys, 32 * sets[s]->n);
    memcpy(pows + set_off[s], sets[s]->powers, 8 * sets[s]->n);
  });
  return valset_hashes_locked(c, pubs, pows, set_off.data(), n_sets, out, d_keep);
}

// Commit.Hash and Data.Hash as tmed_commit_hashes / tmed_txs_hashes compute them, for a caller that
// holds ctx->mu and has collected the submitted windows (validate.hip); n, n_blocks >= 1.
int commit_hashes_held(tmed_ctx *c, const tmed_commit *const *commits, size_t n, uint8_t *out, uint8_t *ok,
                       CommitArena *shared) {
  return commit_hashes_body(c, commits, n, out, ok, /*held=*/true, shared);
}
int txs_hashes_held(tmed_ctx *c, const uint8_t *txs, const uint64_t *tx_off, const uint32_t *block_off, size_t n_blocks,
                    uint8_t *out, uint8_t *d_keep) {
  if (!tx_off || !block_off) return TMED_EINVAL;
  std::vector<uint32_t> counts;
  const int rc = forest_counts(block_off, n_blocks, tx_off, txs, counts);
  if (rc != TMED_OK) return rc;
  return roots_from_host_leaves_locked(c, txs, tx_off, block_off[n_blocks], counts, out, /*txs=*/true, d_keep);
}

// Eligible headers (header_fused_ok) through header_hash_kernel, the others through host-encoded
// leaves and the generic leaf and level kernels; ok = 0 and a zeroed hash where ValidatorsHash is
// empty (Header.Hash returns nil, types/block.go:441-443).
// d_keep (n x 32, device): also receives the hashes there, the headers of the fused route first, in
// their order, then the others in theirs; row_of[i] (n entries) tells header i's row.
template <class HA>
static int header_hashes_any(tmed_ctx *c, HA headers, size_t n, uint8_t *out, uint8_t *ok, uint8_t *d_keep,
                         uint32_t *row_of) {
  std::vector<size_t> fused, rest;
  for (size_t i = 0; i < n; i++) (header_fused_ok(item(headers, i)) ? fused : rest).push_back(i);
  if (row_of) {
    for (size_t j = 0; j < fused.size(); j++) row_of[fused[j]] = (uint32_t)j;
    for (size_t j = 0; j < rest.size(); j++) row_of[rest[j]] = (uint32_t)(fused.size() + j);
  }
  int rc = TMED_OK;
  if (!fused.empty()) rc = header_hashes_fused(c, headers, fused, out, d_keep);
  if (rc == TMED_OK && !rest.empty()) {
    std::vector<uint8_t> leaves, roots(32 * rest.size());
    std::vector<uint64_t> off;
    leaves.reserve(rest.size() * 200);
    off.reserve(rest.size() * 14 + 1);
    off.push_back(0);
    for (const size_t i : rest) header_leaves(item(headers, i), leaves, off);
    const std::vector<uint32_t> counts(rest.size(), 14);
    rc = roots_from_host_leaves_locked(c, leaves.data(), off.data(), off.size() - 1, counts, roots.data(), /*txs=*/false,
                                       d_keep ? d_keep + 32 * fused.size() : nullptr);
    if (rc == TMED_OK)
      for (size_t j = 0; j < rest.size(); j++) memcpy(out + 32 * rest[j], roots.data() + 32 * j, 32);
  }
  if (rc != TMED_OK) return rc;
  for (size_t i = 0; i < n; i++) {
    ok[i] = item(headers, i).hash_lens[2] != 0;
    if (!ok[i]) memset(out + 32 * i, 0, 32);
  }
  return TMED_OK;
}
int header_hashes_locked(tmed_ctx *c, const tmed_header *headers, size_t n, uint8_t *out, uint8_t *ok, uint8_t *d_keep,
                         uint32_t *row_of) {
  return header_hashes_any(c, headers, n, out, ok, d_keep, row_of);
}
int header_hashes_locked(tmed_ctx *c, const tmed_header *const *headers, size_t n, uint8_t *out, uint8_t *ok,
                         uint8_t *d_keep, uint32_t *row_of) {
  return header_hashes_any(c, headers, n, out, ok, d_keep, row_of);
}

}  // namespace tmed

extern "C" {

int tmed_commit_hashes(tmed_ctx *c, const tmed_commit *commits, size_t n, uint8_t *out, uint8_t *ok) {
  if (!c || (n && (!commits || !out || !ok))) return TMED_EINVAL;
  if (n == 0) return TMED_OK;
  return guarded([&] { return commit_hashes_body(c, commits, n, out, ok, /*held=*/false); });
}

int tmed_txs_hashes(tmed_ctx *c, const uint8_t *txs, const uint64_t *tx_off, const uint32_t *block_off,
                    size_t n_blocks, uint8_t *out) {
  return forest_roots(c, txs, tx_off, block_off, n_blocks, out, /*txs=*/true);
}

int tmed_merkle_roots(tmed_ctx *c, const uint8_t *leaves, const uint64_t *leaf_off, const uint32_t *tree_off,
                      size_t n_trees, uint8_t *roots) {
  return forest_roots(c, leaves, leaf_off, tree_off, n_trees, roots, /*txs=*/false);
}

int tmed_valset_hashes(tmed_ctx *c, const uint8_t *pubkeys, const int64_t *powers, const uint32_t *set_off,
                       size_t n_sets, uint8_t *out) {
  if (!c || (n_sets && (!set_off || !out))) return TMED_EINVAL;
  if (n_sets == 0) return TMED_OK;
  const size_t N = set_off[n_sets];
  if (set_off[0] != 0 || (N && (!pubkeys || !powers))) return TMED_EINVAL;
  for (size_t t = 0; t < n_sets; t++)
    if (set_off[t + 1] < set_off[t]) return TMED_EINVAL;
  return guarded([&] {
    return locked(c, /*collect=*/false, [&] { return valset_hashes_locked(c, pubkeys, powers, set_off, n_sets, out); });
  });
}

int tmed_header_hashes(tmed_ctx *c, const tmed_header *headers, size_t n, uint8_t *out, uint8_t *ok) {
  if (!c || (n && (!headers || !out || !ok))) return TMED_EINVAL;
  if (n == 0) return TMED_OK;
  for (size_t i = 0; i < n; i++)
    if (!header_pointers_ok(headers[i])) return TMED_EINVAL;
  return guarded([&] {
    return locked(c, /*collect=*/false, [&] { return header_hashes_locked(c, headers, n, out, ok); });
  });
}

int tmed_partset_roots(tmed_ctx *c, const uint8_t *data, const uint64_t *data_off, size_t n_blocks,
                       uint32_t part_size, uint8_t *roots) {
  if (!c || part_size == 0 || (n_blocks && (!data_off || !roots))) return TMED_EINVAL;
  if (n_blocks == 0) return TMED_OK;
  return guarded([&] {
    std::vector<uint64_t> off;
    std::vector<uint32_t> counts;
    const int rc = split_parts(data, data_off, n_blocks, part_size, off, counts, nullptr);
    if (rc != TMED_OK) return rc;
    return locked(c, /*collect=*/false, [&] {
      return roots_from_host_leaves_locked(c, data, off.data(), off.size() - 1, counts, roots);
    });
  });
}

// ---- Merkle proofs (the generators share proofs_from_host_leaves; arguments checked as the root calls)

int tmed_merkle_proofs(tmed_ctx *c, const uint8_t *leaves, const uint64_t *leaf_off, const uint32_t *tree_off,
                       size_t n_trees, uint8_t *roots, uint8_t *leaf_hashes, uint64_t *aunt_off, uint8_t *aunts,
                       size_t aunts_cap, size_t *aunts_len) {
  return forest_proofs(c, leaves, leaf_off, tree_off, n_trees, /*txs=*/false,
                       ProofOut{roots, leaf_hashes, aunt_off, aunts, aunts_cap, aunts_len});
}

int tmed_txs_proofs(tmed_ctx *c, const uint8_t *txs, const uint64_t *tx_off, const uint32_t *block_off,
                    size_t n_blocks, uint8_t *roots, uint8_t *leaf_hashes, uint64_t *aunt_off, uint8_t *aunts,
                    size_t aunts_cap, size_t *aunts_len) {
  return forest_proofs(c, txs, tx_off, block_off, n_blocks, /*txs=*/true,
                       ProofOut{roots, leaf_hashes, aunt_off, aunts, aunts_cap, aunts_len});
}

int tmed_partset_proofs(tmed_ctx *c, const uint8_t *data, const uint64_t *data_off, size_t n_blocks,
                        uint32_t part_size, uint8_t *roots, uint32_t *part_off, uint8_t *leaf_hashes,
                        uint64_t *aunt_off, uint8_t *aunts, size_t aunts_cap, size_t *aunts_len) {
  if (!c || part_size == 0 || !aunt_off || !aunts_len || !part_off || (n_blocks && !data_off)) return TMED_EINVAL;
  if (n_blocks == 0) {
    aunt_off[0] = 0;
    part_off[0] = 0;
    *aunts_len = 0;
    return TMED_OK;
  }
  return guarded([&] {
    std::vector<uint64_t> off;
    std::vector<uint32_t> counts, poff(n_blocks + 1);
    int rc = split_parts(data, data_off, n_blocks, part_size, off, counts, poff.data());
    if (rc != TMED_OK) return rc;
    rc = proofs_from_host_leaves(c, data, off.data(), off.size() - 1, counts, /*txs=*/false,
                                 ProofOut{roots, leaf_hashes, aunt_off, aunts, aunts_cap, aunts_len});
    if (rc == TMED_OK) memcpy(part_off, poff.data(), (n_blocks + 1) * 4);
    return rc;
  });
}

int tmed_merkle_proofs_verify(tmed_ctx *c, size_t n, const uint8_t *roots, size_t n_roots, const uint32_t *root_of,
                              const uint8_t *leaves, const uint64_t *leaf_off, const uint8_t *leaf_hashes,
                              const int64_t *totals, const int64_t *indexes, const uint64_t *aunt_off,
                              const uint8_t *aunts, uint8_t *out_code) {
  if (!c) return TMED_EINVAL;
  if (n == 0) return TMED_OK;
  if (!roots || !leaf_off || !leaf_hashes || !totals || !indexes || !aunt_off || !out_code || n > 0xffffffffu)
    return TMED_EINVAL;
  for (size_t i = 0; i < n; i++) {
    if (leaf_off[i + 1] < leaf_off[i] || leaf_off[i + 1] - leaf_off[i] > 0xffffffffu - 64) return TMED_EINVAL;
    if (aunt_off[i + 1] < aunt_off[i]) return TMED_EINVAL;
    if ((root_of ? root_of[i] : i) >= n_roots) return TMED_EINVAL;
  }
  const size_t bytes = leaf_off[n] - leaf_off[0];
  const uint64_t A = aunt_off[n] - aunt_off[0];
  if ((bytes && !leaves) || (A && !aunts) || A > (~(size_t)0 >> 5)) return TMED_EINVAL;
  return guarded([&] {
    std::vector<uint64_t> off(2 * (n + 1));  // leaf offsets, then aunt offsets, both from 0
    for (size_t i = 0; i <= n; i++) {
      off[i] = leaf_off[i] - leaf_off[0];
      off[n + 1 + i] = aunt_off[i] - aunt_off[0];
    }
    const ProofIn in{n, roots, n_roots, root_of, bytes ? leaves + leaf_off[0] : nullptr, bytes, leaf_hashes, totals,
                     indexes, A ? aunts + 32 * aunt_off[0] : nullptr, (size_t)A};
    return locked(c, /*collect=*/true, [&] { return verify_proofs_locked(c, in, off, out_code); });
  });
}

}  // extern "C"
