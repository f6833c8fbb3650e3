// kc_resolve.h — the key-set cache's side of a seam call (keycache.h / keycache.hip, SURVEY §8f
// f2): the call's sets resolved onto the cache's pool, and the pin that keeps the pool for the call.
// Part of commit.hip's translation unit, after seam_host.h (it defines the KcCall and kc_addr_index
// that planning declares there).
#pragma once

#include "ctx.h"
#include "set_index.h"

// The validator sets of one seam call that carry no handle, resolved through the context's cache:
// the call then runs on copies of its requests whose sets point into the cache's pool (keyset =
// the pool, keyset_index = the set's entry).  The call pins the pool from its first lookup until
// this object dies, after the call's last batch was collected; then the keys that generic sets of
// the call queued are built by the context's key-build worker (keycache.hip), off this call's
// critical path, in stream order ahead of later calls.
// Its buffers are the calling thread's, kept across calls: a light-client batch rewrites ~20k
// requests onto ~10k sets, and fresh pages cost a fault per 4 KB on every call.
struct KcStore {
  std::vector<tmed_commit_request> reqs;
  std::vector<tmed_valset> vals;           // copies of the resolved sets (reqs[q].vals points here)
  std::vector<const tmed::KcSet *> entry;  // the cache entry of vals[s] (nullptr: not keyed)
  // resolution scratch: the distinct sets and request -> set (ix.set_of)
  struct SetRef {
    const tmed_valset *v;
    size_t sigs;
    const tmed::KcSet *e;
    uint64_t handle;
    bool hit, skip;
    tmed::KcKey key;
  };
  std::vector<SetRef> sets;
  SetIndex ix;
};
struct KcCall {
  tmed_ctx *c = nullptr;
  bool active = false;  // this call's requests were rewritten onto st.vals
  KcStore &st;
  KcCall() : st(store()) {}
  ~KcCall() {
    if (!c) return;
    std::lock_guard<std::mutex> lk(c->mu);
    tmed::keycache_unpin(c);  // entries dropped during the call are freed with the last pin
    tmed::keycache_after_call(c);  // the context's worker builds the queued keys
  }
  static KcStore &store() {
    thread_local KcStore s;
    return s;
  }
};

// The cached address index of a set this call resolved through the cache (nullptr otherwise, or
// when the request's addresses differ from the ones the entry's index was built from).
static const AddrIndex *kc_addr_index(const KcCall *kc, const tmed_valset &vs) {
  const std::vector<tmed_valset> &vals = kc->st.vals;
  if (!kc->active || !vs.addresses || &vs < vals.data() || &vs >= vals.data() + vals.size()) return nullptr;
  const tmed::KcSet *e = kc->st.entry[(size_t)(&vs - vals.data())];
  return e ? e->addr_index(vs.addresses, vs.n) : nullptr;
}

static const tmed_commit_request *keycache_resolve(tmed_ctx *ctx, const tmed_commit_request *reqs, size_t n,
                                                   KcCall &kc) {
  if (!ctx->kc_on || n == 0 || !reqs) return reqs;
  PhaseClock clk;
  KcStore &S = kc.st;
  using SetRef = KcStore::SetRef;
  // the distinct tmed_valset structs of the call, in the order of their first request (set_index.h)
  std::vector<SetRef> &sets = S.sets;
  sets.clear();
  const unsigned nt = set_index_threads(n);
  const size_t nsets = number_sets(reqs, n, S.ix, [&] { clk.lap("sets"); });
  if (nsets == 0) return reqs;
  sets.resize(nsets);
  for (size_t k = 0; k < nsets; k++)
    sets[k] = SetRef{reqs[S.ix.first[k]].vals, S.ix.sigs[k], nullptr, 0, false, false, tmed::KcKey()};
  clk.lap("sigs");
  bool any_keyed = false;
  size_t misses = 0;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    kc.c = ctx;
    tmed::keycache_pin(ctx);
    tmed::keycache_touch(ctx);
    // one pass per set in parallel while this thread holds the lock (no writer can run): the
    // digest (or set_hash), the read-only find, the byte compare while the set's keys are in this
    // thread's cache, and the entry's LRU tick
    const uint64_t tick = tmed::keycache_call_tick(ctx);
    std::vector<size_t> thits(std::max(1u, nt), 0), tsigs(std::max(1u, nt), 0);
    parallel_ranges(sets.size(), nt, [&](size_t lo, size_t hi, unsigned t) {
      size_t h = 0, g = 0;  // this worker's hits and their signatures (stored once: shared lines)
      for (size_t s = lo; s < hi; s++) {  // keys and finds first: the compares below prefetch ahead
        SetRef &sr = sets[s];
        const tmed_valset &v = *sr.v;
        sr.skip = v.keyset || v.n == 0 || !v.pubkeys;
        if (sr.skip) continue;
        sr.key = tmed::kc_key(v.pubkeys, v.n, v.set_hash);
        sr.e = tmed::keycache_find(ctx, sr.key);
      }
      // the byte compares (~5.6 KB per set from the caller, cold, against the pool's key table through
      // the entry's indexes): the next set's keys and indexes are prefetched while this one is compared
      auto prefetch_set = [&](size_t s) {
        if (s >= hi || sets[s].skip || !sets[s].e) return;
        const tmed_valset &v = *sets[s].v;
        const uint8_t *a = v.pubkeys, *b = (const uint8_t *)sets[s].e->idx.data();
        const size_t nb = std::min(v.n, sets[s].e->idx.size());
        for (size_t o = 0; o < 32 * v.n; o += 64) __builtin_prefetch(a + o, 0, 0);
        for (size_t o = 0; o < 4 * nb; o += 64) __builtin_prefetch(b + o, 0, 0);
      };
      prefetch_set(lo);
      for (size_t s = lo; s < hi; s++) {
        SetRef &sr = sets[s];
        prefetch_set(s + 1);
        if (sr.skip) continue;
        const tmed_valset &v = *sr.v;
        sr.hit = sr.e && tmed::keycache_same_keys(ctx, *sr.e, v.pubkeys, v.n);
        if (sr.hit) {
          const_cast<tmed::KcSet *>(sr.e)->touch(tick);
          h++;
          g += sr.sigs;
        }
      }
      thits[t] = h;
      tsigs[t] = g;
    });
    clk.lap("find_compare");
    size_t nh = 0, ns = 0;
    for (size_t t = 0; t < thits.size(); t++) {
      nh += thits[t];
      ns += tsigs[t];
    }
    tmed::keycache_hits(ctx, nh, ns);
    any_keyed = nh > 0;
    const uint64_t pool = tmed::keycache_pool_handle(ctx);
    for (SetRef &sr : sets)
      if (sr.hit) sr.handle = pool;
      else if (!sr.skip) misses++;
    if (misses) {
      // the call's signatures against every key it lacks: a window / batch that pays for them all
      // builds them before its kernels (each set alone may carry too few signatures).  A call too
      // small to pay for even one key (a single commit: C1) counts nothing.
      size_t call_sigs = 0, call_missing = 0;
      for (SetRef &sr : sets)
        if (!sr.hit && !sr.skip) call_sigs += sr.sigs;
      if (call_sigs >= tmed::kKcAmortizeSigsPerKey) {
        std::unordered_set<tmed::Pub32, tmed::Pub32Hash> seen;
        for (SetRef &sr : sets)
          if (!sr.hit && !sr.skip) call_missing += tmed::keycache_missing(ctx, sr.v->pubkeys, sr.v->n, &seen);
      }
      const bool build_all = call_missing && call_sigs >= tmed::kKcAmortizeSigsPerKey * call_missing;
      for (SetRef &sr : sets) {
        if (sr.hit || sr.skip) continue;
        sr.e = nullptr;
        // too few signatures for even one key and not every key pooled: generic now, the keys are
        // sorted out by the worker after the call (the first commit of a new set)
        if (!build_all && sr.sigs < tmed::kKcAmortizeSigsPerKey &&
            !tmed::keycache_all_pooled(ctx, sr.v->pubkeys, sr.v->n)) {
          tmed::keycache_defer(ctx, sr.v->pubkeys, sr.v->n, sr.sigs);
          continue;
        }
        if (tmed::keycache_lookup(ctx, sr.v->pubkeys, sr.v->n, sr.key, sr.sigs, /*may_reset=*/!any_keyed, &sr.handle,
                                  sr.e, build_all)) {
          sr.hit = true;
          any_keyed = true;
        }
      }
    }
  }
  clk.lap("lookups");
  if (!any_keyed) {
    clk.emit("keycache_resolve (generic)", n, sets.size());
    return reqs;
  }
  // the call's requests, rewritten onto copies of the sets that resolved keyed
  S.vals.resize(sets.size());
  S.entry.resize(sets.size());
  S.reqs.resize(n);
  parallel_ranges(sets.size(), nt, [&](size_t lo, size_t hi, unsigned) {
    for (size_t s = lo; s < hi; s++) {
      const SetRef &sr = sets[s];
      S.entry[s] = sr.hit ? sr.e : nullptr;
      if (!sr.hit) continue;
      S.vals[s] = *sr.v;
      S.vals[s].keyset = sr.handle;
      S.vals[s].keyset_index = sr.e->idx.data();
    }
  });
  parallel_ranges(n, nt, [&](size_t lo, size_t hi, unsigned) {
    for (size_t q = lo; q < hi; q++) {
      S.reqs[q] = reqs[q];
      const int32_t s = S.ix.set_of[q];
      if (s >= 0 && sets[s].hit) S.reqs[q].vals = &S.vals[s];
    }
  });
  kc.active = true;
  clk.lap("rewrite");
  clk.emit("keycache_resolve", n, sets.size());
  return S.reqs.data();
}
