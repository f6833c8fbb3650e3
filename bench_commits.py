#!/usr/bin/env python3
"""bench_commits.py — commit-level workloads of BASELINE.json through the drop-in seam.

  --config c1   VerifyCommit p50 latency @175 validators (BASELINE metric, second half):
                end-to-end through tmed_verify_commits (sign-bytes + staging + device + replay),
                generic and key-cached paths, next to the CPU path (the port verifying the
                same 175 tuples sequentially, 1 thread: the reference's loop).
  --config c3   light client: H headers x 175 validators, the set changing by one key per
                height; direct: each (h, h+2) pair = VerifyCommitLightTrusting(1/3) +
                VerifyCommitLight, all pairs in one seam call (light/verifier.go:32-79), median of
                --runs calls with the host plan/verify/replay shares; bisection: targets 150
                heights away, verifySkipping's pivots (light/client.go:706-773), one seam call per round.
  --config c3v  the c3 direct workload through light.Verify itself (tmed_light_verify) over real
                headers, beside (a) the c3 leg and (b) the c3 leg plus separate tmed_header_hashes
                and tmed_valset_hashes calls over the same headers, all in one run.
  --config c4   blocksync replay: B blocks x V validators, VerifyCommitLight per block
                (blockchain/v0/reactor.go:366-367), key-cached; with N ranks the blocks are
                sharded and the per-rank int64 tallies all-reduced (RCCL; gloo on CPU).
  --config mt   block time: state.MedianTime (state/validation.go:123-129) for 1,000 commits x 10,000
                validators and 10,000 x 175, all aligned, one tmed_median_times call per shape: calls/s
                and the selection kernels' device time, the same pairs through tmed_median_times_host
                on one thread, and tmed_verify_commits (VerifyCommit) over the same commits for scale.
  --config votes  free-standing votes: one round's prevotes and precommits (2 x 10,000 against a
                10,000-validator set, and 2 x 175) through tmed_verify_votes (VoteSet.addVote's checks and
                Vote.Verify on the device), beside the route there was before (the sign-bytes of every vote
                on the host, then tmed_verify_batch_keyset) and oracle.port on one thread, in one run:
                votes/s, vote_prepare_kernel's device time, the call's host share.
  --config evidence  duplicate-vote evidence: one block at the byte cap (2,048 evidences against a 10,000-
                validator set) and 1,000 lists x 4 evidences against 175 validators (--evidence-shapes) through
                tmed_verify_duplicate_votes (VerifyDuplicateVote on the device: the address lookup, the checks,
                both signatures) plus tmed_evidence_hashes (every DuplicateVoteEvidence.Hash and EvidenceList.Hash),
                beside the route there was before (tmed_verify_duplicate_votes_host's checks on the host, then
                tmed_verify_votes over the 2n votes; tmed_evidence_bytes, then tmed_merkle_roots), in one run, once
                both routes agree on every code and root: evidences/s, the lookup, prepare and leaf-stage kernels'
                device time, the calls' host share.
  --config lca   light-client-attack evidence: E lunatic evidences x V validators (default 1x10000 and
                 50x175; every common validator signs the conflicting block): one
                 tmed_verify_light_client_attacks call against the route there was before:
                 tmed_verify_commits on the Trusting + Light pairs, tmed_header_hashes on the 2E
                 headers, tmed_byzantine_validators_host on one thread.
  --config vb    block validation: validateBlock (state/validation.go:15-151) over a linked window of B
                 blocks x V validators with a constant set (default 1000x10000 and 10000x175; --vb-shapes):
                 one tmed_validate_blocks call against the composed route there was before it (the
                 seven calls tmed_commit_hashes, tmed_txs_hashes, tmed_evidence_hashes,
                 tmed_header_hashes, tmed_valset_hashes, tmed_median_times, tmed_verify_commits, then the
                 proposer lookup and the compares on the host), alternated in the same run --runs times;
                 --vb-route fused|composed times one route alone (one profiler run per route).
Synthetic data (seeded keys, GPU RFC 8032 signer); prints one JSON line per config.
"""
from __future__ import annotations

import argparse
import dataclasses
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "tendermint-fork_amd"))

T2023 = 1672531200


def block_id(tag: bytes):
    from tmed.types import BlockID
    return BlockID(hashlib.sha256(tag).digest(), 123, hashlib.sha256(tag + b"/psh").digest())


def c1(eng, reps: int, cpu: bool, first_sets: int = 30):
    """VerifyCommit p50 @175 validators through tmed_verify_commits, four ways:
      cache_hit        the drop-in as patched (no key-set handle): the context's
                       key-set cache holds the set (state/validation.go:93-96 checks every block's
                       LastCommit against the same LastValidators) — the headline value;
      first_call_after_set_change  the same harness on `first_sets` sets never seen before, one call
                       each (generic kernels; the call queues the set's keys for the next one), the
                       device idle between calls as between blocks;
      first_call_after_warmed_set_change  sets the node warmed when it learnt them
                       (tmed_keycache_warm at the validator update, two heights ahead), then one call;
      generic_cache_off  the cache off: every call generic;
      explicit_keyset  a tmed_keyset_load handle passed by the caller (round-3 headline path).
    p50 / p90 / min over `reps` calls of one prepared request, and the p50 with the request marshalled
    inside the timed call (what the Go shim rebuilds per call)."""
    import tmed.types as T
    from tmed.workload import make_valset, pubkeys_of, seeds_from_tag, sign_commits
    n = 175

    def c1_set(tag):
        seeds = seeds_from_tag(tag, 0, n)
        vals, order = make_valset(pubkeys_of(eng, seeds), [10] * n)
        addrs = np.array([np.frombuffer(v.address, np.uint8) for v in vals.validators])
        return seeds, vals, order, addrs

    seeds, vals, order, addrs = c1_set(b"tmed-bench-key")
    bid = block_id(b"tmed-c1")
    commit = sign_commits(eng, "test_chain_id", [(seeds[order], addrs, 3, 0, bid, T2023, None)])[0]
    req = (T.MODE_COMMIT, vals, "test_chain_id", bid, 3, commit, 0, 0)

    def timed(pb, k):
        ts = []
        for _ in range(k):
            t0 = time.perf_counter()
            pb.run(eng)
            ts.append(time.perf_counter() - t0)
        return np.array(ts) * 1e3

    def summary(ts, tm=None):
        d = {"p50_ms": round(float(np.median(ts)), 4), "p90_ms": round(float(np.percentile(ts, 90)), 4),
             "min_ms": round(float(ts.min()), 4), "calls": int(ts.shape[0])}
        if tm is not None:
            d["p50_ms_incl_marshal"] = round(float(np.median(tm)), 4)
        return d

    def marshal_timed(k):
        tm = []
        for _ in range(k):
            t0 = time.perf_counter()
            pm = T.PreparedBatch([req])
            pm.run(eng)
            tm.append(time.perf_counter() - t0)
        assert pm.codes()[0] == 0
        return np.array(tm) * 1e3

    out = {}
    ks0 = eng.keycache_stats()
    eng.keycache_config(True)
    pb = T.PreparedBatch([req])
    for _ in range(20):
        pb.run(eng)
    assert pb.codes()[0] == 0 and pb.verified()[0] == n
    s0 = eng.keycache_stats()
    ts = timed(pb, reps)
    s1 = eng.keycache_stats()
    out["cache_hit"] = summary(ts, marshal_timed(max(50, reps // 4)))
    out["cache_hit"]["keycache"] = {"lookups": s1["lookups"] - s0["lookups"], "hits": s1["hits"] - s0["hits"],
                                    "keyed_sets": s1["keyed_sets"] - s0["keyed_sets"]}
    # first calls: fresh sets (other keys), signed once, one untimed idle device between calls
    import torch
    firsts, gen_before = [], eng.keycache_stats()["generic_sets"]
    specs = []
    for k in range(first_sets):
        sd, v2, o2, a2 = c1_set(b"tmed-c1-first-%d" % k)
        specs.append((sd[o2], a2, 3, 0, bid, T2023, None, v2))
    fc = sign_commits(eng, "test_chain_id", [s[:7] for s in specs])
    for (spec, c2) in zip(specs, fc):
        p2 = T.PreparedBatch([(T.MODE_COMMIT, spec[7], "test_chain_id", bid, 3, c2, 0, 0)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p2.run(eng)
        firsts.append(time.perf_counter() - t0)
        assert p2.codes()[0] == 0
        eng.keycache_wait()  # the queued key build finishes before the next block's commit
    out["first_call_after_set_change"] = summary(np.array(firsts) * 1e3)
    out["first_call_after_set_change"]["generic_calls"] = eng.keycache_stats()["generic_sets"] - gen_before
    # the same on sets the node warmed when it learnt them (tmed_keycache_warm: EndBlock's validator
    # updates take effect two heights later, state/execution.go updateState, so the keys are built
    # before the set's first commit arrives) — untimed warm, then the first call
    firsts_w, specs = [], []
    for k in range(first_sets):
        sd, v2, o2, a2 = c1_set(b"tmed-c1-warm-%d" % k)
        specs.append((sd[o2], a2, 3, 0, bid, T2023, None, v2))
    fc = sign_commits(eng, "test_chain_id", [s[:7] for s in specs])
    hits_before = eng.keycache_stats()["hits"]
    for (spec, c2) in zip(specs, fc):
        eng.keycache_warm(spec[7])
        p2 = T.PreparedBatch([(T.MODE_COMMIT, spec[7], "test_chain_id", bid, 3, c2, 0, 0)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p2.run(eng)
        firsts_w.append(time.perf_counter() - t0)
        assert p2.codes()[0] == 0
    out["first_call_after_warmed_set_change"] = summary(np.array(firsts_w) * 1e3)
    out["first_call_after_warmed_set_change"]["cache_hits"] = eng.keycache_stats()["hits"] - hits_before
    eng.keycache_config(False)
    # the same first calls with the cache off (fresh sets, a fresh batch each, the device idle
    # before each): what a first call costs without the cache's resolution and queued build
    firsts_off, specs = [], []
    for k in range(first_sets):
        sd, v2, o2, a2 = c1_set(b"tmed-c1-first-off-%d" % k)
        specs.append((sd[o2], a2, 3, 0, bid, T2023, None, v2))
    fc = sign_commits(eng, "test_chain_id", [s[:7] for s in specs])
    for (spec, c2) in zip(specs, fc):
        p2 = T.PreparedBatch([(T.MODE_COMMIT, spec[7], "test_chain_id", bid, 3, c2, 0, 0)])
        torch.cuda.synchronize()
        time.sleep(0.002)
        t0 = time.perf_counter()
        p2.run(eng)
        firsts_off.append(time.perf_counter() - t0)
        assert p2.codes()[0] == 0
    out["first_call_cache_off"] = summary(np.array(firsts_off) * 1e3)
    for _ in range(20):
        pb.run(eng)
    out["generic_cache_off"] = summary(timed(pb, reps), marshal_timed(max(50, reps // 4)))
    eng.keycache_config(True)
    kv = T.ValidatorSet(list(vals.validators))
    kv.keyset = eng.keyset_load(np.array([np.frombuffer(v.pub_key, np.uint8) for v in vals.validators]))
    pk = T.PreparedBatch([(T.MODE_COMMIT, kv, "test_chain_id", bid, 3, commit, 0, 0)])
    for _ in range(20):
        pk.run(eng)
    assert pk.codes()[0] == 0
    out["explicit_keyset"] = summary(timed(pk, reps))
    eng.keyset_free(kv.keyset)
    res = {"metric": "VerifyCommit p50 latency @175 validators", "unit": "ms", "higher_is_better": False,
           "value": out["cache_hit"]["p50_ms"], "paths": out, "reps": reps,
           "config": {"workload": "C1: 175-validator commit, equal power 10, test_chain_id, height 3, round 0",
                      "seam": "tmed_verify_commits (C++ plan/sign-bytes/replay + gfx950 batch), sets passed "
                              "without key-set handles: the context's key-set cache (tmed_keycache_*) decides",
                      "keycache_before": {k: ks0[k] for k in ("pool_keys", "sets_cached")}}}
    if cpu:
        sys.path.insert(0, ROOT)
        from oracle import port  # cpu_baseline leg only
        from tmed.signbytes import make_template, vote_sign_bytes_batch
        t = make_template("test_chain_id", 3, 0, bid.hash, bid.psh_total, bid.psh_hash)
        msgs, offs = vote_sign_bytes_batch(t, commit.ts_seconds, commit.ts_nanos, commit.flags)
        vp = np.array([np.frombuffer(v.pub_key, np.uint8) for v in vals.validators])
        ts = []
        for _ in range(max(50, reps // 10)):
            t0 = time.perf_counter()
            ok = port.verify_batch(vp, commit.sigs, msgs, offs.astype(np.uint64), 1)
            ts.append(time.perf_counter() - t0)
        assert ok.all()
        p50 = float(np.median(ts)) * 1e3
        res["cpu_baseline"] = {"value": round(p50, 4), "unit": "ms (p50)", "cores": 1, "kind": "port",
                               "sample": "the 175 VerifySignature calls of the same commit, sequential, 1 thread"}
        res["speedup_vs_cpu"] = round(p50 / out["cache_hit"]["p50_ms"], 2)
    return res


def _host_threads():
    """The seam's host worker count (commit.hip host_threads: TMED_HOST_THREADS, default 16,
    capped at the machine's hardware threads)."""
    want = int(os.environ.get("TMED_HOST_THREADS", "16"))
    return {"seam_threads": min(want, os.cpu_count() or 1), "machine_hw_threads": os.cpu_count()}


def _c3_world(eng, headers: int, reach: int, use_keyset: bool):
    """Heights 0 .. headers + reach - 1: validator set h = pool keys [h, h + 175) (one key
    replaced per height, equal powers 10), commit h signed by set h.  use_keyset: one explicit key
    set of the whole pool indexed per set (keyset_index, the round-3 harness); otherwise the sets
    carry no handle and the seam's key-set cache pools their keys itself."""
    from tmed.workload import make_valset, pubkeys_of, seeds_from_tag, sign_commits
    nv = 175
    nh = headers + reach
    pool_seeds = seeds_from_tag(b"tmed-c3-key", 0, nh + nv)
    pool_pubs = pubkeys_of(eng, pool_seeds)
    ks = eng.keyset_load(pool_pubs) if use_keyset else 0
    sets, specs = [], []
    for h in range(nh):
        vals, order = make_valset(pool_pubs[h:h + nv], [10] * nv)
        if ks:
            vals.keyset = ks
            vals.keyset_index = (order + h).astype(np.uint32)
        sets.append(vals)
        addrs = np.array([np.frombuffer(v.address, np.uint8) for v in vals.validators])
        specs.append((pool_seeds[h:h + nv][order], addrs, h + 1, 0, block_id(b"c3-%d" % (h + 1)), T2023 + h, None))
    if not ks and hasattr(eng, "_h"):  # (a GPU engine: tools/c3_host_profile.py passes a stand-in)
        # the light client holds every set's ValidatorSet.Hash() (header.ValidatorsHash /
        # NextValidatorsHash, checked against the set by light/verifier.go): the drop-in passes it as
        # the cache key (tmed_valset.set_hash), computed here by the f3 kernels (tmed_valset_hashes)
        from tmed.merkle import valset_hashes
        for vals, hsh in zip(sets, valset_hashes(eng, sets)):
            vals.set_hash = hsh
    t_sign = time.perf_counter()
    commits = sign_commits(eng, "test_chain_id", specs)
    return sets, commits, ks, time.perf_counter() - t_sign


def _timed_runs(eng, pb, runs: int):
    """`runs` timed seam calls of one prepared batch: (median s, min s, max s, the median host
    phase times of tmed_seam_phase_us as fractions of the median call).  A large call is
    pipelined by the seam: then plan = host plan + staging and replay = host scatter + replay
    (both overlapping device work) and verify = the time the host sat waiting for the device."""
    from tmed.affinity import cgroup_cpu_stat, cgroup_delta
    from tmed.types import seam_phase_us
    import resource
    ts, ph, flt = [], [], []
    cg0, w0 = cgroup_cpu_stat(), time.perf_counter()
    for _ in range(runs):
        f0 = resource.getrusage(resource.RUSAGE_SELF).ru_minflt
        t0 = time.perf_counter()
        pb.run(eng)
        ts.append(time.perf_counter() - t0)
        flt.append(resource.getrusage(resource.RUSAGE_SELF).ru_minflt - f0)
        ph.append(seam_phase_us())
    cg = cgroup_delta(cg0, cgroup_cpu_stat(), time.perf_counter() - w0)
    if cg is not None:
        cg["minor_faults_per_call"] = int(np.median(flt))  # page faults of the whole process
        cg["call_ms"] = [round(t * 1e3, 2) for t in ts]
    ph = np.median(np.array(ph), axis=0)
    med = float(np.median(ts))
    frac = ph / 1e6 / med
    return (med, float(min(ts)), float(max(ts)),
            {"plan_host_ms": round(float(ph[0]) / 1e3, 3), "wait_or_verify_ms": round(float(ph[1]) / 1e3, 3),
             "replay_host_ms": round(float(ph[2]) / 1e3, 3), "plan_frac": round(float(frac[0]), 3),
             "wait_or_verify_frac": round(float(frac[1]), 3), "replay_frac": round(float(frac[2]), 3),
             "host_cgroup": cg})


def _c3_corrupt(sets, commits, headers: int, gap: int, every: int):
    """Known-answer bad signatures for C3's direct leg (every > 0).  Header h verifies commit
    u = h + gap with Trusting(1/3) against set h and Light against set u; commit u is replaced by a
    copy with one flipped signature bit when u % every == 13 (at j = (u * 7919) % 175, anywhere) or
    u % every == 50 (at j = 170, past both loops' crossings).  The expected outcomes follow the
    reference loops at equal powers 10 (types/validator_set.go:722-765, 775-826): Light counts
    every signature in order and stops once 1170 > 1166 (indices 0..116); Trusting counts only
    signatures whose address set h holds (GetByAddress) and stops once 590 > 583 (the 59th such
    match).  A bad signature the loop reaches -> "wrong signature (#j)" (code 4, idx j); else ok.
    Returns (the direct leg's commits, {request index: (code, idx)} for every request)."""
    import tmed.types as T
    dcommits = list(commits)
    exp = {}
    for h in range(headers):
        u = h + gap
        j = None
        if every and u % every == 13:
            j = (u * 7919) % 175
        elif every and u % every == 50:
            j = 170
        if j is None:
            exp[2 * h] = exp[2 * h + 1] = (0, -1)
            continue
        pc = commits[u]
        c = T.PackedCommit(pc.height, pc.round, pc.block_id, pc.flags, pc.addresses, pc.ts_seconds, pc.ts_nanos,
                           pc.sigs.copy(), pc.sig_lens)
        c.sigs[j, 5] ^= 0x20
        dcommits[u] = c
        held = {v.address for v in sets[h].validators}
        matches = [i for i in range(pc.addresses.shape[0]) if pc.addresses[i].tobytes() in held]
        exp[2 * h] = (4, j) if j in matches[:59] else (0, -1)   # Trusting: reached among the first 59 matches
        exp[2 * h + 1] = (4, j) if j <= 116 else (0, -1)         # Light: reached before the crossing
    return dcommits, exp


def _c3_compiled_marshal(eng, sets, dcommits, headers: int, gap: int, runs: int, exp):
    """C3's direct call as the drop-in makes it: the headers' validator sets and commits held as Go
    objects (untimed), each call flattened by the shim's compiled marshal (shim/go_marshal.cpp: one C
    valset per *ValSet with its ValidatorsHash as set_hash, one C commit per *Commit, every set
    flattened anew — a new light-client batch) and then verified through tmed_verify_commits.
    Median marshal and seam seconds over `runs` calls; every outcome checked against `exp`."""
    import tmed.types as T
    from tmed import gomarshal as G
    heap = G.GoHeap()
    used = sorted({h for h in range(headers)} | {h + gap for h in range(headers)})
    si = {h: heap.valset(sets[h]) for h in used}
    ci = {h + gap: heap.commit(dcommits[h + gap]) for h in range(headers)}
    hashes = np.zeros((len(used), 32), np.uint8)
    for h in used:
        hs = getattr(sets[h], "set_hash", None)
        if hs is not None:
            hashes[si[h]] = np.frombuffer(bytes(hs), np.uint8)
    have_hash = all(getattr(sets[h], "set_hash", None) is not None for h in used)
    rows = []
    for h in range(headers):
        u = h + gap
        rows.append((T.MODE_LIGHT_TRUSTING, si[h], ci[u], 0, 1, 3))
        rows.append((T.MODE_LIGHT, si[u], ci[u], u + 1, 0, 0))
    a = np.array(rows, np.int64)
    m = G.Marshal()
    tm, ts, mism = [], [], 0
    for _ in range(runs):
        t0 = time.perf_counter()
        rq = m.requests(heap, a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4], a[:, 5], "test_chain_id",
                        set_hashes=hashes if have_hash else None, forget_sets=True)
        t1 = time.perf_counter()
        res = T.run_requests(eng, rq, len(rows))
        t2 = time.perf_counter()
        tm.append(t1 - t0)
        ts.append(t2 - t1)
        mism = sum(1 for q in range(len(rows))
                   if res[q].code != exp[q][0] or (exp[q][0] == 4 and res[q].idx != exp[q][1]))
    m.free()
    heap.free()
    return {"marshal_seconds_median": round(float(np.median(tm)), 5), "marshal_seconds_min": round(min(tm), 5),
            "seam_seconds_median": round(float(np.median(ts)), 5), "outcome_mismatches": mism,
            "threads": int(os.environ.get("TMED_HOST_THREADS", "16")),
            "note": "shim/go_marshal.cpp: %d requests on %d sets (flattened anew each call, ValidatorsHash as "
                    "set_hash) and %d commits held as Go objects" % (len(rows), len(used), headers)}


def c3(eng, headers: int, gap: int, policy: str = "cache", runs: int = 7, bisect_gap: int = 150,
       corrupt_every: int = 97):
    """Light client (BASELINE C3), two workloads over the same synthetic chain:
      direct:    each header h verified from trusted h - gap in one step (Trusting 1/3 + Light),
                 all headers in one seam call, timed `runs` times (median, spread, phase shares);
      bisection: each header h + bisect_gap from trusted h by light/client.go:706-773
                 verifySkipping — Trusting fails at this distance (the sets share fewer than 1/3
                 of their keys), the client pivots at 9/16 of the interval and retries; one seam
                 call per round over all headers' pending Verify calls, until every header is done.
    policy: "cache" (the sets carry no handle: the seam's key-set cache pools their keys — the
    drop-in as patched), "pool" (one explicit key set of every key, keyset_index per set) or
    "generic" (cache off).  With the cache the first direct call is cold (generic kernels, the keys
    queued) and the second builds the radix-2^12 combs: both are reported, untimed in the median.
    The request marshalling (PreparedBatch: flat arrays + C structs for every request, what the Go
    shim rebuilds per call) is timed beside the seam.  corrupt_every > 0: known-answer bad
    signatures in the direct leg's commits (_c3_corrupt), every request's code and index checked
    (outcome_mismatches).  Every failing Trusting of the bisection is checked for
    ErrNotEnoughVotingPowerSigned Got/Needed."""
    import tmed.types as T
    reach = max(gap, bisect_gap)
    eng.keycache_config(policy != "generic")
    sets, commits, ks, t_sign = _c3_world(eng, headers, reach, policy == "pool")
    res = {"metric": "light-client headers/s (VerifyCommitLightTrusting + VerifyCommitLight per header)",
           "unit": "headers/s", "host": _host_threads(),
           "config": {"workload": "C3: %d headers x 175 validators, trust 1/3, set changes 1 key/height" % headers,
                      "key_policy": policy, "sign_s": round(t_sign, 2), "timed_runs": runs,
                      "set_hash": ("each set's ValidatorSet.Hash() passed as the cache key (the light client's "
                                   "header.ValidatorsHash; the cache still compares the keys byte for byte)"
                                   if policy == "cache" else None)}}
    # ---- direct (gap) ----
    dcommits, exp = _c3_corrupt(sets, commits, headers, gap, corrupt_every)
    reqs = []
    for h in range(headers):
        u = h + gap
        reqs.append((T.MODE_LIGHT_TRUSTING, sets[h], "test_chain_id", None, 0, dcommits[u], 1, 3))
        reqs.append((T.MODE_LIGHT, sets[u], "test_chain_id", dcommits[u].block_id, u + 1, dcommits[u], 0, 0))
    tm = time.perf_counter()
    pb = T.PreparedBatch(reqs)
    t_marshal = time.perf_counter() - tm
    k0 = eng.keycache_stats()
    t0 = time.perf_counter()
    pb.run(eng)  # cold (cache: generic kernels, keys queued)
    t_cold = time.perf_counter() - t0
    eng.keycache_wait()
    t0 = time.perf_counter()
    pb.run(eng)  # warm-up (cache: first keyed call, radix-2^12 combs built)
    t_warm = time.perf_counter() - t0
    k1 = eng.keycache_stats()
    med, lo, hi, phases = _timed_runs(eng, pb, runs)
    k2 = eng.keycache_stats()
    codes = pb.codes()
    ver = int(pb.verified().sum())
    mism = sum(1 for q in range(len(reqs))
               if int(codes[q]) != exp[q][0] or (exp[q][0] == 4 and pb.res[q].idx != exp[q][1]))
    cm = _c3_compiled_marshal(eng, sets, dcommits, headers, gap, runs, exp) if hasattr(eng, "_h") else None
    res["value"] = round(headers / med, 1)
    res["direct"] = {"gap": gap, "headers_per_s": round(headers / med, 1), "verifies_per_s": round(ver / med, 1),
                     "seconds_median": round(med, 4), "seconds_min": round(lo, 4), "seconds_max": round(hi, 4),
                     "headers_per_s_incl_marshal": (round(headers / (med + cm["marshal_seconds_median"]), 1)
                                                    if cm else None),
                     "marshal_compiled": cm,
                     "headers_per_s_incl_python_marshal": round(headers / (med + t_marshal), 1),
                     "python_marshal_seconds": round(t_marshal, 4),
                     "verifies": ver, "outcomes_checked": corrupt_every > 0, "outcome_mismatches": mism,
                     "requests_failing_expected": sum(1 for e in exp.values() if e[0] != 0),
                     "all_ok": mism == 0, "phase_share": phases,
                     "cold_call_seconds": round(t_cold, 4), "second_call_seconds": round(t_warm, 4),
                     "keycache_cold_and_second": {k: k1[k] - k0[k] for k in ("keyed_sets", "generic_sets",
                                                                            "keys_appended", "keys_deferred")},
                     "keycache_timed": {k: k2[k] - k1[k] for k in ("lookups", "hits", "keyed_sets", "generic_sets",
                                                                  "keys_appended")},
                     "pool_keys": k2["pool_keys"]}
    # ---- bisection (verifySkipping) ----
    num, den = 9, 16  # light/client.go:31-32
    total = 175 * 10
    needed = total * 1 // 3
    st = [{"verified": h, "cache": [h + bisect_gap], "depth": 0, "done": False} for h in range(headers)]
    rounds, calls, ver_b, fails, bad_gn = 0, 0, 0, 0, 0
    t_seam = 0.0
    t0 = time.perf_counter()
    while True:
        act = [i for i in range(headers) if not st[i]["done"]]
        if not act:
            break
        reqs = []
        for i in act:
            v, c = st[i]["verified"], st[i]["cache"][st[i]["depth"]]
            reqs.append((T.MODE_LIGHT_TRUSTING, sets[v], "test_chain_id", None, 0, commits[c], 1, 3))
            reqs.append((T.MODE_LIGHT, sets[c], "test_chain_id", commits[c].block_id, c + 1, commits[c], 0, 0))
        pb = T.PreparedBatch(reqs)
        ts = time.perf_counter()
        pb.run(eng)
        t_seam += time.perf_counter() - ts
        rounds += 1
        calls += len(act)
        codes = pb.codes()
        vers = pb.verified()
        for j, i in enumerate(act):
            s_ = st[i]
            v, c = s_["verified"], s_["cache"][s_["depth"]]
            ct, cl = int(codes[2 * j]), int(codes[2 * j + 1])
            ver_b += int(vers[2 * j]) + (int(vers[2 * j + 1]) if ct == 0 else 0)
            if ct == 0 and cl == 0:                    # Verify ok
                if s_["depth"] == 0:
                    s_["done"] = True
                else:
                    s_["verified"] = c
                    s_["cache"] = s_["cache"][:s_["depth"]]
                    s_["depth"] = 0
            elif ct == 5:                              # ErrNewValSetCantBeTrusted
                fails += 1
                r = pb.res[2 * j]
                if r.got != (175 - (c - v)) * 10 or r.needed != needed:
                    bad_gn += 1
                if s_["depth"] == len(s_["cache"]) - 1:
                    pivot = v + (c - v) * num // den
                    s_["cache"] += [pivot, pivot]      # appended twice, as the reference does
                s_["depth"] += 1
            else:
                raise RuntimeError("header %d: verify %d -> %d failed (%d, %d)" % (i, v, c, ct, cl))
    wall = time.perf_counter() - t0
    # headers/s over the seam calls; the Python state machine and request packing of this
    # harness (the light client's own host work, Go in the reference) is reported beside it
    res["bisection"] = {"target_gap": bisect_gap, "headers_per_s": round(headers / t_seam, 1),
                        "seam_seconds": round(t_seam, 4), "harness_seconds": round(wall - t_seam, 4),
                        "rounds": rounds, "verify_calls": calls,
                        "trusting_failures": fails, "got_needed_mismatches": bad_gn, "verifies": ver_b,
                        "all_ok": bad_gn == 0 and fails > 0}
    if ks:
        eng.keyset_free(ks)
    eng.keycache_config(True)
    return res


def c3v(eng, headers: int, gap: int, policy: str = "cache", runs: int = 7):
    """The C3 direct workload through light.Verify itself (tmed_light_verify), over a chain whose
    headers are real: header u's ValidatorsHash / NextValidatorsHash are the hashes of sets u and
    u + 1 and commit u signs the block whose hash is Header.Hash(u).  Header h + gap is verified from
    trusted header h (trusted set: set h, as the c3 leg), all headers in one call.  Three legs over the
    same world, each timed `runs` times after a cold and a warm call (median):
      a  the c3 leg: tmed_verify_commits over Trusting + Light per header (no hashes);
      b  a plus a separate tmed_header_hashes call and a separate tmed_valset_hashes call over the same
         untrusted headers and sets: what a caller stitches light.Verify from without this call;
      v  tmed_light_verify: hashes, both commit checks and the replay in one call.
    b is the yardstick for v.  Outcomes of v are checked: every request OK, one header changed after
    signing -> COMMIT_HEADER_HASH, one wrong set -> VALS_HASH; a sample of header hashes against the
    oracle's restatement."""
    import tmed.light as L
    import tmed.types as T
    from oracle import merkle as OM
    from tmed.merkle import HeaderBatch, header_hashes, valset_hashes, valset_hashes_arrays
    from tmed.workload import make_valset, pubkeys_of, seeds_from_tag, sign_commits
    nv, nh = 175, headers + gap + 1
    eng.keycache_config(policy != "generic")
    pool_seeds = seeds_from_tag(b"tmed-c3-key", 0, nh + nv)
    pool_pubs = pubkeys_of(eng, pool_seeds)
    sets, orders = [], []
    for h in range(nh):
        vals, order = make_valset(pool_pubs[h:h + nv], [10] * nv)
        sets.append(vals)
        orders.append(order)
    hashes = valset_hashes(eng, sets)
    for vals, hsh in zip(sets, hashes):
        vals.set_hash = hsh
    chain = "test_chain_id"
    hdrs = [{"version_block": 11, "version_app": 0, "chain_id": chain, "height": h + 1, "time": (T2023 + h, 0),
             "last_block_id": (hashlib.sha256(b"c3v-prev-%d" % h).digest(), 1, hashlib.sha256(b"c3v-pp-%d" % h).digest()),
             "last_commit_hash": hashlib.sha256(b"c3v-lc-%d" % h).digest(), "data_hash": OM.empty_hash(),
             "validators_hash": hashes[h], "next_validators_hash": hashes[h + 1],
             "consensus_hash": hashlib.sha256(b"cons").digest(), "app_hash": hashlib.sha256(b"app-%d" % h).digest(),
             "last_results_hash": OM.empty_hash(), "evidence_hash": OM.empty_hash(),
             "proposer_address": sets[h].validators[0].address} for h in range(nh - 1)]
    hh = header_hashes(eng, hdrs)
    sample_ok = all(hh[h] == OM.header_hash(hdrs[h]) for h in range(0, nh - 1, max(1, (nh - 1) // 64)))
    specs = []
    for h in range(nh - 1):
        addrs = np.array([np.frombuffer(v.address, np.uint8) for v in sets[h].validators])
        bid = T.BlockID(hh[h], 1, hashlib.sha256(b"c3v-psh-%d" % h).digest())
        specs.append((pool_seeds[h:h + nv][orders[h]], addrs, h + 1, 0, bid, T2023 + h, None))
    t_sign = time.perf_counter()
    commits = sign_commits(eng, chain, specs)
    t_sign = time.perf_counter() - t_sign
    # known answers: one header changed after signing, one pair given the wrong set
    bad_hdr, bad_set = (headers // 3) + gap, (2 * headers // 3)
    hdrs_v = list(hdrs)
    hdrs_v[bad_hdr] = dict(hdrs[bad_hdr], app_hash=hashlib.sha256(b"changed").digest())
    now, period, drift = (T2023 + nh + 10, 0), 14 * 86400 * L.SECOND, 10 * L.SECOND
    pairs, reqs, exp = [], [], []
    for h in range(headers):
        u = h + gap
        uvals = sets[u + 1] if h == bad_set else sets[u]
        pairs.append(L.LightPair(hdrs[h], sets[h], hdrs_v[u], commits[u], uvals, period, now, drift, (1, 3)))
        exp.append(L.COMMIT_HEADER_HASH if u == bad_hdr else L.VALS_HASH if h == bad_set else L.OK)
        reqs.append((T.MODE_LIGHT_TRUSTING, sets[h], chain, None, 0, commits[u], 1, 3))
        reqs.append((T.MODE_LIGHT, sets[u], chain, commits[u].block_id, u + 1, commits[u], 0, 0))
    pb, pl = T.PreparedBatch(reqs), L.PreparedLight(pairs)
    hb = HeaderBatch([hdrs_v[h + gap] for h in range(headers)])
    upk = np.concatenate([sets[h + gap].packed()[0][:nv] for h in range(headers)])
    upw = np.concatenate([sets[h + gap].packed()[1][:nv] for h in range(headers)])
    uoff = (np.arange(headers + 1) * nv).astype(np.uint32)

    class _Stitched:  # leg b as one timed unit
        def run(self, e):
            pb.run(e)
            hb.run(e)
            valset_hashes_arrays(e, upk, upw, uoff)

    res = {"metric": "light-client headers/s through light.Verify (tmed_light_verify)", "unit": "headers/s",
           "host": _host_threads(),
           "config": {"workload": "C3v: %d headers x 175 validators, real headers, trust 1/3, gap %d" % (headers, gap),
                      "key_policy": policy, "sign_s": round(t_sign, 2), "timed_runs": runs}}
    legs = {}
    for name, unit in (("a_verify_commits", pb), ("b_verify_commits_plus_hash_calls", _Stitched()), ("v_light_verify", pl)):
        unit.run(eng)  # cold
        eng.keycache_wait()
        unit.run(eng)  # warm
        med, lo, hi, phases = _timed_runs(eng, unit, runs)
        legs[name] = {"headers_per_s": round(headers / med, 1), "seconds_median": round(med, 5),
                      "seconds_min": round(lo, 5), "seconds_max": round(hi, 5)}
    codes = pl.codes()
    mism = int(sum(1 for q in range(headers) if int(codes[q]) != exp[q]))
    a_ok = int((pb.codes() != 0).sum()) == 0
    res["value"] = legs["v_light_verify"]["headers_per_s"]
    res["legs"] = legs
    res["v_over_b"] = round(legs["v_light_verify"]["headers_per_s"] /
                            legs["b_verify_commits_plus_hash_calls"]["headers_per_s"], 3)
    res["outcome_mismatches"] = mism
    res["header_hash_sample_ok"] = bool(sample_ok)
    res["all_ok"] = mism == 0 and a_ok and bool(sample_ok)
    eng.keycache_config(True)
    return res


def _c4_corrupt(commits, b0: int, every: int, upto: int):
    """Known-answer corruption of a generated C4 window (every > 0): block b with b % every == 13
    gets one flipped bit in the signature at index j = (b * 7919) % upto, before the 2/3 crossing
    -> VerifyCommitLight must return "wrong signature (#j)" after verifying j + 1 signatures; block b
    with b % every == 50 gets a flipped signature at index upto, past the crossing -> still ok, with
    upto signatures verified (types/validator_set.go:740-761: the loop never reaches it).  Returns
    the expected (code, idx, verified) per block."""
    exp = []
    for k, c in enumerate(commits):
        b = b0 + k
        if every and b % every == 13:
            j = (b * 7919) % upto
            c.sigs[j, 5] ^= 0x20
            exp.append((4, j, j + 1))
        else:
            if every and b % every == 50 and upto < c.sigs.shape[0]:
                c.sigs[upto, 40] ^= 0x01
            exp.append((0, -1, upto))
    return exp


STREAM_CHUNK_WINDOWS = 13  # C4 stream mode: windows generated (pinned) at once: 13 x 1000 blocks x 10k x 64 B = 8.3 GB per rank
OVERLAP_RING = 3  # C4 overlapped pass: Go-object windows held per rank (~1.6 GB each)


def c4(eng, blocks: int, nvals: int, rank: int, world: int, dev, window: int, batch: int, corrupt_every: int = 0,
       pregen: bool = False, pinned: bool = True, policy: str = "cache", stream: bool = True,
       marshal: str = "compiled"):
    """Blocksync replay (BASELINE C4): VerifyCommitLight for every block of a contiguous shard
    of the chain per rank, through the pipelined blocksync seam (tmed_blocksync_verify, f4),
    key-cached.  Blocks are generated window by window on the GPU (untimed) and verified
    from host memory, as the reactor holds them; only the verification is timed.  Ranks
    all-reduce int64 tallies and all-gather the per-block decision bitmap.
    corrupt_every > 0: known-answer bad signatures in some blocks (_c4_corrupt); every block's
    outcome (code, error index, signatures verified) is checked against the expected one.
    pregen: generate every window of the shard before the timed part and start the ranks' timed
    parts together (the host rehearsal: no rank's generation competes with another's seam).
    pinned: the commits' signatures are marshalled into page-locked arenas (tmed.PinnedBuffer, one
    per window held at once), as a Go shim that flattens its commits into tmed_host_alloc memory
    would: the seam then DMAs them straight to the device.  The marshalling is timed beside the
    seam (value_incl_marshal): marshal "compiled" — the window's commits built as Go objects
    (types.Commit / []CommitSig, untimed) and flattened by the shim's compiled marshal
    (shim/go_marshal.cpp: C structs, signatures into the arena, each Light commit up to its 2/3
    crossing), what the drop-in pays; "python" — the harness's own numpy marshal (BlocksyncWindow).
    policy: "cache" — the set carries no handle and the seam's key-set cache builds its keys (the
    first, untimed window runs generic and queues them; the drop-in as patched); "explicit" — a
    tmed_keyset_load handle (the round-3 harness)."""
    import torch
    import torch.distributed as dist
    import tmed.types as T
    from tmed import PinnedBuffer, TmedError
    from tmed.dist import aggregate_blocksync, block_range, overlapped_figures
    if stream:
        pregen = True  # every window exists before the timed stream starts (nothing generated inside it)
    from tmed.launch import gpu_count_fields
    from tmed.workload import make_valset, pubkeys_of, seeds_from_tag, sign_commits
    seeds = seeds_from_tag(b"tmed-c4-key", 0, nvals)
    pubs = pubkeys_of(eng, seeds)
    vals, order = make_valset(pubs, [10] * nvals)
    t_ks = time.perf_counter()
    if policy == "explicit":
        vals.keyset = eng.keyset_load(np.array([np.frombuffer(v.pub_key, np.uint8) for v in vals.validators]))
    t_ks = time.perf_counter() - t_ks
    kc0 = eng.keycache_stats()
    addrs = np.array([np.frombuffer(v.address, np.uint8) for v in vals.validators])
    lo, hi = block_range(blocks, rank, world)                       # contiguous shard of heights
    upto = nvals * 2 // 3 + 1                                       # Light stops after this many (equal powers)
    ok_bits = np.zeros(hi - lo, np.uint8)
    ver = 0
    dt = t_gen = t_marshal = 0.0
    mism = 0
    phase = np.zeros(3)
    from tmed.types import seam_phase_us
    if world > 1:
        dist.barrier()
    arenas = []

    pinned_failed = []

    class _Pageable:  # the fallback when page-locked memory runs out (e.g. 8 ranks x 8.3 GB on one node)
        def __init__(self, nbytes):
            self.buf = np.empty(nbytes, np.uint8)
            self.ptr = self.buf.ctypes.data

        def array(self, shape, dtype):
            return self.buf.view(dtype)[:int(np.prod(shape))].reshape(shape)

        def free(self):
            self.buf = None

    from tmed import gomarshal as G

    class _CompiledWindow:
        """A window marshalled by the compiled shim (shim/go_marshal.cpp) from commits laid out as
        Go holds them; run / submit / codes / verified / res as T.BlocksyncWindow's."""

        def __init__(self, m, wptr, n, go=None):
            self.m, self.w, self.n = m, wptr, n
            self.res = G.results(n)
            self.go = go  # (heap, set, commits, heights, arena pointer): marshalled on demand

        def marshal(self):
            """The shim's flatten of the window's Go objects (timed by the caller)."""
            heap, si, ci, hts, arena = self.go
            self.w = self.m.window(heap, si, ci, hts, "test_chain_id", sig_arena=arena)

        def run(self, e, batch_blocks=0):
            rc = T._bind().tmed_blocksync_verify(e._h, self.w, batch_blocks, self.res)
            if rc != 0:
                raise TmedError(rc, "tmed_blocksync_verify")

        def submit(self, e, batch_blocks=0):
            rc = T._bind().tmed_blocksync_submit(e._h, self.w, batch_blocks, self.res)
            if rc != 0:
                raise TmedError(rc, "tmed_blocksync_submit")

        def codes(self):
            return np.array([self.res[h].code for h in range(self.n)], np.int32)

        def verified(self):
            return np.array([self.res[h].verified for h in range(self.n)], np.int64)

    marshals = []  # one shim context per window held at once (a window in flight keeps its arrays)
    # the overlapped pass (every rank): the windows of a chunk flattened again from a RING of the Go
    # objects of its first OVERLAP_RING windows (~1.6 GB each), so the Go memory per rank stays bounded
    # (3 windows, not 13) and an 8-rank node holds 8 x 4.8 GB, not 8 x 21 GB
    overlap = marshal == "compiled" and stream and pregen
    ring = []  # (go tuple, expected outcomes, blocks) of the chunk's first OVERLAP_RING windows

    def to_arena(commits, k):
        if k == len(arenas):
            try:
                arenas.append(PinnedBuffer(window * nvals * 64))
            except TmedError:  # the seam stages pageable signatures itself: slower, same decisions
                pinned_failed.append(k)
                arenas.append(_Pageable(window * nvals * 64))
        a = arenas[k].array((window * nvals, 64), np.uint8)
        o = 0
        for c in commits:
            n = c.sigs.shape[0]
            a[o:o + n] = c.sigs
            c.sigs = a[o:o + n]
            o += n

    def gen(w0, w1, k=0):
        nonlocal t_marshal
        specs = [(seeds[order], addrs, b + 1, 0, block_id(b"c4-%d" % (b + 1)), T2023 + b, None) for b in range(w0, w1)]
        commits = sign_commits(eng, "test_chain_id", specs, sign_upto=upto)
        exp = _c4_corrupt(commits, w0, corrupt_every, upto)
        if marshal == "compiled":
            # the window as the reactor holds it (Go objects, untimed), then the shim's flatten (timed)
            heap = G.GoHeap()
            si = heap.valset(vals)
            ci = np.array([heap.commit(c) for c in commits], np.int64)
            if k == len(marshals):
                marshals.append(G.Marshal())
            if pinned and k == len(arenas):
                try:
                    arenas.append(PinnedBuffer(window * nvals * 64))
                except TmedError:
                    pinned_failed.append(k)
                    arenas.append(_Pageable(window * nvals * 64))
            cw = _CompiledWindow(marshals[k], None, len(commits),
                                 (heap, si, ci, [c.height for c in commits], arenas[k].ptr if pinned else None))
            if overlap:
                # a first flatten, untimed: a reactor reuses its contexts, so the timed flattens below
                # and in the overlapped pass measure the steady state, not each context's first touch
                cw.marshal()
            tm = time.perf_counter()
            cw.marshal()  # the flatten the stream pass verifies (value_incl_marshal: the serial sum)
            t_marshal += time.perf_counter() - tm
            if overlap and k < OVERLAP_RING:
                ring.append((cw.go, exp, len(commits)))
            else:
                heap.free()
            cw.go = None
            return cw, exp, None
        tm = time.perf_counter()
        if pinned:
            to_arena(commits, k)
        win = T.BlocksyncWindow(vals, "test_chain_id", [c.block_id for c in commits], [c.height for c in commits],
                                commits)
        t_marshal += time.perf_counter() - tm
        return win, exp, commits

    def check(w0, w1, win, exp, record=True):
        """(verifies, outcome mismatches) of a collected window; its ok bits into ok_bits (record)"""
        codes, vers = win.codes(), win.verified()
        if record:
            ok_bits[w0 - lo:w1 - lo] = codes == 0
        bad = 0
        for h, (ec, ei, ev) in enumerate(exp):
            if codes[h] != ec or vers[h] != ev or (ec == 4 and win.res[h].idx != ei):
                bad += 1
        return int(vers.sum()), bad

    def run(w0, w1, win, exp):
        nonlocal dt, phase, ver, mism
        t0 = time.perf_counter()
        win.run(eng, batch)
        dt += time.perf_counter() - t0
        phase += np.asarray(seam_phase_us(), np.float64)
        v, m = check(w0, w1, win, exp)
        ver += v
        mism += m

    sync_pass = [0.0, 0, 0]  # the per-window calls of stream mode: seconds, verifies, mismatches
    ov_pass = [0.0, 0, 0, 0.0]  # the stream with the shim's flattens beside it (+ their summed seconds)

    def overlapped_pass(wins):
        """The drop-in's pipeline: each window flattened by the shim right before
        its submit, on a producer thread (the ctypes calls release the GIL), as a reactor's marshalling
        goroutine would beside the one that submits (tmed_blocksync_submit blocks while the device frees
        pipeline slots, so a flatten on the submitting thread would not overlap).  Window i is flattened
        from ring slot i % OVERLAP_RING (the Go objects of one of the chunk's first windows: same shape,
        same cost) into its own shim context and pinned arena, after the stream pass has used them; its
        outcomes are checked against that slot's known answers.  Timed from the first flatten to the
        wait, the flattens summed beside it."""
        import threading
        ows = []
        for i, (w0, w1, win, exp, _) in enumerate(wins):
            go, sexp, n = ring[i % len(ring)]
            ows.append((_CompiledWindow(marshals[i], None, n, go[:4] + (arenas[i].ptr if pinned else None,)), sexp))
        ready = [threading.Event() for _ in ows]
        tmar = [0.0] * len(ows)
        perr = []

        def producer():
            try:
                for i, (ow, _) in enumerate(ows):
                    tq = time.perf_counter()
                    ow.marshal()
                    tmar[i] = time.perf_counter() - tq
                    ready[i].set()
            except BaseException as e:  # wake the submitting thread; it re-raises
                perr.append(e)
                for ev in ready:
                    ev.set()

        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        th = threading.Thread(target=producer)
        th.start()
        try:
            for i, (ow, _) in enumerate(ows):
                ready[i].wait()
                if perr:
                    break
                ow.submit(eng, batch)
            T.blocksync_wait(eng)
        finally:
            th.join()  # the producer writes into the shim contexts: never leave it running
        if perr:
            raise perr[0]
        ov_pass[0] += time.perf_counter() - t0
        ov_pass[3] += sum(tmar)
        for ow, sexp in ows:
            v, m = check(0, 0, ow, sexp, record=False)
            ov_pass[1] += v
            ov_pass[2] += m

    if pregen:  # the windows generated first (in chunks of STREAM_CHUNK_WINDOWS), then all ranks verify together
        starts = list(range(lo, hi, window))
        chunk_w = STREAM_CHUNK_WINDOWS if stream else max(1, len(starts))
        first = True
        for c0 in range(0, len(starts), chunk_w):
            wins = []
            tg = time.perf_counter()
            for k, w0 in enumerate(starts[c0:c0 + chunk_w]):
                w1 = min(hi, w0 + window)
                wins.append((w0, w1) + gen(w0, w1, k))
            t_gen += time.perf_counter() - tg
            if world > 1:
                dist.barrier()
            for _ in range(2 if first else 0):  # untimed warmup (see below)
                wins[0][2].run(eng, batch)
                eng.keycache_wait()
            first = False
            if not stream:
                for w0, w1, win, exp, _ in wins:  # a call per window (tmed_blocksync_verify)
                    run(w0, w1, win, exp)
                del wins
                continue
            # a call per window first (reported beside), then the same windows as ONE stream
            # (tmed_blocksync_submit each, then tmed_blocksync_wait): the device is not drained
            # between windows; timed from the first submit to the wait
            for w0, w1, win, exp, _ in wins:
                t0 = time.perf_counter()
                win.run(eng, batch)
                sync_pass[0] += time.perf_counter() - t0
                v, m = check(w0, w1, win, exp)
                sync_pass[1] += v
                sync_pass[2] += m
                win.res = type(win.res)()  # fresh results for the stream
            if world > 1:
                dist.barrier()
            t0 = time.perf_counter()
            for w0, w1, win, exp, _ in wins:
                win.submit(eng, batch)
                phase += np.asarray(seam_phase_us(), np.float64)
            T.blocksync_wait(eng)
            phase += np.asarray(seam_phase_us(), np.float64)
            dt += time.perf_counter() - t0
            for w0, w1, win, exp, _ in wins:
                v, m = check(w0, w1, win, exp)
                ver += v
                mism += m
            if overlap:
                overlapped_pass(wins)
            for go, _, _ in ring:
                go[0].free()
            ring.clear()
            del wins
    else:
        for w0 in range(lo, hi, window):
            w1 = min(hi, w0 + window)
            tg = time.perf_counter()
            win, exp, commits = gen(w0, w1)
            t_gen += time.perf_counter() - tg
            if w0 == lo:
                # untimed warmup: first-use buffers and events of the seam; with the key-set cache the
                # first call runs generic and queues the keys, the second builds the radix-2^12 combs
                for _ in range(2):
                    win.run(eng, batch)
                    eng.keycache_wait()
            run(w0, w1, win, exp)
            del win, commits
    nbatch = -(-(hi - lo) // batch) if batch else 0
    sdt, sver, smism = sync_pass
    odt, over, omism, omar = ov_pass
    from tmed.launch import BINDING
    mine = [BINDING.get("numa_node", -1), BINDING.get("cpus", 0), int(os.environ.get("TMED_HOST_THREADS", "16")),
            len(arenas) - len(pinned_failed) if pinned else 0, len(pinned_failed) if pinned else len(arenas),
            odt, over, omism]
    agg = aggregate_blocksync(ok_bits, blocks, rank, world, ver, mism + smism + omism, dt,
                              extra_max=[t_marshal, sdt, odt, omar],
                              phases=list(phase) + [nbatch], device=dev, per_rank=mine)
    ov_value, ov_each = overlapped_figures(agg["per_rank"], 5, 6)
    ranks = [{"rank": r, "numa_node": int(p[0]), "cpus": int(p[1]), "host_threads": int(p[2]),
              "pinned_arenas": int(p[3]), "pageable_arenas": int(p[4]),
              "value_incl_marshal_overlapped": ov_each[r], "overlapped_seconds": round(p[5], 4),
              "overlapped_mismatches": int(p[7])}
             for r, p in enumerate(agg["per_rank"])]
    n_pageable = sum(x["pageable_arenas"] for x in ranks)
    n_arenas = sum(x["pinned_arenas"] + x["pageable_arenas"] for x in ranks)
    ok, nb, ver, mism, dt = agg["blocks_ok"], agg["blocks"], agg["verified"], agg["mismatches"], agg["seconds"]
    t_marshal_max, sdt_max, odt_max, omar_max = agg["extra_max"]
    ph_all = [p[:3] + [p[4], p[3]] for p in agg["phases"]]  # plan, wait, replay, seconds, batches
    kc1 = eng.keycache_stats()
    if vals.keyset:
        eng.keyset_free(vals.keyset)
    for a in arenas:
        a.free()
    for m in marshals:
        m.free()
    n_bad = sum(1 for b in range(lo, hi) if corrupt_every and b % corrupt_every == 13)
    return {"metric": "blocksync replay verifies/s (VerifyCommitLight per block)", "value": round(ver / dt, 1),
            "unit": "verifies/s", "blocks_per_s": round(nb / dt, 1), "blocks": nb,
            "value_incl_marshal": round(ver / (dt + t_marshal_max), 1),
            "value_incl_marshal_overlapped": ov_value,
            "overlapped_note": ("every rank: its windows as one stream, each flattened by the shim on a producer "
                                "thread and submitted (tmed_blocksync_submit) as soon as it is ready, so the "
                                "flatten of window k+1 runs while window k is submitted and verified; first "
                                "flatten to tmed_blocksync_wait, all ranks' verifies / the slowest rank's time "
                                "(config.ranks[] per rank). Window k is flattened from the Go objects of window "
                                "k mod %d of its chunk (a ring bounding the Go memory per rank) and checked "
                                "against that window's known answers; outcome mismatches counted with the "
                                "stream's. Every shim context is flattened once, untimed, first (a reactor "
                                "reuses its contexts); marshal_seconds_max_rank is the serial flattens' sum, "
                                "marshal_seconds_overlapped_pass the overlapped pass's flattens summed" % OVERLAP_RING
                                if odt_max > 0 else None),
            "marshal_seconds_max_rank": round(t_marshal_max, 4),
            "marshal_seconds_overlapped_pass": (round(omar_max, 4) if odt_max > 0 else None),
            "marshal_note": ("compiled shim marshal (shim/go_marshal.cpp, %s threads): each window's commits held "
                             "as Go objects (80-B CommitSig structs, per-signature heap slices) flattened into the C "
                             "structs and the pinned arena, each Light commit up to its 2/3 crossing; timed per "
                             "window; value_incl_marshal adds their serial sum to the seam's time" % os.environ.get("TMED_HOST_THREADS", "16")
                             if marshal == "compiled" else
                             "Python harness: the signature arena fill + the window's C structs (BlocksyncWindow)"),
            "key_policy": policy,
            "windows": ("one stream: tmed_blocksync_submit per window, tmed_blocksync_wait at the end (the "
                        "device is not drained between windows), in chunks of %d windows generated beforehand"
                        % STREAM_CHUNK_WINDOWS if stream else "a tmed_blocksync_verify call per window"),
            "per_window_calls": ({"value": round(ver / sdt_max, 1), "seconds": round(sdt_max, 4),
                                  "note": "the same windows, a tmed_blocksync_verify call each (pipeline drained and "
                                          "refilled at every window); outcome mismatches counted with the stream's"}
                                 if stream else None),
            "keycache_rank0": {k: kc1[k] - kc0[k] for k in ("lookups", "hits", "keyed_sets", "generic_sets",
                                                            "keys_appended", "keys_deferred")},
            "all_ok": ok == nb if not corrupt_every else None,
            "blocks_ok": ok, "blocks_with_bad_signature": n_bad if world == 1 else None,
            "outcome_mismatches": mism, "outcomes_checked": corrupt_every > 0,
            "host_phase_ms_rank0": {"plan_and_staging": round(phase[0] / 1e3, 2),
                                    "enqueue_and_wait_for_device": round(phase[1] / 1e3, 2),
                                    "replay": round(phase[2] / 1e3, 2)},
            "host_phase_per_batch_ms": [{"rank": r, "plan_and_staging": round(p[0] / 1e3 / max(1, p[4]), 3),
                                         "enqueue_and_wait_for_device": round(p[1] / 1e3 / max(1, p[4]), 3),
                                         "replay": round(p[2] / 1e3 / max(1, p[4]), 3),
                                         "batches": int(p[4]), "seconds": round(p[3], 3)} for r, p in enumerate(ph_all)],
            "verifies": ver, "seconds": round(dt, 4), **gpu_count_fields(world),
            "config": {"workload": "C4: %d blocks x %d validators, VerifyCommitLight per block, key-cached, "
                                   "blocks sharded over %d GPU(s) (contiguous heights), %d-block windows, "
                                   "%d-block device batches" % (blocks, nvals, world, window, batch),
                       "signed_per_commit": upto,
                       "warmup": "the first window verified twice untimed (first-use buffers of the seam; the "
                                 "key-set cache's generic first call and its key build)",
                       "commit_memory": ("pageable: signatures through the seam's staging copy" if not pinned
                                         else "pinned arenas (tmed_host_alloc) on every rank: signatures DMA'd "
                                              "from them" if n_pageable == 0
                                         else "MIXED: %d of %d arenas over %d rank(s) pageable (tmed_host_alloc "
                                              "failed; those windows go through the seam's staging copy, a slower "
                                              "path): see ranks[]" % (n_pageable, n_arenas, world)),
                       "ranks": ranks,
                       "unsigned_note": "validators past the 2/3 crossing carry random (invalid) signatures "
                                        "the Light loop never reaches",
                       "keyset_build_s": round(t_ks, 3), "generate_s": round(t_gen, 2)}}


def mt(eng, runs: int, shapes=((1000, 10_000), (10_000, 175))):
    """MedianTime of every commit of a window against the window's validator set, per shape
    (commits, validators): one tmed_median_times call (each commit staged once, the set once), the
    same PreparedMedian through tmed_median_times_host (one thread, GetByAddress as a hash lookup,
    a weighted quickselect), and tmed_verify_commits in TMED_MODE_COMMIT over the same commits (all
    signatures valid; warmed, so the key-set cache holds the set).  Votes are stamped base + i ms
    for validator i, powers are 1 + (i mod 100).  Medians of `runs` timed calls."""
    import tmed.state as S
    import tmed.types as T
    from tmed.workload import make_valset, pubkeys_of, seeds_from_tag, sign_commits
    med = lambda xs: float(np.median(xs))
    out = []
    for blocks, nvals in shapes:
        seeds = seeds_from_tag(b"tmed-mt-key", 0, nvals)
        pubs = pubkeys_of(eng, seeds)
        vals, order = make_valset(pubs, [1 + i % 100 for i in range(nvals)])
        addrs = np.array([np.frombuffer(v.address, np.uint8) for v in vals.validators])
        commits = []
        step = max(1, 2_500_000 // nvals)  # signatures per signing call
        for b0 in range(0, blocks, step):
            specs = [(seeds[order], addrs, b + 1, 0, block_id(b"mt-%d" % (b + 1)), T2023 + b, None)
                     for b in range(b0, min(blocks, b0 + step))]
            commits += sign_commits(eng, "test_chain_id", specs)
        print("mt: %d commits x %d validators generated" % (blocks, nvals), file=sys.stderr, flush=True)
        pm = S.PreparedMedian([(c, vals) for c in commits])
        pm.run(eng)  # warm: the staging buffers are allocated
        wall, dev = [], []
        for _ in range(runs):
            t0 = time.perf_counter()
            pm.run(eng)
            wall.append(time.perf_counter() - t0)
            dev.append(eng.last_kernel_ms())
        got, on_device = pm.results(), int(pm.on_device().sum())
        host = []
        for _ in range(min(runs, 3)):
            t0 = time.perf_counter()
            pm.run(None)
            host.append(time.perf_counter() - t0)
        same = pm.results() == got
        pb = T.PreparedBatch([(T.MODE_COMMIT, vals, "test_chain_id", c.block_id, c.height, c, 0, 0) for c in commits])
        for _ in range(2):  # the first call builds the set's keys, the second is keyed
            pb.run(eng)
        eng.keycache_wait()
        ver, ver_dev = [], []
        for _ in range(min(runs, 3)):
            t0 = time.perf_counter()
            pb.run(eng)
            ver.append(time.perf_counter() - t0)
            ver_dev.append(eng.last_kernel_ms())
        out.append({"commits": blocks, "validators": nvals, "pairs_on_device": on_device,
                    "device_equals_host": bool(same), "all_ok": all(r[0] == 0 for r in got),
                    "median_call_ms": round(med(wall) * 1e3, 3), "median_calls_per_s": round(1.0 / med(wall), 2),
                    "median_commits_per_s": round(blocks / med(wall), 1),
                    "median_kernel_ms": round(med(dev), 4), "median_kernel_us_per_commit": round(med(dev) * 1e3 / blocks, 3),
                    "host_1thread_ms": round(med(host) * 1e3, 3), "host_us_per_commit": round(med(host) * 1e6 / blocks, 3),
                    "verify_commits_ms": round(med(ver) * 1e3, 3), "verify_commits_last_kernel_ms": round(med(ver_dev), 4),
                    "verify_commits_all_ok": bool((pb.codes() == 0).all())})
    return {"config": "mt", "metric": "state.MedianTime per window, device vs host vs VerifyCommit", "runs": runs, "shapes": out}


def vb(eng, runs: int, shapes=("1000x10000", "10000x175"), route: str = "both"):
    """validateBlock over a linked window per shape BxV (blocks x validators, one constant set, equal
    powers, every signature valid, two transactions a block, no evidence): the chain is built block by
    block (block h's LastCommit signs Header.Hash of block h - 1, its time is that commit's median), then
    `runs` rounds of one fused tmed_validate_blocks call followed by the composed route over the same
    C structs, each route's Python packing outside the timing.  Outcomes are compared request by request."""
    import tmed.evidence as E
    import tmed.merkle as MK
    import tmed.state as S
    import tmed.types as T
    from tmed.workload import make_valset, pubkeys_of, seeds_from_tag, sign_commits
    med = lambda xs: float(np.median(xs))
    chain = "test_chain_id"
    out = []
    eng.keycache_config(True)
    for shape in shapes:
        blocks, nvals = (int(x) for x in shape.split("x"))
        seeds = seeds_from_tag(b"tmed-vb-key", 0, nvals)
        pubs = pubkeys_of(eng, seeds)
        vals, order = make_valset(pubs, [10] * nvals)
        addrs = np.array([np.frombuffer(v.address, np.uint8) for v in vals.validators])
        vhash = MK.valset_hashes(eng, [vals])[0]
        cons = hashlib.sha256(b"consensus-params").digest()
        t_gen = time.perf_counter()
        reqs, commits, headers = [], [], []
        last_commit, last_id, last_time = T.Commit(0, 0, T.BlockID(), []), T.BlockID(), (T2023, 0)
        st0 = S.BlockState(11, 0, chain, 1, 0, T.BlockID(), last_time, b"", cons, b"", vals, vals, vals, 1 << 20)
        offset = None
        for b in range(blocks + 1):  # block 0 is the initial block: the window is blocks 1 .. B
            height = b + 1
            txs = [b"tx-%d-a" % height, b"tx-%d-bb" % height]
            if b == 0:
                t = last_time
            else:
                if offset is None:  # the commit's median behind its base second, the same for every block
                    code, mt_ = S.median_times(None, [(last_commit, vals)])[0]
                    offset = (mt_[0] - int(last_commit.ts_seconds[0]), mt_[1])
                t = (int(last_commit.ts_seconds[0]) + offset[0], offset[1])
            ch = MK.commit_hashes(eng, [last_commit])[0]
            hdr = {"version_block": 11, "version_app": 0, "chain_id": chain, "height": height, "time": t,
                   "last_block_id": (last_id.hash, last_id.psh_total, last_id.psh_hash), "last_commit_hash": ch,
                   "data_hash": MK.txs_hashes(eng, [txs])[0], "validators_hash": vhash, "next_validators_hash": vhash,
                   "consensus_hash": cons, "app_hash": b"", "last_results_hash": b"",
                   "evidence_hash": hashlib.sha256(b"").digest(), "proposer_address": vals.validators[b % nvals].address}
            st = st0 if b < 2 else dataclasses.replace(st0, last_block_height=-1, last_block_time=(1, 1),
                                                       last_block_id=T.BlockID(b"", 1, last_id.psh_hash))
            if b == 1:
                st = dataclasses.replace(st0, last_block_height=1, last_block_id=last_id, last_block_time=last_time)
            if b >= 1:
                reqs.append((S.Block(hdr, last_commit, txs), st, b >= 2))
                commits.append(last_commit)
                headers.append(hdr)
            bid = T.BlockID(MK.header_hashes(eng, [hdr])[0], 1, hashlib.sha256(b"parts-%d" % height).digest())
            last_commit = sign_commits(eng, chain, [(seeds[order], addrs, height, 0, bid, T2023 + 10 * height, None)])[0]
            last_id, last_time = bid, t
        t_gen = time.perf_counter() - t_gen
        print("vb: %d blocks x %d validators generated in %.1fs" % (blocks, nvals, t_gen), file=sys.stderr, flush=True)
        pb = S.PreparedBlocks(reqs)
        # the composed route's calls over the same objects, packed once
        chb = MK.CommitHashBatch(commits)
        hb = MK.HeaderBatch(headers)
        pm = S.PreparedMedian([(c, vals) for c in commits])
        bids = [T.BlockID(bytes(h["last_block_id"][0]), h["last_block_id"][1], h["last_block_id"][2]) for h in headers]
        pv = T.PreparedBatch([(T.MODE_COMMIT, vals, chain, bids[i], headers[i]["height"] - 1, commits[i], 0, 0)
                              for i in range(blocks)])
        want = {k: np.array([np.frombuffer(h[k], np.uint8) for h in headers]) for k in
                ("last_commit_hash", "data_hash", "evidence_hash", "validators_hash", "next_validators_hash")}
        link_want = np.array([np.frombuffer(h["last_block_id"][0], np.uint8) for h in headers])
        times = np.array([h["time"] for h in headers], np.int64)
        items, list_off = np.zeros(0, np.int64), np.zeros(blocks + 1, np.uint32)

        prop_keys = [h["proposer_address"] for h in headers]
        split = {"calls": 0.0, "host": 0.0}

        def composed():
            """-> codes (the checks the window can fail: the hashes, the link, the commit, the proposer, the time).
            The seven calls and the host part (the proposer lookup and the compares) are timed apart."""
            t0 = time.perf_counter()
            cho, _ = chb.run(eng)
            dh = MK.txs_hashes_packed(eng, pb.txs, pb.tx_off, pb.block_off)
            _, eh, _, _ = E.evidence_hashes_packed(eng, [], items, list_off)
            hh_list = hb.run(eng)
            vh_bytes = MK.valset_hashes(eng, [vals])[0]
            pm.run(eng)
            pv.run(eng)
            t1 = time.perf_counter()
            code = np.zeros(blocks, np.int32)
            first = lambda bad, c: np.where((code == 0) & bad, c, code)
            hh = np.frombuffer(b"".join(hh_list), np.uint8).reshape(blocks, 32)
            vh = np.frombuffer(vh_bytes, np.uint8)
            code = first((cho != want["last_commit_hash"]).any(1), S.VB_LAST_COMMIT_HASH)
            code = first((dh != want["data_hash"]).any(1), S.VB_DATA_HASH)
            code = first((eh != want["evidence_hash"]).any(1), S.VB_EVIDENCE_HASH)
            link = np.zeros(blocks, bool)
            link[1:] = (hh[:-1] != link_want[1:]).any(1)
            code = first(link, S.VB_LAST_BLOCK_ID)
            code = first((vh != want["validators_hash"]).any(1), S.VB_VALIDATORS_HASH)
            code = first((vh != want["next_validators_hash"]).any(1), S.VB_NEXT_VALIDATORS_HASH)
            code = first(pv.codes() != 0, S.VB_LAST_COMMIT)
            index = {}  # HasAddress: one address index of the set per call, one lookup per block
            for i, v in enumerate(vals.validators):
                index.setdefault(v.address, i)
            found = np.array([k in index for k in prop_keys])
            code = first(~found, S.VB_PROPOSER_UNKNOWN)
            mtimes = np.array([r[1] for r in pm.results()], np.int64)
            code = first((mtimes != times).any(1), S.VB_TIME_NOT_MEDIAN)
            split["calls"], split["host"] = t1 - t0, time.perf_counter() - t1
            return code

        do_f, do_c = route in ("both", "fused"), route in ("both", "composed")  # one route alone: for a profiler
        for _ in range(2):  # warm: buffers, and the key-set cache builds the set's keys between the rounds
            if do_f:
                pb.run(eng)
            if do_c:
                composed()
            eng.keycache_wait()
        fused, comp, kern, calls, host = [], [], [], [], []
        mismatches = 0
        for _ in range(runs):  # alternated in one session
            if do_f:
                t0 = time.perf_counter()
                pb.run(eng)
                fused.append(time.perf_counter() - t0)
                kern.append(S.validate_kernel_ms(eng))
            if do_c:
                t0 = time.perf_counter()
                ccodes = composed()
                comp.append(time.perf_counter() - t0)
                calls.append(split["calls"])
                host.append(split["host"])
            if do_f and do_c:
                mismatches += int((pb.codes() != ccodes).sum())
        if not do_f:  # the fields of the route that did not run stay 0
            fused, kern = [0.0], [0.0]
        if not do_c:
            comp, calls, host = [0.0], [0.0], [0.0]
        stats = S.validate_stats(eng) if do_f else (0, 0, 0)
        final = pb.codes() if do_f else ccodes
        out.append({"blocks": blocks, "validators": nvals, "all_ok": bool((final == 0).all()),
                    "outcome_mismatches": mismatches,
                    "fused_call_ms": round(med(fused) * 1e3, 3), "fused_call_ms_runs": [round(x * 1e3, 3) for x in fused],
                    "composed_route_ms": round(med(comp) * 1e3, 3), "composed_route_ms_runs": [round(x * 1e3, 3) for x in comp],
                    "composed_seven_calls_ms": round(med(calls) * 1e3, 3),
                    "composed_seven_calls_ms_runs": [round(x * 1e3, 3) for x in calls],
                    "composed_host_ms": round(med(host) * 1e3, 3), "composed_host_ms_runs": [round(x * 1e3, 3) for x in host],
                    "fused_blocks_per_s": round(blocks / med(fused), 1) if do_f else 0.0,
                    "composed_blocks_per_s": round(blocks / med(comp), 1) if do_c else 0.0, "route": route,
                    "block_check_kernel_ms": round(med(kern), 4), "sets_hashed": stats[0], "sets_staged": stats[1],
                    "blocks_checked": stats[2], "signatures_verified": int(sum(pb.res[q].verified for q in range(blocks))) if do_f else 0,
                    "generate_s": round(t_gen, 2)})
    return {"config": "vb", "metric": "validateBlock per linked window: one tmed_validate_blocks call vs the seven "
                                      "existing calls + host proposer scan and compares", "runs": runs, "shapes": out}


def votes(eng, runs: int, cpu: bool, shapes=(10_000, 175)):
    """One round of free-standing votes per shape: nvals prevotes and nvals precommits at one step
    against an nvals-validator set held as an explicit key set (the key-cached kernels on both routes).
      new   one tmed_verify_votes call over both requests (TMED_VOTES_ADDVOTE);
      old   tmed_votes_sign_bytes for every vote on the host (standing in for the sign-bytes a node
            builds in Go), then one tmed_verify_batch_keyset call over the 2 x nvals tuples: no
            address checks, no error kinds;
      cpu   oracle.port's verify over the same tuples on one thread.
    Every 97th vote carries a flipped signature byte; the three routes must agree on every vote.
    Medians of `runs` timed calls."""
    import tmed.votes as V
    from tmed import pack_messages
    from tmed.workload import make_valset, pubkeys_of, seeds_from_tag
    med = lambda xs: float(np.median(xs))
    chain, height, rnd = "test_chain_id", 1_000_000, 1
    out = []
    for nvals in shapes:
        seeds = seeds_from_tag(b"tmed-votes-key", 0, nvals)
        pubs = pubkeys_of(eng, seeds)
        vals, order = make_valset(pubs, [10] * nvals)
        vpubs, _, vaddrs = vals.packed()
        handle = eng.keyset_load(vpubs[:nvals])
        vals.keyset = handle
        bid = block_id(b"votes-%d" % nvals)
        idx = np.arange(nvals)
        packed = []
        for type_ in (1, 2):
            packed.append(V.PackedVotes.from_arrays(
                types=np.full(nvals, type_), heights=np.full(nvals, height), rounds=np.full(nvals, rnd),
                block_hashes=np.tile(np.frombuffer(bid.hash, np.uint8), (nvals, 1)), block_hash_lens=np.full(nvals, 32),
                psh_totals=np.full(nvals, bid.psh_total), psh_hashes=np.tile(np.frombuffer(bid.psh_hash, np.uint8), (nvals, 1)),
                psh_hash_lens=np.full(nvals, 32), ts_seconds=T2023 + idx // 1000 + type_, ts_nanos=(idx % 1000) * 1_000_000,
                addresses=vaddrs[:nvals], address_lens=np.full(nvals, 20), validator_indexes=idx,
                sigs=np.zeros((nvals, 64), np.uint8), sig_lens=np.full(nvals, 64)))
        # sign every vote over its own sign-bytes (the GPU signer), then flip a byte of every 97th
        for pv in packed:
            msgs = V.sign_bytes(chain, pv)
            flat, off = pack_messages(msgs)
            sigs, _ = eng.sign_arrays(seeds[order], np.concatenate([flat, np.zeros(16, np.uint8)]), off)
            pv.sigs[:] = sigs
            pv.sigs[::97, 5] ^= 1
        reqs = [V.VoteRequest(chain, vals, packed[0], True, height, rnd, 1),
                V.VoteRequest(chain, vals, packed[1], True, height, rnd, 2)]
        n = 2 * nvals
        prep = V.PreparedVotes(reqs)
        prep.run(eng)  # warm: the staging buffers are allocated
        wall, dev, pdev = [], [], []
        for _ in range(runs):
            t0 = time.perf_counter()
            codes = prep.run(eng)
            wall.append(time.perf_counter() - t0)
            dev.append(eng.last_kernel_ms())
            pdev.append(V.last_prepare_ms(eng))
        codes = codes.copy()
        want_bad = np.zeros(n, bool)
        want_bad[:nvals][::97] = True
        want_bad[nvals:][::97] = True
        assert ((codes == V.VOTE_INVALID_SIGNATURE) == want_bad).all() and ((codes == V.VOTE_OK) == ~want_bad).all()
        # the route there was before
        all_sigs = np.concatenate([packed[0].sigs, packed[1].sigs])
        vidx = np.concatenate([idx, idx]).astype(np.uint32)
        old_wall, old_sb, old_dev = [], [], []
        for _ in range(runs):
            t0 = time.perf_counter()
            (f0, o0, _), (f1, o1, _) = V.sign_bytes_arrays(chain, packed[0]), V.sign_bytes_arrays(chain, packed[1])
            flat = np.concatenate([f0, f1, np.zeros(16, np.uint8)])
            off = np.concatenate([o0, o1[1:] + o0[-1]]).astype(np.uint32)
            t1 = time.perf_counter()
            bits = eng.verify_keyset_arrays(handle, vidx, all_sigs, flat, off)
            old_wall.append(time.perf_counter() - t0)
            old_sb.append(t1 - t0)
            old_dev.append(eng.last_kernel_ms())
        assert ((codes == V.VOTE_OK) == bits.astype(bool)).all(), "tmed_verify_votes and the old route disagree"
        r = {"validators": nvals, "votes": n, "invalid": int(want_bad.sum()),
             "verify_votes_ms": round(med(wall) * 1e3, 3), "verify_votes_per_s": round(n / med(wall), 1),
             "kernels_ms": round(med(dev), 4), "vote_prepare_kernel_ms": round(med(pdev), 4),
             "host_share": round(1.0 - med(dev) * 1e-3 / med(wall), 3),
             "old_route_ms": round(med(old_wall) * 1e3, 3), "old_route_votes_per_s": round(n / med(old_wall), 1),
             "old_route_sign_bytes_ms": round(med(old_sb) * 1e3, 3), "old_route_kernels_ms": round(med(old_dev), 4),
             "decisions_equal": True}
        if cpu:
            from oracle import port
            both = np.concatenate([vpubs[:nvals], vpubs[:nvals]])
            t0 = time.perf_counter()
            exp = port.verify_batch(both, all_sigs, flat, off.astype(np.uint64), 1)
            t_cpu = time.perf_counter() - t0
            assert (exp.astype(bool) == bits.astype(bool)).all(), "device and oracle.port disagree"
            r.update({"cpu_1thread_ms": round(t_cpu * 1e3, 2), "cpu_1thread_votes_per_s": round(n / t_cpu, 1)})
        eng.keyset_free(handle)
        out.append(r)
    return {"config": "votes", "metric": "free-standing votes per second: tmed_verify_votes vs host sign-bytes + "
            "tmed_verify_batch_keyset vs oracle.port on one thread", "runs": runs, "shapes": out}


def _evidence_shape(text: str):
    """'NxV': one list of N evidences against V validators; 'LxKxV': L lists of K evidences each."""
    p = [int(x) for x in text.split("x")]
    if len(p) == 2:
        return 1, p[0], p[1]
    if len(p) == 3:
        return p[0], p[1], p[2]
    raise ValueError("--evidence-shapes: NxV or LxKxV")


def evidence(eng, runs: int, shapes=("2048x10000", "1000x4x175")):
    """Duplicate-vote evidence per shape: L lists of K evidences (n = L x K) against a V-validator set held as
    an explicit key set (the key-cached kernels on both routes), evidence i by validator (4877 i) mod V.
      new   one tmed_verify_duplicate_votes call over the n evidences, one tmed_evidence_hashes call over
            the L lists;
      old   tmed_verify_duplicate_votes_host (GetByAddress as a scan per evidence and the checks, on one host
            thread), one tmed_verify_votes call over the 2n votes with the key of the found validator, the
            codes put together as the reference orders them; tmed_evidence_bytes, then tmed_merkle_roots.
    Every 97th evidence carries a flipped byte in VoteB's signature, every 101st a wrong validator power; both
    routes must agree on every code and every root before anything is timed.  Medians of `runs` timed calls."""
    import tmed.evidence as EV
    import tmed.merkle as MK
    import tmed.votes as V
    from tmed import pack_messages
    from tmed.workload import make_valset, pubkeys_of, seeds_from_tag
    med = lambda xs: float(np.median(xs))
    chain, height, rnd = "test_chain_id", 1_000_000, 1
    out = []
    for text in shapes:
        L, K, nvals = _evidence_shape(text)
        n = L * K
        seeds = seeds_from_tag(b"tmed-evidence-key", 0, nvals)
        vals, order = make_valset(pubkeys_of(eng, seeds), [10] * nvals)
        vpubs, _, vaddrs = vals.packed()
        handle = eng.keyset_load(vpubs[:nvals])
        vals.keyset = handle
        who = (np.arange(n) * 4877) % nvals          # evidence -> validator
        vwho = np.repeat(who, 2)                      # vote -> validator
        bids = [block_id(b"evidence-a-%d" % nvals), block_id(b"evidence-b-%d" % nvals)]
        side = np.tile(np.arange(2), n)               # vote -> 0 (VoteA) / 1 (VoteB)
        hashes = np.stack([np.frombuffer(b.hash, np.uint8) for b in bids])[side]
        pshs = np.stack([np.frombuffer(b.psh_hash, np.uint8) for b in bids])[side]
        vidx = np.arange(2 * n)
        pv = V.PackedVotes.from_arrays(
            types=np.full(2 * n, 1), heights=np.full(2 * n, height), rounds=np.full(2 * n, rnd), block_hashes=hashes,
            block_hash_lens=np.full(2 * n, 32), psh_totals=np.full(2 * n, 123), psh_hashes=pshs,
            psh_hash_lens=np.full(2 * n, 32), ts_seconds=T2023 + vidx // 1000, ts_nanos=(vidx % 1000) * 1_000_000,
            addresses=vaddrs[vwho], address_lens=np.full(2 * n, 20), validator_indexes=vwho,
            sigs=np.zeros((2 * n, 64), np.uint8), sig_lens=np.full(2 * n, 64))
        flat, off = pack_messages(V.sign_bytes(chain, pv))
        sigs, _ = eng.sign_arrays(seeds[order][vwho], np.concatenate([flat, np.zeros(16, np.uint8)]), off)
        pv.sigs[:] = sigs
        pv.sigs[1::2][::97, 5] ^= 1
        powers = np.full(n, 10, np.int64)
        powers[::101] = 11
        pe = EV.PackedEvidence.from_arrays(pv, np.full(n, vals.total_voting_power()), powers, T2023 + np.arange(n) // 7,
                                           np.arange(n) % 1000)
        want = np.zeros(n, np.uint8)
        want[::97] = EV.DUPVOTE_VOTE_B_SIGNATURE
        want[::101] = EV.DUPVOTE_VALIDATOR_POWER
        items, list_off = np.arange(n, dtype=np.int64), (np.arange(L + 1) * K).astype(np.uint32)
        prep = EV.PreparedEvidence([EV.EvidenceRequest(chain, vals, pe)])

        def new_route():
            t0 = time.perf_counter()
            codes = prep.run(eng)
            t1 = time.perf_counter()
            k_all, (k_look, k_prep) = eng.last_kernel_ms(), EV.last_kernel_times(eng)
            evh, roots, ev_ok, list_ok = EV.evidence_hashes_packed(eng, pe, items, list_off)
            t2 = time.perf_counter()
            return codes.copy(), evh, roots, (t1 - t0, t2 - t1, k_look, k_prep, k_all - k_look - k_prep, eng.last_kernel_ms())

        def old_route():
            t0 = time.perf_counter()
            pre = prep.run(None).copy()
            found = np.repeat(np.maximum(prep.found[:n], 0), 2).astype(np.int32)
            t1 = time.perf_counter()
            pv.validator_indexes[:] = found           # Vote.Verify with the key GetByAddress found
            vc = V.verify_votes(eng, [V.VoteRequest(chain, vals, pv)])
            k_votes = eng.last_kernel_ms()
            a, b = vc[0::2], vc[1::2]
            remap = np.array([0, 0, 0, 0, 0, 0, EV.DUPVOTE_ADDRESS_NOT_OF_KEY, EV.DUPVOTE_PANIC, 255, EV.DUPVOTE_GO_PATH], np.uint8)
            ca = np.where(a == V.VOTE_INVALID_SIGNATURE, EV.DUPVOTE_VOTE_A_SIGNATURE, remap[a])
            cb = np.where(b == V.VOTE_INVALID_SIGNATURE, EV.DUPVOTE_VOTE_B_SIGNATURE, remap[b])
            codes = np.where(pre != 0, pre, np.where(ca != 0, ca, cb)).astype(np.uint8)
            t2 = time.perf_counter()
            bflat, boff, bok = EV.evidence_bytes_arrays(pe)
            t3 = time.perf_counter()
            roots = MK.merkle_roots_packed(eng, np.concatenate([bflat, np.zeros(8, np.uint8)]), boff.astype(np.uint64), list_off)
            t4 = time.perf_counter()
            return codes, bflat, boff, roots, (t1 - t0, t2 - t1, k_votes, t3 - t2, t4 - t3)

        codes, evh, roots, _ = new_route()  # warm, and the agreement every timed run is held to
        ocodes, bflat, boff, oroots, _ = old_route()
        assert (codes == want).all(), "tmed_verify_duplicate_votes: unexpected codes"
        assert (codes == ocodes).all(), "the two routes disagree on a code"
        assert (roots == oroots).all(), "the two routes disagree on a root"
        raw = bflat.tobytes()
        for i in range(0, n, max(1, n // 64)):
            assert bytes(evh[i]) == hashlib.sha256(raw[boff[i]:boff[i + 1]]).digest(), "DuplicateVoteEvidence.Hash differs"
        new_t, old_t = [], []
        for _ in range(runs):
            c2, _, r2, t = new_route()
            assert (c2 == codes).all() and (r2 == roots).all()
            new_t.append(t)
            c3_, _, _, r3, t = old_route()
            assert (c3_ == codes).all() and (r3 == roots).all()
            old_t.append(t)
        nt, ot = np.array(new_t), np.array(old_t)
        new_wall, old_wall = med(nt[:, 0] + nt[:, 1]), med(ot[:, 0] + ot[:, 1] + ot[:, 3] + ot[:, 4])
        new_dev_ms = med(nt[:, 2] + nt[:, 3] + nt[:, 4] + nt[:, 5])
        r = {"shape": text, "lists": L, "evidences": n, "validators": nvals, "bytes": int(boff[-1]),
             "invalid": int((want != 0).sum()), "routes_agree": True,
             "new_ms": round(new_wall * 1e3, 3), "new_evidences_per_s": round(n / new_wall, 1),
             "verify_call_ms": round(med(nt[:, 0]) * 1e3, 3), "hashes_call_ms": round(med(nt[:, 1]) * 1e3, 3),
             "lookup_kernel_ms": round(med(nt[:, 2]), 4), "prepare_kernel_ms": round(med(nt[:, 3]), 4),
             "verify_kernels_ms": round(med(nt[:, 4]), 4), "hash_leaf_stage_ms": round(med(nt[:, 5]), 4),
             "lookup_share_of_verify_call": round(med(nt[:, 2]) * 1e-3 / med(nt[:, 0]), 4),
             "host_share": round(max(0.0, 1.0 - new_dev_ms * 1e-3 / new_wall), 3),
             "old_ms": round(old_wall * 1e3, 3), "old_evidences_per_s": round(n / old_wall, 1),
             "old_host_checks_ms": round(med(ot[:, 0]) * 1e3, 3), "old_verify_votes_ms": round(med(ot[:, 1]) * 1e3, 3),
             "old_verify_votes_kernels_ms": round(med(ot[:, 2]), 4), "old_evidence_bytes_ms": round(med(ot[:, 3]) * 1e3, 3),
             "old_merkle_roots_ms": round(med(ot[:, 4]) * 1e3, 3), "speedup": round(old_wall / new_wall, 3)}
        eng.keyset_free(handle)
        out.append(r)
    return {"config": "evidence", "metric": "duplicate-vote evidences per second: tmed_verify_duplicate_votes + "
            "tmed_evidence_hashes vs host checks + tmed_verify_votes + tmed_evidence_bytes + tmed_merkle_roots",
            "runs": runs, "shapes": out}


def lca(eng, runs: int, shapes=("1x10000", "50x175")):
    """Light-client-attack evidence per shape ExV: E lunatic evidences against one V-validator set (common and
    conflicting set alike: every common validator signs the conflicting block), each with its own conflicting
    header and commit, commonHeader at another height (so VerifyCommitLightTrusting runs beside
    VerifyCommitLight), the claimed list = all V validators in the reference's order.
      new   one tmed_verify_light_client_attacks call;
      old   tmed_verify_commits over the 2E commit requests, tmed_header_hashes over the 2E headers,
            tmed_byzantine_validators_host (GetByAddress as a scan per signature and a sort, one host thread).
    The seam's key-set cache is on and warm for both.  Both routes must agree (every code OK, equal lists)
    before anything is timed.  Medians of `runs` timed calls."""
    import tmed.evidence as EV
    import tmed.merkle as MK
    import tmed.types as T
    from tmed.workload import make_valset, pubkeys_of, seeds_from_tag, sign_commits
    med = lambda xs: float(np.median(xs))
    chain = "test_chain_id"
    eng.keycache_config(True)
    out = []
    for text in shapes:
        E, nvals = [int(x) for x in text.split("x")]
        seeds = seeds_from_tag(b"tmed-lca-key", 0, nvals)
        vals, order = make_valset(pubkeys_of(eng, seeds), [10] * nvals)
        _, vpowers, vaddrs = vals.packed()

        def header(tag, height):
            h = lambda t: hashlib.sha256(tag + t).digest()
            return {"version_block": 11, "version_app": 0, "chain_id": chain, "height": height, "time": (T2023, 0),
                    "last_block_id": (h(b"/last"), 1, h(b"/last-psh")), "last_commit_hash": h(b"/lc"), "data_hash": h(b"/data"),
                    "validators_hash": h(b"/vals"), "next_validators_hash": h(b"/next"), "consensus_hash": h(b"/cons"),
                    "app_hash": h(b"/app"), "last_results_hash": h(b"/res"), "evidence_hash": h(b"/ev"),
                    "proposer_address": vaddrs[0].tobytes()}

        commits = sign_commits(eng, chain, [(seeds[order], vaddrs[:nvals], 10, 1, block_id(b"lca-%d-%d" % (nvals, e)), T2023, None)
                                            for e in range(E)])
        trusted_commit = T.Commit(10, 1, block_id(b"lca-trusted"), [])
        claimed = (vaddrs[:nvals], vpowers[:nvals])
        reqs, creqs, headers = [], [], []
        for e in range(E):
            ch, th = header(b"lca-conflicting-%d" % e, 10), header(b"lca-trusted-%d" % e, 10)
            ev = EV.LightClientAttackEvidence(ch, commits[e], vals, 4, claimed, vals.total_voting_power())
            reqs.append(EV.LcaRequest(ev, 4, th, trusted_commit, vals))
            creqs += [(T.MODE_LIGHT_TRUSTING, vals, chain, None, 0, commits[e], 1, 3),
                      (T.MODE_LIGHT, vals, chain, commits[e].block_id, 10, commits[e], 0, 0)]
            headers += [ch, th]
        prep, pb, hb = EV.PreparedLca(reqs), T.PreparedBatch(creqs), MK.HeaderBatch(headers)

        def new_route():
            t0 = time.perf_counter()
            prep.run(eng)
            t1 = time.perf_counter()
            return prep.codes(), (t1 - t0,) + EV.last_lca_kernel_times(eng)

        def old_route():
            t0 = time.perf_counter()
            pb.run(eng)
            t1 = time.perf_counter()
            hb.run(eng)
            t2 = time.perf_counter()
            lists = prep.byzantine(None)
            t3 = time.perf_counter()
            return pb.codes(), lists, (t1 - t0, t2 - t1, t3 - t2)

        new_route()                 # the first call meets a cold key-set cache
        eng.keycache_wait()
        codes, _ = new_route()
        new_lists = prep.lists()
        ocodes, olists, _ = old_route()
        assert (codes == EV.LCA_OK).all(), "tmed_verify_light_client_attacks: unexpected codes %s" % codes[:8]
        assert (ocodes == 0).all(), "tmed_verify_commits: unexpected codes"
        want = list(range(nvals))   # equal powers: ascending addresses, the set's own order
        assert all(l == want for l in new_lists) and all(l == (EV.LCA_LUNATIC, EV.BYZ_OK, want) for l in olists), \
            "the two routes disagree on a list"
        new_t, old_t = [], []
        for _ in range(runs):
            c2, t = new_route()
            assert (c2 == codes).all()
            new_t.append(t)
            old_t.append(old_route()[2])
        nt, ot = np.array(new_t), np.array(old_t)
        new_wall, old_wall = med(nt[:, 0]), med(ot.sum(axis=1))
        out.append({"shape": text, "evidences": E, "validators": nvals, "signatures": E * nvals, "routes_agree": True,
                    "new_ms": round(new_wall * 1e3, 3), "new_evidences_per_s": round(E / new_wall, 1),
                    "lookup_kernel_ms": round(med(nt[:, 1]), 4), "rank_kernel_ms": round(med(nt[:, 2]), 4),
                    "old_ms": round(old_wall * 1e3, 3), "old_evidences_per_s": round(E / old_wall, 1),
                    "old_verify_commits_ms": round(med(ot[:, 0]) * 1e3, 3), "old_header_hashes_ms": round(med(ot[:, 1]) * 1e3, 3),
                    "old_byzantine_host_ms": round(med(ot[:, 2]) * 1e3, 3), "speedup": round(old_wall / new_wall, 3)})
    return {"config": "lca", "metric": "light-client-attack evidences per second: tmed_verify_light_client_attacks vs "
            "tmed_verify_commits + tmed_header_hashes + tmed_byzantine_validators_host", "runs": runs, "shapes": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c1,c3,c4")
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--headers", type=int, default=10_000)
    ap.add_argument("--gap", type=int, default=2)
    ap.add_argument("--bisect-gap", type=int, default=150, help="C3 bisection target distance (Trusting fails past 116)")
    ap.add_argument("--runs", type=int, default=7, help="C3 timed repetitions (median reported)")
    ap.add_argument("--blocks", type=int, default=100_000)
    ap.add_argument("--window", type=int, default=1000, help="blocks generated and verified per seam call")
    ap.add_argument("--batch", type=int, default=128, help="blocks per device batch inside the seam")
    ap.add_argument("--validators", type=int, default=10_000)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--c3-policy", choices=["cache", "pool", "generic"], default="cache",
                    help="C3 key handling: the seam's key-set cache (default), one explicit pooled key set, none")
    ap.add_argument("--corrupt-every", type=int, default=97, help="C4: known-answer bad signatures every N blocks (0: none)")
    ap.add_argument("--pregen", action="store_true", help="C4: generate the whole shard before timing (host rehearsal)")
    ap.add_argument("--c4-policy", choices=["cache", "explicit"], default="cache",
                    help="C4 key handling: the seam's key-set cache (default) or an explicit key-set handle")
    ap.add_argument("--no-stream", action="store_true",
                    help="C4: a tmed_blocksync_verify call per window only (no submit/wait stream pass)")
    ap.add_argument("--no-pinned", action="store_true",
                    help="C4: commits in ordinary (pageable) memory: signatures go through the seam's staging copy")
    ap.add_argument("--evidence-shapes", default="2048x10000,1000x4x175",
                    help="evidence: NxV (one list of N evidences, V validators) or LxKxV (L lists of K), comma-separated")
    ap.add_argument("--lca-shapes", default="1x10000,50x175", help="lca: ExV (E evidences, V validators), comma-separated")
    ap.add_argument("--vb-shapes", default="1000x10000,10000x175", help="vb: BxV (B linked blocks, V validators), comma-separated")
    ap.add_argument("--vb-route", choices=["both", "fused", "composed"], default="both",
                    help="vb: time both routes alternated (default), or one alone (a profiler run per route)")
    ap.add_argument("--rule", choices=["go", "zip215"], default="go",
                    help="the context's signature rule for every leg (tmed_set_rule): go, the default, or zip215")
    args = ap.parse_args()
    import torch
    import torch.distributed as dist
    from tmed import Engine
    from tmed.launch import dist_setup, gpu_count_fields
    world, rank, local, dev, coll = dist_setup()
    eng = Engine(local)
    if args.rule == "zip215":
        eng.set_rule(Engine.RULE_ZIP215)
    for cfg in args.config.split(","):
        if cfg == "c1" and rank == 0:
            r = c1(eng, args.reps, not args.no_cpu)
        elif cfg == "c3" and rank == 0:
            r = c3(eng, args.headers, args.gap, args.c3_policy, args.runs, args.bisect_gap)
        elif cfg == "c3v" and rank == 0:
            r = c3v(eng, args.headers, args.gap, args.c3_policy, args.runs)
        elif cfg == "mt" and rank == 0:
            r = mt(eng, args.runs)
        elif cfg == "vb" and rank == 0:
            r = vb(eng, args.runs, tuple(args.vb_shapes.split(",")), args.vb_route)
        elif cfg == "votes" and rank == 0:
            r = votes(eng, args.runs, not args.no_cpu)
        elif cfg == "evidence" and rank == 0:
            r = evidence(eng, min(args.runs, args.reps), tuple(args.evidence_shapes.split(",")))
        elif cfg == "lca" and rank == 0:
            r = lca(eng, min(args.runs, args.reps), tuple(args.lca_shapes.split(",")))
        elif cfg == "c4":
            r = c4(eng, args.blocks, args.validators, rank, world, coll, args.window, args.batch, args.corrupt_every,
                       args.pregen, not args.no_pinned, args.c4_policy, not args.no_stream)
        else:
            continue
        if rank == 0:
            r["rule"] = args.rule
            print(json.dumps(r), flush=True)
    if world > 1:
        dist.destroy_process_group()
    eng.close()


if __name__ == "__main__":
    main()
