"""tmed_verify_duplicate_votes and tmed_evidence_hashes on the device (csrc/evidence.hip: the lookup, prepare
and hash kernels, the verify kernels and the Merkle level builder) against the restatement of
tests/evidence_cases.py, code for code and bit for bit: every case of the host corpus on every route
(generic latency / throughput, an explicit key set, a key set with a permuted index, the key-set cache)
under both rules, the host route of a long chain ID beside a device-route request, the lookup at the
lane-stride boundaries of the set, evidence counts at the workgroup boundaries and after a larger call,
the hashes and roots over the Bytes() sweep at the list sizes that change the tree's shape, lists that mix
opaque items with device-encoded ones, every ev_ok = 0 cause, the Python surface and the bench's CLI."""
import collections
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import evidence_cases as EC
import tmed.evidence as EV
import tmed.merkle as MK
import tmed.types as T
from conftest import engine_with_env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO, ZIP = 0, 1


@pytest.fixture(scope="module")
def main():
    req, names = EC.main_request()
    return req, names, [EC.expected(req, e) for e in req.evidence]


@pytest.fixture(scope="module")
def pool():
    """130 evidences over the main set: the corpus repeated until the pool is full; batches of any size
    are its prefixes."""
    req, names = EC.main_request()
    ev, nm = list(req.evidence), list(names)
    while len(ev) < 130:
        more, nn = EC.main_request("evmain")
        ev += more.evidence
        nm += nn
    ev, nm = ev[:130], nm[:130]
    return req.vals, ev, nm, [EC.expected(req, e) for e in ev]


@pytest.fixture(scope="module")
def sweep():
    good, bad = EC.bytes_sweep()
    return good, bad, [EC.evidence_bytes(e) for _, e in good]


def _check(got, exp, names=None):
    got = [int(g) for g in got]
    print("codes:", dict(collections.Counter(EV.CODE_NAMES[g] for g in got)))
    bad = [(i, names[i] if names else "", EV.CODE_NAMES[e], EV.CODE_NAMES[g]) for i, (g, e) in enumerate(zip(got, exp))
           if g != e]
    assert not bad, bad[:8]
    assert len(got) == len(exp)


def _keyed(engine, vals, perm=None):
    """vals on an explicit key set (perm: key-set position -> validator); returns (set, handle)."""
    pubs = vals.packed()[0]
    n = len(vals.validators)
    if perm is None:
        h = engine.keyset_load(pubs[:n])
        return T.ValidatorSet(vals.validators, keyset=h), h
    h = engine.keyset_load(pubs[perm])
    inv = np.zeros(n, np.uint32)
    inv[perm] = np.arange(n, dtype=np.uint32)
    return T.ValidatorSet(vals.validators, keyset=h, keyset_index=inv), h


# ----------------------------------------------------------------------------- codes

def test_corpus_covers_every_code(main):
    _, names, exp = main
    assert set(exp) == set(range(12))


@pytest.mark.parametrize("rule", [GO, ZIP], ids=["go", "zip215"])
def test_corpus_on_the_generic_route(engine, main, rule):
    req, names, exp = main
    engine.set_rule(rule)
    try:
        _check(EV.verify_duplicate_votes(engine, [req]), exp, names)
    finally:
        engine.set_rule(GO)


def test_corpus_on_the_generic_pipelines(generic_engine, main):
    req, names, exp = main
    _check(EV.verify_duplicate_votes(generic_engine, [req]), exp, names)


@pytest.mark.parametrize("rule", [GO, ZIP], ids=["go", "zip215"])
@pytest.mark.parametrize("permuted", [False, True], ids=["identity", "permuted"])
def test_corpus_on_the_keyed_route(engine, main, rule, permuted):
    req, names, exp = main
    n = len(req.vals.validators)
    perm = np.array([(2 * i + 1) % n for i in range(n)]) if permuted else None  # 2 is coprime to 9
    assert perm is None or sorted(perm) == list(range(n))
    keyed, h = _keyed(engine, req.vals, perm)
    engine.set_rule(rule)
    try:
        _check(EV.verify_duplicate_votes(engine, [EV.EvidenceRequest(req.chain_id, keyed, req.evidence)]), exp, names)
    finally:
        engine.set_rule(GO)
        engine.keyset_free(h)


def test_keyset_index_past_the_key_set_is_a_malformed_call(engine, main):
    req, _, _ = main
    n = len(req.vals.validators)
    h = engine.keyset_load(req.vals.packed()[0][:n])
    try:
        idx = np.arange(n, dtype=np.uint32)
        idx[n - 1] = n
        bad = T.ValidatorSet(req.vals.validators, keyset=h, keyset_index=idx)
        with pytest.raises(EV.TmedError):
            EV.verify_duplicate_votes(engine, [EV.EvidenceRequest(req.chain_id, bad, req.evidence[:3])])
    finally:
        engine.keyset_free(h)


def test_key_set_cache_first_generic_then_keyed(main):
    req, names, exp = main
    eng = engine_with_env(TMED_KEYCACHE=1)
    try:
        s0 = eng.keycache_stats()
        _check(EV.verify_duplicate_votes(eng, [req]), exp, names)
        s1 = eng.keycache_stats()
        assert s1["generic_sets"] - s0["generic_sets"] == 1 and s1["keyed_sets"] == s0["keyed_sets"]
        eng.keycache_wait()
        _check(EV.verify_duplicate_votes(eng, [req]), exp, names)
        s2 = eng.keycache_stats()
        assert s2["keyed_sets"] - s1["keyed_sets"] == 1 and s2["keyed_sigs"] - s1["keyed_sigs"] == 2 * len(names)
    finally:
        eng.close()


def test_long_chain_id_beside_a_device_request(engine, main):
    """A 51-byte chain ID takes the host route (lookup, checks and messages on the host, the verify kernels
    in offset mode) beside a device-route request in the same call; the codes land at the prefix sums."""
    req, names, exp = main
    long_chain = "c" * 51
    vals, seeds = EC.valset(9, "evmain", wrong_address_at=7)
    vals = EC.repeated(vals, 2, 5)
    cs = EC.check_cases(long_chain, vals, seeds, "long")
    lreq = EV.EvidenceRequest(long_chain, vals, [e for _, e in cs])
    lexp = [EC.expected(lreq, e) for e in lreq.evidence]
    assert set(lexp) == set(range(12))
    pe = EV.PreparedEvidence([lreq, req])
    pe.run(None)
    assert list(pe.device_route[:2]) == [0, 1]
    got = EV.verify_duplicate_votes(engine, [lreq, req])
    _check(got[:len(lexp)], lexp, [n for n, _ in cs])
    _check(got[len(lexp):], exp, names)
    keyed, h = _keyed(engine, vals, np.array([(2 * i + 1) % 9 for i in range(9)]))
    try:
        _check(EV.verify_duplicate_votes(engine, [EV.EvidenceRequest(long_chain, keyed, lreq.evidence)]), lexp)
    finally:
        engine.keyset_free(h)


def test_four_groups_interleaved_in_one_call(engine):
    """One call whose requests alternate over all four (route, key set) groups, every group owning
    non-adjacent requests: keyed-device, generic-host (a 51-byte chain ID), generic-device, keyed-host, and
    the four once more with the other set.  Two sets share one key set, so every group packs two distinct
    sets behind each other.  The codes land at each request's prefix sum, and each request alone gives the
    same codes."""
    long_chain = "c" * 51
    va, sa = EC.valset(9, "evmain", wrong_address_at=7)
    sets = [(EC.repeated(va, 2, 5), sa), EC.valset(6, "evgrp", wrong_address_at=1)]
    corpus = {(si, chain): [e for _, e in EC.check_cases(chain, vs, seeds, "g%d" % si)]
              for si, (vs, seeds) in enumerate(sets) for chain in (EC.CHAIN, long_chain)}
    h = engine.keyset_load(np.concatenate([vs.packed()[0][:len(vs.validators)] for vs, _ in sets]))
    try:
        first = [0, len(sets[0][0].validators)]
        keyed = [T.ValidatorSet(vs.validators, keyset=h, keyset_index=np.arange(len(vs.validators), dtype=np.uint32) + b)
                 for (vs, _), b in zip(sets, first)]
        # (set, keyed, chain): keyed-dev, generic-host, generic-dev, keyed-host, and again with the other set
        plan = [(0, True, EC.CHAIN), (0, False, long_chain), (1, False, EC.CHAIN), (1, True, long_chain),
                (0, False, EC.CHAIN), (1, True, EC.CHAIN), (1, False, long_chain), (0, True, long_chain)]
        reqs = []
        for j, (si, is_keyed, chain) in enumerate(plan):
            cs = corpus[si, chain]
            ev = cs[:1] + cs[1 + j::8][:4 + j % 3]  # the valid evidence and every eighth case from 1 + j
            reqs.append(EV.EvidenceRequest(chain, keyed[si] if is_keyed else sets[si][0], ev))
        exp = [[EC.expected(r, e) for e in r.evidence] for r in reqs]
        assert len({len(x) for x in exp}) > 1 and all(x[0] == 0 and len(set(x)) >= 3 for x in exp)
        pe = EV.PreparedEvidence(reqs)
        pe.run(None)
        assert list(pe.device_route[:8]) == [1, 0, 1, 0, 1, 1, 0, 0]
        got = EV.verify_duplicate_votes(engine, reqs)
        off = 0
        for r, x in zip(reqs, exp):
            _check(got[off:off + len(x)], x)
            off += len(x)
        assert off == len(got)
        for r, x in zip(reqs, exp):
            _check(EV.verify_duplicate_votes(engine, [r]), x)
    finally:
        engine.keyset_free(h)


# ----------------------------------------------------------------------------- the lookup

@pytest.fixture(scope="module")
def lookup_requests():
    """Sets of 1, 63, 64, 65, 128 and 129 validators (prefixes of one key list): evidence of the first and
    the last validator and of validators 63 / 64 where the set has them, and of nobody; the sets of 65 and
    129 once more with validator 64 holding validator 63's address (a repeated address across the lanes'
    stride edge: 63 decides)."""
    reqs = []
    for n in (1, 63, 64, 65, 128, 129):
        vals, seeds = EC.valset(n, "evlook")
        idx = sorted({0, n - 1} | {i for i in (62, 63, 64, 65, 127) if i < n})
        ev = [EC.dup(EC.CHAIN, vals, seeds, i, k) for k, i in enumerate(idx)]
        stranger = EC.dup(EC.CHAIN, vals, seeds, 0, 99)
        stranger.vote_a.validator_address = stranger.vote_b.validator_address = b"\x5a" * 20
        reqs.append((EV.EvidenceRequest(EC.CHAIN, vals, ev + [stranger]), idx + [None]))
        if n in (65, 129):
            rep = EC.repeated(vals, 63, 64)
            ev = [EC.dup(EC.CHAIN, rep, seeds, 63, 7), EC.dup(EC.CHAIN, rep, seeds, 63, 8, signer=64)]
            ev.append(EC.dup(EC.CHAIN, rep, seeds, 63, 9, signer=64))
            ev[-1].validator_power = rep.validators[64].voting_power
            reqs.append((EV.EvidenceRequest(EC.CHAIN, rep, ev), [63, 63, 63]))
    return reqs


def test_lookup_boundaries(engine, lookup_requests):
    """Every request alone, then all in one call: different sets, the address bases offset."""
    exp = [[EC.expected(r, e) for e in r.evidence] for r, _ in lookup_requests]
    for (r, found), x in zip(lookup_requests, exp):
        assert [EC.pre_code(r, e)[1] for e in r.evidence] == found
        if found == [63, 63, 63]:  # the repeated address: 63's own evidence, 64's with 63's power, 64's with its own
            assert x == [0, 9, 6]
        else:
            assert x == [0] * (len(found) - 1) + [1]
        _check(EV.verify_duplicate_votes(engine, [r]), x)
    _check(EV.verify_duplicate_votes(engine, [r for r, _ in lookup_requests]), [c for x in exp for c in x])


def test_lookup_boundaries_keyed(engine, lookup_requests):
    """The same in one call on a key set loaded in reverse order: the found validator's key-set index is
    read from the packed index array at the set's base."""
    vals129 = [r.vals for r, found in lookup_requests if len(r.vals.validators) == 129 and found[-1] is None][0]
    perm = np.arange(129)[::-1].copy()
    h = engine.keyset_load(vals129.packed()[0][perm])
    try:
        reqs = []
        for r, _ in lookup_requests:
            n = len(r.vals.validators)
            idx = (128 - np.arange(n)).astype(np.uint32)  # validator i is key 128 - i
            reqs.append(EV.EvidenceRequest(r.chain_id, T.ValidatorSet(r.vals.validators, keyset=h, keyset_index=idx),
                                           r.evidence))
        exp = [EC.expected(r, e) for r, _ in lookup_requests for e in r.evidence]
        _check(EV.verify_duplicate_votes(engine, reqs), exp)
    finally:
        engine.keyset_free(h)


# ----------------------------------------------------------------------------- lanes and workgroups

def test_counts_at_the_workgroup_boundaries(engine, pool):
    """130 first, so the smaller calls run over the scratch a larger call left behind; then the pool
    rearranged so that failing cases sit at the first and the last lane of each workgroup."""
    vals, ev, names, exp = pool
    for n in (130, 1, 63, 64, 65):
        _check(EV.verify_duplicate_votes(engine, [EV.EvidenceRequest(EC.CHAIN, vals, ev[:n])]), exp[:n], names)
    edges = [0, 63, 64, 127, 128, 129]
    failing = [exp.index(x) for x in (1, 4, 6, 8, 9, 10)]
    assert len({exp[i] for i in failing}) == 6
    rest = [i for i in range(130) if i not in failing]
    order = list(rest)
    for pos, i in zip(edges, failing):
        order.insert(pos, i)
    assert sorted(order) == list(range(130)) and [order[p] for p in edges] == failing and exp[order[1]] == 0
    got = EV.verify_duplicate_votes(engine, [EV.EvidenceRequest(EC.CHAIN, vals, [ev[i] for i in order])])
    _check(got, [exp[i] for i in order], [names[i] for i in order])


def test_empty_requests_and_empty_call(engine, main):
    req, names, exp = main
    empty = EV.EvidenceRequest(EC.CHAIN, req.vals, [])
    assert len(EV.verify_duplicate_votes(engine, [])) <= 1
    got = EV.verify_duplicate_votes(engine, [empty, req, empty])
    _check(got, exp, names)


# ----------------------------------------------------------------------------- hashes

def _lists(n_ev, sizes, blobs=()):
    """Lists of the given sizes over evidence indexes 0.., wrapping; blobs are spliced in at every third place."""
    lists, k = [], 0
    for s in sizes:
        lst = []
        for j in range(s):
            if blobs and j % 3 == 1:
                lst.append(blobs[(k + j) % len(blobs)])
            else:
                lst.append(k % n_ev)
                k += 1
        lists.append(lst)
    return lists


def _want_roots(lists, ev_bytes):
    return [EC.list_hash([it if isinstance(it, bytes) else ev_bytes[it] for it in lst]) for lst in lists]


def test_hashes_and_roots_over_the_sweep(engine, sweep):
    good, _, want = sweep
    ev = [e for _, e in good]
    assert len(ev) <= 130
    lists = _lists(len(ev), [0, 1, 2, 3, 64, 65])
    hashes, roots = EV.evidence_hashes(engine, ev, lists)
    for (name, _), h, w in zip(good, hashes, want):
        assert h == hashlib.sha256(w).digest(), name
    want_roots = _want_roots(lists, want)
    assert roots == want_roots and roots[0] == hashlib.sha256(b"").digest()
    # every root equals tmed_merkle_roots over the restatement's bytes
    assert MK.merkle_roots(engine, [[want[i] for i in lst] for lst in lists]) == want_roots
    # hashes alone, no lists
    hashes2, roots2 = EV.evidence_hashes(engine, ev)
    assert hashes2 == hashes and roots2 == []


def test_lists_mixing_opaque_and_encoded_items(engine, sweep):
    good, _, want = sweep
    ev = [e for _, e in good][:40]
    blobs = [b"", b"\x01", bytes(range(200)), b"light-client-attack-evidence" * 40, bytes(55), bytes(56), bytes(1000)]
    lists = _lists(len(ev), [1, 2, 3, 5, 64, 65, 0, 4], blobs) + [[blobs[2]], [blobs[0], blobs[3]], [7, 7, 7], [7], [3, 7]]
    hashes, roots = EV.evidence_hashes(engine, ev, lists)
    assert roots == _want_roots(lists, want)
    assert hashes == [hashlib.sha256(w).digest() for w in want[:40]]
    # two lists naming the same evidence, and one list naming it three times
    assert roots[-2] == EC.list_hash([want[7]]) and roots[-3] == EC.list_hash([want[7]] * 3)


def test_every_ev_ok_cause_zeroes_its_own_evidence_and_lists(engine, sweep):
    good, bad, want = sweep
    ev = [good[3][1]] + [e for _, e in bad] + [good[-1][1], good[5][1]]
    nb = len(bad)
    gi = [0, nb + 1, nb + 2]  # the good ones
    lists = [[0, nb + 1], [nb + 2]] + [[0, 1 + j, nb + 2] for j in range(nb)] + [[1 + j] for j in range(nb)] + [[b"opaque", 0]]
    evh, roots, ev_ok, list_ok = EV.evidence_hashes_packed(
        engine, ev, *_flat(lists))
    assert list(ev_ok) == [1] + [0] * nb + [1, 1]
    for (name, _), h in zip(bad, evh[1:1 + nb]):
        assert bytes(h) == bytes(32), name
    wb = {0: want[3], nb + 1: want[-1], nb + 2: want[5]}
    for i in gi:
        assert bytes(evh[i]) == hashlib.sha256(wb[i]).digest()
    assert list(list_ok) == [1, 1] + [0] * (2 * nb) + [1]
    assert bytes(roots[0]) == EC.list_hash([wb[0], wb[nb + 1]]) and bytes(roots[1]) == EC.list_hash([wb[nb + 2]])
    assert all(bytes(r) == bytes(32) for r in roots[2:2 + 2 * nb])
    assert bytes(roots[-1]) == EC.list_hash([b"opaque", wb[0]])
    hashes, rts = EV.evidence_hashes(engine, ev, lists)
    assert hashes[1] is None and rts[2] is None and rts[0] == bytes(roots[0])


def _flat(lists):
    items, off, blobs = [], [0], []
    for lst in lists:
        for it in lst:
            if isinstance(it, bytes):
                items.append(-1 - len(blobs))
                blobs.append(it)
            else:
                items.append(it)
        off.append(len(items))
    op_off = np.zeros(len(blobs) + 1, np.uint64)
    np.cumsum(np.asarray([len(b) for b in blobs], np.uint64), out=op_off[1:])
    opaque = np.frombuffer(b"".join(blobs) + b"\0" * 8, np.uint8)
    return np.asarray(items, np.int64), np.asarray(off, np.uint32), opaque if blobs else None, op_off if blobs else None


def test_hashes_of_the_signed_corpus_and_argument_errors(engine, main):
    """The check corpus (real signatures, hashes of every length up to 32) through the hash call: what is
    carried hashes to the restatement's value, what is not has ev_ok = 0."""
    req, names, _ = main
    lists = [list(range(len(req.evidence)))]
    hashes, roots = EV.evidence_hashes(engine, req.evidence, lists)
    carried = [EC.carried(e) for e in req.evidence]
    assert not all(carried) and sum(carried) > 40
    for name, e, h, c in zip(names, req.evidence, hashes, carried):
        assert h == (EC.evidence_hash(e) if c else None), name
    assert roots == [None]
    keep = [i for i, c in enumerate(carried) if c]
    _, roots = EV.evidence_hashes(engine, req.evidence, [keep])
    assert roots == [EC.list_hash([EC.evidence_bytes(req.evidence[i]) for i in keep])]
    with pytest.raises(EV.TmedError):
        EV.evidence_hashes(engine, req.evidence, [[len(req.evidence)]])  # names no evidence
    with pytest.raises(EV.TmedError):
        EV.evidence_hashes_packed(engine, req.evidence, np.array([0, -1], np.int64), np.array([0, 2], np.uint32))  # no opaque array


# ----------------------------------------------------------------------------- the Python surface

def test_python_surface(engine, main):
    req, names, exp = main
    seen = set()
    for name, e, x in zip(names, req.evidence, exp):
        if x in seen:
            continue
        seen.add(x)
        if x in (EV.DUPVOTE_PANIC, EV.DUPVOTE_GO_PATH):
            with pytest.raises(type(EV.to_error(x))):
                EV.verify_duplicate_vote(engine, req.chain_id, req.vals, e)
        else:
            err = EV.verify_duplicate_vote(engine, req.chain_id, req.vals, e)
            assert err == EV.to_error(x) and type(err) is type(EV.to_error(x)), name
    assert seen == set(range(12))
    lk, pr = EV.last_kernel_times(engine)
    assert lk > 0 and pr > 0 and engine.last_kernel_ms() >= lk + pr
    from tmed import DuplicateVoteEvidence, EvidenceRequest, evidence_bytes, evidence_hashes, verify_duplicate_votes
    assert DuplicateVoteEvidence is EV.DuplicateVoteEvidence and EvidenceRequest is EV.EvidenceRequest
    e = req.evidence[0]
    (h,), (r,) = evidence_hashes(engine, [e], [[0]])
    (b,) = evidence_bytes([e])
    assert h == hashlib.sha256(b).digest() and r == hashlib.sha256(b"\x00" + b).digest()
    assert list(verify_duplicate_votes(engine, [EvidenceRequest(req.chain_id, req.vals, [e])])) == [0]


def test_bench_cli_at_a_reduced_shape():
    """bench_commits.py --config evidence as a command, at a reduced shape: both routes agree before anything
    is timed, and the result line carries the figures the issue names."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench_commits.py"), "--config", "evidence", "--evidence-shapes",
                        "96x33,6x3x17", "--reps", "2"], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
    assert r["config"] == "evidence" and r["runs"] == 2
    assert [s["shape"] for s in r["shapes"]] == ["96x33", "6x3x17"]
    for s in r["shapes"]:
        assert s["routes_agree"] is True and s["evidences"] in (96, 18)
        for k in ("new_evidences_per_s", "old_evidences_per_s", "lookup_kernel_ms", "prepare_kernel_ms", "verify_kernels_ms",
                  "hash_leaf_stage_ms", "host_share"):
            assert s[k] is not None and s[k] >= 0, k
