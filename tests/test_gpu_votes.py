"""tmed_verify_votes on the device (csrc/votes.hip vote_prepare_kernel + the verify kernels) against
the restatement of tests/vote_cases.py, bit for bit: the corpus at the wave boundary, a batch in
which no two lanes share a field, every route (generic latency / throughput, an explicit key set
with a permuted index, the key-set cache), two requests in one call, the host-assembly route of a
long chain ID, and a 175-signature commit turned into votes."""
import collections

import numpy as np
import pytest

import tmed.types as T
import tmed.votes as V
import vote_cases as VC
from conftest import engine_with_env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus():
    """129 ADDVOTE prevotes over every class, and what the restatement says of each."""
    vals, fields, named = VC.pool(129, 6)
    req = VC.request(vals, fields, named)
    return vals, fields, named, [VC.expected(req, v) for _, v in named]


@pytest.fixture(scope="module")
def hetero():
    """129 votes for Vote.Verify alone, each with its own type, height, round, BlockID and timestamp."""
    vals, seeds = VC.valset(8, "hetero")
    votes = []
    for i in range(129):
        bid = [VC.block_id("h%d" % i), T.BlockID(), T.BlockID(VC.block_id("g%d" % i).hash, 0, b""),
               T.BlockID(b"", i, VC.block_id("p%d" % i).psh_hash)][i % 4]
        v = VC.signed(VC.CHAIN, vals, seeds, (5 * i) % 8, [1, 2, 32, 0, -1, 2**31 - 1][i % 6], 10**6 + 977 * i,
                      [0, 1, 7, 2**31 - 1][i % 4] if i % 5 else -1, bid, (VC.T0[0] + 61 * i, (i * 1000003) % 10**9))
        if i % 11 == 3:
            v.signature = VC.flip(v.signature, i % 64)
        votes.append(v)
    req = V.VoteRequest(VC.CHAIN, vals, votes)
    return req, [VC.expected(req, v) for v in votes]


def _check(got, exp, names=None):
    got = [int(g) for g in got]
    print("codes:", dict(collections.Counter(V.CODE_NAMES[g] for g in got)))
    bad = [(i, names[i] if names else "", V.CODE_NAMES[e], V.CODE_NAMES[g]) for i, (g, e) in enumerate(zip(got, exp))
           if g != e]
    assert not bad, bad[:8]
    assert collections.Counter(got) == collections.Counter(exp)


def test_corpus_covers_every_code(corpus):
    _, _, named, exp = corpus
    assert set(exp) == set(range(10))
    assert set(exp[:63]) == set(range(10))  # the smallest multi-vote batch below already holds every class
    for (name, _), e in zip(named, exp):
        assert e != V.VOTE_GO_PATH or VC.is_go_path_case(name), name


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_corpus_against_the_restatement(engine, corpus, n):
    vals, fields, named, exp = corpus
    got = V.verify_votes(engine, [VC.request(vals, fields, named[:n])])
    _check(got, exp[:n], [name for name, _ in named])
    for (name, _), g in zip(named[:n], got):
        assert g != V.VOTE_GO_PATH or VC.is_go_path_case(name), name


def test_heterogeneous_batch(engine, hetero):
    req, exp = hetero
    assert exp.count(V.VOTE_OK) > 100 and V.VOTE_INVALID_SIGNATURE in exp
    _check(V.verify_votes(engine, [req]), exp)


def test_generic_routes(generic_engine, corpus, hetero):
    vals, fields, named, exp = corpus
    got = V.verify_votes(generic_engine, [VC.request(vals, fields, named), hetero[0]])
    _check(got, exp + hetero[1])


def test_explicit_handle_with_permuted_index(engine, corpus, hetero):
    vals, fields, named, exp = corpus
    handles = []
    try:
        reqs = []
        for vs, votes, extra in ((vals, [v for _, v in named], fields), (hetero[0].vals, hetero[0].votes, {})):
            pubs = vs.packed()[0]
            n = len(vs.validators)
            perm = np.array([(5 * i + 1) % n for i in range(n)])  # key-set position -> validator (5 is coprime to 6 and 8)
            assert sorted(perm) == list(range(n))
            h = engine.keyset_load(pubs[perm])
            handles.append(h)
            inv = np.zeros(n, np.uint32)
            inv[perm] = np.arange(n, dtype=np.uint32)
            keyed = T.ValidatorSet(vs.validators, keyset=h, keyset_index=inv)
            reqs.append(V.VoteRequest(chain_id=VC.CHAIN, vals=keyed, votes=votes, **{k: v for k, v in extra.items()
                                                                                      if k != "chain_id"}))
        _check(V.verify_votes(engine, reqs), exp + hetero[1])
    finally:
        for h in handles:
            engine.keyset_free(h)


def test_key_set_cache_first_generic_then_keyed(corpus):
    vals, fields, named, exp = corpus
    eng = engine_with_env(TMED_KEYCACHE=1)
    try:
        req = VC.request(vals, fields, named)
        s0 = eng.keycache_stats()
        _check(V.verify_votes(eng, [req]), exp)
        s1 = eng.keycache_stats()
        assert s1["generic_sets"] - s0["generic_sets"] == 1 and s1["keyed_sets"] == s0["keyed_sets"]
        eng.keycache_wait()
        _check(V.verify_votes(eng, [req]), exp)
        s2 = eng.keycache_stats()
        assert s2["keyed_sets"] - s1["keyed_sets"] == 1 and s2["generic_sets"] == s1["generic_sets"]
        assert s2["keyed_sigs"] - s1["keyed_sigs"] == len(named)
    finally:
        eng.close()


def test_two_requests_and_a_long_chain_id(engine):
    """Prevotes and precommits against different sets in one call: the codes land at the prefix sums.  A
    third request with a 51-byte chain ID is assembled on the host; its valid votes still verify."""
    va, sa = VC.valset(4, "two-a")
    vb, sb = VC.valset(7, "two-b", wrong_address_at=2)
    long_chain = "c" * 51
    ca = VC.step_cases(VC.CHAIN, va, sa, 1, height=11, round_=0, tag="a")
    cb = VC.step_cases("other-chain", vb, sb, 2, height=12, round_=3, tag="b")
    cc = VC.step_cases(long_chain, va, sa, 2, height=13, round_=1, tag="c")
    reqs = [V.VoteRequest(VC.CHAIN, va, [v for _, v in ca], True, 11, 0, 1),
            V.VoteRequest("other-chain", vb, [v for _, v in cb], True, 12, 3, 2),
            V.VoteRequest(long_chain, va, [v for _, v in cc], True, 13, 1, 2)]
    exp = [[VC.expected(r, v) for v in r.votes] for r in reqs]
    assert all(e.count(V.VOTE_OK) >= 6 for e in exp) and len(ca) != len(cb)
    pv = V.PreparedVotes(reqs)
    pv.run(None)
    assert list(pv.device_route[:3]) == [1, 1, 0]
    got = V.verify_votes(engine, reqs)
    off = 0
    for r, e in zip(reqs, exp):
        _check(got[off:off + len(r.votes)], e)
        off += len(r.votes)
    assert off == len(got)
    # each request alone gives the same codes
    for r, e in zip(reqs, exp):
        _check(V.verify_votes(engine, [r]), e)


def test_four_groups_interleaved_in_one_call(engine):
    """One call whose requests alternate over all four (route, key set) groups, every group owning
    non-adjacent requests: keyed-device, generic-host (a 51-byte chain ID), generic-device, keyed-host, and
    the four once more.  Two sets share one key set (and, on the generic route, one group), one request is
    Vote.Verify alone (no ADDVOTE: its set's addresses are not staged).  The codes land at each request's
    prefix sum, and each request alone gives the same codes."""
    sets = [VC.valset(4, "grp-a"), VC.valset(7, "grp-b", wrong_address_at=2)]
    long_chain = "c" * 51
    h = engine.keyset_load(np.concatenate([vs.packed()[0][:len(vs.validators)] for vs, _ in sets]))
    try:
        first = [0, len(sets[0][0].validators)]
        keyed = [T.ValidatorSet(vs.validators, keyset=h, keyset_index=np.arange(len(vs.validators), dtype=np.uint32) + b)
                 for (vs, _), b in zip(sets, first)]
        # (set, keyed, chain): keyed-dev, generic-host, generic-dev, keyed-host, and again with the other set
        plan = [(0, True, VC.CHAIN), (0, False, long_chain), (1, False, VC.CHAIN), (1, True, long_chain),
                (0, False, "other-chain"), (1, True, VC.CHAIN), (1, False, long_chain), (0, True, long_chain)]
        reqs = []
        for j, (si, is_keyed, chain) in enumerate(plan):
            vs, seeds = sets[si]
            vals = keyed[si] if is_keyed else vs
            if j == 4:  # Vote.Verify alone
                reqs.append(V.VoteRequest(chain, vals, [v for _, v in VC.verify_cases(chain, vs, seeds, "g4")[4::3]]))
                continue
            cs = VC.step_cases(chain, vs, seeds, 1 + j % 2, height=20 + j, round_=j, tag="g%d" % j)
            votes = [v for _, v in cs[:1] + cs[1 + j::5][:4 + j % 3]]  # the valid vote and every fifth class from 1 + j
            reqs.append(V.VoteRequest(chain, vals, votes, True, 20 + j, j, 1 + j % 2))
        exp = [[VC.expected(r, v) for v in r.votes] for r in reqs]
        assert len({len(e) for e in exp}) > 1 and all(V.VOTE_OK in e and len(set(e)) >= 3 for e in exp)
        pv = V.PreparedVotes(reqs)
        pv.run(None)
        assert list(pv.device_route[:8]) == [1, 0, 1, 0, 1, 1, 0, 0]
        got = V.verify_votes(engine, reqs)
        off = 0
        for r, e in zip(reqs, exp):
            _check(got[off:off + len(r.votes)], e)
            off += len(r.votes)
        assert off == len(got)
        for r, e in zip(reqs, exp):
            _check(V.verify_votes(engine, [r]), e)
    finally:
        engine.keyset_free(h)


def test_commit_turned_into_votes(engine):
    """Commit.GetVote (types/block.go:784-796) of a 175-signature commit: every vote OK, equal to
    verify_batch's bits on the same (key, sign-bytes, signature) tuples; one flipped signature gives
    INVALID_SIGNATURE at that vote only."""
    from oracle import commit as C
    from oracle.fixtures import make_block_id, make_commit, make_valset, seed_of
    n = 175
    ovs, seeds = make_valset([seed_of("v175", i) for i in range(n)], [10] * n)
    obid = make_block_id("v175")
    flags = [C.FLAG_NIL if i % 17 == 5 else C.FLAG_COMMIT for i in range(n)]
    cm = make_commit(ovs, seeds, VC.CHAIN, 99, 1, obid, flags=flags)
    vals = T.ValidatorSet([T.Validator(v.pub_key, v.voting_power, 0, v.address) for v in ovs.validators])
    bid = T.BlockID(obid.hash, obid.psh_total, obid.psh_hash)
    votes = [V.Vote(2, cm.height, cm.round, bid if s.flag == C.FLAG_COMMIT else T.BlockID(), s.timestamp, s.address, i,
                    s.signature) for i, s in enumerate(cm.signatures)]
    pubs = [v.pub_key for v in vals.validators]
    msgs = [cm.vote_sign_bytes(VC.CHAIN, i) for i in range(n)]
    assert V.sign_bytes(VC.CHAIN, votes) == msgs
    for flipped in (None, 101):
        if flipped is not None:
            votes[flipped].signature = VC.flip(votes[flipped].signature, 37)
        bits = engine.verify_batch(pubs, msgs, [v.signature for v in votes])
        got = V.verify_votes(engine, [V.VoteRequest(VC.CHAIN, vals, votes, True, 99, 1, 2)])
        want = [V.VOTE_INVALID_SIGNATURE if i == flipped else V.VOTE_OK for i in range(n)]
        assert [int(g) for g in got] == want
        assert [g == V.VOTE_OK for g in got] == [bool(b) for b in bits]
