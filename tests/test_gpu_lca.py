"""LightClientAttackEvidence on the device: tmed_verify_light_client_attacks over the scenario table of
lca_cases.py (mixed and request by request, key-set cache cold and warm, under ZIP-215, with signatures
made by the engine), and tmed_byzantine_validators alone (no signatures) against the restatement and the
host entry at the edges of the lookup's stride, of the rank kernel's tile and of the ordering key."""
import random

import numpy as np
import pytest

import lca_cases as LC
import tmed.evidence as E
import tmed.types as T
from conftest import engine_with_env
from light_cases import BTIME, SignedHeader, gen_keys, h256, to_validators
from oracle import commit as C
from oracle import merkle as M

pytestmark = pytest.mark.gpu

TILE = 128  # csrc/lca.hip kLcaTile
MAX_POWER = ((1 << 63) - 1) // 8


# ----------------------------------------------------------------------------- the whole table

_SIGNERS = {}


def engine_signer(eng):
    """sign(seed, msg) through eng.sign_arrays, one signature per call (remembered: the table's cases share
    their commits)."""
    if id(eng) not in _SIGNERS:
        done = {}

        def sign(seed, msg):
            if (seed, msg) not in done:
                seeds = np.frombuffer(seed, np.uint8).reshape(1, 32).copy()
                msgs = np.frombuffer(msg + bytes(16), np.uint8).copy()
                sigs, _ = eng.sign_arrays(seeds, msgs, np.array([0, len(msg)], np.uint32))
                done[(seed, msg)] = bytes(sigs[0])
            return done[(seed, msg)]

        _SIGNERS[id(eng)] = sign
    return _SIGNERS[id(eng)]


@pytest.fixture(scope="module")
def cached_engine():
    """A context with the seam's key-set cache on (the shared test context has it off)."""
    e = engine_with_env(TMED_KEYCACHE=1)
    yield e
    e.close()


def _check(eng, scen):
    sets = {}
    pl = E.PreparedLca([c.request(sets) for c, _ in scen])
    pl.run(eng)
    got, lists, hashes = pl.errors(), pl.lists(), pl.hashes()
    for q, (case, code) in enumerate(scen):
        exp = case.expected()
        assert pl.res[q].code == code, (case.name, E.LCA_CODE_NAMES[pl.res[q].code], exp)
        assert LC.same_outcome(got[q], exp, code), (case.name, got[q], exp)
        assert pl.res[q].kind == case.kind(), case.name
        assert hashes[q] == (bytes(32) if code in (E.LCA_NOT_DERIVED, E.LCA_GO_PATH) else LC.evidence_hash(case.ev)), case.name
        if code in (E.LCA_OK, E.LCA_AMNESIA_HAS_VALIDATORS, E.LCA_BYZ_COUNT, E.LCA_BYZ_ADDRESS, E.LCA_BYZ_POWER):
            assert (E.BYZ_OK, lists[q]) == case.expected_list(), case.name
        if code in (E.LCA_NOT_DERIVED, E.LCA_GO_PATH):
            assert (pl.res[q].verified_trusting, pl.res[q].verified_light) == (0, 0), case.name  # nothing sent
    return pl


@pytest.mark.parametrize("cache", ["off", "on"])
def test_lca_table_gpu(engine, cached_engine, cache):
    """The whole table as one mixed batch, signatures from eng.sign_arrays; with the key-set cache on, twice:
    cold (generic kernels) and, after tmed_keycache_wait, warm (keyed)."""
    e = engine if cache == "off" else cached_engine
    scen = LC.scenarios(engine_signer(engine))
    assert len(scen) >= 40 and {code for _, code in scen} == set(range(13))
    assert max(len(c.common_vals.validators) for c, _ in scen) <= 130
    for _ in range(2 if cache == "on" else 1):
        if cache == "on":
            e.keycache_wait()
        _check(e, scen)


def test_lca_table_request_by_request_gpu(engine):
    for item in LC.scenarios(engine_signer(engine)):
        _check(engine, [item])


def test_lca_table_under_zip215_gpu(engine):
    """The context rule reaches both commit checks; honest and bit-flipped signatures decide alike."""
    engine.set_rule(engine.RULE_ZIP215)
    try:
        _check(engine, LC.scenarios(engine_signer(engine)))
    finally:
        engine.set_rule(engine.RULE_GO)


def test_lca_beside_a_submitted_blocksync_window_gpu(engine):
    """A blocksync window is submitted, then the call runs (it collects the window first)."""
    from commit_cases import pbid, to_product
    from oracle.fixtures import make_block_id, make_commit, make_valset, seed_of
    vs, seeds = make_valset([seed_of("lca-bs", i) for i in range(8)], [10] * 8)
    bids = [make_block_id("lca-bs%d" % b) for b in range(2)]
    cms = [make_commit(vs, seeds, "lca-bs", 10 + b, 0, bids[b]) for b in range(2)]
    pv = to_product(vs, cms[0])[0]
    w = T.BlocksyncWindow(pv, "lca-bs", [pbid(b) for b in bids], [10, 11], [to_product(vs, cm)[1] for cm in cms])
    w.submit(engine, 1)
    _check(engine, LC.scenarios(engine_signer(engine))[:12])
    T.blocksync_wait(engine)
    assert list(w.codes()) == [0, 0]


# ----------------------------------------------------------------------------- Hash()

def _hash_case(common_height, nil=False):
    (ev, trusted, common) = LC.make_lunatic("lunatic")
    ev = LC._with(ev, common_height=common_height)
    if nil:  # Header.Hash() is nil for an empty ValidatorsHash; the commit keeps naming its own BlockID
        ev = LC._with(ev, conflicting=SignedHeader(dict(ev.conflicting.header, validators_hash=b""), ev.conflicting.commit))
    return LC.Case("hash %d" % common_height, ev, 4, trusted, common)


def test_lca_hash_gpu(engine):
    """CommonHeight at every varint length the issue names (1, 63, 64, 2^31, 2^62: 1, 1, 2, 5 and 10 bytes of
    zigzag varint), negative and extreme ones, a header hash whose byte 31 is non-zero, a nil header hash."""
    heights = [1, 63, 64, 1 << 31, 1 << 62, 0, -1, -64, -65, LC.MAX_INT64, -LC.MAX_INT64 - 1]
    cases = [_hash_case(h) for h in heights] + [_hash_case(h, nil=True) for h in (1, 64, 1 << 62)]
    pl = E.PreparedLca([c.request() for c in cases])
    pl.run(engine)
    hh = M.header_hash(cases[0].ev.conflicting.header)
    assert hh[31] != 0
    for q, c in enumerate(cases):
        assert pl.res[q].code == E.LCA_OK, (c.name, pl.res[q].code)
        want = LC.evidence_hash(c.ev)
        assert pl.hashes()[q] == want, c.name
        if q < len(heights):  # byte 31 of the header hash takes no part
            assert want == LC.evidence_hash_of(hh[:31] + b"\x00", heights[q]) == LC.evidence_hash_of(hh[:31] + b"\xff", heights[q])
        else:
            assert M.header_hash(c.ev.conflicting.header) is None and want == LC.evidence_hash_of(None, c.ev.common_height)
    assert pl.hashes()[len(heights)] == LC.ANCHOR_NIL[2]
    assert len({h for h in pl.hashes()}) == len(cases)


# ----------------------------------------------------------------------------- tmed_byzantine_validators alone

_HDR = {}


def _headers():
    """A (conflicting, trusted-lunatic, trusted-derived) header triple; GetByzantineValidators reads the five
    derived hashes only."""
    if not _HDR:
        vals = to_validators(gen_keys("lca-synth", 2), 10, 0)
        conf = LC.random_header("synth/conflicting", 10, BTIME, vals)
        derived = dict(LC.random_header("synth/trusted", 10, BTIME, vals))
        for k in LC.DERIVED:
            derived[k] = conf[k]
        _HDR["h"] = (conf, LC.random_header("synth/lunatic", 10, BTIME, vals), derived)
    return _HDR["h"]


def _valset(addrs, powers):
    return C.ValidatorSet([C.Validator(bytes([i % 256, i // 256]) + bytes(30), p, 0, a) for i, (a, p) in enumerate(zip(addrs, powers))])


def _commit(round_, sigs):
    """sigs: [(flag, address)]."""
    return C.Commit(10, round_, C.BlockID(h256("synth"), 1, LC.PSH), [C.CommitSig(f, a, BTIME, b"") for f, a in sigs])


def _addresses(rng, n, byte):
    """n addresses that differ only in byte `byte` (n <= 256), in a shuffled order."""
    base = bytearray(rng.randbytes(20))
    vals = rng.sample(range(256), n)
    out = []
    for v in vals:
        a = bytearray(base)
        a[byte] = v
        out.append(bytes(a))
    return out


POWERS = {
    "equal": lambda rng, n: [10] * n,
    "above bit 32": lambda rng, n: [5 + (rng.randrange(4) << 33) for _ in range(n)],
    "0 and max": lambda rng, n: [MAX_POWER if i == n // 2 else 0 for i in range(n)],
    "mixed": lambda rng, n: [rng.choice([1, 2, 1 << 31, 1 << 32, (1 << 32) + 1]) for _ in range(n)],
}


def lunatic_case(rng, n, m, byte, powers):
    """A lunatic evidence over a common set of n and a conflicting commit of m ForBlock signatures (and a few
    that are not): addresses drawn from the set (so a validator is found by several signatures), addresses
    nobody has, and addresses of 19 and 21 bytes.  One address sits in the set twice: the first wins."""
    addrs = _addresses(rng, n, byte)
    if n >= 3:
        addrs[n - 1] = addrs[1]
    common = _valset(addrs, POWERS[powers](rng, n))
    sigs = []
    for k in range(m):
        r = rng.random()
        a = rng.choice(addrs)
        if r < 0.08:
            a = bytes(rng.randbytes(20))
        elif r < 0.12:
            a = a[:19]
        elif r < 0.16:
            a = a + b"\x00"
        sigs.append((C.FLAG_COMMIT, a))
    for k in range(min(m, 3)):  # signatures that are not for the block are no candidates
        sigs.insert(rng.randrange(len(sigs) + 1), (rng.choice([C.FLAG_ABSENT, C.FLAG_NIL]), rng.choice(addrs)))
    conf, lunatic, _ = _headers()
    other = _valset(_addresses(rng, 2, 0), [1, 1])
    ev = LC.Evidence(SignedHeader(conf, _commit(1, sigs)), other, 4, None, 0)
    return LC.Case("lunatic n=%d m=%d byte=%d %s" % (n, m, byte, powers), ev, 4, SignedHeader(lunatic, _commit(1, [])), common)


def equivocation_case(rng, n, byte, powers, form):
    """An equivocation over a set of n whose commit carries the set's addresses; form: "ok", "absent" (an
    all-absent trusted commit), "short" (the trusted commit is shorter: index out of range), "nobody" (a
    lookup finds nobody among several: the sort panics), "one nil" (the only candidate finds nobody)."""
    addrs = _addresses(rng, n, byte)
    vals = _valset(addrs, POWERS[powers](rng, n))
    sigs = [(rng.choice([C.FLAG_COMMIT, C.FLAG_COMMIT, C.FLAG_NIL, C.FLAG_ABSENT]), a) for a in addrs]
    tflags = [rng.choice([C.FLAG_COMMIT, C.FLAG_NIL, C.FLAG_ABSENT]) for _ in addrs]
    if form == "absent":
        tflags = [C.FLAG_ABSENT] * n
    elif form == "short":
        sigs[n - 1] = (C.FLAG_NIL, addrs[n - 1])
        tflags = tflags[:n - 1]
    elif form == "nobody":
        sigs[0], sigs[n - 1] = (C.FLAG_COMMIT, addrs[0]), (C.FLAG_COMMIT, addrs[n - 1][:19])
        tflags[0] = tflags[n - 1] = C.FLAG_COMMIT
    elif form == "one nil":
        tflags = [C.FLAG_ABSENT] * n
        k = rng.randrange(n)
        sigs[k], tflags[k] = (C.FLAG_COMMIT, bytes(rng.randbytes(20))), C.FLAG_NIL
    conf, _, derived = _headers()
    ev = LC.Evidence(SignedHeader(conf, _commit(1, sigs)), vals, 10, None, 0)
    return LC.Case("equivocation n=%d byte=%d %s %s" % (n, byte, powers, form), ev, 10,
                   SignedHeader(derived, _commit(1, [(f, b"") for f in tflags])), vals)


def _lists(eng, cases):
    sets = {}
    reqs = [c.request(sets) for c in cases]
    got = E.byzantine_validators(eng, reqs)
    host = E.byzantine_validators(None, reqs)
    for c, g, h in zip(cases, got, host):
        state, lst = c.expected_list()
        assert g == h == (c.kind(), state, lst), (c.name, g, h, state, lst)
    return got


def _edge_cases():
    rng = random.Random(20250)
    out = []
    for n in (1, 63, 64, 65, 128, 129):
        for m in (0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
            out.append(lunatic_case(rng, n, m, rng.choice([0, 3, 4, 19]), rng.choice(list(POWERS))))
    for byte in (0, 3, 4, 19):  # all powers equal: the address alone orders, byte by byte
        out.append(lunatic_case(rng, 200, 2 * TILE + 1, byte, "equal"))
    for powers in POWERS:
        out.append(lunatic_case(rng, 129, TILE + 1, 4, powers))
    for n in (2, 64, 65, 129):
        for form in ("ok", "absent", "short", "nobody", "one nil"):
            out.append(equivocation_case(rng, n, rng.choice([0, 3, 4, 19]), rng.choice(list(POWERS)), form))
    conf, _, derived = _headers()
    vals = _valset(_addresses(rng, 5, 7), [3] * 5)
    amnesia = LC.Evidence(SignedHeader(conf, _commit(0, [(C.FLAG_COMMIT, v.address) for v in vals.validators])), vals, 10,
                          None, 0)
    out.append(LC.Case("amnesia", amnesia, 10, SignedHeader(derived, _commit(1, [(C.FLAG_COMMIT, b"")] * 5)), vals))
    return out


def test_byzantine_validators_edges_gpu(engine):
    """Set sizes either side of the lookup's stride of 64, candidate counts either side of the rank kernel's
    tile, every power pattern, addresses that differ in one byte only, every equivocation form: requests of
    all sizes mixed in one call; then each alone; then a small call after the large one."""
    cases = _edge_cases()
    got = _lists(engine, cases)
    states = {(k, s) for k, s, _ in got}
    assert {(E.LCA_LUNATIC, E.BYZ_OK), (E.LCA_EQUIVOCATION, E.BYZ_OK), (E.LCA_EQUIVOCATION, E.BYZ_PANIC),
            (E.LCA_AMNESIA, E.BYZ_OK)} == states
    assert any(lst == [-1] for _, _, lst in got) and any(len(lst) > 2 * TILE - 60 for _, _, lst in got)
    assert any(len(lst) != len(set(lst)) for _, _, lst in got), "a validator found by several signatures"
    for c in cases:
        _lists(engine, [c])
    _lists(engine, cases)      # the large call again,
    _lists(engine, cases[:2])  # then a small one over the same staging arena


def test_byzantine_validators_10000_gpu(engine):
    """One lunatic evidence, 10,000 common validators and 10,000 ForBlock signatures: device, host entry and
    the rule by a dictionary and Python's sorted agree entry by entry."""
    n = 10000
    rng = np.random.default_rng(7)
    addrs = rng.integers(0, 256, (n, 20), dtype=np.uint8)
    addrs[:, :16] = addrs[0, :16]  # long common prefixes: the order is decided in the last dword
    addrs[n - 1] = addrs[5]        # one address twice
    powers = rng.choice(np.array([1, 2, 1 << 33, (1 << 33) + 1], np.int64), n)
    vals = T.ValidatorSet([T.Validator(bytes(32), int(p), 0, a.tobytes()) for a, p in zip(addrs, powers)])
    order = rng.permutation(n)
    sig_addr = addrs[order].copy()
    sig_addr[17] = 0  # nobody
    lens = np.full(n, 20, np.uint32)
    lens[23] = 19
    flags = np.full(n, C.FLAG_COMMIT, np.uint8)
    flags[99] = C.FLAG_NIL
    cm = T.PackedCommit(10, 1, T.BlockID(h256("big"), 1, LC.PSH), flags, sig_addr, np.zeros(n, np.int64),
                        np.zeros(n, np.int32), np.zeros((n, 64), np.uint8), np.zeros(n, np.uint32), lens)
    conf, lunatic, _ = _headers()
    small = T.ValidatorSet([T.Validator(bytes(32), 1, 0, bytes(20))])
    empty = T.Commit(10, 1, T.BlockID(h256("big"), 1, LC.PSH), [])
    req = E.LcaRequest(E.LightClientAttackEvidence(conf, cm, small, 4, None, 0), 4, lunatic, empty, vals)
    first = {}
    for i in range(n):
        first.setdefault(addrs[i].tobytes(), i)
    found = [first.get(sig_addr[k].tobytes()) for k in range(n) if flags[k] == C.FLAG_COMMIT and lens[k] == 20]
    want = sorted((i for i in found if i is not None), key=lambda i: (-int(powers[i]), addrs[i].tobytes()))
    assert len(want) == n - 3
    pl = E.PreparedLca([req])
    dev = pl.byzantine(engine)[0]
    host = pl.byzantine(None)[0]
    assert dev[:2] == host[:2] == (E.LCA_LUNATIC, E.BYZ_OK)
    assert dev[2] == want and host[2] == want
    lookup_ms, rank_ms = E.last_lca_kernel_times(engine)
    assert lookup_ms >= 0 and rank_ms >= 0
