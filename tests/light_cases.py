"""light.Verify restated in Python over oracle.commit / oracle.merkle (test helper), and the scenario
builders the CPU and GPU light tests share.

Restates, line for line, ``light/verifier.go``: VerifyNonAdjacent :32-79, VerifyAdjacent :93-132,
Verify :135-151, verifyNewHeaderAndVals :153-192, HeaderExpired :207-210, and
``SignedHeader.ValidateBasic`` (``types/light.go:129-157``; Header.ValidateBasic and
Commit.ValidateBasic are an input, ``basic_err``).  The generators restate
``light/helpers_test.go:67-153`` (ToValidators, signHeader, genHeader, GenSignedHeader) with seeded
keys, and ``tables()`` the cases of ``light/verifier_test.go:19-170`` and ``:172-286``.
"""
import copy
import hashlib
from dataclasses import dataclass

from oracle import commit as C
from oracle import merkle as M
from oracle import port
from oracle.fixtures import seed_of

import tmed.light as L
import tmed.types as T
from commit_cases import to_product

SECOND = 1_000_000_000
MINUTE, HOUR = 60 * SECOND, 3600 * SECOND
MS = 1_000_000
BTIME = (1136214245, 0)        # time.Parse(time.RFC3339, "2006-01-02T15:04:05Z")
MAX_CLOCK_DRIFT = 10 * SECOND  # verifier_test.go:16
VOTE_TIME = (1136214300, 5)    # makeVote's tmtime.Now(), fixed


def h256(s: str) -> bytes:  # helpers_test.go hash()
    return hashlib.sha256(s.encode()).digest()


# ----------------------------------------------------------------------------- Go's time.Time

def time_add(t, d):
    """Time.Add on (Unix seconds, nanoseconds): d / 1e9 and d % 1e9 truncate toward zero."""
    ds = abs(d) // SECOND * (1 if d >= 0 else -1)
    sec, ns = t[0] + ds, t[1] + (d - ds * SECOND)
    if ns >= SECOND:
        sec, ns = sec + 1, ns - SECOND
    elif ns < 0:
        sec, ns = sec - 1, ns + SECOND
    return (sec, ns)


def time_after(a, b):
    return a > b  # tuples compare as (seconds, nanoseconds)


# ----------------------------------------------------------------------------- generators

_VERIFIED = {}


def fast_verify(pub, msg, sig):
    """oracle.commit's per-signature primitive through the C port (same decisions, cached)."""
    k = (pub, msg, sig)
    if k not in _VERIFIED:
        _VERIFIED[k] = len(sig) == 64 and port.verify(pub, msg, sig)
    return _VERIFIED[k]


def gen_keys(tag, n):
    """genPrivKeys: [(seed, pub)] in key order."""
    seeds = [seed_of(tag, i) for i in range(n)]
    return [(s, port.pubkey_from_seed(s)) for s in seeds]


def to_validators(keys, init, inc):
    """privKeys.ToValidators + NewValidatorSet's order (power descending, then address)."""
    vals = [C.Validator(p, init + i * inc) for i, (_, p) in enumerate(keys)]
    vals.sort(key=lambda v: (-v.voting_power, v.address))
    return C.ValidatorSet(vals)


def valset_hash(vs):
    return M.valset_hash([(v.pub_key, v.voting_power) for v in vs.validators])


@dataclass
class SignedHeader:
    header: dict
    commit: C.Commit


def gen_header(chain_id, height, time, valset, next_valset, app_hash, cons_hash, res_hash):
    return {"version_block": 11, "version_app": 0, "chain_id": chain_id, "height": height, "time": tuple(time),
            "last_block_id": (b"", 0, b""), "last_commit_hash": b"", "data_hash": M.empty_hash(),
            "validators_hash": valset_hash(valset), "next_validators_hash": valset_hash(next_valset),
            "consensus_hash": cons_hash, "app_hash": app_hash, "last_results_hash": res_hash, "evidence_hash": b"",
            "proposer_address": valset.validators[0].address}


def sign_header(keys, header, valset, first, last):
    """privKeys.signHeader: every CommitSig absent, then the votes of keys[first:last] at their
    validators' indexes; round 1, PartSetHeader total 1."""
    sigs = [C.CommitSig(C.FLAG_ABSENT) for _ in keys]
    bid = C.BlockID(M.header_hash(header) or b"", 1, h256("psh/%s/%d" % (header["chain_id"], header["height"])))
    cm = C.Commit(header["height"], 1, bid, sigs)
    for seed, pub in keys[first:last]:
        addr = C.address_of(pub)
        idx = next(i for i, v in enumerate(valset.validators) if v.address == addr)
        sigs[idx] = C.CommitSig(C.FLAG_COMMIT, addr, VOTE_TIME, b"")
        sigs[idx].signature = port.sign(seed, cm.vote_sign_bytes(header["chain_id"], idx))
    return cm


def gen_signed_header(keys, chain_id, height, time, valset, next_valset, first, last,
                      app_hash=None, cons_hash=None, res_hash=None):
    h = gen_header(chain_id, height, time, valset, next_valset, app_hash or h256("app_hash"),
                   cons_hash or h256("cons_hash"), res_hash or h256("results_hash"))
    return SignedHeader(h, sign_header(keys, h, valset, first, last))


# ----------------------------------------------------------------------------- the restatement

def header_expired(trusted, trusting_period, now):
    return not time_after(time_add(trusted.header["time"], trusting_period), now)


def signed_header_validate_basic(sh, chain_id, basic_err):
    if basic_err is not None:                                              # light.go:137-142
        return C.GoError(basic_err)
    h = sh.header
    if h["chain_id"] != chain_id:
        return C.GoError("header belongs to another chain %s, not %s" % (L._goq(h["chain_id"]), L._goq(chain_id)))
    if sh.commit.height != h["height"]:
        return C.GoError("header and commit height mismatch: %d vs %d" % (h["height"], sh.commit.height))
    hhash = M.header_hash(h) or b""                                        # bytes.Equal(nil, x) == (len(x) == 0)
    if hhash != sh.commit.block_id.hash:
        return C.GoError("commit signs block %s, header is block %s"
                         % (sh.commit.block_id.hash.hex().upper(), hhash.hex().upper()))
    return None


def verify_new_header_and_vals(untrusted, untrusted_vals, trusted, now, max_clock_drift, basic_err):
    h, t = untrusted.header, trusted.header
    err = signed_header_validate_basic(untrusted, t["chain_id"], basic_err)
    if err is not None:
        return C.GoError("untrustedHeader.ValidateBasic failed: %s" % err)
    if h["height"] <= t["height"]:
        return C.GoError("expected new header height %d to be greater than one of old header %d"
                         % (h["height"], t["height"]))
    if not time_after(h["time"], t["time"]):
        return C.GoError("expected new header time %s to be after old header time %s"
                         % (L.go_time(h["time"]), L.go_time(t["time"])))
    if not time_after(time_add(now, max_clock_drift), h["time"]):
        return C.GoError("new header has a time from the future %s (now: %s; max clock drift: %s)"
                         % (L.go_time(h["time"]), L.go_time(now), L.go_duration(max_clock_drift)))
    vh = valset_hash(untrusted_vals)
    if h["validators_hash"] != vh:
        return C.GoError("expected new header validators (%s) to match those that were supplied (%s) at height %d"
                         % (h["validators_hash"].hex().upper(), vh.hex().upper(), h["height"]))
    return None


def verify_non_adjacent(trusted, trusted_vals, untrusted, untrusted_vals, trusting_period, now, max_clock_drift,
                        trust_level, basic_err=None):
    if untrusted.header["height"] == trusted.header["height"] + 1:
        return C.GoError("headers must be non adjacent in height")
    if header_expired(trusted, trusting_period, now):
        return L.ErrOldHeaderExpired(time_add(trusted.header["time"], trusting_period), now)
    err = verify_new_header_and_vals(untrusted, untrusted_vals, trusted, now, max_clock_drift, basic_err)
    if err is not None:
        return L.ErrInvalidHeader(err)
    chain = trusted.header["chain_id"]
    err = C.verify_commit_light_trusting(trusted_vals, chain, untrusted.commit, trust_level[0], trust_level[1],
                                         verify_fn=fast_verify)
    if err is not None:
        if isinstance(err, C.ErrNotEnoughVotingPowerSigned):
            return L.ErrNewValSetCantBeTrusted(err)
        return err
    err = C.verify_commit_light(untrusted_vals, chain, untrusted.commit.block_id, untrusted.header["height"],
                                untrusted.commit, verify_fn=fast_verify)
    if err is not None:
        return L.ErrInvalidHeader(err)
    return None


def verify_adjacent(trusted, untrusted, untrusted_vals, trusting_period, now, max_clock_drift, basic_err=None):
    if untrusted.header["height"] != trusted.header["height"] + 1:
        return C.GoError("headers must be adjacent in height")
    if header_expired(trusted, trusting_period, now):
        return L.ErrOldHeaderExpired(time_add(trusted.header["time"], trusting_period), now)
    err = verify_new_header_and_vals(untrusted, untrusted_vals, trusted, now, max_clock_drift, basic_err)
    if err is not None:
        return L.ErrInvalidHeader(err)
    if untrusted.header["validators_hash"] != trusted.header["next_validators_hash"]:
        return C.GoError("expected old header next validators (%s) to match those from new header (%s)"
                         % (trusted.header["next_validators_hash"].hex().upper(),
                            untrusted.header["validators_hash"].hex().upper()))
    err = C.verify_commit_light(untrusted_vals, trusted.header["chain_id"], untrusted.commit.block_id,
                                untrusted.header["height"], untrusted.commit, verify_fn=fast_verify)
    if err is not None:
        return L.ErrInvalidHeader(err)
    return None


def verify(trusted, trusted_vals, untrusted, untrusted_vals, trusting_period, now, max_clock_drift, trust_level,
           basic_err=None):
    if untrusted.header["height"] != trusted.header["height"] + 1:
        return verify_non_adjacent(trusted, trusted_vals, untrusted, untrusted_vals, trusting_period, now,
                                   max_clock_drift, trust_level, basic_err)
    return verify_adjacent(trusted, untrusted, untrusted_vals, trusting_period, now, max_clock_drift, basic_err)


def same(a, b):
    """Equal error values: the same type name and the same Error() text (None: no error)."""
    if a is None or b is None:
        return a is None and b is None
    return type(a).__name__ == type(b).__name__ and str(a) == str(b)


def same_outcome(got, exp, code):
    """Equal error values; for HEADER_BASIC the text is the Go method's and only the kind is compared."""
    if code == L.HEADER_BASIC:
        return isinstance(got, L.ErrInvalidHeader) and isinstance(exp, L.ErrInvalidHeader) and \
            str(got).startswith("invalid header: untrustedHeader.ValidateBasic failed: ")
    if code == L.GO_PATH:
        return isinstance(got, L.GoPath)
    return same(got, exp)


# ----------------------------------------------------------------------------- scenarios

@dataclass
class Case:
    """One light.Verify call in oracle types; ``pair()`` is the product's form, ``expected()`` the
    restatement's error."""
    name: str
    trusted: SignedHeader
    trusted_vals: C.ValidatorSet
    untrusted: SignedHeader
    vals: C.ValidatorSet
    trusting_period: int = 3 * HOUR
    now: tuple = time_add(BTIME, 2 * HOUR)
    max_clock_drift: int = MAX_CLOCK_DRIFT
    trust_level: tuple = (1, 3)
    basic_err: str = None

    def expected(self):
        return verify(self.trusted, self.trusted_vals, self.untrusted, self.vals, self.trusting_period, self.now,
                      self.max_clock_drift, self.trust_level, self.basic_err)

    def pair(self, sets=None):
        """The LightPair; sets: a dict shared by the cases of one call so that equal sets are one
        tmed.types.ValidatorSet object (one tmed_valset)."""
        sets = {} if sets is None else sets

        def pv(vs):
            k = tuple((v.pub_key, v.voting_power) for v in vs.validators)
            if k not in sets:
                sets[k] = to_product(vs, self.untrusted.commit)[0]
            return sets[k]

        return L.LightPair(self.trusted.header, pv(self.trusted_vals), self.untrusted.header,
                           to_product(self.vals, self.untrusted.commit)[1], pv(self.vals), self.trusting_period,
                           self.now, self.max_clock_drift, self.trust_level, self.basic_err is None)

    def hashes(self):
        """(Header.Hash or None, untrusted ValidatorSet.Hash) from the oracle."""
        return M.header_hash(self.untrusted.header), valset_hash(self.vals)


def oracle_hash_arrays(cases):
    """The three arrays tmed_light_verify_with takes, from the oracle."""
    import numpy as np
    n = len(cases)
    hh, ok, vh = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8)
    for i, c in enumerate(cases):
        h, v = c.hashes()
        if h is not None:
            hh[i], ok[i] = np.frombuffer(h, np.uint8), 1
        vh[i] = np.frombuffer(v, np.uint8)
    return hh, ok, vh


def oracle_verifier(pubs, sigs, lens, msgs, offs):
    import numpy as np
    out = port.verify_batch(pubs, sigs, msgs, offs.astype(np.uint64), 4)
    out[lens != 64] = 0
    return out


def _world(chain):
    keys = gen_keys("light", 4)
    vals = to_validators(keys, 20, 10)  # 20, 30, 40, 50: the first 3 don't have 2/3, the last 3 do
    trusted = gen_signed_header(keys, chain, 1, BTIME, vals, vals, 0, 4)
    return keys, vals, trusted


_TABLES = []


def tables():
    """[(Case, pinned)] restating verifier_test.go's two tables; pinned: None (no error), a substring of
    the error text, or ("invalid" | "cant_trust", got, needed) for the two pinned error values."""
    if _TABLES:
        return _TABLES
    out = []
    # TestVerifyAdjacentHeaders (:19-170), through Verify
    chain = "TestVerifyAdjacentHeaders"
    keys, vals, header = _world(chain)
    other = to_validators(keys, 10, 1)
    H = lambda t: time_add(BTIME, t)
    G = lambda ch, t, vs, nvs, first: gen_signed_header(keys, ch, 2, H(t), vs, nvs, first, 4)

    def adj(name, sh, nv, pinned, **kw):
        out.append((Case("adjacent/" + name, header, vals, sh, nv, **kw), pinned))

    # 0: the same header: VerifyAdjacent refuses it by height; Verify sends it down the non-adjacent
    # path, where verifyNewHeaderAndVals refuses it
    adj("0 same header", header, vals, "to be greater than one of old header")
    adj("1 different chainID", G("different-chainID", HOUR, vals, vals, 0), vals, "header belongs to another chain")
    adj("2 time before old", G(chain, -HOUR, vals, vals, 0), vals, "to be after old header time")
    adj("3 time from the future", G(chain, 3 * HOUR, vals, vals, 0), vals, "new header has a time from the future")
    adj("4 acceptable drift", G(chain, 2 * HOUR + MAX_CLOCK_DRIFT - MS, vals, vals, 0), vals, None)
    adj("5 3/3 signed", G(chain, HOUR, vals, vals, 0), vals, None)
    adj("6 2/3 signed", G(chain, HOUR, vals, vals, 1), vals, None)
    adj("7 1/3 signed", G(chain, HOUR, vals, vals, 3), vals, ("invalid", 50, 93))
    adj("8 vals differ from trusted next", G(chain, HOUR, other, vals, 0), other, "to match those from new header")
    adj("9 vals inconsistent with header", G(chain, HOUR, vals, vals, 0), other, "to match those that were supplied")
    adj("10 old header expired", G(chain, HOUR, vals, vals, 0), other, "old header has expired",
        trusting_period=HOUR, now=H(HOUR))
    # TestVerifyNonAdjacentHeaders (:172-286)
    chain = "TestVerifyNonAdjacentHeaders"
    keys, vals, header = _world(chain)

    def non(name, ks, height, init, first, pinned):
        vs = to_validators(ks, init, 10)
        sh = gen_signed_header(ks, chain, height, H(HOUR), vs, vs, first, len(ks))
        out.append((Case("non-adjacent/" + name, header, vals, sh, vs), pinned))

    non("0 3/3 new, 3/3 old", keys, 3, 20, 0, None)
    non("1 2/3 new, 3/3 old", keys, 4, 20, 1, None)
    non("2 1/3 new, 3/3 old", keys, 5, 20, 3, ("invalid", 50, 93))
    non("3 3/3 new, 2/3 old", keys[1:], 5, 30, 0, None)
    non("4 3/3 new, 1/3 old", keys[3:], 5, 50, 0, None)
    non("5 3/3 new, <1/3 old", keys[:1], 5, 20, 0, ("cant_trust", 20, 46))
    _TABLES.extend(out)
    return _TABLES


_SCENARIOS = []


def scenarios():
    """[(Case, code)]: one case per outcome code, the precedence pairs, the boundary times and a header
    outside header_hash_kernel's limits; code = the TMED_LIGHT_* outcome it must give."""
    if _SCENARIOS:
        return _SCENARIOS
    chain = "light-chain"
    keys, vals, trusted = _world(chain)
    other_keys = gen_keys("light-other", 4)
    other = to_validators(other_keys, 10, 1)
    H = lambda t: time_add(BTIME, t)
    out = []

    def good(height=2, t=HOUR, **kw):
        return gen_signed_header(keys, chain, height, H(t), vals, vals, 0, 4, **kw)

    def case(name, code, sh, nv=vals, tv=vals, **kw):
        out.append((Case(name, trusted, tv, sh, nv, **kw), code))

    def bad_sig(sh, idx):
        s = bytearray(sh.commit.signatures[idx].signature)
        s[7] ^= 0x20
        sh.commit.signatures[idx].signature = bytes(s)
        return sh

    def edit(sh, **fields):  # the header changed after it was signed
        sh = copy.deepcopy(sh)
        sh.header.update(fields)
        return sh

    # one per outcome code
    case("ok adjacent", L.OK, good())
    case("ok non-adjacent", L.OK, good(5))
    case("expired", L.OLD_HEADER_EXPIRED, good(), trusting_period=HOUR, now=H(HOUR + 1))
    case("header basic", L.HEADER_BASIC, good(), basic_err="invalid header: zero Height")
    case("wrong chain", L.WRONG_CHAIN, gen_signed_header(keys, "another", 2, H(HOUR), vals, vals, 0, 4))
    sh = good()
    sh.commit.height = 3
    case("commit height", L.COMMIT_HEIGHT, sh)
    case("commit header hash", L.COMMIT_HEADER_HASH, edit(good(), app_hash=h256("other app")))
    case("commit header hash, nil Header.Hash", L.COMMIT_HEADER_HASH, edit(good(), validators_hash=b""))
    sh = edit(good(), validators_hash=b"")  # a nil Header.Hash equals an empty commit hash (bytes.Equal)
    sh.commit.block_id = C.BlockID(b"", 1, sh.commit.block_id.psh_hash)
    case("nil Header.Hash and empty commit hash", L.VALS_HASH, sh)
    case("height not greater", L.HEIGHT_NOT_GREATER, good(1))
    case("time not after", L.TIME_NOT_AFTER, good(t=-HOUR))
    case("time from the future", L.TIME_FROM_FUTURE, good(t=3 * HOUR))
    case("vals hash", L.VALS_HASH, good(), nv=other)
    case("next vals hash", L.NEXT_VALS_HASH, gen_signed_header(other_keys, chain, 2, H(HOUR), other, vals, 0, 4),
         nv=other)
    case("trusting: not enough power", L.TRUSTING,
         gen_signed_header(other_keys, chain, 5, H(HOUR), other, other, 0, 4), nv=other)
    case("trusting: zero denominator", L.TRUSTING, good(5), trust_level=(1, 0))
    case("commit: wrong signature", L.COMMIT, bad_sig(good(), 0))
    case("commit: not enough power", L.COMMIT, gen_signed_header(keys, chain, 6, H(HOUR), vals, vals, 3, 4))
    case("go path: now outside the Timestamp range", L.GO_PATH, good(), now=(253402300800, 0))
    # precedence: two checks fail, the earlier one is returned
    case("expired before wrong header hash", L.OLD_HEADER_EXPIRED, edit(good(), app_hash=b"x"),
         trusting_period=HOUR, now=H(HOUR))
    case("wrong header hash before time not after", L.COMMIT_HEADER_HASH,
         edit(good(t=-HOUR), data_hash=h256("d")))
    case("set-hash mismatch before bad signature", L.VALS_HASH, bad_sig(good(), 0), nv=other)
    sh = bad_sig(gen_signed_header(other_keys, chain, 5, H(HOUR), other, other, 0, 4), 0)
    case("trusting failure before light failure", L.TRUSTING, sh, nv=other)
    # boundary times
    case("exactly at expiry", L.OLD_HEADER_EXPIRED, good(), trusting_period=2 * HOUR)
    case("one nanosecond before expiry", L.OK, good(), trusting_period=2 * HOUR + 1)
    case("equal header times", L.TIME_NOT_AFTER, good(t=0))
    case("one nanosecond after the old header", L.OK, good(t=1))
    case("exactly now + drift", L.TIME_FROM_FUTURE, good(t=2 * HOUR + MAX_CLOCK_DRIFT))
    case("one nanosecond before now + drift", L.OK, good(t=2 * HOUR + MAX_CLOCK_DRIFT - 1))
    case("negative period", L.OLD_HEADER_EXPIRED, good(), trusting_period=-1)
    # a header the fused kernel does not take (AppHash of 65 bytes): the host-leaf route, same result
    case("65-byte AppHash", L.OK, good(app_hash=bytes(range(65))))
    case("65-byte AppHash, non-adjacent", L.OK, good(7, app_hash=bytes(range(65))))
    _SCENARIOS.extend(out)
    return _SCENARIOS


def c3_shape(heights=12, n_vals=25):
    """[Case]: a small light-client workload.  The set changes by one key per height (height h is
    signed by keys h .. h + n_vals - 1); all pairs (h, h + k), k = 1 (adjacent) and 2..4, the trusted
    set of a non-adjacent pair being the trusted header's next set, as the light client holds it.
    One header is changed after signing, one supplied set is not the header's, and two commits carry
    a bad signature: one before the 2/3 crossing (reached: an error) and one past it (never reached)."""
    chain = "c3-shape"
    keys = gen_keys("c3", heights + n_vals + 1)
    powers = lambda h: to_validators(keys[h:h + n_vals], 10, 0)
    sets = [powers(h) for h in range(heights + 2)]
    shs = [None]
    for h in range(1, heights + 1):
        shs.append(gen_signed_header(keys[h:h + n_vals], chain, h, time_add(BTIME, h * MINUTE), sets[h], sets[h + 1],
                                     0, n_vals))
    hdr_h, set_h, early_h, late_h = heights // 2 - 1, heights // 2 + 1, heights * 3 // 4, heights - 1  # 5, 7, 9, 11
    shs[hdr_h].header["data_hash"] = h256("changed after signing")
    wrong_set = to_validators(keys[set_h:set_h + n_vals], 10, 1)

    def flip(h, idx):
        s = bytearray(shs[h].commit.signatures[idx].signature)
        s[40] ^= 1
        shs[h].commit.signatures[idx].signature = bytes(s)

    flip(early_h, 2)          # 2/3 of 250 is crossed after 17 signatures, 1/3 after 9: reached by both loops
    flip(late_h, n_vals - 1)  # past both crossings
    out = []
    for h in range(1, heights + 1):
        for k in (1, 2, 3, 4):
            if h + k > heights:
                continue
            u = h + k
            out.append(Case("c3 %d->%d" % (h, u), shs[h], sets[h + 1], shs[u], wrong_set if u == set_h else sets[u],
                            trusting_period=3 * HOUR, now=time_add(BTIME, HOUR)))
    return out
