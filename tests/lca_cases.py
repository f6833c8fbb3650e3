"""VerifyLightClientAttack restated in Python over oracle.commit / oracle.merkle (test helper), and the
scenario builders the CPU and GPU tests of light-client-attack evidence share.

Restates ``evidence/verify.go``: VerifyLightClientAttack :113-154 and validateABCIEvidence :226-271, and
``types/evidence.go``: GetByzantineValidators :233-279 (with Python's ``sorted`` on (-power, address)),
ConflictingHeaderIsInvalid :285-292 and Hash :302-309.  ``scenarios()`` restates the calls of
``evidence/verify_test.go:30-357`` with seeded keys (makeLunaticEvidence :452-520) and adds one case
per remaining outcome code, the ordering pairs and the panics.
"""
import copy
import hashlib
from dataclasses import dataclass

from oracle import commit as C
from oracle import merkle as M
from oracle import port

import tmed.evidence as E
import tmed.types as T
from commit_cases import to_product
from light_cases import (BTIME, HOUR, SignedHeader, fast_verify, gen_header, gen_keys, h256, time_add, time_after,
                         to_validators)
import tmed.light as L

CHAIN = "evidence_chain"  # evidenceChainID
PSH = h256("partshash")
MAX_INT64 = (1 << 63) - 1


class Panic(Exception):
    """The reference panics."""


# ----------------------------------------------------------------------------- the restatement

@dataclass
class Evidence:
    """types.LightClientAttackEvidence in oracle types; byz: None (nil) or a list of C.Validator."""
    conflicting: SignedHeader
    conflicting_vals: C.ValidatorSet
    common_height: int
    byz: object
    total_voting_power: int


DERIVED = ("validators_hash", "next_validators_hash", "consensus_hash", "app_hash", "last_results_hash")


def conflicting_header_is_invalid(ev, trusted_header):  # evidence.go:285-292; bytes.Equal: nil equals empty
    return any(bytes(trusted_header[k]) != bytes(ev.conflicting.header[k]) for k in DERIVED)


def get_byzantine_validators(ev, common_vals, trusted):
    """evidence.go:233-279: None (nil) or the list of validators (None entries: a nil *Validator).
    sort.Sort on a list of two or more calls Less on every element, and Less dereferences."""
    validators = None

    def by_power(vs):
        if vs is not None and len(vs) >= 2 and any(v is None for v in vs):
            raise Panic("nil *Validator in ValidatorsByVotingPower.Less")
        return vs if vs is None or len(vs) < 2 else sorted(vs, key=lambda v: (-v.voting_power, v.address))

    if conflicting_header_is_invalid(ev, trusted.header):
        for sig in ev.conflicting.commit.signatures:
            if not sig.for_block():
                continue
            _, val = common_vals.get_by_address(sig.address)
            if val is None:
                continue
            validators = (validators or []) + [val]
        return by_power(validators)
    if trusted.commit.round == ev.conflicting.commit.round:
        for i, sig_a in enumerate(ev.conflicting.commit.signatures):
            if sig_a.absent():
                continue
            if i >= len(trusted.commit.signatures):
                raise Panic("index out of range")
            if trusted.commit.signatures[i].absent():
                continue
            _, val = ev.conflicting_vals.get_by_address(sig_a.address)
            validators = (validators or []) + [val]
        return by_power(validators)
    return validators


def put_varint(x):  # encoding/binary.PutVarint
    ux = (x << 1) & ((1 << 64) - 1)
    if x < 0:
        ux ^= (1 << 64) - 1
    out = bytearray()
    while ux >= 0x80:
        out.append((ux & 0x7f) | 0x80)
        ux >>= 7
    out.append(ux)
    return bytes(out)


def evidence_hash_of(header_hash, common_height):
    """Hash() from the conflicting header's hash (None: nil)."""
    v = put_varint(common_height)
    bz = bytearray(32 + len(v))
    h = (header_hash or b"")[:31]
    bz[:len(h)] = h
    bz[32:] = v
    return hashlib.sha256(bytes(bz)).digest()


def evidence_hash(ev):  # evidence.go:302-309
    return evidence_hash_of(M.header_hash(ev.conflicting.header), ev.common_height)


def validate_abci_evidence(ev, common_vals, trusted):  # verify.go:226-271
    if ev.total_voting_power != common_vals.total_voting_power():
        return C.GoError("total voting power from the evidence and our validator set does not match (%d != %d)"
                         % (ev.total_voting_power, common_vals.total_voting_power()))
    validators = get_byzantine_validators(ev, common_vals, trusted)
    if validators is None and ev.byz is not None:
        return C.GoError("expected nil validators from an amnesia light client attack but got %d" % len(ev.byz))
    exp, got = len(validators or []), len(ev.byz or [])
    if exp != got:
        return C.GoError("expected %d byzantine validators from evidence but got %d" % (exp, got))
    for idx, val in enumerate(validators or []):
        if val is None:
            raise Panic("nil pointer dereference")
        if ev.byz[idx].address != val.address:
            return C.GoError("evidence contained an unexpected byzantine validator address; expected: %s, got: %s"
                             % (val.address.hex().upper(), ev.byz[idx].address.hex().upper()))
        if ev.byz[idx].voting_power != val.voting_power:
            return C.GoError("evidence contained unexpected byzantine validator power; expected %d, got %d"
                             % (val.voting_power, ev.byz[idx].voting_power))
    return None


def verify_light_client_attack(ev, common_header_height, trusted, common_vals):  # verify.go:113-154
    chain = trusted.header["chain_id"]
    cm = ev.conflicting.commit
    try:
        if common_header_height != ev.conflicting.header["height"]:
            err = C.verify_commit_light_trusting(common_vals, chain, cm, 1, 3, verify_fn=fast_verify)
            if err is not None:
                return C.GoError("skipping verification of conflicting block failed: %s" % err)
        elif conflicting_header_is_invalid(ev, trusted.header):
            return C.GoError("common height is the same as conflicting block height so expected the conflicting"
                             " block to be correctly derived yet it wasn't")
        err = C.verify_commit_light(ev.conflicting_vals, chain, cm.block_id, ev.conflicting.header["height"], cm,
                                    verify_fn=fast_verify)
    except (RuntimeError, ValueError) as e:  # the oracle's loops raise where Go panics
        raise Panic(str(e))
    if err is not None:
        return C.GoError("invalid commit from conflicting block: %s" % err)
    if ev.total_voting_power != common_vals.total_voting_power():
        return C.GoError("total voting power from the evidence and our validator set does not match (%d != %d)"
                         % (ev.total_voting_power, common_vals.total_voting_power()))
    if ev.conflicting.header["height"] > trusted.header["height"] and \
            time_after(ev.conflicting.header["time"], trusted.header["time"]):
        return C.GoError("conflicting block doesn't violate monotonically increasing time (%s is after %s)"
                         % (L.go_time(ev.conflicting.header["time"]), L.go_time(trusted.header["time"])))
    if (M.header_hash(trusted.header) or b"") == (M.header_hash(ev.conflicting.header) or b""):
        return C.GoError("trusted header hash matches the evidence's conflicting header hash: %s"
                         % (M.header_hash(trusted.header) or b"").hex().upper())
    return validate_abci_evidence(ev, common_vals, trusted)


# ----------------------------------------------------------------------------- cases

def index_list(validators, vals):
    """A restated list as the product reports it: indices into vals (identity), -1 for a nil entry."""
    return [-1 if v is None else next(i for i, w in enumerate(vals.validators) if w is v) for v in validators or []]


@dataclass
class Case:
    """One VerifyLightClientAttack call in oracle types."""
    name: str
    ev: Evidence
    common_header_height: int
    trusted: SignedHeader
    common_vals: C.ValidatorSet

    def kind(self):
        if conflicting_header_is_invalid(self.ev, self.trusted.header):
            return E.LCA_LUNATIC
        return E.LCA_EQUIVOCATION if self.trusted.commit.round == self.ev.conflicting.commit.round else E.LCA_AMNESIA

    def lookup_vals(self):
        return self.common_vals if self.kind() == E.LCA_LUNATIC else self.ev.conflicting_vals

    def expected(self):
        """The restatement's error (None: verified), or the string "panic"."""
        try:
            return verify_light_client_attack(self.ev, self.common_header_height, self.trusted, self.common_vals)
        except Panic:
            return "panic"

    def expected_list(self):
        """(state, indices) of GetByzantineValidators alone."""
        try:
            return E.BYZ_OK, index_list(get_byzantine_validators(self.ev, self.common_vals, self.trusted),
                                        self.lookup_vals())
        except Panic:
            return E.BYZ_PANIC, []

    def request(self, sets=None):
        """The LcaRequest; sets: a dict shared by the cases of one call so that equal sets are one
        tmed.types.ValidatorSet object (one tmed_valset)."""
        sets = {} if sets is None else sets

        def pv(vs):
            k = tuple((v.pub_key, v.voting_power, v.address) for v in vs.validators)
            if k not in sets:
                sets[k] = to_product(vs, self.trusted.commit)[0]
            return sets[k]

        ev = self.ev
        byz = None if ev.byz is None else [T.Validator(v.pub_key, v.voting_power, 0, v.address) for v in ev.byz]
        pe = E.LightClientAttackEvidence(ev.conflicting.header, to_product(ev.conflicting_vals, ev.conflicting.commit)[1],
                                         pv(ev.conflicting_vals), ev.common_height, byz, ev.total_voting_power)
        return E.LcaRequest(pe, self.common_header_height, self.trusted.header,
                            to_product(self.common_vals, self.trusted.commit)[1], pv(self.common_vals))


def same_outcome(got, exp, code):
    """Equal error values.  PANIC and GO_PATH are kinds; SAME_HASH's text ends in a hash the result does
    not carry, so its prefix is compared."""
    if code == E.LCA_PANIC:
        return isinstance(got, E.EvidencePanic) and exp == "panic"
    if code == E.LCA_GO_PATH:
        return isinstance(got, E.EvidenceGoPath)
    if exp == "panic" or isinstance(got, RuntimeError):
        return False
    if code == E.LCA_SAME_HASH:
        return got is not None and exp is not None and str(exp).startswith(str(got) + ": ")
    if got is None or exp is None:
        return got is None and exp is None
    return str(got) == str(exp)


def oracle_hash_arrays(cases):
    """The four arrays tmed_verify_light_client_attacks_with takes, from the oracle."""
    import numpy as np
    n = len(cases)
    out = [np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)]
    for i, c in enumerate(cases):
        for k, hdr in ((0, c.ev.conflicting.header), (2, c.trusted.header)):
            h = M.header_hash(hdr)
            if h is not None:
                out[k][i], out[k + 1][i] = np.frombuffer(h, np.uint8), 1
    return out


# ----------------------------------------------------------------------------- generators

def make_commit(keys, valset, chain, header, round_, signers, vote_time=BTIME, psh_total=1000, sign=port.sign):
    """types.MakeCommit: one CommitSig per validator of valset, absent unless its key is in signers
    (a list of (seed, pub)); the BlockID names the header; sign(seed, msg): the signer."""
    bid = C.BlockID(M.header_hash(header) or b"", psh_total, PSH)
    cm = C.Commit(header["height"], round_, bid, [C.CommitSig(C.FLAG_ABSENT) for _ in valset.validators])
    seeds = {C.address_of(p): s for s, p in signers}
    for idx, v in enumerate(valset.validators):
        if v.address in seeds:
            cm.signatures[idx] = C.CommitSig(C.FLAG_COMMIT, v.address, vote_time, b"")
            cm.signatures[idx].signature = sign(seeds[v.address], cm.vote_sign_bytes(chain, idx))
    return cm


def flags_commit(valset, header, round_, flags=None):
    """A commit of which only round, size and flags are read (the trusted one): no signatures."""
    flags = flags if flags is not None else [C.FLAG_COMMIT] * len(valset.validators)
    return C.Commit(header["height"], round_, C.BlockID(M.header_hash(header) or b"", 1000, PSH),
                    [C.CommitSig(f, v.address if f != C.FLAG_ABSENT else b"", BTIME, b"")
                     for f, v in zip(flags, valset.validators)])


def random_header(tag, height, time, vals):
    """makeHeaderRandom: every hash its own."""
    return gen_header(CHAIN, height, time, vals, vals, h256(tag + "/app"), h256(tag + "/cons"), h256(tag + "/res"))


def make_lunatic(tag, height=10, common_height=4, total=10, byz=4, phantom=6, attack_time=None, init=10, inc=0,
                 sign=port.sign):
    """makeLunaticEvidence (verify_test.go:452-520): (Evidence, trusted SignedHeader, common set)."""
    attack_time = attack_time or time_add(BTIME, HOUR)
    ckeys = gen_keys(tag + "/common", total)
    common_vals = to_validators(ckeys, init, inc)
    byz_vals = common_vals.validators[:byz]
    byz_keys = [k for k in ckeys if C.address_of(k[1]) in {v.address for v in byz_vals}]
    pkeys = gen_keys(tag + "/phantom", phantom)
    conf_vals = C.ValidatorSet(sorted([copy.copy(v) for v in byz_vals] + to_validators(pkeys, init, inc).validators,
                                      key=lambda v: (-v.voting_power, v.address)))
    conf_header = random_header(tag + "/conflicting", height, attack_time, conf_vals)
    tkeys = gen_keys(tag + "/trusted", total)
    trusted_vals = to_validators(tkeys, init, inc)
    trusted_header = random_header(tag + "/trusted", height, BTIME, trusted_vals)
    cm = make_commit(None, conf_vals, CHAIN, conf_header, 1, pkeys + byz_keys, sign=sign)
    claimed = sorted(byz_vals, key=lambda v: (-v.voting_power, v.address))
    ev = Evidence(SignedHeader(conf_header, cm), conf_vals, common_height, claimed, common_vals.total_voting_power())
    return ev, SignedHeader(trusted_header, flags_commit(trusted_vals, trusted_header, 1)), common_vals


def make_same_height(tag, n=5, signers=4, conflicting_round=1, init=10, inc=0, sign=port.sign):
    """The equivocation / amnesia set-up (verify_test.go:193-233, :278-317): both headers at height 10
    with the same derived hashes; the first `signers` validators sign the conflicting block."""
    keys = gen_keys(tag, n)
    vals = to_validators(keys, init, inc)
    conf_header = random_header(tag + "/conflicting", 10, BTIME, vals)
    trusted_header = dict(random_header(tag + "/trusted", 10, BTIME, vals))
    for k in DERIVED:
        trusted_header[k] = conf_header[k]
    trusted_header["data_hash"] = h256(tag + "/other data")
    addrs = [v.address for v in vals.validators[:signers]]
    cm = make_commit(None, vals, CHAIN, conf_header, conflicting_round, [k for k in keys if C.address_of(k[1]) in addrs],
                     sign=sign)
    byz = list(vals.validators[:signers]) if conflicting_round == 1 else None
    ev = Evidence(SignedHeader(conf_header, cm), vals, 10, byz, vals.total_voting_power())
    return ev, SignedHeader(trusted_header, flags_commit(vals, trusted_header, 1)), vals


def _bad_sig(ev, idx):
    ev = copy.deepcopy(ev)
    s = bytearray(ev.conflicting.commit.signatures[idx].signature)
    s[11] ^= 0x40
    ev.conflicting.commit.signatures[idx].signature = bytes(s)
    return ev


def _with(ev, **kw):
    ev = copy.copy(ev)
    for k, v in kw.items():
        setattr(ev, k, v)
    return ev


_SCENARIOS = {}


def scenarios(sign=None):
    """[(Case, code)]: code = the TMED_LCA_* outcome the case must give.  sign(seed, msg): the signer of
    every commit (default: the oracle's; the table is built once per signer)."""
    if sign in _SCENARIOS:
        return _SCENARIOS[sign]
    signer = sign or port.sign
    make_lunatic = lambda *a, **kw: globals()["make_lunatic"](*a, sign=signer, **kw)
    make_same_height = lambda *a, **kw: globals()["make_same_height"](*a, sign=signer, **kw)
    out = []

    def case(name, code, ev, chh, trusted, common_vals):
        out.append((Case(name, ev, chh, trusted, common_vals), code))

    # TestVerifyLightClientAttack_Lunatic (:30-65)
    ev, trusted, common = make_lunatic("lunatic")
    case("lunatic: good", E.LCA_OK, ev, 4, trusted, common)
    case("lunatic: same hash", E.LCA_SAME_HASH, ev, 4, ev.conflicting, common)
    case("lunatic: wrong total power", E.LCA_TOTAL_POWER, _with(ev, total_voting_power=10), 4, trusted, common)
    ev3, trusted3, common3 = make_lunatic("lunatic3", byz=3)
    case("lunatic: too few malicious votes", E.LCA_TRUSTING, ev3, 4, trusted3, common3)
    # TestVerify_ForwardLunaticAttack (:135-191)
    evf, trustedf, commonf = make_lunatic("forward", byz=5, phantom=5)
    tf = copy.deepcopy(trustedf)
    tf.header["height"], tf.header["time"] = 8, time_add(BTIME, 2 * HOUR)
    case("forward lunatic: time violated", E.LCA_OK, evf, 4, tf, commonf)
    told = copy.deepcopy(tf)
    told.header["time"] = BTIME
    case("forward lunatic: time not violated", E.LCA_TIME_NOT_VIOLATED, evf, 4, told, commonf)
    # TestVerifyLightClientAttack_Equivocation (:193-276)
    eve, trustede, valse = make_same_height("equivocation")
    case("equivocation: good", E.LCA_OK, eve, 10, trustede, valse)
    case("equivocation: same hash", E.LCA_SAME_HASH, eve, 10, SignedHeader(eve.conflicting.header, trustede.commit), valse)
    bad = copy.deepcopy(eve)
    bad.conflicting.header["next_validators_hash"] = h256("not derived")
    case("equivocation: changed NextValidatorsHash", E.LCA_NOT_DERIVED, bad, 10, trustede, valse)
    # TestVerifyLightClientAttack_Amnesia (:278-351)
    eva, trusteda, valsa = make_same_height("amnesia", signers=5, conflicting_round=0)
    case("amnesia: good", E.LCA_OK, eva, 10, trusteda, valsa)
    case("amnesia: same hash", E.LCA_SAME_HASH, eva, 10, SignedHeader(eva.conflicting.header, trusteda.commit), valsa)
    case("amnesia: a non-nil claimed list", E.LCA_AMNESIA_HAS_VALIDATORS, _with(eva, byz=[]), 10, trusteda, valsa)
    case("amnesia: a claimed validator", E.LCA_AMNESIA_HAS_VALIDATORS, _with(eva, byz=valsa.validators[:1]), 10, trusteda,
         valsa)
    # one per remaining code
    case("commit: wrong signature", E.LCA_COMMIT, _bad_sig(eve, 0), 10, trustede, valse)
    case("byz count", E.LCA_BYZ_COUNT, _with(ev, byz=ev.byz[:1]), 4, trusted, common)
    case("byz count: nil claimed", E.LCA_BYZ_COUNT, _with(ev, byz=None), 4, trusted, common)
    case("byz address: two entries swapped", E.LCA_BYZ_ADDRESS, _with(ev, byz=[ev.byz[1], ev.byz[0]] + ev.byz[2:]), 4, trusted,
         common)
    short = copy.copy(ev.byz[2])
    short.address = short.address[:19]
    case("byz address: 19 bytes", E.LCA_BYZ_ADDRESS, _with(ev, byz=ev.byz[:2] + [short] + ev.byz[3:]), 4, trusted, common)
    rich = copy.copy(ev.byz[3])
    rich.voting_power += 1 << 32
    case("byz power", E.LCA_BYZ_POWER, _with(ev, byz=ev.byz[:3] + [rich]), 4, trusted, common)
    late = copy.deepcopy(trusted)
    late.header["time"] = (253402300800, 0)
    case("go path: a header time outside the Timestamp range", E.LCA_GO_PATH, ev, 4, late, common)
    # varied powers: the order is power descending, then address
    evv, trustedv, commonv = make_lunatic("varied", total=9, byz=5, phantom=4, inc=7)
    case("lunatic: varied powers", E.LCA_OK, evv, 4, trustedv, commonv)
    evq, trustedq, valsq = make_same_height("equivocation-varied", n=7, signers=6, inc=3)
    evq = _with(evq, byz=sorted(evq.byz, key=lambda v: (-v.voting_power, v.address)))
    case("equivocation: varied powers", E.LCA_OK, evq, 10, trustedq, valsq)
    # different heights but a derived header: the Trusting check runs, the list is an equivocation's
    case("equivocation at another common height", E.LCA_OK, eve, 9, trustede, valse)
    # ordering pairs: two failing checks, the earlier one wins
    case("go path before not derived", E.LCA_GO_PATH, bad, 10, SignedHeader(late.header, trustede.commit), valse)
    case("not derived before a bad commit", E.LCA_NOT_DERIVED, _bad_sig(bad, 0), 10, trustede, valse)
    case("trusting before commit", E.LCA_TRUSTING, _bad_sig(ev3, 0), 4, trusted3, common3)
    case("commit before total power", E.LCA_COMMIT, _with(_bad_sig(eve, 1), total_voting_power=1), 10, trustede, valse)
    case("total power before same hash", E.LCA_TOTAL_POWER, _with(ev, total_voting_power=7), 4, ev.conflicting, common)
    case("total power before time", E.LCA_TOTAL_POWER, _with(evf, total_voting_power=1), 4, told, commonf)
    case("time before byz count", E.LCA_TIME_NOT_VIOLATED, _with(evf, byz=evf.byz[:1]), 4, told, commonf)
    case("same hash before byz count", E.LCA_SAME_HASH, _with(ev, byz=ev.byz[:1]), 4, ev.conflicting, common)
    case("byz count before byz address", E.LCA_BYZ_COUNT, _with(ev, byz=[ev.byz[1], ev.byz[0]]), 4, trusted, common)
    both = copy.copy(ev.byz[1])
    both.address, both.voting_power = ev.byz[0].address, 77
    case("byz address before byz power at one index", E.LCA_BYZ_ADDRESS, _with(ev, byz=[ev.byz[0], both] + ev.byz[2:]), 4,
         trusted, common)
    poor = copy.copy(ev.byz[0])
    poor.voting_power = 3
    case("the lower index wins: power at 0, address at 1", E.LCA_BYZ_POWER, _with(ev, byz=[poor, both] + ev.byz[2:]), 4,
         trusted, common)
    # panics
    mal = copy.deepcopy(eve)
    mal.conflicting.commit.block_id = C.BlockID(mal.conflicting.commit.block_id.hash[:31], 1000, PSH)
    case("panic: a malformed BlockID hash in the commit check", E.LCA_PANIC, mal, 10, trustede, valse)
    shorter = SignedHeader(trustede.header, copy.deepcopy(trustede.commit))
    del shorter.commit.signatures[3:]
    case("panic: the trusted commit is shorter", E.LCA_PANIC, eve, 10, shorter, valse)
    stranger = copy.deepcopy(eve)
    stranger.conflicting.commit.signatures[1].address = h256("nobody")[:20]
    case("panic: a lookup finds nobody in a list of four", E.LCA_PANIC, stranger, 10, trustede, valse)
    one = SignedHeader(trustede.header, flags_commit(valse, trustede.header, 1,
                                                     [C.FLAG_ABSENT, C.FLAG_COMMIT] + [C.FLAG_ABSENT] * 3))
    case("panic: one nil entry against one claimed", E.LCA_PANIC, _with(stranger, byz=eve.byz[:1]), 10, one, valse)
    case("one nil entry against two claimed", E.LCA_BYZ_COUNT, _with(stranger, byz=eve.byz[:2]), 10, one, valse)
    case("one nil entry against a nil list", E.LCA_BYZ_COUNT, _with(stranger, byz=None), 10, one, valse)
    case("one found entry", E.LCA_OK, _with(eve, byz=[valse.validators[1]]), 10, one, valse)
    absent = SignedHeader(trustede.header, flags_commit(valse, trustede.header, 1, [C.FLAG_ABSENT] * 5))
    case("an all-absent trusted commit: a nil list", E.LCA_OK, _with(eve, byz=None), 10, absent, valse)
    case("an all-absent trusted commit, an empty claimed list", E.LCA_AMNESIA_HAS_VALIDATORS, _with(eve, byz=[]), 10, absent,
         valse)
    _SCENARIOS[sign] = out
    return out


# A hand-written Hash(): the header hash 01 02 .. 20 (hex), CommonHeight 64.  Zigzag: 64 << 1 = 128 = varint
# 80 01.  The buffer is the first 31 bytes 01 .. 1f, a zero byte, 80 01: 34 bytes.
ANCHOR = (bytes(range(1, 33)), 64, bytes.fromhex("169ea01220043b69ad12a0996227474e2a968dab0c12236e5579980ab893087d"))
# A nil header hash, CommonHeight 1: 32 zero bytes and 02.
ANCHOR_NIL = (None, 1, bytes.fromhex("58cc2f44d3a27866874701fbad573da9ad1cfd88fa3145531c822f20a58beea1"))
