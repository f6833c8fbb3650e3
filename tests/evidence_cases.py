"""DuplicateVoteEvidence (test helper): a Python restatement of DuplicateVoteEvidence.Bytes()
(the generated marshallers proto/tendermint/types/evidence.pb.go:449-497 and types.pb.go:1431-1489,
:1153-1171, :1233-1256, written with Python integers and bytes), of DuplicateVoteEvidence.Hash /
EvidenceList.Hash (types/evidence.go:90-103, :431-442) and of VerifyDuplicateVote
(evidence/verify.go:162-222) as a function returning the seam's code, over hashlib, oracle.merkle,
oracle.signbytes and oracle.ed25519_go; and the corpus the host and device tests share
(tests/test_evidence_host.py, tests/test_gpu_evidence.py)."""
import hashlib

from oracle import ed25519_go as E
from oracle import merkle as M
from oracle.signbytes import timestamp_body, uvarint

import tmed.evidence as EV
import tmed.types as T
import tmed.votes as V
import vote_cases as VC

CHAIN = VC.CHAIN
T0 = VC.T0
MIN_SECONDS, MAX_SECONDS = VC.MIN_SECONDS, VC.MAX_SECONDS
I32_MIN, I32_MAX, I64_MIN, I64_MAX = -2**31, 2**31 - 1, -2**63, 2**63 - 1


# ----------------------------------------------------------------------------- Bytes()

def _varint_field(tag, v):
    """A varint field of an int32 / int64 / uint32: omitted at zero; Go converts to uint64 first."""
    return b"" if v == 0 else bytes([tag]) + uvarint(v)


def _bytes_field(tag, b):
    return b"" if len(b) == 0 else bytes([tag]) + uvarint(len(b)) + bytes(b)


def _msg_field(tag, body):
    """A non-nullable embedded message: always there, an empty body included."""
    return bytes([tag]) + uvarint(len(body)) + body


def vote_proto(v: V.Vote) -> bytes:
    """tmproto.Vote.Marshal (types.pb.go:1431-1489), fields ascending."""
    b = v.block_id
    psh = _varint_field(0x08, b.psh_total) + _bytes_field(0x12, b.psh_hash)          # :1233-1256
    bid = _bytes_field(0x0A, b.hash) + _msg_field(0x12, psh)                         # :1153-1171
    return (_varint_field(0x08, v.type) + _varint_field(0x10, v.height) + _varint_field(0x18, v.round) +
            _msg_field(0x22, bid) + _msg_field(0x2A, timestamp_body(*v.timestamp)) +
            _bytes_field(0x32, v.validator_address) + _varint_field(0x38, v.validator_index) +
            _bytes_field(0x42, v.signature))


def carried(e: EV.DuplicateVoteEvidence) -> bool:
    """What tmed_dup_evidence can reproduce (ev_ok): hashes <= 32, addresses <= 20, signatures <= 64 and
    three timestamps StdTimeMarshal accepts."""
    for v in (e.vote_a, e.vote_b):
        if (len(v.block_id.hash) > 32 or len(v.block_id.psh_hash) > 32 or len(v.validator_address) > 20 or
                len(v.signature) > 64 or not VC.time_encodable(v.timestamp)):
            return False
    return VC.time_encodable(e.timestamp)


def evidence_bytes(e: EV.DuplicateVoteEvidence) -> bytes:
    """DuplicateVoteEvidence.Bytes() (evidence.pb.go:449-497)."""
    return (_msg_field(0x0A, vote_proto(e.vote_a)) + _msg_field(0x12, vote_proto(e.vote_b)) +
            _varint_field(0x18, e.total_voting_power) + _varint_field(0x20, e.validator_power) +
            _msg_field(0x2A, timestamp_body(*e.timestamp)))


def evidence_hash(e) -> bytes:
    return hashlib.sha256(evidence_bytes(e)).digest()


def list_hash(items) -> bytes:
    """EvidenceList.Hash over byte strings (an evidence's Bytes() or an opaque item)."""
    return M.hash_from_byte_slices([bytes(b) for b in items])


# ----------------------------------------------------------------------------- VerifyDuplicateVote

def _equal3(a: bytes, b: bytes, cap: int):
    """bytes.Equal as the structs see it: None where both have the same length above cap (not carried)."""
    if len(a) != len(b):
        return False
    if len(a) > cap:
        return None
    return bytes(a) == bytes(b)


def block_ids_equal(a: T.BlockID, b: T.BlockID):
    """BlockID.Equals (types/block.go:1170-1173): False as soon as one comparison is, else None if one is unknown."""
    h, p = _equal3(a.hash, b.hash, 32), _equal3(a.psh_hash, b.psh_hash, 32)
    if h is False or p is False or a.psh_total != b.psh_total:
        return False
    return None if (h is None or p is None) else True


def get_by_address(vals: T.ValidatorSet, addr: bytes):
    """ValidatorSet.GetByAddress (types/validator_set.go:270-278): the first match in index order."""
    for i, val in enumerate(vals.validators):
        if bytes(val.address) == bytes(addr):
            return i
    return None


def _vote_state(chain_id, v):
    if VC.sign_bytes(chain_id, v) is None:
        return EV.DUPVOTE_PANIC
    if not VC.time_encodable(v.timestamp):
        return EV.DUPVOTE_GO_PATH
    return 0


def pre_code(req: EV.EvidenceRequest, e: EV.DuplicateVoteEvidence):
    """(the first failing check of 1-7 or GO_PATH at check 4, else 0; the found validator or None)."""
    a, b = e.vote_a, e.vote_b
    found = get_by_address(req.vals, a.validator_address)
    if found is None:                                                      # verify.go:163-166
        return EV.DUPVOTE_NOT_A_VALIDATOR, None
    val = req.vals.validators[found]
    if (a.height, a.round, a.type) != (b.height, b.round, b.type):         # :170-176
        return EV.DUPVOTE_HRS_MISMATCH, found
    if bytes(a.validator_address) != bytes(b.validator_address):           # :179-184
        return EV.DUPVOTE_ADDRESS_MISMATCH, found
    same = block_ids_equal(a.block_id, b.block_id)                         # :187-192
    if same is True:
        return EV.DUPVOTE_SAME_BLOCK_ID, found
    if same is None:
        return EV.DUPVOTE_GO_PATH, found
    if T.address_of(val.pub_key) != bytes(a.validator_address):            # :195-199
        return EV.DUPVOTE_ADDRESS_NOT_OF_KEY, found
    if val.voting_power != e.validator_power:                              # :202-205
        return EV.DUPVOTE_VALIDATOR_POWER, found
    if req.vals.total_voting_power() != e.total_voting_power:              # :206-209
        return EV.DUPVOTE_TOTAL_POWER, found
    return 0, found


def expected(req: EV.EvidenceRequest, e: EV.DuplicateVoteEvidence) -> int:
    """VerifyDuplicateVote's outcome as the seam's code."""
    pre, found = pre_code(req, e)
    if pre:
        return pre
    key = req.vals.validators[found].pub_key
    for v, bad in ((e.vote_a, EV.DUPVOTE_VOTE_A_SIGNATURE), (e.vote_b, EV.DUPVOTE_VOTE_B_SIGNATURE)):   # :211-219
        st = _vote_state(req.chain_id, v)
        if st:
            return st
        if len(v.signature) != 64 or not E.verify(key, VC.sign_bytes(req.chain_id, v), bytes(v.signature)):
            return bad
    return EV.DUPVOTE_OK


def host_view(req, e):
    """What tmed_verify_duplicate_votes_host reports: (pre, state A, state B, found or -1, len A, len B)."""
    pre, found = pre_code(req, e)
    st = [_vote_state(req.chain_id, v) for v in (e.vote_a, e.vote_b)]
    lens = [0 if (pre or s) else len(VC.sign_bytes(req.chain_id, v)) for v, s in zip((e.vote_a, e.vote_b), st)]
    return pre, st[0], st[1], -1 if found is None else found, lens[0], lens[1]


# ----------------------------------------------------------------------------- building evidence

_KEYS = {}


def valset(n, tag="ev", **kw):
    """VC.valset with the keys of a tag made once (sets of several sizes are prefixes of one key list)."""
    have = _KEYS.setdefault(tag, [])
    while len(have) < n:
        s = VC.seed_of(tag, len(have))
        have.append((s, E.pubkey_from_seed(s)))
    vals = [T.Validator(pk, 10 + i) for i, (_, pk) in enumerate(have[:n])]
    w = kw.get("wrong_address_at")
    if w is not None:
        vals[w].address = hashlib.sha256(b"wrong" + tag.encode()).digest()[:20]
    return T.ValidatorSet(vals), [s for s, _ in have[:n]]


def dup(chain_id, vals, seeds, idx, k=0, type_=1, height=7, round_=2, bid_a=None, bid_b=None, ts_a=None, ts_b=None,
        signer=None):
    """A valid duplicate-vote evidence of validator idx (k: varies BlockIDs and times).  signer: the votes
    carry validator idx's address but are signed by (and carry the index of) validator `signer`."""
    bid_a = VC.block_id("a%d" % k) if bid_a is None else bid_a
    bid_b = VC.block_id("b%d" % k) if bid_b is None else bid_b
    ts_a = ts_a or (T0[0] + k, (T0[1] + 7919 * k) % 10**9)
    ts_b = ts_b or (T0[0] + k + 1, (T0[1] + 104729 * k) % 10**9)
    s = idx if signer is None else signer
    a = VC.signed(chain_id, vals, seeds, s, type_, height, round_, bid_a, ts_a)
    b = VC.signed(chain_id, vals, seeds, s, type_, height, round_, bid_b, ts_b)
    a.validator_address = b.validator_address = vals.validators[idx].address
    return EV.DuplicateVoteEvidence(a, b, vals.total_voting_power(), vals.validators[idx].voting_power,
                                    (T0[0] + 100 + k, k))


def _edit(o, **kw):
    for f, x in kw.items():
        setattr(o, f, x)
    return o


def check_cases(chain_id, vals, seeds, tag="c"):
    """(name, evidence) over one set: one case per code, the ordering pairs, the first-match cases and
    the address lengths.  `vals` may hold a validator whose stored address is not its key's hash
    (wrong_address_at) and, from repeated(), an address that occurs twice."""
    n = len(seeds)
    cnt = iter(range(10**6))
    good = [i for i, val in enumerate(vals.validators)
            if val.address == T.address_of(val.pub_key) and get_by_address(vals, val.address) == i]

    def ok(idx=None, **kw):
        k = next(cnt)
        return dup(chain_id, vals, seeds, good[k % len(good)] if idx is None else idx, k, **kw)

    def a(e, **kw):
        _edit(e.vote_a, **kw)
        return e

    def b(e, **kw):
        _edit(e.vote_b, **kw)
        return e

    bid = VC.block_id(tag)
    h33, h34 = bid.hash + b"\x01", bid.hash + b"\x01\x02"
    bad_hash = T.BlockID(bid.hash[:31], 123, bid.psh_hash)
    cases = [
        ("valid", ok()),
        ("valid, VoteA for nil", ok(bid_a=T.BlockID())),
        ("valid, VoteB for nil", ok(bid_b=T.BlockID())),
        ("valid, only the totals differ", ok(bid_a=T.BlockID(bid.hash, 1, bid.psh_hash), bid_b=T.BlockID(bid.hash, 2, bid.psh_hash))),
        ("valid, only the part-set hashes differ", ok(bid_a=bid, bid_b=T.BlockID(bid.hash, 123, bid.hash))),
        ("valid, precommits at the first validator", ok(idx=good[0], type_=2)),
        ("valid, the last validator", ok(idx=good[-1])),
        ("valid, other validator indexes in the votes", (lambda e: b(a(e, validator_index=n + 5), validator_index=-3))(ok())),
        # 1
        ("1: nobody has the address", (lambda e: b(a(e, validator_address=b"\x07" * 20), validator_address=b"\x07" * 20))(ok())),
        ("1: address length 19", (lambda e: a(e, validator_address=e.vote_a.validator_address[:19]))(ok())),
        ("1: address length 21", (lambda e: a(e, validator_address=e.vote_a.validator_address + b"\x00"))(ok())),
        ("1: address empty", a(ok(), validator_address=b"")),
        # 2
        ("2: heights differ", b(ok(), height=8)),
        ("2: rounds differ", b(ok(), round=3)),
        ("2: types differ", b(ok(), type=2)),
        # 3
        ("3: VoteB names another validator", b(ok(idx=good[0]), validator_address=vals.validators[good[1]].address)),
        ("3: VoteB address length 19", (lambda e: b(e, validator_address=e.vote_b.validator_address[:19]))(ok())),
        ("3: VoteB address length 21", (lambda e: b(e, validator_address=e.vote_b.validator_address + b"\x00"))(ok())),
        ("3: VoteB address empty", b(ok(), validator_address=b"")),
        # 4
        ("4: the same BlockID", ok(bid_a=bid, bid_b=T.BlockID(bytes(bid.hash), 123, bytes(bid.psh_hash)))),
        ("4: both for nil (nil equals empty)", ok(bid_a=T.BlockID(), bid_b=T.BlockID(b"", 0, bytearray()))),
        ("4: the same malformed BlockID", ok(bid_a=bad_hash, bid_b=T.BlockID(bid.hash[:31], 123, bid.psh_hash))),
        # 11 (b) and its determined neighbours
        ("11: hashes of 33 bytes on both sides", ok(bid_a=T.BlockID(h33, 123, bid.psh_hash), bid_b=T.BlockID(h33, 123, bid.psh_hash))),
        ("11: part-set hashes of 40 bytes on both sides", ok(bid_a=T.BlockID(bid.hash, 1, b"\x05" * 40), bid_b=T.BlockID(bid.hash, 1, b"\x06" * 40))),
        ("8: hashes of 33 and 34 bytes differ, then VoteA panics", ok(bid_a=T.BlockID(h33, 123, bid.psh_hash), bid_b=T.BlockID(h34, 123, bid.psh_hash))),
        ("8: hashes of 33 bytes but the totals differ, then VoteA panics", ok(bid_a=T.BlockID(h33, 1, bid.psh_hash), bid_b=T.BlockID(h33, 2, bid.psh_hash))),
        ("8: hashes of 300 and 556 bytes differ", ok(bid_a=T.BlockID(b"\x01" * 300, 1, b""), bid_b=T.BlockID(b"\x01" * 556, 1, b""))),
        # 6, 7
        ("6: validator power", _edit(ok(), validator_power=9)),
        ("7: total power", (lambda e: _edit(e, total_voting_power=e.total_voting_power + 1))(ok())),
        # 8
        ("8: VoteA malformed", ok(bid_a=bad_hash)),
        ("8: VoteB malformed, VoteA valid", ok(bid_b=T.BlockID(bid.hash, 123, bid.psh_hash[:5]))),
        # 11 (a)
        ("11: VoteA's time out of range", ok(ts_a=(MAX_SECONDS, 0))),
        ("11: VoteB's nanos negative, VoteA valid", ok(ts_b=(T0[0], -1))),
        ("ok: the evidence's own time out of range is not read", _edit(ok(), timestamp=(MAX_SECONDS, 0))),
        # 9, 10
        ("9: VoteA flipped", (lambda e: a(e, signature=VC.flip(e.vote_a.signature, 3)))(ok())),
        ("9: VoteA 63 bytes", (lambda e: a(e, signature=e.vote_a.signature[:63]))(ok())),
        ("9: VoteA bad, VoteB malformed", (lambda e: a(e, signature=VC.flip(e.vote_a.signature, 40)))(ok(bid_b=bad_hash))),
        ("9: VoteA bad, VoteB bad", (lambda e: b(a(e, signature=VC.flip(e.vote_a.signature, 1)), signature=VC.flip(e.vote_b.signature, 1)))(ok())),
        ("10: VoteB flipped", (lambda e: b(e, signature=VC.flip(e.vote_b.signature, 33)))(ok())),
        ("10: VoteB 63 bytes", (lambda e: b(e, signature=e.vote_b.signature[:63]))(ok())),
        ("10: VoteB empty signature", b(ok(), signature=b"")),
        ("9: signed by the key at validator_index, not by the address's validator", ok(idx=good[0], signer=good[1])),
        # two checks fail: the earlier one wins
        ("pair 2+3", (lambda e: b(e, height=9, validator_address=vals.validators[good[0]].address))(ok(idx=good[1]))),
        ("pair 4+6", _edit(ok(bid_a=bid, bid_b=bid), validator_power=1)),
        ("pair 6+7", _edit(ok(), validator_power=1, total_voting_power=1)),
        ("pair 8+10: VoteA malformed, VoteB bad", (lambda e: b(e, signature=VC.flip(e.vote_b.signature, 9)))(ok(bid_a=bad_hash))),
        ("pair 1+2", (lambda e: b(a(e, validator_address=b"\x09" * 20), round=5))(ok())),
        ("pair 7+9", (lambda e: a(_edit(e, total_voting_power=0), signature=bytes(64)))(ok())),
    ]
    wrong = [i for i, val in enumerate(vals.validators) if val.address != T.address_of(val.pub_key)
             and get_by_address(vals, val.address) == i]
    if wrong:
        cases.append(("5: the set's address is not the key's", ok(idx=wrong[0])))
        cases.append(("pair 5+6", _edit(ok(idx=wrong[0]), validator_power=3)))
        cases.append(("pair 4+5", ok(idx=wrong[0], bid_a=bid, bid_b=bid)))
    rep = [(get_by_address(vals, val.address), i) for i, val in enumerate(vals.validators)
           if get_by_address(vals, val.address) != i]
    for first, later in rep[:1]:  # the later validator shares the first one's address: the first decides
        cases.append(("first match: the first validator's own evidence", ok(idx=first)))
        e = ok(idx=first, signer=later)
        cases.append(("first match: signed by the later one, the first one's power: 9", e))
        e = ok(idx=first, signer=later)
        e.validator_power = vals.validators[later].voting_power
        cases.append(("first match: the later one's power: 6", e))
    return cases


def repeated(vals, first, later):
    """The same set with validator `later` holding validator `first`'s address."""
    vs = [T.Validator(v.pub_key, v.voting_power, 0, v.address) for v in vals.validators]
    vs[later].address = vs[first].address
    return T.ValidatorSet(vs)


def main_request(tag="evmain"):
    """One request over a 9-validator set with a wrong stored address (validator 7) and a repeated one
    (validator 5 holds validator 2's): every case of check_cases.  Returns (request, names)."""
    vals, seeds = valset(9, tag, wrong_address_at=7)
    vals = repeated(vals, 2, 5)
    cs = check_cases(CHAIN, vals, seeds, tag)
    return EV.EvidenceRequest(CHAIN, vals, [e for _, e in cs]), [n for n, _ in cs]


# ----------------------------------------------------------------------------- the Bytes() sweep

def _v(type_=0, height=0, round_=0, bid=None, ts=(0, 0), addr=b"", index=0, sig=b""):
    return V.Vote(type_, height, round_, bid or T.BlockID(), ts, addr, index, sig)


def bytes_sweep():
    """(name, evidence) for tmed_evidence_bytes / tmed_evidence_hashes: every field at zero, the varint
    edges, the timestamps, hashes and addresses empty and full, VoteB's signature length over 0..64 and
    the longest Bytes() there is (505 bytes: bound_case() says why not 520); then the evidences the struct
    cannot reproduce."""
    H, P = bytes(0xA0 + i for i in range(32)), bytes(0x10 + i for i in range(32))
    A20, S64 = bytes(0x40 + i for i in range(20)), bytes(0x80 + i for i in range(64))
    out = [("all zero", EV.DuplicateVoteEvidence(_v(), _v(), 0, 0, (0, 0)))]
    edges = [127, 128, 16383, 16384, 2**31 - 1, -1]
    for x in edges + [I64_MIN, I64_MAX]:
        out.append(("height and powers %d" % x, EV.DuplicateVoteEvidence(_v(height=x), _v(), x, -x if x != I64_MIN else x, (0, 0))))
    for x in edges + [I32_MIN, I32_MAX]:
        out.append(("round %d" % x, EV.DuplicateVoteEvidence(_v(), _v(round_=x), 0, 0, (0, 0))))
        out.append(("type %d" % x, EV.DuplicateVoteEvidence(_v(type_=x), _v(), 0, 0, (0, 0))))
        out.append(("index %d" % x, EV.DuplicateVoteEvidence(_v(index=x), _v(index=-x if x != I32_MIN else x), 0, 0, (0, 0))))
    for x in [127, 128, 16383, 16384, 2**31 - 1, 2**32 - 1]:
        out.append(("total %d" % x, EV.DuplicateVoteEvidence(_v(bid=T.BlockID(b"", x, b"")), _v(bid=T.BlockID(H, x, P)), 0, 0, (0, 0))))
    for s in (0, 1, -1, MIN_SECONDS, MAX_SECONDS - 1):
        for ns in (0, 1, 999999999):
            out.append(("time %d.%d" % (s, ns), EV.DuplicateVoteEvidence(_v(ts=(s, ns)), _v(ts=(ns, 0)), 0, 0, (s, ns))))
    for hl, pl, al in ((0, 0, 0), (32, 0, 0), (0, 32, 0), (0, 0, 20), (32, 32, 20), (1, 31, 19), (31, 1, 1)):
        out.append(("lengths %d %d %d" % (hl, pl, al),
                    EV.DuplicateVoteEvidence(_v(bid=T.BlockID(H[:hl], 5, P[:pl]), addr=A20[:al], sig=S64),
                                             _v(bid=T.BlockID(P[:hl], 0, H[:pl]), addr=A20[:al]), 1, 2, T0)))
    full = lambda sl: EV.DuplicateVoteEvidence(  # noqa: E731
        _v(1, 12345, 2, T.BlockID(H, 123, P), T0, A20, 17, S64), _v(1, 12345, 2, T.BlockID(P, 7, H), T0, A20, 17, S64[:sl]),
        1000, 10, (T0[0] + 5, 1))
    for sl in range(65):  # 65 consecutive lengths: every residue of the SHA-256 block boundary
        out.append(("VoteB signature of %d bytes" % sl, full(sl)))
    # the longest timestamp StdTimeMarshal accepts: negative seconds (ten bytes), nanos 999,999,999 (five)
    worst = lambda: _v(-1, -1, -1, T.BlockID(H, 2**32 - 1, P), (-1, 999999999), A20, -1, S64)  # noqa: E731
    out.append(("worst case", EV.DuplicateVoteEvidence(worst(), worst(), -1, -1, (-1, 999999999))))
    # what the struct cannot reproduce (ev_ok = 0), one cause each
    bad = [
        ("not carried: VoteA hash of 33 bytes", EV.DuplicateVoteEvidence(_v(bid=T.BlockID(H + b"\x00", 0, b"")), _v(), 0, 0, (0, 0))),
        ("not carried: VoteB part-set hash of 33 bytes", EV.DuplicateVoteEvidence(_v(), _v(bid=T.BlockID(b"", 0, P + b"\x00")), 0, 0, (0, 0))),
        ("not carried: VoteA address of 21 bytes", EV.DuplicateVoteEvidence(_v(addr=A20 + b"\x00"), _v(), 0, 0, (0, 0))),
        ("not carried: VoteB signature of 65 bytes", EV.DuplicateVoteEvidence(_v(), _v(sig=S64 + b"\x00"), 0, 0, (0, 0))),
        ("panic: VoteA seconds at the range's end", EV.DuplicateVoteEvidence(_v(ts=(MAX_SECONDS, 0)), _v(), 0, 0, (0, 0))),
        ("panic: VoteB seconds before the range", EV.DuplicateVoteEvidence(_v(), _v(ts=(MIN_SECONDS - 1, 0)), 0, 0, (0, 0))),
        ("panic: VoteA nanos -1", EV.DuplicateVoteEvidence(_v(ts=(0, -1)), _v(), 0, 0, (0, 0))),
        ("panic: the evidence's nanos 1e9", EV.DuplicateVoteEvidence(_v(), _v(), 0, 0, (0, 10**9))),
        ("panic: the evidence's seconds at the range's end", EV.DuplicateVoteEvidence(_v(), _v(), 0, 0, (MAX_SECONDS, 0))),
    ]
    return out, bad


def bound_case():
    """The record of the 520-byte bound the kernel's slot is sized to: every field at its longest and the
    three timestamps at nanos -1 (ten bytes).  No Bytes() reaches it, since StdTimeMarshal refuses such a
    timestamp (the longest that is accepted gives the 505 bytes of bytes_sweep's worst case); the encoder
    itself is run on it by tests/native/evidence_host.cpp."""
    H, P = bytes(0xA0 + i for i in range(32)), bytes(0x10 + i for i in range(32))
    A20, S64 = bytes(0x40 + i for i in range(20)), bytes(0x80 + i for i in range(64))
    v = lambda: _v(-1, -1, -1, T.BlockID(H, 2**32 - 1, P), (-1, -1), A20, -1, S64)  # noqa: E731
    return EV.DuplicateVoteEvidence(v(), v(), -1, -1, (-1, -1))
