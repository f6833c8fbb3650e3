"""Free-standing votes (test helper): a Python restatement of the checks VoteSet.addVote runs in
front of the signature (types/vote_set.go:156-218) and of Vote.Verify (types/vote.go:147-156), over
oracle.signbytes.vote_sign_bytes and oracle.ed25519_go, and the corpus the host and device tests of
tmed_verify_votes share (tests/test_votes_host.py, tests/test_gpu_votes.py)."""
import hashlib
import itertools

from oracle import ed25519_go as E
from oracle.signbytes import vote_sign_bytes

import tmed.types as T
import tmed.votes as V

CHAIN = "test_chain_id"
T0 = (1700000000, 123456789)
MIN_SECONDS, MAX_SECONDS = -62135596800, 253402300800  # google.protobuf.Timestamp's range


def seed_of(tag, i):
    return hashlib.sha256(("%s-%d" % (tag, i)).encode()).digest()


def block_id(tag="block"):
    return T.BlockID(hashlib.sha256(tag.encode()).digest(), 123, hashlib.sha256((tag + "/psh").encode()).digest())


def valset(n, tag="votes", wrong_address_at=None):
    """n validators (index order as given) and their seeds.  wrong_address_at: that validator's stored
    address is not its key's hash (a set the reference would accept from a bad genesis file)."""
    seeds = [seed_of(tag, i) for i in range(n)]
    vals = [T.Validator(E.pubkey_from_seed(s), 10 + i) for i, s in enumerate(seeds)]
    if wrong_address_at is not None:
        vals[wrong_address_at].address = hashlib.sha256(b"wrong" + tag.encode()).digest()[:20]
    return T.ValidatorSet(vals), seeds


# ----------------------------------------------------------------------------- the restatement

def malformed(b: T.BlockID):
    return len(b.hash) not in (0, 32) or len(b.psh_hash) not in (0, 32)


def sign_bytes(chain_id, v: V.Vote):
    """VoteSignBytes(chainID, vote); None where CanonicalizeBlockID panics."""
    if malformed(v.block_id):
        return None
    b = v.block_id
    return vote_sign_bytes(chain_id, v.type, v.height, v.round, (bytes(b.hash), b.psh_total, bytes(b.psh_hash)),
                           v.timestamp)


def time_encodable(ts):
    return MIN_SECONDS <= ts[0] < MAX_SECONDS and 0 <= ts[1] < 10**9


def expected(req: V.VoteRequest, v: V.Vote) -> int:
    """The first check that fails, in the reference's order; VOTE_OK when none does."""
    vals = req.vals.validators
    if v.validator_index < 0:                                           # vote_set.go:165
        return V.VOTE_INDEX_NEGATIVE
    if req.addvote and len(v.validator_address) == 0:                   # :167
        return V.VOTE_ADDRESS_EMPTY
    if req.addvote and (v.height, v.round, v.type) != (req.height, req.round, req.type):  # :172-178
        return V.VOTE_UNEXPECTED_STEP
    if v.validator_index >= len(vals):                                  # :181-186
        return V.VOTE_INDEX_NOT_IN_SET
    val = vals[v.validator_index]
    if req.addvote and bytes(v.validator_address) != bytes(val.address):  # :189-194 (bytes.Equal)
        return V.VOTE_ADDRESS_NOT_IN_SET
    if T.address_of(val.pub_key) != bytes(v.validator_address):         # vote.go:148
        return V.VOTE_ADDRESS_NOT_OF_KEY
    msg = sign_bytes(req.chain_id, v)
    if msg is None:                                                     # canonical.go:19-22
        return V.VOTE_PANIC
    if not time_encodable(v.timestamp):                                 # StdTimeMarshal refuses: vote.go:95-98
        return V.VOTE_GO_PATH
    if len(v.signature) != 64 or not E.verify(val.pub_key, msg, bytes(v.signature)):  # vote.go:152
        return V.VOTE_INVALID_SIGNATURE
    return V.VOTE_OK


# ----------------------------------------------------------------------------- building votes

def signed(chain_id, vals, seeds, idx, type_, height, round_, bid, ts=T0, sign_as=None):
    """A vote of validator idx, signed over its own sign-bytes (sign_as: over another vote's)."""
    v = V.Vote(type_, height, round_, bid, ts, vals.validators[idx].address if 0 <= idx < len(seeds) else b"\x00" * 20,
               idx)
    msg = sign_bytes(chain_id, sign_as or v)
    if msg is not None and 0 <= idx < len(seeds):
        v.signature = E.sign(seeds[idx], msg)
    else:
        v.signature = bytes(64)
    return v


def flip(sig, byte):
    s = bytearray(sig)
    s[byte] ^= 1
    return bytes(s)


def step_cases(chain_id, vals, seeds, type_, height=7, round_=2, tag="c"):
    """(name, vote) for one ADDVOTE request at the step (height, round, type_): one vote per class, the
    pairs in which two checks fail, and the cases built for PANIC and GO_PATH.  A validator of `vals`
    may hold a stored address that is not its key's hash (valset(wrong_address_at=...)): votes that do not
    name a validator are spread over the others."""
    n = len(seeds)
    bid = block_id(tag)
    k = itertools.count()
    good = [i for i, val in enumerate(vals.validators) if val.address == T.address_of(val.pub_key)]

    def ok(idx=None, b=bid, ts=None, **kw):
        i = next(k)
        return signed(chain_id, vals, seeds, good[i % len(good)] if idx is None else idx, type_, height, round_, b,
                      ts or (T0[0] + i, (T0[1] + 7919 * i) % 10**9), **kw)

    def edit(v, **kw):
        for f, x in kw.items():
            setattr(v, f, x)
        return v

    bad_hash = T.BlockID(bid.hash[:31], 123, bid.psh_hash)
    bad_psh = T.BlockID(bid.hash, 123, bid.psh_hash[:5])
    other = V.Vote(type_, height, round_, bid, (T0[0] - 1, 5), b"", 0)
    cases = [
        ("valid", ok()),
        ("valid nil vote", ok(b=T.BlockID())),
        ("valid, hash only", ok(b=T.BlockID(bid.hash, 0, b""))),
        ("valid, part-set hash only", ok(b=T.BlockID(b"", 0, bid.psh_hash))),
        ("valid, total only", ok(b=T.BlockID(b"", 9, b""))),
        ("valid, zero time", ok(ts=T.ZERO_TIME)),
        ("flipped R", (lambda v: edit(v, signature=flip(v.signature, 3)))(ok())),
        ("flipped S", (lambda v: edit(v, signature=flip(v.signature, 40)))(ok())),
        ("flipped message", ok(sign_as=other)),
        ("sig_len 0", edit(ok(), signature=b"")),
        ("sig_len 63", (lambda v: edit(v, signature=v.signature[:63]))(ok())),
        ("index negative", edit(ok(), validator_index=-1)),
        ("address empty", edit(ok(), validator_address=b"")),
        ("wrong height", edit(ok(), height=height + 1)),
        ("wrong round", edit(ok(), round=round_ + 1)),
        ("wrong type", edit(ok(), type=3 - type_)),
        ("index == n", edit(ok(), validator_index=n)),
        ("index far past n", edit(ok(), validator_index=2**31 - 1)),
        ("address of another validator", edit(ok(idx=0), validator_address=vals.validators[1].address)),
        ("address length 19", (lambda v: edit(v, validator_address=v.validator_address[:19]))(ok())),
        ("address length 21", (lambda v: edit(v, validator_address=v.validator_address + b"\x00"))(ok())),
        ("panic: hash of 31 bytes", ok(b=bad_hash)),
        ("panic: part-set hash of 5 bytes", ok(b=bad_psh)),
        ("panic: hash of 33 bytes", ok(b=T.BlockID(bid.hash + b"\x01", 123, bid.psh_hash))),
        ("go path: seconds past the range", ok(ts=(MAX_SECONDS, 0))),
        ("go path: seconds before the range", ok(ts=(MIN_SECONDS - 1, 0))),
        ("go path: negative nanos", ok(ts=(T0[0], -1))),
        ("go path: nanos 1e9", ok(ts=(T0[0], 10**9))),
        # two checks fail: the earlier one wins
        ("pair: index negative + address empty", edit(ok(), validator_index=-1, validator_address=b"")),
        ("pair: address empty + wrong step", edit(ok(), validator_address=b"", height=height + 1)),
        ("pair: wrong step + index == n", edit(ok(), round=round_ + 5, validator_index=n)),
        ("pair: index == n + malformed", edit(ok(b=bad_hash), validator_index=n)),
        ("pair: address not in set + malformed", edit(ok(b=bad_hash), validator_address=b"\x07" * 20)),
        ("pair: malformed + bad signature", (lambda v: edit(v, signature=flip(v.signature, 1)))(ok(b=bad_psh))),
        ("pair: malformed + time out of range", ok(b=bad_hash, ts=(MAX_SECONDS, 0))),
        ("pair: time out of range + sig_len 0", edit(ok(ts=(T0[0], -5)), signature=b"")),
    ]
    wrong = [i for i, val in enumerate(vals.validators) if val.address != T.address_of(val.pub_key)]
    if wrong:  # the stored address equals the vote's, the key's hash does not
        cases.append(("address not of key (set holds the vote's address)", ok(idx=wrong[0])))
        cases.append(("pair: address not of key + malformed", ok(idx=wrong[0], b=bad_hash)))
    return cases


def verify_cases(chain_id, vals, seeds, tag="v"):
    """(name, vote) for a request without ADDVOTE (Vote.Verify with the key at validator_index): every
    vote has its own type, height, round and BlockID."""
    n = len(seeds)
    cases = []
    for i in range(12):
        bid = [block_id("%s%d" % (tag, i)), T.BlockID(), T.BlockID(block_id("x%d" % i).hash, 0, b"")][i % 3]
        cases.append(("verify %d" % i, signed(chain_id, vals, seeds, i % n, [1, 2, 32, 0, -1][i % 5], 1000 + 37 * i,
                                              i % 4, bid, (T0[0] + i, i))))
    v = signed(chain_id, vals, seeds, 1, 1, 5, 0, block_id(tag))
    cases += [
        ("verify: address empty", V.Vote(v.type, v.height, v.round, v.block_id, v.timestamp, b"", 1, v.signature)),
        ("verify: address length 19", V.Vote(v.type, v.height, v.round, v.block_id, v.timestamp,
                                             v.validator_address[:19], 1, v.signature)),
        ("verify: another validator's address", V.Vote(v.type, v.height, v.round, v.block_id, v.timestamp,
                                                       vals.validators[0].address, 1, v.signature)),
        ("verify: index negative", V.Vote(v.type, v.height, v.round, v.block_id, v.timestamp, v.validator_address, -7,
                                          v.signature)),
        ("verify: index == n", V.Vote(v.type, v.height, v.round, v.block_id, v.timestamp, v.validator_address, n,
                                      v.signature)),
        ("verify: flipped S", V.Vote(v.type, v.height, v.round, v.block_id, v.timestamp, v.validator_address, 1,
                                     flip(v.signature, 33))),
        ("verify: panic", signed(chain_id, vals, seeds, 2, 2, 5, 0, T.BlockID(b"\x01" * 7, 0, b""))),
        ("verify: go path", signed(chain_id, vals, seeds, 2, 2, 5, 0, block_id(tag), (MAX_SECONDS + 5, 0))),
    ]
    return cases


def is_go_path_case(name):
    return "go path" in name or name == "pair: time out of range + sig_len 0"


def pool(n_votes=129, n_vals=6):
    """One ADDVOTE request of n_votes prevotes over the classes of step_cases, repeated with fresh
    timestamps until the pool is full; batches of any size are its prefixes.  Returns the set, the
    request's fields and (name, vote) in order."""
    vals, seeds = valset(n_vals, "pool", wrong_address_at=n_vals - 1)
    out, rep = [], 0
    while len(out) < n_votes:
        out += step_cases(CHAIN, vals, seeds, 1, height=7, round_=2, tag="pool%d" % rep)
        rep += 1
    return vals, dict(chain_id=CHAIN, addvote=True, height=7, round=2, type=1), out[:n_votes]


def request(vals, fields, named):
    return V.VoteRequest(vals=vals, votes=[v for _, v in named], **fields)
