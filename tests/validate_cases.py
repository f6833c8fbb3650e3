"""validateBlock restated in Python over the oracle modules (test helper), and the case builders the CPU
and GPU block-validation tests share.

Restates, line for line, ``state/validation.go:15-151`` (validateBlock) and ``types/block.go:55-106``
(Block.ValidateBasic; Header.ValidateBasic, Commit.ValidateBasic and the evidences' ValidateBasic are
inputs, as they are of the C call).  The hashes come from the restatements the other suites pin:
``blockhash_cases`` (Commit.Hash, Data.Hash), ``evidence_cases`` (EvidenceList.Hash), ``oracle.merkle``
(Header.Hash, ValidatorSet.Hash); the block time from ``median_cases`` (MedianTime); VerifyCommit from
``oracle.commit``.  The generators restate ``state/helpers_test.go`` (makeState, makeBlock,
makeAndCommitGoodBlock) with seeded keys.
"""
import copy
import hashlib
from dataclasses import dataclass, field, replace

import numpy as np

import blockhash_cases as BH
import evidence_cases as EC
import median_cases as MC
import tmed.state as S
import tmed.types as T
from light_cases import fast_verify, oracle_verifier  # noqa: F401
from tmed.light import go_time as go_time_text
from oracle import commit as C
from oracle import merkle as M
from oracle import port
from oracle.fixtures import seed_of

CHAIN = "validate-chain"
GENESIS = (1546300800, 0)  # 2019-01-01, validation_test.go's defaultEvidenceTime
NANOS = 10 ** 9
MIN_SECONDS, MAX_SECONDS = BH.ZERO_TIME_SECONDS, BH.MAX_SECONDS
EVIDENCE_MAX_BYTES = 1000  # TestValidateBlockEvidence


def h256(s) -> bytes:
    return hashlib.sha256(s if isinstance(s, bytes) else s.encode()).digest()


def time_ok(t):
    return MIN_SECONDS <= t[0] < MAX_SECONDS and 0 <= t[1] < NANOS


# ----------------------------------------------------------------------------- hashes from the oracle

def sig_tuples(commit):
    return [(s.flag, s.address, s.timestamp[0], s.timestamp[1], s.signature) for s in commit.signatures]


def commit_hash(commit):
    """Commit.Hash(), or None where tmed_commit_hashes reports ok = 0 (include/tmed25519.h)."""
    for (_, addr, sec, nanos, sig) in sig_tuples(commit):
        if len(sig) > 64 or len(addr) not in (0, 20) or not time_ok((sec, nanos)):
            return None
    return BH.commit_hash(sig_tuples(commit))


def evidence_hash(evidence):
    """EvidenceList.Hash(), or None where tmed_evidence_hashes reports list_ok = 0."""
    items = []
    for e in evidence:
        if isinstance(e, (bytes, bytearray)):
            items.append(bytes(e))
        elif not EC.carried(e):
            return None
        else:
            items.append(EC.evidence_bytes(e))
    return EC.list_hash(items)


def valset_hash(vs):
    return M.valset_hash([(v.pub_key, v.voting_power) for v in vs.validators])


def oracle_vals(vs):
    return C.ValidatorSet([C.Validator(v.pub_key, v.voting_power, v.proposer_priority, v.address) for v in vs.validators])


def oracle_commit(cm):
    return C.Commit(cm.height, cm.round, C.BlockID(cm.block_id.hash, cm.block_id.psh_total, cm.block_id.psh_hash),
                    [C.CommitSig(s.flag, s.address, tuple(s.timestamp), s.signature) for s in cm.signatures])


# ----------------------------------------------------------------------------- the restatement

def _hexu(b):
    return bytes(b).hex().upper()


def block_validate_basic(blk):
    """Block.ValidateBasic (types/block.go:55-106): (code, error)."""
    h = blk.header
    if not blk.header_basic_ok:
        return S.VB_HEADER_BASIC, S.ErrBlockBasic("invalid header: Header.ValidateBasic failed")
    if blk.last_commit is None:
        return S.VB_COMMIT_BASIC, S.ErrBlockBasic("nil LastCommit")
    if not blk.commit_basic_ok:
        return S.VB_COMMIT_BASIC, S.ErrBlockBasic("wrong LastCommit: Commit.ValidateBasic failed")
    ch = commit_hash(blk.last_commit)
    if ch is None:
        return S.VB_GO_PATH, S.BlockGoPath()
    if h["last_commit_hash"] != ch:
        return S.VB_LAST_COMMIT_HASH, T.GoError("wrong Header.LastCommitHash. Expected %s, got %s"
                                                % (_hexu(ch), _hexu(h["last_commit_hash"])))
    dh = BH.txs_hash(blk.txs)
    if h["data_hash"] != dh:
        return S.VB_DATA_HASH, T.GoError("wrong Header.DataHash. Expected %s, got %s" % (_hexu(dh), _hexu(h["data_hash"])))
    if blk.evidence_basic_bad >= 0:
        return S.VB_EVIDENCE_BASIC, S.ErrBlockBasic("invalid evidence (#%d): Evidence.ValidateBasic failed"
                                                    % blk.evidence_basic_bad)
    eh = evidence_hash(blk.evidence)
    if eh is None:
        return S.VB_GO_PATH, S.BlockGoPath()
    if h["evidence_hash"] != eh:
        return S.VB_EVIDENCE_HASH, T.GoError("wrong Header.EvidenceHash. Expected %s, got %s"
                                             % (_hexu(h["evidence_hash"]), _hexu(eh)))
    return S.VB_OK, None


def validate_block(st, blk, prev=None):
    """validateBlock(state, block): (code, error, skipped).  prev: the previous block of a linked
    request, whose header gives the state's last block hash, height and time.  Checks whose KNOW_* bit is
    clear in st.known are skipped and collected in `skipped`."""
    code, err = block_validate_basic(blk)
    if code != S.VB_OK:
        return code, err, 0
    h = blk.header
    skipped = 0
    last_height, last_time, last_id = st.last_block_height, st.last_block_time, st.last_block_id
    if prev is not None:
        last_height, last_time = prev.header["height"], prev.header["time"]
        last_id = T.BlockID(M.header_hash(prev.header) or b"", last_id.psh_total, last_id.psh_hash)
    if h["version_app"] != st.version_app or h["version_block"] != st.version_block:
        return S.VB_VERSION, T.GoError("wrong Block.Header.Version. Expected {%d %d}, got {%d %d}"
                                       % (st.version_block, st.version_app, h["version_block"], h["version_app"])), skipped
    if h["chain_id"] != st.chain_id:
        return S.VB_CHAIN_ID, T.GoError("wrong Block.Header.ChainID. Expected %s, got %s" % (st.chain_id, h["chain_id"])), skipped
    if last_height == 0 and h["height"] != st.initial_height:
        return S.VB_HEIGHT_INITIAL, T.GoError("wrong Block.Header.Height. Expected %d for initial block, got %d"
                                              % (h["height"], st.initial_height)), skipped
    if last_height > 0 and h["height"] != last_height + 1:
        return S.VB_HEIGHT, T.GoError("wrong Block.Header.Height. Expected %d, got %d" % (last_height + 1, h["height"])), skipped
    hid = T.BlockID(*h["last_block_id"])
    if not hid.equals(last_id):
        return S.VB_LAST_BLOCK_ID, T.GoError("wrong Block.Header.LastBlockID.  Expected %s, got %s" % (last_id, hid)), skipped
    if not st.known & S.KNOW_APP_HASH:
        skipped |= S.KNOW_APP_HASH
    elif h["app_hash"] != st.app_hash:
        return S.VB_APP_HASH, T.GoError("wrong Block.Header.AppHash.  Expected %s, got %s"
                                        % (_hexu(st.app_hash), _hexu(h["app_hash"]))), skipped
    if not st.known & S.KNOW_CONSENSUS_HASH:
        skipped |= S.KNOW_CONSENSUS_HASH
    elif h["consensus_hash"] != st.consensus_hash:
        return S.VB_CONSENSUS_HASH, T.GoError("wrong Block.Header.ConsensusHash.  Expected %s, got %s"
                                              % (_hexu(st.consensus_hash), _hexu(h["consensus_hash"]))), skipped
    if not st.known & S.KNOW_LAST_RESULTS_HASH:
        skipped |= S.KNOW_LAST_RESULTS_HASH
    elif h["last_results_hash"] != st.last_results_hash:
        return S.VB_LAST_RESULTS_HASH, T.GoError("wrong Block.Header.LastResultsHash.  Expected %s, got %s"
                                                 % (_hexu(st.last_results_hash), _hexu(h["last_results_hash"]))), skipped
    if not st.known & S.KNOW_VALIDATORS:
        skipped |= S.KNOW_VALIDATORS
    elif h["validators_hash"] != valset_hash(st.validators):
        return S.VB_VALIDATORS_HASH, T.GoError("wrong Block.Header.ValidatorsHash.  Expected %s, got %s"
                                               % (_hexu(valset_hash(st.validators)), _hexu(h["validators_hash"]))), skipped
    if not st.known & S.KNOW_NEXT_VALIDATORS:
        skipped |= S.KNOW_NEXT_VALIDATORS
    elif h["next_validators_hash"] != valset_hash(st.next_validators):
        return S.VB_NEXT_VALIDATORS_HASH, T.GoError(
            "wrong Block.Header.NextValidatorsHash.  Expected %s, got %s"
            % (_hexu(valset_hash(st.next_validators)), _hexu(h["next_validators_hash"]))), skipped
    if h["height"] == st.initial_height:
        if len(blk.last_commit.signatures) != 0:
            return S.VB_INITIAL_HAS_SIGS, T.GoError("initial block can't have LastCommit signatures"), skipped
    else:
        try:
            err = C.verify_commit(oracle_vals(st.last_validators), st.chain_id,
                                  C.BlockID(last_id.hash, last_id.psh_total, last_id.psh_hash), h["height"] - 1,
                                  oracle_commit(blk.last_commit), verify_fn=blk.verify_fn or fast_verify)
        except RuntimeError:  # an unknown BlockIDFlag: the reference panics
            err = T.GoPanic(-1)
        if err is not None:
            return S.VB_LAST_COMMIT, err, skipped
    if len(h["proposer_address"]) != 20:
        return S.VB_PROPOSER_SIZE, T.GoError("expected ProposerAddress size 20, got %d" % len(h["proposer_address"])), skipped
    if st.known & S.KNOW_VALIDATORS and MC.get_by_address(st.validators, h["proposer_address"])[0] < 0:
        return S.VB_PROPOSER_UNKNOWN, T.GoError("block.Header.ProposerAddress %s is not a validator"
                                                % _hexu(h["proposer_address"])), skipped
    if h["height"] > st.initial_height:
        if not time_ok(h["time"]) or not time_ok(last_time):
            return S.VB_GO_PATH, S.BlockGoPath(), skipped
        if not h["time"] > last_time:
            return S.VB_TIME_NOT_AFTER, T.GoError("block time %s not greater than last block time %s"
                                                  % (go_time_text(h["time"]), go_time_text(last_time))), skipped
        mcode, median = MC.expected(blk.last_commit, st.last_validators)
        if mcode == S.MEDIAN_GO_PATH:
            return S.VB_GO_PATH, S.BlockGoPath(), skipped
        if tuple(h["time"]) != tuple(median):
            return S.VB_TIME_NOT_MEDIAN, T.GoError("invalid block time. Expected %s, got %s"
                                                   % (go_time_text(median), go_time_text(h["time"]))), skipped
    elif h["height"] == st.initial_height:
        if not time_ok(h["time"]) or not time_ok(last_time):
            return S.VB_GO_PATH, S.BlockGoPath(), skipped
        if tuple(h["time"]) != tuple(last_time):
            return S.VB_TIME_NOT_GENESIS, T.GoError("block time %s is not equal to genesis time %s"
                                                    % (go_time_text(h["time"]), go_time_text(last_time))), skipped
    else:
        return S.VB_HEIGHT_BELOW_INITIAL, T.GoError("block height %d lower than initial height %d"
                                                    % (h["height"], st.initial_height)), skipped
    if blk.evidence_byte_size > st.evidence_max_bytes:
        return S.VB_EVIDENCE_OVERFLOW, S.ErrEvidenceOverflow(st.evidence_max_bytes, blk.evidence_byte_size), skipped
    return S.VB_OK, None, skipped


def same(a, b):
    """Equal error values: the same type name and the same Error() text (None: no error)."""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, T.GoPanic) or isinstance(b, T.GoPanic):
        return isinstance(a, T.GoPanic) and isinstance(b, T.GoPanic)
    if isinstance(a, S.BlockGoPath) or isinstance(b, S.BlockGoPath):
        return isinstance(a, S.BlockGoPath) and isinstance(b, S.BlockGoPath)
    return type(a).__name__ == type(b).__name__ and str(a) == str(b)


# ----------------------------------------------------------------------------- cases

@dataclass
class VBlock(S.Block):
    """An S.Block with the verifier the restatement checks its commit with (None: the oracle's)."""
    verify_fn: object = None


@dataclass
class Case:
    """One request: a block against a state, optionally linked to the previous case of its call."""
    name: str
    block: VBlock
    state: S.BlockState
    link: bool = False

    def request(self):
        return (self.block, self.state, self.link)


def expected(cases):
    """[(code, error, skipped)] of the cases of one call."""
    return [validate_block(c.state, c.block, cases[i - 1].block if c.link else None) for i, c in enumerate(cases)]


_KEYS = {}


def keys(tag, n):
    have = _KEYS.setdefault(tag, [])
    while len(have) < n:
        s = seed_of("vb-" + tag, len(have))
        have.append((s, port.pubkey_from_seed(s)))
    return have[:n]


def port_signer(seeds, msgs):
    return [port.sign(s, m) for s, m in zip(seeds, msgs)]


@dataclass
class World:
    """A chain made by makeState + makeAndCommitGoodBlock: the set, and per height the valid block and
    the state it is validated against."""
    chain_id: str
    vals: T.ValidatorSet
    seeds: list
    blocks: list = field(default_factory=list)   # blocks[k]: height initial_height + k
    states: list = field(default_factory=list)   # states[k]: the state block k is validated against
    block_ids: list = field(default_factory=list)
    sig_override: dict = field(default_factory=dict)  # validator index -> the signature every commit carries for it


def make_header(chain_id, height, time, last_block_id, vals, st, last_commit, txs, evidence, proposer):
    return {"version_block": st.version_block, "version_app": st.version_app, "chain_id": chain_id, "height": height,
            "time": tuple(time), "last_block_id": (last_block_id.hash, last_block_id.psh_total, last_block_id.psh_hash),
            "last_commit_hash": commit_hash(last_commit), "data_hash": BH.txs_hash(txs),
            "validators_hash": valset_hash(vals), "next_validators_hash": valset_hash(vals),
            "consensus_hash": st.consensus_hash, "app_hash": st.app_hash, "last_results_hash": st.last_results_hash,
            "evidence_hash": evidence_hash(evidence), "proposer_address": proposer}


def make_commit(w, height, block_id, signer=port_signer, step=1):
    """Every validator's precommit for (height, block_id), timestamps a few seconds after GENESIS."""
    n = len(w.vals.validators)
    base = GENESIS[0] + 10 * height
    sigs = [C.CommitSig(C.FLAG_COMMIT, v.address, (base + (i * step) % 7, 1000 * i), b"") for i, v in enumerate(w.vals.validators)]
    cm = C.Commit(height, 0, C.BlockID(block_id.hash, block_id.psh_total, block_id.psh_hash), sigs)
    out = signer(w.seeds, [cm.vote_sign_bytes(w.chain_id, i) for i in range(n)])
    out = [w.sig_override.get(i, o) for i, o in enumerate(out)]
    return T.Commit(height, 0, block_id, [T.CommitSig(s.flag, s.address, s.timestamp, bytes(o)) for s, o in zip(sigs, out)])


def make_world(n_vals, n_blocks, tag="w", chain_id=CHAIN, initial_height=1, signer=port_signer, txs_per_block=2,
               powers=None, proposer_at=0, evidence_at=None, pub_override=None, sig_override=None, address_of=None):
    """pub_override / sig_override: {validator index: key / signature} in place of the seeded key's;
    address_of: f(index) -> address, for sets that hold an address twice."""
    ks = keys(tag, n_vals)
    powers = powers or [10 + (i % 5) for i in range(n_vals)]
    pub_override = pub_override or {}
    vals = T.ValidatorSet([T.Validator(pub_override.get(i, p), powers[i], 0, address_of(i) if address_of else b"")
                           for i, (_, p) in enumerate(ks)])
    w = World(chain_id, vals, [s for s, _ in ks], sig_override=dict(sig_override or {}))
    st = S.BlockState(11, 0, chain_id, initial_height, 0, T.BlockID(), GENESIS, b"", h256("consensus-params"), b"",
                      vals, vals, vals, EVIDENCE_MAX_BYTES)
    last_commit = T.Commit(0, 0, T.BlockID(), [])
    for k in range(n_blocks):
        height = initial_height + k
        txs = [b"tx-%d-%d" % (height, j) * (j + 1) for j in range(txs_per_block)]
        evidence = evidence_at(height) if evidence_at else []
        time = GENESIS if k == 0 else MC.median_time(last_commit, st.last_validators)
        proposer = vals.validators[proposer_at % n_vals].address
        hdr = make_header(chain_id, height, time, st.last_block_id, vals, st, last_commit, txs, evidence, proposer)
        blk = VBlock(hdr, last_commit, txs, evidence, sum(len(EC.evidence_bytes(e)) for e in evidence if not isinstance(e, bytes)))
        bid = T.BlockID(M.header_hash(hdr), 1, h256("parts-%d" % height))
        w.blocks.append(blk)
        w.states.append(st)
        w.block_ids.append(bid)
        last_commit = make_commit(w, height, bid, signer)
        st = replace(st, last_block_height=height, last_block_id=bid, last_block_time=tuple(time),
                     app_hash=h256("app-%d" % height), last_results_hash=h256("results-%d" % height))
    return w


def with_header(blk, **kw):
    """A copy of blk whose header has the fields of kw replaced (the header's own hash is not the block's to keep)."""
    return replace(blk, header=dict(blk.header, **kw))


def window(w, first=1, count=None, link=True, known=S.KNOW_ALL, name="window"):
    """Blocks first .. of the world as one call; linked requests after the first share block first's state
    apart from what the link supplies (the PartSetHeader half of LastBlockID is each block's own)."""
    count = len(w.blocks) - first if count is None else count
    out = []
    for j in range(count):
        k = first + j
        st = w.states[k]
        if link and j > 0:  # only what a caller has before ApplyBlock: the link supplies the rest
            st = replace(w.states[k], last_block_height=-1, last_block_time=(1, 1),
                         last_block_id=T.BlockID(b"", st.last_block_id.psh_total, st.last_block_id.psh_hash), known=known)
        elif known != S.KNOW_ALL:
            st = replace(st, known=known)
        out.append(Case("%s[%d]" % (name, j), w.blocks[k], st, link and j > 0))
    return out


WRONG_HASH = h256("this hash is wrong")


def header_mutations(blk):
    """TestValidateBlockHeader's table (state/validation_test.go:55-73): (name, mutated block)."""
    h = blk.header
    bh, pt, ph = h["last_block_id"]
    other = T.address_of(port.pubkey_from_seed(seed_of("vb-stranger", 0)))
    return [
        ("Version wrong1", with_header(blk, version_block=h["version_block"] + 2)),
        ("Version wrong2", with_header(blk, version_app=h["version_app"] + 2)),
        ("ChainID wrong", with_header(blk, chain_id="not-the-real-one")),
        ("Height wrong", with_header(blk, height=h["height"] + 10)),
        ("Time wrong", with_header(blk, time=(h["time"][0] - 1, h["time"][1]))),
        ("LastBlockID wrong", with_header(blk, last_block_id=(bh, pt + 10, ph))),
        ("LastCommitHash wrong", with_header(blk, last_commit_hash=WRONG_HASH)),
        ("DataHash wrong", with_header(blk, data_hash=WRONG_HASH)),
        ("ValidatorsHash wrong", with_header(blk, validators_hash=WRONG_HASH)),
        ("NextValidatorsHash wrong", with_header(blk, next_validators_hash=WRONG_HASH)),
        ("ConsensusHash wrong", with_header(blk, consensus_hash=WRONG_HASH)),
        ("AppHash wrong", with_header(blk, app_hash=WRONG_HASH)),
        ("LastResultsHash wrong", with_header(blk, last_results_hash=WRONG_HASH)),
        ("EvidenceHash wrong", with_header(blk, evidence_hash=WRONG_HASH)),
        ("Proposer wrong", with_header(blk, proposer_address=other)),
        ("Proposer invalid", with_header(blk, proposer_address=b"wrong size")),
    ]


_CODE_CASES = {}


def code_mutators(w, k=2):
    """{code: f(block, state) -> (block, state)} making exactly that check fail on block k of the world,
    for every code a single non-initial block can fail with, in code order."""
    other = T.address_of(port.pubkey_from_seed(seed_of("vb-stranger", 0)))

    def hdr(**kw):
        return lambda b, s: (with_header(b, **kw), s)

    def bad_commit(b, s):
        cm = copy.deepcopy(b.last_commit)
        sig = bytearray(cm.signatures[0].signature)
        sig[5] ^= 1
        cm.signatures[0].signature = bytes(sig)
        return replace(with_header(b, last_commit_hash=commit_hash(cm)), last_commit=cm), s

    def time_not_after(b, s):
        return with_header(b, time=tuple(s.last_block_time)), s

    def go_path(b, s):  # a signature longer than 64 bytes: Commit.Hash cannot be reproduced
        cm = copy.deepcopy(b.last_commit)
        cm.signatures[1].signature = bytes(65)
        return replace(b, last_commit=cm), s

    return {
        S.VB_HEADER_BASIC: lambda b, s: (replace(b, header_basic_ok=False), s),
        S.VB_COMMIT_BASIC: lambda b, s: (replace(b, commit_basic_ok=False), s),
        S.VB_LAST_COMMIT_HASH: hdr(last_commit_hash=WRONG_HASH),
        S.VB_DATA_HASH: hdr(data_hash=WRONG_HASH),
        S.VB_EVIDENCE_BASIC: lambda b, s: (replace(b, evidence_basic_bad=3), s),
        S.VB_EVIDENCE_HASH: hdr(evidence_hash=WRONG_HASH),
        S.VB_VERSION: hdr(version_app=7),
        S.VB_CHAIN_ID: hdr(chain_id="not-the-real-one"),
        S.VB_HEIGHT_INITIAL: lambda b, s: (b, replace(s, last_block_height=0)),
        S.VB_HEIGHT: lambda b, s: (b, replace(s, last_block_height=s.last_block_height + 1)),
        S.VB_LAST_BLOCK_ID: lambda b, s: (b, replace(s, last_block_id=T.BlockID(s.last_block_id.hash, 2, s.last_block_id.psh_hash))),
        S.VB_APP_HASH: hdr(app_hash=WRONG_HASH[:20]),  # another length: decided on the host
        S.VB_CONSENSUS_HASH: hdr(consensus_hash=WRONG_HASH),
        S.VB_LAST_RESULTS_HASH: hdr(last_results_hash=b""),
        S.VB_VALIDATORS_HASH: hdr(validators_hash=WRONG_HASH),
        S.VB_NEXT_VALIDATORS_HASH: hdr(next_validators_hash=WRONG_HASH),
        S.VB_INITIAL_HAS_SIGS: lambda b, s: (b, replace(s, initial_height=b.header["height"], last_block_height=0)),
        S.VB_LAST_COMMIT: bad_commit,
        S.VB_PROPOSER_SIZE: hdr(proposer_address=b"wrong size"),
        S.VB_PROPOSER_UNKNOWN: hdr(proposer_address=other),
        S.VB_TIME_NOT_AFTER: time_not_after,
        S.VB_TIME_NOT_MEDIAN: lambda b, s: (with_header(b, time=(b.header["time"][0], b.header["time"][1] + 1)), s),
        S.VB_TIME_NOT_GENESIS: None,      # an initial block: see initial_cases
        S.VB_HEIGHT_BELOW_INITIAL: lambda b, s: (b, replace(s, initial_height=b.header["height"] + 5)),
        S.VB_EVIDENCE_OVERFLOW: lambda b, s: (replace(b, evidence_byte_size=s.evidence_max_bytes + 1), s),
        S.VB_GO_PATH: go_path,
    }


def initial_cases(w):
    """The initial height: the good block (an empty commit), one with a signature (INITIAL_HAS_SIGS), one
    whose time is not the genesis time."""
    b0, s0 = w.blocks[0], w.states[0]
    cm = T.Commit(0, 0, T.BlockID(), [T.CommitSig(T.FLAG_COMMIT, w.vals.validators[0].address, GENESIS, bytes(64))])
    signed = replace(with_header(b0, last_commit_hash=commit_hash(cm)), last_commit=cm)
    late = with_header(b0, time=(GENESIS[0], 5))
    return [(Case("initial ok", b0, s0), S.VB_OK), (Case("initial with a signature", signed, s0), S.VB_INITIAL_HAS_SIGS),
            (Case("initial, not the genesis time", late, s0), S.VB_TIME_NOT_GENESIS)]


def code_cases(w, k=2):
    """[(Case, code)]: one case per outcome code (unlinked requests), OK first."""
    out = [(Case("ok", w.blocks[k], w.states[k]), S.VB_OK)]
    for code, f in code_mutators(w, k).items():
        if f is None:
            continue
        b, s = f(w.blocks[k], w.states[k])
        out.append((Case(S.VB_CODE_NAMES[code], b, s), code))
    return out + initial_cases(w)[1:]


def pair_cases(w, k=2):
    """[(Case, code)]: for every adjacent pair of codes a non-initial block can fail with together, both
    mutations applied: the earlier code must win.  Left out: the pairs no block can fail together (the
    two height checks; INITIAL_HAS_SIGS and LAST_COMMIT, TIME_NOT_MEDIAN and HEIGHT_BELOW_INITIAL, which
    lie on different branches; the two proposer checks, on one field)."""
    muts = [(c, f) for c, f in code_mutators(w, k).items() if f is not None and c != S.VB_GO_PATH]
    never = {(S.VB_HEIGHT_INITIAL, S.VB_HEIGHT), (S.VB_INITIAL_HAS_SIGS, S.VB_LAST_COMMIT),
             (S.VB_PROPOSER_SIZE, S.VB_PROPOSER_UNKNOWN), (S.VB_TIME_NOT_MEDIAN, S.VB_HEIGHT_BELOW_INITIAL)}
    out = []
    for (c1, f1), (c2, f2) in zip(muts, muts[1:]):
        if (c1, c2) in never:
            continue
        b, s = f1(w.blocks[k], w.states[k])
        if (c1, c2) != (S.VB_TIME_NOT_AFTER, S.VB_TIME_NOT_MEDIAN):  # the last block's time is no median either
            b, s = f2(b, s)
        out.append((Case("%s+%s" % (S.VB_CODE_NAMES[c1], S.VB_CODE_NAMES[c2]), b, s), c1))
    return out


KNOWN_FIELDS = [(S.KNOW_APP_HASH, "app_hash"), (S.KNOW_CONSENSUS_HASH, "consensus_hash"),
                (S.KNOW_LAST_RESULTS_HASH, "last_results_hash"), (S.KNOW_VALIDATORS, "validators_hash"),
                (S.KNOW_NEXT_VALIDATORS, "next_validators_hash")]


def known_cases(w, k=2):
    """[(Case, bit)]: each KNOW_* bit clear with that header field wrong: OK with the bit in skipped."""
    return [(Case("unknown " + name, with_header(w.blocks[k], **{name: WRONG_HASH}),
                  replace(w.states[k], known=S.KNOW_ALL & ~bit)), bit) for bit, name in KNOWN_FIELDS]


def broken_links(w):
    """Linked windows of 3 (blocks 1..3) with the link broken at request 1: [(name, cases, code)]."""
    base = window(w, 1, 3)
    out = []
    # the hash only: block 1's LastBlockID names another block
    bh, pt, ph = base[1].block.header["last_block_id"]
    c = list(base)
    c[1] = replace(c[1], block=with_header(c[1].block, last_block_id=(WRONG_HASH, pt, ph)))
    out.append(("hash", c, S.VB_LAST_BLOCK_ID))
    # the height only
    c = list(base)
    c[1] = replace(c[1], block=with_header(c[1].block, height=c[1].block.header["height"] + 1))
    out.append(("height", c, S.VB_HEIGHT))
    # the time equal to the previous block's
    c = list(base)
    c[1] = replace(c[1], block=with_header(c[1].block, time=tuple(c[0].block.header["time"])))
    out.append(("time", c, S.VB_TIME_NOT_AFTER))
    return out


# ----------------------------------------------------------------------------- the _with entry's inputs

def oracle_inputs(cases):
    """Everything tmed_validate_blocks_with takes besides the verifier, from the oracle."""
    n = len(cases)
    z = lambda: np.zeros((n, 32), np.uint8)
    ch, dh, eh, hh, vh, nh = z(), z(), z(), z(), z(), z()
    cok, eok, hok = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    med, prop = [], np.full(n, -1, np.int32)

    def put(arr, i, v):
        arr[i] = np.frombuffer(v, np.uint8)

    for i, c in enumerate(cases):
        b, s = c.block, c.state
        v = commit_hash(b.last_commit) if b.last_commit is not None else None
        if v is not None:
            put(ch, i, v)
            cok[i] = 1
        put(dh, i, BH.txs_hash(b.txs))
        v = evidence_hash(b.evidence)
        if v is not None:
            put(eh, i, v)
            eok[i] = 1
        v = M.header_hash(b.header)
        if v is not None:
            put(hh, i, v)
            hok[i] = 1
        if s.validators is not None:
            put(vh, i, valset_hash(s.validators))
            if len(b.header["proposer_address"]) == 20:
                prop[i] = MC.get_by_address(s.validators, b.header["proposer_address"])[0]
        if s.next_validators is not None:
            put(nh, i, valset_hash(s.next_validators))
        if b.last_commit is not None and s.last_validators is not None:
            code, t = MC.expected(b.last_commit, s.last_validators)
            med.append((code, t if t is not None else (0, 0)))
        else:
            med.append((S.MEDIAN_GO_PATH, (0, 0)))
    return ch, cok, dh, eh, eok, hh, hok, vh, nh, med, prop
