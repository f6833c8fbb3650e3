"""Free-standing votes without a device: tmed_votes_sign_bytes (csrc/vote_free.h, the source
vote_prepare_kernel compiles) byte for byte against oracle.signbytes over the reference's vectors, the
full product of field values and the length boundaries; agreement with tmed_vote_sign_bytes on
precommits; tmed_verify_votes_host's codes against the restatement of tests/vote_cases.py; the same
code as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/native/votes_host.cpp); the device splice of the commit seam on the CPU against the commit
encoder, the free-standing encoder and the oracle (tests/native/vote_wire_host.cpp); the static check
of the Go binding.  The device run of the same corpus
is tests/test_gpu_votes.py."""
import itertools
import json
import os
import struct
import subprocess
import sys

import pytest

import tmed.signbytes as SB
import tmed.types as T
import tmed.votes as V
import vote_cases as VC
from oracle.signbytes import ZERO_TIME, vote_sign_bytes
from tmed._native import TMED_EINVAL, TMED_OK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tendermint-fork_amd", "csrc")

H32 = bytes(0xA0 + i for i in range(32))
P32 = bytes(0x10 + i for i in range(32))
TYPES = [0, 1, 2, 32, -1, 2**31 - 1]
HEIGHTS = [0, 1, -1, 2**63 - 1]
ROUNDS = [0, 1, -1, 2**31 - 1]
BIDS = [(b"", 0, b""), (H32, 123, P32), (H32, 0, b""), (b"", 0, P32), (b"", 7, b""), (H32, 2**32 - 1, P32)]
SECONDS = [0, 1, -62135596800, 2**63 - 1]
NANOS = [0, 1, 999999999]
CHAINS = ["", "test_chain_id", "c" * 50]


def _vote(t, h, r, bid, ts):
    return V.Vote(t, h, r, T.BlockID(*bid), ts, b"", 0)


def _oracle(chain, v):
    b = v.block_id
    return vote_sign_bytes(chain, v.type, v.height, v.round, (b.hash, b.psh_total, b.psh_hash), v.timestamp)


@pytest.fixture(scope="module")
def sweep():
    """The product in itertools.product order (the chain ID varies fastest) and the oracle's bytes."""
    combos = list(itertools.product(TYPES, HEIGHTS, ROUNDS, BIDS, SECONDS, NANOS, CHAINS))
    assert len(combos) == 20736
    return combos, [vote_sign_bytes(c, t, h, r, bid, (s, ns)) for t, h, r, bid, s, ns, c in combos]


# ----------------------------------------------------------------------------- sign-bytes

def test_reference_vectors():
    with open(os.path.join(ROOT, "tests", "golden", "signbytes_vectors.json")) as f:
        vectors = json.load(f)["reference_vectors"]
    assert len(vectors) == 5 and {v["type"] for v in vectors} == {0, 1, 2}
    for v in vectors:
        got = V.sign_bytes(v["chain_id"], [_vote(v["type"], v["height"], v["round"], (b"", 0, b""), ZERO_TIME)])[0]
        assert got.hex() == v["want"], v


def test_full_product_equals_the_oracle(sweep):
    combos, want = sweep
    for chain in CHAINS:
        mine = [(k, c) for k, c in enumerate(combos) if c[6] == chain]
        got = V.sign_bytes(chain, [_vote(t, h, r, bid, (s, ns)) for _, (t, h, r, bid, s, ns, _) in mine])
        for (k, c), g in zip(mine, got):
            assert g == want[k], c
    assert max(len(w) for w in want) <= 185


def _find(target_msg=None, target_body=None):
    """A vote and chain ID whose message (or body) has exactly the wanted length."""
    for bid, h, r, t, s in itertools.product(BIDS, [0, 5], [0, 3], [0, 1, -1], [0, 1, 2**40, -1]):
        for cl in range(0, 60):
            v = _vote(t, h, r, bid, (s, 7))
            m = _oracle("c" * cl, v)
            body = len(m) - (1 if len(m) <= 128 else 2)
            if (target_msg is not None and len(m) == target_msg) or (target_body is not None and body == target_body):
                return "c" * cl, v, m
    raise AssertionError("no vote of that length")


def test_length_boundaries():
    """The length prefix goes from one byte to two between a body of 127 and 128 bytes; with the 64-byte
    R || A prefix SHA-512 takes one block up to a 47-byte message, two up to 175, three from 176."""
    for kw in (dict(target_body=127), dict(target_body=128), dict(target_msg=47), dict(target_msg=48),
               dict(target_msg=175), dict(target_msg=176)):
        chain, v, want = _find(**kw)
        got = V.sign_bytes(chain, [v])[0]
        assert got == want, kw
        prefix = 1 if got[0] < 0x80 else 2
        body = len(got) - prefix
        assert prefix == (1 if body < 128 else 2)
        assert kw.get("target_body", body) == body and kw.get("target_msg", len(got)) == len(got)
    # SHA-512 blocks of R || A || M: 64 + len + the 0x80 byte + the 16-byte length
    assert [(64 + n + 17 + 127) // 128 for n in (47, 48, 175, 176)] == [1, 2, 2, 3]
    # the maximum with a 50-byte chain ID: every field at its longest
    worst = _vote(-1, 1, 1, (H32, 2**32 - 1, P32), (-1, -1))
    got = V.sign_bytes("c" * 50, [worst])[0]
    assert got == _oracle("c" * 50, worst) and len(got) == 185


def test_precommits_equal_the_commit_encoder():
    for chain, h, r, bid, ts in itertools.product(["", "test_chain_id", "c" * 50], [1, 2**63 - 1], [0, 5],
                                                  [(H32, 123, P32), (b"", 0, b""), (H32, 0, b"")],
                                                  [ZERO_TIME, (1700000000, 999999999), (0, 0)]):
        mine = V.sign_bytes(chain, [_vote(2, h, r, bid, ts)])[0]
        assert mine == SB.vote_sign_bytes(chain, h, r, bid, ts, flag=2)
        nil = V.sign_bytes(chain, [_vote(2, h, r, (b"", 0, b""), ts)])[0]
        assert nil == SB.vote_sign_bytes(chain, h, r, bid, ts, flag=3)


def test_malformed_block_id_encodes_nothing():
    votes = [_vote(1, 1, 0, (H32[:31], 1, P32), (1, 1)), _vote(1, 1, 0, (H32, 1, P32 + b"\x00"), (1, 1)),
             _vote(1, 1, 0, (H32, 1, P32), (1, 1))]
    got = V.sign_bytes("x", votes)
    assert got[0] is None and got[1] is None and got[2] == _oracle("x", votes[2])
    l = V._bind()
    pv = V.PackedVotes(votes)
    import ctypes
    import numpy as np
    off = np.zeros(4, np.uint32)
    total = ctypes.c_size_t(0)
    assert l.tmed_votes_sign_bytes(b"x", 1, ctypes.byref(pv.c), None, 0, T._ptr(off), ctypes.byref(total), None) == TMED_EINVAL
    assert l.tmed_votes_sign_bytes(b"x", 1, None, None, 0, T._ptr(off), ctypes.byref(total), None) == TMED_EINVAL


# ----------------------------------------------------------------------------- the checks

@pytest.fixture(scope="module")
def requests():
    """The pool of the device tests, prevote and precommit requests against other sets, a request
    without ADDVOTE, and one with a 51-byte chain ID; with the restatement's codes."""
    vals, fields, named = VC.pool(129, 6)
    va, sa = VC.valset(4, "two-a")
    vb, sb = VC.valset(7, "two-b", wrong_address_at=2)
    vv, sv = VC.valset(5, "vv")
    reqs = [(VC.request(vals, fields, named), [n for n, _ in named])]
    for chain, vs, seeds, type_, h, r in ((VC.CHAIN, va, sa, 1, 11, 0), ("other-chain", vb, sb, 2, 12, 3),
                                          ("c" * 51, va, sa, 2, 13, 1)):
        cs = VC.step_cases(chain, vs, seeds, type_, height=h, round_=r, tag=chain[:3])
        reqs.append((V.VoteRequest(chain, vs, [v for _, v in cs], True, h, r, type_), [n for n, _ in cs]))
    cs = VC.verify_cases(VC.CHAIN, vv, sv)
    reqs.append((V.VoteRequest(VC.CHAIN, vv, [v for _, v in cs]), [n for n, _ in cs]))
    return reqs, [[VC.expected(r, v) for v in r.votes] for r, _ in reqs]


def _pre(code):
    """What the host function reports: the signature's two outcomes are 0 (the signature decides)."""
    return 0 if code in (V.VOTE_OK, V.VOTE_INVALID_SIGNATURE) else code


def test_corpus_covers_classes_and_pairs(requests):
    reqs, exp = requests
    assert set(exp[0]) == set(range(10)) and set(exp[1]) >= set(range(10)) - {V.VOTE_ADDRESS_NOT_OF_KEY}
    want = {"pair: index negative + address empty": V.VOTE_INDEX_NEGATIVE,
            "pair: address empty + wrong step": V.VOTE_ADDRESS_EMPTY,
            "pair: wrong step + index == n": V.VOTE_UNEXPECTED_STEP,
            "pair: index == n + malformed": V.VOTE_INDEX_NOT_IN_SET,
            "pair: address not in set + malformed": V.VOTE_ADDRESS_NOT_IN_SET,
            "pair: address not of key + malformed": V.VOTE_ADDRESS_NOT_OF_KEY,
            "pair: malformed + bad signature": V.VOTE_PANIC,
            "pair: malformed + time out of range": V.VOTE_PANIC,
            "pair: time out of range + sig_len 0": V.VOTE_GO_PATH,
            "panic: hash of 31 bytes": V.VOTE_PANIC, "address length 19": V.VOTE_ADDRESS_NOT_IN_SET,
            "sig_len 63": V.VOTE_INVALID_SIGNATURE, "valid nil vote": V.VOTE_OK}
    names = requests[0][0][1]
    for name, code in want.items():
        assert exp[0][names.index(name)] == code, name
    vnames = reqs[-1][1]
    assert exp[-1][vnames.index("verify: address length 19")] == V.VOTE_ADDRESS_NOT_OF_KEY
    assert exp[-1][vnames.index("verify: address empty")] == V.VOTE_ADDRESS_NOT_OF_KEY


def test_host_codes_equal_the_restatement(requests):
    reqs, exp = requests
    pv = V.PreparedVotes([r for r, _ in reqs])
    got = pv.run(None)
    flat = [e for es in exp for e in es]
    names = [n for _, ns in reqs for n in ns]
    assert len(got) == len(flat)
    for k, (g, e) in enumerate(zip(got, flat)):
        assert int(g) == _pre(e), (names[k], V.CODE_NAMES[e], int(g))
    assert list(pv.device_route[:len(reqs)]) == [1, 1, 1, 0, 1]
    # the message lengths are the oracle's where the signature decides, 0 elsewhere
    k = 0
    for (r, _), es in zip(reqs, exp):
        for v, e in zip(r.votes, es):
            assert pv.msg_lens[k] == (len(VC.sign_bytes(r.chain_id, v)) if _pre(e) == 0 else 0)
            k += 1
    # one request at a time through the public entry point
    for (r, _), es in zip(reqs, exp):
        assert [int(g) for g in V.verify_votes(None, [r])] == [_pre(e) for e in es]


def test_overlong_chain_id_takes_the_host_route():
    """A 51-byte chain ID with every field at its longest: 186 bytes, past the bound the slots are
    derived for, so the request is assembled on the host; the bytes are the oracle's."""
    vals, seeds = VC.valset(2, "long")
    chain = "c" * 51
    v = VC.signed(chain, vals, seeds, 1, -1, 1, 1, T.BlockID(H32, 2**32 - 1, P32), (253402300799, 999999999))
    w = V.Vote(-1, 1, 1, T.BlockID(H32, 2**32 - 1, P32), (-1, -1), b"", 0)
    assert V.sign_bytes(chain, [v, w]) == [_oracle(chain, v), _oracle(chain, w)] and len(_oracle(chain, w)) == 186
    pv = V.PreparedVotes([V.VoteRequest(chain, vals, [v]), V.VoteRequest(chain[:50], vals, [v])])
    assert list(pv.run(None)) == [0, 0]
    assert list(pv.device_route[:2]) == [0, 1] and list(pv.msg_lens[:2]) == [len(_oracle(chain, v)), len(_oracle(chain, v)) - 1]


def test_argument_errors():
    l = V._bind()
    vals, seeds = VC.valset(2, "args")
    v = VC.signed(VC.CHAIN, vals, seeds, 0, 1, 1, 0, T.BlockID())
    for field in ("types", "heights", "rounds", "block_hashes", "psh_totals", "psh_hashes", "ts_seconds", "ts_nanos",
                  "addresses", "validator_indexes", "sigs"):
        pv = V.PreparedVotes([V.VoteRequest(VC.CHAIN, vals, [v], True, 1, 0, 1)])
        setattr(pv.reqs[0].votes.contents, field, None)
        assert l.tmed_verify_votes_host(pv.reqs, 1, T._ptr(pv.codes), None, None) == TMED_EINVAL, field
    pv = V.PreparedVotes([V.VoteRequest(VC.CHAIN, vals, [v], True, 1, 0, 1)])
    assert l.tmed_verify_votes_host(pv.reqs, 1, None, None, None) == TMED_EINVAL
    assert l.tmed_verify_votes(None, pv.reqs, 1, T._ptr(pv.codes)) == TMED_EINVAL
    pv.reqs[0].vals.contents.addresses = None  # read under ADDVOTE
    assert l.tmed_verify_votes_host(pv.reqs, 1, T._ptr(pv.codes), None, None) == TMED_EINVAL
    pv.reqs[0].flags = 0
    assert l.tmed_verify_votes_host(pv.reqs, 1, T._ptr(pv.codes), None, None) == TMED_OK and pv.codes[0] == 0
    # the length arrays may be NULL: 32-byte hashes, 20-byte addresses, 64-byte signatures
    full = VC.signed(VC.CHAIN, vals, seeds, 0, 1, 1, 0, VC.block_id("args"))
    pv = V.PreparedVotes([V.VoteRequest(VC.CHAIN, vals, [full], True, 1, 0, 1)])
    c = pv.reqs[0].votes.contents
    c.block_hash_lens = c.psh_hash_lens = c.address_lens = c.sig_lens = None
    assert l.tmed_verify_votes_host(pv.reqs, 1, T._ptr(pv.codes), T._ptr(pv.msg_lens), None) == TMED_OK
    assert pv.codes[0] == 0 and pv.msg_lens[0] == len(VC.sign_bytes(VC.CHAIN, full))
    assert V.to_error(V.VOTE_OK) is None
    assert V.to_error(V.VOTE_INDEX_NOT_IN_SET) == V.ErrVoteInvalidValidatorIndex()
    assert str(V.to_error(V.VOTE_UNEXPECTED_STEP)) == "unexpected step"
    assert str(V.to_error(V.VOTE_ADDRESS_NOT_OF_KEY)) == "invalid validator address"
    assert str(V.to_error(V.VOTE_INVALID_SIGNATURE)) == "invalid signature"
    assert isinstance(V.to_error(V.VOTE_PANIC), V.VotePanic) and isinstance(V.to_error(V.VOTE_GO_PATH), V.VoteGoPath)


# ----------------------------------------------------------------------------- host build

@pytest.fixture(scope="module")
def votes_host(tmp_path_factory):
    """tests/native/votes_host.cpp built with the sanitizers into a temporary directory."""
    exe = str(tmp_path_factory.mktemp("votes") / "votes_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "votes_host.cpp"), "-o", exe])
    return exe


def test_sweep_under_sanitizers(votes_host, sweep, tmp_path):
    _, want = sweep
    out_bin = tmp_path / "sweep.bin"
    out = subprocess.run([votes_host, "sweep", str(out_bin)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip() == "sweep-ok 20736 %d" % max(len(w) for w in want)
    raw = out_bin.read_bytes()
    pos = 0
    for k, w in enumerate(want):
        (n,) = struct.unpack_from("<H", raw, pos)
        assert raw[pos + 2:pos + 2 + n] == w, k
        pos += 2 + n
    assert pos == len(raw)


def _hex(b):
    return bytes(b).hex() or "-"


def _case_lines(reqs):
    """The text form tests/native/votes_host.cpp reads."""
    lines = []
    for r, _ in reqs:
        lines.append("req %d %d %d %d %s %d %d" % (1 if r.addvote else 0, r.height, r.round, r.type,
                                                   _hex(r.chain_id.encode()), len(r.vals.validators), len(r.votes)))
        lines.extend("val %s %s" % (_hex(val.pub_key), _hex(val.address)) for val in r.vals.validators)
        for v in r.votes:
            b = v.block_id
            lines.append("vote %d %d %d %s %d %s %d %d %s %d %d" % (
                v.type, v.height, v.round, _hex(b.hash), b.psh_total, _hex(b.psh_hash), v.timestamp[0], v.timestamp[1],
                _hex(v.validator_address), v.validator_index, len(v.signature)))
    return "\n".join(lines) + "\n"


def test_checks_under_sanitizers(votes_host, requests, tmp_path):
    reqs, exp = requests
    src = tmp_path / "cases.txt"
    src.write_text(_case_lines(reqs))
    out = subprocess.run([votes_host, "cases", str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    flat = [(r, v, e) for (r, _), es in zip(reqs, exp) for v, e in zip(r.votes, es)]
    assert lines[-1] == "cases-ok" and len(lines) == len(flat) + 1
    for line, (r, v, e) in zip(lines, flat):
        code, mlen = [int(x) for x in line.split()]
        assert code == _pre(e)
        assert mlen == (len(VC.sign_bytes(r.chain_id, v)) if code == 0 else 0)


@pytest.fixture(scope="module")
def wire_cases():
    """The cases of tests/native/vote_wire_host.cpp in its order, with the oracle's bytes: flags 1-3 over the
    product of BlockIDs, heights, rounds, chain-ID lengths, seconds and nanos (any int32 crosses the ABI),
    bodies of 127 and 128 bytes, and the longest chain ID the device template takes (129) and one more."""
    bids = [(b"", 0, b""), (H32, 0, b""), (b"", 0, P32), (H32, 123, P32), (b"", 1, b""), (H32, 2**32 - 1, P32)]
    cases = [(cl, h, r, bid, flag, (s, ns)) for bid, h, r, cl, s, ns, flag in itertools.product(
        bids, [0, 1, 2**63 - 1], [0, 1, 2**31 - 1], [0, 13, 50, 127, 128], [0, 1, -62135596800, 253402300799],
        [0, 1, 999999999, -1], [1, 2, 3])]
    cases += [(cl, 0, 0, bids[0], 1, (0, 0)) for cl in (121, 122)]
    cases += [(cl, 2**63 - 1, 2**31 - 1, bids[5], flag, (-1, -1)) for flag in (1, 2, 3) for cl in (129, 130)]
    want = [vote_sign_bytes("c" * cl, 2, h, r, bid if flag == 2 else None, ts) for cl, h, r, bid, flag, ts in cases]
    return cases, want


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitizers"])
def test_device_splice_on_the_host(san, wire_cases, tmp_path):
    """vote_splice on the device_template record (what assemble_vote_into runs once the record is staged)
    == VoteEncoder::write == vote_free_write inside the program; its messages == the oracle's here."""
    cases, want = wire_cases
    exe = str(tmp_path / "vote_wire_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *san, "-Wno-unknown-pragmas", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "vote_wire_host.cpp"),
                           "-x", "c++", os.path.join(CSRC, "signbytes.hip"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split()
    assert lines[-3:] == ["wire-ok", str(len(cases)), "257"] and len(lines) == len(cases) + 3
    for k, (line, w) in enumerate(zip(lines, want)):
        assert line == w.hex(), cases[k]
    lens = {(cl, flag): len(w) for (cl, _, _, _, flag, _), w in zip(cases, want)}
    assert lens[129, 2] == 256 and lens[130, 2] == 257  # a slot is 256 bytes
    bodies = {cl: len(w) for (cl, *_), w in zip(cases, want) if cl in (121, 122)}
    assert bodies == {121: 1 + 127, 122: 2 + 128}


def test_go_binding_static_check():
    """tools/go_cgo_check.py over the binding with every Go test file (votes_test.go included) and the
    snippets of INTEGRATION.md (the VoteSet.AddVotes patch of §2d among them)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import go_cgo_check as gc
    header = gc.Header()
    go_dir = os.path.dirname(gc.GO_FILE)
    extra = []
    for name in ("tmedgpu_test.go", "proofs_test.go", "light_test.go", "median_test.go", "votes_test.go"):
        with open(os.path.join(go_dir, name)) as f:
            extra.append((name, f.read()))
    with open(gc.GO_FILE) as f:
        go = f.read()
    with open(gc.INTEGRATION) as f:
        md = f.read()
    errs, pkg = gc.check_binding(go, header, extra=extra)
    assert errs + gc.check_snippets(md, header, pkg) == []
    assert "func (e *Engine) VerifyVotes(" in go and "C.tmed_verify_votes(" in go
    assert "eng.VerifyVotes(" in md and "VoteGoPath" in md and "AddVotes(" in md
    assert {"tmed_verify_votes", "tmed_verify_votes_host", "tmed_votes_sign_bytes"} <= set(header.funcs)
    assert {"TMED_VOTE_OK", "TMED_VOTE_PANIC", "TMED_VOTE_GO_PATH", "TMED_VOTES_ADDVOTE"} <= header.macros
