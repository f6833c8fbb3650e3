"""validateBlock without a device: the Python restatement (tests/validate_cases.py) against the outcomes
the reference's own tests pin (state/validation_test.go: TestValidateBlockHeader :55-73,
TestValidateBlockCommit :98-212, TestValidateBlockEvidence :214-283), the seam's replay
(tmed_validate_blocks_with: csrc/validate_host.h) against the restatement with the oracle's hashes,
medians, proposer lookups and verifier, and the replay compiled for the host under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/native/validate_host.cpp, a stand-alone program).  The device run of
the same cases is tests/test_gpu_validate.py."""
import copy
import ctypes
import os
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import tmed.state as S
import tmed.types as T
import validate_cases as VC
from oracle import port
from oracle.fixtures import seed_of
from tmed._native import TMED_EINVAL, TMED_OK, TmedError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def world():
    return VC.make_world(4, 5)


def run_with(cases, verifier=VC.oracle_verifier):
    pb = S.PreparedBlocks([c.request() for c in cases])
    pb.run_with(verifier, *VC.oracle_inputs(cases))
    return pb


def check(cases):
    """The seam's results of one call against the restatement's; returns (PreparedBlocks, expected)."""
    pb = run_with(cases)
    exp = VC.expected(cases)
    for q, (c, (code, err, skipped), got) in enumerate(zip(cases, exp, pb.errors())):
        assert pb.res[q].code == code, (c.name, S.VB_CODE_NAMES[pb.res[q].code], S.VB_CODE_NAMES[code])
        assert VC.same(got, err), (c.name, got, err)
        assert pb.res[q].skipped == skipped, (c.name, pb.res[q].skipped, skipped)
    return pb, exp


# ----------------------------------------------------------------------------- the restatement

def test_restatement_fails_every_header_mutation_and_passes_the_block(world):
    """TestValidateBlockHeader: at every height, each malleated block fails and the good block passes."""
    for k, (blk, st) in enumerate(zip(world.blocks, world.states)):
        assert VC.validate_block(st, blk) == (S.VB_OK, None, 0), k
        muts = VC.header_mutations(blk)
        assert len(muts) == 16
        for name, bad in muts:
            code, err, _ = VC.validate_block(st, bad)
            assert code != S.VB_OK and err is not None, (k, name)


def commit_outcomes(world, k=2):
    """TestValidateBlockCommit's three blocks at height k + 1 > 1: [(name, block)]."""
    blk, st = world.blocks[k], world.states[k]

    def with_commit(cm):
        return replace(VC.with_header(blk, last_commit_hash=VC.commit_hash(cm)), last_commit=cm)

    # votes for `height` where height - 1 is due (#2589)
    wrong_height = VC.make_commit(world, blk.header["height"], st.last_block_id)
    # a commit whose signature count is not the set's size
    wrong_sigs = T.Commit(blk.header["height"] - 1, 0, st.last_block_id, [])
    # the good votes, one of them replaced by a precommit a key outside the set signed
    extra_bad = copy.deepcopy(blk.last_commit)
    extra_bad.signatures[1].signature = port.sign(seed_of("vb-bad-privval", 0),
                                                  VC.oracle_commit(extra_bad).vote_sign_bytes(world.chain_id, 1))
    return [("wrong height", with_commit(wrong_height)), ("wrong sigs", with_commit(wrong_sigs)),
            ("bad precommit", with_commit(extra_bad))]


def test_restatement_reproduces_validate_block_commit(world):
    blk, st = world.blocks[2], world.states[2]
    height = blk.header["height"]
    (_, b1), (_, b2), (_, b3) = commit_outcomes(world)
    code, err, _ = VC.validate_block(st, b1)
    assert code == S.VB_LAST_COMMIT and type(err).__name__ == "ErrInvalidCommitHeight"
    assert (err.expected, err.actual) == (height - 1, height)
    code, err, _ = VC.validate_block(st, b2)
    assert code == S.VB_LAST_COMMIT and type(err).__name__ == "ErrInvalidCommitSignatures"
    assert (err.expected, err.actual) == (4, 0)
    code, err, _ = VC.validate_block(st, b3)
    assert code == S.VB_LAST_COMMIT and str(err).startswith("wrong signature (#1): ")


def test_restatement_reproduces_validate_block_evidence(world):
    """TestValidateBlockEvidence: ErrEvidenceOverflow at ByteSize = max + 1, a pass at exactly max."""
    blk, st = world.blocks[2], world.states[2]
    code, err, _ = VC.validate_block(st, replace(blk, evidence_byte_size=st.evidence_max_bytes + 1))
    assert code == S.VB_EVIDENCE_OVERFLOW and isinstance(err, S.ErrEvidenceOverflow)
    assert (err.max, err.got) == (1000, 1001) and str(err) == "Too much evidence: Max 1000, got 1001"
    assert VC.validate_block(st, replace(blk, evidence_byte_size=st.evidence_max_bytes))[0] == S.VB_OK


# ----------------------------------------------------------------------------- the seam's replay

def test_seam_reproduces_the_reference_tests(world):
    cases = []
    for k, (blk, st) in enumerate(zip(world.blocks, world.states)):
        cases.append(VC.Case("good %d" % k, blk, st))
        cases += [VC.Case("%s @%d" % (name, k), bad, st) for name, bad in VC.header_mutations(blk)]
    blk, st = world.blocks[2], world.states[2]
    cases.append(VC.Case("overflow", replace(blk, evidence_byte_size=1001), st))
    cases.append(VC.Case("at the limit", replace(blk, evidence_byte_size=1000), st))
    cases += [VC.Case(name, b, st) for name, b in commit_outcomes(world)]
    pb, exp = check(cases)
    assert [e[0] for e in exp].count(S.VB_OK) == len(world.blocks) + 1


def test_one_case_per_code(world):
    scen = VC.code_cases(world)
    assert {code for _, code in scen} == set(range(27))  # every outcome code has a case
    pb, exp = check([c for c, _ in scen])
    for q, (c, code) in enumerate(scen):
        assert pb.res[q].code == code, (c.name, pb.res[q].code)
    by = {c.name: pb.res[q] for q, (c, _) in enumerate(scen)}
    r = by["LAST_COMMIT_HASH"]
    assert r.hash_len == 32 and bytes(r.hash) == VC.commit_hash(world.blocks[2].last_commit)
    r = by["VALIDATORS_HASH"]
    assert bytes(r.hash) == VC.valset_hash(world.vals)
    assert by["EVIDENCE_BASIC"].idx == 3
    r = by["TIME_NOT_MEDIAN"]
    assert (r.median_seconds, r.median_nanos) == tuple(world.blocks[2].header["time"])
    assert by["LAST_COMMIT"].commit.code == 4 and by["LAST_COMMIT"].commit.idx == 0
    assert by["ok"].proposer_idx == 0 and by["PROPOSER_UNKNOWN"].proposer_idx == -1


def test_the_earlier_of_two_failing_checks_wins(world):
    scen = VC.pair_cases(world)
    assert len(scen) >= 19
    pb, _ = check([c for c, _ in scen])
    for q, (c, code) in enumerate(scen):
        assert pb.res[q].code == code, (c.name, S.VB_CODE_NAMES[pb.res[q].code])


def test_unknown_fields_are_skipped_and_reported(world):
    scen = VC.known_cases(world)
    pb, _ = check([c for c, _ in scen])
    for q, (c, bit) in enumerate(scen):
        assert pb.res[q].code == S.VB_OK and pb.res[q].skipped == bit, c.name
    # a set whose bit is clear may be NULL: the proposer lookup goes with the validators' hash check
    blk, st = world.blocks[2], world.states[2]
    spec = replace(st, validators=None, next_validators=None, known=S.KNOW_ALL & ~(S.KNOW_VALIDATORS | S.KNOW_NEXT_VALIDATORS))
    stranger = VC.with_header(blk, proposer_address=bytes(20))
    pb, _ = check([VC.Case("no sets", stranger, spec)])
    assert pb.res[0].code == S.VB_OK and pb.res[0].skipped == S.KNOW_VALIDATORS | S.KNOW_NEXT_VALIDATORS
    # a failure behind a skipped check still reports the skip
    pb, _ = check([VC.Case("skip then fail", replace(blk, evidence_byte_size=5000), replace(st, known=0))])
    assert pb.res[0].code == S.VB_EVIDENCE_OVERFLOW and pb.res[0].skipped == S.KNOW_ALL


def test_linked_windows(world):
    good = VC.window(world, 1)
    pb, exp = check(good)
    assert [e[0] for e in exp] == [S.VB_OK] * 4
    check(VC.window(world, 1, known=0))  # the speculative window: nothing ApplyBlock makes is known
    for name, cases, code in VC.broken_links(world):
        pb, exp = check(cases)
        assert pb.res[0].code == S.VB_OK and pb.res[1].code == code, name
    # the computed hash is reported with the broken link
    name, cases, _ = VC.broken_links(world)[0]
    pb = run_with(cases)
    from oracle import merkle as M
    assert pb.res[1].hash_len == 32 and bytes(pb.res[1].hash) == M.header_hash(cases[0].block.header)
    # a failure of request i - 1 does not change request i's outcome
    cases = list(good)
    cases[1] = replace(cases[1], block=replace(cases[1].block, evidence_byte_size=5000))
    pb, _ = check(cases)
    assert [pb.res[q].code for q in range(4)] == [S.VB_OK, S.VB_EVIDENCE_OVERFLOW, S.VB_OK, S.VB_OK]


def test_requests_decided_before_the_commit_send_no_signatures(world):
    scen = VC.code_cases(world)
    pb = run_with([c for c, _ in scen])
    for q, (c, code) in enumerate(scen):
        if code != S.VB_GO_PATH and 0 < code < S.VB_LAST_COMMIT:
            assert pb.res[q].verified == 0, c.name
        if code == S.VB_OK and c.block.header["height"] > 1:
            assert pb.res[q].verified == 4, c.name


def test_batch_equals_one_request_at_a_time(world):
    cases = [c for c, _ in VC.code_cases(world)] + [c for c, _ in VC.pair_cases(world)]
    batch = run_with(cases)
    for q, c in enumerate(cases):
        one = run_with([c])
        assert one.res[0].code == batch.res[q].code, c.name
        assert VC.same(one.errors()[0], batch.errors()[q]), c.name


def test_argument_errors(world):
    l = S._bind_vb()
    case = VC.Case("ok", world.blocks[2], world.states[2])
    fn = T.VERIFY_FN(lambda *a: -3)

    def call(pb, verify=fn, drop=None, n=None):
        ins = VC.oracle_inputs([case])
        arrs = [np.ascontiguousarray(a, np.uint8) for a in ins[:9]]
        med = (S._MedianResultC * 1)()
        ptrs = [T._ptr(a) for a in arrs]
        if drop is not None:
            ptrs[drop] = None
        if n is not None:
            pb.batch.n = n
        return l.tmed_validate_blocks_with(ctypes.byref(pb.batch), pb.res, *ptrs, med, T._ptr(ins[10]), verify, None)

    assert call(S.PreparedBlocks([case.request()]), n=0) == TMED_OK
    assert call(S.PreparedBlocks([case.request()]), drop=0) == TMED_EINVAL
    assert call(S.PreparedBlocks([case.request()]), verify=ctypes.cast(None, T.VERIFY_FN)) == TMED_EINVAL
    assert l.tmed_validate_blocks(None, ctypes.byref(S.PreparedBlocks([case.request()]).batch), None) == TMED_EINVAL
    for field in ("header", "state", "last_commit"):
        pb = S.PreparedBlocks([case.request()])
        setattr(pb.reqs[0], field, None)
        assert call(pb) == TMED_EINVAL, field
    pb = S.PreparedBlocks([case.request()])
    pb.reqs[0].flags = S.VB_LINK_PREV  # a link on request 0
    assert call(pb) == TMED_EINVAL
    pb = S.PreparedBlocks([case.request()])
    pb.reqs[0].flags = 2
    assert call(pb) == TMED_EINVAL
    pb = S.PreparedBlocks([(case.block, replace(case.state, known=64), False)])
    assert call(pb) == TMED_EINVAL
    pb = S.PreparedBlocks([(case.block, replace(case.state, validators=None), False)])  # its bit is set
    assert call(pb) == TMED_EINVAL
    # a nil LastCommit is an outcome, not a malformed call
    pb = S.PreparedBlocks([(replace(case.block, last_commit=None, commit_basic_ok=False), case.state, False)])
    pb.run_with(VC.oracle_verifier, *VC.oracle_inputs([VC.Case("nil", replace(case.block, last_commit=None,
                                                                              commit_basic_ok=False), case.state)]))
    assert pb.res[0].code == S.VB_COMMIT_BASIC and str(pb.errors()[0]) == "nil LastCommit"
    with pytest.raises(TmedError):  # a failing verifier is the call's error, never a decision
        run_with([case], verifier=lambda *a: 1 / 0)


# ----------------------------------------------------------------------------- host build

def test_replay_under_sanitizers(tmp_path):
    """tests/native/validate_host.cpp: validate_host.h driven by stub hashes and a stub verifier, built
    with AddressSanitizer and UndefinedBehaviorSanitizer by its own makefile; it checks its own outcomes."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "native"), "-f", "validate_host.mk",
                           "OUT=%s" % tmp_path])
    out = subprocess.run([str(tmp_path / "validate_host")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split()[-1] == "validate-ok"


def test_go_binding_static_check():
    """tools/go_cgo_check.py over the binding, all its Go tests (validate_test.go included) and the
    snippets of INTEGRATION.md (the BlockExecutor.ValidateBlock wiring among them)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import go_cgo_check as gc
    header = gc.Header()
    go_dir = os.path.dirname(gc.GO_FILE)
    extra = []
    for name in sorted(os.listdir(go_dir)):
        if name.endswith("_test.go"):
            with open(os.path.join(go_dir, name)) as f:
                extra.append((name, f.read()))
    assert "validate_test.go" in [name for name, _ in extra]
    with open(gc.GO_FILE) as f:
        go = f.read()
    with open(gc.INTEGRATION) as f:
        md = f.read()
    errs, pkg = gc.check_binding(go, header, extra=extra)
    assert errs + gc.check_snippets(md, header, pkg) == []
    assert "func (e *Engine) ValidateBlocks(" in go and "C.tmed_validate_blocks(" in go
    assert "eng.ValidateBlocks(" in md and "LinkPrev" in md and "BlockResult.Skipped" in md
    assert {"tmed_validate_blocks", "tmed_validate_blocks_with", "tmed_validate_stats"} <= set(header.funcs)
    assert {"TMED_VB_GO_PATH", "TMED_VB_LINK_PREV", "TMED_VB_KNOW_NEXT_VALIDATORS"} <= header.macros
