"""VerifyLightClientAttack without a device: the Python restatement (tests/lca_cases.py) on the calls
evidence/verify_test.go:30-357 makes, the seam's replay (tmed_verify_light_client_attacks_with:
csrc/lca_host.h) and tmed_byzantine_validators_host against the restatement with the oracle's hashes and
verifier, the same host code as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/native/lca_host.cpp), and the static check of the Go binding.  The
device run of the same scenarios is tests/test_gpu_lca.py."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import lca_cases as LC
import light_cases as LTC
import tmed.evidence as E
import tmed.types as T
from tmed._native import TMED_EINVAL, TMED_OK, TmedError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_with(cases, stats=None):
    sets = {}
    reqs = [c.request(sets) for c in cases]
    return E.verify_light_client_attacks(None, reqs, verifier=LTC.oracle_verifier, hashes=LC.oracle_hash_arrays(cases),
                                         stats=stats)


# ----------------------------------------------------------------------------- the restatement

def test_restatement_on_the_reference_tests_calls():
    exp = {c.name: c.expected() for c, _ in LC.scenarios()}
    for name in ("lunatic: good", "forward lunatic: time violated", "equivocation: good", "amnesia: good"):
        assert exp[name] is None, (name, exp[name])
    for name, text in (("lunatic: same hash", "trusted header hash matches"),
                       ("lunatic: wrong total power", "total voting power from the evidence and our validator set does not"
                                                      " match (10 != 100)"),
                       ("lunatic: too few malicious votes", "skipping verification of conflicting block failed: invalid "
                                                            "commit -- insufficient voting power: got 30, needed more than 33"),
                       ("forward lunatic: time not violated", "doesn't violate monotonically increasing time "
                                                              "(2006-01-02 16:04:05 +0000 UTC is after 2006-01-02 15:04:05"),
                       ("equivocation: same hash", "trusted header hash matches"),
                       ("equivocation: changed NextValidatorsHash", "expected the conflicting block to be correctly derived"),
                       ("amnesia: same hash", "trusted header hash matches"),
                       ("amnesia: a non-nil claimed list", "expected nil validators from an amnesia light client attack but "
                                                           "got 0")):
        assert exp[name] is not None and text in str(exp[name]), (name, exp[name])
    assert set(range(13)) == {code for _, code in LC.scenarios()}, "every outcome code has a case"


def test_hash_anchor_and_varint():
    hh, height, want = LC.ANCHOR
    assert hashlib.sha256(bytes(range(1, 32)) + b"\x00\x80\x01").digest() == want
    assert LC.evidence_hash_of(hh, height) == want
    assert LC.evidence_hash_of(hh[:31] + b"\xee", height) == want  # byte 31 is never copied
    assert LC.evidence_hash_of(*LC.ANCHOR_NIL[:2]) == LC.ANCHOR_NIL[2] == hashlib.sha256(bytes(32) + b"\x02").digest()
    # encoding/binary's own examples of the zigzag varint
    assert [LC.put_varint(x).hex() for x in (0, -1, 1, -2, 63, -64, 64, -65)] == \
        ["00", "01", "02", "03", "7e", "7f", "8001", "8101"]
    assert [len(LC.put_varint(x)) for x in (1, 63, 64, 1 << 31, 1 << 62, LC.MAX_INT64, -LC.MAX_INT64 - 1)] == \
        [1, 1, 2, 5, 10, 10, 10]


# ----------------------------------------------------------------------------- the seam's replay

def test_seam_reproduces_the_restatement_over_the_whole_table():
    cases = [c for c, _ in LC.scenarios()]
    stats = []
    got = run_with(cases, stats)
    for (case, code), g, (gc, kind, lst, h) in zip(LC.scenarios(), got, stats):
        exp = case.expected()
        assert gc == code, (case.name, E.LCA_CODE_NAMES[gc], exp)
        assert LC.same_outcome(g, exp, code), (case.name, g, exp)
        assert kind == case.kind(), case.name
        if code not in (E.LCA_NOT_DERIVED, E.LCA_GO_PATH):
            assert h == LC.evidence_hash(case.ev), case.name
        else:
            assert h == bytes(32), case.name
        if code in (E.LCA_OK, E.LCA_AMNESIA_HAS_VALIDATORS, E.LCA_BYZ_COUNT, E.LCA_BYZ_ADDRESS, E.LCA_BYZ_POWER):
            assert (E.BYZ_OK, lst) == case.expected_list(), case.name


def test_request_by_request_equals_the_batch():
    cases = [c for c, _ in LC.scenarios()]
    batch = run_with(cases)
    for case, b in zip(cases, batch):
        one = run_with([case])[0]
        assert type(one) is type(b) and str(one) == str(b), case.name


def test_byzantine_validators_host_over_the_table():
    cases = [c for c, _ in LC.scenarios()]
    sets = {}
    got = E.byzantine_validators(None, [c.request(sets) for c in cases])
    for case, (kind, state, lst) in zip(cases, got):
        es, el = case.expected_list()
        assert kind == case.kind() and state == es and lst == el, (case.name, kind, state, lst, es, el)


def test_malformed_calls():
    case = LC.scenarios()[0][0]
    hashes = LC.oracle_hash_arrays([case])
    l = E._bind_lca()

    def call(pl, flags=0, byz_off=None):
        off = pl.byz_off if byz_off is None else byz_off
        fn = T.VERIFY_FN(lambda *a: 0)
        return l.tmed_verify_light_client_attacks_with(pl.reqs, 1, flags, T._ptr(pl.byz), T._ptr(off), pl.res,
                                                       *[T._ptr(a) for a in hashes], fn, None)

    assert call(E.PreparedLca([case.request()]), flags=1) == TMED_EINVAL
    for field in ("conflicting_header", "conflicting_commit", "conflicting_vals", "trusted_header", "trusted_commit",
                  "common_vals", "byz_addresses", "byz_powers"):
        pl = E.PreparedLca([case.request()])
        setattr(pl.reqs[0], field, None)
        assert call(pl) == TMED_EINVAL, field
        assert l.tmed_byzantine_validators_host(pl.reqs, 1, T._ptr(pl.byz), T._ptr(pl.byz_off), pl.bres) == \
            (TMED_EINVAL), field
    pl = E.PreparedLca([case.request()])
    pl.reqs[0].byz_is_nil = 1  # a nil list of four
    assert call(pl) == TMED_EINVAL
    pl = E.PreparedLca([case.request()])
    assert call(pl, byz_off=np.array([0, 9], np.uint64)) == TMED_EINVAL  # shorter than the commit's ten signatures
    assert l.tmed_verify_light_client_attacks(None, pl.reqs, 1, 0, T._ptr(pl.byz), T._ptr(pl.byz_off), pl.res) == TMED_EINVAL
    assert l.tmed_byzantine_validators(None, pl.reqs, 1, T._ptr(pl.byz), T._ptr(pl.byz_off), pl.bres) == TMED_EINVAL
    with pytest.raises(TmedError):  # a failing verifier is the call's error, never a decision
        E.verify_light_client_attacks(None, [case.request()], verifier=lambda *a: 1 / 0, hashes=hashes)
    assert E.verify_light_client_attacks(None, [], verifier=LTC.oracle_verifier, hashes=LC.oracle_hash_arrays([])) == []


# ----------------------------------------------------------------------------- host build

def test_host_code_under_sanitizers(tmp_path):
    """tests/native/lca_host.cpp through its makefile (tests/native/lca_host.mk), built into a temporary
    directory."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "native"), "-f", "lca_host.mk",
                           "OUT=%s" % tmp_path])
    out = subprocess.run([str(tmp_path / "lca_host")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["lca-ok"]


def test_go_binding_static_check():
    """tools/go_cgo_check.py over the binding with lca_test.go and the snippets of INTEGRATION.md."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import go_cgo_check as gc
    header = gc.Header()
    go_dir = os.path.dirname(gc.GO_FILE)
    extra = []
    for name in ("tmedgpu_test.go", "lca_test.go"):
        with open(os.path.join(go_dir, name)) as f:
            extra.append((name, f.read()))
    with open(gc.GO_FILE) as f:
        go = f.read()
    with open(gc.INTEGRATION) as f:
        md = f.read()
    errs, pkg = gc.check_binding(go, header, extra=extra)
    assert errs + gc.check_snippets(md, header, pkg) == []
    assert "func (e *Engine) VerifyLightClientAttacks(" in go and "C.tmed_verify_light_client_attacks(" in go
    assert "func (e *Engine) ByzantineValidators(" in go and "C.tmed_byzantine_validators(" in go
    assert "eng.VerifyLightClientAttacks(" in md
    assert {"tmed_verify_light_client_attacks", "tmed_verify_light_client_attacks_with", "tmed_byzantine_validators",
            "tmed_byzantine_validators_host"} <= set(header.funcs)
    assert {"TMED_LCA_GO_PATH", "TMED_LCA_PANIC", "TMED_BYZ_PANIC", "TMED_LCA_AMNESIA"} <= header.macros
