"""light.Verify without a device: the Python restatement (tests/light_cases.py) against the values
the reference's own tables pin (light/verifier_test.go:19-170, :172-286), the seam's replay
(tmed_light_verify_with: csrc/light_host.h) against the restatement with the oracle's hashes and
verifier, the header-leaf encoder and the replay compiled for the host under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/native/light_host.cpp, a stand-alone program), and the static
check of the Go binding.  The device run of the same scenarios is tests/test_gpu_light.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import light_cases as LC
import tmed.light as L
import tmed.types as T
from oracle import commit as C
from oracle import merkle as M
from tmed._native import TMED_EINVAL, TMED_OK, TmedError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tendermint-fork_amd", "csrc")


same_outcome = LC.same_outcome


def run_with(cases, flags=0, stats=None):
    sets = {}
    pairs = [c.pair(sets) for c in cases]
    return L.verify(None, pairs, flags, verifier=LC.oracle_verifier, hashes=LC.oracle_hash_arrays(cases), stats=stats)


# ----------------------------------------------------------------------------- the restatement

def test_restatement_pins_the_reference_tables():
    kinds = set()
    for case, pinned in LC.tables():
        err = case.expected()
        if pinned is None:
            assert err is None, (case.name, err)
        elif isinstance(pinned, str):
            assert err is not None and pinned in str(err), (case.name, err)
        else:
            kind, got, needed = pinned
            want = {"invalid": L.ErrInvalidHeader, "cant_trust": L.ErrNewValSetCantBeTrusted}[kind]
            assert type(err) is want, (case.name, err)
            assert isinstance(err.reason, C.ErrNotEnoughVotingPowerSigned), (case.name, err)
            assert (err.reason.got, err.reason.needed) == (got, needed), (case.name, err)
            kinds.add((kind, got, needed))
    assert kinds == {("invalid", 50, 93), ("cant_trust", 20, 46)}
    expired = [c for c, p in LC.tables() if p == "old header has expired"][0].expected()
    assert isinstance(expired, L.ErrOldHeaderExpired)
    assert str(expired) == ("old header has expired at 2006-01-02 16:04:05 +0000 UTC "
                            "(now: 2006-01-02 16:04:05 +0000 UTC)")


def test_go_time_and_duration_text():
    assert L.go_time((1136214245, 0)) == "2006-01-02 15:04:05 +0000 UTC"
    assert L.go_time((1136214245, 5000000)) == "2006-01-02 15:04:05.005 +0000 UTC"
    assert L.go_time((-62135596800, 0)) == "0001-01-01 00:00:00 +0000 UTC"
    assert [L.go_duration(d) for d in (0, 1, 1500, 10 * LC.SECOND, 3 * LC.HOUR, 90 * LC.SECOND + 5 * LC.MS, -LC.MS)] == \
        ["0s", "1ns", "1.5µs", "10s", "3h0m0s", "1m30.005s", "-1ms"]
    assert LC.time_add((5, 999999999), 1) == (6, 0) and LC.time_add((5, 0), -1) == (4, 999999999)
    assert LC.time_add((5, 1), -2500000001) == (2, 500000000)


# ----------------------------------------------------------------------------- the seam's replay

def test_seam_reproduces_the_reference_tables():
    cases = [c for c, _ in LC.tables()]
    got = run_with(cases)
    for (case, pinned), g in zip(LC.tables(), got):
        assert LC.same(g, case.expected()), (case.name, g, case.expected())
        if isinstance(pinned, tuple):
            assert (g.reason.got, g.reason.needed) == pinned[1:], (case.name, g)


def test_one_case_per_outcome_precedence_and_boundaries():
    scen = LC.scenarios()
    cases = [c for c, _ in scen]
    pl = L.PreparedLight([c.pair() for c in cases])
    pl.run_with(LC.oracle_verifier, *LC.oracle_hash_arrays(cases))
    got = pl.errors()
    assert set(range(14)) == {code for _, code in scen}  # every outcome code has a case
    for q, (case, code) in enumerate(scen):
        assert pl.res[q].code == code, (case.name, pl.res[q].code, code)
        assert same_outcome(got[q], case.expected(), code), (case.name, got[q], case.expected())
        adjacent = case.untrusted.header["height"] == case.trusted.header["height"] + 1
        assert pl.res[q].adjacent == int(adjacent), case.name
    by_name = {c.name: (pl.res[q], got[q]) for q, c in enumerate(cases)}
    r, e = by_name["commit header hash, nil Header.Hash"]
    assert r.hash_len == 0 and str(e).endswith("header is block ")
    r, e = by_name["vals hash"]
    assert r.hash_len == 32 and bytes(r.hash) == LC.valset_hash([c for c in cases if c.name == "vals hash"][0].vals)
    r, e = by_name["exactly at expiry"]
    assert (r.expired_seconds, r.expired_nanos) == LC.time_add(LC.BTIME, 2 * LC.HOUR)
    r, e = by_name["trusting: zero denominator"]
    assert type(e) is T.GoError and str(e) == "trustLevel has zero Denominator"
    r, e = by_name["trusting failure before light failure"]
    assert isinstance(e, L.ErrNewValSetCantBeTrusted) and e.reason.got == 0


def test_requests_decided_on_the_host_send_no_signatures():
    scen = LC.scenarios()
    stats = []
    run_with([c for c, _ in scen], stats=stats)
    for (case, code), (vt, vl) in zip(scen, stats):
        if code not in (L.OK, L.TRUSTING, L.COMMIT):
            assert (vt, vl) == (0, 0), (case.name, vt, vl)
        if code == L.OK:
            assert vl > 0, case.name


def test_batch_equals_one_request_at_a_time():
    cases = [c for c, _ in LC.scenarios()] + [c for c, _ in LC.tables()]
    batch = run_with(cases)
    for c, b in zip(cases, batch):
        one = run_with([c])[0]
        assert LC.same(one, b) or (isinstance(one, L.GoPath) and isinstance(b, L.GoPath)), (c.name, one, b)


def test_ordered_equals_speculative():
    cases = [c for c, _ in LC.scenarios()] + [c for c, _ in LC.tables()] + LC.c3_shape(6, 7)
    s0, s1 = [], []
    spec, ordered = run_with(cases, 0, s0), run_with(cases, L.LIGHT_ORDERED, s1)
    failed_trusting = 0
    for c, a, b, (vt0, vl0), (vt1, vl1) in zip(cases, spec, ordered, s0, s1):
        assert LC.same(a, b) or (isinstance(a, L.GoPath) and isinstance(b, L.GoPath)), (c.name, a, b)
        assert vt0 == vt1, c.name
        adjacent = c.untrusted.header["height"] == c.trusted.header["height"] + 1
        if not adjacent and (isinstance(b, L.ErrNewValSetCantBeTrusted) or (b is not None and type(b) is T.GoError)):
            assert vl1 == 0, (c.name, vl1)  # a failed Trusting check: the Light request never ran
            failed_trusting += 1
    assert failed_trusting >= 3


def test_c3_shape_cpu():
    cases = LC.c3_shape()
    got = run_with(cases)
    kinds = set()
    for c, g in zip(cases, got):
        exp = c.expected()
        assert LC.same(g, exp), (c.name, g, exp)
        kinds.add("ok" if exp is None else str(exp)[:40])
    assert len(kinds) >= 4  # ok, changed header, wrong set, wrong signature


def test_argument_errors():
    l = L._bind()
    case = LC.scenarios()[0][0]
    hh, ok, vh = LC.oracle_hash_arrays([case])
    fn = T.VERIFY_FN(lambda *a: -3)
    P = T._ptr

    def call(pl, flags=0, hashes=(hh, ok, vh), verify=fn, n=1):
        return l.tmed_light_verify_with(pl.reqs, n, flags, *[None if a is None else P(a) for a in hashes], pl.res,
                                        verify, None)

    pl = L.PreparedLight([case.pair()])
    assert call(pl, n=0) == TMED_OK
    assert call(pl, flags=2) == TMED_EINVAL
    assert call(pl, hashes=(None, ok, vh)) == TMED_EINVAL
    assert call(pl, verify=ctypes.cast(None, T.VERIFY_FN)) == TMED_EINVAL
    assert l.tmed_light_verify_with(None, 1, 0, P(hh), P(ok), P(vh), pl.res, fn, None) == TMED_EINVAL
    assert l.tmed_light_verify(None, pl.reqs, 1, 0, pl.res) == TMED_EINVAL
    for field in ("header", "commit", "vals"):
        pl = L.PreparedLight([case.pair()])
        setattr(pl.reqs[0], field, None)
        assert call(pl) == TMED_EINVAL, field
    # trusted_vals may be NULL for an adjacent pair only
    pl = L.PreparedLight([case.pair()])
    pl.reqs[0].trusted_vals = None
    assert pl.reqs[0].header.contents.height == 2
    pl.run_with(LC.oracle_verifier, hh, ok, vh)
    assert pl.res[0].code == L.OK
    non_adjacent = [c for c, _ in LC.scenarios() if c.name == "ok non-adjacent"][0]
    pl = L.PreparedLight([non_adjacent.pair()])
    pl.reqs[0].trusted_vals = None
    assert call(pl, hashes=LC.oracle_hash_arrays([non_adjacent])) == TMED_EINVAL
    with pytest.raises(TmedError):  # a failing verifier is the call's error, never a decision
        L.verify(None, [case.pair()], verifier=lambda *a: 1 / 0, hashes=(hh, ok, vh))


# ----------------------------------------------------------------------------- host builds

@pytest.fixture(scope="module")
def light_host(tmp_path_factory):
    """tests/native/light_host.cpp built with the sanitizers into a temporary directory."""
    exe = str(tmp_path_factory.mktemp("light") / "light_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "light_host.cpp"), "-o", exe])
    return exe


def _header_lines(headers):
    """The text form tests/native/light_host.cpp reads: one header per line, fields in hex."""
    hx = lambda b: bytes(b).hex() or "-"
    lines = []
    for h in headers:
        bh, pt, ph = h["last_block_id"]
        lines.append(" ".join([str(h["version_block"]), str(h["version_app"]), hx(h["chain_id"].encode()),
                               str(h["height"]), str(h["time"][0]), str(h["time"][1]), hx(bh), str(pt), hx(ph)] +
                              [hx(h[k]) for k in M.HEADER_HASH_FIELDS]))
    return "\n".join(lines) + "\n"


def test_header_leaf_encoder_and_replay_under_sanitizers(light_host, tmp_path):
    """The exact encoder, packer and fold header_hash_kernel compiles (csrc/header_leaf.h), run lane by
    lane on the CPU: hashes equal oracle.merkle.header_hash; and the replay driven by a stub verifier."""
    import header_cases as HC
    headers = [h for h in HC.edge_headers() if HC.fused_ok(h)]
    assert len(headers) > 60
    src = tmp_path / "headers.txt"
    src.write_text(_header_lines(headers))
    out = subprocess.run([light_host, str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split()
    assert lines[-1] == "replay-ok"
    assert len(lines) == len(headers) + 1
    for h, got in zip(headers, lines):
        assert got == (M.header_hash(h) or M.hash_from_byte_slices(M.header_leaves(h))).hex(), h


def test_go_binding_static_check():
    """tools/go_cgo_check.py over the binding, all its Go tests (light_test.go included) and the
    snippets of INTEGRATION.md (the light/verifier.go patch among them)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import go_cgo_check as gc
    header = gc.Header()
    go_dir = os.path.dirname(gc.GO_FILE)
    extra = []
    for name in ("tmedgpu_test.go", "proofs_test.go", "light_test.go"):
        with open(os.path.join(go_dir, name)) as f:
            extra.append((name, f.read()))
    with open(gc.GO_FILE) as f:
        go = f.read()
    with open(gc.INTEGRATION) as f:
        md = f.read()
    errs, pkg = gc.check_binding(go, header, extra=extra)
    assert errs + gc.check_snippets(md, header, pkg) == []
    assert "func (e *Engine) LightVerify(" in go and "C.tmed_light_verify(" in go
    assert "eng.LightVerify(" in md and "ErrNewValSetCantBeTrusted" in md
    assert "tmed_light_verify" in header.funcs and "tmed_light_verify_with" in header.funcs
    assert {"TMED_LIGHT_GO_PATH", "TMED_LIGHT_ORDERED", "TMED_LIGHT_NEXT_VALS_HASH"} <= header.macros
