"""The outcomes the ZIP-215 rule must produce at the seam, pinned without a device: the existing
tmed_verify_commits_with and tmed_light_verify_with (the seam's own planning, candidate selection and
replay, host C++) with oracle.zip215.verify as the caller's verifier, on the commits of
tests/zip_rule_cases.py that the two rules disagree on.  Expected outcomes: oracle.commit (and the
light.Verify restatement of tests/light_cases.py) run with that same verifier.  These are the values
tests/test_gpu_zip_rule.py asks of tmed_set_rule(TMED_RULE_ZIP215) on the device; this file checks
the fixtures and passes with or without the rule setting."""
import pytest

import light_cases as LC
import tmed.light as L
import tmed.types as T
import zip_rule_cases as ZR
from commit_cases import pbid, same, to_product


def _requests(mode, n, kind, at, **kw):
    vs, _, bid, h, cm = ZR.commit(n, kind, at, **kw)
    pv, pc = to_product(vs, cm)
    return (vs, bid, h, cm), (mode, pv, ZR.CHAIN, pbid(bid) if mode != T.MODE_LIGHT_TRUSTING else None, h, pc, 1, 3)


@pytest.mark.parametrize("n", [4, 175])
@pytest.mark.parametrize("kind", ["torsion", "noncanon", "flip", "splusl", "flip_torsion"])
def test_verify_commit_under_both_verifiers(n, kind):
    """VerifyCommit on 4 and 175 validators: the divergent signature is WRONG_SIGNATURE at its index
    under the Go verifier and OK under ZIP-215; a flipped bit and S + L fail under both, same index."""
    at = n // 2
    (vs, bid, h, cm), req = _requests(T.MODE_COMMIT, n, kind, at)
    exp_go, exp_zip = ZR.expected(0, vs, bid, h, cm, rule="go"), ZR.expected(0, vs, bid, h, cm, rule="zip")
    assert str(exp_go).startswith("wrong signature (#%d)" % at)
    if kind in ("torsion", "noncanon"):
        assert exp_zip is None
    else:
        assert str(exp_zip) == str(exp_go)
    got = T.verify_commits(None, [req], verifier=ZR.zip_batch_verifier)[0]
    assert same(got, exp_zip), (got, exp_zip)
    got = T.verify_commits(None, [req], verifier=LC.oracle_verifier)[0]
    assert same(got, exp_go), (got, exp_go)


def test_early_exit_loops_on_seven_validators():
    """LIGHT and LIGHT_TRUSTING with the divergent signature in front of the power crossing: under Go
    the loop stops there, under ZIP-215 it runs to the crossing; the tallies differ as oracle.commit says."""
    for mode in (T.MODE_LIGHT, T.MODE_LIGHT_TRUSTING):
        (vs, bid, h, cm), req = _requests(mode, 7, "torsion", 1)
        exp_go, exp_zip = (ZR.expected(mode, vs, bid, h, cm, rule=r) for r in ("go", "zip"))
        assert exp_zip is None and str(exp_go).startswith("wrong signature (#1)")
        stats = []
        got = T.verify_commits(None, [req], verifier=ZR.zip_batch_verifier, stats=stats)[0]
        assert same(got, exp_zip)
        assert same(T.verify_commits(None, [req], verifier=LC.oracle_verifier)[0], exp_go)
    # not enough power once the divergent vote is the only one for the block: `got` differs by its power
    flags = (3, 2, 3, 3, 3, 3, 3)
    (vs, bid, h, cm), req = _requests(T.MODE_LIGHT, 7, "torsion", 1, flags=flags)
    exp_go, exp_zip = (ZR.expected(1, vs, bid, h, cm, rule=r) for r in ("go", "zip"))
    assert str(exp_go).startswith("wrong signature (#1)") and type(exp_zip).__name__ == "ErrNotEnoughVotingPowerSigned"
    assert (exp_zip.got, exp_zip.needed) == (10, 46)
    assert same(T.verify_commits(None, [req], verifier=ZR.zip_batch_verifier)[0], exp_zip)


def test_light_verify_under_both_verifiers():
    cases = ZR.light_cases()
    hh, ok, vh = LC.oracle_hash_arrays(cases)
    for rule, verifier in (("go", LC.oracle_verifier), ("zip", ZR.zip_batch_verifier)):
        sets = {}
        pl = L.PreparedLight([c.pair(sets) for c in cases])
        pl.run_with(verifier, hh, ok, vh)
        for q, c in enumerate(cases):
            exp = ZR.light_expected(c, rule)
            assert (exp is None) == (rule == "zip"), c.name
            assert LC.same_outcome(pl.errors()[q], exp, pl.res[q].code), (c.name, rule, pl.errors()[q], exp)
