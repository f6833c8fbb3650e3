package tmedgpu

// SetRule / Rule and VerifyBatchKeysetZIP215 on tuples of tests/golden/zip215_vectors.json.
// Not run in this repository (no Go toolchain).

import (
	"encoding/hex"
	"testing"
)

func mustHex(t *testing.T, s string) []byte {
	b, err := hex.DecodeString(s)
	if err != nil {
		t.Fatal(err)
	}
	return b
}

func TestRuleSetting(t *testing.T) {
	e := engineOrSkip(t)
	if e.Rule() != RuleGo {
		t.Fatalf("a new engine's rule is %d", e.Rule())
	}
	if err := e.SetRule(RuleZIP215); err != nil {
		t.Fatal(err)
	}
	if e.Rule() != RuleZIP215 {
		t.Fatalf("rule %d after SetRule(RuleZIP215)", e.Rule())
	}
	if err := e.SetRule(7); err == nil {
		t.Fatal("SetRule(7) must fail")
	}
	if err := e.SetRule(RuleGo); err != nil {
		t.Fatal(err)
	}
}

func TestVerifyBatchKeysetZIP215(t *testing.T) {
	e := engineOrSkip(t)
	// class zip_R_mixed (R with a small-order component: ZIP-215 accepts, Go rejects), class zip_flip (both reject)
	pubs := append(mustHex(t, "c6d2268ed0cc479d7441ca16d6b96ab8349697506a08b916b64b60684ff179eb"),
		mustHex(t, "fd546167d7338f2c17077d0c496e2a86d84291b4de643a021366ef9a29dbfe29")...)
	msgs := [][]byte{mustHex(t, "7a69703231352052206d697865642030"), mustHex(t, "7a6970206e65672030")}
	sigs := [][]byte{
		mustHex(t, "9d4763f8e181b5064430afe62920dbcd1c2a93aa2e90d9c0fc44ade8bce40687a217bea09168bed1631e2748349ad503cff027fe71efb5d467cb3debd275c305"),
		mustHex(t, "b740584d1b2fba6b8f40b186a37b7bd0825c06832fa3a4b9a32ad31405687d33586d414938e8c22cd8994aafdacf33705c5c8baecd2b18c730d55e0201383800"),
	}
	h, err := e.LoadKeyset(pubs)
	if err != nil {
		t.Fatal(err)
	}
	defer e.FreeKeyset(h)
	ok, err := e.VerifyBatchKeysetZIP215(h, []uint32{0, 1}, msgs, sigs)
	if err != nil {
		t.Fatal(err)
	}
	if len(ok) != 2 || !ok[0] || ok[1] {
		t.Fatalf("ZIP-215 decisions %v, want [true false]", ok)
	}
	goRule, err := e.VerifyBatch(pubs, msgs, sigs)
	if err != nil {
		t.Fatal(err)
	}
	if goRule[0] || goRule[1] {
		t.Fatalf("Go-rule decisions %v, want [false false]", goRule)
	}
	if _, err := e.VerifyBatchKeysetZIP215(h, []uint32{0, 2}, msgs, sigs); err == nil {
		t.Fatal("a key index past the set must be refused")
	}
}
