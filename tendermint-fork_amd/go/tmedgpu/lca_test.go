package tmedgpu

// ByzantineValidators and VerifyLightClientAttacks on evidence that needs no key material: the lists
// read no signature, and every request of the second test is decided before a signature is looked at.
// Not run in this repository (no Go toolchain); tools/go_cgo_check.py type-checks it.

import (
	"crypto/sha256"
	"testing"
)

// lcaFixture: a set of n validators of power 10 whose addresses differ in byte `at` only, descending
// in index order, and a lunatic request: every validator signs the conflicting block for the block.
func lcaFixture(n, at int) LcaRequest {
	vals := &ValSet{PubKeys: make([]byte, 32*n), Powers: make([]int64, n), Addresses: make([]byte, 20*n), TotalPower: int64(10 * n)}
	cm := &CommitData{Height: 10, Round: 1, Flags: make([]byte, n), Addresses: make([]byte, 20*n), AddrLens: make([]uint32, n),
		TsSeconds: make([]int64, n), TsNanos: make([]int32, n), Sigs: make([]byte, 64*n), SigLens: make([]uint32, n)}
	for i := 0; i < n; i++ {
		vals.Powers[i] = 10
		vals.Addresses[20*i+at] = byte(n - i)
		cm.Flags[i], cm.AddrLens[i] = 2, 20
		copy(cm.Addresses[20*i:20*i+20], vals.Addresses[20*i:20*i+20])
	}
	conflicting := &HeaderData{ChainID: "c", Height: 10, TimeSeconds: 1700000000}
	trusted := &HeaderData{ChainID: "c", Height: 10, TimeSeconds: 1700000000}
	conflicting.Hashes[2], trusted.Hashes[2] = make([]byte, 32), make([]byte, 32)
	conflicting.Hashes[5], trusted.Hashes[5] = []byte{1}, []byte{2} // AppHash differs: a lunatic attack
	return LcaRequest{ConflictingHeader: conflicting, ConflictingCommit: cm, ConflictingVals: vals, CommonHeight: 4,
		TotalVotingPower: int64(10 * n), ByzIsNil: true, CommonHeaderHeight: 4, TrustedHeader: trusted,
		TrustedCommit: &CommitData{Height: 10, Round: 1}, CommonVals: vals}
}

func TestByzantineValidatorsOrder(t *testing.T) {
	e := engineOrSkip(t)
	reqs := []LcaRequest{lcaFixture(5, 0), lcaFixture(70, 3), lcaFixture(130, 19)}
	amnesia := lcaFixture(4, 4)
	amnesia.TrustedHeader = amnesia.ConflictingHeader
	amnesia.TrustedCommit = &CommitData{Height: 10, Round: 0}
	reqs = append(reqs, amnesia)
	res, err := e.ByzantineValidators(reqs)
	if err != nil {
		t.Fatal(err)
	}
	for q, n := range []int{5, 70, 130} {
		if res[q].Kind != LcaLunatic || res[q].State != ByzOK || len(res[q].List) != n {
			t.Fatalf("request %d: kind %d state %d, %d entries", q, res[q].Kind, res[q].State, len(res[q].List))
		}
		for k, v := range res[q].List { // equal powers: ascending addresses, the reverse of the index order
			if int(v) != n-1-k {
				t.Fatalf("request %d entry %d: validator %d", q, k, v)
			}
		}
	}
	if res[3].Kind != LcaAmnesia || res[3].List != nil {
		t.Fatalf("amnesia: %+v", res[3])
	}
}

func TestVerifyLightClientAttacksBeforeTheSignatures(t *testing.T) {
	e := engineOrSkip(t)
	notDerived := lcaFixture(4, 0)
	notDerived.CommonHeaderHeight = 10 // the same heights and an invalid header
	goPath := lcaFixture(4, 0)
	goPath.TrustedHeader.TimeNanos = 1000000000
	trusting := lcaFixture(4, 0) // all-zero signatures: the Trusting check fails at the first one
	res, err := e.VerifyLightClientAttacks([]LcaRequest{notDerived, goPath, trusting})
	if err != nil {
		t.Fatal(err)
	}
	if res[0].Code != LcaNotDerived || res[1].Code != LcaGoPath || res[2].Code != LcaTrusting || res[2].Commit.Code != WrongSignature {
		t.Fatalf("codes: %d %d %d (%d)", res[0].Code, res[1].Code, res[2].Code, res[2].Commit.Code)
	}
	if res[0].Hash != [32]byte{} || res[0].Kind != LcaLunatic {
		t.Fatalf("not derived: %+v", res[0])
	}
	// Hash(): the header hash's first 31 bytes, a zero byte, the zigzag varint of CommonHeight (4 -> 08)
	if res[2].Hash == [32]byte{} || res[2].Hash == sha256.Sum256(nil) {
		t.Fatalf("hash: %x", res[2].Hash)
	}
}
