package tmedgpu

// VerifyDuplicateVotes and EvidenceHashes: the checks in front of the signatures on evidence that
// needs no key material (every evidence here fails a check before a signature is looked at), the
// hash of the all-zero evidence, and the shape of the results.
// Not run in this repository (no Go toolchain); tools/go_cgo_check.py type-checks it.

import (
	"crypto/sha256"
	"testing"
)

// evidenceFixture: the validators of votesFixture and one evidence per validator: two prevotes at
// (7, 2) carrying the validator's address, VoteB for a block, all-zero signatures, the set's powers.
func evidenceFixture(n int) (*ValSet, *DupEvidenceData) {
	vals, _ := votesFixture(n)
	vals.TotalPower = int64(10 * n)
	d := NewDupEvidenceData(n)
	for i := 0; i < n; i++ {
		for k := 0; k < 2; k++ {
			j := 2*i + k
			copy(d.Votes.Addresses[20*j:20*j+20], vals.Addresses[20*i:20*i+20])
			d.Votes.AddrLens[j] = 20
			d.Votes.Types[j], d.Votes.Heights[j], d.Votes.Rounds[j] = 1, 7, 2
			d.Votes.TsSeconds[j] = 1700000000
			d.Votes.ValidatorIndexes[j] = int32(i)
			d.Votes.SigLens[j] = 64
		}
		d.Votes.BlockHashes[32*(2*i+1)] = 0xaa
		d.Votes.BlockHashLens[2*i+1] = 32
		d.TotalVotingPowers[i], d.ValidatorPowers[i] = int64(10*n), 10
		d.TsSeconds[i] = 1700000001
	}
	return vals, d
}

func TestVerifyDuplicateVotesPrechecks(t *testing.T) {
	e := engineOrSkip(t)
	vals, d := evidenceFixture(9)
	d.Votes.Addresses[20*0] ^= 1     // evidence 0: nobody has VoteA's address
	d.Votes.Rounds[2*1+1] = 3        // 1: h/r/s
	d.Votes.AddrLens[2*2+1] = 19     // 2: the addresses differ
	d.Votes.BlockHashLens[2*3+1] = 0 // 3: both for nil: the same BlockID
	d.ValidatorPowers[4] = 11        // 4
	d.TotalVotingPowers[5] = 1       // 5
	d.Votes.BlockHashLens[2*6] = 31  // 6: VoteA's sign-bytes panic
	d.Votes.TsNanos[2*7] = -1        // 7: no time.Time holds this
	want := []uint8{DupVoteNotAValidator, DupVoteHRSMismatch, DupVoteAddressMismatch, DupVoteSameBlockID,
		DupVoteValidatorPower, DupVoteTotalPower, DupVotePanic, DupVoteGoPath, DupVoteVoteASignature}
	res, err := e.VerifyDuplicateVotes([]DupVoteRequest{{ChainID: "test_chain_id", Vals: vals, Evidence: d}})
	if err != nil {
		t.Fatal(err)
	}
	if len(res) != 1 || len(res[0]) != len(want) {
		t.Fatalf("shape: %d requests", len(res))
	}
	for i := range want {
		if res[0][i] != want[i] {
			t.Fatalf("evidence %d: code %d, want %d", i, res[0][i], want[i])
		}
	}
}

func TestEvidenceHashes(t *testing.T) {
	e := engineOrSkip(t)
	d := NewDupEvidenceData(2)
	d.Votes.SigLens[3] = 65 // evidence 1: a signature the arrays do not carry
	zero := []byte{0x0a, 0x06, 0x22, 0x02, 0x12, 0x00, 0x2a, 0x00, 0x12, 0x06, 0x22, 0x02, 0x12, 0x00, 0x2a, 0x00, 0x2a, 0x00}
	lists := [][]EvidenceItem{{{Index: 0}}, {}, {{Index: 0}, {Index: 1}}, {{Opaque: []byte("lca")}}}
	hashes, roots, evOK, listOK, err := e.EvidenceHashes(d, lists)
	if err != nil {
		t.Fatal(err)
	}
	if len(hashes) != 2 || len(roots) != 4 || !evOK[0] || evOK[1] || !listOK[0] || !listOK[1] || listOK[2] || !listOK[3] {
		t.Fatalf("shape or ok flags: %v %v", evOK, listOK)
	}
	if hashes[0] != sha256.Sum256(zero) || hashes[1] != [32]byte{} {
		t.Fatalf("hashes: %x", hashes)
	}
	if roots[0] != sha256.Sum256(append([]byte{0}, zero...)) || roots[1] != sha256.Sum256(nil) || roots[2] != [32]byte{} ||
		roots[3] != sha256.Sum256([]byte("\x00lca")) {
		t.Fatalf("roots: %x", roots)
	}
}
