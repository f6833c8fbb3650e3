package tmedgpu

// ValidateBlocks against the checks of state/validation.go that need no signature: an initial block
// (no VerifyCommit), the outcome codes in the reference's order, the first failing check winning, and
// the Known mask.  Not run in this repository (no Go toolchain); tools/go_cgo_check.py type-checks it.

import (
	"bytes"
	"crypto/sha256"
	"testing"
)

func blockFixture() (*BlockState, *HeaderData, *CommitData) {
	pub := bytes.Repeat([]byte{7}, 32)
	addr := sha256.Sum256(pub)
	vals := &ValSet{PubKeys: pub, Powers: []int64{10}, Addresses: addr[:20], TotalPower: 10}
	empty := sha256.Sum256(nil)
	cons := sha256.Sum256([]byte("consensus-params"))
	st := &BlockState{VersionBlock: 11, ChainID: "block-test", InitialHeight: 1, LastBlockTimeSeconds: 1546300800,
		ConsensusHash: cons[:], Validators: vals, NextValidators: vals, LastValidators: vals, EvidenceMaxBytes: 1000,
		Known: VbKnowAll}
	hdr := &HeaderData{VersionBlock: 11, ChainID: "block-test", Height: 1, TimeSeconds: 1546300800}
	hdr.Hashes[0] = empty[:] // Commit.Hash of no signatures
	hdr.Hashes[1] = empty[:] // Data.Hash of no transactions
	hdr.Hashes[2] = refValsetHash(pub, 10)
	hdr.Hashes[3] = hdr.Hashes[2]
	hdr.Hashes[4] = cons[:]
	hdr.Hashes[7] = empty[:] // EvidenceList.Hash of no evidence
	hdr.Hashes[8] = addr[:20]
	cm := &CommitData{}
	return st, hdr, cm
}

func TestValidateBlocksInitialBlock(t *testing.T) {
	e := engineOrSkip(t)
	st, hdr, cm := blockFixture()
	req := BlockRequest{Header: hdr, LastCommit: cm, State: st, HeaderBasicOK: true, CommitBasicOK: true, EvidenceBasicBad: -1}
	reqs := make([]BlockRequest, 8)
	want := make([]int, len(reqs))
	for i := range reqs {
		reqs[i] = req
	}
	want[0] = VbOK
	reqs[1].HeaderBasicOK = false
	want[1] = VbHeaderBasic
	reqs[2].LastCommit, reqs[2].CommitBasicOK = nil, false
	want[2] = VbCommitBasic
	wrongData := *hdr
	wrongData.Hashes[1] = bytes.Repeat([]byte{1}, 32)
	wrongData.ChainID = "another" // the earlier check wins
	reqs[3].Header = &wrongData
	want[3] = VbDataHash
	wrongVals := *hdr
	wrongVals.Hashes[2] = bytes.Repeat([]byte{2}, 32)
	reqs[4].Header = &wrongVals
	want[4] = VbValidatorsHash
	stranger := *hdr
	stranger.Hashes[8] = make([]byte, 20)
	reqs[5].Header = &stranger
	want[5] = VbProposerUnknown
	late := *hdr
	late.TimeNanos = 5
	reqs[6].Header = &late
	want[6] = VbTimeNotGenesis
	reqs[7].EvidenceByteSize = 1001
	want[7] = VbEvidenceOverflow
	res, err := e.ValidateBlocks(reqs, nil)
	if err != nil {
		t.Fatal(err)
	}
	for i := range res {
		if res[i].Code != want[i] {
			t.Fatalf("request %d: code %d, want %d", i, res[i].Code, want[i])
		}
		if res[i].Verified != 0 {
			t.Fatalf("request %d: an initial block sends no signatures", i)
		}
	}
	if res[0].ProposerIdx != 0 || res[5].ProposerIdx != -1 {
		t.Fatalf("proposer indexes %d, %d", res[0].ProposerIdx, res[5].ProposerIdx)
	}
	if !bytes.Equal(res[4].Hash, hdr.Hashes[2]) {
		t.Fatalf("VbValidatorsHash carries the computed hash, got %x", res[4].Hash)
	}
}

func TestValidateBlocksSkipsUnknownFields(t *testing.T) {
	e := engineOrSkip(t)
	st, hdr, cm := blockFixture()
	spec := *st
	spec.Known = VbKnowAll &^ (VbKnowValidators | VbKnowNextValidators | VbKnowAppHash)
	spec.Validators, spec.NextValidators = nil, nil
	wrong := *hdr
	wrong.Hashes[2] = bytes.Repeat([]byte{2}, 32)
	wrong.Hashes[5] = []byte("an app hash the state does not know yet")
	res, err := e.ValidateBlocks([]BlockRequest{{Header: &wrong, LastCommit: cm, State: &spec, HeaderBasicOK: true,
		CommitBasicOK: true, EvidenceBasicBad: -1}}, nil)
	if err != nil {
		t.Fatal(err)
	}
	if res[0].Code != VbOK || res[0].Skipped != VbKnowValidators|VbKnowNextValidators|VbKnowAppHash {
		t.Fatalf("code %d skipped %#x", res[0].Code, res[0].Skipped)
	}
}
