package tmedgpu

// LightVerify against the checks of light/verifier.go that need no signature: the outcome codes in
// the reference's order, the first failing check winning, and Go's time arithmetic at its edges.
// Not run in this repository (no Go toolchain); tools/go_cgo_check.py type-checks it.

import (
	"bytes"
	"crypto/sha256"
	"testing"
)

// refValsetHash: ValidatorSet.Hash of a one-validator set (types/validator_set.go:347-353): the leaf
// hash of SimpleValidator{PubKey ed25519, VotingPower}.
func refValsetHash(pub []byte, power byte) []byte {
	leaf := append([]byte{0x00, 0x0a, 0x22, 0x0a, 0x20}, pub...)
	leaf = append(leaf, 0x10, power)
	d := sha256.Sum256(leaf)
	return d[:]
}

func lightFixture() (*ValSet, *HeaderData, *CommitData) {
	pub := bytes.Repeat([]byte{7}, 32)
	vals := &ValSet{PubKeys: pub, Powers: []int64{10}, Addresses: make([]byte, 20), TotalPower: 10}
	hdr := &HeaderData{VersionBlock: 11, ChainID: "light-test", Height: 2, TimeSeconds: 1136217845}
	hdr.Hashes[2] = refValsetHash(pub, 10)
	hdr.Hashes[3] = hdr.Hashes[2]
	cm := &CommitData{Height: 2, Round: 1, BlockID: BlockID{Hash: make([]byte, 32), PSHTotal: 1, PSHHash: make([]byte, 32)},
		Flags: []byte{1}, Addresses: make([]byte, 20), AddrLens: []uint32{0}, TsSeconds: []int64{0}, TsNanos: []int32{0},
		Sigs: make([]byte, 64), SigLens: []uint32{0}}
	return vals, hdr, cm
}

func lightRequest(vals *ValSet, hdr *HeaderData, cm *CommitData) LightRequest {
	return LightRequest{ChainID: "light-test", TrustedHeight: 1, TrustedTimeSeconds: 1136214245,
		TrustedNextValsHash: hdr.Hashes[2], TrustedVals: vals, Header: hdr, Commit: cm, Vals: vals, BasicOK: true,
		TrustingPeriodNs: 3 * 3600 * 1000000000, MaxClockDriftNs: 10 * 1000000000, NowSeconds: 1136214245 + 7200,
		TrustNum: 1, TrustDen: 3}
}

func TestLightVerifyHostDecidedOutcomes(t *testing.T) {
	e := engineOrSkip(t)
	vals, hdr, cm := lightFixture()
	reqs := make([]LightRequest, 8)
	for i := range reqs {
		reqs[i] = lightRequest(vals, hdr, cm)
	}
	want := make([]int, len(reqs))
	// the commit signs another block: the header hash is computed and returned
	want[0] = LightCommitHeaderHash
	// exactly at expiry: expired, and that wins over the wrong header hash
	reqs[1].TrustingPeriodNs = 7200 * 1000000000
	want[1] = LightOldHeaderExpired
	reqs[2].BasicOK = false
	want[2] = LightHeaderBasic
	reqs[3].ChainID = "another"
	want[3] = LightWrongChain
	other := *cm
	other.Height = 3
	reqs[4].Commit = &other
	want[4] = LightCommitHeight
	// the header-hash compare comes before the height and time checks
	reqs[5].TrustedHeight = 2
	want[5] = LightCommitHeaderHash
	reqs[6].TrustedTimeSeconds = hdr.TimeSeconds
	want[6] = LightCommitHeaderHash
	reqs[7].NowSeconds = 253402300800
	want[7] = LightGoPath
	for _, flags := range []uint32{0, LightOrdered} {
		res, err := e.LightVerify(reqs, flags)
		if err != nil {
			t.Fatal(err)
		}
		for i := range res {
			if res[i].Code != want[i] {
				t.Fatalf("flags %d request %d: code %d, want %d", flags, i, res[i].Code, want[i])
			}
			if res[i].VerifiedTrusting != 0 || res[i].VerifiedLight != 0 {
				t.Fatalf("request %d sent signatures", i)
			}
		}
		if len(res[0].Hash) != 32 || bytes.Equal(res[0].Hash, cm.BlockID.Hash) {
			t.Fatalf("header hash %x", res[0].Hash)
		}
		if res[1].ExpiredSeconds != 1136214245+7200 || res[1].ExpiredNanos != 0 {
			t.Fatalf("expiry %d.%09d", res[1].ExpiredSeconds, res[1].ExpiredNanos)
		}
		if !res[0].Adjacent || res[5].Adjacent {
			t.Fatalf("adjacent flags")
		}
	}
}

func TestLightVerifyHashChecksAfterTheHeaderHash(t *testing.T) {
	e := engineOrSkip(t)
	vals, hdr, cm := lightFixture()
	// learn the header's hash from the first call, then let the commit sign it
	res, err := e.LightVerify([]LightRequest{lightRequest(vals, hdr, cm)}, 0)
	if err != nil || res[0].Code != LightCommitHeaderHash {
		t.Fatalf("first call: %v %v", res, err)
	}
	cm.BlockID.Hash = res[0].Hash
	reqs := []LightRequest{lightRequest(vals, hdr, cm), lightRequest(vals, hdr, cm), lightRequest(vals, hdr, cm),
		lightRequest(vals, hdr, cm)}
	reqs[0].TrustedHeight = 2 // not greater
	reqs[1].TrustedTimeSeconds = hdr.TimeSeconds
	reqs[2].NowSeconds = hdr.TimeSeconds - 10 // exactly now + drift
	reqs[3].TrustedNextValsHash = make([]byte, 32)
	want := []int{LightHeightNotGreater, LightTimeNotAfter, LightTimeFromFuture, LightNextValsHash}
	res, err = e.LightVerify(reqs, 0)
	if err != nil {
		t.Fatal(err)
	}
	for i := range res {
		if res[i].Code != want[i] {
			t.Fatalf("request %d: code %d, want %d", i, res[i].Code, want[i])
		}
	}
	// the only signature is absent: VerifyCommitLight tallies nothing
	ok, err := e.LightVerify([]LightRequest{lightRequest(vals, hdr, cm)}, LightOrdered)
	if err != nil || ok[0].Code != LightCommit || ok[0].Commit.Code != NotEnoughPower || ok[0].Commit.Needed != 6 {
		t.Fatalf("commit check: %v %v", ok, err)
	}
}
