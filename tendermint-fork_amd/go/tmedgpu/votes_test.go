package tmedgpu

// VerifyVotes: the checks in front of the signature on votes that need no key material (every vote
// here fails a check before its signature is looked at), and the shape of the result.
// Not run in this repository (no Go toolchain); tools/go_cgo_check.py type-checks it.

import (
	"crypto/sha256"
	"testing"
)

// votesFixture: n validators with keys {i+1, 0, ...} and their true addresses, and one vote per
// validator at the step (7, 2, prevote) with a zero BlockID and an all-zero signature.
func votesFixture(n int) (*ValSet, *VoteData) {
	vals := &ValSet{PubKeys: make([]byte, 32*n), Powers: make([]int64, n), Addresses: make([]byte, 20*n)}
	v := NewVoteData(n)
	for i := 0; i < n; i++ {
		vals.PubKeys[32*i] = byte(i + 1)
		vals.Powers[i] = 10
		h := sha256.Sum256(vals.PubKeys[32*i : 32*i+32])
		copy(vals.Addresses[20*i:20*i+20], h[:20])
		copy(v.Addresses[20*i:20*i+20], h[:20])
		v.AddrLens[i] = 20
		v.Types[i], v.Heights[i], v.Rounds[i] = 1, 7, 2
		v.TsSeconds[i] = 1700000000
		v.ValidatorIndexes[i] = int32(i)
		v.SigLens[i] = 64
	}
	return vals, v
}

func TestVerifyVotesPrechecks(t *testing.T) {
	e := engineOrSkip(t)
	vals, v := votesFixture(8)
	v.ValidatorIndexes[0] = -1  // index < 0
	v.AddrLens[1] = 0           // empty address
	v.Rounds[2] = 3             // another step
	v.ValidatorIndexes[3] = 8   // not in the set
	v.Addresses[20*4] ^= 1      // not the set's address
	v.AddrLens[5] = 19          // bytes.Equal: any length but 20 mismatches
	v.BlockHashLens[6] = 31     // malformed hash: VoteSignBytes panics
	v.TsNanos[7] = -1           // no time.Time holds this
	want := []uint8{VoteIndexNegative, VoteAddressEmpty, VoteUnexpectedStep, VoteIndexNotInSet, VoteAddressNotInSet,
		VoteAddressNotInSet, VotePanic, VoteGoPath}
	res, err := e.VerifyVotes([]VoteRequest{{ChainID: "test_chain_id", Vals: vals, Votes: v, AddVote: true, Height: 7, Round: 2, Type: 1}})
	if err != nil {
		t.Fatal(err)
	}
	if len(res) != 1 || len(res[0]) != len(want) {
		t.Fatalf("shape: %d requests", len(res))
	}
	for i := range want {
		if res[0][i] != want[i] {
			t.Fatalf("vote %d: code %d, want %d", i, res[0][i], want[i])
		}
	}
}

func TestVerifyVotesTwoRequests(t *testing.T) {
	e := engineOrSkip(t)
	valsA, a := votesFixture(3)
	valsB, b := votesFixture(5)
	// Vote.Verify alone: the address checks of addVote are off, the all-zero signatures are invalid
	res, err := e.VerifyVotes([]VoteRequest{{ChainID: "a", Vals: valsA, Votes: a}, {ChainID: "b", Vals: valsB, Votes: b}})
	if err != nil {
		t.Fatal(err)
	}
	if len(res) != 2 || len(res[0]) != 3 || len(res[1]) != 5 {
		t.Fatalf("shape: %d requests", len(res))
	}
	for _, r := range res {
		for i, c := range r {
			if c != VoteInvalidSignature {
				t.Fatalf("vote %d: code %d", i, c)
			}
		}
	}
}
