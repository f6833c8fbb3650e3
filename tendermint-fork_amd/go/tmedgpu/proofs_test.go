package tmedgpu

// Merkle proofs (MerkleProofs, PartSetProofs, TxsProofs, VerifyProofs) against a restatement of the
// reference's recursion (crypto/merkle/proof.go:151-181, :216-237) written here with crypto/sha256.
// Not run in this repository (no Go toolchain); tools/go_cgo_check.py type-checks it.

import (
	"bytes"
	"crypto/sha256"
	"testing"
)

func refLeafHash(leaf []byte) []byte {
	d := sha256.Sum256(append([]byte{0}, leaf...))
	return d[:]
}

func refInnerHash(l, r []byte) []byte {
	d := sha256.Sum256(append(append([]byte{1}, l...), r...))
	return d[:]
}

// getSplitPoint (crypto/merkle/tree.go:103-117)
func refSplitPoint(n int) int {
	k := 1
	for 2*k < n {
		k *= 2
	}
	return k
}

// refProofs returns the root of items and every leaf's aunts, bottom-up, by the split-point
// recursion of trailsFromByteSlices: the aunts of a leaf of the left half end with the right half's
// root, and the other way round.
func refProofs(items [][]byte) ([]byte, [][][]byte) {
	if len(items) == 0 {
		d := sha256.Sum256(nil)
		return d[:], nil
	}
	if len(items) == 1 {
		return refLeafHash(items[0]), [][][]byte{nil}
	}
	k := refSplitPoint(len(items))
	lroot, launts := refProofs(items[:k])
	rroot, raunts := refProofs(items[k:])
	out := make([][][]byte, 0, len(items))
	for _, a := range launts {
		out = append(out, append(a[:len(a):len(a)], rroot))
	}
	for _, a := range raunts {
		out = append(out, append(a[:len(a):len(a)], lroot))
	}
	return refInnerHash(lroot, rroot), out
}

func checkTree(t *testing.T, what string, items [][]byte, got TreeProofs) {
	root, aunts := refProofs(items)
	if !bytes.Equal(got.Root[:], root) {
		t.Fatalf("%s: root %x, want %x", what, got.Root, root)
	}
	if len(got.Proofs) != len(items) {
		t.Fatalf("%s: %d proofs for %d leaves", what, len(got.Proofs), len(items))
	}
	for i, p := range got.Proofs {
		if p.Total != int64(len(items)) || p.Index != int64(i) {
			t.Fatalf("%s: proof %d has total %d index %d", what, i, p.Total, p.Index)
		}
		if !bytes.Equal(p.LeafHash, refLeafHash(items[i])) {
			t.Fatalf("%s: leaf hash %d", what, i)
		}
		if len(p.Aunts) != len(aunts[i]) {
			t.Fatalf("%s: proof %d has %d aunts, want %d", what, i, len(p.Aunts), len(aunts[i]))
		}
		for k, h := range p.Aunts {
			if !bytes.Equal(h, aunts[i][k]) {
				t.Fatalf("%s: proof %d aunt %d", what, i, k)
			}
		}
	}
}

func testItems(n, seed int) [][]byte {
	items := make([][]byte, n)
	for i := range items {
		items[i] = bytes.Repeat([]byte{byte(i + seed), byte(i >> 8), byte(seed)}, (i+seed)%23)
	}
	return items
}

func TestMerkleProofsMatchRecursion(t *testing.T) {
	eng := engineOrSkip(t)
	var trees [][][]byte
	for _, n := range []int{0, 1, 2, 3, 5, 0, 64, 65, 100, 129} {
		trees = append(trees, testItems(n, len(trees)))
	}
	got, err := eng.MerkleProofs(trees)
	if err != nil {
		t.Fatal(err)
	}
	want, err := eng.MerkleRoots(trees)
	if err != nil {
		t.Fatal(err)
	}
	for k, tree := range trees {
		checkTree(t, "tree", tree, got[k])
		if got[k].Root != want[k] {
			t.Fatalf("tree %d: proofs root %x, MerkleRoots %x", k, got[k].Root, want[k])
		}
	}
}

// PartSetProofs is NewPartSetFromData: the parts are the partSize chunks of each block.
func TestPartSetProofsMatchRecursion(t *testing.T) {
	eng := engineOrSkip(t)
	partSize := 100
	blocks := [][]byte{nil, {1}, bytes.Repeat([]byte{7}, 100), bytes.Repeat([]byte{8, 9}, 50*7+1)}
	got, err := eng.PartSetProofs(blocks, uint32(partSize))
	if err != nil {
		t.Fatal(err)
	}
	for k, b := range blocks {
		var parts [][]byte
		for at := 0; at < len(b); at += partSize {
			end := at + partSize
			if end > len(b) {
				end = len(b)
			}
			parts = append(parts, b[at:end])
		}
		checkTree(t, "block", parts, got[k])
	}
}

// TxsProofs builds the tree of Txs.Proof: its leaves are SHA-256(tx).
func TestTxsProofsMatchRecursion(t *testing.T) {
	eng := engineOrSkip(t)
	blocks := [][][]byte{nil, testItems(1, 3), testItems(33, 4)}
	got, err := eng.TxsProofs(blocks)
	if err != nil {
		t.Fatal(err)
	}
	for k, blk := range blocks {
		digests := make([][]byte, len(blk))
		for i, tx := range blk {
			d := sha256.Sum256(tx)
			digests[i] = d[:]
		}
		checkTree(t, "txs", digests, got[k])
	}
}

// Every generated proof verifies; the reference's own mutations (crypto/merkle/tree_test.go:46-102)
// and the Total / Index checks give the codes of Proof.Verify.
func TestVerifyProofsCodes(t *testing.T) {
	eng := engineOrSkip(t)
	items := testItems(100, 9)
	got, err := eng.MerkleProofs([][][]byte{items})
	if err != nil {
		t.Fatal(err)
	}
	roots := [][32]byte{got[0].Root}
	rootOf := make([]uint32, len(items))
	codes, err := eng.VerifyProofs(roots, rootOf, items, got[0].Proofs)
	if err != nil {
		t.Fatal(err)
	}
	for i, c := range codes {
		if c != ProofOK {
			t.Fatalf("proof %d: code %d", i, c)
		}
	}
	p := got[0].Proofs[37]
	long := p
	long.Aunts = append(append([][]byte(nil), p.Aunts...), p.Aunts[0])
	short := p
	short.Aunts = p.Aunts[:len(p.Aunts)-1]
	negTotal, negIndex, other := p, p, p
	negTotal.Total = -1
	negIndex.Index = -1
	other.Index = 38
	badRoot := got[0].Root
	badRoot[0] ^= 1
	leaf := items[37]
	wrongLeaf := append([]byte{1}, leaf...)
	codes, err = eng.VerifyProofs([][32]byte{got[0].Root, badRoot}, []uint32{0, 0, 0, 0, 0, 0, 1},
		[][]byte{leaf, leaf, leaf, leaf, leaf, wrongLeaf, leaf}, []Proof{p, long, short, negTotal, negIndex, p, p})
	if err != nil {
		t.Fatal(err)
	}
	want := []uint8{ProofOK, ProofRootHash, ProofRootHash, ProofNegativeTotal, ProofNegativeIndex, ProofLeafHash,
		ProofRootHash}
	for i := range want {
		if codes[i] != want[i] {
			t.Fatalf("case %d: code %d, want %d", i, codes[i], want[i])
		}
	}
	codes, err = eng.VerifyProofs(roots, nil, [][]byte{leaf}, []Proof{other})
	if err != nil {
		t.Fatal(err)
	}
	if codes[0] != ProofRootHash {
		t.Fatalf("another index: code %d", codes[0])
	}
}
