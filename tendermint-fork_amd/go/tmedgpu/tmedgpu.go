// Package tmedgpu is the reference-side cgo binding of libtmed25519_hip.so
// (include/tmed25519.h) for Tendermint Core v0.34.24.
//
// It is NOT compiled in this repository (no Go toolchain in the build image); tools/go_cgo_check.py
// type-checks it statically against include/tmed25519.h instead (tests/test_go_binding.py).  It is
// the shim a maintainer adds under github.com/tendermint/tendermint/crypto/ to route the
// commit-verification loops to the GPU.  See INTEGRATION.md.
//
// Seam (SURVEY.md §8b): ValidatorSet.VerifyCommit / VerifyCommitLight /
// VerifyCommitLightTrusting (types/validator_set.go:667-826) call
// VerifyCommitsGPU instead of looping over crypto.PubKey.VerifySignature
// (crypto/ed25519/ed25519.go:148-155).  Any error returned here means "take the
// original Go path": the caller never guesses a decision.
package tmedgpu

/*
#cgo CFLAGS: -I${SRCDIR}/../../../include
#cgo LDFLAGS: -L${SRCDIR}/../../lib -ltmed25519_hip -Wl,-rpath,${SRCDIR}/../../lib
#include <stdlib.h>
#include "tmed25519.h"
*/
import "C"

import (
	"errors"
	"sync"
	"unsafe"
)

// Engine wraps one tmed_ctx (one per GPU; safe for concurrent use: the
// library serialises calls on a context).
type Engine struct {
	ctx *C.tmed_ctx
	// page-locked arena the blocksync signatures are marshalled into (grow-only, kept across
	// calls): the library DMAs them from it instead of copying them through its staging area
	pinMu  sync.Mutex
	pin    unsafe.Pointer
	pinCap int
	arenas chan *arena // reusable C arenas (getArena / putArena)
}

func newEngine(ctx *C.tmed_ctx) *Engine { return &Engine{ctx: ctx, arenas: make(chan *arena, 8)} }

// pinnedSigs returns the engine's pinned arena grown to at least n bytes (nil if
// tmed_host_alloc fails: the caller then marshals into ordinary C memory).  Holds pinMu.
func (e *Engine) pinnedSigs(n int) unsafe.Pointer {
	if n > e.pinCap {
		if e.pin != nil {
			C.tmed_host_free(e.pin)
			e.pin, e.pinCap = nil, 0
		}
		var p unsafe.Pointer
		if C.tmed_host_alloc(C.size_t(n+n/4), &p) != 0 {
			return nil
		}
		e.pin, e.pinCap = p, n+n/4
	}
	return e.pin
}

var (
	once    sync.Once
	defEng  *Engine
	initErr error
)

// Default returns the process-wide engine on device 0 (or the init error).
func Default() (*Engine, error) {
	once.Do(func() {
		var ctx *C.tmed_ctx
		if rc := C.tmed_init(0, &ctx); rc != 0 {
			initErr = errors.New(C.GoString(C.tmed_strerror(rc)))
			return
		}
		defEng = newEngine(ctx)
	})
	return defEng, initErr
}

// Mode selects the reference loop being replaced.
type Mode int

const (
	ModeCommit         Mode = C.TMED_MODE_COMMIT
	ModeLight          Mode = C.TMED_MODE_LIGHT
	ModeLightTrusting  Mode = C.TMED_MODE_LIGHT_TRUSTING
)

// Outcome codes (see tmed25519.h); the caller formats the same errors Go does.
const (
	OK              = C.TMED_COMMIT_OK
	WrongSetSize    = C.TMED_COMMIT_WRONG_SET_SIZE
	WrongHeight     = C.TMED_COMMIT_WRONG_HEIGHT
	WrongBlockID    = C.TMED_COMMIT_WRONG_BLOCK_ID
	WrongSignature  = C.TMED_COMMIT_WRONG_SIGNATURE
	NotEnoughPower  = C.TMED_COMMIT_NOT_ENOUGH_POWER
	DoubleVote      = C.TMED_COMMIT_DOUBLE_VOTE
	ZeroDenominator = C.TMED_COMMIT_ZERO_DENOMINATOR
	Overflow        = C.TMED_COMMIT_OVERFLOW
	// Panic: the reference loop panics when it reaches signature Idx (unknown BlockIDFlag,
	// malformed BlockID hash); the caller runs the original Go method, which panics as before.
	Panic = C.TMED_COMMIT_PANIC
)

// ValSet / CommitData are flat copies of types.ValidatorSet / types.Commit
// (filled by the caller in package types, which owns those types).
type ValSet struct {
	PubKeys     []byte  // n x 32
	Powers      []int64 // n
	Addresses   []byte  // n x 20 (every Validator.Address is 20 bytes; see verifyCommitGPU)
	TotalPower  int64
	Keyset      uint64   // 0: the engine's key-set cache decides (the default); or a LoadKeyset handle
	KeysetIndex []uint32 // nil, or validator i -> index in the key set
	// nil, or ValidatorSet.Hash() (types/validator_set.go:347-353) when the caller has it at no cost
	// (a header's ValidatorsHash after its check): the key-set cache's key for this set.  Without it
	// the library keys the set by a digest of PubKeys; a hit is compared key by key either way.
	SetHash []byte
	cmem    bool // PubKeys / Powers / Addresses already live in C memory (Batch.NewValSet)
}

// valset builds the C struct of v (its slices copied into the arena).
func (a *arena) valset(v *ValSet) C.tmed_valset {
	var sh *C.uint8_t
	if len(v.SetHash) == 32 {
		sh = a.bytes(v.SetHash)
	}
	t := C.tmed_valset{n: C.size_t(len(v.Powers)), total_power: C.int64_t(v.TotalPower), keyset: C.uint64_t(v.Keyset),
		keyset_index: a.u32(v.KeysetIndex), set_hash: sh}
	if v.cmem {
		t.pubkeys, t.addresses = ptr8(v.PubKeys), ptr8(v.Addresses)
		if len(v.Powers) > 0 {
			t.powers = (*C.int64_t)(unsafe.Pointer(&v.Powers[0]))
		}
	} else {
		t.pubkeys, t.powers, t.addresses = a.bytes(v.PubKeys), a.i64(v.Powers), a.bytes(v.Addresses)
	}
	return t
}

type BlockID struct {
	Hash     []byte
	PSHTotal uint32
	PSHHash  []byte
}

type CommitData struct {
	Height    int64
	Round     int32
	BlockID   BlockID
	Flags     []byte  // BlockIDFlag per signature
	Addresses []byte  // n x 20 (zero-padded slots; AddrLens gives the real lengths)
	AddrLens  []uint32 // len(ValidatorAddress) per signature: only 20 can match (bytes.Equal)
	TsSeconds []int64
	TsNanos   []int32
	Sigs      []byte // n x 64 (zero padded)
	SigLens   []uint32
	cmem      bool // every array already lives in C memory (Batch.NewCommit / WindowBuilder.NewCommit)
}

// newCommitIn: a CommitData of n signatures whose arrays are allocated in C memory (the arena;
// Sigs at sigs when given: a pinned buffer) for the caller to fill in place — the shim then hands
// the library those pointers with no second copy.
func newCommitIn(a *arena, n int, sigs unsafe.Pointer) *CommitData {
	c := &CommitData{cmem: true}
	c.Flags = unsafe.Slice((*byte)(a.alloc(uintptr(n))), n)
	c.Addresses = unsafe.Slice((*byte)(a.alloc(uintptr(20*n))), 20*n)
	c.AddrLens = unsafe.Slice((*uint32)(a.alloc(uintptr(4*n))), n)
	c.TsSeconds = unsafe.Slice((*int64)(a.alloc(uintptr(8*n))), n)
	c.TsNanos = unsafe.Slice((*int32)(a.alloc(uintptr(4*n))), n)
	if sigs == nil {
		sigs = a.alloc(uintptr(64 * n))
	}
	c.Sigs = unsafe.Slice((*byte)(sigs), 64*n)
	c.SigLens = unsafe.Slice((*uint32)(a.alloc(uintptr(4*n))), n)
	return c
}

func newValSetIn(a *arena, n int) *ValSet {
	v := &ValSet{cmem: true}
	v.PubKeys = unsafe.Slice((*byte)(a.alloc(uintptr(32*n))), 32*n)
	v.Powers = unsafe.Slice((*int64)(a.alloc(uintptr(8*n))), n)
	v.Addresses = unsafe.Slice((*byte)(a.alloc(uintptr(20*n))), 20*n)
	return v
}

func ptr8(b []byte) *C.uint8_t {
	if len(b) == 0 {
		return nil
	}
	return (*C.uint8_t)(unsafe.Pointer(&b[0]))
}

// commitC: the C struct of c (its arrays passed as they are when they live in C memory, else
// copied into the arena once).  sigs: where the signatures go instead (nil: as above).
func (a *arena) commitC(c *CommitData, sigs *C.uint8_t) C.tmed_commit {
	t := C.tmed_commit{height: C.int64_t(c.Height), round: C.int32_t(c.Round), block_id: a.blockID(&c.BlockID),
		n_sigs: C.size_t(len(c.Flags))}
	if c.cmem {
		t.flags, t.addresses, t.sigs = ptr8(c.Flags), ptr8(c.Addresses), ptr8(c.Sigs)
		if len(c.Flags) > 0 {
			t.ts_seconds = (*C.int64_t)(unsafe.Pointer(&c.TsSeconds[0]))
			t.ts_nanos = (*C.int32_t)(unsafe.Pointer(&c.TsNanos[0]))
			t.sig_lens = (*C.uint32_t)(unsafe.Pointer(&c.SigLens[0]))
			t.address_lens = (*C.uint32_t)(unsafe.Pointer(&c.AddrLens[0]))
		}
	} else {
		t.flags, t.addresses, t.sigs = a.bytes(c.Flags), a.bytes(c.Addresses), a.bytes(c.Sigs)
		t.ts_seconds, t.ts_nanos = a.i64(c.TsSeconds), a.i32(c.TsNanos)
		t.sig_lens, t.address_lens = a.u32(c.SigLens), a.u32(c.AddrLens)
	}
	if sigs != nil {
		t.sigs = sigs
	}
	return t
}

type Request struct {
	Mode       Mode
	ChainID    string
	Vals       *ValSet
	BlockID    *BlockID
	Height     int64
	Commit     *CommitData
	TrustNum   int64
	TrustDen   int64
}

type Result struct {
	Code                   int
	Got, Needed            int64
	Expected, Actual       int64
	Idx, IdxFirst, ValIdx  int32
}

// cgo pointer rules (Go 1.18: no runtime.Pinner): C memory must not hold Go pointers, so every
// input the library reads lives in C memory for the duration of the call.  An arena is a bump
// allocator over C blocks that are KEPT across calls (Engine.getArena / putArena): a call costs no
// malloc per array and no fresh pages.  The flat arrays of a Batch's commits and validator sets
// are allocated in the arena first and filled by the caller in place (NewCommit / NewValSet: Go
// slices over C memory), so nothing is copied twice; slices the caller built in Go memory (the
// Request form) are copied in once.
type arena struct {
	blocks []unsafe.Pointer // C blocks, reused after reset
	sizes  []uintptr
	cur    int     // block being filled
	off    uintptr // offset in it
}

const arenaBlock = 8 << 20

func (a *arena) alloc(sz uintptr) unsafe.Pointer {
	sz = (sz + 15) &^ 15
	for a.cur < len(a.blocks) {
		if a.off+sz <= a.sizes[a.cur] {
			p := unsafe.Add(a.blocks[a.cur], a.off)
			a.off += sz
			return p
		}
		a.cur++
		a.off = 0
	}
	n := uintptr(arenaBlock)
	if sz > n {
		n = sz
	}
	p := C.malloc(C.size_t(n))
	a.blocks = append(a.blocks, p)
	a.sizes = append(a.sizes, n)
	a.cur, a.off = len(a.blocks)-1, sz
	return p
}

// inArena: b already lives in this arena's C memory (filled in place): pass it as is.
func (a *arena) inArena(b unsafe.Pointer) bool {
	for i, blk := range a.blocks {
		if uintptr(b) >= uintptr(blk) && uintptr(b) < uintptr(blk)+a.sizes[i] {
			return true
		}
	}
	return false
}

func (a *arena) bytes(b []byte) *C.uint8_t {
	if len(b) == 0 {
		return nil
	}
	if a.inArena(unsafe.Pointer(&b[0])) {
		return (*C.uint8_t)(unsafe.Pointer(&b[0]))
	}
	p := a.alloc(uintptr(len(b)))
	copy(unsafe.Slice((*byte)(p), len(b)), b)
	return (*C.uint8_t)(p)
}

func (a *arena) i64(v []int64) *C.int64_t {
	if len(v) == 0 {
		return nil
	}
	if a.inArena(unsafe.Pointer(&v[0])) {
		return (*C.int64_t)(unsafe.Pointer(&v[0]))
	}
	p := a.alloc(uintptr(len(v)) * 8)
	copy(unsafe.Slice((*int64)(p), len(v)), v)
	return (*C.int64_t)(p)
}

func (a *arena) i32(v []int32) *C.int32_t {
	if len(v) == 0 {
		return nil
	}
	if a.inArena(unsafe.Pointer(&v[0])) {
		return (*C.int32_t)(unsafe.Pointer(&v[0]))
	}
	p := a.alloc(uintptr(len(v)) * 4)
	copy(unsafe.Slice((*int32)(p), len(v)), v)
	return (*C.int32_t)(p)
}

func (a *arena) u32(v []uint32) *C.uint32_t {
	if len(v) == 0 {
		return nil
	}
	if a.inArena(unsafe.Pointer(&v[0])) {
		return (*C.uint32_t)(unsafe.Pointer(&v[0]))
	}
	p := a.alloc(uintptr(len(v)) * 4)
	copy(unsafe.Slice((*uint32)(p), len(v)), v)
	return (*C.uint32_t)(p)
}

func (a *arena) cstring(s string) *C.char {
	p := a.alloc(uintptr(len(s)) + 1)
	b := unsafe.Slice((*byte)(p), len(s)+1)
	copy(b, s)
	b[len(s)] = 0
	return (*C.char)(p)
}

// reset keeps the blocks for the next call; free returns them to C.
func (a *arena) reset() { a.cur, a.off = 0, 0 }

func (a *arena) free() {
	for _, p := range a.blocks {
		C.free(p)
	}
	a.blocks, a.sizes = nil, nil
	a.reset()
}

// getArena / putArena: a small free list of arenas per engine (calls may run concurrently).
func (e *Engine) getArena() *arena {
	select {
	case a := <-e.arenas:
		a.reset()
		return a
	default:
		return &arena{}
	}
}

func (e *Engine) putArena(a *arena) {
	select {
	case e.arenas <- a:
	default:
		a.free()
	}
}

func (a *arena) blockID(b *BlockID) C.tmed_block_id {
	return C.tmed_block_id{hash: a.bytes(b.Hash), hash_len: C.uint32_t(len(b.Hash)), psh_total: C.uint32_t(b.PSHTotal),
		psh_hash: a.bytes(b.PSHHash), psh_hash_len: C.uint32_t(len(b.PSHHash))}
}

// LoadKeyset decodes a validator set's keys once and builds their comb tables in HBM.
func (e *Engine) LoadKeyset(pubKeys []byte) (uint64, error) {
	a := e.getArena()
	defer e.putArena(a)
	var h C.uint64_t
	if rc := C.tmed_keyset_load(e.ctx, a.bytes(pubKeys), C.size_t(len(pubKeys)/32), &h); rc != 0 {
		return 0, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	return uint64(h), nil
}

// FreeKeyset releases a key set.
func (e *Engine) FreeKeyset(h uint64) { C.tmed_keyset_free(e.ctx, C.uint64_t(h)) }

// ExtendKeyset appends keys to a key set; existing keys keep their indexes, the new ones start at
// the returned index (tmed_keyset_extend).
func (e *Engine) ExtendKeyset(h uint64, pubKeys []byte) (uint32, error) {
	a := e.getArena()
	defer e.putArena(a)
	var first C.uint32_t
	if rc := C.tmed_keyset_extend(e.ctx, C.uint64_t(h), a.bytes(pubKeys), C.size_t(len(pubKeys)/32), &first); rc != 0 {
		return 0, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	return uint32(first), nil
}

// KeyCacheConfig turns the engine's key-set cache on or off (enabled < 0: unchanged) and sets its
// HBM budget (0: unchanged).  It is on by default: sets passed without a handle reach the
// key-cached kernels from their second call on (tmed_keycache_config).
func (e *Engine) KeyCacheConfig(enabled int, budgetBytes uint64) error {
	if rc := C.tmed_keycache_config(e.ctx, C.int(enabled), C.size_t(budgetBytes)); rc != 0 {
		return errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	return nil
}

// KeyCacheStats returns the cache's counters (tmed_keycache_counters).
func (e *Engine) KeyCacheStats() (C.tmed_keycache_counters, error) {
	var st C.tmed_keycache_counters
	if rc := C.tmed_keycache_stats(e.ctx, &st); rc != 0 {
		return st, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	return st, nil
}

// WarmKeyCache builds a set's missing keys now — e.g. when EndBlock changes the validator set —
// so that even its first commit is keyed (tmed_keycache_warm).
func (e *Engine) WarmKeyCache(v *ValSet) error {
	a := e.getArena()
	defer e.putArena(a)
	cv := a.valset(v)
	if rc := C.tmed_keycache_warm(e.ctx, &cv); rc != 0 {
		return errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	return nil
}

// VerifyCommits verifies many commits with ONE device batch.
func (e *Engine) VerifyCommits(reqs []Request) ([]Result, error) {
	return e.verifyCommitsWith(reqs, func(a *arena, creqs *C.tmed_commit_request, n C.size_t,
		res *C.tmed_commit_result) C.int {
		return C.tmed_verify_commits(e.ctx, creqs, n, res)
	})
}

func (e *Engine) verifyCommitsWith(reqs []Request, call func(*arena, *C.tmed_commit_request, C.size_t,
	*C.tmed_commit_result) C.int) ([]Result, error) {
	a := e.getArena()
	defer e.putArena(a)
	return e.verifyIn(a, reqs, call)
}

func (e *Engine) verifyIn(a *arena, reqs []Request, call func(*arena, *C.tmed_commit_request, C.size_t,
	*C.tmed_commit_result) C.int) ([]Result, error) {
	n := len(reqs)
	if n == 0 {
		return nil, nil
	}
	creqs := (*[1 << 26]C.tmed_commit_request)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_commit_request{})))[:n:n]
	vs := (*[1 << 26]C.tmed_valset)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_valset{})))[:n:n]
	cs := (*[1 << 26]C.tmed_commit)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_commit{})))[:n:n]
	bids := (*[1 << 26]C.tmed_block_id)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_block_id{})))[:n:n]
	// one C copy per distinct *ValSet: requests on the same set share it (the library resolves each
	// set once per call; a light-client batch holds each set twice)
	seen := make(map[*ValSet]*C.tmed_valset, n)
	// one C copy per distinct *CommitData as well: the light client's Trusting + Light pair checks
	// one commit twice, and the library verifies a signature the two share once (same commit)
	seenC := make(map[*CommitData]*C.tmed_commit, n)
	for i := range reqs {
		r := &reqs[i]
		cv, ok := seen[r.Vals]
		if !ok {
			vs[i] = a.valset(r.Vals)
			cv = &vs[i]
			seen[r.Vals] = cv
		}
		c := r.Commit
		cc, ok := seenC[c]
		if !ok {
			cs[i] = a.commitC(c, nil)
			cc = &cs[i]
			seenC[c] = cc
		}
		bids[i] = C.tmed_block_id{}
		if r.BlockID != nil {
			bids[i] = a.blockID(r.BlockID)
		}
		cid := a.cstring(r.ChainID)
		creqs[i] = C.tmed_commit_request{mode: C.int(r.Mode), chain_id: cid, chain_id_len: C.uint32_t(len(r.ChainID)),
			vals: cv, block_id: &bids[i], height: C.int64_t(r.Height), commit: cc,
			trust_num: C.int64_t(r.TrustNum), trust_den: C.int64_t(r.TrustDen)}
	}
	res := make([]C.tmed_commit_result, n)
	if rc := call(a, &creqs[0], C.size_t(n), &res[0]); rc != 0 {
		return nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	return toResults(res), nil
}

// Batch is one VerifyCommits call whose commits and validator sets are flattened by the caller
// straight into C memory (NewCommit / NewValSet), so the shim copies nothing: package types fills
// them from its Commit / ValidatorSet (INTEGRATION.md §2).  Verify, then Release.
type Batch struct {
	e    *Engine
	a    *arena
	reqs []Request
}

func (e *Engine) NewBatch() *Batch { return &Batch{e: e, a: e.getArena()} }

// NewCommit: a commit of n signatures to fill in place.
func (b *Batch) NewCommit(n int) *CommitData { return newCommitIn(b.a, n, nil) }

// NewValSet: a validator set of n validators to fill in place (TotalPower / SetHash set by the caller).
func (b *Batch) NewValSet(n int) *ValSet { return newValSetIn(b.a, n) }

func (b *Batch) Add(r Request) { b.reqs = append(b.reqs, r) }

func (b *Batch) Verify() ([]Result, error) {
	return b.e.verifyIn(b.a, b.reqs, func(a *arena, creqs *C.tmed_commit_request, n C.size_t,
		res *C.tmed_commit_result) C.int {
		return C.tmed_verify_commits(b.e.ctx, creqs, n, res)
	})
}

// Release returns the batch's C memory to the engine (the CommitData / ValSet it made are invalid after).
func (b *Batch) Release() {
	if b.a != nil {
		b.e.putArena(b.a)
		b.a, b.reqs = nil, nil
	}
}

func toResults(res []C.tmed_commit_result) []Result {
	out := make([]Result, len(res))
	for i := range res {
		out[i] = Result{Code: int(res[i].code), Got: int64(res[i].got), Needed: int64(res[i].needed),
			Expected: int64(res[i].expected), Actual: int64(res[i].actual), Idx: int32(res[i].idx),
			IdxFirst: int32(res[i].idx_first), ValIdx: int32(res[i].val_idx)}
	}
	return out
}

// BlocksyncWindow is a run of buffered blocks checked against one (predicted) validator
// set: block h is vals.VerifyCommitLight(ChainID, BlockIDs[h], Heights[h], Commits[h])
// (blockchain/v0/reactor.go:366-367).
type BlocksyncWindow struct {
	ChainID  string
	Vals     *ValSet
	BlockIDs []BlockID
	Heights  []int64
	Commits  []*CommitData
	builder  *WindowBuilder // set by WindowBuilder.Window: the commits already live in its C memory
}

// BlocksyncVerify returns the VerifyCommitLight outcome of every block of the window,
// computed speculatively through the pipelined device path (tmed_blocksync_verify).
// The reactor applies blocks in order and stops at the first non-OK result.
func (e *Engine) BlocksyncVerify(w *BlocksyncWindow, batchBlocks int) ([]Result, error) {
	n := len(w.Commits)
	if n == 0 {
		return nil, nil
	}
	a := e.getArena()
	defer e.putArena(a)
	vs := (*C.tmed_valset)(a.alloc(unsafe.Sizeof(C.tmed_valset{})))
	*vs = a.valset(w.Vals)
	cs := (*[1 << 26]C.tmed_commit)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_commit{})))[:n:n]
	bids := (*[1 << 26]C.tmed_block_id)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_block_id{})))[:n:n]
	// signatures into the pinned arena (direct DMA, include/tmed25519.h tmed_host_alloc)
	total := 0
	for _, c := range w.Commits {
		total += len(c.Sigs)
	}
	e.pinMu.Lock()
	defer e.pinMu.Unlock()
	arenaBase := e.pinnedSigs(total)
	off := 0
	for i, c := range w.Commits {
		sigs := (*C.uint8_t)(nil)
		if !c.cmem && arenaBase != nil && len(c.Sigs) > 0 {
			p := unsafe.Add(arenaBase, off)
			copy(unsafe.Slice((*byte)(p), len(c.Sigs)), c.Sigs)
			sigs, off = (*C.uint8_t)(p), off+len(c.Sigs)
		}
		cs[i] = a.commitC(c, sigs)
		bids[i] = a.blockID(&w.BlockIDs[i])
	}
	cid := a.cstring(w.ChainID)
	win := (*C.tmed_blocksync_window)(a.alloc(unsafe.Sizeof(C.tmed_blocksync_window{})))
	*win = C.tmed_blocksync_window{chain_id: cid, chain_id_len: C.uint32_t(len(w.ChainID)), vals: vs,
		n_blocks: C.size_t(n), block_ids: &bids[0], heights: a.i64(w.Heights), commits: &cs[0]}
	res := make([]C.tmed_commit_result, n)
	if rc := C.tmed_blocksync_verify(e.ctx, win, C.uint32_t(batchBlocks), &res[0]); rc != 0 {
		return nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	return toResults(res), nil
}

// PendingWindow is a window queued by BlocksyncSubmit.  Its results are final once a LATER
// BlocksyncSubmit or BlocksyncWait on the same engine has returned; until then its C copies and
// its pinned signature buffer stay allocated (the library DMAs from them and writes the results
// into C memory: cgo forbids C retaining Go pointers after a call returns).
type PendingWindow struct {
	e   *Engine
	a   *arena
	pin unsafe.Pointer
	res *C.tmed_commit_result
	n   int
}

// BlocksyncSubmit queues a window behind the engine's windows in flight (tmed_blocksync_submit):
// the reactor's replay submits window w+1 before it applies window w, so the device is never
// drained between windows.  When it returns, every earlier submitted window's Results are final.
func (e *Engine) BlocksyncSubmit(w *BlocksyncWindow, batchBlocks int) (*PendingWindow, error) {
	n := len(w.Commits)
	if w.builder != nil { // built in place (NewWindow): its arena and pinned buffer travel with it
		return w.builder.submit(w, batchBlocks)
	}
	p := &PendingWindow{e: e, n: n, a: e.getArena()}
	if n == 0 {
		return p, nil
	}
	return p.submit(w, batchBlocks, true)
}

// submit marshals w into p's arena (signatures into p.pin when copyPin) and queues it.
func (p *PendingWindow) submit(w *BlocksyncWindow, batchBlocks int, copyPin bool) (*PendingWindow, error) {
	e, a, n := p.e, p.a, len(w.Commits)
	vs := (*C.tmed_valset)(a.alloc(unsafe.Sizeof(C.tmed_valset{})))
	*vs = a.valset(w.Vals)
	cs := (*[1 << 26]C.tmed_commit)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_commit{})))[:n:n]
	bids := (*[1 << 26]C.tmed_block_id)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_block_id{})))[:n:n]
	total := 0
	for _, c := range w.Commits {
		total += len(c.Sigs)
	}
	// a pinned buffer per window in flight (the engine's shared arena serves synchronous calls)
	if copyPin && total > 0 && C.tmed_host_alloc(C.size_t(total), &p.pin) != 0 {
		p.pin = nil
	}
	off := 0
	for i, c := range w.Commits {
		sigs := (*C.uint8_t)(nil)
		if copyPin && !c.cmem && p.pin != nil && len(c.Sigs) > 0 {
			q := unsafe.Add(p.pin, off)
			copy(unsafe.Slice((*byte)(q), len(c.Sigs)), c.Sigs)
			sigs, off = (*C.uint8_t)(q), off+len(c.Sigs)
		}
		cs[i] = a.commitC(c, sigs)
		bids[i] = a.blockID(&w.BlockIDs[i])
	}
	cid := a.cstring(w.ChainID)
	win := (*C.tmed_blocksync_window)(a.alloc(unsafe.Sizeof(C.tmed_blocksync_window{})))
	*win = C.tmed_blocksync_window{chain_id: cid, chain_id_len: C.uint32_t(len(w.ChainID)), vals: vs,
		n_blocks: C.size_t(n), block_ids: &bids[0], heights: a.i64(w.Heights), commits: &cs[0]}
	p.res = (*C.tmed_commit_result)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_commit_result{})))
	if rc := C.tmed_blocksync_submit(e.ctx, win, C.uint32_t(batchBlocks), p.res); rc != 0 {
		p.free()
		return nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	return p, nil
}

// BlocksyncWait collects every window submitted on the engine (tmed_blocksync_wait).
func (e *Engine) BlocksyncWait() error {
	if rc := C.tmed_blocksync_wait(e.ctx); rc != 0 {
		return errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	return nil
}

// Results returns the window's outcomes and releases its memory.  Call it only after a later
// BlocksyncSubmit or BlocksyncWait returned without error.  A nil window (the one a failed
// BlocksyncSubmit returns) has no results.
func (p *PendingWindow) Results() []Result {
	if p == nil {
		return nil
	}
	var out []Result
	if p.n > 0 {
		out = toResults(unsafe.Slice(p.res, p.n))
	}
	p.free() // an empty window still holds its arena (and a builder's pinned buffer)
	return out
}

func (p *PendingWindow) free() {
	if p.pin != nil {
		C.tmed_host_free(p.pin)
		p.pin = nil
	}
	if p.a != nil {
		p.e.putArena(p.a)
		p.a = nil
	}
	p.n = 0
}

// WindowBuilder lays a blocksync window out in C memory as the reactor flattens its blocks: each
// commit's arrays in the window's arena, its signatures in the window's pinned buffer (the library
// DMAs them from there), filled in place by package types (INTEGRATION.md §3: up to the
// VerifyCommitLight crossing).  Submit with BlocksyncSubmit(w.Window(...)).
type WindowBuilder struct {
	p   *PendingWindow
	off uintptr
	cap uintptr
}

// NewWindow: room for maxSigs signatures over the window's commits.
func (e *Engine) NewWindow(maxSigs int) *WindowBuilder {
	b := &WindowBuilder{p: &PendingWindow{e: e, a: e.getArena()}}
	if maxSigs > 0 && C.tmed_host_alloc(C.size_t(64*maxSigs), &b.p.pin) != 0 {
		b.p.pin = nil // no page-locked memory: the signatures go to the arena (the library stages them)
	}
	if b.p.pin != nil {
		b.cap = uintptr(64 * maxSigs)
	}
	return b
}

// NewCommit: a commit of n signatures, its Sigs in the pinned buffer when room is left.
func (b *WindowBuilder) NewCommit(n int) *CommitData {
	var sigs unsafe.Pointer
	if b.p.pin != nil && b.off+uintptr(64*n) <= b.cap {
		sigs = unsafe.Add(b.p.pin, b.off)
		b.off += uintptr(64 * n)
	}
	return newCommitIn(b.p.a, n, sigs)
}

// Window wraps the built commits for BlocksyncSubmit.
func (b *WindowBuilder) Window(chainID string, vals *ValSet, blockIDs []BlockID, heights []int64,
	commits []*CommitData) *BlocksyncWindow {
	return &BlocksyncWindow{ChainID: chainID, Vals: vals, BlockIDs: blockIDs, Heights: heights, Commits: commits,
		builder: b}
}

func (b *WindowBuilder) submit(w *BlocksyncWindow, batchBlocks int) (*PendingWindow, error) {
	p := b.p
	p.n = len(w.Commits)
	if p.n == 0 {
		return p, nil
	}
	return p.submit(w, batchBlocks, false)
}

// ValsetHashes returns ValidatorSet.Hash() of every set: set s is validators
// [setOff[s], setOff[s+1]) of (pubKeys n x 32, powers n) in set order (tmed_valset_hashes).
func (e *Engine) ValsetHashes(pubKeys []byte, powers []int64, setOff []uint32) ([][32]byte, error) {
	ns := len(setOff) - 1
	if ns <= 0 {
		return nil, nil
	}
	a := e.getArena()
	defer e.putArena(a)
	out := (*[1 << 26][32]byte)(a.alloc(uintptr(ns) * 32))[:ns:ns]
	if rc := C.tmed_valset_hashes(e.ctx, a.bytes(pubKeys), a.i64(powers), a.u32(setOff), C.size_t(ns),
		(*C.uint8_t)(unsafe.Pointer(&out[0]))); rc != 0 {
		return nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	return append([][32]byte(nil), out...), nil
}

// MerkleRoots returns merkle.HashFromByteSlices of every tree (tmed_merkle_roots).
func (e *Engine) MerkleRoots(trees [][][]byte) ([][32]byte, error) {
	nt := len(trees)
	if nt == 0 {
		return nil, nil
	}
	var flat []byte
	leafOff := []uint64{0}
	treeOff := []uint32{0}
	for _, t := range trees {
		for _, l := range t {
			flat = append(flat, l...)
			leafOff = append(leafOff, uint64(len(flat)))
		}
		treeOff = append(treeOff, uint32(len(leafOff)-1))
	}
	flat = append(flat, make([]byte, 8)...) // the device reader may touch the last dword
	a := e.getArena()
	defer e.putArena(a)
	lo := (*[1 << 26]C.uint64_t)(a.alloc(uintptr(len(leafOff)) * 8))[:len(leafOff):len(leafOff)]
	for i, v := range leafOff {
		lo[i] = C.uint64_t(v)
	}
	out := (*[1 << 26][32]byte)(a.alloc(uintptr(nt) * 32))[:nt:nt]
	if rc := C.tmed_merkle_roots(e.ctx, a.bytes(flat), &lo[0], a.u32(treeOff), C.size_t(nt),
		(*C.uint8_t)(unsafe.Pointer(&out[0]))); rc != 0 {
		return nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	return append([][32]byte(nil), out...), nil
}

// CommitHashes returns Commit.Hash() (types/block.go:894-912) of every commit
// (tmed_commit_hashes: the CommitSig protos are encoded and hashed on the device from the flat
// arrays).  ok[i] is false where those arrays cannot reproduce the hash (a signature longer than 64
// bytes, an address of another length than 0 or 20) or where the reference's Marshal fails and Hash
// panics (timestamp out of range): the caller runs commit.Hash() itself for those.
func (e *Engine) CommitHashes(commits []*CommitData) ([][32]byte, []bool, error) {
	n := len(commits)
	if n == 0 {
		return nil, nil, nil
	}
	a := e.getArena()
	defer e.putArena(a)
	cs := (*[1 << 26]C.tmed_commit)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_commit{})))[:n:n]
	for i, c := range commits {
		cs[i] = a.commitC(c, nil)
	}
	out := (*[1 << 26][32]byte)(a.alloc(uintptr(n) * 32))[:n:n]
	okc := (*[1 << 30]C.uint8_t)(a.alloc(uintptr(n)))[:n:n]
	if rc := C.tmed_commit_hashes(e.ctx, &cs[0], C.size_t(n), (*C.uint8_t)(unsafe.Pointer(&out[0])), &okc[0]); rc != 0 {
		return nil, nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	ok := make([]bool, n)
	for i := range ok {
		ok[i] = okc[i] != 0
	}
	return append([][32]byte(nil), out...), ok, nil
}

// TxsHashes returns Data.Hash() = Txs.Hash() (types/block.go:1004-1012 -> types/tx.go:47-55) of
// every block's transactions (tmed_txs_hashes: SHA-256 of each transaction and the tree over those
// digests both run on the device).
func (e *Engine) TxsHashes(blocks [][][]byte) ([][32]byte, error) {
	nb := len(blocks)
	if nb == 0 {
		return nil, nil
	}
	var flat []byte
	txOff := []uint64{0}
	blockOff := []uint32{0}
	for _, b := range blocks {
		for _, tx := range b {
			flat = append(flat, tx...)
			txOff = append(txOff, uint64(len(flat)))
		}
		blockOff = append(blockOff, uint32(len(txOff)-1))
	}
	flat = append(flat, make([]byte, 8)...) // the device reader may touch the last dword
	a := e.getArena()
	defer e.putArena(a)
	to := (*[1 << 26]C.uint64_t)(a.alloc(uintptr(len(txOff)) * 8))[:len(txOff):len(txOff)]
	for i, v := range txOff {
		to[i] = C.uint64_t(v)
	}
	out := (*[1 << 26][32]byte)(a.alloc(uintptr(nb) * 32))[:nb:nb]
	if rc := C.tmed_txs_hashes(e.ctx, a.bytes(flat), &to[0], a.u32(blockOff), C.size_t(nb),
		(*C.uint8_t)(unsafe.Pointer(&out[0]))); rc != 0 {
		return nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	return append([][32]byte(nil), out...), nil
}

// Proof mirrors merkle.Proof (crypto/merkle/proof.go:24-29).  LeafHash and every aunt are 32-byte
// slices of the buffers one proofs call returns: nothing is allocated per proof or per aunt.
type Proof struct {
	Total    int64
	Index    int64
	LeafHash []byte
	Aunts    [][]byte
}

// TreeProofs is merkle.ProofsFromByteSlices' result for one tree: its root and one proof per leaf.
type TreeProofs struct {
	Root   [32]byte
	Proofs []Proof
}

// Codes of VerifyProofs, in the order Proof.Verify checks (crypto/merkle/proof.go:52-68).
const (
	ProofOK            = C.TMED_PROOF_OK
	ProofNegativeTotal = C.TMED_PROOF_NEGATIVE_TOTAL
	ProofNegativeIndex = C.TMED_PROOF_NEGATIVE_INDEX
	ProofLeafHash      = C.TMED_PROOF_LEAF_HASH
	ProofRootHash      = C.TMED_PROOF_ROOT_HASH
)

func (a *arena) u64(v []uint64) *C.uint64_t {
	if len(v) == 0 {
		return nil
	}
	p := a.alloc(uintptr(len(v)) * 8)
	copy(unsafe.Slice((*uint64)(p), len(v)), v)
	return (*C.uint64_t)(p)
}

// flatten concatenates the byte slices of every group: the bytes (8 spare at the end: the device
// reader may touch the last dword), the slices' offsets and the groups' ranges of slice indices.
func flatten(groups [][][]byte) ([]byte, []uint64, []uint32) {
	var flat []byte
	itemOff := []uint64{0}
	groupOff := []uint32{0}
	for _, g := range groups {
		for _, x := range g {
			flat = append(flat, x...)
			itemOff = append(itemOff, uint64(len(flat)))
		}
		groupOff = append(groupOff, uint32(len(itemOff)-1))
	}
	return append(flat, make([]byte, 8)...), itemOff, groupOff
}

// runProofs drives one generator: the sizing call (aunts = NULL: the aunt offsets and the byte
// count, computed on the host), then the real call into Go buffers of exactly that size.  The
// buffers hold no Go pointers and are only used during the call (cgo pointer rules).
func runProofs(a *arena, nt, nl int, call func(roots, lh *C.uint8_t, ao *C.uint64_t, au *C.uint8_t, room C.size_t,
	need *C.size_t) C.int) ([][32]byte, []byte, []uint64, []byte, error) {
	ao := (*[1 << 26]C.uint64_t)(a.alloc(uintptr(nl+1) * 8))[: nl+1 : nl+1]
	var need C.size_t
	if rc := call(nil, nil, &ao[0], nil, 0, &need); rc != 0 {
		return nil, nil, nil, nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	roots := make([][32]byte, nt)
	leafHashes := make([]byte, 32*nl+32)
	aunts := make([]byte, int(need)+32)
	if rc := call((*C.uint8_t)(unsafe.Pointer(&roots[0])), (*C.uint8_t)(unsafe.Pointer(&leafHashes[0])), &ao[0],
		(*C.uint8_t)(unsafe.Pointer(&aunts[0])), need, &need); rc != 0 {
		return nil, nil, nil, nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	auntOff := make([]uint64, nl+1)
	for i := range auntOff {
		auntOff[i] = uint64(ao[i])
	}
	return roots, leafHashes[:32*nl], auntOff, aunts[:int(need)], nil
}

// treeProofs cuts a generator's flat outputs into per-tree proofs: tree t holds leaves
// [off[t], off[t+1]).  Three allocations for the whole call (the trees, the proofs, the aunt slice
// headers); every hash is a slice of leafHashes or aunts.
func treeProofs(roots [][32]byte, off []uint32, leafHashes []byte, auntOff []uint64, aunts []byte) []TreeProofs {
	out := make([]TreeProofs, len(roots))
	nl := int(off[len(roots)])
	all := make([]Proof, nl)
	hashes := make([][]byte, len(aunts)/32)
	for k := range hashes {
		hashes[k] = aunts[32*k : 32*k+32 : 32*k+32]
	}
	for t := range out {
		lo, hi := int(off[t]), int(off[t+1])
		out[t].Root = roots[t]
		out[t].Proofs = all[lo:hi:hi]
		for i := lo; i < hi; i++ {
			all[i] = Proof{Total: int64(hi - lo), Index: int64(i - lo), LeafHash: leafHashes[32*i : 32*i+32 : 32*i+32],
				Aunts: hashes[auntOff[i]:auntOff[i+1]:auntOff[i+1]]}
		}
	}
	return out
}

// MerkleProofs returns merkle.ProofsFromByteSlices (crypto/merkle/proof.go:35-48) of every tree
// (tmed_merkle_proofs): the root and, per leaf, the proof the reference builds.
func (e *Engine) MerkleProofs(trees [][][]byte) ([]TreeProofs, error) {
	nt := len(trees)
	if nt == 0 {
		return nil, nil
	}
	flat, leafOff, treeOff := flatten(trees)
	a := e.getArena()
	defer e.putArena(a)
	data, lo, to := a.bytes(flat), a.u64(leafOff), a.u32(treeOff)
	roots, lh, ao, au, err := runProofs(a, nt, len(leafOff)-1, func(r, h *C.uint8_t, o *C.uint64_t, u *C.uint8_t,
		room C.size_t, need *C.size_t) C.int {
		return C.tmed_merkle_proofs(e.ctx, data, lo, to, C.size_t(nt), r, h, o, u, room, need)
	})
	if err != nil {
		return nil, err
	}
	return treeProofs(roots, treeOff, lh, ao, au), nil
}

// TxsProofs returns, for every block, Data.Hash() and the merkle.Proof of every transaction as
// Txs.Proof builds it (types/tx.go:80-93; tmed_txs_proofs): the leaves are tx.Hash(), so
// Proofs[i].LeafHash is leafHash(tx.Hash()) and TxProof.Validate verifies tx.Hash() as the leaf.
func (e *Engine) TxsProofs(blocks [][][]byte) ([]TreeProofs, error) {
	nb := len(blocks)
	if nb == 0 {
		return nil, nil
	}
	flat, txOff, blockOff := flatten(blocks)
	a := e.getArena()
	defer e.putArena(a)
	data, to, bo := a.bytes(flat), a.u64(txOff), a.u32(blockOff)
	roots, lh, ao, au, err := runProofs(a, nb, len(txOff)-1, func(r, h *C.uint8_t, o *C.uint64_t, u *C.uint8_t,
		room C.size_t, need *C.size_t) C.int {
		return C.tmed_txs_proofs(e.ctx, data, to, bo, C.size_t(nb), r, h, o, u, room, need)
	})
	if err != nil {
		return nil, err
	}
	return treeProofs(roots, blockOff, lh, ao, au), nil
}

// PartSetProofs is the whole of NewPartSetFromData (types/part_set.go:166-194) for every block's
// bytes (tmed_partset_proofs): the PartSetHeader hash and the proof of every part.  Part p of
// block b is blocks[b][p*partSize : min(len, (p+1)*partSize)] and its proof is out[b].Proofs[p].
func (e *Engine) PartSetProofs(blocks [][]byte, partSize uint32) ([]TreeProofs, error) {
	nb := len(blocks)
	if nb == 0 {
		return nil, nil
	}
	if partSize == 0 {
		return nil, errors.New("tmedgpu: part size 0")
	}
	var flat []byte
	dataOff := []uint64{0}
	nl := 0
	for _, b := range blocks {
		flat = append(flat, b...)
		dataOff = append(dataOff, uint64(len(flat)))
		nl += (len(b) + int(partSize) - 1) / int(partSize)
	}
	flat = append(flat, make([]byte, 8)...) // the device reader may touch the last dword
	a := e.getArena()
	defer e.putArena(a)
	data, do := a.bytes(flat), a.u64(dataOff)
	po := (*[1 << 26]C.uint32_t)(a.alloc(uintptr(nb+1) * 4))[: nb+1 : nb+1]
	roots, lh, ao, au, err := runProofs(a, nb, nl, func(r, h *C.uint8_t, o *C.uint64_t, u *C.uint8_t,
		room C.size_t, need *C.size_t) C.int {
		return C.tmed_partset_proofs(e.ctx, data, do, C.size_t(nb), C.uint32_t(partSize), r, &po[0], h, o, u, room, need)
	})
	if err != nil {
		return nil, err
	}
	partOff := make([]uint32, nb+1)
	for i := range partOff {
		partOff[i] = uint32(po[i])
	}
	return treeProofs(roots, partOff, lh, ao, au), nil
}

// VerifyProofs runs Proof.Verify(roots[rootOf[i]], leaves[i]) for every proof
// (crypto/merkle/proof.go:52-68; tmed_merkle_proofs_verify) and returns one code per proof:
// ProofOK, or the first check that fails.  rootOf == nil: proof i belongs to roots[i].  On a
// non-zero code the caller runs proof.Verify itself for the error's text.  LeafHash and the aunts
// must be 32 bytes each, which Proof.ValidateBasic (proof.go:98-117) guarantees; its limit of 100
// aunts is not needed here (any count is accepted, and no path is longer than 63).
func (e *Engine) VerifyProofs(roots [][32]byte, rootOf []uint32, leaves [][]byte, proofs []Proof) ([]uint8, error) {
	n := len(proofs)
	if len(leaves) != n || (rootOf != nil && len(rootOf) != n) {
		return nil, errors.New("tmedgpu: one leaf and one root index per proof")
	}
	if n == 0 {
		return nil, nil
	}
	if len(roots) == 0 {
		return nil, errors.New("tmedgpu: no roots")
	}
	var flat []byte
	leafOff := []uint64{0}
	auntOff := []uint64{0}
	totals := make([]int64, n)
	indexes := make([]int64, n)
	na := 0
	for _, p := range proofs {
		na += len(p.Aunts)
	}
	lh := make([]byte, 0, 32*n)
	au := make([]byte, 0, 32*na+32)
	for i, p := range proofs {
		if len(p.LeafHash) != 32 {
			return nil, errors.New("tmedgpu: a leaf hash of another size than 32 (Proof.ValidateBasic)")
		}
		for _, h := range p.Aunts {
			if len(h) != 32 {
				return nil, errors.New("tmedgpu: an aunt of another size than 32 (Proof.ValidateBasic)")
			}
			au = append(au, h...)
		}
		flat = append(flat, leaves[i]...)
		leafOff = append(leafOff, uint64(len(flat)))
		auntOff = append(auntOff, uint64(len(au)/32))
		lh = append(lh, p.LeafHash...)
		totals[i], indexes[i] = p.Total, p.Index
	}
	flat = append(flat, make([]byte, 8)...) // the device reader may touch the last dword
	a := e.getArena()
	defer e.putArena(a)
	codes := (*[1 << 30]C.uint8_t)(a.alloc(uintptr(n)))[:n:n]
	if rc := C.tmed_merkle_proofs_verify(e.ctx, C.size_t(n), (*C.uint8_t)(unsafe.Pointer(&roots[0])),
		C.size_t(len(roots)), a.u32(rootOf), a.bytes(flat), a.u64(leafOff), a.bytes(lh), a.i64(totals), a.i64(indexes),
		a.u64(auntOff), a.bytes(au), &codes[0]); rc != 0 {
		return nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	out := make([]uint8, n)
	for i := range out {
		out[i] = uint8(codes[i])
	}
	return out, nil
}

// VoteSignBytes returns Commit.VoteSignBytes for n votes of one commit (tmed_vote_sign_bytes;
// types/block.go:807-810 -> types/vote.go:93-101): vote i has flag flags[i] and timestamp
// (tsSec[i], tsNanos[i]).  The seam builds these itself (on the device); this is for callers and
// tests that sign synthetic commits.
func (e *Engine) VoteSignBytes(chainID string, height int64, round int32, bid *BlockID, flags []byte,
	tsSec []int64, tsNanos []int32) ([][]byte, error) {
	n := len(flags)
	if len(tsSec) != n || len(tsNanos) != n {
		return nil, errors.New("tmedgpu: one flag and one timestamp per vote")
	}
	if n == 0 {
		return nil, nil
	}
	a := e.getArena()
	defer e.putArena(a)
	t := (*C.tmed_vote_template)(a.alloc(unsafe.Sizeof(C.tmed_vote_template{})))
	*t = C.tmed_vote_template{chain_id: a.cstring(chainID), chain_id_len: C.uint32_t(len(chainID)),
		height: C.int64_t(height), round: C.int32_t(round), block_hash: a.bytes(bid.Hash),
		block_hash_len: C.uint32_t(len(bid.Hash)), psh_total: C.uint32_t(bid.PSHTotal), psh_hash: a.bytes(bid.PSHHash),
		psh_hash_len: C.uint32_t(len(bid.PSHHash))}
	fl, sec, ns := a.bytes(flags), a.i64(tsSec), a.i32(tsNanos)
	off := (*[1 << 26]C.uint32_t)(a.alloc(uintptr(n+1) * 4))[: n+1 : n+1]
	var total C.size_t
	if rc := C.tmed_vote_sign_bytes(t, C.size_t(n), fl, sec, ns, nil, 0, &off[0], &total); rc != 0 {
		return nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	buf := (*C.uint8_t)(a.alloc(uintptr(total) + 1))
	if rc := C.tmed_vote_sign_bytes(t, C.size_t(n), fl, sec, ns, buf, total, &off[0], &total); rc != 0 {
		return nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	flat := unsafe.Slice((*byte)(unsafe.Pointer(buf)), int(total))
	out := make([][]byte, n)
	for i := range out {
		out[i] = append([]byte(nil), flat[off[i]:off[i+1]]...)
	}
	return out, nil
}

// batchArgs packs n (pubkey, message, signature) tuples for tmed_verify_batch(_zip215):
// pubKeys n x 32, sigs as given (the lengths travel so a wrong-length signature is rejected
// exactly as ed25519.Verify rejects it), messages concatenated with offsets.
func batchArgs(a *arena, pubKeys []byte, msgs, sigs [][]byte) (pk, sg *C.uint8_t, sl *C.uint32_t,
	mg *C.uint8_t, mo *C.uint32_t) {
	n := len(msgs)
	sigBuf := make([]byte, 64*n)
	lens := make([]uint32, n)
	off := make([]uint32, n+1)
	var flat []byte
	for i := 0; i < n; i++ {
		copy(sigBuf[64*i:64*i+64], sigs[i])
		lens[i] = uint32(len(sigs[i]))
		flat = append(flat, msgs[i]...)
		off[i+1] = uint32(len(flat))
	}
	flat = append(flat, make([]byte, 16)...) // the device reader may touch past the last message
	return a.bytes(pubKeys), a.bytes(sigBuf), a.u32(lens), a.bytes(flat), a.u32(off)
}

// VerifyBatch returns ed25519.Verify (Go 1.18 rule, crypto/ed25519/ed25519.go:148-155) of every
// tuple (tmed_verify_batch).
func (e *Engine) VerifyBatch(pubKeys []byte, msgs, sigs [][]byte) ([]bool, error) {
	return e.batch(pubKeys, msgs, sigs, false)
}

// VerifyBatchZIP215 returns the ZIP-215 decision of every tuple (tmed_verify_batch_zip215):
// OPT-IN, for chains that adopt the rule of spec/core/encoding.md:52-54.
func (e *Engine) VerifyBatchZIP215(pubKeys []byte, msgs, sigs [][]byte) ([]bool, error) {
	return e.batch(pubKeys, msgs, sigs, true)
}

func (e *Engine) batch(pubKeys []byte, msgs, sigs [][]byte, zip215 bool) ([]bool, error) {
	n := len(msgs)
	if len(sigs) != n || len(pubKeys) != 32*n {
		return nil, errors.New("tmedgpu: want one 32-byte key and one signature per message")
	}
	if n == 0 {
		return nil, nil
	}
	a := e.getArena()
	defer e.putArena(a)
	pk, sg, sl, mg, mo := batchArgs(a, pubKeys, msgs, sigs)
	out := (*[1 << 28]C.uint8_t)(a.alloc(uintptr(n)))[:n:n]
	var rc C.int
	if zip215 {
		rc = C.tmed_verify_batch_zip215(e.ctx, pk, sg, sl, mg, mo, C.size_t(n), &out[0])
	} else {
		rc = C.tmed_verify_batch(e.ctx, pk, sg, sl, mg, mo, C.size_t(n), &out[0])
	}
	if rc != 0 {
		return nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	ok := make([]bool, n)
	for i := range ok {
		ok[i] = out[i] != 0
	}
	return ok, nil
}

// The signature rules of an engine's seam calls (tmed_set_rule).
const (
	RuleGo     = 0 // Go 1.18 crypto/ed25519.Verify: the default
	RuleZIP215 = 1 // ZIP-215: permissive decoding of A and R, [8]([S]B - R - [k]A) = O
)

// SetRule sets the signature rule of the engine's seam calls: VerifyCommits, the Blocksync calls,
// LightVerify, VerifyVotes (tmed_set_rule).  A chain on a release that verifies with ZIP-215 calls
// it once after creating the engine.  Only the signature decision changes; the loops, prechecks
// and error values stay v0.34.24's.  VerifyBatch keeps the Go rule whatever is set here.
func (e *Engine) SetRule(rule int) error {
	if rc := C.tmed_set_rule(e.ctx, C.int(rule)); rc != 0 {
		return errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	return nil
}

// Rule returns the engine's signature rule (tmed_rule).
func (e *Engine) Rule() int { return int(C.tmed_rule(e.ctx)) }

// VerifyBatchKeysetZIP215 returns the ZIP-215 decision of every (key index, message, signature)
// tuple against a loaded key set (tmed_verify_batch_keyset_zip215): exact per signature, no random
// weights.  A shim for a release whose VerifyCommit loops differ from 0.34's replays its own loop
// over these bits.
func (e *Engine) VerifyBatchKeysetZIP215(h uint64, valIdx []uint32, msgs, sigs [][]byte) ([]bool, error) {
	n := len(msgs)
	if len(sigs) != n || len(valIdx) != n {
		return nil, errors.New("tmedgpu: want one key index and one signature per message")
	}
	if n == 0 {
		return nil, nil
	}
	a := e.getArena()
	defer e.putArena(a)
	_, sg, sl, mg, mo := batchArgs(a, nil, msgs, sigs)
	out := (*[1 << 28]C.uint8_t)(a.alloc(uintptr(n)))[:n:n]
	rc := C.tmed_verify_batch_keyset_zip215(e.ctx, C.uint64_t(h), a.u32(valIdx), sg, sl, mg, mo, C.size_t(n), &out[0])
	if rc != 0 {
		return nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	ok := make([]bool, n)
	for i := range ok {
		ok[i] = out[i] != 0
	}
	return ok, nil
}

// Pool is one engine per GPU of the node, used from ONE process (a Tendermint node):
// tmed_verify_commits_multi / tmed_blocksync_verify_multi shard the work over the contexts
// concurrently; no collective is needed since host memory is shared.
type Pool struct{ engines []*Engine }

// NewPool opens devices 0..n-1.
func NewPool(n int) (*Pool, error) {
	p := &Pool{}
	for d := 0; d < n; d++ {
		var ctx *C.tmed_ctx
		if rc := C.tmed_init(C.int(d), &ctx); rc != 0 {
			for _, e := range p.engines {
				C.tmed_destroy(e.ctx)
			}
			return nil, errors.New(C.GoString(C.tmed_strerror(rc)))
		}
		p.engines = append(p.engines, newEngine(ctx))
	}
	return p, nil
}

func (p *Pool) ctxs(a *arena) **C.tmed_ctx {
	arr := (*[1 << 10]*C.tmed_ctx)(a.alloc(uintptr(len(p.engines)) * unsafe.Sizeof((*C.tmed_ctx)(nil))))[:len(p.engines):len(p.engines)]
	for i, e := range p.engines {
		arr[i] = e.ctx
	}
	return &arr[0]
}

// LoadKeyset loads the same key set on every GPU; the handles agree when every pool
// member loads the same sets in the same order (the pool is the only loader).
func (p *Pool) LoadKeyset(pubKeys []byte) (uint64, error) {
	var h uint64
	for i, e := range p.engines {
		hi, err := e.LoadKeyset(pubKeys)
		if err != nil {
			return 0, err
		}
		if i > 0 && hi != h {
			return 0, errors.New("tmedgpu: key-set handles diverged across GPUs")
		}
		h = hi
	}
	return h, nil
}

// VerifyCommits is Engine.VerifyCommits sharded over the pool's GPUs.
func (p *Pool) VerifyCommits(reqs []Request) ([]Result, error) {
	if len(reqs) == 0 {
		return nil, nil
	}
	// the request structs are built exactly as Engine.VerifyCommits does
	return p.engines[0].verifyCommitsWith(reqs, func(a *arena, creqs *C.tmed_commit_request, n C.size_t,
		res *C.tmed_commit_result) C.int {
		return C.tmed_verify_commits_multi(p.ctxs(a), C.size_t(len(p.engines)), creqs, n, res)
	})
}

// ---- light.Verify (light/verifier.go:135-151) ----------------------------------------------------

// Outcome codes of LightVerify, numbered in the order the reference checks (see tmed25519.h, which
// cites each check's lines); the first failing check wins.
const (
	LightOK               = C.TMED_LIGHT_OK
	LightOldHeaderExpired = C.TMED_LIGHT_OLD_HEADER_EXPIRED
	LightHeaderBasic      = C.TMED_LIGHT_HEADER_BASIC
	LightWrongChain       = C.TMED_LIGHT_WRONG_CHAIN
	LightCommitHeight     = C.TMED_LIGHT_COMMIT_HEIGHT
	LightCommitHeaderHash = C.TMED_LIGHT_COMMIT_HEADER_HASH
	LightHeightNotGreater = C.TMED_LIGHT_HEIGHT_NOT_GREATER
	LightTimeNotAfter     = C.TMED_LIGHT_TIME_NOT_AFTER
	LightTimeFromFuture   = C.TMED_LIGHT_TIME_FROM_FUTURE
	LightValsHash         = C.TMED_LIGHT_VALS_HASH
	LightNextValsHash     = C.TMED_LIGHT_NEXT_VALS_HASH
	LightTrusting         = C.TMED_LIGHT_TRUSTING
	LightCommit           = C.TMED_LIGHT_COMMIT
	LightGoPath           = C.TMED_LIGHT_GO_PATH
	// LightOrdered (flags): VerifyCommitLight runs in a second batch, only after a passed
	// VerifyCommitLightTrusting (the reference's note at verifier.go:70-72).
	LightOrdered uint32 = C.TMED_LIGHT_ORDERED
)

// HeaderData is a flat copy of the fields of types.Header that Header.Hash reads
// (types/block.go:440-475), in struct order.
type HeaderData struct {
	VersionBlock, VersionApp uint64
	ChainID                  string
	Height                   int64
	TimeSeconds              int64 // Time.Unix()
	TimeNanos                int32 // Time.Nanosecond()
	LastBlockID              BlockID
	// LastCommitHash, DataHash, ValidatorsHash, NextValidatorsHash, ConsensusHash, AppHash,
	// LastResultsHash, EvidenceHash, ProposerAddress
	Hashes [9][]byte
}

// LightRequest holds the arguments of one light.Verify call.
type LightRequest struct {
	// trustedHeader: the fields light.Verify reads
	ChainID             string
	TrustedHeight       int64
	TrustedTimeSeconds  int64
	TrustedTimeNanos    int32
	TrustedNextValsHash []byte
	TrustedVals         *ValSet // non-adjacent only
	// untrusted SignedHeader + set
	Header  *HeaderData
	Commit  *CommitData
	Vals    *ValSet
	BasicOK bool // Header.ValidateBasic() == nil && Commit.ValidateBasic() == nil
	// trustingPeriod, maxClockDrift (time.Duration), now, trustLevel
	TrustingPeriodNs, MaxClockDriftNs int64
	NowSeconds                        int64
	NowNanos                          int32
	TrustNum, TrustDen                int64
}

// LightResult is one request's outcome; the caller builds the reference's error value from it
// (INTEGRATION.md §2c).
type LightResult struct {
	Code           int
	Adjacent       bool
	ExpiredSeconds int64 // LightOldHeaderExpired: trustedHeader.Time.Add(trustingPeriod)
	ExpiredNanos   int32
	Hash           []byte // LightCommitHeaderHash: Header.Hash() (nil as in Go); LightValsHash: untrustedVals.Hash()
	Commit         Result // LightTrusting / LightCommit: the failing VerifyCommitLight* outcome
	VerifiedTrusting, VerifiedLight uint32
}

func (a *arena) headerC(h *HeaderData) C.tmed_header {
	t := C.tmed_header{version_block: C.uint64_t(h.VersionBlock), version_app: C.uint64_t(h.VersionApp),
		chain_id: a.cstring(h.ChainID), chain_id_len: C.uint32_t(len(h.ChainID)), height: C.int64_t(h.Height),
		time_seconds: C.int64_t(h.TimeSeconds), time_nanos: C.int32_t(h.TimeNanos),
		last_block_id: a.blockID(&h.LastBlockID)}
	for k := range h.Hashes {
		t.hashes[k] = a.bytes(h.Hashes[k])
		t.hash_lens[k] = C.uint32_t(len(h.Hashes[k]))
	}
	return t
}

// LightVerify is light.Verify for many (trusted, untrusted) pairs in one call: the header hashes,
// the set hashes and the signatures of both commit checks are computed on the device, then the
// reference's checks are replayed in its order.  An error means "take the original Go path".
func (e *Engine) LightVerify(reqs []LightRequest, flags uint32) ([]LightResult, error) {
	n := len(reqs)
	if n == 0 {
		return nil, nil
	}
	a := e.getArena()
	defer e.putArena(a)
	creqs := (*[1 << 24]C.tmed_light_request)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_light_request{})))[:n:n]
	hs := (*[1 << 24]C.tmed_header)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_header{})))[:n:n]
	cs := (*[1 << 24]C.tmed_commit)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_commit{})))[:n:n]
	vs := (*[1 << 24]C.tmed_valset)(a.alloc(uintptr(2*n) * unsafe.Sizeof(C.tmed_valset{})))[: 2*n : 2*n]
	// one C copy per distinct *ValSet (the library hashes and resolves each set once per call) and
	// per distinct *CommitData
	seen := make(map[*ValSet]*C.tmed_valset, 2*n)
	seenC := make(map[*CommitData]*C.tmed_commit, n)
	nv := 0
	valset := func(v *ValSet) *C.tmed_valset {
		if v == nil {
			return nil
		}
		cv, ok := seen[v]
		if !ok {
			vs[nv] = a.valset(v)
			cv = &vs[nv]
			seen[v] = cv
			nv++
		}
		return cv
	}
	for i := range reqs {
		r := &reqs[i]
		if r.Header == nil || r.Commit == nil || r.Vals == nil {
			return nil, errors.New("tmedgpu: LightVerify: nil header, commit or validator set")
		}
		hs[i] = a.headerC(r.Header)
		cc, ok := seenC[r.Commit]
		if !ok {
			cs[i] = a.commitC(r.Commit, nil)
			cc = &cs[i]
			seenC[r.Commit] = cc
		}
		var basic C.uint8_t
		if r.BasicOK {
			basic = 1
		}
		creqs[i] = C.tmed_light_request{chain_id: a.cstring(r.ChainID), chain_id_len: C.uint32_t(len(r.ChainID)),
			trusted_height: C.int64_t(r.TrustedHeight), trusted_time_seconds: C.int64_t(r.TrustedTimeSeconds),
			trusted_time_nanos: C.int32_t(r.TrustedTimeNanos), trusted_next_vals_hash: a.bytes(r.TrustedNextValsHash),
			trusted_next_vals_hash_len: C.uint32_t(len(r.TrustedNextValsHash)), trusted_vals: valset(r.TrustedVals),
			header: &hs[i], commit: cc, vals: valset(r.Vals), basic_ok: basic,
			trusting_period_ns: C.int64_t(r.TrustingPeriodNs), max_clock_drift_ns: C.int64_t(r.MaxClockDriftNs),
			now_seconds: C.int64_t(r.NowSeconds), now_nanos: C.int32_t(r.NowNanos),
			trust_num: C.int64_t(r.TrustNum), trust_den: C.int64_t(r.TrustDen)}
	}
	res := make([]C.tmed_light_result, n)
	if rc := C.tmed_light_verify(e.ctx, &creqs[0], C.size_t(n), C.uint32_t(flags), &res[0]); rc != 0 {
		return nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	out := make([]LightResult, n)
	for i := range res {
		o := LightResult{Code: int(res[i].code), Adjacent: res[i].adjacent != 0,
			ExpiredSeconds: int64(res[i].expired_seconds), ExpiredNanos: int32(res[i].expired_nanos),
			VerifiedTrusting: uint32(res[i].verified_trusting), VerifiedLight: uint32(res[i].verified_light)}
		o.Commit = toResults([]C.tmed_commit_result{res[i].commit})[0]
		if hl := int(res[i].hash_len); hl > 0 {
			o.Hash = make([]byte, hl)
			for k := 0; k < hl; k++ {
				o.Hash[k] = byte(res[i].hash[k])
			}
		}
		out[i] = o
	}
	return out, nil
}

// ---- state.MedianTime (state/state.go:268-285) ----------------------------------------------------

// Outcome codes of MedianTimes (see tmed25519.h, which cites the reference lines of each rule).
const (
	MedianOK = C.TMED_MEDIAN_OK
	// MedianZeroTime: no signature entered; the reference returns time.Time{}.
	MedianZeroTime = C.TMED_MEDIAN_ZERO_TIME
	// MedianGoPath: Go's int64 arithmetic would decide (a timestamp whose UnixNano is no int64, a
	// negative power, a total past int64): the caller runs state.MedianTime itself.
	MedianGoPath = C.TMED_MEDIAN_GO_PATH
)

// MedianRequest holds the arguments of one MedianTime call: block.LastCommit and
// state.LastValidators, as the flat copies the commit verification of the same block uses.
type MedianRequest struct {
	Commit *CommitData
	Vals   *ValSet
}

// MedianResult is one pair's outcome: with MedianOK the median is time.Unix(Seconds, Nanos).
type MedianResult struct {
	Code     int
	Seconds  int64
	Nanos    int32
	Entered  uint32 // signatures that entered the median
	OnDevice bool   // computed by the kernels (an aligned commit), not by the library's host route
}

// MedianTimes is state.MedianTime for many (commit, validator set) pairs in one call
// (tmed_median_times): each distinct *CommitData and *ValSet is marshalled and staged once.  An
// error means "take the original Go path".
func (e *Engine) MedianTimes(reqs []MedianRequest) ([]MedianResult, error) {
	n := len(reqs)
	if n == 0 {
		return nil, nil
	}
	a := e.getArena()
	defer e.putArena(a)
	creqs := (*[1 << 24]C.tmed_median_request)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_median_request{})))[:n:n]
	cs := (*[1 << 24]C.tmed_commit)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_commit{})))[:n:n]
	vs := (*[1 << 24]C.tmed_valset)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_valset{})))[:n:n]
	seenV := make(map[*ValSet]*C.tmed_valset, n)
	seenC := make(map[*CommitData]*C.tmed_commit, n)
	for i := range reqs {
		r := &reqs[i]
		if r.Commit == nil || r.Vals == nil {
			return nil, errors.New("tmedgpu: MedianTimes: nil commit or validator set")
		}
		cc, ok := seenC[r.Commit]
		if !ok {
			cs[i] = a.commitC(r.Commit, nil)
			cc = &cs[i]
			seenC[r.Commit] = cc
		}
		cv, ok := seenV[r.Vals]
		if !ok {
			vs[i] = a.valset(r.Vals)
			cv = &vs[i]
			seenV[r.Vals] = cv
		}
		creqs[i] = C.tmed_median_request{commit: cc, vals: cv}
	}
	res := make([]C.tmed_median_result, n)
	if rc := C.tmed_median_times(e.ctx, &creqs[0], C.size_t(n), &res[0]); rc != 0 {
		return nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	out := make([]MedianResult, n)
	for i := range res {
		out[i] = MedianResult{Code: int(res[i].code), Seconds: int64(res[i].seconds), Nanos: int32(res[i].nanos),
			Entered: uint32(res[i].entered), OnDevice: res[i].on_device != 0}
	}
	return out, nil
}

// ---- Vote.Verify and the checks of VoteSet.addVote (types/vote.go:147-156, vote_set.go:156-218) ----

// Outcome codes of VerifyVotes: the first check that fails, in the reference's order (see
// tmed25519.h, which cites the reference line of each).
const (
	VoteOK = C.TMED_VOTE_OK
	// VoteIndexNegative / VoteIndexNotInSet: addVote wraps ErrVoteInvalidValidatorIndex.
	VoteIndexNegative = C.TMED_VOTE_INDEX_NEGATIVE
	// VoteAddressEmpty / VoteAddressNotInSet / VoteAddressNotOfKey: ErrVoteInvalidValidatorAddress.
	VoteAddressEmpty = C.TMED_VOTE_ADDRESS_EMPTY
	// VoteUnexpectedStep: ErrVoteUnexpectedStep.
	VoteUnexpectedStep  = C.TMED_VOTE_UNEXPECTED_STEP
	VoteIndexNotInSet   = C.TMED_VOTE_INDEX_NOT_IN_SET
	VoteAddressNotInSet = C.TMED_VOTE_ADDRESS_NOT_IN_SET
	VoteAddressNotOfKey = C.TMED_VOTE_ADDRESS_NOT_OF_KEY
	// VotePanic: VoteSignBytes panics (a malformed BlockID hash); the caller runs the original Go
	// path, which panics as before.
	VotePanic = C.TMED_VOTE_PANIC
	// VoteInvalidSignature: ErrVoteInvalidSignature.
	VoteInvalidSignature = C.TMED_VOTE_INVALID_SIGNATURE
	// VoteGoPath: the flat fields do not determine the reference's outcome (a timestamp outside the
	// proto Timestamp range): the caller runs the original Go path for this vote.
	VoteGoPath = C.TMED_VOTE_GO_PATH
)

// VoteData is a flat copy of n free-standing types.Vote values (filled by the caller in package
// types).  Hashes and addresses sit in fixed slots; the *Lens arrays give the real lengths.
type VoteData struct {
	Types            []int32
	Heights          []int64
	Rounds           []int32
	BlockHashes      []byte   // n x 32
	BlockHashLens    []uint32 // len(BlockID.Hash)
	PSHTotals        []uint32
	PSHHashes        []byte   // n x 32
	PSHHashLens      []uint32
	TsSeconds        []int64
	TsNanos          []int32
	Addresses        []byte   // n x 20
	AddrLens         []uint32 // len(ValidatorAddress)
	ValidatorIndexes []int32
	Sigs             []byte   // n x 64 (zero padded)
	SigLens          []uint32
	cmem             bool // every array already lives in C memory (Batch.NewVotes)
}

// NewVoteData: a VoteData of n votes in Go memory (copied into the call's arena once).
func NewVoteData(n int) *VoteData {
	return &VoteData{Types: make([]int32, n), Heights: make([]int64, n), Rounds: make([]int32, n),
		BlockHashes: make([]byte, 32*n), BlockHashLens: make([]uint32, n), PSHTotals: make([]uint32, n),
		PSHHashes: make([]byte, 32*n), PSHHashLens: make([]uint32, n), TsSeconds: make([]int64, n),
		TsNanos: make([]int32, n), Addresses: make([]byte, 20*n), AddrLens: make([]uint32, n),
		ValidatorIndexes: make([]int32, n), Sigs: make([]byte, 64*n), SigLens: make([]uint32, n)}
}

// NewVotes: a VoteData of n votes whose arrays are allocated in the batch's C memory, for the caller
// to fill in place (as Batch.NewCommit).
func (b *Batch) NewVotes(n int) *VoteData {
	a := b.a
	v := &VoteData{cmem: true}
	v.Types = unsafe.Slice((*int32)(a.alloc(uintptr(4*n))), n)
	v.Heights = unsafe.Slice((*int64)(a.alloc(uintptr(8*n))), n)
	v.Rounds = unsafe.Slice((*int32)(a.alloc(uintptr(4*n))), n)
	v.BlockHashes = unsafe.Slice((*byte)(a.alloc(uintptr(32*n))), 32*n)
	v.BlockHashLens = unsafe.Slice((*uint32)(a.alloc(uintptr(4*n))), n)
	v.PSHTotals = unsafe.Slice((*uint32)(a.alloc(uintptr(4*n))), n)
	v.PSHHashes = unsafe.Slice((*byte)(a.alloc(uintptr(32*n))), 32*n)
	v.PSHHashLens = unsafe.Slice((*uint32)(a.alloc(uintptr(4*n))), n)
	v.TsSeconds = unsafe.Slice((*int64)(a.alloc(uintptr(8*n))), n)
	v.TsNanos = unsafe.Slice((*int32)(a.alloc(uintptr(4*n))), n)
	v.Addresses = unsafe.Slice((*byte)(a.alloc(uintptr(20*n))), 20*n)
	v.AddrLens = unsafe.Slice((*uint32)(a.alloc(uintptr(4*n))), n)
	v.ValidatorIndexes = unsafe.Slice((*int32)(a.alloc(uintptr(4*n))), n)
	v.Sigs = unsafe.Slice((*byte)(a.alloc(uintptr(64*n))), 64*n)
	v.SigLens = unsafe.Slice((*uint32)(a.alloc(uintptr(4*n))), n)
	return v
}

// votesC: the C struct of v (its arrays passed as they are when they live in C memory, else copied
// into the arena once).
func (a *arena) votesC(v *VoteData) C.tmed_votes {
	n := len(v.Types)
	t := C.tmed_votes{n: C.size_t(n)}
	if n == 0 {
		return t
	}
	if v.cmem {
		t.types = (*C.int32_t)(unsafe.Pointer(&v.Types[0]))
		t.heights = (*C.int64_t)(unsafe.Pointer(&v.Heights[0]))
		t.rounds = (*C.int32_t)(unsafe.Pointer(&v.Rounds[0]))
		t.block_hashes, t.psh_hashes = ptr8(v.BlockHashes), ptr8(v.PSHHashes)
		t.block_hash_lens = (*C.uint32_t)(unsafe.Pointer(&v.BlockHashLens[0]))
		t.psh_totals = (*C.uint32_t)(unsafe.Pointer(&v.PSHTotals[0]))
		t.psh_hash_lens = (*C.uint32_t)(unsafe.Pointer(&v.PSHHashLens[0]))
		t.ts_seconds = (*C.int64_t)(unsafe.Pointer(&v.TsSeconds[0]))
		t.ts_nanos = (*C.int32_t)(unsafe.Pointer(&v.TsNanos[0]))
		t.addresses, t.sigs = ptr8(v.Addresses), ptr8(v.Sigs)
		t.address_lens = (*C.uint32_t)(unsafe.Pointer(&v.AddrLens[0]))
		t.validator_indexes = (*C.int32_t)(unsafe.Pointer(&v.ValidatorIndexes[0]))
		t.sig_lens = (*C.uint32_t)(unsafe.Pointer(&v.SigLens[0]))
		return t
	}
	t.types, t.heights, t.rounds = a.i32(v.Types), a.i64(v.Heights), a.i32(v.Rounds)
	t.block_hashes, t.block_hash_lens = a.bytes(v.BlockHashes), a.u32(v.BlockHashLens)
	t.psh_totals, t.psh_hashes, t.psh_hash_lens = a.u32(v.PSHTotals), a.bytes(v.PSHHashes), a.u32(v.PSHHashLens)
	t.ts_seconds, t.ts_nanos = a.i64(v.TsSeconds), a.i32(v.TsNanos)
	t.addresses, t.address_lens = a.bytes(v.Addresses), a.u32(v.AddrLens)
	t.validator_indexes = a.i32(v.ValidatorIndexes)
	t.sigs, t.sig_lens = a.bytes(v.Sigs), a.u32(v.SigLens)
	return t
}

// VoteRequest is one batch of votes against a validator set.  AddVote: the checks of
// VoteSet.addVote against the VoteSet's step (Height, Round, Type) in front of Vote.Verify; else
// Vote.Verify alone, with the key at each vote's ValidatorIndex.
type VoteRequest struct {
	ChainID string
	Vals    *ValSet
	Votes   *VoteData
	AddVote bool
	Height  int64
	Round   int32
	Type    int32
}

// VerifyVotes decides every vote of every request in ONE device batch (tmed_verify_votes) and
// returns the Vote* outcome codes, one slice per request.  VoteSet's own state (duplicates,
// conflicting votes, maj23) stays with the caller.  An error means "take the original Go path".
func (e *Engine) VerifyVotes(reqs []VoteRequest) ([][]uint8, error) {
	n := len(reqs)
	if n == 0 {
		return nil, nil
	}
	a := e.getArena()
	defer e.putArena(a)
	creqs := (*[1 << 24]C.tmed_vote_request)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_vote_request{})))[:n:n]
	cv := (*[1 << 24]C.tmed_votes)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_votes{})))[:n:n]
	vs := (*[1 << 24]C.tmed_valset)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_valset{})))[:n:n]
	seenV := make(map[*ValSet]*C.tmed_valset, n)
	total := 0
	for i := range reqs {
		r := &reqs[i]
		if r.Vals == nil || r.Votes == nil {
			return nil, errors.New("tmedgpu: VerifyVotes: nil votes or validator set")
		}
		set, ok := seenV[r.Vals]
		if !ok {
			vs[i] = a.valset(r.Vals)
			set = &vs[i]
			seenV[r.Vals] = set
		}
		cv[i] = a.votesC(r.Votes)
		var flags C.uint32_t
		if r.AddVote {
			flags = C.TMED_VOTES_ADDVOTE
		}
		creqs[i] = C.tmed_vote_request{chain_id: a.cstring(r.ChainID), chain_id_len: C.uint32_t(len(r.ChainID)),
			vals: set, votes: &cv[i], flags: flags, height: C.int64_t(r.Height), round: C.int32_t(r.Round),
			msg_type: C.int32_t(r.Type)}
		total += len(r.Votes.Types)
	}
	codes := make([]uint8, total+1)
	if rc := C.tmed_verify_votes(e.ctx, &creqs[0], C.size_t(n), (*C.uint8_t)(unsafe.Pointer(&codes[0]))); rc != 0 {
		return nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	out := make([][]uint8, n)
	at := 0
	for i := range reqs {
		m := len(reqs[i].Votes.Types)
		out[i] = codes[at : at+m : at+m]
		at += m
	}
	return out, nil
}

// ---- evidence: VerifyDuplicateVote (evidence/verify.go:162-222), DuplicateVoteEvidence.Hash and
// EvidenceList.Hash (types/evidence.go:90-103, :431-442) ----

// Outcome codes of VerifyDuplicateVotes: the first check that fails, in the reference's order (see
// tmed25519.h, which cites the reference line and error string of each).
const (
	DupVoteOK              = C.TMED_DUPVOTE_OK
	DupVoteNotAValidator   = C.TMED_DUPVOTE_NOT_A_VALIDATOR
	DupVoteHRSMismatch     = C.TMED_DUPVOTE_HRS_MISMATCH
	DupVoteAddressMismatch = C.TMED_DUPVOTE_ADDRESS_MISMATCH
	DupVoteSameBlockID     = C.TMED_DUPVOTE_SAME_BLOCK_ID
	DupVoteAddressNotOfKey = C.TMED_DUPVOTE_ADDRESS_NOT_OF_KEY
	DupVoteValidatorPower  = C.TMED_DUPVOTE_VALIDATOR_POWER
	DupVoteTotalPower      = C.TMED_DUPVOTE_TOTAL_POWER
	// DupVotePanic: VoteSignBytes of the vote under test panics (a malformed BlockID hash); the caller
	// runs the original Go path, which panics as before.
	DupVotePanic          = C.TMED_DUPVOTE_PANIC
	DupVoteVoteASignature = C.TMED_DUPVOTE_VOTE_A_SIGNATURE
	DupVoteVoteBSignature = C.TMED_DUPVOTE_VOTE_B_SIGNATURE
	// DupVoteGoPath: the flat fields do not determine the reference's outcome: the caller runs
	// VerifyDuplicateVote itself for this evidence.
	DupVoteGoPath = C.TMED_DUPVOTE_GO_PATH
)

// DupEvidenceData is a flat copy of n types.DuplicateVoteEvidence values: VoteA of evidence i is
// vote 2i of Votes, VoteB vote 2i+1.
type DupEvidenceData struct {
	Votes             *VoteData // 2n votes
	TotalVotingPowers []int64
	ValidatorPowers   []int64
	TsSeconds         []int64 // DuplicateVoteEvidence.Timestamp
	TsNanos           []int32
}

// NewDupEvidenceData: n evidences in Go memory (copied into the call's arena once).
func NewDupEvidenceData(n int) *DupEvidenceData {
	return &DupEvidenceData{Votes: NewVoteData(2 * n), TotalVotingPowers: make([]int64, n), ValidatorPowers: make([]int64, n),
		TsSeconds: make([]int64, n), TsNanos: make([]int32, n)}
}

func (a *arena) dupEvidenceC(d *DupEvidenceData) C.tmed_dup_evidence {
	n := len(d.TotalVotingPowers)
	t := C.tmed_dup_evidence{n: C.size_t(n), votes: a.votesC(d.Votes)}
	if n == 0 {
		return t
	}
	t.total_voting_powers, t.validator_powers = a.i64(d.TotalVotingPowers), a.i64(d.ValidatorPowers)
	t.ts_seconds, t.ts_nanos = a.i64(d.TsSeconds), a.i32(d.TsNanos)
	return t
}

// DupVoteRequest is one batch of duplicate-vote evidence against the validator set of its height
// (the set Pool.verify loads, evidence/verify.go:55-59).
type DupVoteRequest struct {
	ChainID  string
	Vals     *ValSet
	Evidence *DupEvidenceData
}

// VerifyDuplicateVotes runs VerifyDuplicateVote on every evidence of every request in ONE device
// batch (tmed_verify_duplicate_votes) and returns the DupVote* outcome codes, one slice per request.
// ValidateBasic, the age checks and the pool's lookups stay with the caller.  An error means "take
// the original Go path".
func (e *Engine) VerifyDuplicateVotes(reqs []DupVoteRequest) ([][]uint8, error) {
	n := len(reqs)
	if n == 0 {
		return nil, nil
	}
	a := e.getArena()
	defer e.putArena(a)
	creqs := (*[1 << 24]C.tmed_dup_request)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_dup_request{})))[:n:n]
	ce := (*[1 << 22]C.tmed_dup_evidence)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_dup_evidence{})))[:n:n]
	vs := (*[1 << 24]C.tmed_valset)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_valset{})))[:n:n]
	seenV := make(map[*ValSet]*C.tmed_valset, n)
	total := 0
	for i := range reqs {
		r := &reqs[i]
		if r.Vals == nil || r.Evidence == nil || r.Evidence.Votes == nil ||
			len(r.Evidence.Votes.Types) != 2*len(r.Evidence.TotalVotingPowers) {
			return nil, errors.New("tmedgpu: VerifyDuplicateVotes: nil evidence or validator set, or not two votes per evidence")
		}
		set, ok := seenV[r.Vals]
		if !ok {
			vs[i] = a.valset(r.Vals)
			set = &vs[i]
			seenV[r.Vals] = set
		}
		ce[i] = a.dupEvidenceC(r.Evidence)
		creqs[i] = C.tmed_dup_request{chain_id: a.cstring(r.ChainID), chain_id_len: C.uint32_t(len(r.ChainID)),
			vals: set, ev: &ce[i]}
		total += len(r.Evidence.TotalVotingPowers)
	}
	codes := make([]uint8, total+1)
	if rc := C.tmed_verify_duplicate_votes(e.ctx, &creqs[0], C.size_t(n), (*C.uint8_t)(unsafe.Pointer(&codes[0]))); rc != 0 {
		return nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	out := make([][]uint8, n)
	at := 0
	for i := range reqs {
		m := len(reqs[i].Evidence.TotalVotingPowers)
		out[i] = codes[at : at+m : at+m]
		at += m
	}
	return out, nil
}

// EvidenceItem names one entry of an evidence list: evidence Index of the call's DupEvidenceData, or,
// when Opaque is not nil, the bytes the caller marshalled itself (a LightClientAttackEvidence's Bytes()).
type EvidenceItem struct {
	Index  int
	Opaque []byte
}

// EvidenceHashes returns DuplicateVoteEvidence.Hash() of every evidence of d and EvidenceList.Hash()
// of every list (tmed_evidence_hashes: Bytes() is encoded and hashed on the device).  evOK[i] is false
// where the flat fields cannot reproduce Bytes() (a hash longer than 32, an address longer than 20, a
// signature longer than 64, a timestamp the reference's Marshal rejects), listOK[l] where list l names
// such an evidence: the caller runs the Go method for those.
func (e *Engine) EvidenceHashes(d *DupEvidenceData, lists [][]EvidenceItem) (hashes [][32]byte, roots [][32]byte, evOK []bool, listOK []bool, err error) {
	if d == nil || d.Votes == nil {
		return nil, nil, nil, nil, errors.New("tmedgpu: EvidenceHashes: nil evidence")
	}
	n, nl := len(d.TotalVotingPowers), len(lists)
	if n+nl == 0 {
		return nil, nil, nil, nil, nil
	}
	var items []int64
	var opaque []byte
	listOff := []uint32{0}
	opOff := []uint64{0}
	for _, l := range lists {
		for _, it := range l {
			if it.Opaque != nil {
				items = append(items, int64(-len(opOff)))
				opaque = append(opaque, it.Opaque...)
				opOff = append(opOff, uint64(len(opaque)))
			} else {
				items = append(items, int64(it.Index))
			}
		}
		listOff = append(listOff, uint32(len(items)))
	}
	opaque = append(opaque, make([]byte, 8)...) // the device reader may touch the last dword
	a := e.getArena()
	defer e.putArena(a)
	ce := (*C.tmed_dup_evidence)(a.alloc(unsafe.Sizeof(C.tmed_dup_evidence{})))
	*ce = a.dupEvidenceC(d)
	ho := (*[1 << 26][32]byte)(a.alloc(uintptr(n+1) * 32))[: n+1 : n+1]
	ro := (*[1 << 26][32]byte)(a.alloc(uintptr(nl+1) * 32))[: nl+1 : nl+1]
	eok := (*[1 << 30]C.uint8_t)(a.alloc(uintptr(n + 1)))[: n+1 : n+1]
	lok := (*[1 << 30]C.uint8_t)(a.alloc(uintptr(nl + 1)))[: nl+1 : nl+1]
	var citems *C.int64_t
	if len(items) > 0 {
		citems = a.i64(items)
	}
	if rc := C.tmed_evidence_hashes(e.ctx, ce, citems, a.u32(listOff), C.size_t(nl), a.bytes(opaque), a.u64(opOff),
		(*C.uint8_t)(unsafe.Pointer(&ho[0])), (*C.uint8_t)(unsafe.Pointer(&ro[0])), &eok[0], &lok[0]); rc != 0 {
		return nil, nil, nil, nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	evOK, listOK = make([]bool, n), make([]bool, nl)
	for i := range evOK {
		evOK[i] = eok[i] != 0
	}
	for i := range listOK {
		listOK[i] = lok[i] != 0
	}
	return append([][32]byte(nil), ho[:n]...), append([][32]byte(nil), ro[:nl]...), evOK, listOK, nil
}

// ---- evidence: VerifyLightClientAttack (evidence/verify.go:113-154, :226-271) and
// GetByzantineValidators (types/evidence.go:233-279) ----

// Outcome codes of VerifyLightClientAttacks: the first check that fails, in the reference's order
// (see tmed25519.h, which cites the reference lines of each).
const (
	LcaOK                   = C.TMED_LCA_OK
	LcaTrusting             = C.TMED_LCA_TRUSTING
	LcaNotDerived           = C.TMED_LCA_NOT_DERIVED
	LcaCommit               = C.TMED_LCA_COMMIT
	LcaTotalPower           = C.TMED_LCA_TOTAL_POWER
	LcaTimeNotViolated      = C.TMED_LCA_TIME_NOT_VIOLATED
	LcaSameHash             = C.TMED_LCA_SAME_HASH
	LcaAmnesiaHasValidators = C.TMED_LCA_AMNESIA_HAS_VALIDATORS
	LcaByzCount             = C.TMED_LCA_BYZ_COUNT
	LcaByzAddress           = C.TMED_LCA_BYZ_ADDRESS
	LcaByzPower             = C.TMED_LCA_BYZ_POWER
	// LcaPanic: the reference panics (a commit check, GetByzantineValidators, or a nil validator in
	// the compare); the caller runs the original Go function, which panics as before.
	LcaPanic = C.TMED_LCA_PANIC
	// LcaGoPath: a header time outside the Timestamp range: the caller runs the Go function.
	LcaGoPath = C.TMED_LCA_GO_PATH
	// The attack kinds GetByzantineValidators distinguishes.
	LcaLunatic      = C.TMED_LCA_LUNATIC
	LcaEquivocation = C.TMED_LCA_EQUIVOCATION
	LcaAmnesia      = C.TMED_LCA_AMNESIA
	ByzOK           = C.TMED_BYZ_OK
	ByzPanic        = C.TMED_BYZ_PANIC
)

// LcaRequest holds the arguments of one VerifyLightClientAttack call as flat copies: the evidence
// (ConflictingBlock, CommonHeight, ByzantineValidators, TotalVotingPower), commonHeader.Height, the
// trusted SignedHeader and commonVals.
type LcaRequest struct {
	ConflictingHeader *HeaderData
	ConflictingCommit *CommitData
	ConflictingVals   *ValSet
	CommonHeight      int64
	TotalVotingPower  int64
	// e.ByzantineValidators: ByzIsNil tells a nil slice from an empty one
	// (LightClientAttackEvidenceFromProto makes an empty non-nil slice).
	ByzIsNil     bool
	ByzAddresses []byte   // n x 20
	ByzAddrLens  []uint32 // nil: all 20
	ByzPowers    []int64  // n
	// commonHeader.Height, trustedHeader (its Commit: round, size and flags are read), commonVals
	CommonHeaderHeight int64
	TrustedHeader      *HeaderData
	TrustedCommit      *CommitData
	CommonVals         *ValSet
}

// ByzResult is GetByzantineValidators of one request: validator indices into CommonVals (LcaLunatic)
// or ConflictingVals (LcaEquivocation) in the reference's order; -1 is a nil entry; a nil List is the
// reference's nil slice.  State ByzPanic: the reference panics.
type ByzResult struct {
	Kind, State int
	List        []int32
}

// LcaResult is one request's outcome; the caller builds the reference's error value from it
// (INTEGRATION.md §2d).
type LcaResult struct {
	Code, Kind                      int
	Commit                          Result // LcaTrusting / LcaCommit / a commit check's LcaPanic
	Expected, Actual                int64
	Idx, ValIdx                     int32
	Byz                             []int32 // the computed list where validateABCIEvidence was reached
	VerifiedTrusting, VerifiedLight uint32
	Hash                            [32]byte // LightClientAttackEvidence.Hash() (zero for LcaNotDerived / LcaGoPath)
}

// lcaArgs builds the C requests and the output ranges of reqs in a.
func lcaArgs(a *arena, reqs []LcaRequest) (*C.tmed_lca_request, []int32, []uint64, error) {
	n := len(reqs)
	creqs := (*[1 << 22]C.tmed_lca_request)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_lca_request{})))[:n:n]
	hs := (*[1 << 24]C.tmed_header)(a.alloc(uintptr(2*n) * unsafe.Sizeof(C.tmed_header{})))[: 2*n : 2*n]
	cs := (*[1 << 24]C.tmed_commit)(a.alloc(uintptr(2*n) * unsafe.Sizeof(C.tmed_commit{})))[: 2*n : 2*n]
	vs := (*[1 << 24]C.tmed_valset)(a.alloc(uintptr(2*n) * unsafe.Sizeof(C.tmed_valset{})))[: 2*n : 2*n]
	seenV := make(map[*ValSet]*C.tmed_valset, 2*n)
	seenC := make(map[*CommitData]*C.tmed_commit, 2*n)
	nv, nc := 0, 0
	valset := func(v *ValSet) *C.tmed_valset {
		cv, ok := seenV[v]
		if !ok {
			vs[nv] = a.valset(v)
			cv = &vs[nv]
			seenV[v] = cv
			nv++
		}
		return cv
	}
	commit := func(c *CommitData) *C.tmed_commit {
		cc, ok := seenC[c]
		if !ok {
			cs[nc] = a.commitC(c, nil)
			cc = &cs[nc]
			seenC[c] = cc
			nc++
		}
		return cc
	}
	off := make([]uint64, n+1)
	for i := range reqs {
		r := &reqs[i]
		if r.ConflictingHeader == nil || r.ConflictingCommit == nil || r.ConflictingVals == nil || r.TrustedHeader == nil ||
			r.TrustedCommit == nil || r.CommonVals == nil || len(r.ByzAddresses) != 20*len(r.ByzPowers) {
			return nil, nil, nil, errors.New("tmedgpu: light client attack: nil header, commit or validator set, or a claimed list of two lengths")
		}
		hs[2*i], hs[2*i+1] = a.headerC(r.ConflictingHeader), a.headerC(r.TrustedHeader)
		var isNil C.uint8_t
		if r.ByzIsNil {
			isNil = 1
		}
		creqs[i] = C.tmed_lca_request{conflicting_header: &hs[2*i], conflicting_commit: commit(r.ConflictingCommit),
			conflicting_vals: valset(r.ConflictingVals), common_height: C.int64_t(r.CommonHeight),
			total_voting_power: C.int64_t(r.TotalVotingPower), n_byz: C.size_t(len(r.ByzPowers)), byz_is_nil: isNil,
			byz_addresses: a.bytes(r.ByzAddresses), byz_address_lens: a.u32(r.ByzAddrLens), byz_powers: a.i64(r.ByzPowers),
			common_header_height: C.int64_t(r.CommonHeaderHeight), trusted_header: &hs[2*i+1],
			trusted_commit: commit(r.TrustedCommit), common_vals: valset(r.CommonVals)}
		off[i+1] = off[i] + uint64(len(r.ConflictingCommit.Flags))
	}
	return &creqs[0], make([]int32, off[n]+1), off, nil
}

// ByzantineValidators is GetByzantineValidators for many evidences in one call
// (tmed_byzantine_validators): the address lookups and the order by voting power are computed on the
// device, with no map and no sort on the host.  An error means "take the original Go path".
func (e *Engine) ByzantineValidators(reqs []LcaRequest) ([]ByzResult, error) {
	n := len(reqs)
	if n == 0 {
		return nil, nil
	}
	a := e.getArena()
	defer e.putArena(a)
	creqs, byz, off, err := lcaArgs(a, reqs)
	if err != nil {
		return nil, err
	}
	res := make([]C.tmed_byz_result, n)
	if rc := C.tmed_byzantine_validators(e.ctx, creqs, C.size_t(n), (*C.int32_t)(unsafe.Pointer(&byz[0])),
		(*C.uint64_t)(unsafe.Pointer(&off[0])), &res[0]); rc != 0 {
		return nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	out := make([]ByzResult, n)
	for i := range res {
		out[i] = ByzResult{Kind: int(res[i].kind), State: int(res[i].state)}
		if m := uint64(res[i].count); m > 0 {
			out[i].List = byz[off[i] : off[i]+m : off[i]+m]
		}
	}
	return out, nil
}

// VerifyLightClientAttacks is VerifyLightClientAttack for many evidences in one call
// (tmed_verify_light_client_attacks): both headers' hashes, both commit checks, the byzantine
// validators and Hash() on the device, the reference's checks replayed in its order.  ValidateBasic,
// the header loads and the age checks of Pool.verify stay with the caller.  An error means "take
// the original Go path".
func (e *Engine) VerifyLightClientAttacks(reqs []LcaRequest) ([]LcaResult, error) {
	n := len(reqs)
	if n == 0 {
		return nil, nil
	}
	a := e.getArena()
	defer e.putArena(a)
	creqs, byz, off, err := lcaArgs(a, reqs)
	if err != nil {
		return nil, err
	}
	res := make([]C.tmed_lca_result, n)
	if rc := C.tmed_verify_light_client_attacks(e.ctx, creqs, C.size_t(n), 0, (*C.int32_t)(unsafe.Pointer(&byz[0])),
		(*C.uint64_t)(unsafe.Pointer(&off[0])), &res[0]); rc != 0 {
		return nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	out := make([]LcaResult, n)
	for i := range res {
		o := LcaResult{Code: int(res[i].code), Kind: int(res[i].kind), Expected: int64(res[i].expected),
			Actual: int64(res[i].actual), Idx: int32(res[i].idx), ValIdx: int32(res[i].val_idx),
			VerifiedTrusting: uint32(res[i].verified_trusting), VerifiedLight: uint32(res[i].verified_light)}
		o.Commit = toResults([]C.tmed_commit_result{res[i].commit})[0]
		if m := uint64(res[i].n_byz_expected); m > 0 {
			o.Byz = byz[off[i] : off[i]+m : off[i]+m]
		}
		for k := 0; k < 32; k++ {
			o.Hash[k] = byte(res[i].hash[k])
		}
		out[i] = o
	}
	return out, nil
}

// ---- validateBlock (state/validation.go:15-151 over Block.ValidateBasic, types/block.go:55-106) ----

// Outcome codes of ValidateBlocks: the first check that fails, in the reference's order (see
// tmed25519.h, which cites the reference lines of each).
const (
	VbOK                 = C.TMED_VB_OK
	VbHeaderBasic        = C.TMED_VB_HEADER_BASIC
	VbCommitBasic        = C.TMED_VB_COMMIT_BASIC
	VbLastCommitHash     = C.TMED_VB_LAST_COMMIT_HASH
	VbDataHash           = C.TMED_VB_DATA_HASH
	VbEvidenceBasic      = C.TMED_VB_EVIDENCE_BASIC
	VbEvidenceHash       = C.TMED_VB_EVIDENCE_HASH
	VbVersion            = C.TMED_VB_VERSION
	VbChainID            = C.TMED_VB_CHAIN_ID
	VbHeightInitial      = C.TMED_VB_HEIGHT_INITIAL
	VbHeight             = C.TMED_VB_HEIGHT
	VbLastBlockID        = C.TMED_VB_LAST_BLOCK_ID
	VbAppHash            = C.TMED_VB_APP_HASH
	VbConsensusHash      = C.TMED_VB_CONSENSUS_HASH
	VbLastResultsHash    = C.TMED_VB_LAST_RESULTS_HASH
	VbValidatorsHash     = C.TMED_VB_VALIDATORS_HASH
	VbNextValidatorsHash = C.TMED_VB_NEXT_VALIDATORS_HASH
	VbInitialHasSigs     = C.TMED_VB_INITIAL_HAS_SIGS
	// VbLastCommit: state.LastValidators.VerifyCommit failed; BlockResult.Commit holds its outcome.
	VbLastCommit         = C.TMED_VB_LAST_COMMIT
	VbProposerSize       = C.TMED_VB_PROPOSER_SIZE
	VbProposerUnknown    = C.TMED_VB_PROPOSER_UNKNOWN
	VbTimeNotAfter       = C.TMED_VB_TIME_NOT_AFTER
	VbTimeNotMedian      = C.TMED_VB_TIME_NOT_MEDIAN
	VbTimeNotGenesis     = C.TMED_VB_TIME_NOT_GENESIS
	VbHeightBelowInitial = C.TMED_VB_HEIGHT_BELOW_INITIAL
	VbEvidenceOverflow   = C.TMED_VB_EVIDENCE_OVERFLOW
	// VbGoPath: the flat fields cannot decide the check the replay reached: the caller runs
	// validateBlock itself for this block.
	VbGoPath = C.TMED_VB_GO_PATH
	// The bits of BlockState.Known and BlockResult.Skipped.
	VbKnowAppHash         uint32 = C.TMED_VB_KNOW_APP_HASH
	VbKnowConsensusHash   uint32 = C.TMED_VB_KNOW_CONSENSUS_HASH
	VbKnowLastResultsHash uint32 = C.TMED_VB_KNOW_LAST_RESULTS_HASH
	VbKnowValidators      uint32 = C.TMED_VB_KNOW_VALIDATORS
	VbKnowNextValidators  uint32 = C.TMED_VB_KNOW_NEXT_VALIDATORS
	VbKnowAll             uint32 = C.TMED_VB_KNOW_ALL
)

// BlockState is a flat copy of the fields of state.State that validateBlock reads.  Known is a mask
// of VbKnow*: a check whose bit is clear is skipped and reported in BlockResult.Skipped (a blocksync
// window validated ahead of ApplyBlock does not have those values); the caller evaluates the skipped
// checks in Go before it relies on the block, and first of all when a skipped check orders before a
// failure's code.
type BlockState struct {
	VersionBlock, VersionApp        uint64
	ChainID                         string
	InitialHeight, LastBlockHeight  int64
	LastBlockID                     BlockID
	LastBlockTimeSeconds            int64
	LastBlockTimeNanos              int32
	AppHash                         []byte
	ConsensusHash                   []byte // types.HashConsensusParams(state.ConsensusParams), 32 bytes
	LastResultsHash                 []byte
	Validators, NextValidators      *ValSet // nil allowed where the set's bit is clear
	LastValidators                  *ValSet
	EvidenceMaxBytes                int64
	Known                           uint32
}

// BlockRequest is one block against one state.  LinkPrev (requests 1..): the state's last block hash,
// height and time are the previous request's block's, its Header.Hash computed on the device in the
// same call; the PartSetHeader half of LastBlockID still comes from State.LastBlockID.
type BlockRequest struct {
	Header           *HeaderData
	LastCommit       *CommitData // nil: a nil LastCommit (CommitBasicOK must be false)
	State            *BlockState
	Txs              [][]byte
	Evidence         []EvidenceItem // indexes into ValidateBlocks' evidence argument, or marshalled bytes
	EvidenceByteSize int64          // block.Evidence.ByteSize()
	HeaderBasicOK    bool           // Header.ValidateBasic() == nil
	CommitBasicOK    bool           // LastCommit != nil && LastCommit.ValidateBasic() == nil
	EvidenceBasicBad int32          // -1, or the index of the first evidence whose ValidateBasic fails
	LinkPrev         bool
}

// BlockResult is one block's outcome; the caller builds the reference's error value from it
// (INTEGRATION.md).
type BlockResult struct {
	Code          int
	Skipped       uint32
	Hash          []byte // the computed value of the hash codes (nil where none)
	Commit        Result // VbLastCommit: the failing VerifyCommit's outcome
	MedianSeconds int64  // VbTimeNotMedian: state.MedianTime
	MedianNanos   int32
	Idx           int32 // VbEvidenceBasic
	ProposerIdx   int32 // the proposer's index in State.Validators, -1 where not looked up or not found
	Verified      uint32
}

// ValidateBlocks is validateBlock for many blocks in one call (tmed_validate_blocks): the hashes of
// Block.ValidateBasic, the validator-set hashes, the compares and the proposer lookup on the device,
// VerifyCommit through the commit seam, MedianTime by its kernels, and the reference's checks replayed
// in its order.  evidence holds the DuplicateVoteEvidence of all blocks (nil: none).  An error means
// "take the original Go path".
func (e *Engine) ValidateBlocks(reqs []BlockRequest, evidence *DupEvidenceData) ([]BlockResult, error) {
	n := len(reqs)
	if n == 0 {
		return nil, nil
	}
	a := e.getArena()
	defer e.putArena(a)
	creqs := (*[1 << 24]C.tmed_block_request)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_block_request{})))[:n:n]
	hs := (*[1 << 24]C.tmed_header)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_header{})))[:n:n]
	cs := (*[1 << 24]C.tmed_commit)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_commit{})))[:n:n]
	ss := (*[1 << 24]C.tmed_block_state)(a.alloc(uintptr(n) * unsafe.Sizeof(C.tmed_block_state{})))[:n:n]
	vs := (*[1 << 24]C.tmed_valset)(a.alloc(uintptr(3*n) * unsafe.Sizeof(C.tmed_valset{})))[: 3*n : 3*n]
	// one C copy per distinct *ValSet, *BlockState and *CommitData: the library hashes, stages and
	// resolves each set once per call
	seenV := make(map[*ValSet]*C.tmed_valset, 3)
	seenS := make(map[*BlockState]*C.tmed_block_state, n)
	seenC := make(map[*CommitData]*C.tmed_commit, n)
	nv, ns := 0, 0
	valset := func(v *ValSet) *C.tmed_valset {
		if v == nil {
			return nil
		}
		cv, ok := seenV[v]
		if !ok {
			vs[nv] = a.valset(v)
			cv = &vs[nv]
			seenV[v] = cv
			nv++
		}
		return cv
	}
	var txs, opaque []byte
	var items []int64
	txOff, opOff := []uint64{0}, []uint64{0}
	blockOff, listOff := []uint32{0}, []uint32{0}
	flag := func(b bool) C.uint8_t {
		if b {
			return 1
		}
		return 0
	}
	for i := range reqs {
		r := &reqs[i]
		if r.Header == nil || r.State == nil || (r.LastCommit == nil && r.CommitBasicOK) {
			return nil, errors.New("tmedgpu: ValidateBlocks: nil header, state or commit")
		}
		hs[i] = a.headerC(r.Header)
		var cc *C.tmed_commit
		if r.LastCommit != nil {
			var ok bool
			if cc, ok = seenC[r.LastCommit]; !ok {
				cs[i] = a.commitC(r.LastCommit, nil)
				cc = &cs[i]
				seenC[r.LastCommit] = cc
			}
		}
		st, ok := seenS[r.State]
		if !ok {
			s := r.State
			ss[ns] = C.tmed_block_state{version_block: C.uint64_t(s.VersionBlock), version_app: C.uint64_t(s.VersionApp),
				chain_id: a.cstring(s.ChainID), chain_id_len: C.uint32_t(len(s.ChainID)),
				initial_height: C.int64_t(s.InitialHeight), last_block_height: C.int64_t(s.LastBlockHeight),
				last_block_id: a.blockID(&s.LastBlockID), last_block_time_seconds: C.int64_t(s.LastBlockTimeSeconds),
				last_block_time_nanos: C.int32_t(s.LastBlockTimeNanos), app_hash: a.bytes(s.AppHash),
				app_hash_len: C.uint32_t(len(s.AppHash)), consensus_hash: a.bytes(s.ConsensusHash),
				last_results_hash: a.bytes(s.LastResultsHash), last_results_hash_len: C.uint32_t(len(s.LastResultsHash)),
				validators: valset(s.Validators), next_validators: valset(s.NextValidators),
				last_validators: valset(s.LastValidators), evidence_max_bytes: C.int64_t(s.EvidenceMaxBytes),
				known: C.uint32_t(s.Known)}
			if s.Known&VbKnowConsensusHash != 0 && len(s.ConsensusHash) != 32 {
				return nil, errors.New("tmedgpu: ValidateBlocks: ConsensusHash must be 32 bytes")
			}
			st = &ss[ns]
			seenS[r.State] = st
			ns++
		}
		var flags C.uint32_t
		if r.LinkPrev {
			flags = C.TMED_VB_LINK_PREV
		}
		creqs[i] = C.tmed_block_request{header: &hs[i], last_commit: cc, state: st,
			evidence_byte_size: C.int64_t(r.EvidenceByteSize), header_basic_ok: flag(r.HeaderBasicOK),
			commit_basic_ok: flag(r.CommitBasicOK), evidence_basic_bad: C.int32_t(r.EvidenceBasicBad), flags: flags}
		for _, tx := range r.Txs {
			txs = append(txs, tx...)
			txOff = append(txOff, uint64(len(txs)))
		}
		blockOff = append(blockOff, uint32(len(txOff)-1))
		for _, it := range r.Evidence {
			if it.Opaque != nil {
				items = append(items, int64(-len(opOff)))
				opaque = append(opaque, it.Opaque...)
				opOff = append(opOff, uint64(len(opaque)))
			} else {
				items = append(items, int64(it.Index))
			}
		}
		listOff = append(listOff, uint32(len(items)))
	}
	txs = append(txs, make([]byte, 8)...) // the device readers may touch the last dword
	opaque = append(opaque, make([]byte, 8)...)
	if evidence == nil {
		evidence = NewDupEvidenceData(0)
	}
	ce := (*C.tmed_dup_evidence)(a.alloc(unsafe.Sizeof(C.tmed_dup_evidence{})))
	*ce = a.dupEvidenceC(evidence)
	var citems *C.int64_t
	if len(items) > 0 {
		citems = a.i64(items)
	}
	batch := (*C.tmed_block_batch)(a.alloc(unsafe.Sizeof(C.tmed_block_batch{})))
	*batch = C.tmed_block_batch{n: C.size_t(n), blocks: &creqs[0], txs: a.bytes(txs), tx_off: a.u64(txOff),
		block_off: a.u32(blockOff), ev: ce, items: citems, list_off: a.u32(listOff), opaque: a.bytes(opaque),
		opaque_off: a.u64(opOff)}
	res := make([]C.tmed_block_result, n)
	if rc := C.tmed_validate_blocks(e.ctx, batch, &res[0]); rc != 0 {
		return nil, errors.New(C.GoString(C.tmed_strerror(rc)))
	}
	out := make([]BlockResult, n)
	for i := range res {
		o := BlockResult{Code: int(res[i].code), Skipped: uint32(res[i].skipped), MedianSeconds: int64(res[i].median_seconds),
			MedianNanos: int32(res[i].median_nanos), Idx: int32(res[i].idx), ProposerIdx: int32(res[i].proposer_idx),
			Verified: uint32(res[i].verified)}
		o.Commit = toResults([]C.tmed_commit_result{res[i].commit})[0]
		if hl := int(res[i].hash_len); hl > 0 {
			o.Hash = make([]byte, hl)
			for k := 0; k < hl; k++ {
				o.Hash[k] = byte(res[i].hash[k])
			}
		}
		out[i] = o
	}
	return out, nil
}
