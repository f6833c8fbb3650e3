/*
 * tmed25519.h — C ABI of the MI355X batch ed25519 verification engine
 * (libtmed25519_hip.so, built from tendermint-fork_amd/csrc for gfx950).
 *
 * The reference (Tendermint Core v0.34.24, pure Go) has no native boundary on
 * this path: every signature goes through the Go interface method
 *     crypto.PubKey.VerifySignature(msg, sig []byte) bool      crypto/crypto.go:25
 *     -> ed25519.PubKey.VerifySignature                      crypto/ed25519/ed25519.go:148-155
 * called one at a time from the commit-verification loops
 *     ValidatorSet.VerifyCommit                              types/validator_set.go:667-714 (call :696)
 *     ValidatorSet.VerifyCommitLight                         types/validator_set.go:722-765 (call :752)
 *     ValidatorSet.VerifyCommitLightTrusting                 types/validator_set.go:775-826 (call :813)
 * This header is what a cgo shim at that seam binds: the
 * per-signature calls of one commit (or of many commits) become ONE call that
 * returns a validity byte per tuple, and the shim replays the reference loop
 * over those bytes, so early exits, error values and tallies are unchanged.
 *
 * Conventions
 *   - Plain pointers and sizes only; no allocation is handed across the ABI.
 *   - Return 0 on success, a negative TMED_E* code on failure.  On failure the
 *     caller must not use out_valid (the Go shim then calls the original Go
 *     method — never a guessed decision).  Nothing aborts or throws across the ABI.
 *   - out_valid[i] is 1 iff Go 1.18 crypto/ed25519.Verify would return true for
 *     (pub[i], msg[i], sig[i]) (and len(sig[i]) == 64): cofactorless, S < L
 *     strict, permissive A decoding, byte-compared R.
 *   - All host pointers are only read during the call (cgo pointer rules: the
 *     library copies what it needs before returning).  A context may be shared
 *     by concurrent callers: calls on one context are serialised internally.
 */
#ifndef TMED25519_H
#define TMED25519_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMED_OK 0
#define TMED_EINVAL (-1)    /* bad argument (null pointer, offsets not monotone, ...) */
#define TMED_ENODEV (-2)    /* no usable gfx950 device */
#define TMED_EHIP (-3)      /* HIP runtime error (device lost, launch failure) */
#define TMED_ENOMEM (-4)    /* device or pinned-host allocation failed */
#define TMED_ENOKEYSET (-5) /* unknown key-set handle */
#define TMED_EINTERNAL (-6) /* internal error: a host-side exception inside the library (a bug, never a
                               decision); the call's outputs are unusable.  A seam call that fails this
                               way (or any other way) while blocksync windows are in flight on the
                               context drops those windows: their results are not final, and
                               tmed_blocksync_wait reports the error */

typedef struct tmed_ctx tmed_ctx;

/* Number of visible HIP devices (0 when none). */
int tmed_device_count(void);

/* Create a context bound to HIP device `device` (one process per GPU). */
int tmed_init(int device, tmed_ctx **out);
void tmed_destroy(tmed_ctx *ctx);
const char *tmed_strerror(int code);

/*
 * Batch verification, host buffers.  Replaces n calls of
 * ed25519.PubKey.VerifySignature (crypto/ed25519/ed25519.go:148-155).
 *   pubkeys   n x 32 bytes
 *   sigs      n x 64 bytes (slot i holds the first sig_lens[i] bytes when sig_lens != NULL)
 *   sig_lens  NULL (all 64) or n lengths; any length != 64 is rejected
 *             (ed25519.go:150-152) without touching the device
 *   msgs      concatenated messages; message i is msgs[msg_off[i] .. msg_off[i+1])
 *   msg_off   n + 1 non-decreasing offsets
 *   out_valid n bytes, 0/1
 */
int tmed_verify_batch(tmed_ctx *ctx, const uint8_t *pubkeys, const uint8_t *sigs, const uint32_t *sig_lens,
                      const uint8_t *msgs, const uint32_t *msg_off, size_t n, uint8_t *out_valid);

/*
 * Same, on device-resident buffers (all pointers are device pointers of the
 * context's device; stream = hipStream_t or NULL for the context stream).
 * Asynchronous: completion is ordered on `stream`.  Used when inputs already
 * live in HBM (bench, multi-commit pipelines).
 */
int tmed_verify_batch_device(tmed_ctx *ctx, const uint8_t *d_pubkeys, const uint8_t *d_sigs,
                             const uint8_t *d_msgs, const uint32_t *d_msg_off, size_t n, uint8_t *d_out_valid,
                             void *stream);

/*
 * RFC 8032 signing (crypto/ed25519/ed25519.go:57-60 semantics) used to build
 * synthetic commits at scale (SURVEY.md §7 "synthetic data volume").
 * seeds n x 32, outputs sigs n x 64 and pubkeys n x 32.
 */
int tmed_sign_batch(tmed_ctx *ctx, const uint8_t *seeds, const uint8_t *msgs, const uint32_t *msg_off, size_t n,
                    uint8_t *sigs_out, uint8_t *pubkeys_out);
int tmed_sign_batch_device(tmed_ctx *ctx, const uint8_t *d_seeds, const uint8_t *d_msgs, const uint32_t *d_msg_off,
                           size_t n, uint8_t *d_sigs_out, uint8_t *d_pubkeys_out, void *stream);

/*
 * Diagnostics of the default (half-size scalar) path: for the last chunk of the last
 * tmed_verify_batch / _device call, histograms of the radix-16 window count W the lattice step
 * gave each signature (lane_hist[W]) and of the per-wave maximum the main kernel ran
 * (wave_hist[W], 64 signatures per wave; W = 64 is the unshortened (k, 1) fallback).
 * All zero when the last call took another path.
 */
int tmed_window_stats(tmed_ctx *ctx, uint32_t lane_hist[65], uint32_t wave_hist[65]);

/*
 * Radix (in bits) of the fixed-base B windows of the default path on this context: 26 (two
 * tables of 2^25 + 1 affine multiples of B and 2^128 B, 8.6 GB per device, ten B additions per
 * signature) or 16 (windows of the context's radix-2^16 comb, sixteen additions: TMED_B26=0 or
 * when the large tables could not be allocated).  Diagnostic; decisions are identical.
 */
int tmed_b_window_bits(const tmed_ctx *ctx);
/*
 * The same for the key-cached throughput path: 24 (a shared radix-2^24 comb of B, 11 windows of
 * 2^23 + 1 multiples, 11.8 GB per device, acquired at the context's first tmed_keyset_load:
 * eleven B additions per signature) or 16 (the context's radix-2^16 comb, sixteen: before any
 * key-set load, with TMED_B24=0, or when the allocation failed).  Diagnostic; same decisions.
 */
int tmed_keyset_b_window_bits(const tmed_ctx *ctx);
/*
 * Radix (in bits) of the -A comb the key-cached throughput kernel reads for key set `handle`: 12
 * (21 windows of 2049 multiples, the top one 4225, 5.8 MB per key, built at the set's first
 * throughput batch with the radix-2^24 B comb in use: 32 comb rows per signature) or 8 (the
 * radix-256 comb every key set holds, also used by the latency kernels: TMED_KS_ACOMB=0, before
 * the first throughput batch, or no memory).  -1 for an unknown handle.  Diagnostic; decisions
 * are identical.
 */
int tmed_keyset_a_window_bits(tmed_ctx *ctx, uint64_t handle);
/*
 * Diagnostic (tests): entry j of window `window` of key `key`'s comb in key set `handle`, as the 30
 * int32 limbs (radix 2^25.5) the kernels read: y + x, y - x, 2d x y of the affine point
 * j * R^window * (-A_key), with R = 256 for radix_bits 8 (the comb every key set holds) or
 * R = 2^radix_bits for the throughput comb (radix_bits = tmed_keyset_a_window_bits(handle)).
 * Drains the device first.  TMED_EINVAL for an unknown handle, an index out of range or a comb
 * not built.
 */
int tmed_keyset_comb_entry(tmed_ctx *ctx, uint64_t handle, uint32_t key, int radix_bits, uint32_t window, uint32_t j,
                           int32_t out[30]);

/* Device time (ms) of the last verify/sign launch on this context (HIP events).  A commit batch
 * small enough for the zero-copy latency mode (a single commit), or a tmed_verify_batch of at most
 * 1024 signatures, reports 0 unless kernel timing is on (tmed_set_kernel_timing): its events would
 * add ~8 us to the call. */
float tmed_last_kernel_ms(tmed_ctx *ctx);

/*
 * Per-kernel timing of tmed_verify_batch_device (diagnostics, bench roofline): when on,
 * HIP events are recorded on the launch stream around each kernel of a call;
 * tmed_kernel_times returns, for the last call, the summed device time (ms) and the
 * launch count of each kernel kind: [0] prep (SHA-512, scalar checks, decompression),
 * [1] main (table + Straus), [2] finish (batched inversion + encode + compare).
 */
int tmed_set_kernel_timing(tmed_ctx *ctx, int on);
int tmed_kernel_times(tmed_ctx *ctx, float ms[3], int launches[3]);


/* ------------------------------------------------------- key-set cache */

/*
 * Decode a validator set's keys once (Point.SetBytes rule) and build a
 * signed radix-256 comb of -A per key in HBM.  Signatures
 * are then verified by key index: 64 mixed additions, no doublings, no per-
 * signature decompression.  Decisions are identical to tmed_verify_batch.
 * Callers key the handle by ValidatorSet.Hash() (types/validator_set.go:347-353).
 */
int tmed_keyset_load(tmed_ctx *ctx, const uint8_t *pubkeys, size_t n, uint64_t *handle);
int tmed_keyset_free(tmed_ctx *ctx, uint64_t handle);
/*
 * Append n keys to a loaded key set (its comb tables are built before the call returns).  The keys
 * already in the set keep their indexes; the new ones get first_index .. first_index + n - 1
 * (*first_index = the set's size before the call; may be NULL).  One pooled set can then serve
 * validator sets that change by a few keys per height (tmed_valset.keyset_index), as the light
 * client's do (light/verifier.go:58,73-76).
 */
int tmed_keyset_extend(tmed_ctx *ctx, uint64_t handle, const uint8_t *pubkeys, size_t n, uint32_t *first_index);
int tmed_verify_batch_keyset(tmed_ctx *ctx, uint64_t handle, const uint32_t *val_idx, const uint8_t *sigs,
                             const uint32_t *sig_lens, const uint8_t *msgs, const uint32_t *msg_off, size_t n,
                             uint8_t *out_valid);
int tmed_verify_batch_keyset_device(tmed_ctx *ctx, uint64_t handle, const uint32_t *d_val_idx, const uint8_t *d_sigs,
                                    const uint8_t *d_msgs, const uint32_t *d_msg_off, size_t n, uint8_t *d_out_valid,
                                    void *stream);

/* ---------------------------------------------------------------- ZIP-215 (opt-in) */

/*
 * The OPT-IN ZIP-215 rule (spec/core/encoding.md:52-54: "Tendermint adopted zip215 for verification
 * of ed25519 signatures ... released in 0.35"; the reference's own code, crypto/ed25519/ed25519.go:
 * 148-155, verifies with Go 1.18's cofactorless Verify, which tmed_verify_batch reproduces and which
 * stays the default).  Rule: A and R decoded permissively (y >= p and x = 0 with the sign bit
 * accepted), S < L, k = SHA-512(R || A || M) mod L, accept iff [8]([S]B - R - [k]A) = O.
 * Chunks of up to 2^20 signatures are checked as ONE randomized batch equation (Pippenger MSM with
 * secret 126-bit weights from getrandom); a failing chunk is bisected and the failing groups are
 * decided signature by signature by the exact single check, so out_valid[i] equals the ZIP-215
 * single-signature decision for every i.  sig_lens as in tmed_verify_batch.
 */
int tmed_verify_batch_zip215(tmed_ctx *ctx, const uint8_t *pubkeys, const uint8_t *sigs, const uint32_t *sig_lens,
                             const uint8_t *msgs, const uint32_t *msg_off, size_t n, uint8_t *out_valid);
int tmed_verify_batch_zip215_device(tmed_ctx *ctx, const uint8_t *d_pubkeys, const uint8_t *d_sigs,
                                    const uint8_t *d_msgs, const uint32_t *d_msg_off, size_t n, uint8_t *d_out_valid,
                                    void *stream);
/* Tests only: fix the batch weights' 32-byte seed for this thread's calls (NULL: getrandom again).
 * TMED_EINVAL unless the process environment has TMED_ZIP215_TEST_SEED=1 (known weights would let a
 * forger build invalid signatures whose errors cancel in the batch equation). */
int tmed_zip215_set_seed(const uint8_t *seed32);
/* This thread's last ZIP-215 call: chunks, batch equations evaluated, groups decided signature by
 * signature, signatures decided singly. */
int tmed_zip215_stats(uint32_t out[4]);

/*
 * The same rule by key index.  Same contract as tmed_verify_batch_keyset(_device): the host form
 * returns TMED_EINVAL for a key index past the set, the device form rejects that signature; a key
 * that does not decode rejects its signatures (keys decode identically under both rules: Point.SetBytes
 * is ZIP-215's permissive decoding); sig_lens as in tmed_verify_batch.  out_valid[i] is the ZIP-215
 * single-signature decision stated above.  The decision is exact and deterministic: the key-cached
 * prep and main kernels leave P = [S]B + [k](-A), and one lane per signature decodes R permissively
 * and checks [8](P - R) = O.  No random weights and no host read-back in the middle, which is why
 * this form, and not the batch equation, is what the seam queues under TMED_RULE_ZIP215.
 */
int tmed_verify_batch_keyset_zip215(tmed_ctx *ctx, uint64_t handle, const uint32_t *val_idx, const uint8_t *sigs,
                                    const uint32_t *sig_lens, const uint8_t *msgs, const uint32_t *msg_off, size_t n,
                                    uint8_t *out_valid);
int tmed_verify_batch_keyset_zip215_device(tmed_ctx *ctx, uint64_t handle, const uint32_t *d_val_idx,
                                           const uint8_t *d_sigs, const uint8_t *d_msgs, const uint32_t *d_msg_off,
                                           size_t n, uint8_t *d_out_valid, void *stream);

/*
 * The signature rule of a context's SEAM calls: tmed_verify_commits, tmed_blocksync_verify / _submit /
 * _wait, tmed_light_verify, tmed_verify_votes and the _multi forms (TMED_EINVAL when their contexts'
 * rules differ).  A new context has TMED_RULE_GO.  tmed_set_rule collects the submitted blocksync
 * windows first, as every seam call does, so a window is decided under the rule it was submitted
 * under, and a call reads the rule once: no call mixes rules.  TMED_EINVAL for an unknown rule.
 * ONLY THE SIGNATURE DECISION CHANGES.  The loops, prechecks, early exits, candidate selection and
 * error values stay v0.34.24's: a chain on a later release that verifies with ZIP-215 gets that
 * release's signature decisions inside 0.34's VerifyCommit* / light.Verify / Vote.Verify loops (a
 * shim for a later release's loops replays them over tmed_verify_batch_keyset_zip215's bits).
 * The raw batch calls keep the rule their name states (tmed_verify_batch, tmed_verify_batch_keyset
 * and their _device forms: always the Go rule), the *_with entries take the caller's verifier.
 * The key-set cache is untouched by a rule change (keys decode identically under both rules).
 * Under TMED_RULE_ZIP215 key-cached batches take tmed_verify_batch_keyset_zip215's kernels and
 * generic batches the exact single check per signature (no batch equation in the seam).
 */
#define TMED_RULE_GO 0     /* Go 1.18 crypto/ed25519.Verify: the default, as today */
#define TMED_RULE_ZIP215 1 /* the rule stated at tmed_verify_batch_zip215 */
int tmed_set_rule(tmed_ctx *ctx, int rule);
int tmed_rule(const tmed_ctx *ctx);

/* ---------------------------------------------------------------- commits */

/*
 * The per-commit part of a vote's CanonicalVote sign-bytes:
 * everything Commit.GetVote (types/block.go:784-796) copies from the commit.
 */
typedef struct {
  const char *chain_id;
  uint32_t chain_id_len;
  int64_t height;
  int32_t round;
  const uint8_t *block_hash; /* 0 or 32 bytes (ValidateHash) */
  uint32_t block_hash_len;
  uint32_t psh_total;
  const uint8_t *psh_hash;   /* 0 or 32 bytes */
  uint32_t psh_hash_len;
} tmed_vote_template;

/*
 * Commit.VoteSignBytes(chainID, idx) for n commit signatures
 * (types/block.go:807-810 -> types/vote.go:93-101): flags[i] in {1,2,3}
 * (BlockIDFlag; NULL = all Commit), per-signature timestamp (seconds, nanos).
 * Writes message i to out[out_off[i] .. out_off[i+1]) when out_cap suffices;
 * *out_len receives the total size (call with out = NULL to size the buffer,
 * TMED_ENOMEM when out_cap is too small).  Unknown flags -> TMED_EINVAL
 * (the reference panics, types/block.go:663).
 */
int tmed_vote_sign_bytes(const tmed_vote_template *t, size_t n, const uint8_t *flags, const int64_t *ts_seconds,
                         const int32_t *ts_nanos, uint8_t *out, size_t out_cap, uint32_t *out_off, size_t *out_len);

/* --------------------------------------------------------- diagnostics */

/*
 * Integer-VALU peak probe for the roofline: runs a
 * dependency-free stream of `kind` instructions on every lane of the device
 * (0 v_mad_i64_i32, 1 v_mad_u64_u32, 2 v_add_u32, 3 v_mul_lo_u32, 4 v_ashrrev_i64,
 * 5 v_lshl_add_u64, 6 v_lshl_add_u32, 7 v_add_co_u32+v_addc_co_u32, 8 v_lshrrev_b64,
 * 9 v_alignbit_b32, 10 v_and_b32, 11 v_bfe_i32, 12 v_and_or_b32, 13 v_cndmask_b32,
 * 14 v_ashrrev_i32, 15 v_cndmask_b32_e64 with an SGPR lane mask, 16 / 17 v_cmp_gt_u32 +
 * v_cndmask_b32 through vcc / an SGPR pair, counted as 2)
 * and returns the sustained rate in 1e9 instructions (lane-ops) per second.
 */
int tmed_valu_peak(tmed_ctx *ctx, int kind, double *giga_ops_per_s);

/*
 * Test hooks of the commit seam (process-wide, 0 = off, the product default; tests only):
 * tmed_test_pool_jitter — every part of the seam's host-parallel regions starts up to max_us
 * microseconds late (a part reading what another part of the same region writes then sees it
 * unwritten); tmed_test_stream_delay — a wave sleeping ~us microseconds is queued in front of every
 * batch copy on the copy stream and every key append on the context stream (a kernel lane that does
 * not wait for its producer then reads unfinished data).  tests/test_gpu_jitter.py,
 * tests/test_gpu_stream_delay.py.
 */
void tmed_test_pool_jitter(int max_us);
void tmed_test_stream_delay(int us);

/*
 * Tests only (tests/test_gpu_joint_table.py): the per-lane joint radix-4 table of the half-size
 * main kernel, built on the device for n <= 65536 triples.  a, r: n x 32-byte point encodings
 * (decoded like a public key; the identity when one does not decode), dneg: n bytes, the sign of d
 * (the table is of -A and, for dneg = 0, -R, else +R).  rows: n x 12 x 128 bytes out, row
 * |5i + j| - 1 of a triple the entry i (-A) + j (-+R) as four packed 32-byte field elements
 * (Y+X, Y-X, Z, 2dT).
 */
int tmed_test_joint_rows(tmed_ctx *ctx, const uint8_t *a, const uint8_t *r, const uint8_t *dneg, size_t n,
                         uint8_t *rows);

/*
 * Tests only (tests/test_gpu_lds_rows.py): the same table built through the accessor of the default
 * main kernel, which keeps rows 1 (-+R) and 5 (-A) in LDS without Z and the other ten in the
 * slab.  rows: n x 12 x 128 bytes in and out, the slab: rows 1 and 5 of every triple come back as
 * they went in.  out: n x 13 x 2 x 40 int32, every row 0..12 (0: the identity) read back through
 * the accessor, first as stored, then with Y+X and Y-X exchanged (a negative digit's read), as the
 * ten limbs each of Y+X, Y-X, Z, 2dT that the kernel computes with.
 */
int tmed_test_lds_rows(tmed_ctx *ctx, const uint8_t *a, const uint8_t *r, const uint8_t *dneg, size_t n,
                       uint8_t *rows, int32_t *out);

/*
 * Tests only (tests/test_gpu_hs_k.py): tmed_verify_batch's generic kernels at a chosen k.  Verifies
 * n signatures over empty messages as an ordinary generic call of this context would (the latency
 * kernels up to TMED_GLAT_MAX signatures, the throughput kernels above, the context's main variant
 * and B radix, its chunks), except that signature i uses k32[i] (32 bytes, little-endian, < L) in
 * place of SHA-512(R || A || M) mod L: the lattice step, the recodings, e = d S mod L, the window
 * count and the wave's loop length then follow from a k a test chooses, which no signature can.
 * zip215 != 0: the throughput kernels with the cofactored test, whatever n.  TMED_EINVAL for a
 * k >= L.
 */
int tmed_test_verify_k(tmed_ctx *ctx, const uint8_t *pubkeys, const uint8_t *sigs, const uint8_t *k32, size_t n,
                       int zip215, uint8_t *out);

/*
 * Tests only (tests/test_gpu_table_rows.py): the fixed-base tables of B, row by row.  table: 0 the
 * radix-256 comb (32 windows x 129 rows), 1 the radix-2^16 table (32769 rows), 2 the radix-2^16
 * comb (16 x 32769), 3 the two radix-2^26 tables (2 x (2^25 + 1)), 4 the radix-2^24 comb
 * (11 x (2^23 + 1), present after the first key-set load).
 *
 * tmed_test_b_table_entry: row j of window `window` as the 30 int32 limbs the kernels read (y + x,
 * y - x, 2d x y of the affine point, as tmed_keyset_comb_entry).  Drains the device first.
 * TMED_EINVAL for a table this context does not hold or an index out of range.
 *
 * tmed_test_table_chain: one device lane per row of a whole table: B table `table` (handle = 0), or
 * every key's comb of key set `handle` (radix_bits 8, or tmed_keyset_a_window_bits once that comb is
 * built).  Row (w, 0) must be the identity (1, 1, 0); row (w, j) = row (w, j - 1) + row (w, 1) for
 * j >= 2 (the kernels' own mixed addition, all three coordinates compared fully reduced);
 * row (w + 1, 1) = 2^r row (w, 1) (table 3: 2^128).  Table 4's window 10 follows the chain up to
 * j = 32767 and is the identity beyond; a key that does not decode has every row the identity.
 * *rows: the rows checked; *n_bad: the rows that fail; first_bad: up to 16 of them as
 * window << 32 | j, in any order.  corrupt_j != 0 (tables 0..2 only, handle = 0): the check runs on
 * a scratch copy of the table whose row (corrupt_window, corrupt_j) has limb 0 of its first
 * coordinate one off, so a caller sees the check fail.
 */
int tmed_test_b_table_entry(tmed_ctx *ctx, int table, uint32_t window, uint32_t j, int32_t out[30]);
int tmed_test_table_chain(tmed_ctx *ctx, int table, uint64_t handle, int radix_bits, uint32_t corrupt_window,
                          uint32_t corrupt_j, uint64_t *rows, uint64_t *n_bad, uint64_t first_bad[16]);

/*
 * Tests only (tests/test_gpu_zip_msm.py): the ZIP-215 batch mode's multi-scalar multiplication
 * (csrc/zip215.hip zip_msm: the column sums of c, the two-pass sort, the bucket accumulation, the
 * bucket weights, the wavefront reduction, the final check) on rows a caller gives, over the group
 * [lo, lo + cnt) of a chunk of n <= 65536 signatures.  A small kernel writes the rows, digits and c
 * into the context's ZIP-215 scratch in the layout the prep kernel writes; the call then runs the
 * same launches on the same scratch as a group of tmed_verify_batch_zip215.
 *
 * points: 2n x 32-byte encodings, the n A rows then the n R rows, decoded permissively (as ZIP-215
 * decodes R: y >= p and x = 0 with the sign bit accepted).  The row of a point P holds -P, as the
 * product's rows hold -A and -R, so window w comes out as sum_i digits[w][i] (-P_i) over the rows
 * lo .. lo + cnt - 1 and n + lo .. n + lo + cnt - 1.  digits: [16][2n] int16, signed radix-2^16
 * digits taken as given: any value in windows 0..14 of an A row, 0..4097 in window 15; the R rows'
 * digits of windows 8..15 are ignored.  c: n x 32 bytes, c_i as 8 little-endian words (the product's
 * z_i S_i mod L).
 *
 * windows: 16 x 40 int32 out, window w's value as the limbs of X, Y, Z, T (10 each, radix 2^25.5)
 * that the final kernel reads; ctot: sum of c_i mod L over the group, 8 words; *flag: 1 when
 * [8](sum_w 2^(16 w) window_w + [ctot] B) is the identity, else 0.
 * TMED_EINVAL: n, lo, cnt out of range, a window-15 A digit outside 0..4097, a row that does not
 * decode.
 */
int tmed_test_zip_msm(tmed_ctx *ctx, uint32_t n, const uint8_t *points, const int16_t *digits, const uint8_t *c,
                      uint32_t lo, uint32_t cnt, int32_t windows[640], uint32_t ctot[8], uint32_t *flag);

/*
 * Tests only (tests/test_gpu_keyed_stages.py): two stages of the key-cached throughput route, run by
 * the product's own launchers on the context's own scratch buffers.
 *
 * tmed_test_key_order: the key-grouped visiting order (csrc/kernels.hip launch_key_order: the
 * counting sort of one chunk's key indexes) of val_idx[0..n), 1 <= n <= 2^20, over a key set of
 * nkeys keys (no key set is needed: only the number counts).  The context's order scratch is sized
 * as a key-cached batch sizes it, its permutation region filled with 0xFFFFFFFF, and the launcher
 * run with index_base.  perm_out: n entries, index_base + i for every i of [0, n), grouped by bin
 * (v >> *shift_out; every v >= nkeys in the last bin).  cursor_out: room for 4096 words; the first
 * *nbins_out hold the scratch words after the scatter, bin b's being the end of bin b in perm_out.
 * TMED_EINVAL: n = 0 or n > 2^20, nkeys = 0 or nkeys > 2^24 (the launcher refuses those),
 * index_base + n past 32 bits.
 *
 * tmed_test_finish: the batched finish (launch_finish, verify_finish_kernel, verify_core.h
 * finish_group) of m <= 2^20 projective points a caller gives.  xyz: m x 30 int32, the limbs of X, Y,
 * Z (10 each, radix 2^25.5) of position p, written into fin slot p in the layout the main kernels
 * write.  r: m x 32 bytes, position p's R, written as the R half of signature row fin_base + p, or
 * perm[fin_base + p] when perm (fin_base + m entries, each below fin_base + m) is not NULL.
 * bits_in: m bytes, the bit `out` holds for position p before the finish.  bits_out: fin_base + m
 * bytes, `out` after the finish: position p's byte is bits_in && Z != 0 && enc(X/Z, Y/Z) == r at
 * that same index; a byte no position owns is 0xAA.
 * TMED_EINVAL: m = 0, m > 2^20, fin_base + m > 2^21, a perm entry out of range.
 *
 * tmed_test_finish_zip215: the same arguments through the ZIP-215 finish (launch_finish_zip,
 * keyset_finish_zip_kernel, zip_finish.h) on the context's own fin buffer: position p's byte is
 * bits_in && Z != 0 && r decodes permissively && [8]((X : Y : Z) - r) is the identity.
 */
int tmed_test_key_order(tmed_ctx *ctx, const uint32_t *val_idx, uint32_t n, uint32_t nkeys, uint32_t index_base,
                        uint32_t *perm_out, uint32_t *cursor_out, uint32_t *nbins_out, uint32_t *shift_out);
int tmed_test_finish(tmed_ctx *ctx, uint32_t m, const int32_t *xyz, const uint8_t *r, const uint32_t *perm,
                     uint32_t fin_base, const uint8_t *bits_in, uint8_t *bits_out);
int tmed_test_finish_zip215(tmed_ctx *ctx, uint32_t m, const int32_t *xyz, const uint8_t *r, const uint32_t *perm,
                            uint32_t fin_base, const uint8_t *bits_in, uint8_t *bits_out);

/*
 * With TMED_DEBUG_ZERO set at the first pipelined generic batch: every staged candidate whose
 * device bit is 0 is recorded (request, signature, staging position, the staged and the device
 * copies of its key and signature, the assembled sign-bytes).  Copies up to cap records into out
 * and removes them; *n = records copied; returns the record size in bytes (tools/stress/c3_stress.py).
 */
int tmed_debug_zero_bits(void *out, size_t cap, size_t *n);

/* ------------------------------------------------------- commit seam (C++) */

/* BlockID as compared by BlockID.Equals (types/block.go:1170-1173). */
typedef struct {
  const uint8_t *hash;
  uint32_t hash_len;
  uint32_t psh_total;
  const uint8_t *psh_hash;
  uint32_t psh_hash_len;
} tmed_block_id;

/* ValidatorSet (types/validator_set.go:51-58), index order = commit order. */
typedef struct {
  size_t n;
  const uint8_t *pubkeys;   /* n x 32 (ed25519 keys; other key types stay on the Go path) */
  const int64_t *powers;    /* n voting powers */
  const uint8_t *addresses; /* n x 20, PubKey.Address(); needed by LightTrusting only (may be NULL otherwise).
                               Every validator address must be 20 bytes (Validator.ValidateBasic,
                               types/validator.go:49): a caller holding another length takes the Go path */
  int64_t total_power;      /* vals.TotalVotingPower() (its panics stay in Go, :298-321) */
  uint64_t keyset;          /* 0 (the context's key-set cache decides, see tmed_keycache_config), or a
                               tmed_keyset_load handle holding these pubkeys (key-cached path) */
  const uint32_t *keyset_index; /* NULL: validator i is key i of the key set; else its index there
                                   (one key set can then serve many validator sets, e.g. the light client) */
  const uint8_t *set_hash;  /* NULL, or ValidatorSet.Hash() of this set (32 bytes, types/validator_set.go:
                               347-353): the key-set cache's key for it (else a digest of the key bytes).
                               Either way a cached set is compared key by key before it is used. */
} tmed_valset;

/* Commit + CommitSigs (types/block.go:575-634, 737-752). */
typedef struct {
  int64_t height;
  int32_t round;
  tmed_block_id block_id;
  size_t n_sigs;
  const uint8_t *flags;       /* BlockIDFlag per signature: 1 Absent, 2 Commit, 3 Nil */
  const uint8_t *addresses;   /* n_sigs x 20 ValidatorAddress (LightTrusting only; may be NULL otherwise) */
  const int64_t *ts_seconds;  /* Timestamp.Unix() */
  const int32_t *ts_nanos;    /* Timestamp.Nanosecond() */
  const uint8_t *sigs;        /* n_sigs x 64 (first sig_lens[i] bytes meaningful) */
  const uint32_t *sig_lens;   /* NULL = all 64 */
  const uint32_t *address_lens; /* NULL = all 20; else len(ValidatorAddress) per signature.  GetByAddress
                                   compares with bytes.Equal (types/validator_set.go:270-277): an address
                                   whose length is not 20 matches no validator, so LightTrusting skips
                                   that signature (its 20-byte slot is then ignored) */
} tmed_commit;

#define TMED_MODE_COMMIT 0         /* ValidatorSet.VerifyCommit              :667-714 */
#define TMED_MODE_LIGHT 1          /* ValidatorSet.VerifyCommitLight         :722-765 */
#define TMED_MODE_LIGHT_TRUSTING 2 /* ValidatorSet.VerifyCommitLightTrusting :775-826 */

typedef struct {
  int mode;
  const char *chain_id;
  uint32_t chain_id_len;
  const tmed_valset *vals;
  const tmed_block_id *block_id; /* COMMIT / LIGHT: expected BlockID */
  int64_t height;                /* COMMIT / LIGHT: expected height */
  const tmed_commit *commit;
  int64_t trust_num, trust_den;  /* LIGHT_TRUSTING: tmmath.Fraction (libs/math/fraction.go:11-18) */
} tmed_commit_request;

/* ------------------------------------------------- key-set cache of the commit seam (f2) */

/*
 * tmed_verify_commits / tmed_blocksync_verify (and their _multi forms) give every validator set
 * that carries no handle (tmed_valset.keyset == 0) to the context's key-set cache, so the
 * reference's callers reach the key-cached kernels without managing handles: LastCommit against
 * LastValidators every block (state/validation.go:93-96), the blocksync window against
 * state.Validators (blockchain/v0/reactor.go:366-367), the light client's trusted / untrusted sets
 * (light/verifier.go:58,73-76).  The cache holds ONE pooled key set per context (a key held by many
 * sets is built once) and an entry per validator set, keyed by set_hash when given, else by a digest
 * of the ordered keys, and compared key by key on every hit.  On a miss: a set whose keys are all in
 * the pool is keyed at once; a call whose own signatures pay for building the missing keys (>= 2048
 * per key: a blocksync window, a light-client batch) builds them first and is keyed; otherwise the
 * call runs the generic kernels and the missing keys are built right after it by a worker thread of
 * the context (off the caller's critical path), so the next call against that set is keyed (C1: the first VerifyCommit after a set change is generic, the rest
 * are cache hits).  Decisions are identical either way.
 *   enabled: 1 on, 0 off (sets without a handle stay generic), -1 unchanged (default on; env
 *            TMED_KEYCACHE=0 turns it off at tmed_init);
 *   budget_bytes: 0 unchanged, else the pool's HBM budget (default 160 GiB, env TMED_KEYCACHE_GB;
 *            ~6.3 MB per key with the radix-2^12 comb): a set that does not fit empties the pool
 *            when no call is using it, else stays generic.
 */
int tmed_keycache_config(tmed_ctx *ctx, int enabled, size_t budget_bytes);
typedef struct {
  uint64_t enabled, budget_bytes;
  uint64_t lookups, hits;                 /* validator-set lookups by seam calls; hits on a cached entry */
  uint64_t keyed_sets, generic_sets;      /* lookups resolved to the key-cached / generic kernels */
  uint64_t keyed_sigs, generic_sigs;      /* signatures of the requests resolved each way */
  uint64_t keys_appended, keys_deferred;  /* keys built into the pool; of those, built after a generic call */
  uint64_t pool_resets, sets_evicted;     /* pool emptied to fit a set; entries dropped (LRU bound) */
  uint64_t pool_keys, pool_capacity_keys, pool_bytes, pool_a_window_bits;
  uint64_t sets_cached, pending_keys;
} tmed_keycache_counters;
int tmed_keycache_stats(tmed_ctx *ctx, tmed_keycache_counters *out);
/* Wait until the keys queued by generic calls are built (the context's build worker is idle and
 * the device has finished): the next call against those sets is keyed.  Tests and benches. */
int tmed_keycache_wait(tmed_ctx *ctx);
/* Drop every cached set and the pool (TMED_EINVAL while a call is using it). */
int tmed_keycache_flush(tmed_ctx *ctx);
/* Build a set's missing keys now (e.g. at a validator-set change, before its first commit), so
 * even its first call is keyed.  TMED_ENOMEM when it does not fit the budget. */
int tmed_keycache_warm(tmed_ctx *ctx, const tmed_valset *vals);

/* Outcome codes: the reference's return value, to be formatted by the caller exactly as Go does. */
#define TMED_COMMIT_OK 0
#define TMED_COMMIT_WRONG_SET_SIZE 1   /* ErrInvalidCommitSignatures{expected, actual} (types/errors.go:32-41) */
#define TMED_COMMIT_WRONG_HEIGHT 2     /* ErrInvalidCommitHeight{expected, actual} (types/errors.go:21-30) */
#define TMED_COMMIT_WRONG_BLOCK_ID 3   /* "invalid commit -- wrong block ID: want %v, got %v" */
#define TMED_COMMIT_WRONG_SIGNATURE 4  /* "wrong signature (#%d): %X" (idx) */
#define TMED_COMMIT_NOT_ENOUGH_POWER 5 /* ErrNotEnoughVotingPowerSigned{got, needed} (:856-863) */
#define TMED_COMMIT_DOUBLE_VOTE 6      /* "double vote from %v (%d and %d)" (val_idx, idx_first, idx) */
#define TMED_COMMIT_ZERO_DENOMINATOR 7 /* "trustLevel has zero Denominator" */
#define TMED_COMMIT_OVERFLOW 8         /* "int64 overflow while calculating voting power needed..." */
#define TMED_COMMIT_PANIC 9            /* the reference loop PANICS when it reaches signature idx: an unknown
                                          BlockIDFlag in VerifyCommit (CommitSig.BlockID, types/block.go:652-665)
                                          or a malformed BlockID hash in the sign-bytes of a Commit-flag vote
                                          (CanonicalizeBlockID, types/canonical.go:18-22).  Every earlier
                                          signature the loop reached was valid.  The caller runs the original
                                          Go method for this request, which panics exactly as before. */

typedef struct {
  int code;
  int64_t got, needed;     /* NOT_ENOUGH_POWER */
  int64_t expected, actual;/* WRONG_SET_SIZE / WRONG_HEIGHT */
  int32_t idx;             /* WRONG_SIGNATURE / PANIC index; DOUBLE_VOTE second index */
  int32_t idx_first;       /* DOUBLE_VOTE first index */
  int32_t val_idx;         /* DOUBLE_VOTE validator index */
  uint32_t verified;       /* signatures sent to the device for this request */
} tmed_commit_result;

/*
 * Verify n commit requests with ONE device batch: run the reference prechecks,
 * collect the signatures each loop would reach (all non-absent for COMMIT; the
 * ForBlock prefix up to the >2/3 (resp. trust-level) crossing for LIGHT /
 * LIGHT_TRUSTING, stopping at a double vote), build their CanonicalVote
 * sign-bytes, verify them on the GPU, then replay each reference loop over the
 * validity bits — same first-error index, same early exit, same Got/Needed.
 * Inputs on which the reference loop panics (unknown BlockIDFlag, malformed BlockID
 * hash) give that request the outcome TMED_COMMIT_PANIC at the index where the loop
 * would panic — only if the loop reaches it; the other requests are unaffected.
 * TMED_EINVAL is reserved for malformed calls (null pointers, unknown mode).
 */
int tmed_verify_commits(tmed_ctx *ctx, const tmed_commit_request *reqs, size_t n, tmed_commit_result *out);

/*
 * The same seam with the batch verifier supplied by the caller (same contract
 * as tmed_verify_batch; return 0 on success).  tmed_verify_commits is this
 * with the context's GPU verifier.  Lets a host integrate its own verifier
 * (e.g. the Go shim's fallback is the original Go method, not this) and lets
 * the CPU test-suite check the plan/replay logic against the oracle.
 */
typedef int (*tmed_batch_verify_fn)(void *user, const uint8_t *pubkeys, const uint8_t *sigs, const uint32_t *sig_lens,
                                    const uint8_t *msgs, const uint32_t *msg_off, size_t n, uint8_t *out_valid);
int tmed_verify_commits_with(const tmed_commit_request *reqs, size_t n, tmed_commit_result *out,
                             tmed_batch_verify_fn verify, void *user);

/*
 * Diagnostics: wall time in microseconds of the three phases of the calling thread's last
 * tmed_verify_commits / tmed_verify_commits_with / tmed_blocksync_verify call — [0] host plan
 * (prechecks, candidate collection), [1] verify (sign-bytes, staging, device, copy back),
 * [2] host replay.  For a call the seam pipelines (large batches: two vote slots), [0] is the
 * host plan + staging time, [1] the time the host is blocked waiting for the device and [2]
 * the host scatter + replay time; [0] and [2] overlap device work there.
 */
int tmed_seam_phase_us(double out_us[3]);

/* ------------------------------------------------ Merkle hashing (f3) */

/*
 * crypto/merkle.HashFromByteSlices (crypto/merkle/tree.go:9-22; RFC-6962 leaf 0x00 /
 * inner 0x01 prefixes, crypto/merkle/hash.go:19-27) for n_trees trees at once: tree t's
 * leaves are leaf indices [tree_off[t], tree_off[t+1]); leaf i is
 * leaves[leaf_off[i] .. leaf_off[i+1]).  roots: n_trees x 32 bytes.  An empty tree's root is
 * SHA-256("") as in the reference.  SHA-256 runs on the device (one lane per leaf, then one
 * launch per tree level across all trees).
 */
int tmed_merkle_roots(tmed_ctx *ctx, const uint8_t *leaves, const uint64_t *leaf_off, const uint32_t *tree_off,
                      size_t n_trees, uint8_t *roots);

/*
 * ValidatorSet.Hash (types/validator_set.go:347-353) for n_sets ed25519 validator sets:
 * set s = validators [set_off[s], set_off[s+1]) in set order; leaves are
 * Validator.Bytes() = SimpleValidator{PubKey ed25519, VotingPower} (types/validator.go:117-133),
 * encoded on the device.  out: n_sets x 32 bytes.
 */
int tmed_valset_hashes(tmed_ctx *ctx, const uint8_t *pubkeys, const int64_t *powers, const uint32_t *set_off,
                       size_t n_sets, uint8_t *out);

/* Header fields hashed by Header.Hash (types/block.go:440-475), in struct order. */
typedef struct {
  uint64_t version_block, version_app;  /* tmversion.Consensus */
  const char *chain_id;
  uint32_t chain_id_len;
  int64_t height;
  int64_t time_seconds;                 /* Time.Unix() */
  int32_t time_nanos;                   /* Time.Nanosecond() */
  tmed_block_id last_block_id;
  /* LastCommitHash, DataHash, ValidatorsHash, NextValidatorsHash, ConsensusHash, AppHash,
     LastResultsHash, EvidenceHash, ProposerAddress */
  const uint8_t *hashes[9];
  uint32_t hash_lens[9];
} tmed_header;

/*
 * Header.Hash for n headers: out[i] (32 bytes) with ok[i] = 1, or ok[i] = 0 (out[i] zeroed) where
 * the reference returns nil (empty ValidatorsHash, :441-443).  A header whose 14 leaves each fit
 * two SHA-256 blocks (chain_id_len <= 50, the reference's MaxChainIDLen, types/genesis.go:21; every
 * hash field and both LastBlockID hashes <= 64 bytes; the LastBlockID leaf <= 118 bytes) is hashed by
 * header_hash_kernel in one launch: 16 lanes per header, lane l encodes leaf l (gogoproto wrappers
 * as cdcEncode, types/encoding_helper.go) in registers from a packed record and the 14-leaf tree is
 * reduced across the lanes.  The limits are the kernel's, not the data's (AppHash may be of any
 * length): any other header of the call has its leaves encoded on the host and hashed by the
 * generic leaf and level kernels.  Results are identical either way.
 */
int tmed_header_hashes(tmed_ctx *ctx, const tmed_header *headers, size_t n, uint8_t *out, uint8_t *ok);

/*
 * PartSet root hash of n_blocks byte strings (NewPartSetFromData, types/part_set.go:166-194):
 * block b = data[data_off[b] .. data_off[b+1]) split into part_size chunks
 * (types.BlockPartSizeBytes = 65536 in the reference); roots: n_blocks x 32 bytes.
 */
int tmed_partset_roots(tmed_ctx *ctx, const uint8_t *data, const uint64_t *data_off, size_t n_blocks,
                       uint32_t part_size, uint8_t *roots);

/*
 * The two other hashes Block.ValidateBasic recomputes for every block (types/block.go:55-106;
 * Evidence.Hash is tmed_evidence_hashes below).
 *
 * tmed_commit_hashes: Commit.Hash() (types/block.go:894-912) for n commits =
 * HashFromByteSlices over cs.ToProto().Marshal() of every CommitSig, encoded on the device from the
 * flat arrays of tmed_commit (height, round and block_id are not hashed).  The CommitSig encoding is
 * the reference's rule as derived from the generated marshaller
 * (proto/tendermint/types/types.pb.go:1563-1596, gogoproto StdTime; fields in ascending order):
 *     08 varint(flag)   only if flag != 0
 *     12 len addr       only if len(addr) > 0
 *     1a len ts         always; ts = [08 varint(uint64(seconds))] if seconds != 0,
 *                                    [10 varint(nanos)] if nanos != 0
 *     22 len sig        only if len(sig) > 0
 * The reference holds no Commit.Hash known answer: the rule is pinned only by its size bound,
 * MaxCommitSigBytes = 109 (types/block.go:591, types/block_test.go:260-274).
 * out: n x 32 bytes.  ok[i] = 0 (out[i] zeroed, the other commits unaffected; the caller runs the Go
 * method) where this struct cannot reproduce the hash: a sig_lens[j] > 64 or an address length
 * other than 0 or 20 (the struct does not carry those bytes), or a timestamp the reference's
 * Marshal rejects, so that Commit.Hash panics (seconds outside [-62135596800, 253402300800), nanos
 * outside [0, 10^9)).  n_sigs == 0 gives SHA-256("") with ok = 1.  TMED_EINVAL: addresses == NULL
 * with an address length of 20, or another array the commit's signatures need is NULL.
 * Submitted blocksync windows are collected first, as by every seam call.
 *
 * tmed_txs_hashes: Data.Hash() = Txs.Hash() (types/block.go:1004-1012 -> types/tx.go:47-55) for
 * n_blocks blocks: block b's transactions are indices [block_off[b], block_off[b+1]), transaction i
 * is txs[tx_off[i] .. tx_off[i+1]); every leaf is SHA-256(tx), hashed on the device.  out:
 * n_blocks x 32 bytes; a block without transactions gives SHA-256("").
 *
 * After either call tmed_last_kernel_ms reports the device time of its leaf kernel.
 */
int tmed_commit_hashes(tmed_ctx *ctx, const tmed_commit *commits, size_t n, uint8_t *out, uint8_t *ok);
int tmed_txs_hashes(tmed_ctx *ctx, const uint8_t *txs, const uint64_t *tx_off, const uint32_t *block_off,
                    size_t n_blocks, uint8_t *out);

/*
 * Merkle proofs: merkle.ProofsFromByteSlices (crypto/merkle/proof.go:35-48, trailsFromByteSlices
 * :216-237) and Proof.Verify (:52-68, computeHashFromAunts :151-181) for many trees per call.
 *
 * The three generators take the inputs of their root call and return, besides roots, every
 * leaf's proof.  L = the call's leaf count; leaf i of the call is leaf (i - first leaf of its tree)
 * of its tree, so Proof.Total and Proof.Index are implied by the tree's leaf count and the leaf's
 * position.
 *   roots        n_trees x 32, as the root call writes them (SHA-256("") for an empty tree, which
 *                has no proofs)
 *   leaf_hashes  L x 32: Proof.LeafHash = leafHash(leaf)
 *   aunt_off     L + 1 entries, in units of hashes: leaf i's aunts are hashes
 *                [aunt_off[i], aunt_off[i+1]) of aunts; a one-leaf tree gives none
 *   aunts        32-byte hashes back to back, each leaf's in Proof.Aunts order (FlattenAunts,
 *                proof.go:197-212): the leaf's sibling first, the root's child last
 *   aunts_cap    bytes available at aunts; *aunts_len receives the bytes needed, 32 * aunt_off[L]
 * Sizing follows tmed_vote_sign_bytes: with aunts == NULL the call fills aunt_off (and part_off)
 * and *aunts_len on the host, touches no device (roots and leaf_hashes may be NULL) and returns
 * TMED_OK (so a full call passes a non-NULL aunts even where no leaf has an aunt); with aunts_cap
 * smaller than the bytes needed it returns TMED_ENOMEM and writes nothing.  TMED_EINVAL as
 * the root calls.  The trees are built level by level as the root calls build them, every level
 * kept; merkle_aunts_kernel then copies each leaf's siblings out.  After a generator
 * tmed_last_kernel_ms reports that kernel's device time.  Submitted blocksync windows are
 * collected first, as by every seam call.
 *
 * tmed_merkle_proofs: ProofsFromByteSlices over byte-slice trees (inputs of tmed_merkle_roots).
 * tmed_partset_proofs: the whole of NewPartSetFromData (types/part_set.go:166-194) for n_blocks
 * byte strings (inputs of tmed_partset_roots): part_off (n_blocks + 1 entries) receives block b's
 * range of leaf indices, [part_off[b], part_off[b+1]); part p of block b is leaf part_off[b] + p
 * and its bytes are the p-th part_size chunk of the block.
 * tmed_txs_proofs: the tree of Txs.Proof (types/tx.go:80-93), whose leaves are SHA-256(tx) (inputs
 * of tmed_txs_hashes); leaf_hashes[i] = leafHash(tx.Hash()).
 */
int tmed_merkle_proofs(tmed_ctx *ctx, const uint8_t *leaves, const uint64_t *leaf_off, const uint32_t *tree_off,
                       size_t n_trees, uint8_t *roots, uint8_t *leaf_hashes, uint64_t *aunt_off, uint8_t *aunts,
                       size_t aunts_cap, size_t *aunts_len);
int tmed_partset_proofs(tmed_ctx *ctx, const uint8_t *data, const uint64_t *data_off, size_t n_blocks,
                        uint32_t part_size, uint8_t *roots, uint32_t *part_off, uint8_t *leaf_hashes,
                        uint64_t *aunt_off, uint8_t *aunts, size_t aunts_cap, size_t *aunts_len);
int tmed_txs_proofs(tmed_ctx *ctx, const uint8_t *txs, const uint64_t *tx_off, const uint32_t *block_off,
                    size_t n_blocks, uint8_t *roots, uint8_t *leaf_hashes, uint64_t *aunt_off, uint8_t *aunts,
                    size_t aunts_cap, size_t *aunts_len);

/* out_code of tmed_merkle_proofs_verify, in the order Proof.Verify checks (proof.go:52-68) */
#define TMED_PROOF_OK 0
#define TMED_PROOF_NEGATIVE_TOTAL 1 /* "proof total must be positive" (Total < 0) */
#define TMED_PROOF_NEGATIVE_INDEX 2 /* "proof index cannot be negative" */
#define TMED_PROOF_LEAF_HASH 3      /* leafHash(leaf) differs from the proof's LeafHash */
#define TMED_PROOF_ROOT_HASH 4      /* the computed root differs, or computeHashFromAunts returns nil */

/*
 * Proof.Verify(rootHash, leaf) for n proofs, one lane each.  Proof i: Total = totals[i], Index =
 * indexes[i], LeafHash = leaf_hashes[32 i ..), Aunts = hashes [aunt_off[i], aunt_off[i+1]) of aunts
 * (units of hashes, as the generators write them); its leaf is leaves[leaf_off[i] .. leaf_off[i+1])
 * and its root is roots[32 r ..) with r = root_of[i] (root_of == NULL: r = i); roots holds n_roots
 * hashes.  out_code[i] is one of TMED_PROOF_*.  TMED_PROOF_ROOT_HASH also covers every case in
 * which computeHashFromAunts returns nil: index >= total, total == 0, or an aunt count other than
 * the path length of (index, total), in which case no aunt is read.  Any aunt count is accepted;
 * Proof.ValidateBasic's limit of 100 aunts (proof.go:16, :108-110) is the caller's check, and a path
 * is at most 63 long.  On a non-zero code the caller runs the Go method for the error's text.
 * TMED_EINVAL for malformed calls only: a NULL array, offsets that decrease, a leaf longer than
 * 2^32 - 65 bytes, a root index >= n_roots.  After the call tmed_last_kernel_ms reports
 * merkle_verify_kernel's device time.
 */
int tmed_merkle_proofs_verify(tmed_ctx *ctx, size_t n, const uint8_t *roots, size_t n_roots, const uint32_t *root_of,
                              const uint8_t *leaves, const uint64_t *leaf_off, const uint8_t *leaf_hashes,
                              const int64_t *totals, const int64_t *indexes, const uint64_t *aunt_off,
                              const uint8_t *aunts, uint8_t *out_code);

/* ------------------------------------------------- light client: light.Verify */

/*
 * light.Verify (light/verifier.go:135-151) for n (trusted, untrusted) pairs in one call: the
 * untrusted headers' Header.Hash (header_hash_kernel), the untrusted sets' ValidatorSet.Hash and
 * the commit checks on the device, then the reference's checks replayed on the host in the
 * reference's order.  One request = the arguments of one light.Verify call.
 */
typedef struct {
  /* trustedHeader: the fields light.Verify reads */
  const char *chain_id;
  uint32_t chain_id_len;
  int64_t trusted_height, trusted_time_seconds; /* Time.Unix() */
  int32_t trusted_time_nanos;                   /* Time.Nanosecond() */
  const uint8_t *trusted_next_vals_hash;        /* trustedHeader.NextValidatorsHash (adjacent only) */
  uint32_t trusted_next_vals_hash_len;
  const tmed_valset *trusted_vals;              /* non-adjacent only (may be NULL for an adjacent pair) */
  /* untrusted SignedHeader + set */
  const tmed_header *header;
  const tmed_commit *commit;
  const tmed_valset *vals;
  uint8_t basic_ok; /* Header.ValidateBasic() == nil && Commit.ValidateBasic() == nil, run by the caller in Go */
  int64_t trusting_period_ns, max_clock_drift_ns, now_seconds; /* time.Duration; now.Unix() */
  int32_t now_nanos;
  int64_t trust_num, trust_den; /* trustLevel */
} tmed_light_request;

/* Outcome codes, numbered in the order the reference checks; the first failing check wins.
 * Adjacent (VerifyAdjacent, verifier.go:93-132) iff header->height == trusted_height + 1, otherwise
 * non-adjacent (VerifyNonAdjacent, :32-79). */
#define TMED_LIGHT_OK 0
#define TMED_LIGHT_OLD_HEADER_EXPIRED 1  /* :46 / :105 HeaderExpired (:207-210): ErrOldHeaderExpired{expired_*, now} */
/* 2..9: ErrInvalidHeader{reason}: verifyNewHeaderAndVals (:153-192) over SignedHeader.ValidateBasic
 * (types/light.go:129-157) */
#define TMED_LIGHT_HEADER_BASIC 2        /* light.go:137-142: basic_ok == 0 (the caller re-runs the Go method for the text) */
#define TMED_LIGHT_WRONG_CHAIN 3         /* light.go:144-146 "header belongs to another chain %q, not %q" */
#define TMED_LIGHT_COMMIT_HEIGHT 4       /* light.go:149-151 "header and commit height mismatch: %d vs %d" */
#define TMED_LIGHT_COMMIT_HEADER_HASH 5  /* light.go:152-154 "commit signs block %X, header is block %X": hash / hash_len */
#define TMED_LIGHT_HEIGHT_NOT_GREATER 6  /* verifier.go:164-168 */
#define TMED_LIGHT_TIME_NOT_AFTER 7      /* verifier.go:170-174 */
#define TMED_LIGHT_TIME_FROM_FUTURE 8    /* verifier.go:176-181 */
#define TMED_LIGHT_VALS_HASH 9           /* verifier.go:183-189: hash = untrustedVals.Hash() */
#define TMED_LIGHT_NEXT_VALS_HASH 10     /* adjacent, verifier.go:117-123: a plain error */
#define TMED_LIGHT_TRUSTING 11           /* non-adjacent, verifier.go:58-66: VerifyCommitLightTrusting failed, its outcome
                                            in `commit`: NOT_ENOUGH_POWER is ErrNewValSetCantBeTrusted{e}, anything else
                                            the bare error */
#define TMED_LIGHT_COMMIT 12             /* verifier.go:73-76 / :126-129: VerifyCommitLight failed, its outcome in
                                            `commit`; the caller wraps it in ErrInvalidHeader */
#define TMED_LIGHT_GO_PATH 13            /* the structs cannot express this request (a time outside the proto Timestamp
                                            range documented at tmed_commit_hashes): the caller runs the Go function;
                                            the other requests are unaffected */

#define TMED_LIGHT_ORDERED 1u /* flags: verify the VerifyCommitLight requests in a second batch, and only for pairs
                                 whose VerifyCommitLightTrusting passed (the reference's note at verifier.go:70-72:
                                 untrustedVals can be made very large).  0: both speculatively in one batch.
                                 Outcomes are identical; only verified_light differs. */

typedef struct {
  int code;
  int adjacent;               /* 1: VerifyAdjacent's path was taken */
  int64_t expired_seconds;    /* OLD_HEADER_EXPIRED: trustedHeader.Time.Add(trustingPeriod) */
  int32_t expired_nanos;
  uint32_t hash_len;          /* COMMIT_HEADER_HASH: 32, or 0 where Header.Hash() is nil; VALS_HASH: 32 */
  uint8_t hash[32];           /* COMMIT_HEADER_HASH: Header.Hash(); VALS_HASH: untrustedVals.Hash() */
  tmed_commit_result commit;  /* TRUSTING / COMMIT: the failing call's result (else zero) */
  uint32_t verified_trusting; /* signatures sent to the verifier for VerifyCommitLightTrusting */
  uint32_t verified_light;    /* ... and for VerifyCommitLight */
} tmed_light_result;

/*
 * Checks of one request, in the reference's order (the first failing one is the outcome):
 * OLD_HEADER_EXPIRED, HEADER_BASIC, WRONG_CHAIN, COMMIT_HEIGHT, COMMIT_HEADER_HASH (a nil Header.Hash
 * compares as empty bytes, as bytes.Equal does), HEIGHT_NOT_GREATER, TIME_NOT_AFTER, TIME_FROM_FUTURE,
 * VALS_HASH, then NEXT_VALS_HASH (adjacent) or TRUSTING (non-adjacent), then COMMIT.  Times are compared
 * as Go's Time.Add / After / Before on (Unix seconds, nanoseconds).
 *
 * Device work of one call: header_hash_kernel over the untrusted headers of the requests that pass
 * the checks before COMMIT_HEADER_HASH; the valset leaf and level kernels over the untrusted sets of
 * the requests that also pass the host-decidable checks after it, each distinct tmed_valset pointer
 * once; then one pass of tmed_verify_commits' plan -> batch -> replay (key-set cache and pipelining
 * included) over two commit requests per non-adjacent pair and one per adjacent pair, for the pairs
 * that passed every earlier check: a request that fails an earlier check sends no signatures.
 * Submitted blocksync windows are collected first, as by every seam call.
 * TMED_EINVAL for malformed calls only (a NULL header, commit or vals, a NULL trusted_vals of a
 * non-adjacent pair, unknown flags).
 *
 * tmed_light_verify_with: the same replay with the hashes and the batch verifier supplied by the
 * caller (the CPU test-suite: the oracle's hashes and verifier): header_hashes n x 32 with header_ok
 * (0 = nil) and vals_hashes n x 32, one entry per request.
 */
int tmed_light_verify(tmed_ctx *ctx, const tmed_light_request *reqs, size_t n, uint32_t flags,
                      tmed_light_result *out);
int tmed_light_verify_with(const tmed_light_request *reqs, size_t n, uint32_t flags, const uint8_t *header_hashes,
                           const uint8_t *header_ok, const uint8_t *vals_hashes, tmed_light_result *out,
                           tmed_batch_verify_fn verify, void *user);

/* ------------------------------------------------- block time: state.MedianTime */

/*
 * state.MedianTime(commit, validators) (state/state.go:268-285) over tmtime.WeightedMedian
 * (types/time/time.go:35-58) for n (commit, validator set) pairs in one call: the value
 * validateBlock compares block.Time with (state/validation.go:123-129) and State.MakeBlock stamps
 * on a proposal (state/state.go:245-250).
 *
 * The rule, per pair:
 *   - signature i enters iff flags[i] != 1 (only commitSig.Absent() is tested, state.go:273: Nil
 *     votes and unknown flag values enter) and GetByAddress(address_i) finds a validator
 *     (state.go:276-278; types/validator_set.go:270-278 compares with bytes.Equal, so an
 *     address_lens[i] other than 20 matches nothing).  The first validator of the set with that
 *     address gives the weight w_i = power.  An address that is not in the set is skipped, one that
 *     occurs twice in the commit enters twice, and n_sigs is never compared with vals->n;
 *   - total = the sum of the entering weights (state.go:279), median = total / 2 (time.go:36);
 *   - the sort key is Time.UnixNano() = ts_seconds * 1e9 + ts_nanos (time.go:46);
 *   - the result is the Time of the smallest entering key t with W(<= t) >= median, W(<= t) being
 *     the sum of the entering weights with key <= t: what the reference's sort and walk
 *     (time.go:38-56) return for non-negative weights, whatever the order inside a group of equal
 *     keys.  With median == 0 that is the smallest entering key.
 * Outcome codes:
 *   TMED_MEDIAN_OK         seconds / nanos hold the median Time (Unix(), Nanosecond())
 *   TMED_MEDIAN_ZERO_TIME  nothing entered: the reference returns time.Time{} (time.go:35 `res`);
 *                          seconds / nanos hold its Unix() = -62135596800 and 0
 *   TMED_MEDIAN_GO_PATH    the rule above does not determine the reference's value: an entering
 *                          timestamp whose UnixNano is not an int64 or whose nanos lie outside
 *                          [0, 10^9), a negative entering weight, or a total past int64.  The caller
 *                          runs MedianTime itself; the other pairs are unaffected
 * entered: the signatures that entered (0 with GO_PATH).  on_device: 1 when the pair's result comes
 * from the kernels, 0 when the library computed it on the host.
 *
 * tmed_median_times stages each commit's flags, addresses and timestamps once and each distinct
 * tmed_valset pointer's addresses and powers once (one copy in), runs one launch per kernel shape
 * and copies the outcomes back (one copy out).  The kernels take a pair iff n_sigs == vals->n and
 * every non-absent signature has a 20-byte address equal to the set's address at the same index,
 * the pairing VerifyCommit requires (types/validator_set.go:667-714): they compare the two address
 * arrays, then select without sorting, a search over the bits of the key with exact int64 weight
 * sums (csrc/median.hip: one wavefront per commit up to 512 signatures, one workgroup per commit
 * above).  Every other pair of the call, a pair of more than 2^24 signatures, and a pair whose set
 * holds an address twice (the first match then need not be the validator at the same index) is
 * computed by the host function below inside the same call; results are identical either way.
 * Submitted blocksync windows are collected first, as by every seam call.  After the call
 * tmed_last_kernel_ms reports the selection kernels' device time.  Of the commit the call reads
 * flags, addresses, address_lens, ts_seconds, ts_nanos and n_sigs; of the set addresses, powers and n.
 * TMED_EINVAL for malformed calls only: a NULL commit or vals, NULL flags, addresses, ts_seconds or
 * ts_nanos with n_sigs > 0, NULL addresses or powers with vals->n > 0.
 *
 * tmed_median_times_host: the same computation with no device and no context (GetByAddress
 * through a hash index of the set, a weighted quickselect over the entering pairs): csrc/median_host.h.
 */
#define TMED_MEDIAN_OK 0
#define TMED_MEDIAN_ZERO_TIME 1
#define TMED_MEDIAN_GO_PATH 2

typedef struct {
  const tmed_commit *commit; /* block.LastCommit */
  const tmed_valset *vals;   /* state.LastValidators */
} tmed_median_request;

typedef struct {
  int code;
  int64_t seconds;  /* median.Unix() */
  int32_t nanos;    /* median.Nanosecond() */
  uint32_t entered;
  uint8_t on_device;
} tmed_median_result;

int tmed_median_times(tmed_ctx *ctx, const tmed_median_request *reqs, size_t n, tmed_median_result *out);
int tmed_median_times_host(const tmed_median_request *reqs, size_t n, tmed_median_result *out);

/* ------------------------------------------------- free-standing votes */

/*
 * Vote.Verify (types/vote.go:147-156) and the checks VoteSet.addVote runs in front of it
 * (types/vote_set.go:156-218) for batches of free-standing votes: a drained peerMsgQueue, the
 * last commit rebuilt by CommitToVoteSet (types/block.go:767), a WAL replay, the two votes of
 * every DuplicateVoteEvidence of a block (evidence/verify.go:211-219).  Unlike a Commit's, these
 * votes share nothing: each carries its own type, height, round, BlockID and timestamp.
 *
 * tmed_votes: n votes as flat arrays (a cgo caller fills them in place).  A hash longer than 32
 * bytes or an address longer than 20 is described by its length alone; the slot's bytes are ignored.
 */
typedef struct {
  size_t n;
  const int32_t *types;            /* SignedMsgType (any int32: the encoding is the reference's for every value) */
  const int64_t *heights;
  const int32_t *rounds;
  const uint8_t *block_hashes;     /* n x 32 */
  const uint32_t *block_hash_lens; /* NULL = all 32; else len(BlockID.Hash) */
  const uint32_t *psh_totals;      /* BlockID.PartSetHeader.Total */
  const uint8_t *psh_hashes;       /* n x 32 */
  const uint32_t *psh_hash_lens;   /* NULL = all 32 */
  const int64_t *ts_seconds;       /* Timestamp.Unix() */
  const int32_t *ts_nanos;         /* Timestamp.Nanosecond() */
  const uint8_t *addresses;        /* n x 20 ValidatorAddress */
  const uint32_t *address_lens;    /* NULL = all 20 */
  const int32_t *validator_indexes;
  const uint8_t *sigs;             /* n x 64 (first sig_lens[i] bytes meaningful) */
  const uint32_t *sig_lens;        /* NULL = all 64 */
} tmed_votes;

#define TMED_VOTES_ADDVOTE 1u /* flags: the checks of VoteSet.addVote (2, 3 and 5 below) in front of Vote.Verify */

typedef struct {
  const char *chain_id;
  uint32_t chain_id_len;
  const tmed_valset *vals;  /* the VoteSet's valSet; keyset 0 = the key-set cache decides, as for commits.
                               `addresses` is read under TMED_VOTES_ADDVOTE only (NULL otherwise); `powers`
                               and `total_power` are not read */
  const tmed_votes *votes;
  uint32_t flags;
  int64_t height;           /* TMED_VOTES_ADDVOTE: voteSet.height, .round, .signedMsgType */
  int32_t round;
  int32_t msg_type;
} tmed_vote_request;

/* One outcome per vote: the FIRST check that fails, in the reference's order. */
#define TMED_VOTE_OK 0
#define TMED_VOTE_INDEX_NEGATIVE 1      /* "index < 0: %w" ErrVoteInvalidValidatorIndex (types/vote_set.go:165-166) */
#define TMED_VOTE_ADDRESS_EMPTY 2       /* ADDVOTE: "empty address: %w" ErrVoteInvalidValidatorAddress (:167-168) */
#define TMED_VOTE_UNEXPECTED_STEP 3     /* ADDVOTE: height, round or type differ from the VoteSet's: ErrVoteUnexpectedStep
                                           (:172-178) */
#define TMED_VOTE_INDEX_NOT_IN_SET 4    /* GetByIndex finds no validator (validator_index >= vals->n):
                                           ErrVoteInvalidValidatorIndex (:181-186) */
#define TMED_VOTE_ADDRESS_NOT_IN_SET 5  /* ADDVOTE: !bytes.Equal(valAddr, lookupAddr), any length but 20 included:
                                           ErrVoteInvalidValidatorAddress (:189-194) */
#define TMED_VOTE_ADDRESS_NOT_OF_KEY 6  /* Vote.Verify: pubKey.Address() = SHA-256(key)[:20] differs from the vote's
                                           address: ErrVoteInvalidValidatorAddress (types/vote.go:148-150,
                                           crypto/ed25519/ed25519.go:136-141) */
#define TMED_VOTE_PANIC 7               /* VoteSignBytes panics: a BlockID hash or part-set hash whose length is
                                           neither 0 nor 32 (CanonicalizeBlockID, types/canonical.go:19-22).  Only
                                           when no earlier check fails; the caller runs the original Go path, which
                                           panics exactly as before */
#define TMED_VOTE_INVALID_SIGNATURE 8   /* ErrVoteInvalidSignature (types/vote.go:152-154); a signature of any length
                                           but 64 included (crypto/ed25519/ed25519.go:150-152) */
#define TMED_VOTE_GO_PATH 9             /* the structs do not determine the reference's outcome: a timestamp outside
                                           google.protobuf.Timestamp's range (seconds in [-62135596800,
                                           253402300800), nanos in [0, 1e9)), which StdTimeMarshal refuses (VoteSignBytes
                                           then panics, types/vote.go:95-98).  Only when no earlier check fails; the
                                           caller runs the original Go path for this vote */

/*
 * codes[k]: the outcome of vote k, request r's votes starting at the sum of the vote counts of the
 * requests before it.  All requests go to the device as ONE batch: vote_prepare_kernel
 * (csrc/votes.hip) runs the checks 1-7 one lane per vote and writes each vote's sign-bytes, the
 * verify kernels of the commit seam (key-cached when the set resolves to a key set, generic
 * otherwise) decide the signatures.  The duplicate lookup of vote_set.go:197-202, between checks 5
 * and 6 in the reference, reads the VoteSet's state: it stays in Go, as do conflicting votes, maj23
 * and addVerifiedVote.  A request whose chain ID is longer than 50 bytes (MaxChainIDLen) has its
 * messages assembled on the host by the same source; decisions are identical.
 * Submitted blocksync windows are collected first, as by every seam call.  After the call
 * tmed_last_kernel_ms reports vote_prepare_kernel's device time plus the verify kernels'.
 * TMED_EINVAL for malformed calls only (a NULL array with n > 0, NULL vals, NULL vals->pubkeys with
 * vals->n > 0, NULL vals->addresses under ADDVOTE, a keyset_index past the key set).
 */
int tmed_verify_votes(tmed_ctx *ctx, const tmed_vote_request *reqs, size_t n_reqs, uint8_t *codes);
/* vote_prepare_kernel's share of tmed_last_kernel_ms after tmed_verify_votes (benches). */
float tmed_votes_last_prepare_ms(tmed_ctx *ctx);

/*
 * Host entries, no device and no context (csrc/votes_host.h over csrc/vote_free.h, the source the
 * kernel compiles):
 * tmed_votes_sign_bytes: VoteSignBytes(chainID, vote) of the n votes, message i at
 *   out[out_off[i] .. out_off[i+1]) (sizing and TMED_ENOMEM as tmed_vote_sign_bytes).  A vote whose
 *   BlockID is malformed encodes nothing (an empty range) and sets malformed[i] = 1; with malformed
 *   NULL such a vote is TMED_EINVAL.
 * tmed_verify_votes_host: the checks in front of the signature for every vote of the requests, lane
 *   by lane: codes[k] = the first failing check, 0 where the signature would decide; msg_lens[k]
 *   (nullable) = the length of the vote's sign-bytes (0 where a check fails); device_route[r]
 *   (nullable) = 1 when tmed_verify_votes assembles request r's messages on the device.
 */
int tmed_votes_sign_bytes(const char *chain_id, uint32_t chain_id_len, const tmed_votes *votes, uint8_t *out,
                          size_t out_cap, uint32_t *out_off, size_t *out_len, uint8_t *malformed);
int tmed_verify_votes_host(const tmed_vote_request *reqs, size_t n_reqs, uint8_t *codes, uint32_t *msg_lens,
                           uint8_t *device_route);

/* ------------------------------------------------- evidence */

/*
 * n DuplicateVoteEvidence (types/evidence.go:35-47) as flat arrays: the shared struct of
 * tmed_verify_duplicate_votes and tmed_evidence_hashes.  A hash longer than 32 bytes, an address
 * longer than 20 or a signature longer than 64 is described by its length alone, as in tmed_votes.
 */
typedef struct {
  size_t n;                          /* evidences */
  tmed_votes votes;                  /* 2n votes: VoteA of evidence i at 2i, VoteB at 2i+1 (votes.n == 2n) */
  const int64_t *total_voting_powers;
  const int64_t *validator_powers;
  const int64_t *ts_seconds;         /* DuplicateVoteEvidence.Timestamp */
  const int32_t *ts_nanos;
} tmed_dup_evidence;

typedef struct {
  const char *chain_id;
  uint32_t chain_id_len;
  const tmed_valset *vals;  /* the set Pool.verify loads for the evidence's height (evidence/verify.go:55-59);
                               `pubkeys`, `addresses`, `powers` and `total_power` are read; keyset 0 = the key-set
                               cache decides, as for votes */
  const tmed_dup_evidence *ev;
} tmed_dup_request;

/* One outcome per evidence: the FIRST check that fails, in the reference's order (evidence/verify.go:162-222). */
#define TMED_DUPVOTE_OK 0
#define TMED_DUPVOTE_NOT_A_VALIDATOR 1    /* "address %X was not a validator at height %d": GetByAddress(VoteA.
                                             ValidatorAddress) finds nobody (:163-166).  The match is the first
                                             validator, in index order, whose address equals it under bytes.Equal
                                             (types/validator_set.go:270-278); a vote address of any length but 20
                                             matches none */
#define TMED_DUPVOTE_HRS_MISMATCH 2       /* "h/r/s does not match": height, round or type differ (:170-176) */
#define TMED_DUPVOTE_ADDRESS_MISMATCH 3   /* "validator addresses do not match": !bytes.Equal(A.addr, B.addr), lengths
                                             included (:179-184) */
#define TMED_DUPVOTE_SAME_BLOCK_ID 4      /* "block IDs are the same (%v) - not a real duplicate vote": BlockID.Equals
                                             (types/block.go:1170-1173): hashes, totals and part-set hashes all equal;
                                             an empty slice equals a nil one (:187-192) */
#define TMED_DUPVOTE_ADDRESS_NOT_OF_KEY 5 /* "address (%X) doesn't match pubkey": SHA-256(found key)[:20] differs from
                                             VoteA's address (:195-199); the set's `addresses` may disagree with its keys */
#define TMED_DUPVOTE_VALIDATOR_POWER 6    /* powers[found] differs from the evidence's ValidatorPower (:202-205) */
#define TMED_DUPVOTE_TOTAL_POWER 7        /* vals->total_power differs from the evidence's TotalVotingPower (:206-209) */
#define TMED_DUPVOTE_PANIC 8              /* VoteSignBytes of the vote now under test panics on a malformed BlockID, as
                                             TMED_VOTE_PANIC; the caller runs the Go path, which panics as before */
#define TMED_DUPVOTE_VOTE_A_SIGNATURE 9   /* "verifying VoteA: %w" ErrVoteInvalidSignature, a length other than 64
                                             included (:214-216) */
#define TMED_DUPVOTE_VOTE_B_SIGNATURE 10  /* "verifying VoteB: %w" (:217-219) */
#define TMED_DUPVOTE_GO_PATH 11           /* the structs do not determine the outcome; the caller runs Go for this
                                             evidence: (a) a vote timestamp StdTimeMarshal refuses, as TMED_VOTE_GO_PATH;
                                             (b) at check 4 BlockID.Equals hangs on a pair of hashes of the same length
                                             above 32, whose bytes are not carried (when another of its three
                                             comparisons is false the answer is "different" and the checks go on) */

/*
 * VerifyDuplicateVote (evidence/verify.go:162-222) for many evidences per call; codes[k]: the outcome
 * of evidence k, request r's evidences starting at the sum of the counts of the requests before it.
 * The reference computes VoteA's sign-bytes, verifies VoteA, then VoteB's and verifies VoteB; so the
 * code is: the first failing check of 1-7 (or GO_PATH at check 4); else VoteA's PANIC / GO_PATH; else 9
 * if VoteA's signature is invalid; else VoteB's PANIC / GO_PATH; else 10; else 0.  Both signatures are
 * checked against the key of the validator GetByAddress found (keyset_index[found] on the keyed
 * route, its 32 bytes on the generic one): the votes' validator_indexes are never used for this.
 * The context's rule (tmed_set_rule) applies, as to every seam call.
 *
 * Device work (csrc/evidence.hip; the checks are csrc/evidence_free.h, compiled by host and device
 * alike): evidence_lookup_kernel (one wavefront per evidence scans the set's addresses; no sort, no
 * host map), evidence_prepare_kernel (one lane per evidence: checks 2-7, the votes' states, both
 * sign-bytes into kVoteSlot slots, both keys), then the unchanged verify kernels over the 2n slots.
 * A request whose chain ID is longer than 50 bytes takes a host route by the same source, as votes
 * do; decisions are identical.  Submitted blocksync windows are collected first.  After the call
 * tmed_last_kernel_ms reports the two new kernels plus the verify kernels;
 * tmed_evidence_kernel_times gives the lookup's (ms[0]) and the prepare kernel's (ms[1]) share.
 * What stays in Go: ValidateBasic (the contract at verify.go:110), the age and time checks, the
 * committed / pending lookups and the duplicate-hash loop of Pool.verify / CheckEvidence.
 * LightClientAttackEvidence has its own call, tmed_verify_light_client_attacks (below).
 * TMED_EINVAL for malformed calls only: a NULL array with n > 0, votes.n != 2n, NULL vals->pubkeys,
 * addresses or powers with vals->n > 0, a keyset_index past the key set.
 */
int tmed_verify_duplicate_votes(tmed_ctx *ctx, const tmed_dup_request *reqs, size_t n_reqs, uint8_t *codes);
int tmed_evidence_kernel_times(tmed_ctx *ctx, float ms[2]);

/*
 * DuplicateVoteEvidence.Hash() = tmhash.Sum(Bytes()) (types/evidence.go:90-103) for every evidence of
 * `ev`, and EvidenceList.Hash() = HashFromByteSlices(evl[i].Bytes()) (:431-442) for n_lists lists.
 * List l's items are items[list_off[l] .. list_off[l+1]): items[k] >= 0 names an evidence of ev;
 * items[k] < 0 names the host-marshalled byte string -1 - items[k] of opaque / opaque_off (string j =
 * opaque[opaque_off[j] .. opaque_off[j+1])): that is how a LightClientAttackEvidence enters a list.
 * ev_hashes: n x 32 (nullable); roots: n_lists x 32; ev_ok: n (nullable); list_ok: n_lists (nullable).
 * ev_ok[i] = 0, with the hash zeroed, where the struct cannot reproduce Bytes(): a hash longer than
 * 32 or an address longer than 20 (bytes not carried), a signature longer than 64, or a timestamp,
 * a vote's or the evidence's, that StdTimeMarshal refuses (Bytes() panics).  list_ok[l] = 0, with the
 * root zeroed, if one of its evidences has ev_ok = 0.  An empty list gives SHA-256("") with list_ok = 1.
 *
 * The Bytes() rule is DERIVED from the generated marshallers (evidence.pb.go:449-497, types.pb.go:
 * 1431-1489, :1153-1171, :1233-1256; csrc/evidence_free.h states it field by field): the reference
 * holds no known answer and no size bound for these bytes (evidence_test.go only round-trips), so
 * unlike CommitSig's 109 the 234-byte Vote and 520-byte evidence bounds are this library's own.
 *
 * Device work: evidence_hash_kernel (one lane per evidence encodes into an LDS slot and hashes it
 * twice: SHA-256(bytes) and the leaf SHA-256(0x00 || bytes)), the byte-slice leaf kernel over the
 * opaque items, a gather into level 0, then the level builder of the other root calls.
 * tmed_last_kernel_ms reports the leaf stage (those three kernels).  TMED_EINVAL: a NULL array that
 * is needed, votes.n != 2n, offsets that decrease, an item naming an evidence >= ev->n.
 */
int tmed_evidence_hashes(tmed_ctx *ctx, const tmed_dup_evidence *ev, const int64_t *items, const uint32_t *list_off,
                         size_t n_lists, const uint8_t *opaque, const uint64_t *opaque_off, uint8_t *ev_hashes,
                         uint8_t *roots, uint8_t *ev_ok, uint8_t *list_ok);

/*
 * Host entries, no device and no context (csrc/evidence_host.h over csrc/evidence_free.h):
 * tmed_evidence_bytes: Bytes() of every evidence, evidence i at out[out_off[i] .. out_off[i+1])
 *   (sizing and TMED_ENOMEM as tmed_vote_sign_bytes).  Where ev_ok would be 0 nothing is encoded (an
 *   empty range) and ok[i] = 0; with ok NULL such an evidence is TMED_EINVAL.
 * tmed_verify_duplicate_votes_host: lane by lane, pre_codes[k] = the first failing check of 1-7 (or
 *   GO_PATH at check 4; 0 where the signatures would decide); vote_states[2k], [2k+1] (nullable) = 0,
 *   PANIC or GO_PATH of VoteA / VoteB; found[k] (nullable) = the validator GetByAddress finds or -1;
 *   msg_lens[2k], [2k+1] (nullable) = the lengths of the sign-bytes (0 where none are made);
 *   device_route[r] (nullable) = 1 when request r's messages are assembled on the device.
 */
int tmed_evidence_bytes(const tmed_dup_evidence *ev, uint8_t *out, size_t out_cap, uint32_t *out_off, size_t *out_len,
                        uint8_t *ok);
int tmed_verify_duplicate_votes_host(const tmed_dup_request *reqs, size_t n_reqs, uint8_t *pre_codes,
                                     uint8_t *vote_states, int32_t *found, uint32_t *msg_lens, uint8_t *device_route);

/* ------------------------------------------------- evidence: light client attacks */

/*
 * The arguments of one VerifyLightClientAttack call (evidence/verify.go:113-154) as existing structs.
 * The chain ID of both commit checks is trusted_header's (:118, :130).
 */
typedef struct {
  /* e.ConflictingBlock */
  const tmed_header *conflicting_header;
  const tmed_commit *conflicting_commit;  /* `addresses` is read (n_sigs x 20; address_lens NULL = all 20) */
  const tmed_valset *conflicting_vals;    /* `addresses` and `powers` are read beside the keys */
  int64_t common_height;                  /* e.CommonHeight: read by Hash() only */
  int64_t total_voting_power;             /* e.TotalVotingPower */
  /* e.ByzantineValidators, the claimed list */
  size_t n_byz;
  uint8_t byz_is_nil;                     /* 1: the slice is nil (a detector-made evidence may hold nil; n_byz must be
                                             0); 0: non-nil, possibly empty: LightClientAttackEvidenceFromProto makes
                                             an empty non-nil slice (types/evidence.go:405) */
  const uint8_t *byz_addresses;           /* n_byz x 20 */
  const uint32_t *byz_address_lens;       /* NULL = all 20; else len(Address) per entry (the 20-byte slot of any
                                             other length is ignored: it equals no validator's) */
  const int64_t *byz_powers;              /* n_byz */
  /* commonHeader, trustedHeader, commonVals */
  int64_t common_header_height;           /* commonHeader.Height */
  const tmed_header *trusted_header;
  const tmed_commit *trusted_commit;      /* trustedHeader.Commit: only round, n_sigs and flags are read */
  const tmed_valset *common_vals;         /* `addresses`, `powers` and `total_power` are read beside the keys */
} tmed_lca_request;

/* What GetByzantineValidators takes the evidence for (types/evidence.go:233-279). */
#define TMED_LCA_LUNATIC 0      /* ConflictingHeaderIsInvalid(trusted.Header) (:285-292): one of ValidatorsHash,
                                   NextValidatorsHash, ConsensusHash, AppHash, LastResultsHash differs under
                                   bytes.Equal (lengths count, nil equals empty) */
#define TMED_LCA_EQUIVOCATION 1 /* otherwise, and trusted_commit->round == conflicting_commit->round (:253) */
#define TMED_LCA_AMNESIA 2      /* otherwise: no validators, a nil list (:275-278) */

#define TMED_BYZ_OK 0
#define TMED_BYZ_PANIC 1 /* the reference panics inside GetByzantineValidators (equivocation only): a non-absent
                            conflicting signature at an index >= trusted_commit->n_sigs (:264, index out of range),
                            or a lookup that finds nobody while the list has >= 2 entries (:269-272: the nil
                            *Validator reaches ValidatorsByVotingPower.Less, which dereferences it; Go 1.18's
                            sort.Sort compares every element at least once for n >= 2) */

typedef struct {
  int kind;       /* TMED_LCA_* */
  int state;      /* TMED_BYZ_* (count is 0 under PANIC) */
  uint32_t count; /* entries written; 0 = the reference returns nil (`var validators []*Validator` never appended to) */
} tmed_byz_result;

/*
 * GetByzantineValidators (types/evidence.go:233-279) for n evidences per call, without a host map and
 * without a host sort.  Request r's list is written to byz[byz_off[r] .. byz_off[r+1]), a range that
 * must hold conflicting_commit->n_sigs entries; out[r].count of them are written, the rest of the
 * range is left as it was.  The entries are validator INDICES, into common_vals for a lunatic attack
 * and into conflicting_vals for an equivocation, in the reference's order.
 *   Lunatic: for each ForBlock signature of the conflicting commit, in commit order,
 *     GetByAddress(sig.ValidatorAddress) in common_vals: the first match in index order; an address
 *     whose address_lens entry is not 20 matches nobody; signatures that find nobody are dropped; a
 *     validator found by two signatures appears twice.
 *   Equivocation: for each i with conflicting sig i not absent and trusted sig i not absent,
 *     GetByAddress(conflicting sig i's address) in conflicting_vals (not vals[i]).  TMED_BYZ_PANIC as
 *     stated above.  A single-entry list whose one lookup found nobody is count 1, entry -1 (the
 *     reference returns a slice holding one nil *Validator).
 *   Order: ValidatorsByVotingPower (types/validator_set.go:906-911): power descending as int64, then
 *     address ascending under bytes.Compare.  On found validators (power, address) determines the
 *     index (the first match wins), so the output is unique although sort.Sort is not stable.
 * Only the round, n_sigs and flags of trusted_commit, the hashes of the two headers and the flags,
 * addresses and address_lens of conflicting_commit are read, besides the two sets' addresses and
 * powers; no signature is.
 *
 * Device work (csrc/lca.hip; the rule is csrc/lca_free.h, compiled by host and device alike):
 * lca_lookup_kernel, one wavefront per candidate signature (the address scan of
 * evidence_lookup_kernel: one routine, two callers), writes the found validator's ordering key;
 * lca_rank_kernel, one lane per candidate, counts the candidates of its request that order before it
 * (ties by commit position, so the ranks are a permutation) over LDS tiles and writes its validator
 * index at its rank.  Nothing is sorted.  Requests of any size mix in one launch.
 * tmed_lca_kernel_times gives the two kernels' times of the context's last call (ms[0] lookup,
 * ms[1] rank), of tmed_byzantine_validators or tmed_verify_light_client_attacks.
 * tmed_byzantine_validators_host: the same rule lane by lane on the host (csrc/lca_host.h), no context.
 * TMED_EINVAL for malformed calls only: a NULL struct or array that is read, n_byz > 0 with
 * byz_is_nil, byz_off not ascending or a range shorter than conflicting_commit->n_sigs.
 */
int tmed_byzantine_validators(tmed_ctx *ctx, const tmed_lca_request *reqs, size_t n, int32_t *byz,
                              const uint64_t *byz_off, tmed_byz_result *out);
int tmed_byzantine_validators_host(const tmed_lca_request *reqs, size_t n, int32_t *byz, const uint64_t *byz_off,
                                   tmed_byz_result *out);
int tmed_lca_kernel_times(tmed_ctx *ctx, float ms[2]);

/* Outcome codes of tmed_verify_light_client_attacks, numbered in the order the reference checks; the
 * first failing check wins. */
#define TMED_LCA_OK 0
#define TMED_LCA_TRUSTING 1          /* verify.go:117-121: common_header_height != conflicting height and
                                        commonVals.VerifyCommitLightTrusting(chain, commit, 1/3) failed, its outcome
                                        in `commit` ("skipping verification of conflicting block failed: %w") */
#define TMED_LCA_NOT_DERIVED 2       /* :124-127: the same heights and ConflictingHeaderIsInvalid(trusted.Header) */
#define TMED_LCA_COMMIT 3            /* :130-133: conflicting_vals.VerifyCommitLight(chain, commit.BlockID,
                                        conflicting height, commit) failed, its outcome in `commit` ("invalid commit
                                        from conflicting block: %w").  The expected BlockID is the commit's own, so
                                        only the height precheck and the loop can fail */
#define TMED_LCA_TOTAL_POWER 4       /* :136-139 (and again :231-234): expected = e.TotalVotingPower, actual =
                                        common_vals->total_power, the order the message prints them in */
#define TMED_LCA_TIME_NOT_VIOLATED 5 /* :142-145: conflicting height > trusted height and
                                        ConflictingBlock.Time.After(trustedHeader.Time) */
#define TMED_LCA_SAME_HASH 6         /* :148-151: bytes.Equal(trustedHeader.Hash(), ConflictingBlock.Hash()); two nil
                                        hashes are equal */
#define TMED_LCA_AMNESIA_HAS_VALIDATORS 7 /* :243-248: the computed list is nil and byz_is_nil == 0; actual = n_byz */
#define TMED_LCA_BYZ_COUNT 8         /* :250-252: expected = the computed count, actual = n_byz */
#define TMED_LCA_BYZ_ADDRESS 9       /* :255-260: !bytes.Equal(claimed[idx].Address, computed[idx].Address), lengths
                                        included; idx, and val_idx = the expected validator's index */
#define TMED_LCA_BYZ_POWER 10        /* :262-267: the powers differ; idx, val_idx, expected = the validator's power,
                                        actual = the claimed one */
#define TMED_LCA_PANIC 11            /* the reference panics; the caller runs Go, which panics as before: a
                                        TMED_COMMIT_PANIC of either commit check (carried in `commit`), a
                                        TMED_BYZ_PANIC, or a computed list of one nil entry against a claimed list of
                                        one entry (:255 dereferences nil; any other claimed count is BYZ_COUNT first) */
#define TMED_LCA_GO_PATH 12          /* a header time outside the range documented at TMED_LIGHT_GO_PATH */

typedef struct {
  int code;
  int kind;                   /* TMED_LCA_LUNATIC / EQUIVOCATION / AMNESIA, whatever the code */
  tmed_commit_result commit;  /* TRUSTING / COMMIT / PANIC of a commit check: the failing call's result (else zero) */
  int64_t expected, actual;   /* TOTAL_POWER, AMNESIA_HAS_VALIDATORS, BYZ_COUNT, BYZ_POWER */
  int32_t idx, val_idx;       /* BYZ_ADDRESS / BYZ_POWER: the list position and the expected validator's index */
  uint32_t n_byz_expected;    /* the computed list's length where it was computed (the byz range holds it) */
  uint32_t verified_trusting; /* signatures sent to the verifier for VerifyCommitLightTrusting */
  uint32_t verified_light;    /* ... and for VerifyCommitLight */
  uint8_t hash[32];           /* LightClientAttackEvidence.Hash() (types/evidence.go:302-309) of every request whose
                                 header hashes were computed (any code but NOT_DERIVED and GO_PATH; else zero) */
} tmed_lca_result;

/*
 * VerifyLightClientAttack (evidence/verify.go:113-154, with validateABCIEvidence :226-271 and
 * GetByzantineValidators) for n evidences in one call, the reference's checks replayed in its order
 * (csrc/lca_host.h).  Request r's computed list is written to byz[byz_off[r] ..) as by
 * tmed_byzantine_validators, for the requests that reach validateABCIEvidence.
 *
 * Hash(): SHA-256 over a buffer of 32 + n bytes, n = the length of binary.PutVarint(CommonHeight), the
 * ZIGZAG varint: the first 31 bytes of the conflicting header's hash (copy(bz[:tmhash.Size-1], ...);
 * a nil header hash leaves 31 zero bytes), byte 31 zero, then the varint.
 *
 * Device work of one call: GO_PATH and NOT_DERIVED are decided on the host first and send nothing to
 * the device; header_hash_kernel over the two headers of every other request; one plan -> batch ->
 * replay pass of the commit seam over the Trusting + Light pair on the one Commit for requests whose
 * heights differ and the Light request alone otherwise (key-set cache, context rule and pipelining as
 * for tmed_verify_commits); then, for the requests still undecided, the two kernels of
 * tmed_byzantine_validators, and lca_hash_kernel (one lane per request) for Hash().  The claimed list
 * is compared on the host.  Submitted blocksync windows are collected first.  flags must be 0.
 * TMED_EINVAL for malformed calls only.
 *
 * tmed_verify_light_client_attacks_with: the same replay with no device: the header hashes
 * (conflicting_* / trusted_*: n x 32 with n ok bytes, 0 = nil) and the batch verifier are the
 * caller's, the lists and Hash() are computed on the host by the same source.
 */
int tmed_verify_light_client_attacks(tmed_ctx *ctx, const tmed_lca_request *reqs, size_t n, uint32_t flags,
                                     int32_t *byz, const uint64_t *byz_off, tmed_lca_result *out);
int tmed_verify_light_client_attacks_with(const tmed_lca_request *reqs, size_t n, uint32_t flags, int32_t *byz,
                                          const uint64_t *byz_off, tmed_lca_result *out,
                                          const uint8_t *conflicting_hashes, const uint8_t *conflicting_ok,
                                          const uint8_t *trusted_hashes, const uint8_t *trusted_ok,
                                          tmed_batch_verify_fn verify, void *user);

/* ------------------------------------------------- block validation: validateBlock */

/*
 * validateBlock (state/validation.go:15-151) with the Block.ValidateBasic it runs first
 * (types/block.go:55-106) for n blocks in one call: what blocksync runs twice per block
 * (blockchain/v0/reactor.go:371 and ApplyBlock, state/execution.go) and consensus on every proposal.
 * (The section stands behind the evidence section, whose tmed_dup_evidence the batch carries.)
 *
 * tmed_block_state: the fields of State that validateBlock reads.
 */
#define TMED_VB_KNOW_APP_HASH 1u
#define TMED_VB_KNOW_CONSENSUS_HASH 2u
#define TMED_VB_KNOW_LAST_RESULTS_HASH 4u
#define TMED_VB_KNOW_VALIDATORS 8u
#define TMED_VB_KNOW_NEXT_VALIDATORS 16u
#define TMED_VB_KNOW_ALL 31u

typedef struct {
  uint64_t version_block, version_app; /* state.Version.Consensus */
  const char *chain_id;
  uint32_t chain_id_len;
  int64_t initial_height, last_block_height;
  tmed_block_id last_block_id;
  int64_t last_block_time_seconds;     /* LastBlockTime.Unix() */
  int32_t last_block_time_nanos;       /* LastBlockTime.Nanosecond() */
  const uint8_t *app_hash;
  uint32_t app_hash_len;
  const uint8_t *consensus_hash;       /* HashConsensusParams(state.ConsensusParams): 32 bytes from the caller (one
                                          SHA-256 of an 18-byte proto) */
  const uint8_t *last_results_hash;
  uint32_t last_results_hash_len;
  const tmed_valset *validators;       /* may be NULL iff TMED_VB_KNOW_VALIDATORS is clear: the proposer lookup is then
                                          skipped with the hash check; `pubkeys`, `powers` and `addresses` are read */
  const tmed_valset *next_validators;  /* may be NULL iff TMED_VB_KNOW_NEXT_VALIDATORS is clear */
  const tmed_valset *last_validators;  /* VerifyCommit and MedianTime of LastCommit: everything tmed_verify_commits
                                          and tmed_median_times read.  May be NULL for a block at the initial height */
  int64_t evidence_max_bytes;          /* state.ConsensusParams.Evidence.MaxBytes */
  /*
   * A mask of TMED_VB_KNOW_*.  AppHash, LastResultsHash, the consensus params and the two validator
   * sets exist only after ApplyBlock of the previous block, so a blocksync window validated ahead of
   * execution does not have them (or has a prediction: a predicted set WITH its bit set is checked
   * against the header's hash like a known one).  A check whose bit is clear is skipped, and the bit
   * is set in the result's `skipped` when the replay reached the check.  THE CALLER'S DUTY: a skipped
   * check is not a passed one.  When code == TMED_VB_OK the caller evaluates the skipped checks in Go
   * before it relies on the block; when code != TMED_VB_OK and a skipped check orders before `code`,
   * the caller evaluates the skipped checks in Go first, since the reference would have reported the
   * first of them that fails.
   */
  uint32_t known;
} tmed_block_state;

#define TMED_VB_LINK_PREV 1u /* request flag, blocks i >= 1 (TMED_EINVAL on block 0): the state's last_block_id.hash,
                                last_block_height and last block time are block i-1's of the same call, not the `state`
                                struct's: the hash is Header.Hash() of block i-1 computed on the device in this call (a
                                nil hash compares as empty bytes), the height and the time are its header's.  The
                                PartSetHeader half of LastBlockID still comes from state->last_block_id (the caller has
                                it from tmed_partset_roots / MakePartSet, reactor.go:359-361).  A failure of request
                                i-1 does not change request i's outcome: the caller stops at the first failure. */

typedef struct {
  const tmed_header *header;
  const tmed_commit *last_commit;  /* may be NULL when commit_basic_ok == 0 (a nil LastCommit); with n_sigs > 0 its
                                      flags, addresses, ts_seconds, ts_nanos and sigs must all be given */
  const tmed_block_state *state;
  int64_t evidence_byte_size;      /* block.Evidence.ByteSize(), computed by the caller */
  uint8_t header_basic_ok;         /* Header.ValidateBasic() == nil, run in Go as basic_ok of tmed_light_request is */
  uint8_t commit_basic_ok;         /* LastCommit != nil && LastCommit.ValidateBasic() == nil */
  int32_t evidence_basic_bad;      /* -1, or the index of the first evidence whose ValidateBasic fails */
  uint32_t flags;                  /* TMED_VB_LINK_PREV */
} tmed_block_request;

/*
 * n blocks.  The transactions are the arrays of tmed_txs_hashes (block b's are [block_off[b],
 * block_off[b+1]); block_off == NULL: no block has transactions).  The evidence is the arrays of
 * tmed_evidence_hashes with list b belonging to block b (list_off == NULL: no block has evidence;
 * `opaque` / `opaque_off` carry LightClientAttackEvidence).
 */
typedef struct {
  size_t n;
  const tmed_block_request *blocks;
  const uint8_t *txs;
  const uint64_t *tx_off;
  const uint32_t *block_off;
  const tmed_dup_evidence *ev;
  const int64_t *items;
  const uint32_t *list_off;
  const uint8_t *opaque;
  const uint64_t *opaque_off;
} tmed_block_batch;

/* Outcome codes, numbered in the order the reference checks; the first failing check wins. */
#define TMED_VB_OK 0
#define TMED_VB_HEADER_BASIC 1          /* types/block.go:63-65 "invalid header: %w": header_basic_ok == 0 (the caller
                                           re-runs the Go method for the text) */
#define TMED_VB_COMMIT_BASIC 2          /* block.go:68-73 "nil LastCommit" / "wrong LastCommit: %v": commit_basic_ok == 0 */
#define TMED_VB_LAST_COMMIT_HASH 3      /* block.go:75-80: hash = LastCommit.Hash() */
#define TMED_VB_DATA_HASH 4             /* block.go:83-89: hash = Data.Hash() */
#define TMED_VB_EVIDENCE_BASIC 5        /* block.go:92-96 "invalid evidence (#%d): %v": idx = evidence_basic_bad */
#define TMED_VB_EVIDENCE_HASH 6         /* block.go:98-103: hash = Evidence.Hash() */
#define TMED_VB_VERSION 7               /* state/validation.go:22-28 */
#define TMED_VB_CHAIN_ID 8              /* :29-34 */
#define TMED_VB_HEIGHT_INITIAL 9        /* :35-38: LastBlockHeight == 0 and Height != InitialHeight */
#define TMED_VB_HEIGHT 10               /* :39-44: LastBlockHeight > 0 and Height != LastBlockHeight + 1 */
#define TMED_VB_LAST_BLOCK_ID 11        /* :46-51: hash / hash_len = the linked request's computed Header.Hash() */
#define TMED_VB_APP_HASH 12             /* :54-59 */
#define TMED_VB_CONSENSUS_HASH 13       /* :60-66 */
#define TMED_VB_LAST_RESULTS_HASH 14    /* :67-72 */
#define TMED_VB_VALIDATORS_HASH 15      /* :73-78: hash = state.Validators.Hash() */
#define TMED_VB_NEXT_VALIDATORS_HASH 16 /* :79-84: hash = state.NextValidators.Hash() */
#define TMED_VB_INITIAL_HAS_SIGS 17     /* :87-90 "initial block can't have LastCommit signatures" */
#define TMED_VB_LAST_COMMIT 18          /* :93-96: state.LastValidators.VerifyCommit failed; its tmed_commit_result in
                                           `commit`, TMED_COMMIT_PANIC included (the caller runs Go, which panics) */
#define TMED_VB_PROPOSER_SIZE 19        /* :102-107: len(ProposerAddress) != 20 */
#define TMED_VB_PROPOSER_UNKNOWN 20     /* :108-112: !state.Validators.HasAddress(ProposerAddress) */
#define TMED_VB_TIME_NOT_AFTER 21       /* :117-122: Height > InitialHeight and !Time.After(LastBlockTime) */
#define TMED_VB_TIME_NOT_MEDIAN 22      /* :123-129: !Time.Equal(MedianTime(LastCommit, LastValidators)); the median in
                                           median_seconds / median_nanos */
#define TMED_VB_TIME_NOT_GENESIS 23     /* :131-138: Height == InitialHeight and !Time.Equal(LastBlockTime) */
#define TMED_VB_HEIGHT_BELOW_INITIAL 24 /* :140-142: the switch's default, reached whatever last_block_height is */
#define TMED_VB_EVIDENCE_OVERFLOW 25    /* :146-148 ErrEvidenceOverflow{evidence_max_bytes, evidence_byte_size} */
#define TMED_VB_GO_PATH 26              /* the structs cannot decide the check the replay has reached: ok = 0 from
                                           Commit.Hash or EvidenceList.Hash (tmed_commit_hashes / tmed_evidence_hashes
                                           say when), TMED_MEDIAN_GO_PATH, or a block time or last block time outside
                                           the proto Timestamp range (documented at tmed_commit_hashes) at the time
                                           checks.  The caller runs the Go function; the other requests are unaffected */

typedef struct {
  int code;
  uint32_t skipped;          /* TMED_VB_KNOW_* bits of the checks the replay reached and skipped */
  uint32_t hash_len;         /* 32 with the hash codes; LAST_BLOCK_ID of a linked request: 32, or 0 for a nil hash */
  uint8_t hash[32];          /* the computed value for LAST_COMMIT_HASH, DATA_HASH, EVIDENCE_HASH, VALIDATORS_HASH,
                                NEXT_VALIDATORS_HASH and (linked) LAST_BLOCK_ID */
  tmed_commit_result commit; /* LAST_COMMIT: the failing VerifyCommit's result (else zero) */
  int64_t median_seconds;    /* TIME_NOT_MEDIAN: MedianTime as (Unix(), Nanosecond()) */
  int32_t median_nanos;
  int32_t idx;               /* EVIDENCE_BASIC: the evidence index */
  int32_t proposer_idx;      /* the first validator of state.Validators with ProposerAddress, where the lookup ran
                                and found one; else -1 */
  uint32_t verified;         /* signatures sent to the verifier for this block's VerifyCommit */
} tmed_block_result;

/*
 * The replay follows validation.go literally (csrc/validate_host.h validate_run), the `switch` on the
 * height included.  Times are compared as Go's After / Equal on (seconds, nanoseconds); bytes.Equal
 * against a header field of another length than the computed hash's is a mismatch.  It runs in two
 * phases, so that a request failing an earlier check sends no signatures:
 *   A  for the requests that pass the two basic checks: Commit.Hash, Data.Hash, EvidenceList.Hash,
 *      Header.Hash (of block i-1 of every linked request i) and ValidatorSet.Hash of the known sets,
 *      each distinct tmed_valset pointer once per call (a linked window over a constant set hashes it
 *      once; tmed_valset.set_hash is a cache key and is never trusted here);
 *   B  for the requests that pass everything through INITIAL_HAS_SIGS: VerifyCommit (the commit seam
 *      in TMED_MODE_COMMIT under the context's rule, key-set cache and pipelining as for
 *      tmed_verify_commits), MedianTime and the proposer lookup.
 *
 * Device work of tmed_validate_blocks: phase A's hashes by the kernels of tmed_commit_hashes,
 * tmed_txs_hashes, tmed_evidence_hashes, tmed_header_hashes and tmed_valset_hashes under ONE hold of
 * the context's lock.  The last commits' flags, addresses, timestamps and signatures are copied to the
 * device once per call, into an arena of their own: the CommitSig leaf kernel reads them there and so
 * do the median kernels of phase B (the verifier keeps its candidate staging: it packs only the
 * signatures the loop reaches, with key references).  Every hash routine leaves its roots on the device
 * as well; block_check_kernel (csrc/validate.hip): one wavefront per block, four blocks per 256-thread
 * workgroup, compares the header's 32-byte fields with those device-resident hashes (48 lanes, one
 * dword each, one ballot) and writes one uint32 mask of mismatches per block, and the same wave runs
 * GetByAddress for ProposerAddress over the set's staged addresses (the scan of
 * evidence_lookup_kernel; each distinct set's addresses staged once).  The decision reads only the
 * masks and the proposer indexes; the computed hashes are also copied back, for the error values.
 * Phase B: the commit seam, then the median kernels over the arena's arrays, for the blocks whose
 * commit verified.  The call takes the context's lock three times, one hold after the other (phase A,
 * the commit seam, the medians), as tmed_light_verify takes its own; another call on the context may
 * run between them (a second tmed_validate_blocks refills the arena: the medians then stage their
 * commits themselves).  Submitted blocksync windows are collected first, as by every seam call.  After
 * the call tmed_last_kernel_ms reports the median kernels' time and tmed_validate_kernel_ms
 * block_check_kernel's.
 * TMED_EINVAL for malformed calls only: a NULL struct or array that is read, TMED_VB_LINK_PREV on
 * block 0, unknown flags or `known` bits, a NULL set whose bit is set, transaction or evidence arrays
 * tmed_txs_hashes / tmed_evidence_hashes would refuse.  Both entries check the same things.
 *
 * tmed_validate_blocks_with: the same replay with no device: every hash (n x 32 each, with n ok
 * bytes where the hash can be nil or undecidable: commit_ok, evidence_ok, header_ok; header_hashes[i]
 * is Header.Hash() of block i, read for block i+1's link), the medians (medians[i] for block i), the
 * proposer lookups (proposer_idx[i], -1 for nobody) and the batch verifier are the caller's; the
 * compares block_check_kernel makes run on the host.  The CPU test-suite drives it with the oracle.
 */
int tmed_validate_blocks(tmed_ctx *ctx, const tmed_block_batch *batch, tmed_block_result *out);
int tmed_validate_blocks_with(const tmed_block_batch *batch, tmed_block_result *out, const uint8_t *commit_hashes,
                              const uint8_t *commit_ok, const uint8_t *data_hashes, const uint8_t *evidence_hashes,
                              const uint8_t *evidence_ok, const uint8_t *header_hashes, const uint8_t *header_ok,
                              const uint8_t *validators_hashes, const uint8_t *next_validators_hashes,
                              const tmed_median_result *medians, const int32_t *proposer_idx,
                              tmed_batch_verify_fn verify, void *user);
/* block_check_kernel's device time (ms) in the context's last tmed_validate_blocks. */
float tmed_validate_kernel_ms(tmed_ctx *ctx);
/* Counters of the context's last tmed_validate_blocks: out[0] the validator sets whose ValidatorSet.Hash
 * was computed (distinct tmed_valset pointers), out[1] the sets whose addresses were staged for the
 * proposer lookup, out[2] the blocks block_check_kernel took. */
int tmed_validate_stats(tmed_ctx *ctx, uint64_t out[3]);

/* ------------------------------------------------- blocksync replay (f4) */

/*
 * A window of blocks for the blocksync reactor: for each block h of the
 * window, the reactor's check  state.Validators.VerifyCommitLight(chainID, firstID,
 * first.Height, second.LastCommit)  (blockchain/v0/reactor.go:366-367, with first/second
 * from pool.PeekTwoBlocks, pool.go:193-205).  All blocks of a window are verified against
 * the same validator set (the state's set, predicted for the window; the reactor confirms
 * ValidatorsHash as it applies each block and re-verifies from there if the set changed).
 */
typedef struct {
  const char *chain_id;
  uint32_t chain_id_len;
  const tmed_valset *vals;          /* use a key-set handle for the key-cached kernels */
  size_t n_blocks;
  const tmed_block_id *block_ids;   /* firstID of each block */
  const int64_t *heights;           /* first.Height */
  const tmed_commit *commits;       /* second.LastCommit */
} tmed_blocksync_window;

/*
 * out[h] = the VerifyCommitLight outcome for block h — identical to tmed_verify_commits
 * over TMED_MODE_LIGHT requests — computed speculatively for the whole window, so the
 * caller applies blocks in order and stops at the first non-OK one (the reactor then
 * redoes that request, reactor.go:368-388).  The window is processed in device batches
 * of batch_blocks blocks (0 = 128, the measured best) through a pipeline of up to three batches:
 * while the device verifies batch b, the host plans and stages batch b+1 and replays batch b-2.
 */
int tmed_blocksync_verify(tmed_ctx *ctx, const tmed_blocksync_window *w, uint32_t batch_blocks,
                          tmed_commit_result *out);

/*
 * The same as a stream of windows: a replay that verifies its backlog window after window
 * (blockchain/v0/reactor.go:349-418 over the pool's pending blocks, pool.go:31-34) submits window
 * w+1 before it consumes window w.  tmed_blocksync_submit queues the window's batches behind the
 * context's batches in flight and returns once the results of every EARLIER submitted window are
 * final in their `out` arrays; the window's own last batches may still be in flight, so the device
 * is never drained between windows (a call per window drains the pipeline and refills it: the
 * first batch's planning and copy-in).  tmed_blocksync_wait collects everything submitted and
 * returns the first error of any submitted window (or TMED_OK).  Until the window's results are
 * final, `out` and the memory the window's structs point to (block hashes, the commits' arrays —
 * signatures in pinned memory are DMA'd from there — and the set's keys, powers and addresses)
 * must stay valid and unchanged; the structs themselves (the window, its block_ids / heights /
 * commits arrays, the tmed_valset, the chain ID) are copied by submit.  Any other seam call on the context
 * (tmed_verify_commits, tmed_blocksync_verify) first collects every submitted window.
 * Results are identical to tmed_blocksync_verify on each window.
 */
int tmed_blocksync_submit(tmed_ctx *ctx, const tmed_blocksync_window *w, uint32_t batch_blocks,
                          tmed_commit_result *out);
int tmed_blocksync_wait(tmed_ctx *ctx);

/*
 * Pinned (page-locked) host memory for the commit arrays a caller marshals its commits into
 * (the Go shim flattens every Commit into sigs / flags / timestamps arrays anyway).  When a
 * candidate run's signatures lie in such memory, a large seam batch (tmed_blocksync_verify,
 * tmed_verify_commits) DMAs them straight from the caller's array to the device instead of
 * copying them through the library's pinned staging area first: one pass over host memory
 * instead of three (read, staging write, DMA read) for 64 of the 85 bytes staged per vote.
 * Decisions are identical either way.  tmed_host_alloc: hipHostMalloc'd memory (*p, freed with
 * tmed_host_free); tmed_host_register: page-lock existing memory (hipHostRegister; undo with
 * tmed_host_unregister before freeing it).  Process-wide, any context.
 */
int tmed_host_alloc(size_t bytes, void **p);
int tmed_host_free(void *p);
int tmed_host_register(void *p, size_t bytes);
int tmed_host_unregister(void *p);

/* ------------------------------------------ several GPUs in ONE process (§8e) */

/*
 * A Tendermint node is one process: with one context per GPU (tmed_init(0..N-1)), these
 * split the work into contiguous shards balanced by signature count, run every shard on
 * its own context concurrently, and write each result in place — no collective is needed
 * because the host memory is shared.  Results are identical to the single-context calls.
 * A key-set handle in a request must be loaded on EVERY context under the same handle
 * value (load the set on each context in the same order).  Returns the first error.
 */
int tmed_verify_commits_multi(tmed_ctx *const *ctxs, size_t n_ctx, const tmed_commit_request *reqs, size_t n,
                              tmed_commit_result *out);
int tmed_blocksync_verify_multi(tmed_ctx *const *ctxs, size_t n_ctx, const tmed_blocksync_window *w,
                                uint32_t batch_blocks, tmed_commit_result *out);

#ifdef __cplusplus
}
#endif
#endif /* TMED25519_H */
