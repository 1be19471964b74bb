/* bfhip — C ABI of the MI355X-native Circle-STARK prover backend for the Brainfuck zkVM.
 *
 * This is the drop-in boundary: every entry point replaces one operation of stwo's backend trait surface
 * (`Backend = ColumnOps + FieldOps + PolyOps + QuotientOps + FriOps + AccumulationOps` + `MerkleOps<H>` + `GrindOps<C>`)
 * which the reference fixes to `SimdBackend` at crates/brainfuck_prover/src/brainfuck_air/mod.rs:56,399,480,486-487,497,732 and
 * crates/brainfuck_prover/src/components/mod.rs:42. A Rust `HipBackend` binds these with `extern "C"`.
 *
 * Conventions
 *  - every function returns int32 status: 0 = ok, <0 = error (bfhip_last_error() gives the text); no exceptions cross the boundary.
 *  - `*_d` pointers are device pointers obtained from bfhip_malloc; `*_h` are host pointers borrowed for the call only.
 *  - M31 values are canonical u32 in [0, 2^31-1); QM31 values are 4 x u32; secure columns are 4 separate u32 columns (SoA).
 *  - columns are in bit-reversed circle-domain order, exactly like stwo's CircleEvaluation<_, _, BitReversedOrder>.
 *  - one ctx = one GPU + one HIP stream; calls on a ctx are serial; distinct ctxs may be driven from distinct threads.
 */
#ifndef BFHIP_H
#define BFHIP_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bfhip_ctx bfhip_ctx;
typedef struct bfhip_trace bfhip_trace;

/* Byte-level conventions of the un-vendored stwo-prover @ 31e8dbc (Cargo.toml:41) that cannot be confirmed offline (SURVEY.md Appendix B.2;
 * DESIGN.md section 6 lists every such point). Each is one named switch so that a comparison against a real stwo proof can flip one at a
 * time. The zero value of every field is the default = the published stwo code of that period to the best of our reconstruction.
 *  merkle_node_hash  Blake2sMerkleHasher::hash_node (core/vcs/blake2_merkle.rs), used by Blake2sMerkleChannel (mod.rs:56,486-487):
 *      BFHIP_MERKLE_STWO_COMPRESS  state = 0^32; if children: state = compress(state, left || right, 0,0,0,0); then for the column values
 *                                  in zero-padded chunks of 16 words: state = compress(state, chunk, 0,0,0,0). No parameter block, byte
 *                                  counter or final flag (blake2s_ref::compress is the bare RFC 7693 F function).
 *      BFHIP_MERKLE_RFC7693        node = Blake2s-256(left || right || LE u32 values), the standard hash of the same byte string.
 *  mix_u64           Blake2sChannel::mix_u64 (core/channel/blake2s.rs), used for the claim (components/mod.rs:133) and the proof of work:
 *      BFHIP_MIX_U64_COMPRESS      digest = compress(digest words, [n_lo, n_hi, 0 x 14], 0,0,0,0) — what SimdBackend's grind searches.
 *      BFHIP_MIX_U64_HASH          digest = Blake2s-256(digest || LE64(n) zero padded to 32 bytes) (form of older revisions).
 *  logup_mask_order  mask offsets of each component's last logUp column in LogupAtRow::finalize (reached from finalize_logup(),
 *                    e.g. components/memory/component.rs:133): BFHIP_LOGUP_MASK_CUR_PREV = [0, -1], BFHIP_LOGUP_MASK_PREV_CUR = [-1, 0].
 *                    Changes the order of those columns' two sampled values (and with it the transcript). */
enum { BFHIP_MERKLE_STWO_COMPRESS = 0, BFHIP_MERKLE_RFC7693 = 1 };
enum { BFHIP_MIX_U64_COMPRESS = 0, BFHIP_MIX_U64_HASH = 1 };
enum { BFHIP_LOGUP_MASK_CUR_PREV = 0, BFHIP_LOGUP_MASK_PREV_CUR = 1 };
/* merkle_channel is not a convention but the protocol variant, carried in the same struct so that it reaches prover and verifier alike:
 *      BFHIP_CHANNEL_BLAKE2S      Blake2sMerkleChannel — what the reference instantiates (mod.rs:56,486-487). Default.
 *      BFHIP_CHANNEL_POSEIDON252  Poseidon252MerkleChannel (BASELINE.json config 5; an upstream stwo capability over starknet-crypto 0.6.2,
 *                                 Cargo.lock:821-864, which the reference never instantiates): Poseidon252MerkleHasher nodes, Poseidon252Channel
 *                                 transcript, felt252 hashes serialised as "0x.." hex strings. merkle_node_hash and mix_u64 do not apply. */
enum { BFHIP_CHANNEL_BLAKE2S = 0, BFHIP_CHANNEL_POSEIDON252 = 1 };
typedef struct bfhip_conventions {
    uint32_t merkle_node_hash;
    uint32_t mix_u64;
    uint32_t logup_mask_order;
    uint32_t merkle_channel;
    uint32_t reserved[4];   /* must be zero */
} bfhip_conventions;

const char* bfhip_last_error(void);
/* Number of visible HIP devices (0 when there is no GPU). */
int32_t bfhip_device_count(void);
/* hipMemGetInfo of one device: bytes free right now and in total (either pointer may be NULL). What a caller sizes a pool with, and what
 * the leak test of a failed bfhip_ctx_create compares before / after. */
int32_t bfhip_device_memory(int32_t device_id, uint64_t* free_bytes, uint64_t* total_bytes);

/* Context: owns the stream, the twiddle tree and scratch memory.
 * max_log_domain = log2 of the largest evaluation domain that will be used (reference: LOG_MAX_ROWS + log_blowup + 1 = 26, since
 * SimdBackend::precompute_twiddles(CanonicCoset::new(LOG_MAX_ROWS + log_blowup + 2).circle_domain().half_coset), mod.rs:480-484).
 * Range [6, 29]: columns of up to 2^29 cells (LOG_MAX_ROWS <= 27). */
/* A context owns a main HIP stream, creates its side stream at its first proof (the preprocessed commitment runs there) and two partner streams on
 * demand (bfhip_ctx_set_overlap, shard groups). HIP gives every stream one of GPU_MAX_HW_QUEUES (default 4) hardware queues at creation; with two
 * streams per context up to four proofs in flight per process need no setting (profiles/r05_inflight_history.txt). Several proofs in flight on one GPU:
 * a pool (bfhip_pool_create below) behind one caller thread, or one context and one host thread each.
 * A creation that fails (no device, out of memory at the twiddle tree, ...) releases everything it had allocated. */
int32_t bfhip_ctx_create(int32_t device_id, uint32_t max_log_domain, bfhip_ctx** out);
int32_t bfhip_ctx_destroy(bfhip_ctx* ctx);
int32_t bfhip_ctx_sync(bfhip_ctx* ctx);
/* Intra-proof overlap on the context's partner streams (events only, bytes unchanged); default 0 = off. bit 1: the FRI first-layer tree is
 * hashed level by level behind the quotient launches (compute_fri_quotients inside mod.rs:732); bit 0: the Merkle layers of a tree's largest
 * columns are hashed while its smaller columns are still being transformed (tree_builder.commit, mod.rs:500,583,723). Both pairs of kernels
 * are VALU-limited on gfx950 and stretch each other when they co-run: measured gain 0-0.3 ms of 31 (profiles/r03_overlap_ab*.txt).
 * bit 2 (shard groups only): the column -> row send-receive of a tree's largest size class is issued on the partner stream and overlaps the
 * transforms of the tree's smaller columns; the rest follows in a second send-receive on the same stream (every rank of the group must use
 * the same mask: it changes the number of collectives). A context that never called this function (and was not created under BFHIP_OVERLAP)
 * behaves as if bit 2 were set while it is a member of a group whose ranks sit on DIFFERENT GPUs (RCCL groups; in-process groups over several
 * devices from their second collective on): there the exchange is an xGMI transfer. Calling it with bit 2 clear switches that default off.
 * Unmeasured on multi-GPU hardware. */
int32_t bfhip_ctx_set_overlap(bfhip_ctx* ctx, uint32_t mask);
/* Device memory of this context in bytes: out[0] = reserved by its per-proof arena (1 GiB chunks, kept until the context is destroyed),
 * out[1] = the arena's high-water mark over all proofs so far, out[2] = twiddle tree + inverse, out[3] = arena bytes in use now. */
int32_t bfhip_ctx_memory(bfhip_ctx* ctx, uint64_t out[4]);
/* The scratch reserve. Call-scoped device memory outside the arena — the driver's buffer of bfhip_air_prove, the scan buffers of
 * bfhip_logup_program_generate_batch, the staging of bfhip_air_compose and of the other generic entry points — is by default one
 * hipMalloc on entry and one hipFree on exit per call, and hipFree waits for the WHOLE device, not for one stream: with k proofs in flight
 * on one GPU every proof would stall on the others' kernels. bfhip_ctx_set_scratch_reserve makes ONE hipMalloc of `bytes`, kept until it
 * is set again or the context is destroyed; a call-scoped request is then placed in it when it fits behind what is in use (256-byte
 * aligned) and goes to hipMalloc exactly as before when it does not. The scopes of one context nest, so the reserve is a stack: a scope
 * rewinds to where it found it, behind the same wait for the context's stream as before. Results are the same bytes either way.
 * bytes = 0: no reserve, the default. Refused (-1) while a commitment-scheme session is open on the context; a failed allocation is -1 and
 * leaves the context without a reserve.
 * bfhip_ctx_scratch_stats: out[0] = the reserve's bytes, out[1] = the high-water mark of its use since it was set — what a caller sizes
 * the reserve by: set a generous one, run the largest shape, read the mark —, out[2] = the device allocations made by call-scoped scopes
 * since the context was created, out[3] = the requests served from a reserve since the context was created. */
int32_t bfhip_ctx_set_scratch_reserve(bfhip_ctx* ctx, uint64_t bytes);
int32_t bfhip_ctx_scratch_stats(bfhip_ctx* ctx, uint64_t out[4]);
/* Host waits of this context: 0 (default) = poll briefly, then yield / block; 1 = hipStreamSynchronize at once (hosts with more waiting
 * contexts than cores). Waits inside a shard group are always bounded polls (BFHIP_COMM_TIMEOUT_S, default 300 s).
 * Mailboxes (small proofs, LOG_MAX_ROWS <= 21: the launches behind a Fiat-Shamir point are enqueued before the host knows the challenge and a
 * one-workgroup kernel waits on the GPU for the host's post) are OFF by default under policy 1 — the kernel would spin at the head of a
 * hardware queue while the host thread sleeps. Where they are on (policy 0, or forced with BFHIP_MAILBOX=1), a host thread that is stalled for
 * longer than BFHIP_MAILBOX_TIMEOUT_MS (default 10 000 ms: SIGSTOP, a debugger, heavy oversubscription) makes that proof FAIL with a
 * "mailbox kernel gave up waiting for the host" error instead of merely being slow; the context stays usable and the next proof starts
 * clean. At most one proof per GPU of a process runs in the mailbox order at a time (two could block each other through a shared hardware queue): with several
 * proofs in flight the others keep the plain order. BFHIP_MAILBOX=0 switches them off altogether. All members of a group must use the same overlap mask (bfhip_ctx_set_overlap). */
int32_t bfhip_ctx_set_sync_policy(bfhip_ctx* ctx, int32_t blocking);
/* Mailbox settings of a live context (what BFHIP_MAILBOX / BFHIP_MAILBOX_TIMEOUT_MS set at creation):
 * mode -2 = keep the current mode, -1 = automatic (see above), 0 = off, 1 = on; timeout_ms 0 = keep the current timeout; test_delay_ms: the
 * host sleeps that long before every post — a test hook that exists only in the test-hooks build of the library (libbfhip_testhooks.so,
 * -DBFHIP_TEST_HOOKS: there BFHIP_MAILBOX_TEST_DELAY_MS presets it); the default build accepts <= 0 (no delay) and rejects anything else.
 * Takes effect at the next proof. */
int32_t bfhip_ctx_set_mailbox(bfhip_ctx* ctx, int32_t mode, uint32_t timeout_ms, int32_t test_delay_ms);

/* Conventions used by every operation of this context (prover, bfhip_merkle_commit_layer, bfhip_grind). conv == NULL restores the defaults. */
int32_t bfhip_ctx_set_conventions(bfhip_ctx* ctx, const bfhip_conventions* conv);
int32_t bfhip_ctx_get_conventions(bfhip_ctx* ctx, bfhip_conventions* out);

/* PcsConfig of the commitment scheme (stwo's `PcsConfig { pow_bits, fri_config: FriConfig { log_last_layer_degree_bound, log_blowup_factor,
 * n_queries } }`): what CommitmentSchemeProver::new(config, ..) and CommitmentSchemeVerifier::new(config) take. Conjectured security in bits:
 * pow_bits + log_blowup_factor x n_queries (the default's 5 + 1 x 3 = 8 bits only shows that the pipeline works).
 * The proof JSON does not carry the config (the reference's has no field for it either): a verifier must be given the config the proof was
 * made with, and a proof checked under any other config is rejected.
 * Accepted values (anything else is rejected with -1 and a message in bfhip_last_error()):
 *   pow_bits                     <= 32
 *   log_blowup_factor            1 <= b <= 16 (stwo's FriConfig range); every column domain must stay within the M31 circle: a proof needs
 *                                log_max_rows + b + 1 <= 30 (the verifier rejects anything larger, the prover's twiddle tree stops at 2^29)
 *   log_last_layer_degree_bound  0 only
 *   n_queries                    1 <= q <= 256 (BFHIP_MAX_QUERIES)
 *   reserved                     all zero
 * A Poseidon252-channel proof (bfhip_conventions.merkle_channel = 1) with pow_bits > 12 is refused when the proof starts: that channel's nonce
 * search runs on the host. A context in a shard group keeps the default config (set refuses, and joining refuses a context that has another). */
enum { BFHIP_MAX_QUERIES = 256, BFHIP_MAX_LOG_BLOWUP = 16, BFHIP_MAX_POW_BITS = 32 };
typedef struct bfhip_pcs_config {
    uint32_t pow_bits;                    /* PcsConfig::pow_bits                      default 5 */
    uint32_t log_blowup_factor;           /* FriConfig::log_blowup_factor             default 1 */
    uint32_t log_last_layer_degree_bound; /* FriConfig::log_last_layer_degree_bound   default 0 (only 0 supported) */
    uint32_t n_queries;                   /* FriConfig::n_queries                     default 3 */
    uint32_t reserved[4];                 /* must be zero */
} bfhip_pcs_config;
/* The config of every later proof of this context (pcs == NULL: the defaults). A context proving under log_blowup_factor b needs
 * max_log_domain >= log_max_rows + b + 1 (bfhip_ctx_create); the proof names the size it needs otherwise. */
int32_t bfhip_ctx_set_pcs_config(bfhip_ctx* ctx, const bfhip_pcs_config* pcs);
int32_t bfhip_ctx_get_pcs_config(bfhip_ctx* ctx, bfhip_pcs_config* out);

/* Device buffers (ColumnOps storage: BaseColumn / SecureColumnByCoords live in HBM behind these). */
int32_t bfhip_malloc(bfhip_ctx* ctx, size_t bytes, void** out_d);
int32_t bfhip_free(bfhip_ctx* ctx, void* ptr_d);
int32_t bfhip_upload(bfhip_ctx* ctx, void* dst_d, const void* src_h, size_t bytes);
int32_t bfhip_download(bfhip_ctx* ctx, void* dst_h, const void* src_d, size_t bytes);
int32_t bfhip_memset_zero(bfhip_ctx* ctx, void* dst_d, size_t bytes);

/* PolyOps::precompute_twiddles — done once in bfhip_ctx_create; this returns the device buffers (layered like stwo's TwiddleTree
 * rooted at Coset::half_odds(max_log_domain - 1)): 2^(max_log_domain-1) u32 each. */
int32_t bfhip_twiddles(bfhip_ctx* ctx, const uint32_t** tw_d, const uint32_t** itw_d, uint32_t* root_log);

/* PolyOps::interpolate_columns (tree_builder.extend_evals, mod.rs:497,550-562,690-702): n_cols evaluations of 2^log_size cells on
 * CanonicCoset(log_size).circle_domain() -> coefficients of the same size. cols_h = host array of device pointers. In place when
 * dst == src. replicated != 0: the columns hold one value per *table row* (2^(log_size-4) cells) standing for a column whose
 * values are broadcast 16x (memory/table.rs:95-104); the output then holds the 2^(log_size-4) coefficients of index = 0 mod 16
 * (all other coefficients of such a column are zero). */
int32_t bfhip_interpolate(bfhip_ctx* ctx, uint32_t* const* src_cols_h, uint32_t* const* dst_cols_h, uint32_t n_cols, uint32_t log_size, int32_t replicated);
/* PolyOps::evaluate_polynomials (tree_builder.commit -> LDE, mod.rs:500,583,723): coefficients of 2^log_size -> evaluations on
 * CanonicCoset(log_eval).circle_domain(), log_eval >= log_size. replicated as above (output is row-granular, 2^(log_eval-4) cells). */
int32_t bfhip_evaluate(bfhip_ctx* ctx, uint32_t* const* coeff_cols_h, uint32_t* const* dst_cols_h, uint32_t n_cols, uint32_t log_size, uint32_t log_eval, int32_t replicated);

/* gen_is_first::<B>(log_size) followed by interpolate (mod.rs:497 `tree_builder.extend_evals(gen_is_first(..))`, one call per
 * log_size in log_min..=log_max): the coefficients of the indicator of cell 0, written in closed form by ONE launch (no transform).
 * dst_cols_h[n - log_min] = device pointer to 2^n words, or NULL to skip that size. 4 <= log_min <= log_max < log_min + 28. */
int32_t bfhip_is_first_coeffs(bfhip_ctx* ctx, uint32_t log_min, uint32_t log_max, uint32_t* const* dst_cols_h);
/* The same columns committed (tree_builder.commit -> LDE, mod.rs:500): the evaluations of IsFirst(n) on CanonicCoset(n + log_blowup).circle_domain()
 * for n = log_min..=log_max, written in closed form by ONE launch — word for word what bfhip_is_first_coeffs followed by bfhip_evaluate leaves, with
 * neither coefficients nor transforms. dst_cols_h[n - log_min] = device pointer to 2^(n + log_blowup) words, or NULL to skip that size.
 * 4 <= log_min <= log_max < log_min + 28, log_max + log_blowup within the context's twiddle tree. */
int32_t bfhip_is_first_lde(bfhip_ctx* ctx, uint32_t log_min, uint32_t log_max, uint32_t log_blowup, uint32_t* const* dst_cols_h);
/* PolyOps::eval_at_point of IsFirst(log_size) in closed form (no coefficients): what bfhip_eval_at_point returns for the column bfhip_is_first_coeffs
 * writes. point_h = x then y (u32[8]), out_h = u32[4]. 4 <= log_size <= 31, within the context's twiddle tree. */
int32_t bfhip_is_first_eval_at_point(bfhip_ctx* ctx, uint32_t log_size, const uint32_t point_h[8], uint32_t out_h[4]);

/* ---- single backend operations (each is what one stwo trait method would call; all reached from mod.rs:732 prover::prove unless noted) ----
 * A secure (QM31) column is passed as 4 coordinate pointers. Values/points passed from the host are u32[4] per QM31. */

/* The 16-lane broadcast of `trace_evaluation` (memory/table.rs:95-104: trace[col].data[row] = value.into()): dst[16 r + l] = rows[r].
 * Only for callers that want the full-size column; the prover itself keeps such columns row-granular. */
int32_t bfhip_broadcast16(bfhip_ctx* ctx, const uint32_t* rows_d, uint32_t* dst_d, size_t n_rows);
/* ColumnOps::bit_reverse_column: dst[bit_reverse(i)] = src[i] (out of place), 2^log_size cells. */
int32_t bfhip_bit_reverse(bfhip_ctx* ctx, const uint32_t* src_d, uint32_t* dst_d, uint32_t log_size);
/* FieldOps::batch_inverse over M31: dst[i] = src[i]^-1, src[i] != 0. */
int32_t bfhip_batch_inverse_m31(bfhip_ctx* ctx, const uint32_t* src_d, uint32_t* dst_d, size_t n);
/* FieldOps::batch_inverse over QM31 (the PackedSecureField denominators of LogupTraceGenerator::finalize_col, memory/table.rs:513):
 * 4 coordinate columns in, 4 out (may alias), n elements, none zero. */
int32_t bfhip_batch_inverse_qm31(bfhip_ctx* ctx, const uint32_t* const src_d[4], uint32_t* const dst_d[4], size_t n);
/* AccumulationOps::accumulate: dst[i] += src[i] in M31. */
int32_t bfhip_accumulate(bfhip_ctx* ctx, uint32_t* dst_d, const uint32_t* src_d, size_t n);
/* PolyOps::eval_at_point (CommitmentSchemeProver::prove_values): f(P) for P = (x, y) in QM31^2 given as u32[8] = x[4] || y[4];
 * coeffs_d holds 2^log_size coefficients (replicated != 0: the 2^(log_size-4) coefficients of index 0 mod 16). out_h = u32[4]. */
int32_t bfhip_eval_at_point(bfhip_ctx* ctx, const uint32_t* coeffs_d, uint32_t log_size, int32_t replicated, const uint32_t point_h[8], uint32_t out_h[4]);
/* MerkleOps<Blake2sMerkleHasher>::commit_on_layer (tree_builder.commit, mod.rs:500,583,723): 2^log_size nodes,
 * node i = hash_node(prev[2i], prev[2i+1], [cols[k][i >> col_shift[k]] for k < n_cols]) under the context's merkle_node_hash convention;
 * prev_layer_d may be NULL (deepest layer). col_shifts_h may be NULL (all 0). Hashes are 32-byte records. */
int32_t bfhip_merkle_commit_layer(bfhip_ctx* ctx, uint32_t log_size, const void* prev_layer_d, const uint32_t* const* cols_h, const uint32_t* col_shifts_h,
                                  uint32_t n_cols, void* out_hashes_d);
/* MerkleOps<Poseidon252MerkleHasher>::commit_on_layer (upstream stwo capability named by BASELINE.json config 5; the reference itself
 * only uses Blake2s — SURVEY.md F9): node i = poseidon_hash_many([prev[2i], prev[2i+1]]? ++ blocks), block = 8 M31 column values packed
 * as w = w * 2^31 + v (zero padded). Hashes are felt252 values stored as 8 little-endian u32 limbs (32 bytes), canonical form. */
int32_t bfhip_merkle_commit_layer_poseidon252(bfhip_ctx* ctx, uint32_t log_size, const void* prev_layer_d, const uint32_t* const* cols_h,
                                             const uint32_t* col_shifts_h, uint32_t n_cols, void* out_hashes_d);
/* One Hades permutation (Starknet Poseidon, width 3) of three canonical felt252 values, 8 LE u32 limbs each — the known-answer-test hook. */
int32_t bfhip_hades_permutation(bfhip_ctx* ctx, const uint32_t in_h[24], uint32_t out_h[24]);
/* FriOps::fold_line: 2^log_size evaluations over LineDomain(Coset::half_odds(log_size)) -> 2^(log_size-1); alpha_h = u32[4]. */
int32_t bfhip_fold_line(bfhip_ctx* ctx, const uint32_t* const src_d[4], uint32_t* const dst_d[4], uint32_t log_size, const uint32_t alpha_h[4]);
/* FriOps::fold_circle_into_line: dst = dst * alpha^2 + fold(src); src has 2^log_size cells on CanonicCoset(log_size).circle_domain(). */
int32_t bfhip_fold_circle_into_line(bfhip_ctx* ctx, uint32_t* const dst_d[4], const uint32_t* const src_d[4], uint32_t log_size, const uint32_t alpha_h[4]);
/* One FRI commit step on a layer of 2^log_size rows as ONE launch: the fold that produces the layer and the deepest level of its Merkle tree.
 * Replaces FriOps::fold_line (src_d, 2^(log_size+1) rows) followed, when quot_d != NULL, by FriOps::fold_circle_into_line (quot_d, a circle
 * evaluation of 2^(log_size+1) cells) on the result, followed by MerkleOps<Blake2sMerkleHasher>::commit_on_layer(log_size, prev = NULL, the 4
 * coordinate columns) — what FriProver::commit does per layer (prover::prove, mod.rs:732). src_d == NULL: the first line layer, a
 * fold_circle_into_line of quot_d into a zero destination. dst_d receives the folded coordinate columns, out_hashes_d the 2^log_size 32-byte
 * leaf hashes under the context's merkle_node_hash convention. Whole layers only (no row range). */
int32_t bfhip_fri_fold_leaf(bfhip_ctx* ctx, const uint32_t* const src_d[4], const uint32_t* const quot_d[4], uint32_t* const dst_d[4], uint32_t log_size,
                            const uint32_t alpha_h[4], void* out_hashes_d);
/* GrindOps::grind for Blake2sChannel: smallest nonce such that mix_u64(nonce) on `digest_h` (32 bytes) leaves >= pow_bits trailing zeros. */
int32_t bfhip_grind(bfhip_ctx* ctx, const uint8_t digest_h[32], uint32_t pow_bits, uint64_t* nonce);
/* GrindOps::grind for Poseidon252Channel: the smallest nonce >= start_nonce such that poseidon_hash(digest, nonce) — the digest after
 * mix_u64(nonce) — has >= pow_bits trailing zeros in that channel's sense. digest_h: the felt252 digest as its canonical 32
 * little-endian bytes (a value >= p is refused). tried (may be NULL): nonces scanned = launches x span. */
int32_t bfhip_grind_poseidon252(bfhip_ctx* ctx, const uint8_t digest_h[32], uint32_t pow_bits, uint64_t start_nonce,
                                uint64_t* nonce, uint64_t* tried);
/* Decommitment reads: out_h[j] = col_d[idx_h[j]] for n positions of one column. */
int32_t bfhip_gather(bfhip_ctx* ctx, const uint32_t* col_d, const uint64_t* idx_h, size_t n, uint32_t* out_h);

/* ---- per-component AIR operations (what `ComponentProver` / `LogupTraceGenerator` / `QuotientOps` of a HipBackend would call) ----
 * component: 0 memory, 1 instruction, 2 program, 3 processor, 4 jump-if-not-zero, 5 jump-if-zero, 6 input, 7 left, 8 minus, 9 output,
 * 10 plus, 11 right, 12 end_of_execution (the numbering of `bfhip_trace_column`). lookup_h = u32[24]: (z[4], alpha[4]) of the Memory, Instruction and Processor relations, in that order
 * (mod.rs:589-597 draws them in this order). */

/* Shape of one component: main-trace columns, logUp (secure) columns, constraints. Returns -1 for an unknown component. */
int32_t bfhip_component_shape(int32_t component, uint32_t* n_main_cols, uint32_t* n_logup_cols, uint32_t* n_constraints);
/* `interaction_trace_evaluation` of one component (e.g. memory/table.rs:485-518, processor/table.rs:456-529): LogupTraceGenerator
 * new_col / write_frac / finalize_col / finalize_last. main_rows_h: n_main device pointers to row-granular columns (2^(log_size-4)
 * rows). out_cols_h: 4 * n_logup device pointers to coordinate columns in bit-reversed circle-domain order; the last 4 (the prefix-
 * summed column) hold 2^log_size cells, earlier ones are 16-lane replicated and are written row-granular (2^(log_size-4) cells).
 * claimed_sum_h = u32[4] receives the component's claimed sum. */
int32_t bfhip_logup_generate(bfhip_ctx* ctx, int32_t component, uint32_t log_size, const uint32_t* const* main_rows_h, const uint32_t lookup_h[24],
                             uint32_t* const* out_cols_h, uint32_t claimed_sum_h[4]);
/* `ComponentProver::evaluate_constraint_quotients_on_domain` of one component (FrameworkComponent<XEval>, components/<name>/component.rs):
 * every constraint of the component on CanonicCoset(log_size + 1).circle_domain(), each multiplied by its random-coefficient power
 * and by the inverse of the trace-domain vanishing polynomial, added into acc_d (4 coordinate columns of 2^(log_size+1) cells).
 * is_first_d: the preprocessed IsFirst LDE (2^(log_size+1) cells). main_lde_h / inter_lde_h: device pointers to the n_main and
 * 4 * n_logup LDE columns; *_shifts_h (may be NULL = 0) give the replication shift of each (cell i is read at index i >> shift).
 * coeffs_h = u32[4 * n_constraints]: the coefficient of constraint j in evaluation order (the caller reverses the accumulator's
 * power slice the way `accum.columns()` does; bfhip_air_compose_coeffs writes exactly these, for all components). claimed_sum_h = the component's logUp total. */
int32_t bfhip_eval_constraints(bfhip_ctx* ctx, int32_t component, uint32_t log_size, const uint32_t* is_first_d, const uint32_t* const* main_lde_h,
                               const uint32_t* main_shifts_h, const uint32_t* const* inter_lde_h, const uint32_t* inter_shifts_h, const uint32_t lookup_h[24],
                               const uint32_t claimed_sum_h[4], const uint32_t* coeffs_h, uint32_t* const acc_d[4]);
/* ---- the AIRs asserted on the trace domain: which component, which constraint, which row ----
 * stwo's `assert_constraints`, which every component test of the reference is built on (positive: memory/component.rs:201-208 and all 13
 * components at mod.rs:252-396; negative: memory/component.rs:211-609, whose panic texts quote the failing row and value). A proof of a
 * trace that is not a valid execution only fails with "ConstraintsNotSatisfied" at its out-of-domain check; these entry points say where.
 * A cell is a storage index i in [0, 2^log_size) of CanonicCoset(log_size) in bit-reversed circle-domain order; table row = i >> 4.
 * IsFirst is 1 at cell 0. Constraints are numbered in evaluation order (bfhip_component_shape gives their count, at most 12), the logUp
 * constraints last. A base-field constraint's value is reported as (v, 0, 0, 0). */
typedef struct bfhip_check_report {
    uint32_t component, log_size;
    uint64_t n_bad_cells;              /* cells where at least one constraint is non-zero */
    uint64_t first_bad_cell;           /* storage index; table row = >> 4; UINT64_MAX if none */
    int32_t  first_bad_constraint;     /* lowest constraint that is non-zero at first_bad_cell; -1 if none */
    uint32_t first_bad_value[4];       /* its value there */
    uint64_t bad_per_constraint[16];   /* cells where constraint j is non-zero */
    uint32_t claimed_sum[4];           /* the component's logUp total the check ran with */
    uint32_t reserved[3];
} bfhip_check_report;
/* One component on caller-supplied columns: the pointers and layouts bfhip_logup_generate takes and produces. main_rows_h: n_main device
 * pointers to row-granular columns (2^(log_size-4) rows); logup_cols_h: 4 * n_logup device pointers to coordinate columns, the last 4 of
 * 2^log_size cells, earlier ones row-granular; claimed_sum_h = the total the last logUp column closes on. The previous row of the last
 * logUp column is its neighbour at coset offset -1 on the trace domain itself. Returns 0 whether or not the trace is valid — the verdict
 * is in *out, and bfhip_last_error() is not touched by violations; -1 only for bad arguments (unknown component, log_size outside
 * [4, 29], null pointers, a context in a shard group) and HIP errors. */
int32_t bfhip_check_constraints(bfhip_ctx* ctx, int32_t component, uint32_t log_size, const uint32_t* const* main_rows_h, const uint32_t* const* logup_cols_h,
                                const uint32_t lookup_h[24], const uint32_t claimed_sum_h[4], bfhip_check_report* out);
/* `QuotientOps::accumulate_quotients` (compute_fri_quotients, reached from mod.rs:732) for the columns of one LDE size: n_cols
 * columns of 2^log_size cells on CanonicCoset(log_size).circle_domain() (bit-reversed; col_shifts_h as above: 0 or >= 2, may be NULL).
 * Column k has n_samples_h[k] samples; sample_points_h (u32[8] each: x[4] || y[4]) and sample_values_h (u32[4] each) list them column
 * by column. Batches are formed per distinct point in BTreeMap order like ColumnSampleBatch::new_vec. out_d: 4 coordinate columns. */
int32_t bfhip_accumulate_quotients(bfhip_ctx* ctx, uint32_t log_size, const uint32_t* const* cols_h, const uint32_t* col_shifts_h, uint32_t n_cols,
                                   const uint32_t* n_samples_h, const uint32_t* sample_points_h, const uint32_t* sample_values_h,
                                   const uint32_t random_coeff_h[4], uint32_t* const out_d[4]);

/* prove_brainfuck (crates/brainfuck_prover/src/brainfuck_air/mod.rs:471-735), device resident: compiles and runs `code` on the
 * host VM (crates/brainfuck_vm), builds the 13 component tables, then commits, evaluates constraints, samples, builds the FRI
 * quotients, runs FRI, grinds and decommits on the GPU. *proof_json receives the serde_json form of BrainfuckProof (mod.rs:71-76),
 * malloc'd — release with bfhip_free_host. log_max_rows = LOG_MAX_ROWS (mod.rs:428: 24; 20 under cfg(test), mod.rs:433); the
 * context must have been created with max_log_domain >= log_max_rows + 2.
 * transcript (optional): channel digests after each stage, "name:hex\n". phase_seconds (optional): 10 doubles
 * {preprocessed, tables(host), main_trace, interaction, composition, oods, quotients, fri(+pow+decommit), decommit, total}. */
int32_t bfhip_prove_brainfuck(bfhip_ctx* ctx, const char* code, const uint8_t* input_h, size_t n_input, uint32_t log_max_rows,
                              char** proof_json, size_t* proof_len, char** transcript, double* phase_seconds);
void bfhip_free_host(void* p);
/* What the last COMPLETED proof of this context actually did (0 before the first): bit 0 = it ran in the mailbox order (forcing mode 1 does not
 * guarantee it: one proof per GPU holds that order at a time, see bfhip_ctx_set_sync_policy), bit 1 = it took the context's kept preprocessed tree
 * (bfhip_ctx_reuse_preprocessed), bit 2 = it took a pool's shared preprocessed tree (bfhip_pool_set_preprocessed), bit 3 = shard group: the transforms were replicated
 * (bfhip_ctx_set_shard_policy), bit 4 = the decommitment's gather request table outgrew a quarter of the staging ring and was split over
 * several launches (many queries at a large LOG_MAX_ROWS), bit 5 = FRI layers were folded inside the leaf launch of their Merkle tree
 * (bfhip_fri_fold_leaf's kernel: layers of 2^17 rows and above, device channel, one process), bit 6 = the preflight ran and passed
 * (bfhip_ctx_set_preflight). Tests and tools read it so that
 * a setting that silently did not apply is visible. */
int32_t bfhip_ctx_last_proof_flags(bfhip_ctx* ctx, uint32_t* flags);
/* ---- one proof over several GPUs (shard group) ------------------------------------------------------------------------------------------
 * north_star: "trace columns shard naturally across the 8 GPUs of one node, with the Merkle root and FRI fold reduced via RCCL over xGMI"
 * (SURVEY.md section 8(e)). The ranks of a group prove ONE trace together and all return the byte-identical proof of the single-GPU path:
 *   - the full-size columns of the interaction and composition trees are COLUMN-sharded for interpolation / LDE (greedy by size), then one
 *     grouped send-receive cuts every LDE column into contiguous bit-reversed ROW ranges (contiguous ranges of a bit-reversed circle domain
 *     are sub-cosets), together with a previous-row copy of each component's last logUp column (its mask offset -1 is not a halo);
 *   - Merkle subtrees, constraint evaluation, FRI quotients and the FRI folds down to 2^14 rows per rank are row-local; one all-gather per
 *     tree completes the layer of 256 nodes per rank, the top is hashed redundantly so that every rank feeds the same root to its channel;
 *   - out-of-domain samples and decommitment words are each produced by one rank and completed by a max-reduce (exact: zero elsewhere).
 * Every exchange is issued by the library on the context's own stream with device buffers on both ends; the host program supplies no
 * callbacks. Two transports:
 *   RCCL  — one process per GPU: rank 0 calls bfhip_rccl_unique_id, the host program hands the 128 bytes to the other ranks (any control
 *           channel: torch.distributed, MPI, a file), every rank calls bfhip_ctx_join_rccl_group. librccl is loaded on first use.
 *   local — the N contexts belong to one process and are driven by N host threads; they may share a GPU (how the tests run N ranks on a
 *           one-GPU box) or own one each (peer copies between the GPUs, ordered by HIP events).
 * count must be a power of two in [2, 64]. Every rank must issue the same sequence of prove calls on the same trace. */
typedef struct bfhip_local_group bfhip_local_group;
int32_t bfhip_local_group_create(uint32_t count, bfhip_local_group** out);
int32_t bfhip_local_group_destroy(bfhip_local_group* group);
int32_t bfhip_ctx_join_local_group(bfhip_ctx* ctx, bfhip_local_group* group, uint32_t rank);
int32_t bfhip_rccl_unique_id(uint8_t id[128]);
int32_t bfhip_ctx_join_rccl_group(bfhip_ctx* ctx, const uint8_t id[128], uint32_t rank, uint32_t count);
int32_t bfhip_ctx_leave_group(bfhip_ctx* ctx);
/* How a shard group divides a proof (every rank of a group the same value; takes effect at the next proof; byte-identical proofs either way):
 *   0  exchange: the transforms are column-sharded and one grouped send-receive per tree cuts the LDE columns into row ranges (the default of rounds 2-5;
 *      1.03 / 0.84 / 0.72 GB per fib19 proof and rank at 2 / 4 / 8 ranks, over N - 1 xGMI links per GPU);
 *   1  replicate the transforms: every rank interpolates and extends every column and evaluates the constraints on every row itself (the transforms are
 *      20 % of a proof), and ONLY the Merkle hashing, the quotient rows and the FRI folds are divided by row range — no column -> row exchange at all,
 *      what travels is the per-tree all-gather of 256 nodes per rank and the max-reduces;
 *  -1  automatic (default): 1 for a group of two ranks on different GPUs (their exchange would cross ONE xGMI link: 13.5 ms at 76 GB/s against 5.6 ms of
 *      transforms), 0 otherwise. Unmeasured on multi-GPU hardware: DESIGN.md section 7 has the arithmetic. */
int32_t bfhip_ctx_set_shard_policy(bfhip_ctx* ctx, int32_t policy);
/* Since the group was joined: out = {all-gathers, max-reduces, grouped send-receives, payload bytes this rank sent to other ranks}. */
int32_t bfhip_ctx_group_stats(bfhip_ctx* ctx, uint64_t out[4]);
/* GPU-side milliseconds this rank's stream spent inside {all-gathers, max-reduces, grouped send-receives} since the group was joined (one
 * HIP-event pair per collective): the communication share of a proof over several GPUs. Synchronises the context's stream. */
int32_t bfhip_ctx_group_times(bfhip_ctx* ctx, double out_ms[3]);
/* Per-collective latency of this rank since the group was joined (or since the last call with reset != 0), for {all-gathers, max-reduces, grouped
 * send-receives} in that order, 7 numbers each: {count, GPU-side p50, p90, max, host-side p50, p90, max} in microseconds. GPU side = the HIP-event pair
 * around the collective on its stream (includes waiting for the slowest peer); host side = the time the calling thread spent inside the transport's
 * call (RCCL: the enqueue). A proof over N GPUs issues ~31 collectives of mostly small payloads: on hardware their latency decides, not their bytes.
 * Synchronises the context's stream. */
int32_t bfhip_ctx_group_latency(bfhip_ctx* ctx, int32_t reset, double out_us[21]);
/* Test entry: joins an RCCL group (unique id, rank, count), runs ONE grouped send-receive on the given blocks and leaves. With the real library
 * the blocks must be device memory. In the test-hooks build of the library (libbfhip_testhooks.so, -DBFHIP_TEST_HOOKS) the environment variable
 * BFHIP_RCCL_LIBRARY names a test double of the RCCL entry points (tests/mock_rccl.c: host-memory blocks, no GPU needed); the default build
 * ignores that variable and loads librccl only. stats_out (optional) = the counters of bfhip_ctx_group_stats. */
int32_t bfhip_rccl_exchange_raw(const uint8_t id[128], uint32_t rank, uint32_t count, uint32_t n_sends, const uint32_t* send_peer, void* const* send_ptr,
                                const size_t* send_bytes, uint32_t n_recvs, const uint32_t* recv_peer, void* const* recv_ptr, const size_t* recv_bytes,
                                uint64_t stats_out[4]);
/* Exercises the RCCL transport with a one-rank communicator on this context's GPU (library load, communicator, all-gather, max-reduce,
 * grouped exchange): what a single-GPU box can check of the multi-process path. */
int32_t bfhip_rccl_selftest(bfhip_ctx* ctx);
/* rank / count (0 / 1 outside a group) and a static description of the transport. Any pointer may be NULL. */
int32_t bfhip_ctx_group_info(bfhip_ctx* ctx, uint32_t* rank, uint32_t* count, const char** transport);

/* Optional (off by default): keep the preprocessed tree (IsFirst(LOG_MAX_ROWS..=4): polynomials, LDE columns, Merkle layers, root) of
 * the first proof in the context and reuse it for later proofs with the same LOG_MAX_ROWS. The reference recommits it in every
 * prove_brainfuck call (mod.rs:495-500); proof bytes are identical either way. Call with on = 0 before bfhip_ctx_destroy to release it.
 * Joining or leaving a shard group drops the cached tree (it is rebuilt by the next proof): the ranks of a group must all reuse or all rebuild,
 * which holds when every rank sets this option the same way and starts its membership with an empty cache. */
int32_t bfhip_ctx_reuse_preprocessed(bfhip_ctx* ctx, int32_t on);

/* The two halves of prove_brainfuck, so that a caller (and the benchmark) can keep the prover input resident in HBM:
 * bfhip_trace_create = VM run + the 13 `XTable::from(&vm_trace)` builders (mod.rs:508-547) + upload of the row-granular columns;
 * bfhip_prove_trace  = everything from the preprocessed commitment (mod.rs:493) to the finished proof (mod.rs:734). */
int32_t bfhip_trace_create(bfhip_ctx* ctx, const char* code, const uint8_t* input_h, size_t n_input, bfhip_trace** out,
                           uint32_t log_sizes[13], uint64_t* n_steps, uint64_t* main_cells, uint64_t* interaction_cells);
/* The same with the VM's RAM size given (MachineBuilder::with_ram_size, machine.rs:56-60; `--ram-size` of bin/brainfuck_prover.rs);
 * ram_size = 0 selects Machine::DEFAULT_RAM_SIZE = 30000 (machine.rs:114). */
int32_t bfhip_trace_create_ram(bfhip_ctx* ctx, const char* code, const uint8_t* input_h, size_t n_input, size_t ram_size, bfhip_trace** out,
                               uint32_t log_sizes[13], uint64_t* n_steps, uint64_t* main_cells, uint64_t* interaction_cells);
/* What prove_brainfuck(&Machine) actually receives (mod.rs:471-473): an EXECUTED machine — its register trace (`inputs.trace()`, mod.rs:508;
 * n_rows rows of 7 u32: clk, ip, ci, ni, mp, mv, mvi, the final ci = ni = 0 row included) and its compiled program (`inputs.program()`,
 * n_code words incl. the jump-target words). No re-execution: the rows are uploaded as they are and the 13 tables are built from them.
 * Values must be canonical M31 (< 2^31 - 1); the trace must be non-empty. With the GPU table builder (the default) the rows reach the device
 * in one copy and are transposed and checked by one kernel (bfhip_prove_registers names the offending row; this entry keeps its text). */
int32_t bfhip_trace_create_from_registers(bfhip_ctx* ctx, const uint32_t* trace7_h, size_t n_rows, const uint32_t* code_words_h, size_t n_code,
                                          bfhip_trace** out, uint32_t log_sizes[13], uint64_t* main_cells, uint64_t* interaction_cells);
int32_t bfhip_trace_destroy(bfhip_ctx* ctx, bfhip_trace* trace);
/* Where the 13 `XTable::from(&vm_trace)` builders (mod.rs:511-547) of this context run: 1 = on the GPU (default; sorts, clk-gap fill, padding,
 * pairing and per-opcode selection as gfx950 kernels), 0 = host builders + upload. Results are identical. */
int32_t bfhip_ctx_set_table_builder(bfhip_ctx* ctx, int32_t on_gpu);
/* Row-granular main-trace column `column` of component `component` (claim order) of a resident trace -> host. out_h may be NULL (size query). */
int32_t bfhip_trace_column(bfhip_ctx* ctx, const bfhip_trace* trace, uint32_t component, uint32_t column, uint32_t* out_h, size_t cap, size_t* n_rows);
int32_t bfhip_prove_trace(bfhip_ctx* ctx, const bfhip_trace* trace, uint32_t log_max_rows, char** proof_json, size_t* proof_len,
                          char** transcript, double* phase_seconds);
/* prove_brainfuck(&Machine) (mod.rs:471-473) in ONE call: the executed machine's register rows (`inputs.trace()`, mod.rs:508) and program words
 * in, the proof out — the bytes of bfhip_trace_create_from_registers followed by bfhip_prove_trace. The rows go to the device in one copy
 * and are transposed into columns and checked there; that and the table build are enqueued while the GPU already works on the preprocessed
 * commitment (what bfhip_prove_brainfuck does for a program text), and the tables live in the proof's arena: no resident trace.
 * A non-canonical register is reported with its place: "register value is not a canonical M31 (row R, register K)", the lowest
 * (row, register) of the trace, register K in the order clk, ip, ci, ni, mp, mv, mvi. n_rows >= 2^31 is refused. Outputs as for
 * bfhip_prove_brainfuck. */
int32_t bfhip_prove_registers(bfhip_ctx* ctx, const uint32_t* trace7_h, size_t n_rows, const uint32_t* code_words_h, size_t n_code,
                              uint32_t log_max_rows, char** proof_json, size_t* proof_len, char** transcript, double* phase_seconds);

/* The 13 components of a resident trace (bfhip_trace_create*): for each the logUp columns are generated with the prover's own logUp kernels
 * into the context's arena (which is reset like a proof resets it) and bfhip_check_constraints' pass runs over them; out[k] = component k.
 * logup_total_h = the sum of the 13 claimed sums: zero iff `lookup_sum_valid` (mod.rs:207-226) holds. *n_bad_components = components with
 * n_bad_cells != 0 (may be NULL). The trace is an execution trace the prover will accept iff that count is 0 and the total is zero.
 * lookup_h: (z, alpha) of Memory, Instruction, Processor (u32[24], as above). NULL = what `MemoryElements::draw`, `InstructionElements::draw`
 * and `ProcessorElements::draw` (mod.rs:589-597, in this order) give on `Blake2sChannel::default()`: the k-th `draw_felts(2)` is the
 * eight base-field words of Blake2s-256(0^32 || LE32(k) || 0^28), each reduced mod 2^31 - 1 (no word of these three draws reaches
 * 2 (2^31 - 1), so none is redrawn): z = words 0..3, alpha = words 4..7. Not the elements of any proof — those depend on the commitments —
 * but fixed, so a report can be reproduced. A context in a shard group is refused. Returns 0 whether or not the trace is valid. */
int32_t bfhip_trace_check(bfhip_ctx* ctx, const bfhip_trace* trace, const uint32_t* lookup_h /* u32[24] or NULL */,
                          bfhip_check_report out[13], uint32_t logup_total_h[4], int32_t* n_bad_components);

/* ---- the lookup tuples that do not cancel: which relation entry is yielded and never used, or used and never yielded ----
 * stwo's relation tracker (the second debugging tool it ships for AIR authors beside `assert_constraints`) over the row-granular tables.
 * A non-zero logUp total (bfhip_trace_check; `lookup_sum_valid`, mod.rs:207-226) says that the lookups do not balance, not which
 * tuple is to blame; a trace can satisfy all 13 AIRs row by row and still fail there (an opcode that is no instruction: the Processor
 * table yields its row into the Processor relation and no opcode table consumes it). These entry points name the tuples.
 * The three relations, their tuples and who adds to them (`add_to_relation` of components/<name>/component.rs, restated in csrc/air.h; d = the
 * table's dummy column; the multiplicity of a table row is its logUp numerator, an M31 value):
 *   0 Memory      (clk, mp, mv), 3 words               yields (1 - d): Processor cols 0, 4, 5, d = col 7
 *                                                      uses   (d - 1): Memory cols 0, 1, 2, d = col 3
 *   1 Instruction (ip, ci, ni), 3 words                yields (1 - d): Processor cols 1, 2, 3; Program cols 0, 1, 2, d = col 3
 *                                                      uses   (d - 1): Instruction cols 0, 1, 2, d = col 3
 *   2 Processor   (clk, ip, ci, ni, mp, mv, mvi), 7    yields (1 - d): Processor cols 0..6
 *                                                      uses   (d - 1): jnz, jz cols 0..6, d = col 11; input, left, minus, output, plus, right
 *                                                                      cols 0..6, d = col 7; end_of_execution cols 0..6, always -1
 * A table row with numerator 0 contributes nothing and is no entry. Numerator 1 counts as a yield, p - 1 as a use, anything else (a d that
 * is not boolean) as "other". net of a tuple = the sum of its numerators in M31, canonical; a tuple is unbalanced iff net != 0. Counts
 * are per TABLE ROW: every row stands for 16 trace cells (LOG_N_LANES = 4), so the logUp sum sees 16 x net of each tuple.
 * Layouts (natural alignment, declaration order):
 *   bfhip_relation_entry   96 bytes: relation 0, n_words 4, tuple 8, net 36, n_yield 40, n_use 48, n_other 56, first_yield_table 64,
 *                                    first_use_table 68, first_yield_row 72, first_use_row 80, reserved 88
 *   bfhip_relation_report  48 bytes: relation 0, n_words 4, n_entries 8, n_tuples 16, n_unbalanced 24, n_reported 32, reserved 40
 *   bfhip_relation_table   16 bytes: component 0, log_size 4, main_rows_h 8 */
typedef struct bfhip_relation_entry {
    uint32_t relation, n_words;
    uint32_t tuple[7];                 /* the tuple's words, zero padded beyond n_words */
    uint32_t net;                      /* sum of the numerators, canonical M31; never 0 in a reported entry */
    uint64_t n_yield, n_use, n_other;  /* table rows with numerator 1 / p - 1 / anything else non-zero */
    int32_t  first_yield_table, first_use_table;   /* index into the table list; -1 if none */
    uint64_t first_yield_row, first_use_row;       /* table row; UINT64_MAX if none. "first" = the lowest (table index, row) */
    uint32_t reserved[2];
} bfhip_relation_entry;
typedef struct bfhip_relation_report {
    uint32_t relation, n_words;
    uint64_t n_entries;                /* table rows with a non-zero numerator */
    uint64_t n_tuples;                 /* distinct tuples among them */
    uint64_t n_unbalanced;             /* tuples with net != 0, whatever the cap */
    uint64_t n_reported;               /* min(n_unbalanced, cap_per_relation) */
    uint32_t reserved[2];
} bfhip_relation_report;
typedef struct bfhip_relation_table {
    int32_t component;                 /* claim order, 0..12 */
    uint32_t log_size;                 /* 2^(log_size - 4) table rows */
    const uint32_t* const* main_rows_h;   /* host array of device pointers to the row-granular main columns: what bfhip_check_constraints takes */
} bfhip_relation_table;
/* Any list of 1..64 caller-supplied tables; a component may be absent or repeated (an integrator of the Rust HipBackend builds the tables
 * outside this library). out[r] = relation r; relation r's entries go to entries_h + r * cap_per_relation: the unbalanced tuples in
 * lexicographic order of their words (word 0 most significant, unsigned), the first cap_per_relation of them; slots beyond n_reported are not written. entries_h == NULL with
 * cap_per_relation == 0 gives the counts only. Every field is an integer and the same whatever the schedule. Uses the context's arena
 * (reset like a proof resets it). Returns 0 whether or not anything is unbalanced, and bfhip_last_error() is not touched by imbalances;
 * -1 only for bad arguments (unknown component, log_size outside [4, 29], null pointers, more than 2^31 table rows in total, a context
 * in a shard group) and HIP errors. */
int32_t bfhip_relation_summary(bfhip_ctx* ctx, const bfhip_relation_table* tables, uint32_t n_tables, bfhip_relation_report out[3],
                               bfhip_relation_entry* entries_h, uint32_t cap_per_relation);
/* The 13 tables of a resident trace (bfhip_trace_create*): table index = component. */
int32_t bfhip_trace_relations(bfhip_ctx* ctx, const bfhip_trace* trace, bfhip_relation_report out[3], bfhip_relation_entry* entries_h,
                              uint32_t cap_per_relation);

/* ---- preflight: a proof that first rejects a trace it cannot prove, naming row and tuple ---------------------------------------------------
 * A trace that is canonical but is not an execution costs a whole proof before it fails at the out-of-domain check with
 * "ConstraintsNotSatisfied"; one whose 13 AIRs hold row by row but whose lookups do not balance is not stopped by the prover at all (it has
 * no `lookup_sum_valid` check, mod.rs:207-226: a verifier rejects the proof). With the preflight on, every proving entry point of the
 * context (bfhip_prove_trace, bfhip_prove_brainfuck, bfhip_prove_registers, and through them a pool's jobs) runs bfhip_trace_check's
 * assertion on its row-granular tables — a resident trace's columns, or the tables just built in the proof's arena — before anything of the
 * main-trace phase is enqueued: the logUp pass (4 launches), the cells of all 13 components in ONE launch, one launch of 13 + 1 waves
 * (first failing constraint of each component; the QM31 sum of the 13 claimed sums), ONE read-back. Each component's total is read on the
 * device from the slot the logUp pass wrote. The lookup elements are the fixed defaults of bfhip_trace_check(.., NULL, ..), so the 13
 * reports and the total are those of that call on the same tables. Scratch comes from the proof's arena and is given back before the
 * main-trace phase allocates.
 *   pass    the proof goes on exactly as without the preflight (same launches, bytes and transcript); bit 6 of bfhip_ctx_last_proof_flags.
 *   fail    (a component with n_bad_cells != 0, or a non-zero total) nothing further of the proof is enqueued, the side stream is joined
 *           as at the other early exits, and the call returns BFHIP_TRACE_REJECTED with the text of bfhip_format_preflight in
 *           bfhip_last_error(). If the total is non-zero, bfhip_relation_summary's pass runs over the same 13 tables with a cap of 4
 *           entries per relation. The context stays usable; the next proof starts clean.
 * A FILTER, NOT A SOUNDNESS GATE: the elements are fixed and public, so a trace built to cancel under them passes — and then ends as it does
 * without the preflight. A context in a shard group is not supported: bfhip_ctx_set_preflight(ctx, 1) on a member is refused
 * (bfhip_ctx_leave_group first), and a context with the preflight on cannot join (bfhip_ctx_set_preflight(ctx, 0) first).
 * Layout (natural alignment, declaration order):
 *   bfhip_preflight_report  4064 bytes: ran 0, rejected 4, n_bad_components 8, n_entries 12, logup_total 16, components 32, relations 2736,
 *                                       entries 2880, seconds 4032, reserved 4040 */
enum { BFHIP_TRACE_REJECTED = -3 };
/* default 0; takes effect at the next proof */
int32_t bfhip_ctx_set_preflight(bfhip_ctx* ctx, int32_t on);
int32_t bfhip_ctx_get_preflight(bfhip_ctx* ctx, int32_t* on);
typedef struct bfhip_preflight_report {
    uint32_t ran, rejected;            /* of the last proof call of this context that reached the preflight */
    int32_t  n_bad_components; uint32_t n_entries;       /* entries[] slots in use: the sum of relations[r].n_reported */
    uint32_t logup_total[4];
    bfhip_check_report    components[13];
    bfhip_relation_report relations[3];                  /* zero unless the relation summary ran */
    bfhip_relation_entry  entries[12];                   /* relation r at entries[4 r ..], n_reported of them */
    double   seconds;                                    /* host wall time of the preflight */
    uint64_t reserved[3];
} bfhip_preflight_report;
/* All zero before the first proof of the context that reached the preflight. */
int32_t bfhip_ctx_last_preflight(bfhip_ctx* ctx, bfhip_preflight_report* out);
/* Host only, no GPU: the text a rejection carries, lines joined by '\n':
 *   "TraceRejected: <n> of 13 components violate their constraints", "TraceRejected: the logUp total is not zero", or both joined by " and ";
 *   one line per failing component: "<name>: constraint <j> fails at table row <r> (cell <i>), value (a, b, c, d); <n> cells violate it";
 *   "logUp: the 13 claimed sums add up to (a, b, c, d), not zero" when they do;
 *   one line per reported tuple: "<relation> relation: (<words>) net <+n>: yielded <n>x (first: <table> row <r>), used <n>x (first: ..)"
 *   [", <n> rows with another multiplicity"], then "<relation> relation: <n> more unbalanced tuples not listed" per cut relation.
 * A report that was not rejected gives "preflight: ok" (ran) or "preflight: did not run". *need (may be NULL) = bytes needed, the
 * terminating NUL included. Returns 0, or -2 ("capacity") when cap < *need: buf then holds the first cap - 1 bytes, NUL-terminated
 * (buf may be NULL with cap 0: size query). */
int32_t bfhip_format_preflight(const bfhip_preflight_report* rep, char* buf, size_t cap, size_t* need);

/* ---- proofs in flight: a pool of sub-contexts on one GPU behind ONE caller thread -------------------------------------------------------------
 * The reference's caller is a single thread of control (prove_brainfuck, mod.rs:471-735); a single proof leaves the GPU partly idle in its
 * single-workgroup chains (tree tops, small FRI layers) and at its Fiat-Shamir round trips. A pool proves the proofs of a batch n_in_flight at a
 * time on internal worker threads (one sub-context each) and returns when all are done: +19 % (2 in flight) / +23 % (3) throughput at 2^22 rows,
 * +36..57 % at 2^20 rows, +10 % for fib19. Proof bytes are those of bfhip_prove_trace, proof by proof.
 * The sub-contexts share the twiddle tree and point tables of the first one, and — by default — ONE preprocessed commitment per batch:
 *   bfhip_pool_set_preprocessed(pool, mode): 0 = every proof recommits IsFirst(LOG_MAX_ROWS..=4) as the reference does in every prove_brainfuck
 *   call (mod.rs:495-500); 1 (default) = once per batch, committed by a builder context beside the first proofs' main-trace phase; 2 = kept
 *   across batches while LOG_MAX_ROWS, the hasher and log_blowup_factor stay the same. Byte-neutral: the tree depends on LOG_MAX_ROWS, the hasher
 *   and log_blowup_factor only.
 * Traces of a batch must be resident on the pool's device: create them with bfhip_trace_create*(bfhip_pool_ctx(pool, i), ...) — any i — between
 * batches (a sub-context must not be used by the caller while a batch runs). n_in_flight in [1, 16]; 2-3 is where the gain saturates. */
typedef struct bfhip_pool bfhip_pool;
int32_t bfhip_pool_create(int32_t device_id, uint32_t n_in_flight, uint32_t max_log_domain, bfhip_pool** out);
int32_t bfhip_pool_destroy(bfhip_pool* pool);
int32_t bfhip_pool_size(bfhip_pool* pool, uint32_t* n_in_flight);
/* Sub-context i (borrowed: owned by the pool, never pass it to bfhip_ctx_destroy): for bfhip_trace_create*, per-context settings, memory queries. */
int32_t bfhip_pool_ctx(bfhip_pool* pool, uint32_t i, bfhip_ctx** out);
/* bfhip_ctx_set_conventions on every sub-context and on the builder of the shared preprocessed tree (conv == NULL: the defaults). */
int32_t bfhip_pool_set_conventions(bfhip_pool* pool, const bfhip_conventions* conv);
int32_t bfhip_pool_set_preprocessed(bfhip_pool* pool, int32_t mode);
/* bfhip_ctx_set_pcs_config on every sub-context and on the builder of the shared preprocessed tree (pcs == NULL: the defaults). */
int32_t bfhip_pool_set_pcs_config(bfhip_pool* pool, const bfhip_pcs_config* pcs);
/* bfhip_ctx_set_preflight on every sub-context: a job whose trace is rejected ends with status BFHIP_TRACE_REJECTED and the rejection text
 * (a queued job's behind its "job <ticket>: " prefix); the other jobs and the pool are unaffected. Refused while jobs are outstanding. */
int32_t bfhip_pool_set_preflight(bfhip_pool* pool, int32_t on);
/* n x bfhip_prove_trace. Outputs are arrays of n entries, each optional (NULL): proofs_json[i] (malloc'd, bfhip_free_host; NULL when proof i failed),
 * proof_lens[i], statuses[i] (0 = ok, < 0 = that proof's error). seconds (optional) has n + 1 entries: each proof's own wall time from its start on
 * its worker, then the wall time of the whole batch. Returns 0 when every proof succeeded, -1 otherwise (bfhip_last_error: the first failed
 * proof's message); the other proofs of the batch are still delivered. statuses[i] = BFHIP_TRACE_REJECTED for a trace the preflight rejected. */
int32_t bfhip_prove_batch(bfhip_pool* pool, const bfhip_trace* const* traces, uint32_t n, uint32_t log_max_rows, char** proofs_json, size_t* proof_lens,
                          int32_t* statuses, double* seconds);
/* n x bfhip_prove_brainfuck: VM run, table build and upload of proof i happen inside its worker, beside the other workers' GPU work.
 * inputs_h may be NULL (no program reads input); n_inputs[i] bytes at inputs_h[i] otherwise. Outputs as above. */
int32_t bfhip_prove_batch_brainfuck(bfhip_pool* pool, const char* const* codes, const uint8_t* const* inputs_h, const size_t* n_inputs, uint32_t n,
                                    uint32_t log_max_rows, char** proofs_json, size_t* proof_lens, int32_t* statuses, double* seconds);

/* ---- the pool as a QUEUE: submit returns at once, results come back as they complete ---------------------------------------------------
 * A batch call returns when its LAST proof is done and nothing can be added while it runs; a deployment with a stream of executed machines
 * (the caller of prove_brainfuck(&Machine), mod.rs:471-473) wants the first proof's bytes as soon as they exist and the workers never idle.
 *   submit    returns at once with a ticket (1, 2, 3, ... per pool). Jobs START in ticket order on whichever worker is free; results are
 *             delivered in COMPLETION order, each exactly once. Program text, input bytes and program words are copied at submit; register
 *             rows and traces are BORROWED until that ticket's result has been taken (an AIR statement's rule: bfhip_pool_submit_air,
 *             below the generic entry points). What needs no GPU to check fails the submit itself
 *             (-1, no ticket): null pointers, zero rows, n_rows >= 2^31, more than BFHIP_POOL_MAX_OUTSTANDING jobs outstanding (queued +
 *             running + finished and not taken), a batch call in progress. Everything else fails the JOB.
 *   traces    for bfhip_pool_submit_trace may come from ANY context on the pool's device, e.g. one the caller owns: a trace is plain device
 *             memory (bfhip_trace_destroy ignores its context argument). The pool's sub-contexts stay off limits to the caller while
 *             anything is outstanding.
 *   wait      timeout_ms 0 polls, UINT32_MAX waits without limit. Returns 0 = *out holds a result, 1 = timed out with jobs outstanding,
 *             2 = nothing outstanding, -1 = error (null pool or null out: returned without blocking; the pool is being destroyed).
 *             The result owns proof_json and error: release both with bfhip_free_host.
 *   failures  a failed job is a result with status -1 and its own text, "job <ticket>: <message>"; whatever a job throws ends as that job's
 *             result, and the other jobs and the pool are unaffected. With bfhip_pool_set_preflight on, a job whose trace the preflight
 *             rejects has status BFHIP_TRACE_REJECTED instead: bad input, not an internal failure.
 *   cancel    0 = the job was still queued: it is removed and delivered with status BFHIP_JOB_CANCELLED; 1 = already running or finished (a
 *             running job is never interrupted); -1 = no such ticket was issued.
 *   destroy   bfhip_pool_destroy with jobs outstanding drops the queued jobs, lets the running ones finish and frees the untaken results.
 *   threads   one producer thread may submit while one consumer thread waits; destroy waits for calls in progress to return.
 *   shared preprocessed tree (bfhip_pool_set_preprocessed): 0 as for batches; in queue use 1 and 2 both mean "kept while LOG_MAX_ROWS, the
 *             hasher and log_blowup_factor match". The pool keeps up to two such trees (two values of LOG_MAX_ROWS interleaved in one
 *             stream both find theirs) and recommits one only when no running job uses it; a job that matches neither meanwhile commits its
 *             own. Proof bytes are the same either way; flags bit 2 says what a proof did. The queue creates no stream of its own.
 *   batches   bfhip_prove_batch*, bfhip_pool_set_conventions, bfhip_pool_set_pcs_config, bfhip_pool_set_preflight and bfhip_pool_set_preprocessed return -1
 *             ("jobs outstanding") while anything is queued, running or not yet taken; otherwise they behave as before.
 * Layout (natural alignment, declaration order):
 *   bfhip_pool_result  88 bytes: ticket 0, user_tag 8, status 16, worker 20, flags 24, log_max_rows 28, proof_json 32, proof_len 40,
 *                                error 48, seconds_queued 56, seconds_proving 64, reserved 72 */
enum { BFHIP_JOB_CANCELLED = -2, BFHIP_POOL_MAX_OUTSTANDING = 4096 };
typedef struct bfhip_pool_result {
    uint64_t ticket, user_tag;
    int32_t  status;                 /* 0 ok; -1 that proof's error; BFHIP_JOB_CANCELLED; BFHIP_TRACE_REJECTED */
    uint32_t worker;                 /* the sub-context that ran it (0 for a cancelled job) */
    uint32_t flags;                  /* bfhip_ctx_last_proof_flags of that proof (0 unless status == 0) */
    uint32_t log_max_rows;
    char*    proof_json; size_t proof_len;   /* malloc'd (bfhip_free_host); NULL unless status == 0 */
    char*    error;                  /* malloc'd text when status != 0, else NULL */
    double   seconds_queued, seconds_proving;   /* submit -> start on a worker; start -> done */
    uint64_t reserved[2];
} bfhip_pool_result;
int32_t bfhip_pool_submit_trace(bfhip_pool* pool, const bfhip_trace* trace, uint32_t log_max_rows, uint64_t user_tag, uint64_t* ticket);
int32_t bfhip_pool_submit_brainfuck(bfhip_pool* pool, const char* code, const uint8_t* input_h, size_t n_input, uint32_t log_max_rows, uint64_t user_tag,
                                    uint64_t* ticket);
/* What bfhip_prove_registers takes, as a job: rows borrowed, program words copied. */
int32_t bfhip_pool_submit_registers(bfhip_pool* pool, const uint32_t* trace7_h, size_t n_rows, const uint32_t* code_words_h, size_t n_code,
                                    uint32_t log_max_rows, uint64_t user_tag, uint64_t* ticket);
int32_t bfhip_pool_wait(bfhip_pool* pool, uint32_t timeout_ms, bfhip_pool_result* out);
/* Jobs queued, running, and finished but not yet taken by bfhip_pool_wait (any pointer may be NULL). */
int32_t bfhip_pool_outstanding(bfhip_pool* pool, uint32_t* queued, uint32_t* running, uint32_t* finished_not_taken);
int32_t bfhip_pool_cancel(bfhip_pool* pool, uint64_t ticket);

/* verify_brainfuck (mod.rs:738-797): replays the channel, checks the logUp sum (mod.rs:207-227), the OODS consistency, the proof of work,
 * every Merkle decommitment and FRI. Host only (the reference verifies on the CPU as well). Returns 0 = accepted, 1 = rejected with the
 * reason written to err (VerificationError name), -1 = internal error. */
int32_t bfhip_verify_brainfuck(const char* proof_json, size_t proof_len, uint32_t log_max_rows, char* err, size_t err_cap);
/* The same under explicit conventions (NULL = defaults): a proof verifies only under the conventions it was produced with. */
int32_t bfhip_verify_brainfuck_conv(const char* proof_json, size_t proof_len, uint32_t log_max_rows, const bfhip_conventions* conv, char* err, size_t err_cap);
/* The same under an explicit PcsConfig as well (pcs == NULL: PcsConfig::default()): a proof verifies only under the config it was made with.
 * An invalid config (see bfhip_pcs_config) returns -1. */
int32_t bfhip_verify_brainfuck_pcs(const char* proof_json, size_t proof_len, uint32_t log_max_rows, const bfhip_conventions* conv,
                                   const bfhip_pcs_config* pcs, char* err, size_t err_cap);

/* ---- Commitment-scheme session: commit and open ANY AIR's columns on the fused PCS path ---------------------------------------------------
 * bfhip_prove_* prove the 13 components of one snapshot of the reference. An AIR that differs from it (another column, another component)
 * computes its constraints from a constraint program (bfhip_air_*, below) or with bfhip_logup_generate / bfhip_eval_constraints, and keeps everything else:
 * the session below is stwo's CommitmentSchemeProver / CommitmentSchemeVerifier over trees of arbitrary columns opened at arbitrary points,
 * run by the same driver and the same fused launches as a Brainfuck proof (subtree / top Merkle kernels, batched sampling, one quotient launch
 * per size group, the device-stepped channel of the FRI commit phase with k_fri_fold_leaf / k_fri_layer / k_fri_tail, one gather for the
 * whole decommitment). INTEGRATION.md section 2e assembles the Brainfuck protocol from it.
 *   stwo                                                         here
 *   Blake2sChannel::default() / Poseidon252Channel::default()    bfhip_channel_create
 *   channel.mix_* / draw_felts / CirclePoint::get_random_point   bfhip_channel_mix_* / _draw_felts / _draw_point
 *   CommitmentSchemeProver::new(config, twiddles)                bfhip_pcs_create (the context's PcsConfig and twiddle tree)
 *   tree_builder.extend_evals / extend_polys + commit(channel)   bfhip_pcs_commit (form 0 / form 1)
 *   commitment_scheme.trees[t].polynomials / .evaluations        bfhip_pcs_tree_columns
 *   commitment_scheme.prove_values(sample_points, channel)       bfhip_pcs_prove_values
 *   CommitmentSchemeVerifier::new / commit / verify_values       bfhip_pcs_verifier_create / _commit / _verify_values
 *
 * The channel (host only, no GPU): created under a bfhip_conventions (NULL = defaults): merkle_channel selects Blake2sChannel or
 * Poseidon252Channel, mix_u64 the Blake2s form of mix_u64. Felts are 4 canonical words each, a point is x (4 words) then y (4 words); a
 * non-canonical word (>= 2^31 - 1) is refused, and so is a root that is no canonical felt252 under the Poseidon252 channel.
 * draw_felts(n) is stwo's: ceil(n / 2) draws of 8 base felts, two secure felts per draw (n = 1 is draw_felt, n = 2 a lookup element's draw).
 * draw_point is CirclePoint::get_random_point: t = draw_felt(), ((1 - t^2) / (1 + t^2), 2 t / (1 + t^2)). */
typedef struct bfhip_channel bfhip_channel;
int32_t bfhip_channel_create(const bfhip_conventions* conv, bfhip_channel** out);
int32_t bfhip_channel_destroy(bfhip_channel* ch);
int32_t bfhip_channel_mix_root(bfhip_channel* ch, const uint8_t hash32[32]);
int32_t bfhip_channel_mix_u64(bfhip_channel* ch, uint64_t v);
int32_t bfhip_channel_mix_felts(bfhip_channel* ch, const uint32_t* felts_h, size_t n);
int32_t bfhip_channel_draw_felts(bfhip_channel* ch, size_t n, uint32_t* out_h);
int32_t bfhip_channel_draw_point(bfhip_channel* ch, uint32_t point_out[8]);
/* digest (32 bytes; Poseidon252: the felt252 as canonical little-endian bytes) and the draw counter; either pointer may be NULL */
int32_t bfhip_channel_state(bfhip_channel* ch, uint8_t digest[32], uint32_t* n_sent);
/* Channel::trailing_zeros of the digest: what a proof of work is checked against */
int32_t bfhip_channel_trailing_zeros(bfhip_channel* ch, uint32_t* out);
/* Mask points: out = p + offset * CanonicCoset(log_size).step(), the point at which a column of 2^log_size rows is opened for the row
 * offset `offset` of a constraint (offset -1: the previous row). 1 <= log_size <= 30. Host only. */
int32_t bfhip_circle_point_offset(const uint32_t p[8], uint32_t log_size, int32_t offset, uint32_t out[8]);
/* The one AIR-dependent step of a VERIFIER of the snapshot's AIR assembled from the session: Components::eval_composition_polynomial_at_point
 * at `point_h`, which stwo's verify() compares with the sampled value of the composition polynomial (its four coordinate columns combined)
 * before it calls verify_values. n_cols_h[3] / n_samples_h / sampled_h: the sampled values of the preprocessed, main-trace and interaction
 * trees in the description of bfhip_pcs_prove_values (columns in commit order, n_samples_h[] per column, values flat, 4 words each).
 * lookup_h: 24 words as for bfhip_logup_generate. Host only. */
int32_t bfhip_brainfuck_composition_at_point(const uint32_t log_sizes_h[13], const uint32_t* claimed_sums_h, uint32_t log_max_rows, const uint32_t lookup_h[24],
                                             const uint32_t point_h[8], const uint32_t n_cols_h[3], const uint32_t* n_samples_h, const uint32_t* sampled_h,
                                             const uint32_t random_coeff_h[4], const bfhip_conventions* conv, uint32_t out_h[4]);

/* The prover session. One open session per context: bfhip_pcs_create waits for the context's streams and resets its arena as a proof does;
 * the session's polynomials, LDE columns, Merkle layers, quotients and FRI layers live in the arena until bfhip_pcs_destroy, which puts the
 * arena's bookkeeping (bfhip_ctx_memory out[3]) back to what it was. Conventions, hasher and PcsConfig are the context's at creation.
 * While a session is open these entry points of its context return -1 with "a commitment-scheme session is open" — they reset, or borrow
 * from, the arena, or change what the session was created under:
 *   bfhip_prove_trace, bfhip_prove_brainfuck, bfhip_prove_registers (and every pool job or batch that lands on the context),
 *   bfhip_trace_create, bfhip_trace_create_ram, bfhip_trace_create_from_registers (the GPU table builders' scratch),
 *   bfhip_trace_check, bfhip_check_constraints, bfhip_relation_summary, bfhip_trace_relations, bfhip_relation_program_summary,
 *   bfhip_relation_program_multiplicities,
 *   bfhip_ctx_set_conventions, bfhip_ctx_set_pcs_config, bfhip_ctx_join_local_group, bfhip_ctx_join_rccl_group, bfhip_ctx_destroy,
 *   bfhip_air_prove (it opens a session of its own),
 *   and a second bfhip_pcs_create.
 * Everything else keeps working, which is what the caller's constraint sweep needs: bfhip_malloc / bfhip_free / bfhip_upload / bfhip_download /
 * bfhip_memset_zero, bfhip_interpolate, bfhip_evaluate, bfhip_is_first_coeffs, bfhip_is_first_lde, bfhip_eval_at_point, bfhip_logup_generate, bfhip_eval_constraints,
 * bfhip_air_eval_domain, bfhip_air_kernel_eval_domain (and bfhip_air_compile), bfhip_logup_program_generate, bfhip_columns_from_rows, bfhip_rows_from_columns, bfhip_accumulate, the Merkle / fold / grind / gather single operations, resident traces' getters and the profiler.
 * Not supported: a context in a shard group (create refuses; joining refuses while a session is open); a pool's sub-context while anything
 * is queued, running or not yet taken on the pool.
 * Launch order: the plain one only (wait, draw, copy, launch). No mailbox order, and the overlap mask (bfhip_ctx_set_overlap) is ignored.
 * Columns are full size: 2^log_size words each (no row-granular storage).
 *
 * bfhip_pcs_commit: n_cols device columns, column k of 2^log_sizes_h[k] words, in the caller's order; sizes in any order, repeats allowed.
 *   form 0: evaluations on CanonicCoset(log_size).circle_domain() in bit-reversed order (interpolated here); form 1: coefficients, what
 *   bfhip_interpolate produces (stwo commits the composition polynomial this way). The columns are borrowed for the call and not modified.
 *   The root is mixed into ch and returned (Poseidon252: canonical little-endian bytes of the felt252).
 * bfhip_pcs_tree_columns: per column of committed tree `tree` the device pointers of its coefficients (2^log_size words) and of its LDE
 *   (2^(log_size + log_blowup_factor) words, bit-reversed), valid until bfhip_pcs_destroy; either array may be NULL, both NULL: *n_cols only;
 *   -2 = cap too small.
 * bfhip_pcs_prove_values: points_h = n_points points (8 words each). For every column of every tree, in commit order, n_samples_h[] counts
 *   its samples and point_idx_h lists them as indices into points_h, in the order the sampled values are to appear. It samples every
 *   (column, point), mixes the sampled values, draws the quotient coefficient, accumulates the quotients per LDE size, runs the FRI commit
 *   phase, grinds, draws the queries and decommits. *proof_json = the serde form of CommitmentSchemeProof {commitments, sampled_values,
 *   decommitments, queried_values, proof_of_work, fri_proof} — byte for byte the "proof" member of a BrainfuckProof — malloc'd, release
 *   with bfhip_free_host. sampled_out_h (optional): the sampled values flat, 4 words each, same order. A column without samples is
 *   committed and decommitted but enters no quotient. The call ends the session's proving life, also when it fails after its checks:
 *   only bfhip_pcs_tree_columns and bfhip_pcs_destroy remain. A failure waits for the context's streams before it returns.
 * Caps (each refused with a message that names it; none grows a kernel):
 *   log_size                 4 <= log_size <= max_log_domain - log_blowup_factor (the twiddle tree; the Brainfuck path uses every size from 4)
 *   samples per column       <= 2 = BFHIP_PCS_MAX_SAMPLES_PER_COLUMN (the quotient tables hold two (point, value) pairs per column)
 *   points                   <= 64 = BFHIP_PCS_MAX_POINTS (fixed tables of the batch builder); two indices may name equal points: one batch
 *   columns per tree         <= 4096 = BFHIP_PCS_MAX_COLUMNS (descriptors, pointer arrays and pass tables of one commitment share the 8 MiB staging ring)
 *   trees                    <= 64 = BFHIP_PCS_MAX_TREES
 *   FRI layers               <= 40 (FRI_MAX_LAYERS of the commit phase): cannot be exceeded, the largest LDE has at most 2^29 rows
 *   quotient columns         one per distinct LDE size by construction: "two quotient columns of one size" cannot arise
 *   at least one tree and one column per tree; log_last_layer_degree_bound 0; Poseidon252 channel: pow_bits <= 12 (refused at prove_values). */
enum { BFHIP_PCS_MAX_SAMPLES_PER_COLUMN = 2, BFHIP_PCS_MAX_POINTS = 64, BFHIP_PCS_MAX_COLUMNS = 4096, BFHIP_PCS_MAX_TREES = 64 };
typedef struct bfhip_pcs bfhip_pcs;
int32_t bfhip_pcs_create(bfhip_ctx* ctx, bfhip_pcs** out);
int32_t bfhip_pcs_destroy(bfhip_pcs* pcs);
int32_t bfhip_pcs_commit(bfhip_pcs* pcs, bfhip_channel* ch, const uint32_t* const* cols_h, const uint32_t* log_sizes_h, uint32_t n_cols, int32_t form, uint8_t root_out[32]);
int32_t bfhip_pcs_tree_columns(bfhip_pcs* pcs, uint32_t tree, const uint32_t** coeffs_d_out, const uint32_t** lde_d_out, uint32_t cap, uint32_t* n_cols);
int32_t bfhip_pcs_prove_values(bfhip_pcs* pcs, bfhip_channel* ch, const uint32_t* points_h, uint32_t n_points, const uint32_t* n_samples_h,
                               const uint32_t* point_idx_h, uint32_t* sampled_out_h, char** proof_json, size_t* proof_len);

/* The verifier session (host only). create: the conventions and PcsConfig the proof was made under (NULL = defaults).
 * commit = CommitmentSchemeVerifier::commit: the TRACE-domain log sizes of the tree's columns (the blowup is added inside, 1 <= log_size <=
 * 30 - log_blowup_factor); mixes the root into ch. verify_values: the same point / index description as bfhip_pcs_prove_values;
 * 0 = accepted, 1 = rejected (VerificationError name in err, the names of bfhip_verify_brainfuck), -1 = internal / bad arguments.
 * The proof's commitments must equal the roots committed above. */
typedef struct bfhip_pcs_verifier bfhip_pcs_verifier;
int32_t bfhip_pcs_verifier_create(const bfhip_conventions* conv, const bfhip_pcs_config* pcs, bfhip_pcs_verifier** out);
int32_t bfhip_pcs_verifier_destroy(bfhip_pcs_verifier* v);
int32_t bfhip_pcs_verifier_commit(bfhip_pcs_verifier* v, bfhip_channel* ch, const uint8_t root[32], const uint32_t* log_sizes_h, uint32_t n_cols);
int32_t bfhip_pcs_verifier_verify_values(bfhip_pcs_verifier* v, bfhip_channel* ch, const uint32_t* points_h, uint32_t n_points, const uint32_t* n_samples_h,
                                         const uint32_t* point_idx_h, const char* proof_json, size_t proof_len, char* err, size_t err_cap);

/* ---- Constraint programs: evaluate ANY AIR's constraints, on the GPU over the constraint domain and on the host at a point ------------------
 * bfhip_eval_constraints runs one of 13 compiled-in kernels. stwo's `FrameworkEval::evaluate` hands a backend an expression, not a kernel; a
 * program is that expression as data: a flat, straight-line bytecode for one component. It is evaluated two ways:
 *   bfhip_air_eval_domain    ONE gfx950 kernel for every program, on the constraint domain: what
 *                            `ComponentProver::evaluate_constraint_quotients_on_domain` does for a FrameworkComponent (reached from mod.rs:732);
 *   bfhip_air_eval_at_point  the host evaluator at the out-of-domain point: stwo's PointEvaluator, the composition check of verify (mod.rs:738-797).
 * With the session above, bfhip_pcs_* + bfhip_air_* prove and verify an AIR this library has never seen.
 *
 * A program is n_instr instructions of four u32 words {op, dst, a, b}. Two register files: m[] holds M31 values (one word), q[] QM31 values
 * (four words). No branches; a register must be written before it is read; words an instruction does not use are ignored.
 *   BFHIP_AIR_M_COL    dst, col, off   m[dst] = column `col` at the row at trace offset `off` (b is an int32, |off| <= 16)
 *   BFHIP_AIR_M_CONST  dst, v          m[dst] = v, v < 2^31 - 1
 *   BFHIP_AIR_M_ADD / _M_SUB / _M_MUL  dst, a, b     M31 arithmetic on m[a], m[b]
 *   BFHIP_AIR_M_NEG    dst, a          m[dst] = -m[a]
 *   BFHIP_AIR_Q_COL    dst, col, off   q[dst] = the secure value whose coordinates are columns col..col+3 at offset off
 *   BFHIP_AIR_Q_PARAM  dst, i          q[dst] = params[i]: the caller's QM31 values (lookup z, alpha powers, claimed sums)
 *   BFHIP_AIR_Q_FROM_M dst, a          q[dst] = (m[a], 0, 0, 0)
 *   BFHIP_AIR_Q_ADD / _Q_SUB / _Q_MUL  dst, a, b     QM31 arithmetic on q[a], q[b]
 *   BFHIP_AIR_Q_MULM   dst, a, b       q[dst] = q[a] * m[b]
 *   BFHIP_AIR_C_BASE   -, a            the next constraint is m[a]     } constraints are numbered in program order
 *   BFHIP_AIR_C_EXT    -, a            the next constraint is q[a]     }
 * "The row at offset off" is the point of this row plus off * CanonicCoset(log_size).step(), on whichever domain is evaluated; at a point it
 * is bfhip_circle_point_offset. IsFirst is just a column the caller passes.
 * The mask of a program: the distinct (col, off) pairs it reads, ordered by column and, within a column, by first use; a Q_COL contributes its
 * four columns at the same offset. This is the order in which a caller lists a column's samples for bfhip_pcs_prove_values, and the order of
 * mask_values_h below.
 * Caps (a program beyond one is refused): 96 m registers, 24 q registers, 4096 instructions, 256 columns, 64 parameters, 64 constraints.
 *
 * bfhip_air_create (host only): validates everything — opcode, register range, read before write, col (and col + 3) within n_cols, parameter
 *   index, offset range, v < p, at least one constraint, the caps. Each refusal is -1 and names the instruction index and the rule:
 *   "bfhip_air_create: instruction <i>: <rule>" (rules about the program as a whole name the instruction count).
 * bfhip_air_shape: out = {columns, parameters, constraints, instructions, m registers used, q registers used, minimum offset, maximum offset
 *   (both int32 stored in a u32)}.
 * bfhip_air_mask: the mask in the order above; *n = its length. -2 ("capacity") when cap < *n; all of cols_out, offs_out NULL with cap 0: size query.
 * bfhip_air_eval_domain: column k of cols_h holds 2^(log_size + log_expand) cells on CanonicCoset(log_size + log_expand).circle_domain(),
 *   bit-reversed; with col_shifts_h[k] = s (0 or >= 2, as elsewhere; NULL = all 0) it holds 2^(log_size + log_expand - s) cells and is read at
 *   row >> s. A shifted column that the program reads at a non-zero offset is refused. For every row
 *       acc[row] += (sum_j coeffs[j] * C_j(row)) * 1 / coset_vanishing(CanonicCoset(log_size).coset, point(row)).
 *   params_h = 4 * n_params words, coeffs_h = 4 * n_coeffs words; the counts must be the program's. 1 <= log_expand <= 3, log_size >= 1 and
 *   log_size + log_expand <= max_log_domain. With log_expand = 1 this is bfhip_eval_constraints' contract, to the bit. Whole domains only. A
 *   context in a shard group is refused. Works while a session is open, like bfhip_eval_constraints.
 * bfhip_air_eval_at_point (host only): the same program over QM31. mask_values_h = n_mask values of 4 words in mask order; a Q_COL combines
 *   its four sampled coordinates as SecureField::from_partial_evals does; the result is multiplied by 1 / coset_vanishing at the point. */
enum { BFHIP_AIR_M_COL = 0, BFHIP_AIR_M_CONST = 1, BFHIP_AIR_M_ADD = 2, BFHIP_AIR_M_SUB = 3, BFHIP_AIR_M_MUL = 4, BFHIP_AIR_M_NEG = 5, BFHIP_AIR_Q_COL = 6,
       BFHIP_AIR_Q_PARAM = 7, BFHIP_AIR_Q_FROM_M = 8, BFHIP_AIR_Q_ADD = 9, BFHIP_AIR_Q_SUB = 10, BFHIP_AIR_Q_MUL = 11, BFHIP_AIR_Q_MULM = 12, BFHIP_AIR_C_BASE = 13,
       BFHIP_AIR_C_EXT = 14 };
enum { BFHIP_AIR_MAX_M_REGS = 96, BFHIP_AIR_MAX_Q_REGS = 24, BFHIP_AIR_MAX_INSTRUCTIONS = 4096, BFHIP_AIR_MAX_COLUMNS = 256, BFHIP_AIR_MAX_PARAMS = 64,
       BFHIP_AIR_MAX_CONSTRAINTS = 64, BFHIP_AIR_MAX_OFFSET = 16 };
typedef struct bfhip_air bfhip_air;
int32_t bfhip_air_create(const uint32_t* code, size_t n_words, uint32_t n_cols, uint32_t n_params, bfhip_air** out);
int32_t bfhip_air_destroy(bfhip_air* air);
int32_t bfhip_air_shape(const bfhip_air* air, uint32_t out[8]);
int32_t bfhip_air_mask(const bfhip_air* air, uint32_t* cols_out, int32_t* offs_out, uint32_t cap, uint32_t* n);
int32_t bfhip_air_eval_domain(bfhip_ctx* ctx, const bfhip_air* air, uint32_t log_size, uint32_t log_expand, const uint32_t* const* cols_h, const uint32_t* col_shifts_h,
                              const uint32_t* params_h, uint32_t n_params, const uint32_t* coeffs_h, uint32_t n_coeffs, uint32_t* const acc_d[4]);
int32_t bfhip_air_eval_at_point(const bfhip_air* air, uint32_t log_size, const uint32_t point_h[8], const uint32_t* mask_values_h, uint32_t n_mask,
                                const uint32_t* params_h, uint32_t n_params, const uint32_t* coeffs_h, uint32_t n_coeffs, uint32_t out_h[4]);

/* ---- Compiled constraint programs: an AIR's own gfx950 kernel, generated and compiled at run time ---------------------------------------------
 * bfhip_air_eval_domain interprets: per instruction a scalar fetch, a branch and an LDS round trip per operand. A program is straight-line code
 * whose registers are written before they are read, so it translates in one pass into HIP source with every value a named local, which
 * libhiprtc (part of ROCm; opened with dlopen at the first compile, never linked) compiles in-process for the device's architecture. The
 * interpreter stays: it needs no compile time, and it is what a compiled kernel is held to, bit for bit.
 * bfhip_air_source (host only, no GPU): the generated source, without a terminating NUL; *len = its length. -2 ("capacity") when cap < *len;
 *   buf NULL with cap 0: size query. The same program gives the same bytes. Compiled with -DBFHIP_AIR_GEN_HOST the text is plain C++ (the
 *   row function `bfair::air_row(const bfair::Launch*, uint32_t row)` without the kernel wrapper).
 * bfhip_air_compile: generates, compiles (-O3 -std=c++17, --offload-arch = the device's gcnArchName as reported) and loads the kernel. The
 *   kernel keeps its own copy of the program: the program may be destroyed. A context keeps one module per distinct source: compiling an
 *   equal program again while a kernel of it is alive does not run the compiler (bfhip_air_kernel_info out[7] = 1). -1 when libhiprtc or
 *   one of its symbols is missing (the message names it) and when the compiler fails (the message carries its log, truncated). Nothing is
 *   written to disk. One kernel serves every log_size, log_expand in 1..3, shift pattern and parameter set.
 * bfhip_air_kernel_eval_domain: bfhip_air_eval_domain with the kernel in place of the program — the same arguments, the same checks with
 *   the same messages (they name bfhip_air_eval_domain), the same one copy through the staging ring, no arena use (works while a session
 *   is open), the same result to the bit. ctx must be the context that compiled the kernel; a context in a shard group is refused.
 * bfhip_air_kernel_info: out = {VGPRs, SGPRs (0xffffffff if the code object does not say), private-segment (scratch) bytes per lane, static
 *   LDS bytes, code-object bytes, source bytes, generate + compile + load time in microseconds (of the compile that built the module), 1 if
 *   the context's cache served this kernel}. Scratch above 0 is reported, not refused.
 * bfhip_air_kernel_destroy: the module is unloaded when its last kernel goes (after a wait for the context's stream).
 * bfhip_ctx_destroy with live kernels cleans up: it unloads their modules; the kernel objects stay valid to destroy, and to nothing else
 *   (eval_domain and info return -1). */
typedef struct bfhip_air_kernel bfhip_air_kernel;
int32_t bfhip_air_source(const bfhip_air* air, char* buf, size_t cap, size_t* len);
int32_t bfhip_air_compile(bfhip_ctx* ctx, const bfhip_air* air, bfhip_air_kernel** out);
int32_t bfhip_air_kernel_eval_domain(bfhip_ctx* ctx, bfhip_air_kernel* kernel, uint32_t log_size, uint32_t log_expand, const uint32_t* const* cols_h,
                                     const uint32_t* col_shifts_h, const uint32_t* params_h, uint32_t n_params, const uint32_t* coeffs_h, uint32_t n_coeffs,
                                     uint32_t* const acc_d[4]);
int32_t bfhip_air_kernel_info(bfhip_air_kernel* kernel, uint32_t out[8]);
int32_t bfhip_air_kernel_destroy(bfhip_air_kernel* kernel);

/* ---- Composition: ALL components of an AIR to the composition polynomial's four coefficient columns, in one call ----------------------------
 * `ComponentProvers::compute_composition_polynomial` (reached from prover::prove) for an AIR given as programs: what a caller of
 * bfhip_air_eval_domain otherwise does by hand — coefficient slices, one sweep and one accumulator pass per component, one interpolation per
 * size, the additions of DomainEvaluationAccumulator::finalize — and its mirror at a point for the verifier. No channel, no session, no
 * protocol: the caller draws random_coeff and commits the result (bfhip_pcs_commit, form 1).
 *
 * Coefficients. T = the sum of the components' constraint counts. The constraint with global index g (components in list order, constraints
 *   in program order) gets random_coeff^(T - 1 - g): what `accum.columns()` hands the components on the domain and what
 *   PointEvaluationAccumulator's Horner sum gives at a point. bfhip_air_compose_coeffs (host only) writes these T values of 4 words in global
 *   order, so that a caller who sweeps component by component uses the same numbers; a count outside 1..64 constraints is refused.
 * Buckets. Component k is evaluated on the domain of el_k = log_size_k + log_expand_k. Components of equal el share an accumulator, whatever
 *   their log_size. For every row of a bucket the accumulator holds the sum, over the bucket's components in list order, of
 *       (sum_j coeff_j C_j(row)) * 1 / coset_vanishing(CanonicCoset(log_size_k).coset, point(row)):
 *   for a single component bfhip_air_eval_domain's value from a zero accumulator, bit for bit.
 * Finalize. Each bucket is interpolated on its own domain and the smaller buckets' coefficients are added onto the prefix of the largest
 *   one: evaluating a polynomial on a larger domain is zero extension of its coefficients, and interpolation is linear. dst_d receives the 4
 *   coefficient columns of 2^dst_log words, overwritten, not accumulated. dst_log must equal max_k el_k; another value is refused and the
 *   message names the expected one.
 * bfhip_air_compose: the interpreted components (kernel == NULL) run in one gfx950 kernel in which a wave owns 64 rows of a bucket, walks the
 *   bucket's components and writes the row's sum once, with no read and no zero fill (one launch for all buckets below 2^16 rows, one per
 *   larger bucket: DESIGN.md section 9n); a component given as its compiled kernel (this
 *   context's bfhip_air_compile; program may then be NULL) runs after that, one launch each, and adds into its bucket. Then one batched
 *   inverse transform over all buckets and the additions. Works while a commitment-scheme session is open and takes nothing from the arena:
 *   with more than one bucket it makes one hipMalloc of at most 16 * 2^dst_log bytes for the smaller buckets' accumulators (the largest
 *   accumulates in dst_d), freed before return (the call then waits for the stream); with one bucket it allocates nothing and does not
 *   wait. A context in a shard group is refused.
 *   Refusals: -1 with "bfhip_air_compose: component <k>: <rule>", or "bfhip_air_compose: <rule>" for a rule about the list; nothing has
 *   been enqueued and the context stays usable. n outside 1..64, null pointers, reserved != 0, neither program nor kernel, a kernel of
 *   another context, every rule of bfhip_air_eval_domain about one component (log_expand, log_size, max_log_domain, shifts, a shifted
 *   column read at an offset, the parameter count, canonical words), a non-canonical random_coeff, dst_log != max_k el_k, and a list
 *   whose staged blocks do not fit the context's staging ring (the message names the bytes).
 * bfhip_air_compose_at_point (host only, plain C++): `Components::eval_composition_polynomial_at_point` — for every component
 *   bfhip_air_eval_at_point under its slice of the coefficients, summed. Refusals as above, in its own name.
 * Layouts (natural alignment, LP64):
 *   bfhip_air_component        56 bytes: program 0, kernel 8, log_size 16, log_expand 20, cols_h 24, col_shifts_h 32, params_h 40, n_params 48,
 *                              reserved 52
 *   bfhip_air_point_component  40 bytes: program 0, log_size 8, n_mask 12, mask_values_h 16, params_h 24, n_params 32, reserved 36 */
enum { BFHIP_AIR_COMPOSE_MAX_COMPONENTS = 64 };
typedef struct bfhip_air_component {
    const bfhip_air*  program;      /* interpreted when kernel == NULL */
    bfhip_air_kernel* kernel;       /* optional: the component's compiled kernel (this context's); program may then be NULL */
    uint32_t log_size, log_expand;  /* as for bfhip_air_eval_domain */
    const uint32_t* const* cols_h;  /* columns on CanonicCoset(log_size + log_expand).circle_domain(), bit-reversed */
    const uint32_t* col_shifts_h;   /* NULL = all 0; same rules as bfhip_air_eval_domain */
    const uint32_t* params_h; uint32_t n_params, reserved;   /* reserved must be 0 */
} bfhip_air_component;
int32_t bfhip_air_compose_coeffs(const uint32_t* n_constraints_h, uint32_t n, const uint32_t random_coeff_h[4], uint32_t* coeffs_out /* 4 * T words */);
int32_t bfhip_air_compose(bfhip_ctx* ctx, const bfhip_air_component* comps, uint32_t n, const uint32_t random_coeff_h[4],
                          uint32_t dst_log, uint32_t* const dst_d[4]);
typedef struct bfhip_air_point_component {
    const bfhip_air* program; uint32_t log_size, n_mask;
    const uint32_t* mask_values_h; const uint32_t* params_h; uint32_t n_params, reserved;
} bfhip_air_point_component;
int32_t bfhip_air_compose_at_point(const bfhip_air_point_component* comps, uint32_t n, const uint32_t point_h[8],
                                   const uint32_t random_coeff_h[4], uint32_t out_h[4]);

/* ---- Constraint programs asserted on the trace domain: which constraint of ANY AIR is non-zero at which cell ---------------------------------
 * stwo's `assert_constraints` for a program, the generic counterpart of bfhip_check_constraints (which runs one of 13 compiled-in AIRs). A wrong
 * trace cell or a wrongly written constraint otherwise shows only after a whole commit, sweep and open, as a sampled composition value that is
 * not bfhip_air_eval_at_point's ("OodsNotMatching"), naming neither constraint nor row. bfhip_air_eval_domain cannot stand in: it folds all
 * constraints into one accumulator under random coefficients and divides by a polynomial that is zero on the trace domain.
 *
 * bfhip_air_check: ONE gfx950 interpreter kernel over CanonicCoset(log_size) itself, then one wave at the first bad cell, ONE read-back. No
 *   coefficients, no vanishing polynomial, no accumulator; constraints are numbered in program order. Column k of cols_h holds 2^log_size
 *   cells of CanonicCoset(log_size).circle_domain(), bit-reversed; with col_shifts_h[k] = s (0, or 2 <= s <= log_size; NULL = all 0) it holds
 *   2^(log_size - s) cells and is read at cell >> s. A shifted column that the program reads at a non-zero offset is refused. "The row at
 *   offset off" is the point plus off * CanonicCoset(log_size).step() on the trace domain itself: a move of off in coset order, the order
 *   finalize_last's prefix sum runs in (bfhip_logup_program_generate). IsFirst is a column the caller passes: 1 at cell 0. A cell is a storage
 *   index, as in bfhip_check_report. params_h = 4 * n_params canonical words; the count must be the program's. 1 <= log_size <= max_log_domain.
 *   A context in a shard group is refused. Works while a session is open (its scratch is not the arena's: bfhip_ctx_memory out[3] is
 *   unchanged by the call). Returns 0 whether or not the trace is valid — the verdict is in *out, and bfhip_last_error() is not touched by
 *   violations; -1 only for bad arguments and HIP errors, with "bfhip_air_check: <rule>". Every field is an integer and does not depend on
 *   the schedule. A trace that is wrong everywhere costs up to 130 atomics per 64 cells; a valid one costs its loads.
 * bfhip_format_air_check (host only, no GPU): "air check: ok" for a report without violations; otherwise, lines joined by '\n':
 *   "air check: <n> of <N> cells violate <k> of <K> constraints", then one line per failing constraint in constraint order:
 *   "constraint <j>: <n> cells, first at cell <i>", with ", value (a, b, c, d)" appended for first_bad_constraint. buf / cap / need / -2 as in
 *   bfhip_format_preflight.
 * Layout (natural alignment, declaration order):
 *   bfhip_air_check_report  1088 bytes: log_size 0, n_constraints 4, n_bad_cells 8, first_bad_cell 16, first_bad_constraint 24, reserved0 28,
 *                                       first_bad_value 32, bad_per_constraint 48, first_cell_per_constraint 560, reserved 1072 */
typedef struct bfhip_air_check_report {
    uint32_t log_size, n_constraints;
    uint64_t n_bad_cells;                     /* cells where at least one constraint is non-zero */
    uint64_t first_bad_cell;                  /* lowest such storage index; UINT64_MAX if none */
    int32_t  first_bad_constraint;            /* lowest constraint that is non-zero there; -1 if none */
    uint32_t reserved0;
    uint32_t first_bad_value[4];              /* its value there; a C_BASE constraint as (v, 0, 0, 0) */
    uint64_t bad_per_constraint[64];          /* cells where constraint j is non-zero (BFHIP_AIR_MAX_CONSTRAINTS) */
    uint64_t first_cell_per_constraint[64];   /* lowest cell where constraint j is non-zero; UINT64_MAX if none or j >= n_constraints */
    uint64_t reserved[2];
} bfhip_air_check_report;
int32_t bfhip_air_check(bfhip_ctx* ctx, const bfhip_air* air, uint32_t log_size, const uint32_t* const* cols_h, const uint32_t* col_shifts_h,
                        const uint32_t* params_h, uint32_t n_params, bfhip_air_check_report* out);
int32_t bfhip_format_air_check(const bfhip_air_check_report* rep, char* buf, size_t cap, size_t* need);

/* ---- Fraction programs: the logUp interaction trace of ANY AIR, on the GPU over the trace domain ---------------------------------------------
 * bfhip_logup_generate runs one of 13 compiled-in branches (`interaction_trace_evaluation` of memory/table.rs:485-518, processor/table.rs:456-529,
 * ...: the calls prove makes at mod.rs:596-687) and is built on their 16-fold replicated rows. A fraction program is what such a function hands
 * to LogupTraceGenerator::{new_col, write_frac, finalize_col, finalize_last}, as data: a constraint program's bytecode (same four-word
 * instructions, same two register files, same caps: 96 m registers, 24 q registers, 4096 instructions, 256 columns, 64 parameters) without
 * constraints and with two opcodes that exist only here:
 *   BFHIP_LOGUP_FRAC     -, a, b   add the fraction q[a] / q[b] to the open logUp column (write_frac)
 *   BFHIP_LOGUP_END_COL  -         close the open column (finalize_col); the next FRAC opens the next one (new_col)
 * The value of logUp column k at a cell is the value of column k - 1 at that cell (0 for k = 0) plus the sum of column k's fractions at that
 * cell. Fractions are field elements: the sum is a value, not an evaluation order (n1/d1 + n2/d2 and (n1 d2 + n2 d1)/(d1 d2) are the same
 * canonical words). The last column is then replaced by its inclusive prefix sum in coset order (finalize_last: coset index i is circle-domain
 * index coset_index_to_circle_domain_index(i, log_size), stored bit-reversed — the order the row at offset -1 of a constraint program steps
 * backwards through), and the claimed sum is the last coset element of that prefix sum: the sum of the last column's per-cell values over
 * all cells. With bfhip_pcs_* and bfhip_air_* this proves an AIR with lookups that the library has never seen.
 *
 * bfhip_logup_create (host only): every rule of bfhip_air_create (opcode, register range, read before write, col and col + 3 within n_cols,
 *   parameter index, v < p, the instruction / column / parameter caps), and: C_BASE and C_EXT are refused; M_COL and Q_COL at a non-zero offset
 *   are refused (the generator reads a row's own cells: a "next" value is a column); a FRAC that no END_COL follows, an END_COL with no FRAC
 *   since the previous one, a program without any column, more than 8 = BFHIP_LOGUP_MAX_COLUMNS columns or 32 = BFHIP_LOGUP_MAX_FRACTIONS
 *   fractions are refused. Each refusal is -1 with "bfhip_logup_create: instruction <i>: <rule>" (rules about the program as a whole name the
 *   instruction count). bfhip_air_create keeps refusing opcodes 15 and 16.
 * bfhip_logup_shape: out = {columns, parameters, logUp columns, fractions, instructions, m registers used, q registers used, 0}.
 * bfhip_logup_program_generate: column k of cols_h holds 2^log_size cells of CanonicCoset(log_size).circle_domain(), bit-reversed; with
 *   col_shifts_h[k] = s (0 or >= 2; NULL = all 0) it holds 2^(log_size - s) cells and is read at cell >> s. out_cols_h = 4 * n_logup_columns
 *   device pointers, every one a full-size coordinate column of 2^log_size cells (no row-granular output). params_h = 4 * n_params canonical
 *   words; the count must be the program's. 1 <= log_size <= max_log_domain. claimed_sum_h = u32[4]. A context in a shard group is refused.
 *   Works while a session is open (its scratch is not the arena's). Scratch: one hipMalloc of at most
 *       24 * 2^log_size + 2^log_size / 128 + 64 bytes,
 *   freed before the call returns; a failed allocation is -1 with "bfhip_logup_program_generate: cannot allocate <n> bytes of scratch".
 *   A zero denominator (stwo panics there) is -1 with "bfhip_logup_program_generate: fraction <f> has a zero denominator at cell <c>": <c> the
 *   lowest such cell (storage index), <f> the lowest such fraction (numbered in program order from 0) at that cell; the outputs are then
 *   unspecified and the context stays usable. */
enum { BFHIP_LOGUP_FRAC = 15, BFHIP_LOGUP_END_COL = 16, BFHIP_LOGUP_MAX_COLUMNS = 8, BFHIP_LOGUP_MAX_FRACTIONS = 32 };
typedef struct bfhip_logup bfhip_logup;
int32_t bfhip_logup_create(const uint32_t* code, size_t n_words, uint32_t n_cols, uint32_t n_params, bfhip_logup** out);
int32_t bfhip_logup_destroy(bfhip_logup* lp);
int32_t bfhip_logup_shape(const bfhip_logup* lp, uint32_t out[8]);
int32_t bfhip_logup_program_generate(bfhip_ctx* ctx, const bfhip_logup* lp, uint32_t log_size, const uint32_t* const* cols_h, const uint32_t* col_shifts_h,
                                     const uint32_t* params_h, uint32_t n_params, uint32_t* const* out_cols_h, uint32_t claimed_sum_h[4]);

/* ---- Fraction programs, batched: the logUp interaction trace of ALL components of an AIR, in one call ---------------------------------------
 * The calls prove makes to every component's `interaction_trace_evaluation` (mod.rs:596-687) for an AIR given as fraction programs: what a
 * caller of bfhip_logup_program_generate otherwise does component by component, each call with its own allocation, staging, four launches,
 * blocking read-back and free. No channel, no session, no protocol: the caller mixes the claimed sums and commits the columns.
 *
 * Semantics. For every component k the output columns and claimed_sums_h[4 k .. 4 k + 3] are exactly what bfhip_logup_program_generate
 *   produces for that component alone, word for word (the field arithmetic is exact). total_h, when not NULL, receives the sum of the n
 *   claimed sums: what `lookup_sum_valid` tests against zero.
 * Launches. Row stage: one gfx950 kernel in which a wave owns 64 consecutive cells of one component, which it finds in a table; one
 *   launch for all components, except that a component of 2^16 cells and more gets a launch of its own when the register files of the
 *   list's largest program would lower its occupancy. Scan stage: three launches for the whole list (tiles, tile
 *   totals, last column).
 * Cost. One hipMalloc, of at most the sum over the list of bfhip_logup_program_generate's stated bound
 *       24 * 2^log_size + 2^log_size / 128 + 64 bytes,
 *   one read-back of 32 * n bytes, one hipFree. Nothing is taken from the arena: the call works while a commitment-scheme session is open
 *   and bfhip_ctx_memory out[3] does not move. Programs, descriptors, parameters and the lookup tables of the launches go through the
 *   context's staging ring; a program that appears several times in the list is staged once. A failed allocation is -1 with
 *   "bfhip_logup_program_generate_batch: cannot allocate <n> bytes of scratch".
 * Zero denominators. Each component keeps its own record. The call is -1 with
 *   "bfhip_logup_program_generate_batch: component <k>: fraction <f> has a zero denominator at cell <c>", <k> the lowest component index that
 *   has one, <f> and <c> as for bfhip_logup_program_generate. The outputs (claimed_sums_h and total_h too) are then unspecified, nothing
 *   faults and the context stays usable.
 * Refusals: -1 with "bfhip_logup_program_generate_batch: component <k>: <rule>", or "bfhip_logup_program_generate_batch: <rule>" for a rule
 *   about the list; nothing has been enqueued and the context stays usable. n outside 1..64, null pointers (comps, claimed_sums_h; a
 *   component's program, out_cols_h, cols_h where the program has columns, params_h where n_params != 0), reserved != 0, every rule of
 *   bfhip_logup_program_generate about one component in the same words (log_size range, shifts, the parameter count, canonical words, a null
 *   column or output column pointer), a context in a shard group, a list of more than 2^31 cells in all (the message names the count), a
 *   list whose staged blocks do not fit the context's staging ring (the message names the bytes), and an output column whose byte range — 4 * 2^log_size bytes; an input column of shift s has
 *   4 * 2^(log_size - s) — shares a byte with an input column or with another output column anywhere in the list: the components run side
 *   by side. The message names the two components. Input columns may be shared.
 * Layout (natural alignment, LP64):
 *   bfhip_logup_component  56 bytes: program 0, log_size 8, n_params 12, cols_h 16, col_shifts_h 24, params_h 32, out_cols_h 40, reserved 48 */
enum { BFHIP_LOGUP_BATCH_MAX_COMPONENTS = 64 };
typedef struct bfhip_logup_component {
    const bfhip_logup* program;
    uint32_t log_size, n_params;    /* as for bfhip_logup_program_generate */
    const uint32_t* const* cols_h;  /* columns on CanonicCoset(log_size).circle_domain(), bit-reversed */
    const uint32_t* col_shifts_h;   /* NULL = all 0; same rules as bfhip_logup_program_generate */
    const uint32_t* params_h;
    uint32_t* const* out_cols_h;    /* 4 * n_logup_columns device pointers, every one a full-size coordinate column */
    uint64_t reserved;              /* must be 0 */
} bfhip_logup_component;
int32_t bfhip_logup_program_generate_batch(bfhip_ctx* ctx, const bfhip_logup_component* comps, uint32_t n, uint32_t* claimed_sums_h /* 4 * n words */,
                                           uint32_t total_h[4] /* may be NULL */);

/* ---- Proving an AIR given as programs: the protocol driver and its verifier ----------------------------------------------------------------
 * `prover::prove` / `verify` for an AIR that is not the Brainfuck snapshot: the order of mixes and draws, the interaction tree's column order,
 * the coefficient draw, the constraint domain when log_blowup_factor != log_expand, the mask points, the per-column sample description, the
 * out-of-domain sanity check and the same replay on the verifier's side — what a caller of bfhip_pcs_* + bfhip_air_compose +
 * bfhip_logup_program_generate_batch otherwise writes by hand. No kernel of its own: the device work of a proof is
 * the session's launches, bfhip_air_compose's (or the compiled kernels') and the batch's, and bfhip_evaluate's where a constraint domain is
 * not the session's LDE.
 *
 * The statement: the AIR as data, shared by prover and verifier. It holds no device pointers.
 *   Caller trees, in commit order: n_cols columns with trace-domain log_sizes_h, form (0 = evaluations, 1 = coefficients: bfhip_pcs_commit's),
 *     and n_mix words mix_u64_h that are mixed with bfhip_channel_mix_u64 immediately before that tree's commit (a claim: the Brainfuck
 *     protocol mixes its 13 log sizes in front of tree 1).
 *   n_relations: the number of lookup-element draws; draw r is one draw_felts(2) = (z_r, alpha_r).
 *   Components, in list order: the constraint program, log_size, log_expand in 1..3, an optional fraction program (NULL = none), and
 *     col_trees_h[c] / col_columns_h[c] for every column c of the constraint program: a caller tree and a column of it, or
 *       BFHIP_AIR_TREE_INTERACTION and j = the j-th of this component's own 4 * n_logup_columns interaction coordinate columns (logUp
 *       columns in program order, four coordinates each); only a component with a fraction program may use it;
 *     frac_trees_h[c] / frac_columns_h[c] for every column c of the fraction program: a caller tree of form 0 and a column of it;
 *     params_h: one rule per parameter of the constraint program —
 *       BFHIP_AIR_PARAM_CONST             value[4]
 *       BFHIP_AIR_PARAM_LOOKUP_Z          z of relation `relation`
 *       BFHIP_AIR_PARAM_LOOKUP_ALPHA_POW  alpha^power of relation `relation`, power <= 63 = BFHIP_AIR_STATEMENT_MAX_POWER
 *       BFHIP_AIR_PARAM_CLAIMED_SUM       this component's own claimed sum (needs a fraction program)
 *     The fraction program's parameters are the first n_params(fractions) rules of the same table; none of them may be CLAIMED_SUM.
 *
 * bfhip_air_prove. tree_cols_h[t][c] = device column c of caller tree t, 2^log_size words, full size, as for bfhip_pcs_commit.
 *   kernels (may be NULL): kernels[k], where not NULL, is component k's bfhip_air_kernel of this context, compiled from the statement's
 *   program; it is handed to bfhip_air_compose in place of the program. ch is the caller's channel and may already carry mixes.
 *   The protocol, in this order (normative):
 *    1. bfhip_pcs_create. A context with an open session, or one in a shard group, is refused.
 *    2. per caller tree: mix_u64 of its words, then bfhip_pcs_commit.
 *    3. draw_felts(2) = (z_r, alpha_r) for r = 0 .. n_relations - 1.
 *    4. if any component has a fraction program: ONE bfhip_logup_program_generate_batch over those components in list order, into columns
 *       of the driver; mix_felts([claimed_k]) per such component in list order; bfhip_pcs_commit of the interaction tree in form 0
 *       (components in list order, logUp columns in program order, four coordinates each). Otherwise there is no interaction tree.
 *    5. random_coeff = draw_felt().
 *    6. ONE bfhip_air_compose over all components. Component k reads its columns on CanonicCoset(log_size + log_expand).circle_domain():
 *       where log_expand == log_blowup_factor the session's own LDE columns (bfhip_pcs_tree_columns), otherwise the tree's coefficient
 *       columns evaluated on that domain (bfhip_evaluate) into scratch — an LDE of another blowup is no superset of it. Only the columns
 *       some component reads are evaluated, once per (column, log_expand).
 *    7. bfhip_pcs_commit of the four composition columns in form 1, log size max_k(log_size_k + log_expand_k).
 *    8. oods = draw_point(). Point 0 is oods; then one point per distinct (log_size, offset != 0) in order of first use — components in
 *       list order, within a component bfhip_air_mask's order — bfhip_circle_point_offset(oods, log_size, offset). A column's samples
 *       are the points of all components that read it, in first-use order, each once; a column no component reads gets none; the
 *       composition columns get [0].
 *    9. bfhip_pcs_prove_values.
 *   10. The sanity check of prover::prove: the sampled composition value (from_partial_evals of the four coordinates) must equal
 *       bfhip_air_compose_at_point over the sampled mask values; otherwise -1 with "bfhip_air_prove: ConstraintsNotSatisfied".
 *   11. *proof_json = {"claimed_sums":[...],"proof":<CommitmentSchemeProof>}: one SecureField per component with a fraction program, in
 *       the serde form of interaction_claim.*.claimed_sum; the "proof" member is byte for byte what bfhip_pcs_prove_values returned.
 *       malloc'd, release with bfhip_free_host.
 *   flags: BFHIP_AIR_PROVE_CHECK — after step 4's batch, bfhip_air_check on every component over the trace-domain columns (every tree a
 *     component binds must then be form 0); a violation is -1 with "bfhip_air_prove: component <k>: " and the first failing line of
 *     bfhip_format_air_check.
 *   Validation: everything the statement alone decides is checked by one host function before anything is enqueued and before the session
 *     opens; bfhip_air_verify runs the same function. -1 with "bfhip_air_prove: component <k>: <rule>", "bfhip_air_prove: tree <t>: <rule>"
 *     or "bfhip_air_prove: <rule>"; the context stays usable. Caps: trees <= 8, relations <= 16, components <= 64; null pointers and
 *     reserved fields; column and tree indices in range; a bound column's log_size equal to the component's; 4 <= log_size <=
 *     max_log_domain - max(log_blowup_factor, log_expand); as many rules as the constraint program has parameters, at least as many as
 *     the fraction program has; relation and power indices in range; CLAIMED_SUM without, or among the parameters of, a fraction program;
 *     a fraction column bound to a form-1 tree; BFHIP_AIR_TREE_INTERACTION without a fraction program; a column that would be opened at
 *     more than BFHIP_PCS_MAX_SAMPLES_PER_COLUMN points (the message names it); more than BFHIP_PCS_MAX_POINTS points. A failure of a
 *     call the driver makes comes back as "bfhip_air_prove: " + that call's message (in the batch's, a component index counts the
 *     components with a fraction program).
 *   Memory: the driver's own buffers (interaction columns, composition columns, constraint-domain scratch) are ONE hipMalloc (or one
 *     request to the context's scratch reserve, bfhip_ctx_set_scratch_reserve), not the session's arena, freed before return on every path after a wait for the context's streams; the session is destroyed on every
 *     path: bfhip_ctx_memory out[3] is what it was before the call. A failed allocation is -1 with "bfhip_air_prove: cannot allocate <n> bytes
 *     ...", before the session opens. After a failure behind that point the channel has advanced: replay with a fresh one.
 * bfhip_air_verify (host only, plain C++): replays steps 2 to 8 with the roots of proof.commitments (bfhip_pcs_verifier_commit, trace-domain
 *   log sizes), tests the claimed sums' total ("InvalidLookup: Invalid LogUp sum", where the Brainfuck verifier tests it: after the draws of
 *   step 3), compares bfhip_air_compose_at_point over proof.sampled_values with the sampled composition value ("OodsNotMatching") and calls
 *   bfhip_pcs_verifier_verify_values, whose rejection names pass through. A proof that does not parse, or a wrong number of commitments,
 *   sampled columns, samples or claimed sums is "InvalidStructure". conv / pcs (NULL = defaults): what the proof was made under.
 *   0 = accepted, 1 = rejected (the name in err), -1 = bad arguments (the validator's refusals, in bfhip_air_verify's name).
 * Layouts (natural alignment, LP64):
 *   bfhip_air_statement_tree       32 bytes: n_cols 0, form 4, log_sizes_h 8, mix_u64_h 16, n_mix 24, reserved 28
 *   bfhip_air_param_rule           32 bytes: kind 0, relation 4, power 8, reserved 12, value 16
 *   bfhip_air_statement_component  72 bytes: program 0, fractions 8, log_size 16, log_expand 20, col_trees_h 24, col_columns_h 32,
 *                                  frac_trees_h 40, frac_columns_h 48, params_h 56, n_params 64, reserved 68
 *   bfhip_air_statement            32 bytes: trees 0, components 8, n_trees 16, n_relations 20, n_components 24, reserved 28 */
enum { BFHIP_AIR_TREE_INTERACTION = 255, BFHIP_AIR_PROVE_CHECK = 1, BFHIP_AIR_STATEMENT_MAX_TREES = 8, BFHIP_AIR_STATEMENT_MAX_RELATIONS = 16,
       BFHIP_AIR_STATEMENT_MAX_POWER = 63 };
enum { BFHIP_AIR_PARAM_CONST = 0, BFHIP_AIR_PARAM_LOOKUP_Z = 1, BFHIP_AIR_PARAM_LOOKUP_ALPHA_POW = 2, BFHIP_AIR_PARAM_CLAIMED_SUM = 3 };
typedef struct bfhip_air_statement_tree {
    uint32_t n_cols, form;            /* form: 0 = evaluations, 1 = coefficients */
    const uint32_t* log_sizes_h;      /* n_cols trace-domain log sizes */
    const uint64_t* mix_u64_h;        /* n_mix words mixed in front of this tree's commit; may be NULL when n_mix = 0 */
    uint32_t n_mix, reserved;         /* reserved must be 0 */
} bfhip_air_statement_tree;
typedef struct bfhip_air_param_rule {
    uint32_t kind, relation, power, reserved;   /* BFHIP_AIR_PARAM_*; reserved must be 0 */
    uint32_t value[4];                          /* BFHIP_AIR_PARAM_CONST */
} bfhip_air_param_rule;
typedef struct bfhip_air_statement_component {
    const bfhip_air* program;
    const bfhip_logup* fractions;     /* NULL = the component has no lookups */
    uint32_t log_size, log_expand;
    const uint32_t* col_trees_h;      /* per column of program: a caller tree, or BFHIP_AIR_TREE_INTERACTION */
    const uint32_t* col_columns_h;    /* its column in that tree / among the component's own interaction columns */
    const uint32_t* frac_trees_h;     /* per column of fractions: a caller tree of form 0 */
    const uint32_t* frac_columns_h;
    const bfhip_air_param_rule* params_h;
    uint32_t n_params, reserved;      /* reserved must be 0 */
} bfhip_air_statement_component;
typedef struct bfhip_air_statement {
    const bfhip_air_statement_tree* trees;
    const bfhip_air_statement_component* components;
    uint32_t n_trees, n_relations, n_components, reserved;   /* reserved must be 0 */
} bfhip_air_statement;
int32_t bfhip_air_prove(bfhip_ctx* ctx, const bfhip_air_statement* statement, const uint32_t* const* const* tree_cols_h, bfhip_air_kernel* const* kernels,
                        bfhip_channel* ch, uint32_t flags, char** proof_json, size_t* proof_len);
int32_t bfhip_air_verify(const bfhip_air_statement* statement, const bfhip_conventions* conv, const bfhip_pcs_config* pcs, bfhip_channel* ch,
                         const char* proof_json, size_t proof_len, char* err, size_t err_cap);
/* The sample description both of them derive from the statement (host only): the validator, then counts = {trees (caller trees, the
 * interaction tree if any, the composition tree), points, columns of all trees, point indices of all columns}. With every array NULL that is
 * all (a size query); otherwise every array is written: tree_n_cols[trees], the points as (point_log_sizes, point_offsets)[points] — point 0,
 * the drawn point itself, as (0, 0) — and n_samples[columns] / point_idx[indices] as bfhip_pcs_prove_values takes them. pcs = the PcsConfig
 * the rules are checked under (NULL = defaults), with max_log_domain 30. Refusals are the validator's, in this function's name. */
int32_t bfhip_air_statement_samples(const bfhip_air_statement* statement, const bfhip_pcs_config* pcs, uint32_t counts[4], uint32_t* tree_n_cols,
                                    uint32_t* point_log_sizes, int32_t* point_offsets, uint32_t* n_samples, uint32_t* point_idx);

/* ---- AIR statements as jobs of a pool's queue -----------------------------------------------------------------------------------------------
 * bfhip_pool_submit_air: what bfhip_air_prove takes, as a job of the queue above ("the pool as a QUEUE"): the worker that takes the job runs
 * bfhip_air_prove on its sub-context, the launches are exactly that call's and the bytes are its bytes. bfhip_pool_wait delivers
 * {"claimed_sums":...,"proof":...} in proof_json; log_max_rows and flags of such a result are 0. Brainfuck jobs and these may be interleaved
 * in one queue; cancel, outstanding, destroy and the "jobs outstanding" refusals apply unchanged. flags: BFHIP_AIR_PROVE_CHECK or 0.
 *   copied    at submit: the statement (trees, log sizes, mix words, components, bindings, parameter rules), the table tree_cols_h down to
 *             the device pointers, the kernel table, and the channel's STATE: the caller's channel object is not advanced by the job and may
 *             be reused or destroyed at once. Every host array behind the statement may be freed when the submit returns.
 *   borrowed  until that ticket's result has been taken: the program handles (bfhip_air, bfhip_logup; immutable), the device columns, and
 *             the kernels.
 *   kernels   kernels_h is NULL, or n_in_flight x n_components entries: row w holds component k's bfhip_air_kernel as compiled on
 *             bfhip_pool_ctx(pool, w), or NULL = interpreted. A job uses the row of the worker that runs it. A kernel of another context
 *             fails the job by name, as in bfhip_air_prove. Compile while nothing is outstanding: no compiler runs inside a worker.
 *   submit    fails (-1, no ticket, nothing queued, "bfhip_pool_submit_air: ...") on: null arguments; whatever the validator of
 *             bfhip_air_prove refuses, under the pool's current PcsConfig and max_log_domain, word for word; a channel created under other
 *             conventions (merkle_channel, mix_u64) than the pool's; more than BFHIP_POOL_MAX_OUTSTANDING jobs outstanding; a batch call in
 *             progress.
 *   the job   fails on everything else — status -1, "job <ticket>: bfhip_air_prove: ...": ConstraintsNotSatisfied, a zero denominator, the
 *             line of BFHIP_AIR_PROVE_CHECK, a null column pointer, unknown flags. The worker and the other jobs are unaffected.
 *   sessions  the job's session is the worker's own; the caller's bfhip_pcs_create (and bfhip_air_prove) on a sub-context stays refused while
 *             anything is outstanding. Such a job takes no shared preprocessed tree — a statement's preprocessed columns are a tree like
 *             any other — and creates no stream: the session, the batch and the composition enqueue on the sub-context's one stream.
 * bfhip_pool_set_scratch_reserve: bfhip_ctx_set_scratch_reserve(bytes_per_worker) on every sub-context, so that a job of a shape its
 * worker has seen makes no device allocation; refused ("jobs outstanding") while anything is queued, running or not yet taken. */
int32_t bfhip_pool_submit_air(bfhip_pool* pool, const bfhip_air_statement* statement, const uint32_t* const* const* tree_cols_h,
                              bfhip_air_kernel* const* kernels_h, const bfhip_channel* ch, uint32_t flags, uint64_t user_tag, uint64_t* ticket);
int32_t bfhip_pool_set_scratch_reserve(bfhip_pool* pool, uint64_t bytes_per_worker);

/* ---- Row order: a trace as its author writes it -> the storage-order columns of ANY AIR, and back ------------------------------------------
 * Every entry point above takes device columns in STORAGE order: CanonicCoset(log_size).circle_domain() bit-reversed. An AIR author writes a
 * witness in ROW order — row r + 1 is "the row at offset +1", the coset order. stwo's step between the two is
 * CircleEvaluation::new_canonical_ordered plus the bit reversal; here it is one launch, the first step of the generic pipeline
 * (INTEGRATION.md section 2e), in front of bfhip_pcs_commit / bfhip_air_check / bfhip_logup_program_generate(_batch) / bfhip_relation_program_* /
 * bfhip_air_prove.
 * The order (normative). n = 2^log_size. Cell (storage index) s holds row (coset index) i:
 *     d = bit_reverse(s, log_size);   i = 2 d if d < n / 2, else 2 (n - 1 - d) + 1.
 * Equivalently, for every d < n / 2 with s = bit_reverse(d, log_size): row 2 d lives in cell s, row 2 d + 1 in cell ~s & (n - 1).
 *
 * bfhip_cell_of_row / bfhip_row_of_cell (host only): that map and its inverse, 1 <= log_size <= 30, argument below 2^log_size; otherwise -1 with
 *   "bfhip_cell_of_row: <rule>" / "bfhip_row_of_cell: <rule>". bfhip_air_check and bfhip_logup_program_generate report CELLS: with
 *   bfhip_row_of_cell "first at cell 37" becomes the row the author wrote.
 *
 * bfhip_columns_from_rows: a table of n_rows rows and n_cols source columns of u32 words, in row order, to n_out storage-order columns.
 *   table->layout BFHIP_ROWS_ROW_MAJOR: word (r, c) at rows_d[r * row_stride + c]; row_stride in words, >= n_cols (a table of structs with
 *     trailing fields works); r * row_stride may exceed 2^32: source offsets are 64-bit. cols_h is ignored.
 *   table->layout BFHIP_ROWS_COLUMN_MAJOR: cols_h = host array of n_cols device pointers, each to n_rows words in row order. rows_d and
 *     row_stride are ignored.
 *   0 <= n_rows <= 2^log_size, 1 <= log_size <= 30, n_cols >= 1.
 *   src_cols_h[k] = the source column of output column k; NULL = the identity (then n_out <= n_cols). A subset, a permutation, the same
 *     source column more than once: one row table can feed several trees.
 *   out_cols_h: n_out device pointers, each to 2^log_size words, written in storage order. 1 <= n_out <= 256 = BFHIP_AIR_MAX_COLUMNS.
 *   Padding, rows n_rows .. 2^log_size - 1: the constant pad_h[k] of output column k (NULL = 0; a value >= p = 2^31 - 1 is refused on the
 *     host), or with BFHIP_ROWS_REPEAT_LAST in table->flags a copy of row n_rows - 1 (refused with n_rows = 0; pad_h is then ignored).
 *   Canonicity: every word read is checked on the way. A word >= 2^31 - 1 makes the call return -1 with
 *     "bfhip_columns_from_rows: row <r>, column <k>: <v> is not a canonical M31 value" — the lowest row, then the lowest OUTPUT column k
 *     (a 64-bit integer atomicMin over row * 256 + k). The outputs are then unspecified; nothing faults and the context stays usable.
 *   One launch on the context's stream and one read-back (the bad-word record: the call returns when the columns are written); a refused
 *     word costs a second, 4-byte one to quote its value. The table is borrowed for the call and not modified.
 *   Memory: nothing from the arena (bfhip_ctx_memory out[3] is unchanged) and no allocation — column descriptors and the record come from
 *     the staging ring. Works while a commitment-scheme session is open.
 *   Refused, -1 with "bfhip_columns_from_rows: <rule>", nothing enqueued, the context usable: null pointers (ctx aside: "null context");
 *     log_size out of range; n_rows > 2^log_size; row_stride < n_cols; a column index not below n_cols; n_out of 0 or above
 *     BFHIP_AIR_MAX_COLUMNS; an unknown layout or flag bit; reserved != 0; pad >= p; REPEAT_LAST with n_rows = 0; an output column whose byte
 *     range shares a byte with the source (row-major: the whole table from word (0, 0) to the last word of the last row; column-major: any
 *     source column) or with another output column — the message names the two; a context in a shard group.
 * bfhip_rows_from_columns: the inverse. n_cols storage-order columns of 2^log_size words -> words (r, c), r < n_rows, c < n_cols, of the
 *   row-major device table rows_d with row_stride >= n_cols; the rest of each row is left untouched. No canonicity check, no read-back: the
 *   launch is enqueued on the context's stream (bfhip_download behind it is ordered). What a caller uses to read a generated column back in
 *   row order: multiplicities, a logUp column. Refused in its own name: null pointers, log_size, n_rows, row_stride, n_cols of 0 or above
 *   BFHIP_AIR_MAX_COLUMNS, reserved != 0, the table sharing a byte with a column, a context in a shard group.
 * Kernel (csrc/rows.hip): tiles of 1024 rows through LDS, 8 or 16 columns per pass; log_size below 10: one thread per cell.
 * Not built: shard groups, row-granular (shifted) outputs, host-pointer sources streamed in chunks, pool jobs for generic statements.
 * Layout (natural alignment, declaration order):
 *   bfhip_rows_table  48 bytes: layout 0, n_cols 4, rows_d 8, cols_h 16, n_rows 24, row_stride 32, flags 40, reserved 44 */
enum { BFHIP_ROWS_ROW_MAJOR = 0, BFHIP_ROWS_COLUMN_MAJOR = 1, BFHIP_ROWS_REPEAT_LAST = 1 };
typedef struct bfhip_rows_table {
    uint32_t layout;                  /* BFHIP_ROWS_ROW_MAJOR or BFHIP_ROWS_COLUMN_MAJOR */
    uint32_t n_cols;                  /* source columns */
    const uint32_t* rows_d;           /* row-major: device table */
    const uint32_t* const* cols_h;    /* column-major: host array of n_cols device pointers */
    uint64_t n_rows;
    uint64_t row_stride;              /* row-major: words from one row to the next */
    uint32_t flags, reserved;         /* flags: BFHIP_ROWS_REPEAT_LAST; reserved must be 0 */
} bfhip_rows_table;
int32_t bfhip_columns_from_rows(bfhip_ctx* ctx, const bfhip_rows_table* table, uint32_t log_size, const uint32_t* src_cols_h, const uint32_t* pad_h,
                                uint32_t* const* out_cols_h, uint32_t n_out);
int32_t bfhip_rows_from_columns(bfhip_ctx* ctx, const uint32_t* const* cols_h, uint32_t n_cols, uint32_t log_size, uint32_t* rows_d, uint64_t n_rows,
                                uint64_t row_stride, uint32_t reserved);
int32_t bfhip_cell_of_row(uint32_t log_size, uint64_t row, uint64_t* cell);
int32_t bfhip_row_of_cell(uint32_t log_size, uint64_t cell, uint64_t* row);

/* ---- Row selection: filter and sort a row-order table on the device, straight into storage-order columns ---------------------------------------
 * Most tables of a VM-shaped AIR are not the register trace itself but a selection of it: an instruction sub-table is "the rows where
 * ci == opcode, beside their successor", a memory-consistency table is "the rows sorted by (address, clk)". bfhip_rows_select is
 * bfhip_columns_from_rows with a row filter, a stable sort and per-output row offsets in front: the selected, reordered rows are written where
 * bfhip_columns_from_rows would put the same rows, without a trip through the host.
 * Source: a bfhip_rows_table, unchanged, both layouts. Candidates: source rows sel->row_begin .. sel->row_end - 1.
 * Selected rows (normative):
 *   A candidate row r is selected iff every term holds: word(r, term.col) <op> term.value as unsigned integers, op one of BFHIP_SELECT_EQ, NE,
 *     LT, LE, GT, GE. The terms are a conjunction; n_terms = 0 selects every candidate.
 *   The selected rows are ordered by the keys, keys[0] most significant: ascending in word(r, key.col), or descending with
 *     BFHIP_SELECT_DESCENDING in key.flags. The sort is stable — equal keys keep source-row order —; n_keys = 0 is source-row order.
 *   *n_selected = their number S; order[i] = the source row of output row i, i < S.
 * Outputs: output row i < S of output column k is the source word (order[i] + outs_h[k].offset, outs_h[k].col): a sub-table's "next" values
 *   are offset +1 of the same selection, without a pass of their own. Rows S .. 2^log_size - 1 hold outs_h[k].pad, or with
 *   BFHIP_ROWS_REPEAT_LAST in table->flags a copy of output row S - 1 (pads are then ignored). out_cols_h: n_out device pointers, each to
 *   2^log_size words, written whole in storage order (the order of "Row order" above). 1 <= n_out <= 256, 1 <= log_size <= 30.
 * order_d: NULL, or row_end - row_begin device words of which the first S receive order[] (32-bit: row_end <= 2^32 when given) — which
 *   register row a table row is.
 * Count-only form: out_cols_h == NULL with n_out == 0 and log_size == 0 returns *n_selected and writes no column (order_d still, if given):
 *   how a caller sizes the domain. Otherwise S > 2^log_size is -1 with "bfhip_rows_select: <S> rows selected, the domain has <2^log_size>",
 *   and REPEAT_LAST with S = 0 is -1 with "bfhip_rows_select: BFHIP_ROWS_REPEAT_LAST needs at least one selected row"; both are found after
 *   the count (*n_selected is set) and before any column is written.
 * Canonicity: checked are the term words of EVERY candidate row, and the key words and the output words (offsets applied) of every selected
 *   row; the key words only where the sort runs (not in the count-only form without order_d). A word >= 2^31 - 1 makes the call return -1 with
 *   "bfhip_rows_select: row <r>, column <c>: <v> is not a canonical M31 value" — the lowest SOURCE row, then the lowest SOURCE column (a 64-bit
 *   integer atomicMin over row * 2^24 + column). The outputs are then unspecified; nothing faults and the context stays usable. The two
 *   refusals by the count come first.
 * Launches: flags, a scan and a compaction; per pair of keys one key gather and one stable radix sort (rocPRIM), least significant pair
 *   first; the gather (csrc/rows_select.hip, DESIGN.md section 9t: tiles of 1024 output rows through LDS as csrc/rows.hip, the tile's
 *   permutation kept in LDS; log_size below 10: one thread per cell). Two read-backs: S, which the sort and the gather need on the host, and
 *   the bad-word record at the end (the call returns when the columns are written); a refused word costs a third, 4-byte one.
 * Memory: nothing from the arena (bfhip_ctx_memory out[3] is unchanged): works while a commitment-scheme session is open. Descriptors come
 *   from the staging ring; flags, positions, two permutations, two key arrays and rocPRIM's temporary are call-scoped scratch, served from the
 *   scratch reserve where one is set (bfhip_ctx_set_scratch_reserve: no device allocation on the second call of a shape).
 * Refused, -1 with "bfhip_rows_select: <rule>", nothing enqueued, the context usable — the rule names the term, key or output index where
 *   there is one: everything bfhip_columns_from_rows refuses about the table (null pointers, unknown layout or flag bit, reserved != 0,
 *   row_stride < n_cols, no columns), the outputs (log_size, n_out, a null output column, pad >= p unless REPEAT_LAST) and overlaps (an output
 *   column or order_d sharing a byte with the source or with an earlier output; the message names the two); out_cols_h NULL with n_out or
 *   log_size not 0; n_terms above BFHIP_SELECT_MAX_TERMS or n_keys above BFHIP_SELECT_MAX_KEYS, either non-zero with a null array; an unknown
 *   op or key flag bit; a term value >= p; a term, key or output column index not below n_cols; row_begin > row_end; row_end > n_rows; more
 *   than 2^30 candidates; an output offset with row_begin + offset < 0 or row_end + offset > n_rows, so that no read can leave the table;
 *   sel->reserved != 0; n_rows above 2^40 or n_cols above 2^24 (the bad-word record's fields); a context in a shard group.
 * bfhip_rows_select_host (host only, no GPU): the same definition over a host row-major table, the result in ROW order — out_rows_h = 2^log_size
 *   x n_out words, order_h = row_end - row_begin words or NULL; out_rows_h NULL with n_out 0 and log_size 0 is the count-only form.
 *   repeat_last is 0 or 1. The kernels are held to it word for word. The same refusals and failures under "bfhip_rows_select_host: ".
 * Not built: a multi-source selection (several source tables are concatenated by the caller's layout: the Instruction table's program rows
 *   in front of the trace's, "Row filling" below), disjunctions and column-to-column terms, pool jobs, shard groups, row-granular (shifted)
 *   outputs. Row insertion — the Memory table's clk-gap dummy rows, the dummies that pad a table — is bfhip_rows_fill, "Row filling" below.
 * Layout (natural alignment, declaration order):
 *   bfhip_select_term  12 bytes: col 0, op 4, value 8
 *   bfhip_select_key    8 bytes: col 0, flags 4
 *   bfhip_select_out   12 bytes: col 0, offset 4, pad 8
 *   bfhip_rows_select_desc  48 bytes: terms 0, keys 8, n_terms 16, n_keys 20, row_begin 24, row_end 32, reserved 40 */
enum { BFHIP_SELECT_EQ = 0, BFHIP_SELECT_NE = 1, BFHIP_SELECT_LT = 2, BFHIP_SELECT_LE = 3, BFHIP_SELECT_GT = 4, BFHIP_SELECT_GE = 5,
       BFHIP_SELECT_DESCENDING = 1, BFHIP_SELECT_MAX_TERMS = 8, BFHIP_SELECT_MAX_KEYS = 4 };
typedef struct bfhip_select_term { uint32_t col, op, value; } bfhip_select_term;      /* word(row, col) <op> value, as integers */
typedef struct bfhip_select_key { uint32_t col, flags; } bfhip_select_key;            /* flags: BFHIP_SELECT_DESCENDING */
typedef struct bfhip_select_out { uint32_t col; int32_t offset; uint32_t pad; } bfhip_select_out;
typedef struct bfhip_rows_select_desc {
    const bfhip_select_term* terms;   /* host array of n_terms */
    const bfhip_select_key* keys;     /* host array of n_keys, most significant first */
    uint32_t n_terms, n_keys;
    uint64_t row_begin, row_end;      /* candidates: source rows row_begin .. row_end - 1 */
    uint32_t reserved[2];             /* must be 0 */
} bfhip_rows_select_desc;
int32_t bfhip_rows_select(bfhip_ctx* ctx, const bfhip_rows_table* table, const bfhip_rows_select_desc* sel, uint32_t log_size,
                          const bfhip_select_out* outs_h, uint32_t* const* out_cols_h, uint32_t n_out, uint32_t* order_d, uint64_t* n_selected);
int32_t bfhip_rows_select_host(const uint32_t* table_h, uint64_t n_rows, uint32_t n_cols, uint64_t row_stride, uint32_t repeat_last,
                               const bfhip_rows_select_desc* sel, uint32_t log_size, const bfhip_select_out* outs_h, uint32_t n_out,
                               uint32_t* out_rows_h, uint32_t* order_h, uint64_t* n_selected);

/* ---- Row filling: insert the missing rows of a table on the device, straight into storage-order columns ----------------------------------------
 * A memory-consistency table is not a selection of the trace: it is the (address, clk)-sorted rows with a dummy row for every clk that is
 * skipped inside one address, padded by dummies that keep counting, each row beside its successor — one pairing dummy past the end included
 * (memory/table.rs:249-303, 121-151). bfhip_rows_fill is that step for any AIR: the entries of a bfhip_rows_table, in the order a
 * bfhip_rows_select call wrote or in source order, with the missing rows inserted, written where bfhip_columns_from_rows would put the same rows.
 * Entries (normative): entry i < n_entries is source row order_d[i]; with order_d == NULL it is source row row_begin + i. row_begin must be 0
 *   when order_d is given.
 * Gaps: filled only with BFHIP_FILL_GAPS in fill->flags, which needs a step_col. Before entry i >= 1, with prev = entry i - 1, there is a gap
 *   iff every group word (group_cols, n_group of them) of the two is equal and step(i) > step(prev) + 1 as integers; it holds
 *   g_i = step(i) - step(prev) - 1 inserted rows, numbered t = 1 .. g_i. Otherwise g_i = 0: equal or descending steps and a group change
 *   insert nothing. g_0 = 0. With n_group = 0 every consecutive pair is one group.
 * The sequence is infinite: the entries, each with its inserted rows in front — T = n_entries + sum g_i elements, counted in 64 bits —, then
 *   the tail: inserted rows behind the last entry with t = 1, 2, ... without end.
 * Values, by outs_h[k].kind:
 *   BFHIP_FILL_KEEP  a real row holds word(row, col); an inserted row holds its predecessor entry's word(col), and if col == step_col that
 *                    word + t as an M31 sum (only the tail can wrap past p - 1).
 *   BFHIP_FILL_SET   a real row holds word(row, col); an inserted row holds `value`.
 *   BFHIP_FILL_MARK  a real row holds 0; an inserted row holds `value`; col is ignored. The `d` column of a table.
 * Outputs: output row i of output column k is sequence element i + outs_h[k].offset, 0 <= offset <= BFHIP_FILL_MAX_OFFSET = 16: a row's
 *   successor is offset 1 of the same call. Every output row is defined, the pairing dummy at 2^log_size included: the call has no pad array.
 *   out_cols_h: n_out device pointers, each to 2^log_size words, written whole in storage order. 1 <= n_out <= 256, 1 <= log_size <= 30.
 * *n_filled = T. Count-only form: out_cols_h == NULL with n_out == 0 and log_size == 0 returns T and writes nothing: how a caller sizes the
 *   domain. Otherwise T > 2^log_size is -1 with "bfhip_rows_fill: <T> rows after filling, the domain has <2^log_size>", found after the count
 *   (*n_filled is set) and before any column is written — also when T exceeds 2^32: the total is a 64-bit sum, nothing wraps.
 * Canonicity: checked are the group and step words of every entry (with BFHIP_FILL_GAPS) and every source word an output reads (an inserted
 *   row of a SET column and a MARK column read nothing). A word >= 2^31 - 1 makes the call return -1 with
 *   "bfhip_rows_fill: row <r>, column <c>: <v> is not a canonical M31 value" — the lowest SOURCE row, then the lowest SOURCE column. The
 *   outputs are then unspecified; nothing faults and the context stays usable. The refusal by the count comes first.
 * order_d: every word must be below n_rows, else -1 with "bfhip_rows_fill: order[<i>] = <r> is not a row of the table (<n_rows> rows)", the
 *   lowest i — found by a launch that reads only order_d, before any launch reads the table through it: no read leaves the table, nothing
 *   is written.
 * Launches (csrc/rows_fill.hip): the order check; with BFHIP_FILL_GAPS the counts c_i = 1 + g_i with their 64-bit total
 *   and a scan for the positions; the gather — tiles of 1024 output rows through LDS as bfhip_rows_select's, each run of 32 rows resolved to
 *   (entry, t) once; log_size below 10: one thread per cell. Two read-backs: T together with the order record, and the bad-word record at
 *   the end (the call returns when the columns are written); a refused word costs a third, 4-byte one.
 * Memory: nothing from the arena (bfhip_ctx_memory out[3] is unchanged): works while a commitment-scheme session is open. Descriptors and
 *   records come from the staging ring; counts and positions are call-scoped scratch, served from the scratch reserve where one is set.
 * Refused, -1 with "bfhip_rows_fill: <rule>", nothing enqueued, the context usable: everything bfhip_rows_select refuses about the table
 *   (null pointers, unknown layout or flag bit, reserved != 0, row_stride < n_cols, no columns, n_rows above 2^40, n_cols above 2^24), the
 *   outputs (log_size, n_out, a null output column) and overlaps (an output column sharing a byte with the source, with order_d or with an
 *   earlier output; the message names the two); out_cols_h NULL with n_out or log_size not 0; n_entries of 0 ("needs at least one entry")
 *   or above 2^30; row_begin + n_entries > n_rows; row_begin != 0 with order_d; n_group above BFHIP_FILL_MAX_GROUP or non-zero with a null
 *   array; a group, step or output column index not below n_cols; BFHIP_FILL_GAPS without a step column; an unknown kind or flag bit; a SET
 *   or MARK value >= p; an offset above 16; fill->reserved != 0; BFHIP_ROWS_REPEAT_LAST in table->flags (the tail is this call's padding);
 *   a context in a shard group.
 * bfhip_rows_fill_host (host only, no GPU): the same definition over a host row-major table, fill->order_d a HOST array there, the result
 *   in ROW order — out_rows_h = 2^log_size x n_out words; out_rows_h NULL with n_out 0 and log_size 0 is the count-only form. The kernels are
 *   held to it word for word. The same refusals and failures under "bfhip_rows_fill_host: ".
 * Not built: a multi-source bfhip_rows_select without the caller's layout (lay the row blocks into one device table, as the Instruction
 *   table of brainfuck_rows_fill does); the per-instruction sub-tables' dummy rows (their padding counts from the SUCCESSOR entry, which a
 *   witness program over the selected columns covers); an origin map per output row; pool jobs; shard groups; row-granular (shifted) outputs.
 * Layout (natural alignment, declaration order):
 *   bfhip_fill_out  16 bytes: col 0, kind 4, value 8, offset 12
 *   bfhip_rows_fill_desc  48 bytes: group_cols 0, n_group 8, step_col 12, order_d 16, n_entries 24, row_begin 32, flags 40, reserved 44 */
enum { BFHIP_FILL_KEEP = 0, BFHIP_FILL_SET = 1, BFHIP_FILL_MARK = 2,
       BFHIP_FILL_GAPS = 1,
       BFHIP_FILL_NO_STEP = 4294967295u /* 0xFFFFFFFF */, BFHIP_FILL_MAX_GROUP = 4, BFHIP_FILL_MAX_OFFSET = 16 };
typedef struct bfhip_fill_out { uint32_t col, kind, value, offset; } bfhip_fill_out;
typedef struct bfhip_rows_fill_desc {
    const uint32_t* group_cols;       /* host array of n_group source columns */
    uint32_t n_group, step_col;       /* step_col: a source column, or BFHIP_FILL_NO_STEP */
    const uint32_t* order_d;          /* NULL, or n_entries device words: the source row of entry i, as bfhip_rows_select writes order_d */
    uint64_t n_entries, row_begin;
    uint32_t flags, reserved;         /* flags: BFHIP_FILL_GAPS; reserved must be 0 */
} bfhip_rows_fill_desc;
int32_t bfhip_rows_fill(bfhip_ctx* ctx, const bfhip_rows_table* table, const bfhip_rows_fill_desc* fill, uint32_t log_size,
                        const bfhip_fill_out* outs_h, uint32_t* const* out_cols_h, uint32_t n_out, uint64_t* n_filled);
int32_t bfhip_rows_fill_host(const uint32_t* table_h, uint64_t n_rows, uint32_t n_cols, uint64_t row_stride, const bfhip_rows_fill_desc* fill,
                             uint32_t log_size, const bfhip_fill_out* outs_h, uint32_t n_out, uint32_t* out_rows_h, uint64_t* n_filled);

/* ---- Relation programs: the lookup tuples of ANY AIR that do not cancel ------------------------------------------------------------------------
 * bfhip_relation_summary / bfhip_trace_relations know the three Brainfuck relations and the 13 table layouts. An AIR proved through bfhip_pcs_* +
 * bfhip_air_* + bfhip_logup_* whose lookups do not balance learns only that its claimed sums do not add up to zero; a
 * fraction program cannot name the tuple to blame, its denominators are already z - sum alpha^i v_i. A relation program is what a component's
 * `add_to_relation(relation, multiplicity, values)` calls are, as data — stwo's relation tracker, the tool it ships beside `assert_constraints`:
 * a constraint program's bytecode (same four-word instructions, same m[] register file, same caps: 96 m registers, 4096 instructions, 256
 * columns), base field only, with two opcodes that exist only here:
 *   BFHIP_REL_WORD   -, a          append m[a] to the pending tuple
 *   BFHIP_REL_ENTRY  relation, a   one add_to_relation: the entry (relation `dst`, the pending tuple, multiplicity m[a]); the pending tuple is then empty
 * A relation program reads a row's own cells, and the multiplicity of an entry is an M31 value, as on the main trace. Admitted: M_COL at offset
 * 0 (a "next" value is a column, as in fraction programs), M_CONST, M_ADD, M_SUB, M_MUL, M_NEG, REL_WORD, REL_ENTRY. There are no parameters.
 * Relations are numbered 0 .. n_relations - 1 by the caller; relation r has relation_words_h[r] words, 1 to 7 (what bfhip_relation_entry.tuple
 * holds: the structs of bfhip_relation_summary are reused unchanged).
 *
 * bfhip_relation_program_create (host only): every rule of bfhip_air_create that applies (opcode, register range, read before write, column
 *   within n_cols, v < p, the instruction and column caps), and: every Q_* opcode, C_BASE, C_EXT, FRAC and END_COL are refused; M_COL at a
 *   non-zero offset is refused; a relation index not below n_relations, an ENTRY whose pending tuple has not exactly that relation's width, a
 *   WORD when 7 words are pending, a write to a register that is a word of the pending tuple (the tuple holds registers, not copies, until
 *   its ENTRY), a WORD that no ENTRY follows, a program without any ENTRY or with more than 32 =
 *   BFHIP_RELATION_PROGRAM_MAX_ENTRIES, n_relations outside 1 .. 16 = BFHIP_RELATION_PROGRAM_MAX_RELATIONS and a width outside 1 .. 7 =
 *   BFHIP_RELATION_PROGRAM_MAX_WORDS are refused. Each refusal is -1 with "bfhip_relation_program_create: instruction <i>: <rule>" (rules
 *   about the program as a whole name the instruction count). bfhip_air_create and bfhip_logup_create keep refusing opcodes 17 and 18.
 * bfhip_relation_program_shape: out = {columns, relations, entries, instructions, m registers used, 0, 0, 0}.
 * bfhip_relation_program_eval_row (host only): the entries of ONE row in program order, zero multiplicities included: col_values_h = n_cols
 *   canonical words; entry e is (relations_out[e], mults_out[e], tuples_out[7 e ..], zero padded). *n = the program's entries; -2
 *   ("capacity") when cap < *n; all three outputs NULL with cap 0: size query.
 * bfhip_relation_program_summary: bfhip_relation_summary's semantics, word for word, over 1..64 tables of any programs. Table t is a program
 *   and its columns: column k holds 2^(log_size - s_k) words (s_k = col_shifts_h[k]; NULL = every s_k = row_shift) of cells of
 *   CanonicCoset(log_size).circle_domain(), bit-reversed, and the program is evaluated ONCE per 2^row_shift cells: row r of 2^(log_size -
 *   row_shift) stands for cell r << row_shift and reads column k at (r << row_shift) >> s_k. Row-granular Brainfuck tables are row_shift 4 with
 *   NULL shifts; full-size columns of a session are row_shift 0. A row's entry with multiplicity 0 is no entry; multiplicity 1 counts as a
 *   yield, p - 1 as a use, anything else as "other"; net = the canonical M31 sum; a tuple is reported iff net != 0. out[r] = relation r,
 *   r < n_relations; its reported tuples, in lexicographic order of their words, the first cap_per_relation of them, go to entries_h + r *
 *   cap_per_relation; first_* = the lowest (table index, row r). entries_h == NULL with cap 0 gives the counts only. Counts are per evaluated
 *   ROW: with row_shift = s every row stands for 2^s cells, and the logUp sum sees 2^s x net. A relation no program of the list adds to gets a
 *   report of zeros with its n_words set. Every program of the list must have been created with this n_relations and the same widths:
 *   otherwise -1, naming the table. Every field is an integer and the same whatever the schedule: entries stand in (table, row, program
 *   order), no atomics in the extraction. Uses the context's arena (reset as a proof resets it; bfhip_ctx_memory out[3] is put back) and is
 *   therefore refused while a commitment-scheme session is open: the author's check belongs in front of bfhip_pcs_create, it needs no lookup
 *   elements. Returns 0 whether or not anything is unbalanced, and bfhip_last_error() is not touched by imbalances; -1 with
 *   "bfhip_relation_program_summary: <rule>" for null arguments, n_tables outside 1..64, log_size outside [1, max_log_domain], row_shift or a
 *   column shift above log_size, more than 2^31 (rows x ENTRY instructions of one relation) in total, a context in a shard group, and HIP
 *   errors.
 * Not built (each would be half a feature): tuples wider than 7 words (a new entry layout), extension-field multiplicities, column offsets,
 * use inside an open session, a generic preflight, shard groups.
 * Layout (natural alignment, declaration order):
 *   bfhip_relation_program_table  32 bytes: program 0, log_size 8, row_shift 12, cols_h 16, col_shifts_h 24 */
enum { BFHIP_REL_WORD = 17, BFHIP_REL_ENTRY = 18, BFHIP_RELATION_PROGRAM_MAX_RELATIONS = 16, BFHIP_RELATION_PROGRAM_MAX_WORDS = 7,
       BFHIP_RELATION_PROGRAM_MAX_ENTRIES = 32 };
typedef struct bfhip_relation_program bfhip_relation_program;
int32_t bfhip_relation_program_create(const uint32_t* code, size_t n_words, uint32_t n_cols, const uint32_t* relation_words_h, uint32_t n_relations,
                                      bfhip_relation_program** out);
int32_t bfhip_relation_program_destroy(bfhip_relation_program* rp);
int32_t bfhip_relation_program_shape(const bfhip_relation_program* rp, uint32_t out[8]);
int32_t bfhip_relation_program_eval_row(const bfhip_relation_program* rp, const uint32_t* col_values_h, uint32_t* relations_out, uint32_t* mults_out,
                                        uint32_t* tuples_out, uint32_t cap, uint32_t* n);
typedef struct bfhip_relation_program_table {
    const bfhip_relation_program* program;
    uint32_t log_size;                 /* the component's trace: 2^log_size cells */
    uint32_t row_shift;                /* 0..log_size: ONE evaluation per 2^row_shift cells */
    const uint32_t* const* cols_h;     /* host array of n_cols device pointers */
    const uint32_t* col_shifts_h;      /* host array of n_cols shifts; NULL = every s_k = row_shift */
} bfhip_relation_program_table;
int32_t bfhip_relation_program_summary(bfhip_ctx* ctx, const bfhip_relation_program_table* tables, uint32_t n_tables, uint32_t n_relations,
                                       bfhip_relation_report* out, bfhip_relation_entry* entries_h, uint32_t cap_per_relation);

/* ---- Lookup multiplicities: fill the looked-up table's multiplicity column of ANY AIR on the device -----------------------------------------
 * The relation tracker reports nets; this entry point writes them. A lookup AIR needs, before anything can be swept, generated or committed,
 * the multiplicity column of its table: how often every row's tuple is used. bfhip_relation_program_multiplicities counts that from the
 * relation programs themselves, so the consumers' columns never leave the GPU.
 *   tables, n_tables, n_relations: exactly what bfhip_relation_program_summary takes — row and column shifts, the validation of the list and
 *     the limit of 2^31 (rows x ENTRY instructions of one relation) are the same; the target's rows count towards that limit.
 *   The target — the table side of the lookup — is the target_entry-th ENTRY instruction OF RELATION `relation`, in program order from 0, of
 *     the program of tables[target_table]. Its tuple is evaluated at every row of that table; its multiplicity operand is evaluated and
 *     IGNORED: the column it reads may hold anything, and may be out_d itself.
 *   Every other entry of the relation counts as in the summary (multiplicity 0 is no entry): the other tables', and the other ENTRYs of the
 *     target table, others of the same relation included.
 *   out_d: one word per evaluated row of the target table, 2^(log_size - row_shift) words. For each distinct tuple T among the target's rows
 *     the LOWEST row holding T receives net(T), the canonical M31 sum of the other entries' multiplicities with tuple T; every other row —
 *     every later duplicate of T included — receives 0. A table side written relation_entry(r, -mult, [t...]) with out_d as its mult column
 *     is then balanced against everything its rows hold. out_d is written only after every read of the extraction has completed.
 *   Missing tuples: a tuple with net != 0 among the other entries that NO target row holds cannot be balanced by this table. The first `cap`
 *     of them, in the lexicographic order of the summary, go to missing_h as bfhip_relation_entry (reused unchanged; net, n_yield, n_use,
 *     n_other and first_* have their meaning over the other entries). missing_h == NULL with cap 0 gives the counts only. Missing tuples are
 *     a result, not an error: the call returns 0 and leaves bfhip_last_error() alone.
 *   Every field of the report and every word of out_d is an integer and the same whatever the schedule: the extraction has no atomics, the
 *     lowest row is a 64-bit atomicMin, the three tuple counts are integer atomicAdds.
 *   Uses the context's arena like the summary (bfhip_ctx_memory out[3] is put back on every path) and belongs in front of bfhip_pcs_create.
 *   Refused, -1 with "bfhip_relation_program_multiplicities: <rule>" and the context still usable: everything the summary refuses; relation
 *     >= n_relations; target_table >= n_tables; a target program with fewer than target_entry + 1 ENTRYs of that relation (both numbers
 *     named); NULL out_d or report (or NULL missing_h with cap > 0); an open commitment-scheme session; a context in a shard group.
 * Not built: extension-field multiplicities, tuples wider than 7 words, column offsets, use inside an open session, shard groups.
 * Layout (natural alignment, declaration order):
 *   bfhip_multiplicity_report  80 bytes: relation 0, n_words 4, target_table 8, target_entry 12, n_rows 16, n_row_tuples 24, n_entries 32,
 *                              n_tuples 40, n_filled 48, n_missing 56, n_reported 64, reserved 72 */
typedef struct bfhip_multiplicity_report {
    uint32_t relation, n_words;
    uint32_t target_table, target_entry;
    uint64_t n_rows;        /* evaluated rows of the target table, 2^(log_size - row_shift) */
    uint64_t n_row_tuples;  /* distinct tuples among them (n_rows - n_row_tuples rows are duplicates and get 0) */
    uint64_t n_entries;     /* entries of the relation from everything BUT the target ENTRY, non-zero multiplicity */
    uint64_t n_tuples;      /* distinct tuples among those */
    uint64_t n_filled;      /* target rows that received a non-zero value */
    uint64_t n_missing;     /* tuples with net != 0 among the other entries that no target row holds, whatever the cap */
    uint64_t n_reported;    /* min(n_missing, cap) */
    uint32_t reserved[2];
} bfhip_multiplicity_report;
int32_t bfhip_relation_program_multiplicities(bfhip_ctx* ctx, const bfhip_relation_program_table* tables, uint32_t n_tables, uint32_t n_relations,
                                              uint32_t relation, uint32_t target_table, uint32_t target_entry, uint32_t* out_d,
                                              bfhip_multiplicity_report* report, bfhip_relation_entry* missing_h, uint32_t cap);

/* ---- Witness programs: derive the columns an author does not have, row by row, on the device ------------------------------------------------
 * Between bfhip_columns_from_rows and the first commitment stand the columns an AIR's author does not hold but can compute from the ones they
 * do: the inverse of an is-zero gadget, a padding flag, a selector, the bits of a byte, and every "next" value — fraction and relation
 * programs read a row's own cells only, so a "next" value is a column, and in storage order row r + 1 is not pointer + 1. A witness program
 * is a constraint program's bytecode (same four-word {op, dst, a, b} instructions, same m[] register file, same caps: 96 m registers, 4096
 * instructions, 256 columns, offsets -16..16), base field only, run ONCE PER ROW of CanonicCoset(log_size): it reads input columns at trace
 * offsets and stores output columns. Admitted from the shared set: M_COL at any offset in -BFHIP_AIR_MAX_OFFSET..BFHIP_AIR_MAX_OFFSET (the
 * coset-order move, cyclic over 2^log_size: exactly what bfhip_air_check reads for that mask entry), M_CONST, M_ADD, M_SUB, M_MUL, M_NEG.
 * Opcodes that exist only here:
 *   BFHIP_WIT_ARG      dst, k       m[dst] = args[k]: a per-call array of canonical M31 words — what differs from trace to trace, such as
 *                                   the number of real rows
 *   BFHIP_WIT_ROW      dst          m[dst] = the row's coset index: the r of bfhip_columns_from_rows (bfhip_row_of_cell of the cell)
 *   BFHIP_WIT_INV0     dst, a       m[dst] = m[a]^-1, and 0 for 0 (the convention of the VM's mvi)
 *   BFHIP_WIT_IS_ZERO  dst, a       m[dst] = 1 if m[a] == 0, else 0
 *   BFHIP_WIT_LT       dst, a, b    m[dst] = 1 if m[a] < m[b] as integers in [0, p), else 0
 *   BFHIP_WIT_AND      dst, a, imm  m[dst] = m[a] & imm; imm < 2^31 in the b word
 *   BFHIP_WIT_SHR      dst, a, imm  m[dst] = m[a] >> imm; imm in 0..30
 *   BFHIP_WIT_STORE    out, a       output column `out` (the dst word) of this row receives m[a]
 * Every value a program produces is a canonical M31 word when its inputs are (bfhip_columns_from_rows checks that on the way in): there is
 * no run-time failure and no report.
 *
 * bfhip_witness_program_create (host only): every rule of bfhip_air_create that applies (opcode, register range, read before write, column
 *   within n_cols, offset, v < p, the instruction and column caps), and: every Q_* opcode, C_BASE, C_EXT, FRAC, END_COL, REL_WORD and
 *   REL_ENTRY are refused; an ARG index not below n_args; n_args above BFHIP_AIR_MAX_PARAMS; an AND immediate of 2^31 or more; a SHR
 *   immediate above 30; n_out outside 1 .. 256; a STORE index not below n_out; an output stored a second time ("STORE: output <k> is stored
 *   a second time"); an output no STORE writes ("the program ends with output <k> never stored"). Each refusal is -1 with
 *   "bfhip_witness_program_create: instruction <i>: <rule>" (rules about the program as a whole name the instruction count). bfhip_air_create,
 *   bfhip_logup_create and bfhip_relation_program_create keep refusing opcodes 19 and up.
 * bfhip_witness_program_shape: out = {columns, outputs, args, instructions, m registers used, min offset, max offset, 0}; the offsets are
 *   int32 in uint32 words.
 * bfhip_witness_program_eval_table (host only): the whole program over a row-major table in ROW order — table_h = 2^log_size x n_cols words,
 *   out_h = 2^log_size x n_out words; row r reads column c at offset `off` in row (r + off) mod 2^log_size. The definition the kernel is held
 *   to. 1 <= log_size <= 30. Refused, -1 with "bfhip_witness_program_eval_table: <rule>": null arguments, log_size, n_args other than the
 *   program's, an arg or a table word that is not canonical (the word's row and column are named).
 * bfhip_witness_program_generate: the program at every cell of the trace domain. cols_h: the program's n_cols device columns, out_cols_h:
 *   n_out device columns; all of them full size — 2^log_size words in storage order, shift 0. args_h: n_args host words. ONE launch on the
 *   context's stream and no read-back: ordered like bfhip_rows_from_columns, so bfhip_download behind it sees the result. The inputs are not
 *   checked for canonicity (they come from bfhip_columns_from_rows or from an entry point that wrote canonical words); output columns are
 *   written whole.
 *   Memory: descriptors, args and code go through the staging ring; nothing from the arena (bfhip_ctx_memory out[3] is unchanged) and no
 *     allocation. Works while a commitment-scheme session is open.
 *   Refused, -1 with "bfhip_witness_program_generate: <rule>", nothing enqueued, the context usable: null arguments ("null argument"; a null
 *     column names itself: "input column <j> is a null pointer", "output column <k> is a null pointer"); a context in a shard group; log_size
 *     outside [1, max_log_domain]; n_out or n_args other than the program's ("<n> output columns, the program has <m>", "<n> args, the
 *     program has <m>"); "arg <k>: <v> is not a canonical M31 value"; an output column sharing a byte with an input or with another output:
 *     "output column <k> overlaps input column <j>" / "output column <k> overlaps output column <j>".
 * Kernel (csrc/witness_program.hip): the instruction core of the four program kernels on the row of bfhip_air_check;
 *   one lane per cell, one wave per workgroup, the register file in LDS.
 * Not built: row insertion and sorting inside a program (the Memory table's clk-gap dummy rows and the Instruction table's program rows
 *   beside the trace's are bfhip_rows_fill, "Row filling" above; a sort or a row filter alone is bfhip_rows_select), extension-field values,
 *   shifted (row-granular) columns, reading an output of the same call at an offset (run a second program), witness programs compiled with
 *   hiprtc, pool jobs, shard groups. */
enum { BFHIP_WIT_ARG = 19, BFHIP_WIT_ROW = 20, BFHIP_WIT_INV0 = 21, BFHIP_WIT_IS_ZERO = 22, BFHIP_WIT_LT = 23, BFHIP_WIT_AND = 24, BFHIP_WIT_SHR = 25,
       BFHIP_WIT_STORE = 26 };
typedef struct bfhip_witness_program bfhip_witness_program;
int32_t bfhip_witness_program_create(const uint32_t* code, size_t n_words, uint32_t n_cols, uint32_t n_out, uint32_t n_args, bfhip_witness_program** out);
int32_t bfhip_witness_program_destroy(bfhip_witness_program* wp);
int32_t bfhip_witness_program_shape(const bfhip_witness_program* wp, uint32_t out[8]);
int32_t bfhip_witness_program_eval_table(const bfhip_witness_program* wp, uint32_t log_size, const uint32_t* table_h, const uint32_t* args_h, uint32_t n_args,
                                         uint32_t* out_h);
int32_t bfhip_witness_program_generate(bfhip_ctx* ctx, const bfhip_witness_program* wp, uint32_t log_size, const uint32_t* const* cols_h,
                                       const uint32_t* args_h, uint32_t n_args, uint32_t* const* out_cols_h, uint32_t n_out);

/* Host-only pieces of the drop-in (usable without a GPU): the Brainfuck compiler (crates/brainfuck_vm/src/compiler.rs:17-37), the VM
 * (crates/brainfuck_vm/src/machine.rs:141-238; trace rows are 7 u32: clk, ip, ci, ni, mp, mv, mvi) and the 13 table builders
 * (`XTable::from`, the table.rs files under crates/brainfuck_prover/src/components; component index = claim order of mod.rs:85-99), row-major out. */
int32_t bfhip_host_compile(const char* code, uint32_t* out, size_t cap, size_t* n);
int32_t bfhip_host_run(const char* code, const uint8_t* input_h, size_t n_input, uint8_t* out, size_t out_cap, size_t* n_out,
                       uint32_t* trace7, size_t trace_cap_rows, size_t* n_rows);
/* bfhip_host_run with the RAM size given (Machine::new_with_config, machine.rs:116-131); ram_size = 0: the default 30000 cells. */
int32_t bfhip_host_run_ram(const char* code, const uint8_t* input_h, size_t n_input, size_t ram_size, uint8_t* out, size_t out_cap, size_t* n_out,
                           uint32_t* trace7, size_t trace_cap_rows, size_t* n_rows);
int32_t bfhip_host_table(const uint32_t* trace7, size_t n_trace, const uint32_t* code, size_t n_code, int32_t component,
                         uint32_t* out_row_major, size_t cap, size_t* n_rows, size_t* n_cols);

/* Optional per-kernel timing with HIP events on the context's stream (used by bench.py for the roofline object).
 * Report: JSON {"kernel": {"calls": n, "total_ms": t, "bytes": algorithmic_bytes}, ...}, malloc'd (bfhip_free_host). */
/* mode: 0 off, 1 every instrumented kernel, 2 only k_merkle_layer (the dominant kernel; lowest overhead). */
int32_t bfhip_profile_enable(bfhip_ctx* ctx, int32_t mode);
int32_t bfhip_profile_reset(bfhip_ctx* ctx);
int32_t bfhip_profile_report(bfhip_ctx* ctx, char** json);
/* Diagnostic: the shader clock this device sustains under the dominant kernel's instruction mix — a register-only loop of the Blake2s compression
 * (no memory traffic) launched back to back for `seconds` (>= 0.5 for a settled clock), every workgroup stamping the shader-cycle counter against
 * the constant 100 MHz counter around its loop. out = {median GHz over the workgroups of the last launch, min, max, 10^9 compressions/s of the last
 * launches, launches issued, ms per launch}. bench.py prices the Merkle kernel's VALU fraction against the nominal 2.4 GHz AND against this clock:
 * devices of one model differ by up to 12 % on compute-bound loops, and a line that only knows the nominal clock cannot tell a slow device from a
 * slow kernel. Never part of a proof. */
int32_t bfhip_clock_probe(bfhip_ctx* ctx, double seconds, double out[6]);
/* The same question under the REAL dominant kernel: k_merkle_layer itself (an inner layer of 2^log_nodes nodes, 16 <= log_nodes <= 26, over pseudo-random hashes: VALU plus its memory traffic) is
 * launched back to back for `seconds` while a one-wave sampler on the context's other stream stamps the shader-cycle counter against the 100 MHz counter from before the
 * first launch until the host stops it — no stamp executes in the kernel itself. out = {GHz the device held under that mix, 10^9 compressions/s of the kernel on this shape,
 * launches, us per launch, 1 if the sampler spanned the window (0: it ran into its own bound and the clock is not to be trusted), seconds the sampler covered}. A device can
 * hold its clock under the register-only loop of bfhip_clock_probe and still be slow in a proof (measured, r06): probing the proof's own largest layer shape (log_nodes 25:
 * 3 GiB of hashes in flight) is what tells. Uses 96 B x 2^log_nodes of device memory for the duration of the call. Never part of a proof. */
int32_t bfhip_clock_probe_mix(bfhip_ctx* ctx, double seconds, uint32_t log_nodes, double out[6]);

#ifdef __cplusplus
}
#endif
#endif /* BFHIP_H */
