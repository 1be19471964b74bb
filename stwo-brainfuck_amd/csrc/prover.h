// The prover's host driver (prover.hip, prover_commit.hip, prover_oods.hip, prover_fri.hip) and its C ABI (api_prove.hip): the device-side
// bookkeeping types and struct HipProver. Internal to the library. One-line accessors and what sits on the per-launch path (Gather::add*,
// DCol, mark) are inline here; every other member is defined in the file named beside its declaration.
#pragma once
#include "../../include/bfhip.h"
#include "ctx.h"
#include "host/circle.h"
#include "host/quotients.h"
#include "host/proof.h"
#include <chrono>
#include <functional>
#include <map>
#include <string>
#include <vector>

namespace bf {

// tables.hip
void build_tables_device(Ctx& c, const std::vector<u32> trace7_soa[7], u32 n, const std::vector<u32>& code, const std::function<u32*(size_t)>& alloc,
                         std::vector<std::vector<u32*>>& cols_out, u32 log_sizes_out[13]);
// the same from a register trace that is already on the device (ingest.hip); the host-vector form uploads and calls this one
void build_tables_device(Ctx& c, const TraceSoA& t, const std::vector<u32>& code, const std::function<u32*(size_t)>& alloc,
                         std::vector<std::vector<u32*>>& cols_out, u32 log_sizes_out[13]);

static constexpr u32 OWNER_ALL = 0xFFFFFFFFu;   // a polynomial every rank of a shard group holds and transforms itself

struct DCol {
    u32* ptr = nullptr; u32 log_size = 0; u32 shift = 0;   // 2^log_size domain cells, stored as 2^(log_size - shift) u32
    // Row-sharded column of a shard group (lc = log2(ranks) > 0): this rank stores only its contiguous range of 2^(log_size - lc) rows and
    // `ptr` is a VIRTUAL BASE — the slice's address minus the range's first row — so that kernels keep addressing rows by their global
    // index; only rows of the rank's own range may be dereferenced.
    u32 lc = 0;
    bool sliced() const { return lc != 0; }
    size_t stored() const { return size_t(1) << (log_size - shift - lc); }
    ColDesc desc() const { return ColDesc{ptr, shift, 0}; }
    bool mine(u64 cell, u32 rank) const { return lc == 0 || (cell >> (log_size - lc)) == rank; }
};
// layer k: node i stored at i >> shifts[k]. In a shard group (Ctx::shard.count > 1) the layers k with band_lo < k <= band_hi hold only this
// rank's contiguous share of the nodes (node i belongs to rank i >> (k - log2 count)); layer band_lo and everything below is complete.
// cols: the tree's columns in descending size order (what the decommitment walks; kept from the commitment so that the last round trip of a
// proof does not sort 128 descriptors again)
struct DevMerkle { std::vector<u32*> layers; std::vector<u32> shifts; u32 max_log = 0; Hash32 root; int band_lo = 0, band_hi = -1; std::vector<DCol> cols; };
// owner[i]: the rank that holds polynomial i (coefficients) and computes its LDE, or OWNER_ALL. prev[i]: previous-row copy of evals[i]
// (row-sharded last logUp columns only; ptr == nullptr otherwise).
// is_first_closed: the preprocessed tree built without coefficient columns (build_preprocessed: polys[i].ptr == nullptr, evaluations written in closed
// form) — whoever needs IsFirst(n) elsewhere (an out-of-domain sample, the constraint domain) takes the closed form too (kernels.h: is_first_samples, is_first_lde).
struct DTree { std::vector<DCol> polys, evals, prev; std::vector<u32> owner; DevMerkle mk; bool is_first_closed = false; };
struct DSecure {
    u32* c[4]; u32 log_size; u32 lc = 0;     // lc > 0: row-sharded, c[] are virtual bases (see DCol)
    bool mine(u64 cell, u32 rank) const { return lc == 0 || (cell >> (log_size - lc)) == rank; }
};

struct Gather {
    std::vector<GatherReq> reqs;
    u32 n_words = 0;
    // each returns the position of the first gathered word in the output of run(); mine == false: another rank of the shard group holds
    // the word (this rank contributes a zero, the max-reduce completes it)
    size_t add(const u32* base, u64 idx, bool mine = true) { reqs.push_back({mine ? base : nullptr, idx, n_words, 1u}); n_words += 1; return n_words - 1; }
    size_t add_hash(const u32* layer, u64 node_slot, bool mine) { reqs.push_back({mine ? layer : nullptr, node_slot * 8, n_words, 8u}); n_words += 8; return n_words - 8; }
    size_t add_col(const DCol& col, u64 cell, u32 rank) { return add(col.ptr, cell >> col.shift, col.mine(cell, rank)); }
    // stamp_slot >= 0 (inside a proof, one process per proof): the host polls a stamp word written behind the gather instead of an event
    std::vector<u32> run(Ctx& c, int stamp_slot = -1);      // prover_fri.hip
};

// The prover's input once resident in HBM: row-granular main-trace columns of the 13 components (what the reference's
// `XTable::from(&vm_trace).trace_evaluation()` calls produce, mod.rs:511-547, minus the 16x lane broadcast).
struct TraceInput {
    std::vector<std::vector<DCol>> rows;   // [component][column]
    u32 log_sizes[N_COMPONENTS];
    u64 n_steps = 0, main_cells = 0, interaction_cells = 0;
    std::vector<u32*> owned;
    void release() { for (u32* p : owned) (void)hipFree(p); owned.clear(); rows.clear(); }
};

// Optional, off by default: the preprocessed tree (IsFirst columns) depends only on LOG_MAX_ROWS, so a deployment that proves many
// programs can commit it once per context and reuse polynomials, LDE columns and Merkle layers. The reference recomputes it in every
// prove_brainfuck call (mod.rs:495-500); bench.py's headline number does the same (reuse only with --reuse-preprocessed).
// The kept tree is only valid for the configuration it was built under: LOG_MAX_ROWS, the node-hash convention, the blowup and the shard group
// (share-wise layers hold one rank's share only) — any change rebuilds it.
struct PreprocessedCache {
    bool enabled = false, valid = false, replicate = false; u32 lmr = 0, node_conv = 0, channel = 0, log_blowup = 0, shard_rank = 0, shard_count = 1; DTree tree; Arena keep;
    bool matches(const Ctx& c, u32 log_max_rows) const {
        // the hasher is (merkle_channel, merkle_node_hash): a Blake2s tree must never serve a Poseidon252 proof or the reverse; the IsFirst LDE
        // lives on a domain of log_size + log_blowup_factor
        return enabled && valid && lmr == log_max_rows && node_conv == c.conv.merkle_node_hash && channel == c.conv.merkle_channel && log_blowup == c.pcs.log_blowup &&
               shard_rank == c.shard.rank && shard_count == c.shard.count && replicate == (c.shard.count > 1 && c.shard_replicate);
    }
};

// A pool's shared preprocessed tree (include/bfhip.h: bfhip_pool_*; pool.hip): committed ONCE per batch (or once per pool) by the pool's
// builder context and read by every proof of the batch instead of being recommitted by each — byte-neutral, the tree depends on LOG_MAX_ROWS,
// the hasher and the blowup only. The builder enqueues the commitment and records `ready` behind it BEFORE the workers are woken; a proof copies the
// layout at its start and waits (host side) for `ready` where it would have joined its own side stream, so the commitment runs beside the
// batch's first main-trace phases like a proof's own would.
struct SharedPreprocessed {
    bool valid = false; u32 lmr = 0, node_conv = 0, channel = 0, log_blowup = 0;
    DTree tree;                         // storage: the builder context's arena (not reset while a batch can read it)
    hipEvent_t ready = nullptr;         // recorded on the builder's stream behind the tree (and the root's copy into pinned memory)
    const Hash32* pinned_root = nullptr;
    u32 root_slot = 0;                  // which 32-byte slot of the builder's pinned block receives the root (a pool keeps two trees)
    bool matches(const Ctx& c, u32 log_max_rows) const {
        return valid && lmr == log_max_rows && node_conv == c.conv.merkle_node_hash && channel == c.conv.merkle_channel && log_blowup == c.pcs.log_blowup &&
               c.shard.count == 1;
    }
};

// ---- the AIRs asserted on the trace domain (check.hip): what bfhip_check_constraints / bfhip_trace_check (api_air.hip) and a proof's preflight
// (prover_preflight.hip) share --------------------------------------------------------------------------------------------------------------
inline CheckReportDev check_report_init() { CheckReportDev r{}; r.first_bad_cell = ~u64(0); r.first_bad_constraint = 0xffffffffu; return r; }
inline void check_report_fill(bfhip_check_report& out, const CheckReportDev& r, int component, u32 log_size, Q31 claimed) {
    out = bfhip_check_report{};
    out.component = (u32)component; out.log_size = log_size;
    out.n_bad_cells = r.n_bad_cells; out.first_bad_cell = r.first_bad_cell; out.first_bad_constraint = (int32_t)r.first_bad_constraint;
    for (int w = 0; w < 4; w++) out.first_bad_value[w] = r.first_bad_value[w];
    for (int j = 0; j < 16; j++) out.bad_per_constraint[j] = r.bad_per_constraint[j];
    out.claimed_sum[0] = claimed.a.a; out.claimed_sum[1] = claimed.a.b; out.claimed_sum[2] = claimed.b.a; out.claimed_sum[3] = claimed.b.b;
}
// main: row-granular; logup: 4 coordinate columns per logUp column, the last logUp column full size, earlier ones row-granular
inline CheckLaunch check_launch_of(int component, u32 log_size, const u32* const* main_rows, const u32* const* logup_cols, const Lookups& el, Q31 total_sum,
                                   CheckReportDev* d_report) {
    CheckLaunch L{};
    const u32 n_inter = 4 * n_logup_cols(component);
    for (u32 j = 0; j < n_main_cols(component); j++) L.trace[j] = ColDesc{main_rows[j], LOG_N_LANES, 0};
    for (u32 j = 0; j < n_inter; j++) L.inter[j] = ColDesc{logup_cols[j], j + 4 < n_inter ? LOG_N_LANES : 0u, 0};
    L.el = el; L.total_sum = total_sum; L.log_size = log_size; L.report = d_report;
    return L;
}
// The logUp pass of a whole-trace check: the 13 launches of logup_batch_init over the row-granular tables, their storage taken from the
// arena — per component the logUp coordinate columns (inter[k][j]; the last logUp column full size, earlier ones row-granular), then vrow,
// wloc and totals. d_claimed: the device address of the 13 claimed-sum slots. Every log size lies in [LOG_N_LANES, 29].
static inline std::vector<LogupLaunch> check_logup_launches(Ctx& c, const u32* rows[N_COMPONENTS][13], const u32 log_sizes[N_COMPONENTS], uint4* d_claimed,
                                                     const u32* inter[N_COMPONENTS][12]) {
    std::vector<LogupLaunch> logups(N_COMPONENTS);
    for (int k = 0; k < N_COMPONENTS; k++) {
        const u32 log_rows = log_sizes[k] - LOG_N_LANES, nl = n_logup_cols(k);
        const size_t M = size_t(1) << log_rows;
        LogupLaunch L{};
        for (u32 j = 0; j < n_main_cols(k); j++) L.cols[j] = rows[k][j];
        for (u32 j = 0; j < 4 * nl; j++) {
            u32* p = c.alloc_u32(j + 4 < 4 * nl ? M : 16 * M);
            inter[k][j] = p;
            if (j + 4 < 4 * nl) L.out_rep[j] = p; else L.out_last[j - 4 * (nl - 1)] = p;
        }
        L.vrow = c.arena.alloc(sizeof(uint4) * M);
        L.wloc = c.arena.alloc(sizeof(uint4) * M);
        L.totals = c.arena.alloc(sizeof(uint4) * (M / 1024 + 2));
        L.claimed = d_claimed + k;
        L.log_rows = log_rows; L.comp = k;
        logups[k] = L;
    }
    return logups;
}
// The lookup elements of bfhip_trace_check(.., NULL, ..): MemoryElements::draw, InstructionElements::draw, ProcessorElements::draw
// (mod.rs:589-597) on Blake2sChannel::default()
inline Lookups default_check_lookups() {
    Lookups el;
    Channel ch;
    { Q31 z, a; ch.draw_two_felts(z, a); el.memory = make_lookup(z, a); }
    { Q31 z, a; ch.draw_two_felts(z, a); el.instruction = make_lookup(z, a); }
    { Q31 z, a; ch.draw_two_felts(z, a); el.processor = make_lookup(z, a); }
    return el;
}

// waits for the context's main, side and partner streams
inline void sync_both(Ctx& c) { c.sync(); if (c.stream2) BF_HIP(hipStreamSynchronize(c.stream2)); for (auto a : c.aux) if (a) BF_HIP(hipStreamSynchronize(a)); }

struct PhaseTimes { double preprocessed = 0, main_trace = 0, interaction = 0, composition = 0, oods = 0, quotients = 0, fri = 0, decommit = 0, tables = 0, total = 0; };

struct HipProver {
    Ctx& c;
    PcsConfig cfg;
    u32 log_max_rows;
    Channel ch;
    PhaseTimes tm;
    std::string transcript;   // "name:hexdigest\n" per stage, for divergence hunting against the oracle
    bool want_transcript = false;

    HipProver(Ctx& ctx, u32 lmr) : c(ctx), cfg(ctx.pcs), log_max_rows(lmr) {}

    void tap(const char* name);      // prover.hip
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    // BFHIP_TRACE_HOST=1: host-side timestamps of the Fiat-Shamir round trips of a proof (label, microseconds since the proof started),
    // printed to stderr when the proof is done — what the host does while the GPU waits for a challenge (tools: point.py)
    std::vector<std::pair<const char*, double>> host_marks;
    bool trace_host = [] { const char* v = getenv("BFHIP_TRACE_HOST"); return v && (v[0] == '1' || v[0] == '2'); }();
    bool trace_host_mean = [] { const char* v = getenv("BFHIP_TRACE_HOST"); return v && v[0] == '2'; }();      // 2: means over every 20 proofs instead of every proof
    double mark_t0 = 0;
    void mark(const char* label) { if (trace_host) host_marks.push_back({label, (now() - mark_t0) * 1e6}); }
    void print_marks();      // prover.hip
    void check_config() const;      // prover.hip: what every proof and the pool's preprocessed build check first
    BrainfuckProof prove(const TraceInput& in) { return prove([&]() -> const TraceInput& { return in; }); }
    BrainfuckProof prove(const std::function<const TraceInput&()>& get_input);      // prover.hip
    // prover_preflight.hip (bfhip_ctx_set_preflight): the 13 AIRs and the logUp total asserted on the proof's tables before its main-trace
    // phase; fills c.preflight_last, throws TraceRejected for a trace that cannot be proved
    void preflight(const TraceInput& in);

    // ---- prover_commit.hip: transforms, Merkle trees, tree commitments, the preprocessed tree ------------------------------------------------
    FftPlan fft_prepare(bool inverse, const std::vector<DCol>& src, const std::vector<DCol>& dst);
    void fft_launch(const FftPlan& plan);
    void fft_cols(bool inverse, const std::vector<DCol>& src, const std::vector<DCol>& dst);
    // A phase's parameter blocks, staged by f(), reach the device in ONE copy: made by the kernel of mailbox mbx once the host posts (mailbox
    // order: the launches that follow wait behind it), or without a mailbox by the staging batch's copy at once.
    template <class F> void stage_blocks(Mailbox* mbx, F&& f) {
        if (mbx) { mbx->begin(); f(); mbx->arm(); }
        else { StageBatch sb(c); f(); sb.end(); }
    }

    // ---- Merkle (a4) -----------------------------------------------------------------------------------------------------------
    // defer_root: leave the 32-byte root copy pending in pinned memory (*pinned_root) instead of synchronising the stream.
    // no_readback: the root stays on the device (the caller collects it; FRI commit phase).
    // step: FRI commit phase — the device channel mixes the root and draws the next alpha right behind the tree (fused into the top kernel).
    struct ChannelStep { u32* chan; u32* alpha8; u32* root_copy; };
    // A tree is committed in two steps so that several trees can share ONE staging copy (the FRI commit phase plans all its layers first:
    // every separate copy is a ~9 us blit in front of the kernels that need it): merkle_plan = host-side layout (levels, replication shifts,
    // arena storage, column descriptors written to the staging ring — inside the caller's StageBatch), merkle_run = the launches.
    struct MerklePlan {
        DevMerkle mk; std::vector<DCol> cols; std::vector<size_t> off; std::vector<double> bytes; size_t n_all = 0;
        const ColDesc* d_all = nullptr; MerkleTreeDesc tree{}; bool poseidon = false;
        // launches: levels [max_log .. sub_hi + 1] one each (k_merkle_layer), [sub_hi .. 9] one (k_merkle_subtree; sub_hi == 0: none and the
        // single-level launches go down to fused_top), [fused_top - 1 .. 0] one (k_merkle_top; fused_top == 0: none)
        u32 fused_top = 0, sub_hi = 0;
        double top_bytes = 0, top_comp = 0, sub_bytes = 0, sub_comp = 0;
        // shard group: the band's last levels [band_lo .. band_fuse_hi] as ONE launch over this rank's share (k_merkle_subtree in its general
        // form, a workgroup per 2^band_fuse_r nodes of level band_lo); band_fuse_hi < 0: single-level launches all the way down
        int band_fuse_hi = -1; u32 band_fuse_r = 0; double band_bytes = 0, band_comp = 0;
        // FRI commit phase: the deepest level's four columns are PRODUCED by its launch (merkle.hip: k_fri_fold_leaf folds the previous layer
        // into them and hashes each row) — planned with folded_leaves = true, `fold` filled in before merkle_run
        bool folded_leaves = false; FriFoldLeafArgs fold{}; int fold_mode = -1;
    };
    MerklePlan merkle_plan(const std::vector<DCol>& cols_in, bool folded_leaves = false);
    // waits: before the level `level` (and everything below it) is hashed the stream waits for `ev` — the columns of that size are produced
    // on another stream while the larger layers are being hashed. Sorted by descending level.
    struct LevelWait { int level; hipEvent_t ev; };
    DevMerkle merkle_run(MerklePlan& p, Hash32* pinned_root = nullptr, bool no_readback = false, const ChannelStep* step = nullptr, const std::vector<LevelWait>* waits = nullptr,
                         int stamp_slot = -1, bool* stamped = nullptr);
    DevMerkle merkle_commit(const std::vector<DCol>& cols_in, Hash32* pinned_root = nullptr, bool no_readback = false, const ChannelStep* step = nullptr);

    // ---- shard group (one proof over several GPUs): which columns are cut into row ranges ---------------------------------------------
    // A full-size column of the preprocessed / interaction / composition trees, a quotient column or an FRI layer with at least 2^14 rows per rank is
    // ROW-sharded: rank r holds rows [r * 2^(log - lc), (r + 1) * 2^(log - lc)) — a contiguous range of a bit-reversed circle domain, i.e.
    // a sub-coset, so Merkle subtrees, offset-0 masks, quotient rows and FRI sibling pairs are all local. Smaller columns, the 16x-replicated
    // (row-granular) columns and the preprocessed / main trees stay complete on every rank.
    // 2^14 rows per rank: below that a transform, a fold or a subtree costs less than the latency of the exchange that would divide it
    static constexpr u32 SLICE_MIN_LOG_PER_RANK = 14;
    // a Merkle layer is hashed share-wise while a rank's share has at least 2^14 stored nodes (64 workgroups); see merkle_plan
    static constexpr u32 SHARE_MIN_LOG_PER_RANK = 14;
    bool sharded() const { return c.shard.count > 1; }
    u32 lc() const { return c.shard.log_count; }
    bool slice_log(u32 log) const { return sharded() && log >= lc() + SLICE_MIN_LOG_PER_RANK; }
    // Shard policy "replicate the transforms" (bfhip_ctx_set_shard_policy, r06): every rank interpolates and extends EVERY column itself and evaluates the
    // constraints on every row — no column -> row exchange, no rows -> columns exchange of the composition accumulators — while the Merkle band, the quotient
    // rows and the FRI folds stay divided by row range through VIRTUALLY sliced columns: DCol::lc is set and the storage is the whole column, so the virtual
    // base of DCol is the real base. What is exchanged shrinks to the per-tree all-gather of 256 nodes per rank and the max-reduces. For groups whose
    // exchange would cross ONE xGMI link (N = 2: 1.03 GB per proof and rank at 76 GB/s = 13.5 ms against 5.6 ms of transforms) — DESIGN.md section 7.
    bool replicate() const { return sharded() && c.shard_replicate; }
    // does this rank hold the coefficients / compute the LDE of a polynomial with this owner entry?
    bool transforms_here(u32 owner) const { return owner == OWNER_ALL || owner == c.shard.rank || replicate(); }
    // A 16x-replicated (row-granular, shift = 4) column is cut into row ranges when a rank's range still holds 2^14 STORED words — then every
    // layer it enters lies inside the share-wise Merkle band (merkle_plan) and its rows' constraint / quotient launches are range-restricted.
    bool slice_col(u32 log, u32 shift) const { return sharded() && log >= shift + lc() + SLICE_MIN_LOG_PER_RANK; }
    size_t slice_cells(u32 log) const { return size_t(1) << (log - lc()); }
    size_t slice_first(u32 log) const { return (size_t)c.shard.rank << (log - lc()); }
    u32* alloc_slice(u32 log, u32 shift = 0);
    std::vector<u32> assign_owners(const std::vector<DCol>& polys, u32 log_blowup) const;
    void commit_tree(DTree& t, Hash32* pinned_root = nullptr, bool with_prev = false);
    // evals_ready: t.evals already holds the evaluations (build_preprocessed) — no transforms, only the Merkle tree is planned and run
    void commit_tree_overlapped(DTree& t, Hash32* pinned_root, const std::vector<DCol>* interp_src = nullptr, int stamp_slot = -1, bool evals_ready = false);
    static void upload_trace(Ctx& c, const std::vector<Registers>& vm_trace, const std::vector<u32>& code, TraceInput& in, bool use_arena = false, bool on_gpu = true);
    // The same from the caller's register rows (n_rows x 7 u32) and program words: device-side ingestion (ingest.hip) + GPU table builders, or
    // with c.tables_on_gpu off the host path above. with_place: a non-canonical register is reported with its (row, register).
    static void upload_registers(Ctx& c, const u32* trace7_h, size_t n_rows, const u32* code_words_h, size_t n_code, TraceInput& in, bool use_arena, bool with_place);
    void build_preprocessed(DTree& tree, Hash32* pinned_root);
    void build_shared_preprocessed(SharedPreprocessed& sp);

    // ---- prover_oods.hip: composition polynomial, out-of-domain sampling, FRI quotients ------------------------------------------------------
    // ComponentProvers::compute_composition_polynomial + DomainEvaluationAccumulator::finalize
    // Everything about the 13 constraint launches that does not depend on the interaction phase's challenge-side results (random coefficient,
    // claimed sums): accumulators, column descriptors, vanishing inverses. Built while the GPU is still hashing the interaction tree.
    struct CompositionPlan {
        std::vector<ConstraintLaunch> launches; std::vector<DSecure> acc; std::vector<bool> have; u32 total = 0, max_log = 0;
        ConstraintLaunch* h_staged = nullptr;      // mailbox mode: the launch table in the staging ring, completed by composition_fill
    };
    CompositionPlan composition_prepare(std::vector<DTree>& trees, const BrainfuckProof& bp, const size_t* main_off, const size_t* inter_off, const Lookups& el);
    static void composition_challenge_fields(const BrainfuckProof& bp, u32 total, Q31 random_coeff, ConstraintLaunch* launches);
    void composition_fill(const BrainfuckProof& bp, CompositionPlan& cp, Q31 random_coeff);
    void compute_composition(std::vector<DTree>& trees, const BrainfuckProof& bp, CompositionPlan& cp, Q31 random_coeff, Mailbox* mbx = nullptr);
    // PolyOps::eval_at_point for every (column, mask point).
    // sample_prepare: the job list (addresses, sizes, which point) — known before the out-of-domain point is drawn.
    // isf: the samples of a tree with is_first_closed, evaluated in closed form into the same output slots
    struct SamplePlan { std::vector<EvalJob> jobs; std::vector<IsFirstSample> isf; u32 partial_off = 0, n_all = 0; };
    SamplePlan sample_prepare(const std::vector<DTree>& trees, const std::vector<std::vector<std::vector<u32>>>& mask);
    static void sample_factors(const std::vector<PtQ>& points, uint4* factors);
    struct SampleRun { uint4* h_factors = nullptr; uint4* d_out = nullptr; };
    SampleRun sample_launch(const SamplePlan& sp, const std::vector<PtQ>& points, Mailbox* mbx);
    const uint4* sample_results() const { return reinterpret_cast<const uint4*>(c.h_small + 4096); }
    void sample_unpack(const std::vector<DTree>& trees, const std::vector<std::vector<std::vector<u32>>>& mask, const uint4* out, u32 n_all, StarkProof& pf);
    void sample(const std::vector<DTree>& trees, const std::vector<std::vector<std::vector<u32>>>& mask, const std::vector<PtQ>& points, StarkProof& pf, const SamplePlan& sp);
    // compute_fri_quotients: one secure column per distinct LDE size, descending. A size group: the LDE columns of that size, their mask points
    // (ColumnSampleBatch::new_vec) and where each column's sampled values are in the proof.
    struct QuotientGroup {
        u32 log = 0; std::vector<ColDesc> descs; std::vector<ColSamples> cols; std::vector<std::pair<size_t, size_t>> src;   // (tree, column) per column
        QuotientBatch* h_batches = nullptr; QuotientEntry* h_entries = nullptr; size_t n_batches = 0, n_entries = 0;      // mailbox order: the staged tables
    };
    struct QuotientRun { std::vector<QuotientGroup> groups; std::vector<DSecure> out; };
    std::vector<QuotientGroup> quotient_groups(const std::vector<DTree>& trees, const std::vector<std::vector<std::vector<u32>>>& mask);
    static void quotient_constants(QuotientGroup& g, const std::vector<PtQ>& points, const StarkProof* pf, Q31 random_coeff,
                                   std::vector<QuotientBatch>& batches, std::vector<QuotientEntry>& entries);
    QuotientRun compute_quotients(const std::vector<DTree>& trees, const std::vector<std::vector<std::vector<u32>>>& mask, const std::vector<PtQ>& points,
                                  const StarkProof* pf, Q31 random_coeff, std::vector<LevelWait>* q_waits, Mailbox* mb0 = nullptr, Mailbox* mb1 = nullptr);
    void quotients_fill(QuotientRun& qr, const std::vector<PtQ>& points, const StarkProof& pf, Q31 random_coeff, Mailbox* mb0, Mailbox* mb1);

    // ---- prover_fri.hip: FRI commit phase, proof of work, decommitment -------------------------------------------------------------------------
    // MerkleProver::decommit — control flow on the host, data through one gather.
    // Requests go into the shared gather `g`; the returned closure fills the outputs once the gathered words are available.
    typedef std::function<void(const std::vector<u32>&)> Finisher;
    Finisher decommit(Gather& g, const DevMerkle& mk, const std::vector<DCol>& cols_in, const std::map<u32, std::vector<size_t>>& queries_per_log,
                      std::vector<u32>* queried_values, MerkleDecommitment* dec);
    static std::vector<size_t> fold_queries(const std::vector<size_t>& q, u32 n);
    static void positions_and_witness(const std::vector<size_t>& queries, std::vector<size_t>& positions, std::vector<size_t>& witness_pos);
    Finisher gather_secure_deferred(Gather& g, const DSecure& s, const std::vector<size_t>& pos, std::vector<Q31>* out);
    static std::vector<DCol> secure_cols(const DSecure& s);
    // what the commit phase hands to the decommitment: the first-layer tree over the coordinate columns of every quotient, and every inner
    // layer's evaluation with its tree
    // layers, path, d_alpha, d_chan: what the test hook of the commit phase (bfhip_test_fri_commit) reads back — every line layer (the last one
    // included), alpha || alpha^2 per channel step, the device channel, and per layer who produced it: path[k] = who folded layer k (FRI_BY_*),
    // | FRI_QUOTIENT when a circle evaluation was folded in, | who hashed its tree << 4 (FRI_NO_TREE: the last layer). Written by the driver
    // where it takes each decision.
    enum : u32 { FRI_BY_LAUNCHES = 0, FRI_BY_FOLD_LEAF = 1, FRI_BY_LAYER_KERNEL = 2, FRI_BY_TAIL = 3, FRI_QUOTIENT = 4, FRI_NO_TREE = 15 };
    static constexpr size_t FRI_MAX_LAYERS = 40;
    struct FriCommitted {
        struct Inner { DSecure ev; DevMerkle tree; }; DevMerkle first_tree; std::vector<DCol> first_cols; std::vector<Inner> inner;
        std::vector<DSecure> layers; std::vector<u32> path; u32* d_alpha = nullptr; u32* d_chan = nullptr;
    };
    // last_layer_poly = false (the test hook: arbitrary columns have no low degree): the 2^b evaluations of the last layer are left as they
    // are — no degree check, no coefficient mixed into the channel, pf untouched
    FriCommitted fri_commit(std::vector<DSecure>& quotients, StarkProof& pf, const std::vector<LevelWait>& q_waits, const std::function<void()>& while_the_commit_phase_runs,
                            bool last_layer_poly = true);
    void grind(StarkProof& pf);
    void decommit_queries(std::vector<DTree>& trees, const std::vector<DSecure>& quotients, const FriCommitted& fc, StarkProof& pf);
};

}  // namespace bf

// include/bfhip.h: a trace resident in HBM (bfhip_trace_create*); bf::trace_columns (prover.hip) hands its columns to the checkers
struct bfhip_trace { bf::TraceInput in; };
