// Device-resident counterpart of prove_brainfuck (crates/brainfuck_prover/src/brainfuck_air/mod.rs:471-735) and of the stwo
// driver code it calls (CommitmentSchemeProver / TreeBuilder / prover::prove / FriProver). Everything that touches a column runs
// in the gfx950 kernels; the host keeps only the Fiat–Shamir channel, the sample/batch bookkeeping and the decommitment control
// flow (which depends on query positions, never on column data). There is no CPU fallback for any column operation.
// This file: the proof itself (HipProver::prove) and its host-side marks. prover_commit.hip, prover_oods.hip and prover_fri.hip hold the phases
// it calls, prover.h the types they share, api_prove.hip the C entry points.
#include <atomic>
#include "prover.h"
#include "host/verifier.h"
#include <algorithm>
#include <cstdio>
#include <mutex>
#include <thread>

namespace bf {

void HipProver::tap(const char* name) {
    if (!want_transcript) return;
    char buf[3]; transcript += name; transcript += ':';
    for (int i = 0; i < 32; i++) { snprintf(buf, sizeof buf, "%02x", ch.digest.b[i]); transcript += buf; }
    transcript += '\n';
}
void HipProver::print_marks() {
    if (!trace_host) return;
    if (trace_host_mean) {
        static std::mutex mu; static std::vector<std::pair<const char*, double>> sum; static int n = 0;
        std::lock_guard<std::mutex> g(mu);
        if (sum.size() != host_marks.size()) { sum.assign(host_marks.size(), {nullptr, 0.0}); n = 0; }
        double prev = 0;
        for (size_t i = 0; i < host_marks.size(); i++) { sum[i].first = host_marks[i].first; sum[i].second += host_marks[i].second - prev; prev = host_marks[i].second; }
        if (++n == 20) {
            double at = 0;
            for (auto& m : sum) { at += m.second / n; fprintf(stderr, "[bfhip host mean of 20] %10.1f us  (+%7.1f)  %s\n", at, m.second / n, m.first); }
            sum.clear(); n = 0;
        }
        return;
    }
    double prev = 0;
    for (auto& m : host_marks) { fprintf(stderr, "[bfhip host] %10.1f us  (+%7.1f)  %s\n", m.second, m.second - prev, m.first); prev = m.second; }
    fprintf(stderr, "[bfhip host] staging ring: %zu bytes in use after this proof\n", c.stage_used);
}

// What every proof and the pool's preprocessed build check first, before anything is enqueued (the context stays usable).
void HipProver::check_config() const {
    if (log_max_rows + cfg.log_blowup + 1 > c.tw_root_log + 1)
        throw HipError("context twiddle tree too small for log_max_rows " + std::to_string(log_max_rows) + " at log_blowup_factor " + std::to_string(cfg.log_blowup) +
                       ": create the context with max_log_domain >= " + std::to_string(log_max_rows + cfg.log_blowup + 1));
    if (cfg.log_last_layer_degree_bound != 0) throw HipError("the device prover supports log_last_layer_degree_bound 0 only");
    if (sharded() && !cfg.is_default()) throw HipError("a shard group proves under the default PcsConfig only");
    if (c.conv.merkle_channel == 1 && cfg.pow_bits > 12)
        throw HipError("Poseidon252 channel: pow_bits > 12 is not supported (its nonce search runs on the host), got " + std::to_string(cfg.pow_bits));
}

// get_input() runs on the host AFTER the (trace-independent) preprocessed phase has been enqueued, so a caller that still has to
// run the VM and build the tables overlaps that host work with GPU work (bfhip_prove_brainfuck does).
BrainfuckProof HipProver::prove(const std::function<const TraceInput&()>& get_input) {
    double t_start = now();
    mark_t0 = t_start;
    c.refuse_in_session("proof");
    check_config();
    struct SpinScope { Ctx& c; double saved; ~SpinScope() { c.spin_seconds = saved; } } spin_scope{c, c.spin_seconds};
    if (!c.sync_blocking) c.spin_seconds = 8e-3;      // bfhip_ctx_set_sync_policy(blocking): hosts with more contexts than cores keep the short poll
    c.arena.reset();
    // shard policy of this proof (every rank of a group resolves it the same way: same setting, same group size, and "spans several GPUs" is a
    // rendezvous decision): -1 = automatic = replicate the transforms for a group of TWO ranks on different GPUs (one xGMI link would carry 1 GB)
    c.shard_replicate = sharded() && (c.shard_policy == 1 || (c.shard_policy < 0 && c.shard.count == 2 && c.shard.comm && c.shard.comm->spans_devices()));
    // Mailboxes (mailbox.hip): one process per proof only — a shard group's exchanges are rendezvous points of their own. The ring must
    // not need recycling while a mailbox kernel waits for this thread, so it is recycled here, where nothing of this context is in flight.
    // Not by default under the blocking sync policy either: a mailbox kernel spins on the GPU until this thread posts, and a host that
    // asked for sleeping waits is one whose threads may be descheduled for long (BFHIP_MAILBOX=1 still forces it; wait_stamp then sleeps).
    c.use_mailbox = c.mailbox_mode < 0 ? (log_max_rows <= 21 && !c.sync_blocking) : c.mailbox_mode != 0;
    // At most ONE proof of the process runs in the mailbox order at a time (r05). HIP multiplexes the streams of all contexts onto a few
    // hardware queues; with two proofs in that order, A's stamp-producing kernels can sit behind B's spinning mailbox kernel on a shared
    // queue while B's sit behind A's — each host thread waits for a stamp that cannot be written until the other posts: both give up after
    // BFHIP_MAILBOX_TIMEOUT_MS (seen with three 2^20-row proofs in flight, profiles/r05_bench.json of the first pass). A proof that does not
    // get the token keeps the order wait -> draw -> copy -> launch: behind one spinning kernel it is merely later, never stuck.
    // The token is per GPU (hardware queues are per device), and a proof that unwinds on an error keeps it until its streams have drained:
    // its mailbox kernels may still be spinning (the Mailbox destructors, which run first, post them) and must not meet another proof's.
    struct MailboxToken {
        Ctx& c; bool held = false; int entered = std::uncaught_exceptions();
        explicit MailboxToken(Ctx& c_) : c(c_) {}
        static std::atomic<int>& flag(int device) { static std::atomic<int> f[64]; return f[device & 63]; }
        bool acquire() { int z = 0; held = flag(c.device).compare_exchange_strong(z, 1); return held; }
        ~MailboxToken() {
            if (!held) return;
            if (std::uncaught_exceptions() > entered) for (hipStream_t st : {c.stream, c.id_main, c.stream2}) if (st) (void)hipStreamSynchronize(st);
            flag(c.device).store(0);
        }
    } mailbox_token(c);
    if (c.use_mailbox && !sharded() && !(c.overlap & 2u) && !mailbox_token.acquire()) c.use_mailbox = false;
    const bool mb = c.use_mailbox && !sharded() && !(c.overlap & 2u);
    c.last_proof_flags = 0;       // completed below: what this proof actually did (bfhip_ctx_last_proof_flags)
    if (++c.proof_seq == 0) c.proof_seq = 1;
    c.reap_some();
    if (mb && c.stage_used > c.stage_bytes / 4) {
        sync_both(c);
        c.stage_used = 0;
    }
    for (int k = 0; k <= 5; k++) c.mailbox_err_host()[2 * k] = 0;
    Mailbox mb_logup(c, 1), mb_constraints(c, 2), mb_samples(c, 3), mb_quot0(c, 4), mb_quot1(c, 5);
    ch = Channel(c.conv);
    if (log_max_rows < LOG_N_LANES) throw HipError("log_max_rows must be at least LOG_N_LANES (4)");
    std::vector<DTree> trees(4);
    BrainfuckProof bp;

    // ---- Phase 0: preprocessed IsFirst(LOG_MAX_ROWS ..= LOG_N_LANES) (mod.rs:495-500) ---------------------------------
    // Trace independent, and nothing on the GPU depends on its root: it is enqueued on the side stream and runs beside the
    // caller's trace preparation (get_input) and the main-trace phase; both roots are read after ONE synchronisation and mixed
    // in protocol order (root0, claim, root1).
    double t0 = now();
    PreprocessedCache& cache = preprocessed_cache_of(c);
    Hash32* pinned_root0 = reinterpret_cast<Hash32*>(c.h_small);
    Hash32* pinned_root1 = pinned_root0 + 1;
    // a pool's batch (pool.hip): the tree its builder context commits once for all proofs of the batch
    const SharedPreprocessed* shared = c.shared_pre && c.shared_pre->matches(c, log_max_rows) ? c.shared_pre : nullptr;
    const bool reuse = shared || cache.matches(c, log_max_rows);
    BF_HIP(hipMemsetAsync(c.d_counters, 0, 4 * 64 * sizeof(u32), c.stream));      // ticket counters (a failed proof may have left one mid-count)
    BF_HIP(hipEventRecord(c.ev[0], c.stream));
    // In a shard group everything stays on the main stream: the group's exchanges are issued in one order on one stream per rank.
    const bool use_side = !sharded() && !c.single_stream;
    if (shared) trees[0] = shared->tree;        // layout only: complete (and its root known) once shared->ready has completed — awaited below
    else if (reuse) trees[0] = cache.tree;
    else {
        if (use_side) {
            c.ensure_side();
            BF_HIP(hipStreamWaitEvent(c.stream2, c.ev[0], 0));   // stream2 starts after whatever preceded this proof on the main stream
            std::swap(c.stream, c.stream2); c.side_busy = true;
        }
        try {
            if (cache.enabled) { cache.keep.reset(); std::swap(c.arena, cache.keep); }   // build the tree in memory that survives arena.reset()
            try { build_preprocessed(trees[0], pinned_root0); } catch (...) { if (cache.enabled) std::swap(c.arena, cache.keep); throw; }
            if (cache.enabled) std::swap(c.arena, cache.keep);
            BF_HIP(hipEventRecord(c.ev[1], c.stream));
        } catch (...) { if (use_side) { std::swap(c.stream, c.stream2); (void)hipStreamSynchronize(c.stream2); c.side_busy = false; } throw; }
        if (use_side) std::swap(c.stream, c.stream2);
    }
    // the side stream's work ends with ev[1]: when the event has completed there is nothing to wait for (a hipStreamSynchronize call
    // costs ~13 us even then — on the critical path of the first Fiat-Shamir round trip)
    auto join_side = [&]() {
        if (!c.side_busy) return;
        if (reuse || hipEventQuery(c.ev[1]) != hipSuccess) (void)hipStreamSynchronize(c.stream2);
        (void)hipGetLastError();
        c.side_busy = false;
    };
    const TraceInput* in_p = nullptr;
    try { in_p = &get_input(); } catch (...) { join_side(); throw; }
    const TraceInput& in = *in_p;
    // bfhip_ctx_set_preflight: a trace that cannot be proved is refused here, before anything of the main-trace phase is enqueued — the
    // side stream's commitment is joined as at the other early exits, and a pool's shared tree has not been awaited yet
    const bool preflight_ran = c.preflight && !sharded();
    if (preflight_ran) { try { preflight(in); } catch (...) { join_side(); throw; } }

    // ---- Phase 1: main trace (mod.rs:506-583) -----------------------------------------------------------------------------
    const std::vector<std::vector<DCol>>& rows = in.rows;   // row-granular table columns (also feed the logUp pass)
    size_t main_off[N_COMPONENTS], inter_off[N_COMPONENTS];
    {
        size_t mo = 0, io = 0;
        for (int k = 0; k < N_COMPONENTS; k++) { main_off[k] = mo; inter_off[k] = io; mo += n_main_cols(k); io += 4 * n_logup_cols(k); }
    }
    // Everything the logUp launches need apart from the lookup elements (storage of the 60 interaction columns, the scratch of the scans,
    // the launch table) is laid out while the GPU still hashes the main-trace tree (r04: 27 us off the first Fiat-Shamir round trip).
    uint4* d_claimed = nullptr;
    CompositionPlan composition_plan;
    SamplePlan sample_plan;
    std::vector<DCol> inter_vals;
    std::vector<LogupLaunch> logups(N_COMPONENTS);
    std::function<bool(size_t)> kept = [](size_t) { return true; };
    auto prepare_logup = [&]() {
        for (int k = 0; k < N_COMPONENTS; k++) bp.log_sizes[k] = in.log_sizes[k];
        // the claimed sums: in HBM for a shard group (read back at once), else written by the scan kernel into their pinned slot
        d_claimed = sharded() ? (uint4*)c.arena.alloc(sizeof(uint4) * N_COMPONENTS) : c.small_alias(reinterpret_cast<uint4*>(c.h_small + 2048));
        // the interaction columns in commit order (mod.rs:690-702): per component its logUp columns but the last row-granular (4 coordinates
        // each), then the last one full-size
        for (int k = 0; k < N_COMPONENTS; k++) {
            const u32 log = bp.log_sizes[k], nl = n_logup_cols(k);
            for (u32 j = 0; j < 4 * nl; j++) { DCol col; col.log_size = log; col.shift = j + 4 < 4 * nl ? LOG_N_LANES : 0; inter_vals.push_back(col); }
        }
        // Shard group: the full-size columns (each component's last logUp column, 4 coordinates) are column-sharded — only the owner of a
        // coordinate column keeps, interpolates and extends it, so only the owner has the logUp kernel write it (the others pass a null
        // pointer: no storage, no store); the row-granular columns and the small ones are written and transformed by every rank.
        if (sharded()) trees[2].owner = assign_owners(inter_vals, cfg.log_blowup);
        kept = [&](size_t i) { return !sharded() || transforms_here(trees[2].owner[i]); };
        for (size_t i = 0; i < inter_vals.size(); i++) if (kept(i)) inter_vals[i].ptr = c.alloc_u32(inter_vals[i].stored());
        for (int k = 0; k < N_COMPONENTS; k++) {
            u32 log = bp.log_sizes[k], log_rows = log - LOG_N_LANES;
            size_t M = size_t(1) << log_rows;
            LogupLaunch L{};
            for (u32 j = 0; j < n_main_cols(k); j++) L.cols[j] = rows[k][j].ptr;
            u32 nl = n_logup_cols(k);
            for (u32 j = 0; j + 4 < 4 * nl; j++) L.out_rep[j] = inter_vals[inter_off[k] + j].ptr;
            for (int w = 0; w < 4; w++) L.out_last[w] = inter_vals[inter_off[k] + 4 * (nl - 1) + w].ptr;
            L.vrow = c.arena.alloc(sizeof(uint4) * M);
            L.wloc = c.arena.alloc(sizeof(uint4) * M);
            L.totals = c.arena.alloc(sizeof(uint4) * (M / 1024 + 2));
            L.claimed = d_claimed + k;
            L.log_rows = log_rows; L.comp = k;       // L.el stays empty: the lookup elements, drawn after the main-trace root, go into the batch
            logups[k] = L;
        }
    };
    uint4* pinned_claimed = reinterpret_cast<uint4*>(c.h_small + 2048);
    Hash32* pinned_root2 = reinterpret_cast<Hash32*>(c.h_small + 2304);
    LogupBatch* h_lb = nullptr;           // the logUp batch in the staging ring (mailbox mode): its `el` is filled in after the draw
    // The 13 interaction_trace_evaluation calls (mod.rs:596-687) as one batch: four launches; one process per proof: then the interaction
    // tree. mbx: the launches wait behind that mailbox, and the staged batch is returned for the host to fill in the lookup elements.
    auto enqueue_interaction = [&](const Lookups& el, Mailbox* mbx) {
        LogupBatch lb;
        logup_batch_init(lb, el, logups.data(), N_COMPONENTS);
        c.stage_checkpoint();
        if (mbx) mbx->begin();
        const LogupBatch* d_lb = c.stage(&lb, 1);
        if (mbx) mbx->arm();
        logup_batch_run(c.stream, d_lb, lb);
        mark("logUp launched");
        BF_HIP(hipGetLastError());
        trees[2].polys = inter_vals;                  // interpolate in place
        if (!sharded()) commit_tree_overlapped(trees[2], pinned_root2, &inter_vals, mbx ? 2 : -1);
        return mbx ? mbx->host(d_lb) : nullptr;
    };
    try {
        for (int k = 0; k < N_COMPONENTS; k++) {
            bp.log_sizes[k] = in.log_sizes[k];
            if (bp.log_sizes[k] > log_max_rows) throw HipError("a component exceeds LOG_MAX_ROWS");
            for (u32 j = 0; j < n_main_cols(k); j++) { DCol p = rows[k][j]; p.ptr = nullptr; trees[1].polys.push_back(p); }
        }
        {
            std::vector<DCol> src;
            for (int k = 0; k < N_COMPONENTS; k++) for (auto& r : rows[k]) src.push_back(r);
            if (sharded()) {
                // Shard group: the main-trace columns are column-sharded like the other trees' — a column of at least 2^14 stored words
                // per rank after the extension is interpolated and extended by its owner only, which then hands every rank its row
                // range (row-granular: a sixteenth of the bytes of a full-size column); the small ones are transformed by every rank.
                trees[1].owner = assign_owners(trees[1].polys, cfg.log_blowup);
                std::vector<DCol> s_mine, p_mine;
                for (size_t i = 0; i < src.size(); i++) {
                    if (!transforms_here(trees[1].owner[i])) continue;
                    trees[1].polys[i].ptr = c.alloc_u32(trees[1].polys[i].stored());
                    s_mine.push_back(src[i]); p_mine.push_back(trees[1].polys[i]);
                }
                fft_cols(true, s_mine, p_mine);
                commit_tree(trees[1], pinned_root1);
            } else {
                for (auto& p : trees[1].polys) p.ptr = c.alloc_u32(p.stored());
                commit_tree_overlapped(trees[1], pinned_root1, &src, mb ? 1 : -1);
            }
        }
        BF_HIP(hipEventRecord(c.ev[2], c.stream));
        mark("main tree enqueued");
        prepare_logup();                 // host work under the main tree's kernels: only the lookup elements are missing afterwards
        if (mb) {
            // the whole interaction phase goes onto the stream now, behind a mailbox that will deliver the lookup elements
            h_lb = enqueue_interaction(Lookups{}, &mb_logup);
            mark("interaction phase enqueued behind its mailbox");
            c.wait_stamp(1);
        } else c.sync();
        mark("main root arrived");
    } catch (...) { join_side(); throw; }
    join_side();
    mark("side stream joined");
    if (shared) {
        // The batch's tree: its commitment was enqueued on the builder's stream before this proof started. Nothing of this proof has read it
        // yet; from here on the constraint, sampling, quotient and decommitment launches do, so the host waits for it here (normally long done).
        const auto w0 = std::chrono::steady_clock::now();
        for (u32 polls = 0;; polls++) {
            hipError_t e = hipEventQuery(shared->ready);
            if (e == hipSuccess) break;
            if (e != hipErrorNotReady) BF_HIP(e);
            if (polls > 64) std::this_thread::yield();
            if ((polls & 1023u) == 1023u && std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count() > 120.0)
                throw HipError("pool: the batch's shared preprocessed commitment did not complete");
        }
        trees[0].mk.root = *shared->pinned_root;
        mark("shared preprocessed tree ready");
    }
    if (!reuse) {
        trees[0].mk.root = *pinned_root0;
        if (cache.enabled) {
            cache.tree = trees[0]; cache.lmr = log_max_rows; cache.node_conv = c.conv.merkle_node_hash; cache.channel = c.conv.merkle_channel; cache.log_blowup = cfg.log_blowup;
            cache.shard_rank = c.shard.rank; cache.shard_count = c.shard.count; cache.replicate = replicate(); cache.valid = true;
        }
    }
    trees[1].mk.root = *pinned_root1;
    ch.mix_root(trees[0].mk.root);
    tap("root0");
    for (int k = 0; k < N_COMPONENTS; k++) ch.mix_u64(bp.log_sizes[k]);   // claim.mix_into (mod.rs:102-116)
    ch.mix_root(trees[1].mk.root);
    tap("root1");
    // the host wall time of the two overlapped phases; split in proportion to their GPU-side durations once the events behind them have
    // certainly completed (at the end of the proof: a stamp can arrive before the event recorded behind the kernel that wrote it)
    const double wall_phase01 = now() - t0;

    // ---- Phase 2: interaction trace (mod.rs:589-723) ------------------------------------------------------------------------
    t0 = now();
    Lookups el;
    { Q31 z, a; ch.draw_two_felts(z, a); el.memory = make_lookup(z, a); }         // MemoryElements::draw
    { Q31 z, a; ch.draw_two_felts(z, a); el.instruction = make_lookup(z, a); }    // InstructionElements::draw
    { Q31 z, a; ch.draw_two_felts(z, a); el.processor = make_lookup(z, a); }      // ProcessorElements::draw
    mark("lookup elements drawn");
    auto take_claimed = [&](const uint4* h_claimed) {
        for (int k = 0; k < N_COMPONENTS; k++) bp.claimed_sums[k] = q_make(h_claimed[k].x, h_claimed[k].y, h_claimed[k].z, h_claimed[k].w);
        for (int k = 0; k < N_COMPONENTS; k++) ch.mix_felts(&bp.claimed_sums[k], 1);   // interaction_claim.mix_into (mod.rs:189-203)
    };
    // per tree, per column: list of point indices (Components::mask_points + composition mask); independent of the challenges
    std::vector<std::vector<std::vector<u32>>> mask(4);
    auto build_mask = [&]() {
        mask[0].assign(trees[0].polys.size(), {});
        for (int k = 0; k < N_COMPONENTS; k++) mask[0][log_max_rows - bp.log_sizes[k]] = {0};
        for (int k = 0; k < N_COMPONENTS; k++) {
            for (u32 j = 0; j < n_main_cols(k); j++) mask[1].push_back({0});
            u32 ni = 4 * n_logup_cols(k);
            // last logUp column of a component: offsets {0, -1} (LogupAtRow::finalize); which comes first is Conventions::logup_mask_order
            for (u32 j = 0; j < ni; j++) {
                if (j + 4 >= ni) { if (c.conv.logup_mask_order == 1) mask[2].push_back({(u32)(1 + k), 0}); else mask[2].push_back({0, (u32)(1 + k)}); }
                else mask[2].push_back({0});
            }
        }
        mask[3].assign(4, {0});
    };
    Hash32* pinned_root3 = reinterpret_cast<Hash32*>(c.h_small + 2368);
    Q31 random_coeff;
    if (mb) {
        // The logUp kernels and the interaction tree are already on the stream, behind their mailbox: hand over the lookup elements.
        h_lb->el = el;
        mb_logup.post();
        mark("lookup elements posted");
        // ---- prover::prove (mod.rs:732): the composition phase goes onto the stream behind ITS mailbox while the GPU works on the
        // interaction phase: the 13 constraint launches (coefficient powers and claimed sums still empty), the composition transforms,
        // the composition tree, a stamp
        composition_plan = composition_prepare(trees, bp, main_off, inter_off, el);
        compute_composition(trees, bp, composition_plan, q_zero(), &mb_constraints);
        build_mask();
        commit_tree_overlapped(trees[3], pinned_root3, nullptr, 3);
        sample_plan = sample_prepare(trees, mask);
        mark("composition phase enqueued behind its mailbox");
        c.wait_stamp(2);
        mark("interaction root arrived");
        take_claimed(pinned_claimed);
        trees[2].mk.root = *pinned_root2;
        ch.mix_root(trees[2].mk.root);
        tap("root2");
        tm.interaction = now() - t0;
        t0 = now();
        random_coeff = ch.draw_felt();
        composition_fill(bp, composition_plan, random_coeff);
        mb_constraints.post();
        mark("random coefficient posted");
    } else {
        enqueue_interaction(el, nullptr);
        if (sharded()) {
            uint4 h_claimed[N_COMPONENTS];
            c.read_back(h_claimed, d_claimed, sizeof(h_claimed));
            take_claimed(h_claimed);
            std::vector<DCol> mine_cols;
            for (size_t i = 0; i < inter_vals.size(); i++) if (kept(i)) mine_cols.push_back(inter_vals[i]);
            fft_cols(true, mine_cols, mine_cols);
            commit_tree(trees[2], nullptr, /*with_prev=*/true);
        } else {
            // Nothing on the GPU waits for the claimed sums: they travel to their pinned slot behind the logUp kernels, the interaction tree is
            // enqueued right away, and the host mixes claim and root in protocol order after ONE synchronisation (no idle gap between the logUp
            // kernels and the transforms).
            composition_plan = composition_prepare(trees, bp, main_off, inter_off, el);      // host work under the tree's kernels
            mark("interaction tree enqueued + composition prepared");
            c.sync();
            mark("interaction root arrived");
            take_claimed(pinned_claimed);
            trees[2].mk.root = *pinned_root2;
            ch.mix_root(trees[2].mk.root);
        }
        tap("root2");
        tm.interaction = now() - t0;

        // ---- prover::prove (mod.rs:732): composition polynomial -------------------------------------------------------------
        t0 = now();
        random_coeff = ch.draw_felt();
        if (sharded()) composition_plan = composition_prepare(trees, bp, main_off, inter_off, el);
        compute_composition(trees, bp, composition_plan, random_coeff);
        mark("constraints + composition transforms launched");
        build_mask();
        if (sharded()) commit_tree(trees[3]);
        else {
            // the composition tree is enqueued; the sampling jobs (which only need the polynomials' addresses) are listed while it is hashed
            commit_tree_overlapped(trees[3], pinned_root3);
            sample_plan = sample_prepare(trees, mask);
            mark("composition tree enqueued + samples prepared");
        }
    }

    // ---- OODS sampling (a8) ------------------------------------------------------------------------------------------------------
    // sample points: index 0 = P, 1 + k = P - trace_step(component k)
    std::vector<PtQ> points(1 + N_COMPONENTS);
    PtQ oods;
    auto draw_oods = [&]() {
        Q31 t = ch.draw_felt();
        Q31 t2 = q_mul(t, t);
        Q31 d = q_inv(q_addm(t2, 1));
        oods.x = q_mul(q_sub(q_one(), t2), d);
        oods.y = q_mul(q_add(t, t), d);
        points[0] = oods;
        for (int k = 0; k < N_COMPONENTS; k++) points[1 + k] = pq_add(oods, pq_neg(to_q(index_to_point(subgroup_gen(bp.log_sizes[k])))));
    };
    auto mix_samples = [&]() {
        std::vector<Q31> flat;
        for (auto& t : bp.proof.sampled_values) for (auto& col : t) for (auto& v : col) flat.push_back(v);
        ch.mix_felts(flat.data(), flat.size());
    };
    std::vector<LevelWait> q_waits;
    std::vector<DSecure> quotients;
    if (mb) {
        // the sampling kernels behind their mailbox (the point's factor tables still empty) while the GPU evaluates the constraints
        const SampleRun sr = sample_launch(sample_plan, points, &mb_samples);
        c.post_stamp(4);
        mark("sampling enqueued behind its mailbox");
        c.wait_stamp(3);
        mark("composition root arrived");
        trees[3].mk.root = *pinned_root3;
        ch.mix_root(trees[3].mk.root);
        tap("root3");
        tm.composition = now() - t0;
        t0 = now();
        draw_oods();
        sample_factors(points, sr.h_factors);
        mb_samples.post();
        mark("out-of-domain point posted");
        // the quotient kernels behind two mailboxes (largest size group; the rest): batch structure from the points, sampled values still empty
        QuotientRun qr = compute_quotients(trees, mask, points, nullptr, q_one(), nullptr, &mb_quot0, &mb_quot1);
        BF_HIP(hipEventRecord(c.ev[5], c.stream));
        quotients = qr.out;
        mark("quotients enqueued behind their mailboxes");
        c.wait_stamp(4);
        sample_unpack(trees, mask, sample_results(), sample_plan.n_all, bp.proof);
        mark("sampled values arrived");
        mix_samples();
        tap("sampled");
        tm.oods = now() - t0;
        t0 = now();
        Q31 q_coeff = ch.draw_felt();
        mark("sampled values mixed, quotient coefficient drawn");
        quotients_fill(qr, points, bp.proof, q_coeff, &mb_quot0, &mb_quot1);
        mark("quotient constants posted");
    } else {
        if (!sharded()) {
            c.sync();
            mark("composition root arrived");
            trees[3].mk.root = *pinned_root3;
            ch.mix_root(trees[3].mk.root);
        }
        tap("root3");
        tm.composition = now() - t0;
        t0 = now();
        draw_oods();
        if (sharded()) sample_plan = sample_prepare(trees, mask);
        sample(trees, mask, points, bp.proof, sample_plan);
        mark("sampled values arrived");
        mix_samples();
        tap("sampled");
        tm.oods = now() - t0;

        // ---- FRI quotients (a9) ----------------------------------------------------------------------------------------------------
        t0 = now();
        Q31 q_coeff = ch.draw_felt();
        mark("sampled values mixed, quotient coefficient drawn");
        BF_HIP(hipEventRecord(c.ev[4], c.stream));
        quotients = compute_quotients(trees, mask, points, &bp.proof, q_coeff, &q_waits).out;
        BF_HIP(hipEventRecord(c.ev[5], c.stream));
        mark("quotients launched");
    }
    // no host wait here: the FRI phase is planned (layer storage, 26 tree layouts, one staging copy) while the quotient kernels run;
    // the phase time comes from the two events


    // ---- FRI commit (a10), proof of work (a11), decommitment (a12) -------------------------------------------------------------------
    // Sanity check of prover::prove (composition OODS value == constraints evaluated on the sampled mask values): host arithmetic on values
    // known since the sampling — done while the GPU runs the FRI commit phase, not after the proof's last kernel (r04)
    auto mailbox_gave_up = [&]() { for (int k = 1; k <= 5; k++) if (c.mailbox_err_host()[2 * k]) return true; return false; };
    const char* mailbox_msg = "a mailbox kernel gave up waiting for the host (BFHIP_MAILBOX_TIMEOUT_MS): the proof was computed from stale challenge words";
    auto sanity_check = [&]() {
        // the mailbox error words are final here (every mailbox kernel ran before stamp 4 was written): a kernel that gave up made the
        // phases run on stale challenge words, and THAT is the error to report — not the constraint mismatch it causes
        if (mb && mailbox_gave_up()) throw HipError(mailbox_msg);
        Q31 want = eval_composition_at_point(bp.log_sizes, bp.claimed_sums, log_max_rows, el, oods, bp.proof.sampled_values, random_coeff, c.conv);
        const auto& cv = bp.proof.sampled_values[3];
        std::vector<Q31> ce[4] = {cv[0], cv[1], cv[2], cv[3]};
        if (!q_eq(HostPointEval::combine(ce, 0), want)) throw HipError("ConstraintsNotSatisfied");
    };
    const FriCommitted fri = fri_commit(quotients, bp.proof, q_waits, sanity_check);
    grind(bp.proof);
    decommit_queries(trees, quotients, fri, bp.proof);
    for (int k = 1; k <= 5; k++) if (c.mailbox_err_host()[2 * k]) *c.mailbox_err_host() = c.mailbox_err_host()[2 * k];
    if (mb && trace_host) {
        // how long each mailbox kernel waited for the host (second word of its error slot, GPU clock in 10 ns ticks), as that far after the previous mark
        static const char* const waited[5] = {"mailbox 1 waited for the host (GPU clock, 10 ns ticks):", "mailbox 2 waited", "mailbox 3 waited", "mailbox 4 waited", "mailbox 5 waited"};
        for (int k = 1; k <= 5; k++) host_marks.push_back({waited[k - 1], host_marks.back().second + c.mailbox_err_host()[2 * k + 1] * 0.01});
    }
    if (*c.mailbox_err_host()) throw HipError(mailbox_msg);
    {
        float ms0 = 0.f, ms1 = 0.f;
        if (!reuse) BF_HIP(hipEventElapsedTime(&ms0, c.ev[0], c.ev[1]));
        BF_HIP(hipEventElapsedTime(&ms1, c.ev[0], c.ev[2]));
        const double tot = (double)ms0 + (double)ms1;
        tm.preprocessed = tot > 0 ? wall_phase01 * ms0 / tot : 0.0;
        tm.main_trace = wall_phase01 - tm.preprocessed;
    }
    {
        float ms_q = 0.f;
        BF_HIP(hipEventElapsedTime(&ms_q, c.ev[4], c.ev[5]));      // both completed: decommit_queries ends with host waits
        tm.quotients = ms_q * 1e-3;
        tm.fri = (now() - t0) - tm.quotients;
    }

    c.last_proof_flags = (c.last_proof_flags & 48u) | (mb ? 1u : 0u) | (reuse && !shared ? 2u : 0u) | (shared ? 4u : 0u) | (replicate() ? 8u : 0u) | (preflight_ran ? 64u : 0u);
    tm.total = now() - t_start;
    mark("done");
    print_marks();
    return bp;
}

}  // namespace bf

// api_air.hip (bfhip_trace_check): the row-granular main-trace columns and the log sizes of a resident trace
void bf::trace_columns(const bfhip_trace* t, const u32* cols[N_COMPONENTS][13], u32 log_sizes[N_COMPONENTS]) {
    for (int k = 0; k < N_COMPONENTS; k++) {
        log_sizes[k] = t->in.log_sizes[k];
        for (u32 j = 0; j < n_main_cols(k); j++) cols[k][j] = t->in.rows[k][j].ptr;
    }
}
