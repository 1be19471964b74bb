// Proofs in flight as a capability of the library (include/bfhip.h: bfhip_pool_*): ONE caller thread — the reference's prove_brainfuck has a
// single thread of control (crates/brainfuck_prover/src/brainfuck_air/mod.rs:471-735; SURVEY.md section 8(b) "Who calls it") — hands a batch
// of resident traces (or of programs) to a pool of k sub-contexts on one GPU; k internal worker threads prove them, k at a time, and the call
// returns when every proof of the batch is done. While one proof sits in a single-workgroup chain (tree tops, small FRI layers) or waits for
// its host at a Fiat-Shamir point, the wide kernels of another fill the GPU: +19 % (2 in flight) / +23 % (3) at 2^22 rows, +36..57 % at 2^20
// (profiles/r05_inflight.jsonl, measured with k Python threads over k full contexts; this file makes it one C call).
//
// What the sub-contexts share (all byte-neutral):
//   - the twiddle tree and the circle-point tables of sub-context 0 (read-only after creation; 2 x 2^(max_log_domain - 1) words not held k times);
//   - by default ONE preprocessed commitment per batch (IsFirst(LOG_MAX_ROWS ..= 4): trace independent, mod.rs:495-500 recommits it in every
//     prove_brainfuck call): a builder context enqueues it before the workers start and every proof of the batch reads that tree
//     (prover.h: SharedPreprocessed). With it a worker needs ONE stream, so k workers + the builder stay within the 4 hardware queues a
//     process gets by default (ctx.h: ensure_aux / ensure_side).
// Everything else is per sub-context as before: arena, staging ring, pinned slots, streams.
//
// The same workers also serve a QUEUE (bfhip_pool_submit_* / bfhip_pool_wait): jobs start in ticket order on whichever worker is free and
// their results are taken in completion order. A pool is in one of the two uses at a time: a batch call is refused while jobs are outstanding
// and a submit is refused while a batch runs. In queue use the pool keeps up to two shared preprocessed trees (two values of LOG_MAX_ROWS
// interleaved in one stream both find theirs), each in an arena of its own that the builder context borrows for the commitment; a tree is
// recommitted only while no running job reads it.
//
// A fourth kind of job is an AIR given as a statement (bfhip_pool_submit_air): the worker runs bfhip_air_prove on its sub-context. The
// statement, the table of column pointers and the channel's state are copied at submit (air_statement_copy.h); program handles, device
// columns and kernels are borrowed. Such a job opens a commitment-scheme session, which a sub-context refuses while jobs are outstanding:
// the worker names itself in Ctx::pool_job_thread around the call, and only that thread passes. It takes no shared preprocessed tree and
// creates no stream: session, batch and composition all enqueue on the sub-context's one stream.
#include "../../include/bfhip.h"
#include "api_guard.h"
#include "prover.h"
#include "pcs_types.h"
#include "air_statement_copy.h"
#include <atomic>
#include <deque>
#include <new>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>
#include <string>
#include <chrono>

using namespace bf;

namespace {

struct Job {
    const bfhip_trace* const* traces = nullptr;            // kind 0: resident traces (bfhip_prove_trace per proof)
    const char* const* codes = nullptr;                     // kind 1: programs (bfhip_prove_brainfuck per proof: VM + tables inside the worker)
    const uint8_t* const* inputs = nullptr; const size_t* n_inputs = nullptr;
    uint32_t n = 0, log_max_rows = 0;
    char** json = nullptr; size_t* len = nullptr; int32_t* status = nullptr; double* seconds = nullptr;
    std::atomic<uint32_t> next{0}, failed{0};
    std::mutex err_mu; std::string first_error; uint32_t first_failed = 0xFFFFFFFFu;
};

// One job of the queue. What the caller may free after submit (program text, input, program words) is copied; register rows and traces are borrowed.
struct QJob {
    uint64_t ticket = 0, tag = 0; uint32_t log_max_rows = 0;
    int kind = 0;                                            // 0 resident trace, 1 program text, 2 register rows, 3 AIR statement
    const bfhip_trace* trace = nullptr;
    std::string code; std::vector<uint8_t> input;
    const uint32_t* rows = nullptr; size_t n_rows = 0; std::vector<uint32_t> words;
    // kind 3: the statement and the column pointers (copied), the channel's state (copied), row w of the caller's kernels for worker w (copied
    // pointers, n_in_flight x n_components, or empty)
    AirStatementCopy air; std::unique_ptr<bfhip_channel> channel; std::vector<bfhip_air_kernel*> kernels; uint32_t air_flags = 0;
    std::chrono::steady_clock::time_point submitted;
};

char* dup_text(const std::string& s) {
    char* p = (char*)malloc(s.size() + 1);
    if (p) memcpy(p, s.c_str(), s.size() + 1);
    return p;
}

}  // namespace

struct bfhip_pool {
    int device = 0; uint32_t k = 0, max_log_domain = 0;
    std::vector<bfhip_ctx*> subs;               // subs[0] owns the twiddle tree and the point tables
    bfhip_ctx* builder = nullptr;               // commits the shared preprocessed tree; its arena holds it
    // The shared preprocessed trees. A batch uses slot 0 only; the queue uses both. Each tree lives in its slot's arena, which the builder
    // context holds only while it enqueues the commitment (std::swap), so committing one tree never touches the memory of the other.
    struct PreSlot { SharedPreprocessed* sp = nullptr; Arena arena; uint32_t users = 0; uint64_t last_use = 0; };
    PreSlot slots[2];
    SharedPreprocessed*& shared = slots[0].sp;
    std::mutex pre_mu; uint64_t pre_clock = 0;   // guards slots[].users / last_use and the builder context in queue use
    int pre_mode = 1;                           // 0: every proof commits its own (the reference's behaviour), 1: once per batch, 2: kept across batches
    std::vector<std::thread> threads;
    std::mutex mu; std::condition_variable cv_work, cv_done;
    uint64_t generation = 0; bool quit = false; uint32_t active = 0;
    Job* job = nullptr;
    std::mutex call_mu;                         // batches of one pool are serial (a second caller thread waits)
    // ---- the queue (all under mu) ----
    std::deque<QJob*> queued; uint32_t running = 0; std::deque<bfhip_pool_result> done;
    uint64_t next_ticket = 1; bool batch_active = false;
    uint32_t calls_inside = 0;                  // submit / wait / cancel calls in progress: destroy waits for them
    std::condition_variable cv_result, cv_calls;
    uint32_t outstanding() const { return (uint32_t)queued.size() + running + (uint32_t)done.size(); }
    struct CallScope {                          // counts a queue call in progress; refuses once destroy has begun
        bfhip_pool* p; std::unique_lock<std::mutex> lk;
        explicit CallScope(bfhip_pool* p_) : p(p_), lk(p_->mu) { if (p->quit) throw HipError("the pool is being destroyed"); p->calls_inside++; }
        ~CallScope() { if (!lk.owns_lock()) lk.lock(); if (--p->calls_inside == 0) p->cv_calls.notify_all(); }
    };

    // commits slot's tree for (worker's conventions and config, log_max_rows) on the builder context, in the slot's own arena
    void build_slot(PreSlot& slot, const Ctx& like, uint32_t log_max_rows) {
        builder->c.conv = like.conv;
        builder->c.pcs = like.pcs;
        std::swap(builder->c.arena, slot.arena);
        try { shared_preprocessed_build(slot.sp, builder->c, log_max_rows); } catch (...) { std::swap(builder->c.arena, slot.arena); throw; }
        std::swap(builder->c.arena, slot.arena);
    }
    // queue use: the tree a job starting on sub-context w reads, or nullptr (mode 0; or both trees are being read by running jobs of another
    // LOG_MAX_ROWS / hasher / blowup: that job commits its own)
    PreSlot* acquire_tree(uint32_t w, uint32_t log_max_rows) {
        std::lock_guard<std::mutex> g(pre_mu);
        if (pre_mode == 0) return nullptr;
        Ctx& wc = subs[w]->c;
        PreSlot* pick = nullptr;
        for (auto& sl : slots) if (shared_preprocessed_matches(sl.sp, wc, log_max_rows)) { pick = &sl; break; }
        if (!pick) {
            for (auto& sl : slots) if (sl.users == 0 && (!pick || sl.last_use < pick->last_use)) pick = &sl;
            if (!pick) return nullptr;
            // a build the builder refuses (LOG_MAX_ROWS beyond the twiddle tree, ...) is not this job's last word: the proof itself reports it
            try { build_slot(*pick, wc, log_max_rows); } catch (...) { return nullptr; }
            if (!shared_preprocessed_matches(pick->sp, wc, log_max_rows)) return nullptr;      // e.g. a sub-context in a shard group
        }
        pick->users++; pick->last_use = ++pre_clock;
        return pick;
    }
    void release_tree(PreSlot* sl) { if (sl) { std::lock_guard<std::mutex> g(pre_mu); sl->users--; } }

    // Runs one queued job on sub-context w. Never throws: whatever the job throws, std::bad_alloc included, becomes its result.
    bfhip_pool_result run_queued(QJob& q, uint32_t w) {
        bfhip_pool_result r; memset(&r, 0, sizeof r);
        r.ticket = q.ticket; r.user_tag = q.tag; r.worker = w; r.log_max_rows = q.log_max_rows; r.status = -1;
        const auto t0 = std::chrono::steady_clock::now();
        r.seconds_queued = std::chrono::duration<double>(t0 - q.submitted).count();
        std::string err;
        PreSlot* tree = nullptr;
        char* js = nullptr; size_t n = 0;
        try {
            if (q.kind != 3) tree = acquire_tree(w, q.log_max_rows);
            subs[w]->c.shared_pre = tree ? tree->sp : nullptr;
            int32_t rc;
            if (q.kind == 3) {
                // the session this call opens is the worker's own: bfhip_pcs_create lets this thread pass while jobs are outstanding
                struct Own { Ctx& c; explicit Own(Ctx& c_) : c(c_) { c.pool_job_thread = std::this_thread::get_id(); } ~Own() { c.pool_job_thread = std::thread::id(); } } own(subs[w]->c);
                const size_t nk = q.air.st.n_components;
                rc = bfhip_air_prove(subs[w], &q.air.st, q.air.tree_cols.data(), q.kernels.empty() ? nullptr : q.kernels.data() + nk * w, q.channel.get(), q.air_flags, &js, &n);
            }
            else if (q.kind == 0) rc = bfhip_prove_trace(subs[w], q.trace, q.log_max_rows, &js, &n, nullptr, nullptr);
            else if (q.kind == 1) rc = bfhip_prove_brainfuck(subs[w], q.code.c_str(), q.input.data(), q.input.size(), q.log_max_rows, &js, &n, nullptr, nullptr);
            else rc = bfhip_prove_registers(subs[w], q.rows, q.n_rows, q.words.data(), q.words.size(), q.log_max_rows, &js, &n, nullptr, nullptr);
            if (rc == 0) { r.status = 0; r.proof_json = js; r.proof_len = n; r.flags = q.kind == 3 ? 0 : subs[w]->c.last_proof_flags; js = nullptr; }
            else { if (rc == BFHIP_TRACE_REJECTED) r.status = rc; err = bfhip_last_error(); }      // bad input, not an internal failure
        } catch (const std::exception& e) { err = e.what(); } catch (...) { err = "unknown error"; }
        subs[w]->c.shared_pre = nullptr;
        try { release_tree(tree); } catch (...) {}
        if (r.status != 0) {
            free(js);
            // the text is best effort (the allocation of the message may be what failed): status -1 is the result either way
            try { r.error = dup_text("job " + std::to_string(q.ticket) + ": " + err); } catch (...) { r.error = nullptr; }
        }
        r.seconds_proving = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return r;
    }

    void worker(uint32_t w) {
        uint64_t seen = 0;
        for (;;) {
            Job* j = nullptr; QJob* q = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_work.wait(lk, [&] { return quit || generation != seen || !queued.empty(); });
                if (quit) return;               // queued jobs are dropped by the destructor
                if (generation != seen) { seen = generation; j = job; }
                else { q = queued.front(); queued.pop_front(); running++; }
            }
            if (q) {
                bfhip_pool_result r = run_queued(*q, w);
                delete q;
                std::lock_guard<std::mutex> lk(mu);
                running--;
                // the deque's node is the one allocation between a finished job and its delivery: should it fail, the job is still accounted
                // for — as a failed one, without its buffers
                for (;;) {
                    try { done.push_back(r); break; }
                    catch (...) { free(r.proof_json); free(r.error); r.proof_json = nullptr; r.proof_len = 0; r.error = nullptr; r.status = -1; std::this_thread::yield(); }
                }
                cv_result.notify_all();
                continue;
            }
            for (uint32_t i; (i = j->next.fetch_add(1)) < j->n;) run_one(*j, w, i);
            {
                std::lock_guard<std::mutex> lk(mu);
                if (--active == 0) cv_done.notify_all();
            }
        }
    }
    void run_one(Job& j, uint32_t w, uint32_t i) {
        double phases[10] = {0};
        char* js = nullptr; size_t n = 0;
        int32_t rc;
        if (j.traces) rc = bfhip_prove_trace(subs[w], j.traces[i], j.log_max_rows, j.json ? &js : nullptr, &n, nullptr, phases);
        else rc = bfhip_prove_brainfuck(subs[w], j.codes[i], j.inputs ? j.inputs[i] : nullptr, j.inputs && j.n_inputs ? j.n_inputs[i] : 0, j.log_max_rows,
                                        j.json ? &js : nullptr, &n, nullptr, phases);
        if (j.json) j.json[i] = rc == 0 ? js : nullptr;
        if (j.len) j.len[i] = rc == 0 ? n : 0;
        if (j.status) j.status[i] = rc;
        if (j.seconds) j.seconds[i] = phases[9];
        if (rc != 0) {
            j.failed++;
            std::lock_guard<std::mutex> g(j.err_mu);
            if (i < j.first_failed) { j.first_failed = i; j.first_error = "proof " + std::to_string(i) + " of the batch: " + bfhip_last_error(); }
        }
    }
    int32_t run(Job& j) {
        std::lock_guard<std::mutex> call(call_mu);
        const auto t0 = std::chrono::steady_clock::now();
        {
            std::lock_guard<std::mutex> lk(mu);
            if (outstanding()) throw HipError("jobs outstanding: a batch call needs an empty queue (take every result with bfhip_pool_wait first)");
            batch_active = true;
        }
        struct BatchScope { bfhip_pool* p; ~BatchScope() { std::lock_guard<std::mutex> lk(p->mu); p->batch_active = false; } } batch_scope{this};
        for (uint32_t i = 0; i < j.n; i++) { if (j.json) j.json[i] = nullptr; if (j.len) j.len[i] = 0; if (j.status) j.status[i] = -1; if (j.seconds) j.seconds[i] = 0.0; }
        // the batch's preprocessed tree: enqueued on the builder's stream now, awaited by each proof where it first needs it
        const SharedPreprocessed* use = nullptr;
        if (pre_mode != 0 && j.n > 0) {
            builder->c.conv = subs[0]->c.conv;          // a worker whose conventions were changed individually does not match and commits its own
            builder->c.pcs = subs[0]->c.pcs;
            if (pre_mode == 1 || !shared_preprocessed_matches(shared, builder->c, j.log_max_rows)) build_slot(slots[0], builder->c, j.log_max_rows);
            use = shared;
        }
        for (auto* s : subs) s->c.shared_pre = use;
        {
            std::unique_lock<std::mutex> lk(mu);
            job = &j; active = k; generation++;
            cv_work.notify_all();
            cv_done.wait(lk, [&] { return active == 0; });
            job = nullptr;
        }
        for (auto* s : subs) s->c.shared_pre = nullptr;
        if (j.seconds) j.seconds[j.n] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (j.failed.load()) { bfhip_set_error(j.first_error); return -1; }
        return 0;
    }
    // settings change between uses only
    void require_idle(const char* what) {
        std::lock_guard<std::mutex> lk(mu);
        if (outstanding()) throw HipError(std::string(what) + ": jobs outstanding");
    }
    void invalidate_trees() { std::lock_guard<std::mutex> g(pre_mu); for (auto& sl : slots) shared_preprocessed_invalidate(sl.sp); }
    ~bfhip_pool() {
        {
            std::unique_lock<std::mutex> lk(mu);
            quit = true;
            cv_result.notify_all();
            cv_calls.wait(lk, [&] { return calls_inside == 0; });     // a waiter wakes, sees quit and leaves before anything is freed
        }
        cv_work.notify_all();
        for (auto& t : threads) if (t.joinable()) t.join();           // running jobs finish
        for (QJob* q : queued) delete q;                               // queued jobs are dropped
        for (auto& r : done) { free(r.proof_json); free(r.error); }    // untaken results and their buffers
        if (builder) { if (builder->c.stream) { (void)hipSetDevice(device); (void)hipStreamSynchronize(builder->c.stream); } }
        for (auto& sl : slots) { shared_preprocessed_destroy(sl.sp); sl.sp = nullptr; sl.arena.release(); }
        (void)bfhip_ctx_destroy(builder);
        for (size_t i = subs.size(); i-- > 0;) (void)bfhip_ctx_destroy(subs[i]);      // subs[0] (the tables' owner) last
    }
};

extern "C" {

int32_t bfhip_pool_create(int32_t device_id, uint32_t n_in_flight, uint32_t max_log_domain, bfhip_pool** out) {
    API_TRY
    if (!out) throw HipError("null argument");
    if (n_in_flight < 1 || n_in_flight > 16) throw HipError("bfhip_pool_create: n_in_flight must be in [1, 16]");
    bfhip_pool* pool = new bfhip_pool();
    try {
        pool->device = device_id; pool->k = n_in_flight; pool->max_log_domain = max_log_domain;
        for (uint32_t i = 0; i < n_in_flight; i++) {
            pool->subs.push_back(new bfhip_ctx());
            pool->subs.back()->c.init(device_id, max_log_domain, i ? &pool->subs[0]->c : nullptr);
            pool->subs.back()->c.pool_busy = [pool] { std::lock_guard<std::mutex> lk(pool->mu); return pool->batch_active || pool->outstanding() != 0; };
        }
        pool->builder = new bfhip_ctx();
        pool->builder->c.init(device_id, max_log_domain, &pool->subs[0]->c);
        for (uint32_t i = 0; i < 2; i++) { pool->slots[i].sp = shared_preprocessed_create(pool->builder->c); pool->slots[i].sp->root_slot = i; }
        for (uint32_t w = 0; w < n_in_flight; w++) pool->threads.emplace_back([pool, w] { pool->worker(w); });
    } catch (...) { delete pool; throw; }      // ~bfhip_pool joins the workers and releases whatever exists
    *out = pool;
    return 0;
    API_CATCH
}

int32_t bfhip_pool_destroy(bfhip_pool* pool) { API_TRY delete pool; return 0; API_CATCH }

int32_t bfhip_pool_size(bfhip_pool* pool, uint32_t* n_in_flight) { API_POOL(pool) if (!n_in_flight) throw HipError("null argument"); *n_in_flight = pool->k; return 0; API_CATCH }

int32_t bfhip_pool_ctx(bfhip_pool* pool, uint32_t i, bfhip_ctx** out) {
    API_POOL(pool)
    if (!out) throw HipError("null argument");
    if (i >= pool->k) throw HipError("bfhip_pool_ctx: index out of range");
    *out = pool->subs[i];
    return 0;
    API_CATCH
}

int32_t bfhip_pool_set_conventions(bfhip_pool* pool, const bfhip_conventions* conv) {
    API_POOL(pool)
    std::lock_guard<std::mutex> call(pool->call_mu);
    pool->require_idle("bfhip_pool_set_conventions");
    for (auto* s : pool->subs) if (bfhip_ctx_set_conventions(s, conv) != 0) return -1;
    if (bfhip_ctx_set_conventions(pool->builder, conv) != 0) return -1;
    pool->invalidate_trees();
    return 0;
    API_CATCH
}

int32_t bfhip_pool_set_pcs_config(bfhip_pool* pool, const bfhip_pcs_config* pcs) {
    API_POOL(pool)
    std::lock_guard<std::mutex> call(pool->call_mu);
    pool->require_idle("bfhip_pool_set_pcs_config");
    for (auto* s : pool->subs) if (bfhip_ctx_set_pcs_config(s, pcs) != 0) return -1;
    if (bfhip_ctx_set_pcs_config(pool->builder, pcs) != 0) return -1;
    pool->invalidate_trees();
    return 0;
    API_CATCH
}

int32_t bfhip_pool_set_preflight(bfhip_pool* pool, int32_t on) {
    API_POOL(pool)
    std::lock_guard<std::mutex> call(pool->call_mu);
    pool->require_idle("bfhip_pool_set_preflight");
    for (auto* s : pool->subs) if (bfhip_ctx_set_preflight(s, on) != 0) return -1;
    return 0;
    API_CATCH
}

int32_t bfhip_pool_set_preprocessed(bfhip_pool* pool, int32_t mode) {
    API_POOL(pool)
    if (mode < 0 || mode > 2) throw HipError("bfhip_pool_set_preprocessed: 0 = per proof, 1 = per batch, 2 = kept across batches");
    std::lock_guard<std::mutex> call(pool->call_mu);
    pool->require_idle("bfhip_pool_set_preprocessed");
    { std::lock_guard<std::mutex> g(pool->pre_mu); pool->pre_mode = mode; }
    if (mode != 2) pool->invalidate_trees();
    return 0;
    API_CATCH
}

int32_t bfhip_prove_batch(bfhip_pool* pool, const bfhip_trace* const* traces, uint32_t n, uint32_t log_max_rows, char** proofs_json, size_t* proof_lens,
                          int32_t* statuses, double* seconds) {
    API_POOL(pool)
    if (n && !traces) throw HipError("null argument");
    for (uint32_t i = 0; i < n; i++) if (!traces[i]) throw HipError("null trace in the batch");
    Job j; j.traces = traces; j.n = n; j.log_max_rows = log_max_rows; j.json = proofs_json; j.len = proof_lens; j.status = statuses; j.seconds = seconds;
    return pool->run(j);
    API_CATCH
}

int32_t bfhip_prove_batch_brainfuck(bfhip_pool* pool, const char* const* codes, const uint8_t* const* inputs_h, const size_t* n_inputs, uint32_t n,
                                    uint32_t log_max_rows, char** proofs_json, size_t* proof_lens, int32_t* statuses, double* seconds) {
    API_POOL(pool)
    if (n && !codes) throw HipError("null argument");
    if (inputs_h && !n_inputs) throw HipError("inputs without their lengths");
    for (uint32_t i = 0; i < n; i++) {
        if (!codes[i]) throw HipError("null program text in the batch");
        if (inputs_h && n_inputs[i] && !inputs_h[i]) throw HipError("null input in the batch");
    }
    Job j; j.codes = codes; j.inputs = inputs_h; j.n_inputs = n_inputs; j.n = n; j.log_max_rows = log_max_rows; j.json = proofs_json; j.len = proof_lens;
    j.status = statuses; j.seconds = seconds;
    return pool->run(j);
    API_CATCH
}

// ---- the queue ---------------------------------------------------------------------------------------------------------------------------
static int32_t pool_submit(bfhip_pool* pool, QJob* raw, uint64_t* ticket, const std::string& me = "bfhip_pool_submit") {
    std::unique_ptr<QJob> q(raw);
    bfhip_pool::CallScope call(pool);
    if (pool->batch_active) throw HipError(me + ": a batch call is in progress");
    if (pool->outstanding() >= BFHIP_POOL_MAX_OUTSTANDING) throw HipError(me + ": more than BFHIP_POOL_MAX_OUTSTANDING (4096) jobs outstanding");
    q->ticket = pool->next_ticket; q->submitted = std::chrono::steady_clock::now();
    pool->queued.push_back(q.get());
    *ticket = q.release()->ticket;
    pool->next_ticket++;
    pool->cv_work.notify_one();
    return 0;
}

int32_t bfhip_pool_submit_trace(bfhip_pool* pool, const bfhip_trace* trace, uint32_t log_max_rows, uint64_t user_tag, uint64_t* ticket) {
    API_POOL(pool)
    if (!trace || !ticket) throw HipError("null argument");
    QJob* q = new QJob(); q->kind = 0; q->trace = trace; q->log_max_rows = log_max_rows; q->tag = user_tag;
    return pool_submit(pool, q, ticket);
    API_CATCH
}

int32_t bfhip_pool_submit_brainfuck(bfhip_pool* pool, const char* code, const uint8_t* input_h, size_t n_input, uint32_t log_max_rows, uint64_t user_tag,
                                    uint64_t* ticket) {
    API_POOL(pool)
    if (!code || !ticket || (!input_h && n_input)) throw HipError("null argument");
    std::unique_ptr<QJob> q(new QJob()); q->kind = 1; q->code = code; q->log_max_rows = log_max_rows; q->tag = user_tag;
    if (n_input) q->input.assign(input_h, input_h + n_input);
    return pool_submit(pool, q.release(), ticket);
    API_CATCH
}

int32_t bfhip_pool_submit_registers(bfhip_pool* pool, const uint32_t* trace7_h, size_t n_rows, const uint32_t* code_words_h, size_t n_code,
                                    uint32_t log_max_rows, uint64_t user_tag, uint64_t* ticket) {
    API_POOL(pool)
    if (!trace7_h || !code_words_h || !ticket) throw HipError("null argument");
    if (n_rows == 0) throw HipError("EmptyTrace");
    if (n_rows >= (size_t(1) << 31)) throw HipError("bfhip_pool_submit_registers: n_rows >= 2^31");
    std::unique_ptr<QJob> q(new QJob()); q->kind = 2; q->rows = trace7_h; q->n_rows = n_rows; q->log_max_rows = log_max_rows; q->tag = user_tag;
    q->words.assign(code_words_h, code_words_h + n_code);      // n_code == 0 fails the job ("empty program"), like the one-call entry
    return pool_submit(pool, q.release(), ticket);
    API_CATCH
}

int32_t bfhip_pool_submit_air(bfhip_pool* pool, const bfhip_air_statement* statement, const uint32_t* const* const* tree_cols_h, bfhip_air_kernel* const* kernels_h,
                              const bfhip_channel* ch, uint32_t flags, uint64_t user_tag, uint64_t* ticket) {
    API_TRY
    const std::string me = "bfhip_pool_submit_air";
    if (!pool || !statement || !tree_cols_h || !ch || !ticket) throw HipError(me + ": null argument");
    // settings change only while nothing is outstanding, and jobs read them: the first sub-context's are the pool's
    const Ctx& c0 = pool->subs[0]->c;
    (void)air_statement_plan(me, statement, c0.pcs.log_blowup, c0.tw_root_log + 1);
    if (ch->conv.merkle_channel != c0.conv.merkle_channel || (c0.conv.merkle_channel == 0 && ch->conv.mix_u64 != c0.conv.mix_u64))
        throw HipError(me + ": the channel was created under other conventions (merkle_channel, mix_u64) than the pool's");
    std::unique_ptr<QJob> q(new QJob()); q->kind = 3; q->tag = user_tag; q->air_flags = flags;
    q->air.assign(me, statement, tree_cols_h);
    q->channel.reset(new bfhip_channel(*ch));
    if (kernels_h) q->kernels.assign(kernels_h, kernels_h + (size_t)pool->k * statement->n_components);
    return pool_submit(pool, q.release(), ticket, me);
    API_CATCH
}

int32_t bfhip_pool_set_scratch_reserve(bfhip_pool* pool, uint64_t bytes_per_worker) {
    API_POOL(pool)
    std::lock_guard<std::mutex> call(pool->call_mu);
    pool->require_idle("bfhip_pool_set_scratch_reserve");
    for (auto* s : pool->subs) if (bfhip_ctx_set_scratch_reserve(s, bytes_per_worker) != 0) return -1;
    return 0;
    API_CATCH
}

int32_t bfhip_pool_wait(bfhip_pool* pool, uint32_t timeout_ms, bfhip_pool_result* out) {
    API_POOL(pool)
    if (!out) throw HipError("null argument");
    bfhip_pool::CallScope call(pool);
    auto ready = [&] { return pool->quit || !pool->done.empty() || pool->outstanding() == 0; };
    if (timeout_ms == UINT32_MAX) pool->cv_result.wait(call.lk, ready);
    else if (timeout_ms) pool->cv_result.wait_for(call.lk, std::chrono::milliseconds(timeout_ms), ready);
    if (pool->quit) throw HipError("the pool is being destroyed");
    if (!pool->done.empty()) { *out = pool->done.front(); pool->done.pop_front(); return 0; }
    return pool->outstanding() ? 1 : 2;
    API_CATCH
}

int32_t bfhip_pool_outstanding(bfhip_pool* pool, uint32_t* queued, uint32_t* running, uint32_t* finished_not_taken) {
    API_POOL(pool)
    std::lock_guard<std::mutex> lk(pool->mu);
    if (queued) *queued = (uint32_t)pool->queued.size();
    if (running) *running = pool->running;
    if (finished_not_taken) *finished_not_taken = (uint32_t)pool->done.size();
    return 0;
    API_CATCH
}

int32_t bfhip_pool_cancel(bfhip_pool* pool, uint64_t ticket) {
    API_POOL(pool)
    bfhip_pool::CallScope call(pool);
    if (ticket == 0 || ticket >= pool->next_ticket) throw HipError("bfhip_pool_cancel: no such ticket");
    for (auto it = pool->queued.begin(); it != pool->queued.end(); ++it) {
        if ((*it)->ticket != ticket) continue;
        QJob* q = *it;
        bfhip_pool_result r; memset(&r, 0, sizeof r);
        r.ticket = q->ticket; r.user_tag = q->tag; r.log_max_rows = q->log_max_rows; r.status = BFHIP_JOB_CANCELLED;
        r.seconds_queued = std::chrono::duration<double>(std::chrono::steady_clock::now() - q->submitted).count();
        r.error = dup_text("job " + std::to_string(ticket) + ": cancelled");
        try { pool->done.push_back(r); } catch (...) { free(r.error); throw; }      // nothing changed: the job stays queued
        pool->queued.erase(it);
        delete q;
        pool->cv_result.notify_all();
        return 0;
    }
    return 1;
    API_CATCH
}

}  // extern "C"
