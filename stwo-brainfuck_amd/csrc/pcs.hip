// The prover half of the commitment-scheme session (include/bfhip.h "Commitment-scheme session"): stwo's CommitmentSchemeProver over trees of
// ARBITRARY columns — tree_builder.extend_evals / extend_polys + commit, then prove_values — driven through the pieces HipProver::prove() is
// made of (prover.h): commit_tree, sample_prepare / sample, compute_quotients, fri_commit, grind, decommit_queries. Nothing of them is
// restated here; this file checks the caller's description, keeps the trees and moves the caller's channel in and out of the driver.
// Launch order: the plain one (wait -> draw -> copy -> launch). No mailbox, and the context's overlap mask is not consulted: commit_tree is
// the one-stream commitment, compute_quotients gets no level waits and fri_commit an empty wait list. Columns are full size (shift 0).
// The host-only half (channel, verifier session) is pcs_host.hip.
#include "prover.h"
#include "api_guard.h"
#include "pcs_types.h"

using namespace bf;

struct bfhip_pcs {
    bfhip_ctx* ctx;
    HipProver pv;                        // cfg = the context's PcsConfig when the session was created
    Conventions conv;                    // the context's conventions at that moment (they cannot change while the session is open)
    std::vector<DTree> trees;
    bool proved = false;                 // prove_values was called: only tree_columns and destroy remain
    Arena::Mark before;                  // the arena's bookkeeping when the session was created, put back by destroy
#ifdef BFHIP_TEST_HOOKS
    std::vector<u32> fri_path;           // HipProver::FriCommitted::path of prove_values (bfhip_test_pcs_fri_path)
#endif
    explicit bfhip_pcs(bfhip_ctx* x) : ctx(x), pv(x->c, 0), conv(x->c.conv) {}
};

namespace {

// every stream of the context: before the arena is handed out again, and before an error unwinds under running kernels
void drain(Ctx& c) { for (hipStream_t st : {c.stream, c.id_main, c.stream2, c.aux[0], c.aux[1]}) if (st) (void)hipStreamSynchronize(st); }

void check_channel(const bfhip_pcs* s, const bfhip_channel* ch, const char* what) {
    if (ch->conv.merkle_channel != s->conv.merkle_channel || (s->conv.merkle_channel == 0 && ch->conv.mix_u64 != s->conv.mix_u64))
        throw HipError(std::string(what) + ": the channel was created under other conventions (merkle_channel, mix_u64) than the session's context");
}

}  // namespace

extern "C" {

int32_t bfhip_pcs_create(bfhip_ctx* ctx, bfhip_pcs** out) {
    API_CTX(ctx)
    if (!out) throw HipError("null argument");
    Ctx& c = ctx->c;
    // a pool's own worker opens the session of the job it runs (pool.hip: bfhip_pool_submit_air); the caller's threads stay refused, and
    // are refused first: the session that is open may be a worker's
    if (c.pool_refuses_this_thread()) throw HipError("bfhip_pcs_create: not supported on a pool's sub-context while jobs are outstanding on the pool");
    if (c.pcs_session_open) throw HipError("bfhip_pcs_create: a commitment-scheme session is open on this context (one session per context)");
    if (c.shard.count > 1) throw HipError("bfhip_pcs_create: not supported on a member of a shard group (bfhip_ctx_leave_group first)");
    auto* s = new bfhip_pcs(ctx);
    try {
        // like a proof: nothing of this context is in flight, its per-proof memory starts empty, no mailbox order
        drain(c);
        s->before = c.arena.mark();
        c.arena.reset();
        c.use_mailbox = false;
        c.stage_checkpoint();
        BF_HIP(hipMemsetAsync(c.d_counters, 0, 4 * 64 * sizeof(u32), c.stream));
    } catch (...) { delete s; throw; }
    c.pcs_session_open = true;
    *out = s;
    return 0;
    API_CATCH
}

int32_t bfhip_pcs_destroy(bfhip_pcs* pcs) {
    API_TRY
    if (!pcs) return 0;
    Ctx& c = pcs->ctx->c;
    c.bind();
    drain(c);
    c.arena.rewind(pcs->before);
    c.pcs_session_open = false;
    delete pcs;
    return 0;
    API_CATCH
}

int32_t bfhip_pcs_commit(bfhip_pcs* pcs, bfhip_channel* ch, const uint32_t* const* cols_h, const uint32_t* log_sizes_h, uint32_t n_cols, int32_t form, uint8_t root_out[32]) {
    API_TRY
    if (!pcs || !ch || !cols_h || !log_sizes_h || !root_out) throw HipError("null argument");
    Ctx& c = pcs->ctx->c;
    c.bind();
    if (pcs->proved) throw HipError("bfhip_pcs_commit: bfhip_pcs_prove_values ended this session's proving life");
    if (form != 0 && form != 1) throw HipError("bfhip_pcs_commit: form must be 0 (evaluations) or 1 (coefficients)");
    if (n_cols == 0) throw HipError("bfhip_pcs_commit: a tree has at least one column");
    if (n_cols > BFHIP_PCS_MAX_COLUMNS) throw HipError("bfhip_pcs_commit: " + std::to_string(n_cols) + " columns, more than BFHIP_PCS_MAX_COLUMNS (4096) in one tree");
    if (pcs->trees.size() >= BFHIP_PCS_MAX_TREES) throw HipError("bfhip_pcs_commit: more than BFHIP_PCS_MAX_TREES (64) trees");
    check_channel(pcs, ch, "bfhip_pcs_commit");
    const u32 blowup = pcs->pv.cfg.log_blowup, max_log_domain = c.tw_root_log + 1;
    DTree t;
    std::vector<DCol> src(n_cols);
    for (u32 k = 0; k < n_cols; k++) {
        if (!cols_h[k]) throw HipError("bfhip_pcs_commit: null column pointer");
        if (log_sizes_h[k] < LOG_N_LANES || log_sizes_h[k] + blowup > max_log_domain)
            throw HipError("bfhip_pcs_commit: column " + std::to_string(k) + " has log_size " + std::to_string(log_sizes_h[k]) + ", outside [4, max_log_domain - log_blowup_factor] = [4, " +
                           std::to_string(max_log_domain > blowup ? max_log_domain - blowup : 0) + "]");
        src[k].ptr = const_cast<u32*>(cols_h[k]); src[k].log_size = log_sizes_h[k];
    }
    try {
        c.use_mailbox = false;
        for (u32 k = 0; k < n_cols; k++) { DCol p; p.log_size = log_sizes_h[k]; p.ptr = c.alloc_u32(p.stored()); t.polys.push_back(p); }
        if (form == 1) for (u32 k = 0; k < n_cols; k++) BF_HIP(hipMemcpyAsync(t.polys[k].ptr, src[k].ptr, sizeof(u32) << log_sizes_h[k], hipMemcpyDeviceToDevice, c.stream));
        else pcs->pv.fft_cols(true, src, t.polys);
        pcs->pv.ch = ch->ch;
        pcs->pv.commit_tree(t);              // LDE, Merkle tree, root read back and mixed into pv.ch
    } catch (...) { drain(c); throw; }
    ch->ch = pcs->pv.ch;
    memcpy(root_out, t.mk.root.b, 32);
    pcs->trees.push_back(std::move(t));
    return 0;
    API_CATCH
}

int32_t bfhip_pcs_tree_columns(bfhip_pcs* pcs, uint32_t tree, const uint32_t** coeffs_d_out, const uint32_t** lde_d_out, uint32_t cap, uint32_t* n_cols) {
    API_TRY
    if (!pcs || !n_cols) throw HipError("null argument");
    if (tree >= pcs->trees.size()) throw HipError("bfhip_pcs_tree_columns: tree " + std::to_string(tree) + " was not committed");
    const DTree& t = pcs->trees[tree];
    *n_cols = (uint32_t)t.polys.size();
    if (!coeffs_d_out && !lde_d_out) return 0;
    if (cap < t.polys.size()) { bfhip_set_error("capacity"); return -2; }
    for (size_t k = 0; k < t.polys.size(); k++) { if (coeffs_d_out) coeffs_d_out[k] = t.polys[k].ptr; if (lde_d_out) lde_d_out[k] = t.evals[k].ptr; }
    return 0;
    API_CATCH
}

int32_t bfhip_pcs_prove_values(bfhip_pcs* pcs, bfhip_channel* ch, const uint32_t* points_h, uint32_t n_points, const uint32_t* n_samples_h,
                               const uint32_t* point_idx_h, uint32_t* sampled_out_h, char** proof_json, size_t* proof_len) {
    API_TRY
    if (!pcs || !ch || !n_samples_h || !proof_json || (!points_h && n_points)) throw HipError("null argument");
    Ctx& c = pcs->ctx->c;
    c.bind();
    if (pcs->proved) throw HipError("bfhip_pcs_prove_values: already called on this session (only bfhip_pcs_tree_columns and bfhip_pcs_destroy remain)");
    if (pcs->trees.empty()) throw HipError("bfhip_pcs_prove_values: nothing was committed");
    if (n_points > BFHIP_PCS_MAX_POINTS) throw HipError("bfhip_pcs_prove_values: " + std::to_string(n_points) + " points, more than BFHIP_PCS_MAX_POINTS (64)");
    check_channel(pcs, ch, "bfhip_pcs_prove_values");
    std::vector<PtQ> points(n_points);
    for (u32 p = 0; p < n_points; p++) points[p] = canonical_point(points_h + 8 * p, "bfhip_pcs_prove_values: point");
    std::vector<size_t> cols_per_tree;
    for (auto& t : pcs->trees) cols_per_tree.push_back(t.polys.size());
    const auto mask = sample_mask(cols_per_tree, n_points, n_samples_h, point_idx_h);
    HipProver& pv = pcs->pv;
    pv.check_config();                       // log_last_layer_degree_bound 0; Poseidon252 channel: pow_bits <= 12
    pcs->proved = true;
    StarkProof pf;
    try {
        c.use_mailbox = false;
        c.stage_checkpoint();
        pv.ch = ch->ch;
        const HipProver::SamplePlan plan = pv.sample_prepare(pcs->trees, mask);
        pv.sample(pcs->trees, mask, points, pf, plan);
        std::vector<Q31> flat;
        for (auto& t : pf.sampled_values) for (auto& col : t) for (auto& v : col) flat.push_back(v);
        pv.ch.mix_felts(flat.data(), flat.size());
        const Q31 q_coeff = pv.ch.draw_felt();
        std::vector<DSecure> quotients = pv.compute_quotients(pcs->trees, mask, points, &pf, q_coeff, nullptr).out;
        const HipProver::FriCommitted fri = pv.fri_commit(quotients, pf, {}, [] {});
#ifdef BFHIP_TEST_HOOKS
        pcs->fri_path = fri.path;
#endif
        pv.grind(pf);
        pv.decommit_queries(pcs->trees, quotients, fri, pf);
        if (sampled_out_h) for (size_t i = 0; i < flat.size(); i++) q31_words(flat[i], sampled_out_h + 4 * i);
    } catch (...) { drain(c); throw; }       // the arena must not be handed out again under running kernels
    ch->ch = pv.ch;
    std::string js;
    js.reserve(1 << 16);
    stark_proof_to_json(js, pf, pcs->conv.merkle_channel == 1);
    *proof_json = (char*)malloc(js.size() + 1);
    if (!*proof_json) throw HipError("out of host memory");
    memcpy(*proof_json, js.c_str(), js.size() + 1);
    if (proof_len) *proof_len = js.size();
    return 0;
    API_CATCH
}

#ifdef BFHIP_TEST_HOOKS
// libbfhip_testhooks.so only (Makefile); not declared in include/bfhip.h. Which launch folded and which hashed each line layer of the
// session's FRI commit phase: HipProver::FriCommitted::path (prover.h), one word per layer, the last layer included. *n = the number of
// layers (0 before bfhip_pcs_prove_values); out may be NULL to ask for it.
int32_t bfhip_test_pcs_fri_path(bfhip_pcs* pcs, uint32_t* out, uint32_t cap, uint32_t* n) {
    API_TRY
    if (!pcs || !n) throw HipError("null argument");
    *n = (uint32_t)pcs->fri_path.size();
    if (!out) return 0;
    if (cap < pcs->fri_path.size()) { bfhip_set_error("capacity"); return -2; }
    for (size_t k = 0; k < pcs->fri_path.size(); k++) out[k] = pcs->fri_path[k];
    return 0;
    API_CATCH
}
#endif

}  // extern "C"
