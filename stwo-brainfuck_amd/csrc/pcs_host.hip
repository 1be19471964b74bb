// The host-only half of the commitment-scheme session (include/bfhip.h "Commitment-scheme session"): the channel object stwo passes to
// commit / prove_values / verify_values, the mask-point helper and the verifier session (CommitmentSchemeVerifier over host/verifier.h's
// verify_values). No GPU, no HIP call: this file also compiles with a plain C++ compiler, which is how the sanitizer run of
// tests/test_pcs_session_cpu.py builds it. The prover session is pcs.hip.
#include "api_guard.h"
#include "pcs_types.h"
#include <cstdio>

using namespace bf;

// include/bfhip.h `bfhip_pcs_config`: the accepted ranges (the same for a context and for the verifier).
PcsConfig pcs_config_from(const bfhip_pcs_config* p) {
    PcsConfig cfg;
    if (!p) return cfg;
    for (uint32_t r : p->reserved) if (r) throw HipError("bfhip_pcs_config: reserved fields must be zero");
    if (p->log_blowup_factor < 1 || p->log_blowup_factor > BFHIP_MAX_LOG_BLOWUP)
        throw HipError("bfhip_pcs_config: log_blowup_factor must be in [1, 16], got " + std::to_string(p->log_blowup_factor));
    if (p->n_queries < 1 || p->n_queries > BFHIP_MAX_QUERIES) throw HipError("bfhip_pcs_config: n_queries must be in [1, 256], got " + std::to_string(p->n_queries));
    if (p->pow_bits > BFHIP_MAX_POW_BITS) throw HipError("bfhip_pcs_config: pow_bits must be at most 32, got " + std::to_string(p->pow_bits));
    if (p->log_last_layer_degree_bound != 0)
        throw HipError("bfhip_pcs_config: only log_last_layer_degree_bound 0 is supported, got " + std::to_string(p->log_last_layer_degree_bound));
    cfg.pow_bits = p->pow_bits; cfg.log_blowup = p->log_blowup_factor; cfg.log_last_layer_degree_bound = 0; cfg.n_queries = p->n_queries;
    return cfg;
}

extern "C" {

// Blake2sChannel::default() / Poseidon252Channel::default() by conv->merkle_channel; mix_u64 follows conv->mix_u64
int32_t bfhip_channel_create(const bfhip_conventions* conv, bfhip_channel** out) {
    API_TRY
    if (!out) throw HipError("null argument");
    const Conventions cv = conventions_from(conv);
    *out = new bfhip_channel{Channel(cv), cv};
    return 0;
    API_CATCH
}
int32_t bfhip_channel_destroy(bfhip_channel* ch) { API_TRY delete ch; return 0; API_CATCH }
int32_t bfhip_channel_mix_root(bfhip_channel* ch, const uint8_t hash32[32]) {
    API_TRY
    if (!ch || !hash32) throw HipError("null argument");
    if (ch->conv.merkle_channel == 1 && !fe252::canonical_bytes_in_range(hash32)) throw HipError("bfhip_channel_mix_root: the root is not a canonical felt252");
    Hash32 h; memcpy(h.b, hash32, 32);
    ch->ch.mix_root(h);
    return 0;
    API_CATCH
}
int32_t bfhip_channel_mix_u64(bfhip_channel* ch, uint64_t v) { API_TRY if (!ch) throw HipError("null argument"); ch->ch.mix_u64(v); return 0; API_CATCH }
int32_t bfhip_channel_mix_felts(bfhip_channel* ch, const uint32_t* felts_h, size_t n) {
    API_TRY
    if (!ch || (!felts_h && n)) throw HipError("null argument");
    std::vector<Q31> f(n);
    for (size_t i = 0; i < n; i++) f[i] = canonical_q31(felts_h + 4 * i, "bfhip_channel_mix_felts");
    ch->ch.mix_felts(f.data(), n);
    return 0;
    API_CATCH
}
// Channel::draw_felts(n): secure felts taken from successive draws of 8 base felts, two per draw; what is left of the last draw is dropped
int32_t bfhip_channel_draw_felts(bfhip_channel* ch, size_t n, uint32_t* out_h) {
    API_TRY
    if (!ch || (!out_h && n)) throw HipError("null argument");
    for (size_t i = 0; i < n; i += 2) {
        u32 f[8];
        ch->ch.draw_base_felts(f);
        memcpy(out_h + 4 * i, f, (n - i >= 2 ? 8 : 4) * sizeof(u32));
    }
    return 0;
    API_CATCH
}
// CirclePoint::get_random_point: t = draw_felt(), ((1 - t^2) / (1 + t^2), 2 t / (1 + t^2))
int32_t bfhip_channel_draw_point(bfhip_channel* ch, uint32_t point_out[8]) {
    API_TRY
    if (!ch || !point_out) throw HipError("null argument");
    const Q31 t = ch->ch.draw_felt(), t2 = q_mul(t, t), d = q_inv(q_addm(t2, 1));
    q31_words(q_mul(q_sub(q_one(), t2), d), point_out);
    q31_words(q_mul(q_add(t, t), d), point_out + 4);
    return 0;
    API_CATCH
}
int32_t bfhip_channel_state(bfhip_channel* ch, uint8_t digest[32], uint32_t* n_sent) {
    API_TRY
    if (!ch) throw HipError("null argument");
    if (digest) memcpy(digest, ch->ch.digest.b, 32);
    if (n_sent) *n_sent = ch->ch.n_sent;
    return 0;
    API_CATCH
}
int32_t bfhip_channel_trailing_zeros(bfhip_channel* ch, uint32_t* out) { API_TRY if (!ch || !out) throw HipError("null argument"); *out = ch->ch.trailing_zeros(); return 0; API_CATCH }

// out = p + offset * CanonicCoset(log_size).step(): the mask point of a column of 2^log_size rows at row offset `offset`
int32_t bfhip_circle_point_offset(const uint32_t p[8], uint32_t log_size, int32_t offset, uint32_t out[8]) {
    API_TRY
    if (!p || !out) throw HipError("null argument");
    if (log_size < 1 || log_size > 30) throw HipError("bfhip_circle_point_offset: log_size must be in [1, 30]");
    const PtQ at = canonical_point(p, "bfhip_circle_point_offset");
    // the step generates a group of order 2^log_size: the offset counts modulo that order (two's complement does the negative ones)
    const u32 k = (u32)offset & ((1u << log_size) - 1u);
    const PtQ r = pq_add(at, to_q(index_to_point(k * subgroup_gen(log_size))));
    q31_words(r.x, out); q31_words(r.y, out + 4);
    return 0;
    API_CATCH
}

// Components::eval_composition_polynomial_at_point of the snapshot's 13 components: what stwo's verify() compares with the composition
// polynomial's sampled value before it calls verify_values — the one AIR-dependent step of a verifier assembled from bfhip_pcs_verifier_*
int32_t bfhip_brainfuck_composition_at_point(const uint32_t log_sizes_h[13], const uint32_t* claimed_sums_h, uint32_t log_max_rows, const uint32_t lookup_h[24],
                                             const uint32_t point_h[8], const uint32_t n_cols_h[3], const uint32_t* n_samples_h, const uint32_t* sampled_h,
                                             const uint32_t random_coeff_h[4], const bfhip_conventions* conv, uint32_t out_h[4]) {
    API_TRY
    if (!log_sizes_h || !claimed_sums_h || !lookup_h || !point_h || !n_cols_h || !n_samples_h || !sampled_h || !random_coeff_h || !out_h) throw HipError("null argument");
    const Conventions cv = conventions_from(conv);
    const char* me = "bfhip_brainfuck_composition_at_point";
    Q31 claimed[N_COMPONENTS];
    size_t want_cols[3] = {0, 0, 0};
    for (int k = 0; k < N_COMPONENTS; k++) {
        if (log_sizes_h[k] < LOG_N_LANES || log_sizes_h[k] > log_max_rows || log_max_rows > 29) throw HipError(std::string(me) + ": a log_size outside [4, log_max_rows]");
        claimed[k] = canonical_q31(claimed_sums_h + 4 * k, me);
        want_cols[1] += n_main_cols(k); want_cols[2] += 4 * n_logup_cols(k);
    }
    want_cols[0] = log_max_rows - LOG_N_LANES + 1;
    std::vector<std::vector<std::vector<Q31>>> sv(3);
    size_t ci = 0, si = 0;
    for (int t = 0; t < 3; t++) {
        if (n_cols_h[t] != want_cols[t]) throw HipError(std::string(me) + ": tree " + std::to_string(t) + " has " + std::to_string(want_cols[t]) + " columns");
        sv[t].resize(n_cols_h[t]);
        for (u32 c = 0; c < n_cols_h[t]; c++, ci++) for (u32 s = 0; s < n_samples_h[ci]; s++, si++) sv[t][c].push_back(canonical_q31(sampled_h + 4 * si, me));
    }
    Lookups el;
    Q31 lk[6];
    for (int i = 0; i < 6; i++) lk[i] = canonical_q31(lookup_h + 4 * i, me);
    el.memory = make_lookup(lk[0], lk[1]); el.instruction = make_lookup(lk[2], lk[3]); el.processor = make_lookup(lk[4], lk[5]);
    Q31 r;
    // a column of the mask without its sampled value: std::out_of_range from the evaluator's .at()
    try { r = eval_composition_at_point(log_sizes_h, claimed, log_max_rows, el, canonical_point(point_h, me), sv, canonical_q31(random_coeff_h, me), cv); }
    catch (const std::out_of_range&) { throw HipError(std::string(me) + ": a sampled value the AIR reads is missing"); }
    q31_words(r, out_h);
    return 0;
    API_CATCH
}

// ---- CommitmentSchemeVerifier ----------------------------------------------------------------------------------------------------------
int32_t bfhip_pcs_verifier_create(const bfhip_conventions* conv, const bfhip_pcs_config* pcs, bfhip_pcs_verifier** out) {
    API_TRY
    if (!out) throw HipError("null argument");
    auto* v = new bfhip_pcs_verifier();
    try { v->conv = conventions_from(conv); v->cfg = pcs_config_from(pcs); } catch (...) { delete v; throw; }
    *out = v;
    return 0;
    API_CATCH
}
int32_t bfhip_pcs_verifier_destroy(bfhip_pcs_verifier* v) { API_TRY delete v; return 0; API_CATCH }
int32_t bfhip_pcs_verifier_commit(bfhip_pcs_verifier* v, bfhip_channel* ch, const uint8_t root[32], const uint32_t* log_sizes_h, uint32_t n_cols) {
    API_TRY
    if (!v || !ch || !root || !log_sizes_h) throw HipError("null argument");
    if (n_cols == 0) throw HipError("bfhip_pcs_verifier_commit: a tree has at least one column");
    if (v->roots.size() >= BFHIP_PCS_MAX_TREES) throw HipError("bfhip_pcs_verifier_commit: more than BFHIP_PCS_MAX_TREES (64) trees");
    if (ch->conv.merkle_channel != v->conv.merkle_channel) throw HipError("bfhip_pcs_verifier_commit: the channel and the verifier were created under different merkle_channel values");
    if (v->conv.merkle_channel == 1 && !fe252::canonical_bytes_in_range(root)) throw HipError("bfhip_pcs_verifier_commit: the root is not a canonical felt252");
    std::vector<u32> logs(n_cols);
    for (u32 k = 0; k < n_cols; k++) {
        // CanonicCoset(n) lives in the subgroup of order 2^(n+1) of the M31 circle (order 2^31): every LDE domain has n <= 30
        if (log_sizes_h[k] < 1 || log_sizes_h[k] + v->cfg.log_blowup > 30)
            throw HipError("bfhip_pcs_verifier_commit: column " + std::to_string(k) + " has log_size " + std::to_string(log_sizes_h[k]) + ", outside [1, 30 - log_blowup_factor]");
        logs[k] = log_sizes_h[k] + v->cfg.log_blowup;
    }
    Hash32 h; memcpy(h.b, root, 32);
    v->roots.push_back(h); v->col_logs.push_back(std::move(logs));
    ch->ch.mix_root(h);
    return 0;
    API_CATCH
}
int32_t bfhip_pcs_verifier_verify_values(bfhip_pcs_verifier* v, bfhip_channel* ch, const uint32_t* points_h, uint32_t n_points, const uint32_t* n_samples_h,
                                         const uint32_t* point_idx_h, const char* proof_json, size_t proof_len, char* err, size_t err_cap) {
    API_TRY
    if (!v || !ch || !n_samples_h || !proof_json || (!points_h && n_points)) throw HipError("null argument");
    if (v->roots.empty()) throw HipError("bfhip_pcs_verifier_verify_values: nothing was committed");
    std::vector<PtQ> points(n_points);
    for (u32 p = 0; p < n_points; p++) points[p] = canonical_point(points_h + 8 * p, "bfhip_pcs_verifier_verify_values: point");
    std::vector<size_t> cols_per_tree;
    for (auto& t : v->col_logs) cols_per_tree.push_back(t.size());
    const auto mask = sample_mask(cols_per_tree, n_points, n_samples_h, point_idx_h);
    std::string reason;
    try {
        const size_t nt = v->roots.size();
        const StarkProof pf = stark_proof_from_json(proof_json, proof_len, v->conv.merkle_channel == 1);
        std::vector<std::vector<std::vector<PtQ>>> sp(nt);
        for (size_t t = 0; t < nt; t++) { sp[t].resize(mask[t].size()); for (size_t c = 0; c < mask[t].size(); c++) for (u32 i : mask[t][c]) sp[t][c].push_back(points[i]); }
        auto structure = [&]() -> std::string {
            if (pf.commitments.size() != nt || pf.sampled_values.size() != nt || pf.decommitments.size() != nt || pf.queried_values.size() != nt) return "InvalidStructure";
            for (size_t t = 0; t < nt; t++) {
                if (pf.sampled_values[t].size() != sp[t].size()) return "InvalidStructure: sampled_values";
                for (size_t c = 0; c < sp[t].size(); c++) if (pf.sampled_values[t][c].size() != sp[t][c].size()) return "InvalidStructure: sampled_values";
            }
            for (size_t t = 0; t < nt; t++) if (!(pf.commitments[t] == v->roots[t])) return "InvalidStructure: commitment " + std::to_string(t) + " is not the committed root";
            return "";
        };
        reason = structure();
        if (reason.empty()) reason = verify_values(ch->ch, v->col_logs, sp, pf, v->cfg, v->conv);
    } catch (const std::exception& e) { reason = std::string("InvalidStructure: ") + e.what(); }
    if (err && err_cap) snprintf(err, err_cap, "%s", reason.c_str());
    return reason.empty() ? 0 : 1;
    API_CATCH
}

}  // extern "C"
