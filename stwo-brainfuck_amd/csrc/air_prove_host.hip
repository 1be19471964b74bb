// bfhip_air_verify (include/bfhip.h "Proving an AIR given as programs"): stwo's `verify` for an AIR given as a statement — the channel replay
// of bfhip_air_prove's steps 2 to 8 over bfhip_pcs_verifier_*, the claimed sums' total, the composition check at the drawn point
// (bfhip_air_compose_at_point) and verify_values. No GPU, no HIP call: this file also compiles with a plain C++ compiler, together with
// air_program_host.hip, logup_program_host.hip and pcs_host.hip, which is how tests/native/air_prove_host_sanitize.cpp puts it under the
// sanitizers. It stands beside air_program_host.hip rather than in it because it needs the channel and the verifier session of pcs_host.hip,
// which the sanitizer programs of air_program_host.hip do not link. The driver is air_prove.hip.
#include "api_guard.h"
#include "pcs_types.h"
#include "air_statement.h"
#include <cstdio>

using namespace bf;

PcsConfig pcs_config_from(const bfhip_pcs_config* p);

namespace {

struct Handles {
    bfhip_pcs_verifier* v = nullptr;
    ~Handles() { if (v) bfhip_pcs_verifier_destroy(v); }
};

void ok(int32_t rc, const std::string& me) { if (rc != 0) throw HipError(me + ": " + bfhip_last_error()); }

// "" = accepted, else the rejection name
std::string verify(const std::string& me, const bfhip_air_statement* st, const AirPlan& plan, const bfhip_conventions* conv, const bfhip_pcs_config* pcs, bfhip_channel* ch,
                   const char* proof_json, size_t proof_len) {
    const bool felt = conventions_from(conv).merkle_channel == 1;
    StarkProof pf;
    std::vector<u32> claimed(4 * (size_t)st->n_components, 0);
    try {
        const JVal root = json_document(proof_json, proof_len);
        if (root.kind != JVal::OBJ || root.obj.size() != 2) throw std::runtime_error("expected {claimed_sums, proof}");
        const std::vector<JVal>& sums = jv_list(root.get("claimed_sums"));
        if (sums.size() != plan.frac_comps.size()) return "InvalidStructure: claimed_sums";
        for (size_t i = 0; i < sums.size(); i++) q31_words(jv_qm31(sums[i]), claimed.data() + 4 * (size_t)plan.frac_comps[i]);
        pf = stark_proof_from_jval(root.get("proof"), felt);
    } catch (const std::exception& e) { return std::string("InvalidStructure: ") + e.what(); }
    const size_t nt = plan.tree_logs.size();
    if (pf.commitments.size() != nt || pf.sampled_values.size() != nt || pf.decommitments.size() != nt || pf.queried_values.size() != nt) return "InvalidStructure";
    std::vector<std::vector<std::vector<u32>>> sv(nt);
    for (size_t t = 0; t < nt; t++) {
        if (pf.sampled_values[t].size() != plan.samples[t].size()) return "InvalidStructure: sampled_values";
        sv[t].resize(plan.samples[t].size());
        for (size_t c = 0; c < plan.samples[t].size(); c++) {
            if (pf.sampled_values[t][c].size() != plan.samples[t][c].size()) return "InvalidStructure: sampled_values";
            sv[t][c].resize(4 * plan.samples[t][c].size());
            for (size_t s = 0; s < plan.samples[t][c].size(); s++) q31_words(pf.sampled_values[t][c][s], sv[t][c].data() + 4 * s);
        }
    }

    Handles h;
    ok(bfhip_pcs_verifier_create(conv, pcs, &h.v), me);
    for (u32 t = 0; t < st->n_trees; t++) {
        for (u32 i = 0; i < st->trees[t].n_mix; i++) ok(bfhip_channel_mix_u64(ch, st->trees[t].mix_u64_h[i]), me);
        ok(bfhip_pcs_verifier_commit(h.v, ch, pf.commitments[t].b, plan.tree_logs[t].data(), (u32)plan.tree_logs[t].size()), me);
    }
    std::vector<u32> lookup(8 * (size_t)st->n_relations + 8, 0);
    for (u32 r = 0; r < st->n_relations; r++) ok(bfhip_channel_draw_felts(ch, 2, lookup.data() + 8 * (size_t)r), me);
    if (plan.has_interaction) {
        Q31 total = q_zero();
        for (u32 k : plan.frac_comps) total = q_add(total, canonical_q31(claimed.data() + 4 * (size_t)k, me.c_str()));
        if (!q_is_zero(total)) return "InvalidLookup: Invalid LogUp sum";
        for (u32 k : plan.frac_comps) ok(bfhip_channel_mix_felts(ch, claimed.data() + 4 * (size_t)k, 1), me);
        const u32 t = plan.interaction_tree();
        ok(bfhip_pcs_verifier_commit(h.v, ch, pf.commitments[t].b, plan.tree_logs[t].data(), (u32)plan.tree_logs[t].size()), me);
    }
    u32 random_coeff[4], oods[8];
    ok(bfhip_channel_draw_felts(ch, 1, random_coeff), me);
    {
        const u32 t = plan.composition_tree();
        ok(bfhip_pcs_verifier_commit(h.v, ch, pf.commitments[t].b, plan.tree_logs[t].data(), 4), me);
    }
    ok(bfhip_channel_draw_point(ch, oods), me);
    const std::vector<u32> points = air_statement_points(plan, oods, me);

    const Q31 want = air_statement_composition_at_point(me, st, plan, sv, lookup.data(), claimed.data(), oods, random_coeff);
    Q31 coords[4];
    for (int w = 0; w < 4; w++) coords[w] = pf.sampled_values[plan.composition_tree()][w][0];
    if (!q_eq(air_from_partial_evals(coords), want)) return "OodsNotMatching";

    std::vector<u32> n_samples, point_idx;
    air_statement_flat_samples(plan, n_samples, point_idx);
    std::string js;
    js.reserve(proof_len);
    stark_proof_to_json(js, pf, felt);
    char reason[512] = {0};
    const int32_t rc = bfhip_pcs_verifier_verify_values(h.v, ch, points.data(), (u32)plan.points.size(), n_samples.data(), point_idx.empty() ? nullptr : point_idx.data(), js.data(),
                                                        js.size(), reason, sizeof reason);
    if (rc < 0) throw HipError(me + ": " + bfhip_last_error());
    return rc == 0 ? "" : reason[0] ? std::string(reason) : "rejected";
}

}  // namespace

extern "C" int32_t bfhip_air_statement_samples(const bfhip_air_statement* statement, const bfhip_pcs_config* pcs, uint32_t counts[4], uint32_t* tree_n_cols,
                                               uint32_t* point_log_sizes, int32_t* point_offsets, uint32_t* n_samples, uint32_t* point_idx) {
    API_TRY
    const std::string me = "bfhip_air_statement_samples";
    if (!statement || !counts) throw HipError(me + ": null argument");
    const AirPlan plan = air_statement_plan(me, statement, pcs_config_from(pcs).log_blowup, 30);
    std::vector<u32> ns, idx;
    air_statement_flat_samples(plan, ns, idx);
    counts[0] = (u32)plan.tree_logs.size(); counts[1] = (u32)plan.points.size(); counts[2] = (u32)ns.size(); counts[3] = (u32)idx.size();
    if (!tree_n_cols && !point_log_sizes && !point_offsets && !n_samples && !point_idx) return 0;
    if (!tree_n_cols || !point_log_sizes || !point_offsets || !n_samples || !point_idx) throw HipError(me + ": null argument");
    for (size_t t = 0; t < plan.tree_logs.size(); t++) tree_n_cols[t] = (u32)plan.tree_logs[t].size();
    for (size_t i = 0; i < plan.points.size(); i++) { point_log_sizes[i] = plan.points[i].log_size; point_offsets[i] = plan.points[i].off; }
    for (size_t i = 0; i < ns.size(); i++) n_samples[i] = ns[i];
    for (size_t i = 0; i < idx.size(); i++) point_idx[i] = idx[i];
    return 0;
    API_CATCH
}

extern "C" int32_t bfhip_air_verify(const bfhip_air_statement* statement, const bfhip_conventions* conv, const bfhip_pcs_config* pcs, bfhip_channel* ch,
                                    const char* proof_json, size_t proof_len, char* err, size_t err_cap) {
    API_TRY
    const std::string me = "bfhip_air_verify";
    if (!statement || !ch || !proof_json) throw HipError(me + ": null argument");
    const PcsConfig cfg = pcs_config_from(pcs);
    const AirPlan plan = air_statement_plan(me, statement, cfg.log_blowup, 30);
    const std::string reason = verify(me, statement, plan, conv, pcs, ch, proof_json, proof_len);
    if (err && err_cap) snprintf(err, err_cap, "%s", reason.c_str());
    return reason.empty() ? 0 : 1;
    API_CATCH
}
