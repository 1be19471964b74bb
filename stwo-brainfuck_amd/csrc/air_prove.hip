// bfhip_air_prove (include/bfhip.h "Proving an AIR given as programs"): stwo's `prover::prove` for an AIR given as a statement. A driver and
// nothing else: it orders the calls of the library's own entry points — bfhip_pcs_* (the session), bfhip_channel_*,
// bfhip_logup_program_generate_batch, bfhip_air_check, bfhip_evaluate, bfhip_air_compose, bfhip_air_compose_at_point — and owns one device
// buffer. No kernel is launched from this file. The statement's rules and the sample description are air_statement.h, shared with the
// verifier (air_prove_host.hip).
#include "api_guard.h"
#include "pcs_types.h"
#include "air_statement.h"
#include <map>
#include <tuple>

using namespace bf;

namespace {

// The session, closed on every path. Declared behind the driver's buffer (a DeviceScratch), so closed before the buffer goes:
// bfhip_pcs_destroy waits for every stream of the context, and then no launch reads the buffer any more
struct Session {
    bfhip_pcs* pcs = nullptr;
    ~Session() { if (pcs) (void)bfhip_pcs_destroy(pcs); }
};

}  // namespace

extern "C" int32_t bfhip_air_prove(bfhip_ctx* ctx, const bfhip_air_statement* st, const uint32_t* const* const* tree_cols_h, bfhip_air_kernel* const* kernels,
                                   bfhip_channel* ch, uint32_t flags, char** proof_json, size_t* proof_len) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    const std::string me = "bfhip_air_prove";
    auto ok = [&](int32_t rc) { if (rc != 0) throw HipError(me + ": " + bfhip_last_error()); };
    if (!st || !tree_cols_h || !ch || !proof_json) throw HipError(me + ": null argument");
    if (flags & ~(uint32_t)BFHIP_AIR_PROVE_CHECK) throw HipError(me + ": unknown flags " + std::to_string(flags));
    // step 1's refusal on a pool's sub-context, in its words and before this context's own state is read: a worker may be inside a job
    if (c.pool_refuses_this_thread()) throw HipError(me + ": bfhip_pcs_create: not supported on a pool's sub-context while jobs are outstanding on the pool");
    if (c.pcs_session_open) throw HipError(me + ": a commitment-scheme session is open on this context (bfhip_pcs_destroy first)");
    if (c.shard.count > 1) throw HipError(me + ": a context in a shard group is not supported (bfhip_ctx_leave_group first)");
    const u32 blowup = c.pcs.log_blowup, max_log_domain = c.tw_root_log + 1;

    // ---- everything that can be refused, before the session opens and before anything is enqueued ----------------------------------------
    const AirPlan plan = air_statement_plan(me, st, blowup, max_log_domain);
    const u32 n = st->n_components, it = plan.interaction_tree();
    for (u32 t = 0; t < st->n_trees; t++) {
        if (!tree_cols_h[t]) throw HipError(me + ": tree " + std::to_string(t) + ": null argument");
        for (u32 col = 0; col < st->trees[t].n_cols; col++)
            if (!tree_cols_h[t][col]) throw HipError(me + ": tree " + std::to_string(t) + ": null column pointer");
    }
    for (u32 k = 0; k < n; k++) {
        const bfhip_air_statement_component& p = st->components[k];
        const std::string mk = me + ": component " + std::to_string(k);
        if (flags & BFHIP_AIR_PROVE_CHECK)
            for (u32 col = 0; col < p.program->n_cols; col++)
                if (p.col_trees_h[col] != BFHIP_AIR_TREE_INTERACTION && st->trees[p.col_trees_h[col]].form != 0)
                    throw HipError(mk + ": column " + std::to_string(col) + ": BFHIP_AIR_PROVE_CHECK needs trace-domain evaluations, tree " + std::to_string(p.col_trees_h[col]) +
                                   " is committed as coefficients (form 1)");
        if (kernels && kernels[k]) {
            const bfhip_air& kp = air_kernel_program(ctx, kernels[k], mk);
            if (kp.code != p.program->code || kp.n_cols != p.program->n_cols || kp.n_params != p.program->n_params) throw HipError(mk + ": the kernel was compiled from another program");
        }
    }

    // ---- the driver's one buffer: interaction columns, composition columns, constraint-domain scratch -------------------------------------
    // a column of a tree on the constraint domain of log_expand: the session's LDE where log_expand is the blowup, else evaluated into scratch
    std::map<std::tuple<u32, u32, u32>, u32*> expanded;      // (tree, column, log_expand) -> scratch
    size_t words = 0;
    std::vector<size_t> inter_at;
    if (plan.has_interaction) for (u32 l : plan.tree_logs[it]) { inter_at.push_back(words); words += size_t(1) << l; }
    const size_t comp_at = words;
    words += size_t(4) << plan.composition_log;
    auto bound = [&](u32 k, u32 col) {
        const bfhip_air_statement_component& p = st->components[k];
        const bool inter = p.col_trees_h[col] == BFHIP_AIR_TREE_INTERACTION;
        return std::make_pair(inter ? it : p.col_trees_h[col], inter ? plan.inter_first[k] + p.col_columns_h[col] : p.col_columns_h[col]);
    };
    std::vector<std::pair<std::tuple<u32, u32, u32>, size_t>> scratch_at;
    for (u32 k = 0; k < n; k++) {
        const bfhip_air_statement_component& p = st->components[k];
        if (p.log_expand == blowup) continue;
        for (u32 col = 0; col < p.program->n_cols; col++) {
            const auto b = bound(k, col);
            const auto key = std::make_tuple(b.first, b.second, p.log_expand);
            if (expanded.emplace(key, nullptr).second) { scratch_at.emplace_back(key, words); words += size_t(1) << (p.log_size + p.log_expand); }
        }
    }

    DeviceScratch scratch(c);
    u32* buf = nullptr;
    if (scratch.try_alloc(&buf, words * sizeof(u32)) != hipSuccess)
        throw HipError(me + ": cannot allocate " + std::to_string(words * sizeof(u32)) + " bytes for the interaction, composition and constraint-domain columns");
    Session own;
    for (auto& s : scratch_at) expanded[s.first] = buf + s.second;
    u32* comp_cols[4];
    for (int w = 0; w < 4; w++) comp_cols[w] = buf + comp_at + (size_t(w) << plan.composition_log);

    // ---- 1, 2: the session; the caller's trees ---------------------------------------------------------------------------------------------
    ok(bfhip_pcs_create(ctx, &own.pcs));
    uint8_t root[32];
    for (u32 t = 0; t < st->n_trees; t++) {
        const bfhip_air_statement_tree& tr = st->trees[t];
        for (u32 i = 0; i < tr.n_mix; i++) ok(bfhip_channel_mix_u64(ch, tr.mix_u64_h[i]));
        ok(bfhip_pcs_commit(own.pcs, ch, tree_cols_h[t], tr.log_sizes_h, tr.n_cols, (int32_t)tr.form, root));
    }

    // ---- 3: the lookup elements ------------------------------------------------------------------------------------------------------------
    std::vector<u32> lookup(8 * (size_t)st->n_relations + 8, 0);
    for (u32 r = 0; r < st->n_relations; r++) ok(bfhip_channel_draw_felts(ch, 2, lookup.data() + 8 * (size_t)r));

    // ---- 4: the interaction trace of every component with a fraction program, in one call -------------------------------------------------
    std::vector<u32> claimed(4 * (size_t)n, 0);
    std::vector<u32*> inter_cols;
    if (plan.has_interaction) {
        for (size_t at : inter_at) inter_cols.push_back(buf + at);
        const size_t nf = plan.frac_comps.size();
        std::vector<bfhip_logup_component> lc(nf);
        std::vector<std::vector<const u32*>> in(nf);
        std::vector<std::vector<u32>> pars(nf);
        std::vector<u32> sums(4 * nf);
        for (size_t i = 0; i < nf; i++) {
            const u32 k = plan.frac_comps[i];
            const bfhip_air_statement_component& p = st->components[k];
            for (u32 col = 0; col < p.fractions->n_cols; col++) in[i].push_back(tree_cols_h[p.frac_trees_h[col]][p.frac_columns_h[col]]);
            std::vector<u32> all;
            air_statement_params(p, lookup.data(), nullptr, all);      // the validator admits no CLAIMED_SUM among these
            pars[i].assign(all.begin(), all.begin() + 4 * (size_t)p.fractions->n_params);
            lc[i] = bfhip_logup_component{p.fractions, p.log_size, p.fractions->n_params, in[i].empty() ? nullptr : in[i].data(), nullptr, pars[i].empty() ? nullptr : pars[i].data(),
                                          inter_cols.data() + plan.inter_first[k], 0};
        }
        ok(bfhip_logup_program_generate_batch(ctx, lc.data(), (u32)nf, sums.data(), nullptr));
        for (size_t i = 0; i < nf; i++) {
            memcpy(claimed.data() + 4 * (size_t)plan.frac_comps[i], sums.data() + 4 * i, 16);
            ok(bfhip_channel_mix_felts(ch, sums.data() + 4 * i, 1));
        }
        ok(bfhip_pcs_commit(own.pcs, ch, inter_cols.data(), plan.tree_logs[it].data(), (u32)inter_cols.size(), 0, root));
    }
    std::vector<std::vector<u32>> params(n);
    for (u32 k = 0; k < n; k++) air_statement_params(st->components[k], lookup.data(), claimed.data() + 4 * (size_t)k, params[k]);

    if (flags & BFHIP_AIR_PROVE_CHECK) {
        for (u32 k = 0; k < n; k++) {
            const bfhip_air_statement_component& p = st->components[k];
            std::vector<const u32*> cols;
            for (u32 col = 0; col < p.program->n_cols; col++) {
                const auto b = bound(k, col);
                cols.push_back(b.first == it ? inter_cols[b.second] : tree_cols_h[b.first][b.second]);
            }
            bfhip_air_check_report rep;
            ok(bfhip_air_check(ctx, p.program, p.log_size, cols.empty() ? nullptr : cols.data(), nullptr, params[k].empty() ? nullptr : params[k].data(), p.n_params, &rep));
            if (rep.n_bad_cells == 0) continue;
            size_t need = 0;
            (void)bfhip_format_air_check(&rep, nullptr, 0, &need);
            std::string text(need + 1, '\0');
            ok(bfhip_format_air_check(&rep, &text[0], text.size(), nullptr));
            text.resize(strlen(text.c_str()));
            const size_t first = text.find('\n');      // the headline, then one line per failing constraint
            const size_t end = first == std::string::npos ? std::string::npos : text.find('\n', first + 1);
            throw HipError(me + ": component " + std::to_string(k) + ": " + (first == std::string::npos ? text : text.substr(first + 1, end == std::string::npos ? end : end - first - 1)));
        }
    }

    // ---- 5, 6: the composition polynomial --------------------------------------------------------------------------------------------------
    u32 random_coeff[4];
    ok(bfhip_channel_draw_felts(ch, 1, random_coeff));
    const u32 n_session_trees = st->n_trees + (plan.has_interaction ? 1u : 0u);
    std::vector<std::vector<const u32*>> coeffs_d(n_session_trees), lde_d(n_session_trees);
    for (u32 t = 0; t < n_session_trees; t++) {
        u32 got = 0;
        coeffs_d[t].resize(plan.tree_logs[t].size()); lde_d[t].resize(plan.tree_logs[t].size());
        ok(bfhip_pcs_tree_columns(own.pcs, t, coeffs_d[t].data(), lde_d[t].data(), (u32)plan.tree_logs[t].size(), &got));
    }
    {   // one bfhip_evaluate per (log_size, log_expand) that is not the session's own LDE
        std::map<std::pair<u32, u32>, std::pair<std::vector<u32*>, std::vector<u32*>>> groups;
        for (auto& e : expanded) {
            const u32 t = std::get<0>(e.first), col = std::get<1>(e.first), le = std::get<2>(e.first);
            auto& g = groups[std::make_pair(plan.tree_logs[t][col], le)];
            g.first.push_back(const_cast<u32*>(coeffs_d[t][col])); g.second.push_back(e.second);
        }
        for (auto& g : groups) ok(bfhip_evaluate(ctx, g.second.first.data(), g.second.second.data(), (u32)g.second.first.size(), g.first.first, g.first.first + g.first.second, 0));
    }
    std::vector<bfhip_air_component> ac(n);
    std::vector<std::vector<const u32*>> comp_in(n);
    for (u32 k = 0; k < n; k++) {
        const bfhip_air_statement_component& p = st->components[k];
        for (u32 col = 0; col < p.program->n_cols; col++) {
            const auto b = bound(k, col);
            comp_in[k].push_back(p.log_expand == blowup ? lde_d[b.first][b.second] : expanded.at(std::make_tuple(b.first, b.second, p.log_expand)));
        }
        ac[k] = bfhip_air_component{p.program, kernels ? kernels[k] : nullptr, p.log_size, p.log_expand, comp_in[k].empty() ? nullptr : comp_in[k].data(), nullptr,
                                    params[k].empty() ? nullptr : params[k].data(), p.n_params, 0};
    }
    ok(bfhip_air_compose(ctx, ac.data(), n, random_coeff, plan.composition_log, comp_cols));

    // ---- 7: the composition tree -----------------------------------------------------------------------------------------------------------
    ok(bfhip_pcs_commit(own.pcs, ch, comp_cols, plan.tree_logs[plan.composition_tree()].data(), 4, 1, root));

    // ---- 8, 9: the mask and the opening ----------------------------------------------------------------------------------------------------
    u32 oods[8];
    ok(bfhip_channel_draw_point(ch, oods));
    const std::vector<u32> points = air_statement_points(plan, oods, me);
    std::vector<u32> n_samples, point_idx;
    air_statement_flat_samples(plan, n_samples, point_idx);
    std::vector<u32> sampled(4 * plan.n_samples());
    char* inner = nullptr;
    size_t inner_len = 0;
    ok(bfhip_pcs_prove_values(own.pcs, ch, points.data(), (u32)plan.points.size(), n_samples.data(), point_idx.data(), sampled.data(), &inner, &inner_len));
    struct Host { char* p; ~Host() { bfhip_free_host(p); } } inner_owner{inner};

    // ---- 10: the sanity check of prover::prove ---------------------------------------------------------------------------------------------
    std::vector<std::vector<std::vector<u32>>> sv(plan.samples.size());
    {
        size_t at = 0;
        for (size_t t = 0; t < plan.samples.size(); t++) {
            sv[t].resize(plan.samples[t].size());
            for (size_t col = 0; col < plan.samples[t].size(); col++) {
                const size_t m = 4 * plan.samples[t][col].size();
                sv[t][col].assign(sampled.begin() + at, sampled.begin() + at + m);
                at += m;
            }
        }
    }
    const Q31 want = air_statement_composition_at_point(me, st, plan, sv, lookup.data(), claimed.data(), oods, random_coeff);
    Q31 coords[4];
    for (int w = 0; w < 4; w++) coords[w] = canonical_q31(sv[plan.composition_tree()][w].data(), me.c_str());
    if (!q_eq(air_from_partial_evals(coords), want)) throw HipError(me + ": ConstraintsNotSatisfied");

    // ---- 11: {"claimed_sums":[...],"proof":<what bfhip_pcs_prove_values returned>} -------------------------------------------------------
    std::string js = "{\"claimed_sums\":[";
    for (size_t i = 0; i < plan.frac_comps.size(); i++) {
        if (i) js += ',';
        json::qm31(js, canonical_q31(claimed.data() + 4 * (size_t)plan.frac_comps[i], me.c_str()));
    }
    js += "],\"proof\":";
    js.append(inner, inner_len);
    js += '}';
    *proof_json = (char*)malloc(js.size() + 1);
    if (!*proof_json) throw HipError(me + ": out of host memory");
    memcpy(*proof_json, js.c_str(), js.size() + 1);
    if (proof_len) *proof_len = js.size();
    return 0;
    API_CATCH
}
