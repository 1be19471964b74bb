// The statement of bfhip_air_prove / bfhip_air_verify (include/bfhip.h "Proving an AIR given as programs"): the one validator both sides run
// before anything else, and what they derive from the statement alone — the trees in commit order, the mask points, every column's samples
// and, per component, where each mask value is found among the sampled values. Host only, plain C++: tests/native/air_prove_host_sanitize.cpp
// puts it under the sanitizers. air_prove.hip (the driver) and air_prove_host.hip (the verifier) include it; nothing here knows a channel.
#pragma once
#include "logup_program.h"
#include "../../include/bfhip.h"
#include <stdexcept>
#include <string>
#include <vector>

namespace bf {

struct AirPlan {
    struct Point { u32 log_size; int32_t off; };          // point 0 is the out-of-domain point itself: {0, 0}
    struct Ref { u32 tree, col, pos; };                   // a mask value: sampled_values[tree][col][pos]
    u32 n_caller_trees = 0;
    bool has_interaction = false;
    u32 composition_log = 0;
    std::vector<std::vector<u32>> tree_logs;              // trace-domain log sizes of every tree in commit order: caller trees, interaction, composition
    std::vector<Point> points;
    std::vector<std::vector<std::vector<u32>>> samples;   // [tree][column] = point indices, in first-use order
    std::vector<std::vector<Ref>> mask_refs;              // [component][mask entry]
    std::vector<u32> frac_comps;                          // the components with a fraction program, in list order
    std::vector<u32> inter_first;                         // [component]: its first column in the interaction tree (components without fractions: 0)
    u32 interaction_tree() const { return n_caller_trees; }
    u32 composition_tree() const { return n_caller_trees + (has_interaction ? 1u : 0u); }
    size_t n_samples() const { size_t n = 0; for (auto& t : samples) for (auto& c : t) n += c.size(); return n; }
};

// Every rule that the statement alone decides, in the caller's name `me`; then the plan. log_blowup and max_log_domain are the context's (the
// verifier's: its PcsConfig and 30, the largest canonic coset of the M31 circle).
inline AirPlan air_statement_plan(const std::string& me, const bfhip_air_statement* st, u32 log_blowup, u32 max_log_domain) {
    auto refuse = [&](const std::string& rule) { throw std::runtime_error(me + ": " + rule); };
    if (!st) refuse("null statement");
    if (st->reserved != 0) refuse("reserved must be 0");
    if (st->n_trees < 1 || st->n_trees > BFHIP_AIR_STATEMENT_MAX_TREES) refuse("1 to BFHIP_AIR_STATEMENT_MAX_TREES (8) trees, got " + std::to_string(st->n_trees));
    if (st->n_relations > BFHIP_AIR_STATEMENT_MAX_RELATIONS) refuse("at most BFHIP_AIR_STATEMENT_MAX_RELATIONS (16) relations, got " + std::to_string(st->n_relations));
    if (st->n_components < 1 || st->n_components > BFHIP_AIR_COMPOSE_MAX_COMPONENTS)
        refuse("1 to BFHIP_AIR_COMPOSE_MAX_COMPONENTS (64) components, got " + std::to_string(st->n_components));
    if (!st->trees || !st->components) refuse("null argument");

    AirPlan plan;
    plan.n_caller_trees = st->n_trees;
    for (u32 t = 0; t < st->n_trees; t++) {
        const bfhip_air_statement_tree& tr = st->trees[t];
        const std::string mt = "tree " + std::to_string(t);
        if (tr.reserved != 0) refuse(mt + ": reserved must be 0");
        if (tr.form > 1) refuse(mt + ": form must be 0 (evaluations) or 1 (coefficients)");
        if (tr.n_cols < 1 || tr.n_cols > BFHIP_PCS_MAX_COLUMNS) refuse(mt + ": 1 to BFHIP_PCS_MAX_COLUMNS (4096) columns, got " + std::to_string(tr.n_cols));
        if (!tr.log_sizes_h || (!tr.mix_u64_h && tr.n_mix)) refuse(mt + ": null argument");
        for (u32 c = 0; c < tr.n_cols; c++)
            if (tr.log_sizes_h[c] < 4 || tr.log_sizes_h[c] + log_blowup > max_log_domain)
                refuse(mt + " column " + std::to_string(c) + ": log_size " + std::to_string(tr.log_sizes_h[c]) + " outside [4, max_log_domain - log_blowup_factor] = [4, " +
                       std::to_string(max_log_domain > log_blowup ? max_log_domain - log_blowup : 0) + "]");
        plan.tree_logs.emplace_back(tr.log_sizes_h, tr.log_sizes_h + tr.n_cols);
    }

    // ---- every component on its own ------------------------------------------------------------------------------------------------------
    std::vector<u32> inter_logs;
    plan.inter_first.assign(st->n_components, 0);
    for (u32 k = 0; k < st->n_components; k++) {
        const bfhip_air_statement_component& p = st->components[k];
        auto no = [&](const std::string& rule) { refuse("component " + std::to_string(k) + ": " + rule); };
        if (p.reserved != 0) no("reserved must be 0");
        if (!p.program) no("null program");
        const bfhip_air* air = p.program;
        const bfhip_logup* lp = p.fractions;
        if ((air->n_cols && (!p.col_trees_h || !p.col_columns_h)) || (lp && lp->n_cols && (!p.frac_trees_h || !p.frac_columns_h)) || (p.n_params && !p.params_h)) no("null argument");
        if (p.log_expand < 1 || p.log_expand > 3) no("log_expand must be 1, 2 or 3, got " + std::to_string(p.log_expand));
        const u32 widest = log_blowup > p.log_expand ? log_blowup : p.log_expand;
        if (p.log_size < 4 || p.log_size + widest > max_log_domain)
            no("log_size " + std::to_string(p.log_size) + " outside [4, max_log_domain - max(log_blowup_factor, log_expand)] = [4, " +
               std::to_string(max_log_domain > widest ? max_log_domain - widest : 0) + "]");
        if (p.n_params != air->n_params) no("the constraint program takes " + std::to_string(air->n_params) + " parameters, got " + std::to_string(p.n_params) + " rules");
        if (lp && lp->n_params > p.n_params) no("the fraction program takes " + std::to_string(lp->n_params) + " parameters, the table has " + std::to_string(p.n_params) + " rules");
        for (u32 i = 0; i < p.n_params; i++) {
            const bfhip_air_param_rule& r = p.params_h[i];
            const std::string mr = "parameter " + std::to_string(i) + ": ";
            if (r.reserved != 0) no(mr + "reserved must be 0");
            switch (r.kind) {
                case BFHIP_AIR_PARAM_CONST:
                    for (int w = 0; w < 4; w++) if (r.value[w] >= P31) no(mr + "a word is not a canonical M31");
                    break;
                case BFHIP_AIR_PARAM_LOOKUP_ALPHA_POW:
                    if (r.power > BFHIP_AIR_STATEMENT_MAX_POWER) no(mr + "power " + std::to_string(r.power) + " above BFHIP_AIR_STATEMENT_MAX_POWER (63)");
                    // fall through
                case BFHIP_AIR_PARAM_LOOKUP_Z:
                    if (r.relation >= st->n_relations) no(mr + "relation " + std::to_string(r.relation) + " out of range (n_relations " + std::to_string(st->n_relations) + ")");
                    break;
                case BFHIP_AIR_PARAM_CLAIMED_SUM:
                    if (!lp) no(mr + "CLAIMED_SUM without a fraction program");
                    if (i < lp->n_params) no(mr + "CLAIMED_SUM among the fraction program's parameters");
                    break;
                default: no(mr + "unknown kind " + std::to_string(r.kind));
            }
        }
        const u32 n_inter = lp ? 4 * lp->n_logup_cols : 0;
        for (u32 c = 0; c < air->n_cols; c++) {
            const u32 t = p.col_trees_h[c], col = p.col_columns_h[c];
            const std::string mc = "column " + std::to_string(c) + ": ";
            if (t == BFHIP_AIR_TREE_INTERACTION) {
                if (!lp) no(mc + "BFHIP_AIR_TREE_INTERACTION without a fraction program");
                if (col >= n_inter) no(mc + "interaction column " + std::to_string(col) + " out of range (the component has " + std::to_string(n_inter) + ")");
                continue;
            }
            if (t >= st->n_trees) no(mc + "tree " + std::to_string(t) + " out of range (n_trees " + std::to_string(st->n_trees) + ")");
            if (col >= st->trees[t].n_cols) no(mc + "tree " + std::to_string(t) + " has " + std::to_string(st->trees[t].n_cols) + " columns, got column " + std::to_string(col));
            if (st->trees[t].log_sizes_h[col] != p.log_size)
                no(mc + "tree " + std::to_string(t) + " column " + std::to_string(col) + " has log_size " + std::to_string(st->trees[t].log_sizes_h[col]) + ", the component " + std::to_string(p.log_size));
        }
        for (u32 c = 0; lp && c < lp->n_cols; c++) {
            const u32 t = p.frac_trees_h[c], col = p.frac_columns_h[c];
            const std::string mc = "fraction column " + std::to_string(c) + ": ";
            if (t >= st->n_trees) no(mc + "tree " + std::to_string(t) + " out of range (n_trees " + std::to_string(st->n_trees) + ")");
            if (col >= st->trees[t].n_cols) no(mc + "tree " + std::to_string(t) + " has " + std::to_string(st->trees[t].n_cols) + " columns, got column " + std::to_string(col));
            if (st->trees[t].form != 0) no(mc + "tree " + std::to_string(t) + " is committed as coefficients (form 1): fractions run on trace-domain evaluations");
            if (st->trees[t].log_sizes_h[col] != p.log_size)
                no(mc + "tree " + std::to_string(t) + " column " + std::to_string(col) + " has log_size " + std::to_string(st->trees[t].log_sizes_h[col]) + ", the component " + std::to_string(p.log_size));
        }
        if (lp) {
            plan.frac_comps.push_back(k);
            plan.inter_first[k] = (u32)inter_logs.size();
            inter_logs.insert(inter_logs.end(), n_inter, p.log_size);
        }
        if (p.log_size + p.log_expand > plan.composition_log) plan.composition_log = p.log_size + p.log_expand;
    }
    if (plan.composition_log + log_blowup > max_log_domain)
        refuse("the composition polynomial has log size " + std::to_string(plan.composition_log) + ", above max_log_domain - log_blowup_factor = " +
               std::to_string(max_log_domain > log_blowup ? max_log_domain - log_blowup : 0));
    plan.has_interaction = !inter_logs.empty();
    if (plan.has_interaction) {
        if (inter_logs.size() > BFHIP_PCS_MAX_COLUMNS) refuse("the interaction tree has " + std::to_string(inter_logs.size()) + " columns, more than BFHIP_PCS_MAX_COLUMNS (4096)");
        plan.tree_logs.push_back(inter_logs);
    }
    plan.tree_logs.push_back(std::vector<u32>(4, plan.composition_log));

    // ---- the sample description: points in order of first use, a column's samples in order of first use, each once ------------------------
    plan.samples.resize(plan.tree_logs.size());
    for (size_t t = 0; t < plan.tree_logs.size(); t++) plan.samples[t].resize(plan.tree_logs[t].size());
    plan.points.push_back(AirPlan::Point{0, 0});
    plan.mask_refs.resize(st->n_components);
    for (u32 k = 0; k < st->n_components; k++) {
        const bfhip_air_statement_component& p = st->components[k];
        const bfhip_air* air = p.program;
        for (size_t i = 0; i < air->mask_cols.size(); i++) {
            const u32 c = air->mask_cols[i];
            const int32_t off = air->mask_offs[i];
            u32 pt = 0;
            if (off != 0) {
                for (pt = 1; pt < plan.points.size(); pt++) if (plan.points[pt].log_size == p.log_size && plan.points[pt].off == off) break;
                if (pt == plan.points.size()) {
                    if (plan.points.size() == BFHIP_PCS_MAX_POINTS) refuse("component " + std::to_string(k) + ": the mask needs more than BFHIP_PCS_MAX_POINTS (64) points");
                    plan.points.push_back(AirPlan::Point{p.log_size, off});
                }
            }
            const bool inter = p.col_trees_h[c] == BFHIP_AIR_TREE_INTERACTION;
            const u32 tree = inter ? plan.interaction_tree() : p.col_trees_h[c], col = inter ? plan.inter_first[k] + p.col_columns_h[c] : p.col_columns_h[c];
            std::vector<u32>& s = plan.samples[tree][col];
            u32 pos = 0;
            while (pos < s.size() && s[pos] != pt) pos++;
            if (pos == s.size()) {
                if (s.size() == BFHIP_PCS_MAX_SAMPLES_PER_COLUMN)
                    refuse("component " + std::to_string(k) + ": " + (inter ? "interaction column " + std::to_string(p.col_columns_h[c]) : "tree " + std::to_string(tree) + " column " + std::to_string(col)) +
                           " would be opened at more than BFHIP_PCS_MAX_SAMPLES_PER_COLUMN (2) points");
                s.push_back(pt);
            }
            plan.mask_refs[k].push_back(AirPlan::Ref{tree, col, pos});
        }
    }
    for (auto& c : plan.samples[plan.composition_tree()]) c.push_back(0);
    return plan;
}

// The parameter table of component k resolved to words: lookup = (z_r, alpha_r) per relation, 8 words each; claimed = the component's own sum
inline void air_statement_params(const bfhip_air_statement_component& p, const u32* lookup, const u32* claimed, std::vector<u32>& out) {
    out.assign(4 * (size_t)p.n_params, 0);
    for (u32 i = 0; i < p.n_params; i++) {
        const bfhip_air_param_rule& r = p.params_h[i];
        u32* w = out.data() + 4 * (size_t)i;
        if (r.kind == BFHIP_AIR_PARAM_CONST) for (int j = 0; j < 4; j++) w[j] = r.value[j];
        else if (r.kind == BFHIP_AIR_PARAM_LOOKUP_Z) for (int j = 0; j < 4; j++) w[j] = lookup[8 * r.relation + j];
        else if (r.kind == BFHIP_AIR_PARAM_CLAIMED_SUM) for (int j = 0; j < 4; j++) w[j] = claimed ? claimed[j] : 0;
        else {
            const u32* a = lookup + 8 * r.relation + 4;
            const Q31 alpha = q_make(a[0], a[1], a[2], a[3]);
            Q31 cur = q_one();
            for (u32 e = 0; e < r.power; e++) cur = q_mul(cur, alpha);
            w[0] = cur.a.a; w[1] = cur.a.b; w[2] = cur.b.a; w[3] = cur.b.b;
        }
    }
}

// The mask points at the drawn point: point 0 = oods, the others bfhip_circle_point_offset(oods, log_size, off). 8 words each.
inline std::vector<u32> air_statement_points(const AirPlan& plan, const u32 oods[8], const std::string& me) {
    std::vector<u32> pts(8 * plan.points.size());
    for (int w = 0; w < 8; w++) pts[w] = oods[w];
    for (size_t i = 1; i < plan.points.size(); i++)
        if (bfhip_circle_point_offset(oods, plan.points[i].log_size, plan.points[i].off, pts.data() + 8 * i) != 0) throw std::runtime_error(me + ": " + bfhip_last_error());
    return pts;
}

// (n_samples per column, point indices) flat, as bfhip_pcs_prove_values and bfhip_pcs_verifier_verify_values take them
inline void air_statement_flat_samples(const AirPlan& plan, std::vector<u32>& n_samples, std::vector<u32>& point_idx) {
    n_samples.clear(); point_idx.clear();
    for (auto& t : plan.samples) for (auto& c : t) { n_samples.push_back((u32)c.size()); for (u32 i : c) point_idx.push_back(i); }
}

// SecureField::from_partial_evals over four sampled coordinate values of 4 words each
inline Q31 air_from_partial_evals(const Q31 v[4]) {
    Q31 r = v[0];
    r = q_add(r, q_mul(v[1], q_make(0, 1, 0, 0)));
    r = q_add(r, q_mul(v[2], q_make(0, 0, 1, 0)));
    return q_add(r, q_mul(v[3], q_make(0, 0, 0, 1)));
}

// Components::eval_composition_polynomial_at_point over the statement: every component's mask values picked from the sampled values
// sv[tree][column][sample] (4 words each, flat per column) through the plan, its parameters resolved, then bfhip_air_compose_at_point.
// claimed = 4 words per component of the statement (unused where a component has no fraction program).
inline Q31 air_statement_composition_at_point(const std::string& me, const bfhip_air_statement* st, const AirPlan& plan, const std::vector<std::vector<std::vector<u32>>>& sv,
                                              const u32* lookup, const u32* claimed, const u32 oods[8], const u32 random_coeff[4]) {
    std::vector<std::vector<u32>> masks(st->n_components), params(st->n_components);
    std::vector<bfhip_air_point_component> pc(st->n_components);
    for (u32 k = 0; k < st->n_components; k++) {
        const bfhip_air_statement_component& p = st->components[k];
        for (const AirPlan::Ref& r : plan.mask_refs[k]) {
            const std::vector<u32>& col = sv.at(r.tree).at(r.col);
            if (4 * (size_t)r.pos + 4 > col.size()) throw std::out_of_range("a sampled value the AIR reads is missing");
            masks[k].insert(masks[k].end(), col.begin() + 4 * r.pos, col.begin() + 4 * r.pos + 4);
        }
        air_statement_params(p, lookup, claimed + 4 * (size_t)k, params[k]);
        pc[k] = bfhip_air_point_component{p.program, p.log_size, (u32)plan.mask_refs[k].size(), masks[k].empty() ? nullptr : masks[k].data(),
                                          params[k].empty() ? nullptr : params[k].data(), p.n_params, 0};
    }
    u32 out[4];
    if (bfhip_air_compose_at_point(pc.data(), st->n_components, oods, random_coeff, out) != 0) throw std::runtime_error(me + ": " + bfhip_last_error());
    return q_make(out[0], out[1], out[2], out[3]);
}

}  // namespace bf
