// A deep copy of a bfhip_air_statement and of the table of column pointers that goes with it: what a job of the pool's queue keeps of the
// caller's arguments (pool.hip: bfhip_pool_submit_air), so that the caller may free every host array behind the statement as soon as the
// submit returns. Copied: trees, log sizes, mix words, components, bindings, parameter rules, and tree_cols_h down to the device pointers.
// NOT copied, because they are handles and device memory: the programs (bfhip_air, bfhip_logup; immutable, air_program.h) and the device
// columns themselves. Host only, plain C++: tests/native/pool_air_host_sanitize.cpp runs it under the sanitizers.
//
// The array lengths are the ones air_statement_plan (air_statement.h) has checked: copy a statement only after the validator accepted it.
#pragma once
#include "air_statement.h"
#include <stdexcept>
#include <string>
#include <vector>

namespace bf {

struct AirStatementCopy {
    bfhip_air_statement st{};                               // points into the members below
    std::vector<const u32* const*> tree_cols;               // what bfhip_air_prove takes as tree_cols_h
    AirStatementCopy() = default;
    AirStatementCopy(const AirStatementCopy&) = delete; AirStatementCopy& operator=(const AirStatementCopy&) = delete;

    // `me`: the caller's name for the one refusal of its own, a null row of tree_cols_h
    void assign(const std::string& me, const bfhip_air_statement* src, const u32* const* const* tree_cols_h) {
        const u32 nt = src->n_trees, nc = src->n_components;
        trees.assign(src->trees, src->trees + nt);
        logs.resize(nt); mixes.resize(nt); cols.resize(nt); tree_cols.resize(nt);
        for (u32 t = 0; t < nt; t++) {
            bfhip_air_statement_tree& tr = trees[t];
            if (!tree_cols_h[t]) throw std::runtime_error(me + ": tree " + std::to_string(t) + ": null argument");
            logs[t].assign(tr.log_sizes_h, tr.log_sizes_h + tr.n_cols);
            if (tr.n_mix) mixes[t].assign(tr.mix_u64_h, tr.mix_u64_h + tr.n_mix);
            cols[t].assign(tree_cols_h[t], tree_cols_h[t] + tr.n_cols);
            tr.log_sizes_h = logs[t].data();
            tr.mix_u64_h = tr.n_mix ? mixes[t].data() : nullptr;
            tree_cols[t] = cols[t].data();
        }
        comps.assign(src->components, src->components + nc);
        bind.resize(4 * (size_t)nc); rules.resize(nc);
        auto keep = [](std::vector<u32>& into, const u32*& p, u32 n) { if (n) into.assign(p, p + n); p = n ? into.data() : nullptr; };
        for (u32 k = 0; k < nc; k++) {
            bfhip_air_statement_component& p = comps[k];
            const u32 n_air = p.program->n_cols, n_frac = p.fractions ? p.fractions->n_cols : 0;
            keep(bind[4 * (size_t)k + 0], p.col_trees_h, n_air);
            keep(bind[4 * (size_t)k + 1], p.col_columns_h, n_air);
            keep(bind[4 * (size_t)k + 2], p.frac_trees_h, n_frac);
            keep(bind[4 * (size_t)k + 3], p.frac_columns_h, n_frac);
            if (p.n_params) rules[k].assign(p.params_h, p.params_h + p.n_params);
            p.params_h = p.n_params ? rules[k].data() : nullptr;
        }
        st = *src;
        st.trees = trees.data();
        st.components = comps.data();
    }

  private:
    std::vector<bfhip_air_statement_tree> trees;
    std::vector<std::vector<u32>> logs;
    std::vector<std::vector<uint64_t>> mixes;
    std::vector<std::vector<const u32*>> cols;
    std::vector<bfhip_air_statement_component> comps;
    std::vector<std::vector<u32>> bind;                      // per component: col_trees, col_columns, frac_trees, frac_columns
    std::vector<std::vector<bfhip_air_param_rule>> rules;
};

}  // namespace bf
