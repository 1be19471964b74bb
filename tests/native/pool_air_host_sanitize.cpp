// CPU sanitizer harness for the two host-only headers behind bfhip_pool_submit_air and the scratch reserve:
//   stwo-brainfuck_amd/csrc/air_statement_copy.h   the deep copy a queued job keeps of the caller's statement and column-pointer table
//   stwo-brainfuck_amd/csrc/scratch_reserve.h      the bookkeeping of bfhip_ctx_set_scratch_reserve (marks, alignment, fallback, high water)
// tests/test_pool_air_cpu.py compiles this file TOGETHER with air_prove_host.hip, air_program_host.hip, logup_program_host.hip and
// pcs_host.hip (as C++: none makes a HIP call) under g++ -fsanitize=address,undefined and runs the program directly:
//   pool_air_host_sanitize <log_blowup> <max_log_domain> <statement.txt> [<statement.txt> ...]
// statement.txt: the format of tests/native/air_prove_host_sanitize.cpp. Per statement: every array the statement points to is a heap block
// of its exact size; the plan of the original is taken (air_statement_plan), the statement is copied, every source block is overwritten and
// freed, and the plan of the copy must be the original's, word for word, and the copied column pointers the original's. One line
// "copy ok <trees> <components> <plan words>" per statement, then "reserve ok <checks>".
#include "../../stwo-brainfuck_amd/csrc/air_statement_copy.h"
#include "../../stwo-brainfuck_amd/csrc/scratch_reserve.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

// what api_ctx.hip provides inside the library
static std::string g_error;
void bfhip_set_error(const std::string& s) { g_error = s; }
extern "C" const char* bfhip_last_error(void) { return g_error.c_str(); }
extern "C" void bfhip_free_host(void* p) { free(p); }

using bf::u32;

struct Comp {
    bfhip_air* air = nullptr; bfhip_logup* lp = nullptr;
    uint32_t log_size = 0, log_expand = 0;
    std::vector<uint32_t> col_t, col_c, frac_t, frac_c;
    std::vector<bfhip_air_param_rule> rules;
};
struct Tree { uint32_t form = 0; std::vector<uint64_t> mix; std::vector<uint32_t> logs; };

// heap blocks of exact size, remembered so that they can be overwritten and freed behind the copy
struct Blocks {
    std::vector<std::pair<void*, size_t>> all;
    template <class T> T* dup(const std::vector<T>& v) {
        if (v.empty()) return nullptr;
        T* p = (T*)malloc(v.size() * sizeof(T));
        memcpy(p, v.data(), v.size() * sizeof(T));
        all.emplace_back(p, v.size() * sizeof(T));
        return p;
    }
    void scribble_and_free() { for (auto& b : all) { memset(b.first, 0xA5, b.second); free(b.first); } all.clear(); }
};

static std::string words_of(const bf::AirPlan& p) {
    std::ostringstream o;
    o << p.n_caller_trees << ' ' << p.has_interaction << ' ' << p.composition_log;
    for (auto& t : p.tree_logs) { o << " T" << t.size(); for (u32 l : t) o << ' ' << l; }
    for (auto& pt : p.points) o << " P" << pt.log_size << ',' << pt.off;
    for (auto& t : p.samples) for (auto& c : t) { o << " S" << c.size(); for (u32 i : c) o << ' ' << i; }
    for (auto& m : p.mask_refs) { o << " M" << m.size(); for (auto& r : m) o << ' ' << r.tree << ',' << r.col << ',' << r.pos; }
    for (u32 k : p.frac_comps) o << " F" << k;
    for (u32 k : p.inter_first) o << " I" << k;
    return o.str();
}

static int fail(const char* what) { printf("FAILED: %s\n", what); return 3; }

static int check_reserve() {
    using R = bf::ScratchReserve;
    int checks = 0;
#define EXPECT(cond) do { if (!(cond)) return fail(#cond); checks++; } while (0)
    R r;
    // no block: nothing is served, guards still open and close
    { auto m = r.open(); EXPECT(r.take(16) == R::kNone); EXPECT(r.close(m)); EXPECT(r.idle()); }
    r.set(4096);
    EXPECT(r.bytes == 4096 && r.used == 0 && r.high_water == 0);
    auto outer = r.open();
    EXPECT(r.take(0) == R::kNone);                                   // an empty request is the device's to answer, as before
    EXPECT(r.take(100) == 0 && r.used == 100);
    EXPECT(r.take(1) == 256 && r.used == 257);                       // placed on the next multiple of 256
    auto inner = r.open();
    EXPECT(r.take(1000) == 512 && r.used == 1512 && r.high_water == 1512);
    EXPECT(r.take(4096) == R::kNone && r.used == 1512);              // does not fit behind what is in use: nothing changes
    EXPECT(r.take(4096 - 1536) == 1536 && r.used == 4096);           // fits exactly
    EXPECT(r.take(1) == R::kNone);                                   // full
    EXPECT(!r.close(outer) && r.used == 4096 && r.depth == 2);       // out of order: refused, nothing changes
    auto innermost = r.open();
    EXPECT(!r.close(inner));
    EXPECT(r.close(innermost) && r.close(inner) && r.used == 257 && r.depth == 1);
    EXPECT(!r.close(inner));                                         // twice
    EXPECT(r.take(300) == 512 && r.high_water == 4096);              // the space of the closed guard is handed out again; the mark stays
    EXPECT(r.close(outer) && r.idle() && r.high_water == 4096);
    EXPECT(!r.close(outer));                                         // no guard open
    EXPECT(r.served == 5 && r.device_allocs == 0);
    // a request larger than size_t arithmetic would survive
    { auto m = r.open(); EXPECT(r.take(~size_t(0)) == R::kNone && r.take(~size_t(0) - 255) == R::kNone); EXPECT(r.close(m)); }
    r.set(100);                                                      // smaller than one alignment step
    { auto m = r.open(); EXPECT(r.take(100) == 0 && r.take(1) == R::kNone && r.high_water == 100); EXPECT(r.close(m)); }
    r.set(0);
    EXPECT(r.bytes == 0 && r.high_water == 0 && r.served == 6);
#undef EXPECT
    printf("reserve ok %d\n", checks);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: pool_air_host_sanitize <log_blowup> <max_log_domain> <statement.txt> ...\n"); return 2; }
    const uint32_t log_blowup = (uint32_t)atoi(argv[1]), max_log_domain = (uint32_t)atoi(argv[2]);
    for (int a = 3; a < argc; a++) {
        std::ifstream in(argv[a]);
        std::string line;
        std::vector<Tree> trees;
        std::vector<Comp> comps;
        uint32_t n_relations = 0;
        while (std::getline(in, line)) {
            std::istringstream ss(line);
            std::string what;
            if (!(ss >> what)) continue;
            uint64_t n, v;
            if (what == "relations") { ss >> n; n_relations = (uint32_t)n; }
            else if (what == "tree") {
                Tree t; ss >> t.form >> n;
                for (uint64_t i = 0; i < n; i++) { ss >> v; t.mix.push_back(v); }
                ss >> n;
                for (uint64_t i = 0; i < n; i++) { ss >> v; t.logs.push_back((uint32_t)v); }
                trees.push_back(t);
            } else if (what == "comp") { Comp c; ss >> c.log_size >> c.log_expand; comps.push_back(c); }
            else if (what == "air" || what == "logup") {
                uint64_t n_cols, n_params;
                ss >> n_cols >> n_params;
                std::vector<uint32_t> code;
                while (ss >> v) code.push_back((uint32_t)v);
                const int32_t rc = what == "air" ? bfhip_air_create(code.data(), code.size(), (uint32_t)n_cols, (uint32_t)n_params, &comps.back().air)
                                                 : bfhip_logup_create(code.data(), code.size(), (uint32_t)n_cols, (uint32_t)n_params, &comps.back().lp);
                if (rc != 0) { printf("internal: a listed program is refused: %s\n", g_error.c_str()); return 2; }
            } else if (what == "cols" || what == "frac") {
                Comp& c = comps.back();
                ss >> n;
                for (uint64_t i = 0; i < n; i++) { uint32_t t, col; ss >> t >> col; (what == "cols" ? c.col_t : c.frac_t).push_back(t); (what == "cols" ? c.col_c : c.frac_c).push_back(col); }
            } else if (what == "params") {
                ss >> n;
                for (uint64_t i = 0; i < n; i++) { bfhip_air_param_rule r{}; ss >> r.kind >> r.relation >> r.power >> r.value[0] >> r.value[1] >> r.value[2] >> r.value[3]; comps.back().rules.push_back(r); }
            } else { printf("internal: unknown item %s\n", what.c_str()); return 2; }
        }

        // ---- the statement and the table of column pointers, every array a heap block of its exact size ----------------------------------
        Blocks heap;
        std::vector<bfhip_air_statement_tree> st_trees;
        std::vector<bfhip_air_statement_component> st_comps;
        std::vector<const u32* const*> table;
        std::vector<std::vector<const u32*>> want_cols;              // the "device pointers": numbers that are never dereferenced
        for (size_t t = 0; t < trees.size(); t++) {
            st_trees.push_back(bfhip_air_statement_tree{(uint32_t)trees[t].logs.size(), trees[t].form, heap.dup(trees[t].logs), heap.dup(trees[t].mix), (uint32_t)trees[t].mix.size(), 0});
            std::vector<const u32*> cols;
            for (size_t c = 0; c < trees[t].logs.size(); c++) cols.push_back(reinterpret_cast<const u32*>(uintptr_t(0x1000000) * (t + 1) + 256 * c));
            want_cols.push_back(cols);
            table.push_back(heap.dup(cols));
        }
        for (const Comp& c : comps)
            st_comps.push_back(bfhip_air_statement_component{c.air, c.lp, c.log_size, c.log_expand, heap.dup(c.col_t), heap.dup(c.col_c), heap.dup(c.frac_t), heap.dup(c.frac_c), heap.dup(c.rules),
                                                             (uint32_t)c.rules.size(), 0});
        bfhip_air_statement* st = (bfhip_air_statement*)malloc(sizeof(bfhip_air_statement));
        *st = bfhip_air_statement{heap.dup(st_trees), heap.dup(st_comps), (uint32_t)st_trees.size(), n_relations, (uint32_t)st_comps.size(), 0};
        heap.all.emplace_back(st, sizeof *st);
        const u32* const* const* tree_cols = heap.dup(table);

        std::string before;
        try { before = words_of(bf::air_statement_plan("pool_air_host_sanitize", st, log_blowup, max_log_domain)); }
        catch (const std::exception& e) { printf("internal: the statement is refused: %s\n", e.what()); return 2; }

        bf::AirStatementCopy copy;
        copy.assign("pool_air_host_sanitize", st, tree_cols);
        heap.scribble_and_free();                                    // what the caller may do once the submit has returned

        std::string after;
        try { after = words_of(bf::air_statement_plan("pool_air_host_sanitize", &copy.st, log_blowup, max_log_domain)); }
        catch (const std::exception& e) { printf("FAILED: the copy is refused: %s\n", e.what()); return 3; }
        if (after != before) return fail("the plan of the copy is not the plan of the original");
        if (copy.tree_cols.size() != want_cols.size()) return fail("the copy has another number of trees");
        for (size_t t = 0; t < want_cols.size(); t++)
            for (size_t c = 0; c < want_cols[t].size(); c++)
                if (copy.tree_cols[t][c] != want_cols[t][c]) return fail("a copied column pointer differs");
        // the parameter rules and the mix words are not part of the plan: compare them with what was parsed
        for (size_t t = 0; t < trees.size(); t++)
            for (size_t i = 0; i < trees[t].mix.size(); i++)
                if (copy.st.trees[t].mix_u64_h[i] != trees[t].mix[i]) return fail("a copied mix word differs");
        for (size_t k = 0; k < comps.size(); k++) {
            const bfhip_air_statement_component& p = copy.st.components[k];
            if (p.program != comps[k].air || p.fractions != comps[k].lp || p.n_params != comps[k].rules.size()) return fail("a copied component differs");
            for (size_t i = 0; i < comps[k].rules.size(); i++)
                if (memcmp(&p.params_h[i], &comps[k].rules[i], sizeof(bfhip_air_param_rule)) != 0) return fail("a copied parameter rule differs");
            for (size_t i = 0; i < comps[k].frac_t.size(); i++)
                if (p.frac_trees_h[i] != comps[k].frac_t[i] || p.frac_columns_h[i] != comps[k].frac_c[i]) return fail("a copied fraction binding differs");
        }
        // a null row of the pointer table is the copy's one refusal of its own
        {
            std::vector<const u32* const*> rows(copy.tree_cols);
            rows.back() = nullptr;
            bf::AirStatementCopy other;
            bool refused = false;
            try { other.assign("me", &copy.st, rows.data()); } catch (const std::exception& e) { refused = std::string(e.what()) == "me: tree " + std::to_string(rows.size() - 1) + ": null argument"; }
            if (!refused) return fail("a null row of tree_cols_h is not refused by name");
        }
        printf("copy ok %zu %zu %s\n", trees.size(), comps.size(), after.c_str());
        for (Comp& c : comps) { bfhip_air_destroy(c.air); if (c.lp) bfhip_logup_destroy(c.lp); }
    }
    return check_reserve();
}
