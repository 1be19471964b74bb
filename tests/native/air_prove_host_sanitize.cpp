// CPU sanitizer harness for the host-only half of bfhip_air_prove / bfhip_air_verify (stwo-brainfuck_amd/csrc/air_statement.h: the validator
// and the sample-description builder; csrc/air_prove_host.hip: bfhip_air_statement_samples and bfhip_air_verify with its parsing).
// tests/test_air_prove_cpu.py compiles this file TOGETHER with air_prove_host.hip, air_program_host.hip, logup_program_host.hip and
// pcs_host.hip (as C++: none makes a HIP call) under g++ -fsanitize=address,undefined and runs the program directly:
//   air_prove_host_sanitize <statement.txt> <c0> <c1> <c2> <c3> <pow_bits> <log_blowup> <n_queries> [<proof.json> ...]
// statement.txt, one item per line (what the test writes from an AirStatement):
//   relations <n>
//   tree <form> <n_mix> <mix words> <n_cols> <log sizes>
//   comp <log_size> <log_expand>
//     air <n_cols> <n_params> <words>            the component's constraint program
//     logup <n_cols> <n_params> <words>          its fraction program (absent: none)
//     cols <n> <tree column>*   frac <n> <tree column>*   params <n> <kind relation power v0 v1 v2 v3>*
// Output: "samples <trees> <points> ..." (the description, flat), one verdict line per proof ("ok" or the rejection name), then
// "refused <a> of <b>" for the validator's refusals tried on mutated copies of the statement. Every array has its exact size.
#include "../../include/bfhip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

// what api_ctx.hip provides inside the library
static std::string g_error;
void bfhip_set_error(const std::string& s) { g_error = s; }
extern "C" const char* bfhip_last_error(void) { return g_error.c_str(); }
extern "C" void bfhip_free_host(void* p) { free(p); }

struct Comp {
    bfhip_air* air = nullptr; bfhip_logup* lp = nullptr;
    uint32_t log_size = 0, log_expand = 0;
    std::vector<uint32_t> col_t, col_c, frac_t, frac_c;
    std::vector<bfhip_air_param_rule> rules;
};
struct Tree { uint32_t form = 0; std::vector<uint64_t> mix; std::vector<uint32_t> logs; };
struct Built {
    std::vector<bfhip_air_statement_tree> trees; std::vector<bfhip_air_statement_component> comps; bfhip_air_statement st;
};

// exact-size arrays: an empty vector's data() may be null, which is what the statement then carries
static std::unique_ptr<Built> build(const std::vector<Tree>& trees, const std::vector<Comp>& comps, uint32_t n_relations) {
    std::unique_ptr<Built> b(new Built());
    for (const Tree& t : trees) b->trees.push_back(bfhip_air_statement_tree{(uint32_t)t.logs.size(), t.form, t.logs.data(), t.mix.data(), (uint32_t)t.mix.size(), 0});
    for (const Comp& c : comps)
        b->comps.push_back(bfhip_air_statement_component{c.air, c.lp, c.log_size, c.log_expand, c.col_t.data(), c.col_c.data(), c.frac_t.data(), c.frac_c.data(), c.rules.data(),
                                                         (uint32_t)c.rules.size(), 0});
    b->st = bfhip_air_statement{b->trees.data(), b->comps.data(), (uint32_t)b->trees.size(), n_relations, (uint32_t)b->comps.size(), 0};
    return b;
}

int main(int argc, char** argv) {
    if (argc < 9) { fprintf(stderr, "usage: air_prove_host_sanitize <statement.txt> <4 conventions> <pow_bits> <log_blowup> <n_queries> [proofs]\n"); return 2; }
    std::ifstream in(argv[1]);
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
    bfhip_conventions conv{};
    conv.merkle_node_hash = (uint32_t)atoi(argv[2]); conv.mix_u64 = (uint32_t)atoi(argv[3]); conv.logup_mask_order = (uint32_t)atoi(argv[4]); conv.merkle_channel = (uint32_t)atoi(argv[5]);
    bfhip_pcs_config pcs{};
    pcs.pow_bits = (uint32_t)atoi(argv[6]); pcs.log_blowup_factor = (uint32_t)atoi(argv[7]); pcs.n_queries = (uint32_t)atoi(argv[8]);

    // ---- the sample description, into arrays of exactly the stated sizes ------------------------------------------------------------------
    auto good = build(trees, comps, n_relations);
    uint32_t counts[4];
    if (bfhip_air_statement_samples(&good->st, &pcs, counts, nullptr, nullptr, nullptr, nullptr, nullptr) != 0) { printf("internal: the statement is refused: %s\n", g_error.c_str()); return 2; }
    {
        std::vector<uint32_t> per_tree(counts[0]), logs(counts[1]), ns(counts[2]), idx(counts[3] ? counts[3] : 1);
        std::vector<int32_t> offs(counts[1]);
        if (bfhip_air_statement_samples(&good->st, &pcs, counts, per_tree.data(), logs.data(), offs.data(), ns.data(), idx.data()) != 0) return 2;
        printf("samples %u %u", counts[0], counts[1]);
        for (uint32_t v : per_tree) printf(" %u", v);
        for (uint32_t i = 0; i < counts[1]; i++) printf(" %u %d", logs[i], offs[i]);
        for (uint32_t v : ns) printf(" %u", v);
        for (uint32_t i = 0; i < counts[3]; i++) printf(" %u", idx[i]);
        printf("\n");
    }

    // ---- the verifier over the given proofs ------------------------------------------------------------------------------------------------
    for (int a = 9; a < argc; a++) {
        std::ifstream pf(argv[a], std::ios::binary);
        std::stringstream buf; buf << pf.rdbuf();
        const std::string js = buf.str();
        std::vector<char> exact(js.begin(), js.end());      // no terminating NUL: a read past proof_len is the sanitizer's to find
        bfhip_channel* ch = nullptr;
        if (bfhip_channel_create(&conv, &ch) != 0) return 2;
        char err[512] = {0};
        const int32_t rc = bfhip_air_verify(&good->st, &conv, &pcs, ch, exact.empty() ? "" : exact.data(), exact.size(), err, sizeof err);
        bfhip_channel_destroy(ch);
        if (rc < 0) printf("error %s\n", g_error.c_str()); else printf("%s\n", rc == 0 ? "ok" : err);
    }

    // ---- the validator's refusals on mutated copies ---------------------------------------------------------------------------------------
    int refused = 0, tried = 0;
    auto expect = [&](const std::function<void(std::vector<Tree>&, std::vector<Comp>&, uint32_t&)>& mutate, const std::function<void(Built&)>& patch, const char* what) {
        std::vector<Tree> t = trees; std::vector<Comp> c = comps; uint32_t nr = n_relations;
        if (mutate) mutate(t, c, nr);
        auto b = build(t, c, nr);
        if (patch) patch(*b);
        uint32_t cnt[4];
        const int32_t rc = bfhip_air_statement_samples(&b->st, &pcs, cnt, nullptr, nullptr, nullptr, nullptr, nullptr);
        tried++;
        if (rc == -1 && g_error.find(what) != std::string::npos && g_error.find("bfhip_air_statement_samples: ") == 0) refused++;
        else printf("not refused as expected (%s): %d %s\n", what, rc, g_error.c_str());
    };
    using TV = std::vector<Tree>; using CV = std::vector<Comp>;
    expect(nullptr, [](Built& b) { b.st.reserved = 1; }, "reserved must be 0");
    expect(nullptr, [](Built& b) { b.st.n_trees = 0; }, "BFHIP_AIR_STATEMENT_MAX_TREES");
    expect(nullptr, [](Built& b) { b.st.n_trees = 9; }, "BFHIP_AIR_STATEMENT_MAX_TREES");
    expect(nullptr, [](Built& b) { b.st.n_relations = 17; }, "BFHIP_AIR_STATEMENT_MAX_RELATIONS");
    expect(nullptr, [](Built& b) { b.st.n_components = 0; }, "BFHIP_AIR_COMPOSE_MAX_COMPONENTS");
    expect(nullptr, [](Built& b) { b.st.n_components = 65; }, "BFHIP_AIR_COMPOSE_MAX_COMPONENTS");
    expect(nullptr, [](Built& b) { b.st.trees = nullptr; }, "null argument");
    expect(nullptr, [](Built& b) { b.trees[0].reserved = 2; }, "tree 0: reserved must be 0");
    expect([](TV& t, CV&, uint32_t&) { t[0].form = 2; }, nullptr, "tree 0: form must be");
    expect([](TV& t, CV&, uint32_t&) { t[0].logs[0] = 3; }, nullptr, "tree 0 column 0: log_size 3 outside");
    expect([](TV& t, CV&, uint32_t&) { t[0].logs[0] = 30; }, nullptr, "tree 0 column 0: log_size 30 outside");
    expect(nullptr, [](Built& b) { b.trees[0].log_sizes_h = nullptr; }, "tree 0: null argument");
    expect(nullptr, [](Built& b) { b.comps[0].reserved = 1; }, "component 0: reserved must be 0");
    expect(nullptr, [](Built& b) { b.comps[0].program = nullptr; }, "component 0: null program");
    expect(nullptr, [](Built& b) { b.comps[0].col_trees_h = nullptr; }, "component 0: null argument");
    expect([](TV&, CV& c, uint32_t&) { c[0].log_expand = 0; }, nullptr, "component 0: log_expand must be 1, 2 or 3, got 0");
    expect([](TV&, CV& c, uint32_t&) { c[0].log_expand = 4; }, nullptr, "component 0: log_expand must be 1, 2 or 3, got 4");
    expect([](TV&, CV& c, uint32_t&) { c[0].log_size = 3; }, nullptr, "component 0: log_size 3 outside");
    expect([](TV&, CV& c, uint32_t&) { c[0].log_size += 1; }, nullptr, "has log_size");
    expect([](TV&, CV& c, uint32_t&) { c[0].rules.pop_back(); }, nullptr, "component 0: the constraint program takes");
    expect([](TV&, CV& c, uint32_t&) { c[0].col_t[0] = 7; }, nullptr, "component 0: column 0: tree 7 out of range");
    expect([](TV&, CV& c, uint32_t&) { c[0].col_c[0] = 100000; }, nullptr, "component 0: column 0: tree");
    expect([](TV&, CV& c, uint32_t&) { if (!c[0].rules.empty()) c[0].rules[0].kind = 9; }, nullptr, "parameter 0: unknown kind 9");
    expect([](TV&, CV& c, uint32_t&) { if (!c[0].rules.empty()) c[0].rules[0].reserved = 1; }, nullptr, "parameter 0: reserved must be 0");
    expect([](TV&, CV& c, uint32_t&) { if (!c[0].rules.empty()) { c[0].rules[0].kind = BFHIP_AIR_PARAM_CONST; c[0].rules[0].value[2] = 0x7fffffffu; } }, nullptr, "parameter 0: a word is not a canonical M31");
    expect([](TV&, CV& c, uint32_t& nr) { if (!c[0].rules.empty()) { c[0].rules[0].kind = BFHIP_AIR_PARAM_LOOKUP_Z; c[0].rules[0].relation = nr; } }, nullptr, "parameter 0: relation");
    expect([](TV&, CV& c, uint32_t&) { if (!c[0].rules.empty()) { c[0].rules[0].kind = BFHIP_AIR_PARAM_LOOKUP_ALPHA_POW; c[0].rules[0].relation = 0; c[0].rules[0].power = 64; } }, nullptr, "parameter 0: power 64");
    if (comps[0].lp) {
        expect([](TV&, CV& c, uint32_t&) { c[0].rules[0].kind = BFHIP_AIR_PARAM_CLAIMED_SUM; }, nullptr, "parameter 0: CLAIMED_SUM among the fraction program's parameters");
        expect([](TV&, CV& c, uint32_t&) { c[0].lp = nullptr; }, nullptr, "without a fraction program");
        expect([](TV&, CV& c, uint32_t&) { c[0].frac_t[0] = 8; }, nullptr, "component 0: fraction column 0: tree 8 out of range");
        expect([](TV& t, CV& c, uint32_t&) { t[c[0].frac_t[0]].form = 1; }, nullptr, "fractions run on trace-domain evaluations");
        expect([](TV&, CV& c, uint32_t&) { for (size_t i = 0; i < c[0].col_t.size(); i++) if (c[0].col_t[i] == BFHIP_AIR_TREE_INTERACTION) { c[0].col_c[i] = 4000; break; } }, nullptr, "interaction column 4000 out of range");
    }
    printf("refused %d of %d\n", refused, tried);
    for (Comp& c : comps) { bfhip_air_destroy(c.air); if (c.lp) bfhip_logup_destroy(c.lp); }
    return refused == tried ? 0 : 3;
}
