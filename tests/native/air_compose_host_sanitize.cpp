// CPU sanitizer harness for the host-only composition entries (stwo-brainfuck_amd/csrc/air_program_host.hip: bfhip_air_compose_coeffs,
// bfhip_air_compose_at_point). tests/test_air_compose_cpu.py compiles this file TOGETHER with air_program_host.hip (as C++: the file makes
// no HIP call) under g++ -fsanitize=address,undefined and runs the program directly:
//   air_compose_host_sanitize <programs.txt>
// programs.txt: one accepted program per line, "<n_cols> <n_params> <word> <word> ...": the components of one AIR in list order (the test
// writes the 13 Brainfuck programs under both mask orders). The program composes every prefix of the list at a point with random
// canonical values, checks the sum against the per-component evaluator under bfhip_air_compose_coeffs' slices, runs the coefficient cases
// of the test ([1], the 13 Brainfuck counts in both forms, 64 x 64) against powers computed here, and tries every refusal. Prints two summary lines.
#include "../../include/bfhip.h"
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

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t next64() { g_state += 0x9E3779B97F4A7C15ull; uint64_t z = g_state; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static const uint32_t P = 0x7fffffffu;
static uint32_t word() { return next64() % 4 == 0 ? P - 1 : (uint32_t)(next64() % P); }

// QM31 = CM31[u] / (u^2 - 2 - i), written from the definition
struct Q { uint64_t v[4]; };
static void cmul(uint64_t a0, uint64_t a1, uint64_t b0, uint64_t b1, uint64_t& r0, uint64_t& r1) { r0 = (a0 * b0 % P + (P - a1 * b1 % P)) % P; r1 = (a0 * b1 % P + a1 * b0 % P) % P; }
static Q qmul(const Q& x, const Q& y) {
    uint64_t ac0, ac1, ad0, ad1, bc0, bc1, bd0, bd1, e0, e1;
    cmul(x.v[0], x.v[1], y.v[0], y.v[1], ac0, ac1); cmul(x.v[0], x.v[1], y.v[2], y.v[3], ad0, ad1);
    cmul(x.v[2], x.v[3], y.v[0], y.v[1], bc0, bc1); cmul(x.v[2], x.v[3], y.v[2], y.v[3], bd0, bd1);
    cmul(bd0, bd1, 2, 1, e0, e1);
    return Q{{(ac0 + e0) % P, (ac1 + e1) % P, (ad0 + bc0) % P, (ad1 + bc1) % P}};
}

static int check_coeffs(const std::vector<uint32_t>& counts, const uint32_t r[4]) {
    size_t total = 0;
    for (uint32_t c : counts) total += c;
    std::vector<uint32_t> out(4 * total);      // exactly 4 * T words: a write past them is the sanitizer's to find
    if (bfhip_air_compose_coeffs(counts.data(), (uint32_t)counts.size(), r, out.data()) != 0) return 1;
    Q cur{{1, 0, 0, 0}};
    const Q rq{{r[0], r[1], r[2], r[3]}};
    for (size_t g = total; g-- > 0;) {
        for (int w = 0; w < 4; w++) if (out[4 * g + w] != cur.v[w]) return 2;
        cur = qmul(cur, rq);
    }
    return 0;
}

struct Comp { bfhip_air* air; uint32_t shape[8]; uint32_t n_mask, log_size; std::vector<uint32_t> mask, params; };

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: air_compose_host_sanitize <programs.txt>\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    std::vector<Comp> comps;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        uint64_t n_cols, n_params, w;
        ss >> n_cols >> n_params;
        std::vector<uint32_t> code;
        while (ss >> w) code.push_back((uint32_t)w);
        Comp c{};
        if (bfhip_air_create(code.data(), code.size(), (uint32_t)n_cols, (uint32_t)n_params, &c.air) != 0) { printf("internal: a listed program is refused: %s\n", g_error.c_str()); return 2; }
        if (bfhip_air_shape(c.air, c.shape) != 0 || bfhip_air_mask(c.air, nullptr, nullptr, 0, &c.n_mask) != 0) return 2;
        c.log_size = 1 + (uint32_t)(next64() % 30);
        c.mask.resize(4 * (size_t)c.n_mask); c.params.resize(4 * (size_t)c.shape[1]);      // exact sizes again
        for (auto& v : c.mask) v = word();
        for (auto& v : c.params) v = word();
        comps.push_back(std::move(c));
    }
    if (comps.empty() || comps.size() > 64) { printf("internal: 1 to 64 listed programs\n"); return 2; }
    const uint32_t point[8] = {11, 12, 13, 14, 15, 16, 17, 18};      // the evaluator needs x and a non-zero denominator, not a point of the circle
    const uint32_t r[4] = {word(), word(), word(), word()};
    auto point_comps = [&](size_t n) {
        std::vector<bfhip_air_point_component> pc(n);
        for (size_t k = 0; k < n; k++) {
            const Comp& c = comps[k];
            pc[k] = bfhip_air_point_component{c.air, c.log_size, c.n_mask, c.mask.empty() ? nullptr : c.mask.data(), c.params.empty() ? nullptr : c.params.data(), c.shape[1], 0};
        }
        return pc;
    };
    // every prefix: the composed value = the per-component values under the slices of bfhip_air_compose_coeffs, added up
    int mismatches = 0;
    for (size_t n = 1; n <= comps.size(); n++) {
        const auto pc = point_comps(n);
        uint32_t got[4];
        if (bfhip_air_compose_at_point(pc.data(), (uint32_t)n, point, r, got) != 0) { printf("internal: prefix %zu: %s\n", n, g_error.c_str()); return 2; }
        std::vector<uint32_t> counts(n);
        size_t total = 0;
        for (size_t k = 0; k < n; k++) { counts[k] = comps[k].shape[2]; total += counts[k]; }
        std::vector<uint32_t> coeffs(4 * total);
        if (bfhip_air_compose_coeffs(counts.data(), (uint32_t)n, r, coeffs.data()) != 0) return 2;
        uint64_t sum[4] = {0, 0, 0, 0};
        size_t first = 0;
        for (size_t k = 0; k < n; k++) {
            uint32_t one[4];
            if (bfhip_air_eval_at_point(comps[k].air, comps[k].log_size, point, pc[k].mask_values_h, pc[k].n_mask, pc[k].params_h, pc[k].n_params, coeffs.data() + 4 * first,
                                        counts[k], one) != 0) return 2;
            for (int w = 0; w < 4; w++) sum[w] = (sum[w] + one[w]) % P;
            first += counts[k];
        }
        for (int w = 0; w < 4; w++) if (got[w] != sum[w]) mismatches++;
    }
    // the coefficient cases of the test
    const uint32_t r2[4] = {P - 1, 0, 5, P - 2};
    int coeff_fail = check_coeffs({1}, r) + check_coeffs({12, 11, 5, 10, 9, 9, 6, 6, 7, 7, 7, 6, 2}, r) + check_coeffs({12, 11, 5, 10, 9, 9, 7, 7, 8, 8, 8, 7, 2}, r) + check_coeffs(std::vector<uint32_t>(64, 64), r2);
    printf("prefixes: %zu composed, %d mismatching words; coefficient cases failing: %d\n", comps.size(), mismatches, coeff_fail);

    // refusals: each is -1, none reads through a null pointer or past a list
    int refused = 0, tried = 0;
    auto expect = [&](int32_t rc, const char* what) { tried++; if (rc == -1 && g_error.find(what) != std::string::npos) refused++; else printf("not refused as expected (%s): %d %s\n", what, rc, g_error.c_str()); };
    uint32_t out4[4], big[4 * 65];
    const uint32_t one_count[1] = {1}, zero_count[1] = {0}, many[65] = {}, bad_r[4] = {0, P, 0, 0};
    auto pc = point_comps(1);
    expect(bfhip_air_compose_coeffs(nullptr, 1, r, big), "null argument");
    expect(bfhip_air_compose_coeffs(one_count, 1, nullptr, big), "null argument");
    expect(bfhip_air_compose_coeffs(one_count, 1, r, nullptr), "null argument");
    expect(bfhip_air_compose_coeffs(one_count, 0, r, big), "bfhip_air_compose_coeffs: 1 to BFHIP_AIR_COMPOSE_MAX_COMPONENTS");
    expect(bfhip_air_compose_coeffs(many, 65, r, big), "bfhip_air_compose_coeffs: 1 to BFHIP_AIR_COMPOSE_MAX_COMPONENTS");
    expect(bfhip_air_compose_coeffs(zero_count, 1, r, big), "component 0: a component has 1 to");
    expect(bfhip_air_compose_coeffs(one_count, 1, bad_r, big), "canonical");
    expect(bfhip_air_compose_at_point(nullptr, 1, point, r, out4), "null argument");
    expect(bfhip_air_compose_at_point(pc.data(), 1, nullptr, r, out4), "null argument");
    expect(bfhip_air_compose_at_point(pc.data(), 1, point, nullptr, out4), "null argument");
    expect(bfhip_air_compose_at_point(pc.data(), 1, point, r, nullptr), "null argument");
    expect(bfhip_air_compose_at_point(pc.data(), 0, point, r, out4), "bfhip_air_compose_at_point: 1 to BFHIP_AIR_COMPOSE_MAX_COMPONENTS");
    expect(bfhip_air_compose_at_point(pc.data(), 65, point, r, out4), "bfhip_air_compose_at_point: 1 to BFHIP_AIR_COMPOSE_MAX_COMPONENTS");
    expect(bfhip_air_compose_at_point(pc.data(), 1, point, bad_r, out4), "canonical");
    { auto q = pc; q[0].reserved = 1; expect(bfhip_air_compose_at_point(q.data(), 1, point, r, out4), "component 0: reserved must be 0"); }
    { auto q = pc; q[0].program = nullptr; expect(bfhip_air_compose_at_point(q.data(), 1, point, r, out4), "component 0: null argument"); }
    { auto q = pc; q[0].n_mask++; expect(bfhip_air_compose_at_point(q.data(), 1, point, r, out4), "component 0: the program's mask has"); }
    { auto q = pc; q[0].n_params++; q[0].params_h = big; expect(bfhip_air_compose_at_point(q.data(), 1, point, r, out4), "component 0: the program takes"); }
    { auto q = pc; q[0].log_size = 0; expect(bfhip_air_compose_at_point(q.data(), 1, point, r, out4), "component 0: log_size"); }
    { auto q = pc; q[0].log_size = 31; expect(bfhip_air_compose_at_point(q.data(), 1, point, r, out4), "component 0: log_size"); }
    if (comps[0].n_mask) {
        auto q = pc;
        std::vector<uint32_t> m = comps[0].mask;
        m[1] = P; q[0].mask_values_h = m.data();
        expect(bfhip_air_compose_at_point(q.data(), 1, point, r, out4), "component 0: a word is not a canonical M31");
    }
    if (comps.size() > 1) { auto q = point_comps(2); q[1].reserved = 7; expect(bfhip_air_compose_at_point(q.data(), 2, point, r, out4), "component 1: reserved must be 0"); }
    printf("refused %d of %d\n", refused, tried);
    for (Comp& c : comps) bfhip_air_destroy(c.air);
    return mismatches == 0 && coeff_fail == 0 && refused == tried ? 0 : 3;
}
