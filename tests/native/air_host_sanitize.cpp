// CPU sanitizer harness for the host-only half of the constraint programs (stwo-brainfuck_amd/csrc/air_program_host.hip: bfhip_air_create,
// bfhip_air_shape, bfhip_air_mask, bfhip_air_eval_at_point). tests/test_air_program_cpu.py compiles this file TOGETHER with
// air_program_host.hip (as C++: the file makes no HIP call) under g++ -fsanitize=address,undefined and runs the program directly:
//   air_host_sanitize <programs.txt>
// programs.txt: one program per line, "<expected: 1 accepted / 0 refused> <n_cols> <n_params> <word> <word> ...". After the listed programs
// come 10 000 seeded random word arrays, mostly invalid: none may crash the validator, and whatever it accepts goes through shape, mask and
// the point evaluator with random canonical values. Prints three summary lines.
#include "../../include/bfhip.h"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

// what api_ctx.hip provides inside the library
static std::string g_error;
void bfhip_set_error(const std::string& s) { g_error = s; }

static uint64_t g_state = 0x2545F4914F6CDD1Dull;
static uint64_t next64() { g_state += 0x9E3779B97F4A7C15ull; uint64_t z = g_state; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static uint32_t below(uint32_t n) { return (uint32_t)(next64() % n); }
static const uint32_t P = 0x7fffffffu;

// an accepted program: shape, mask (size query, too small, exact) and the point evaluator at a point off the trace domain
static int exercise(bfhip_air* air) {
    uint32_t shape[8];
    if (bfhip_air_shape(air, shape) != 0) return 1;
    uint32_t n = 0;
    if (bfhip_air_mask(air, nullptr, nullptr, 0, &n) != 0) return 2;
    std::vector<uint32_t> cols(n + 1);
    std::vector<int32_t> offs(n + 1);
    if (n && bfhip_air_mask(air, cols.data(), offs.data(), n - 1, &n) != -2) return 3;
    if (bfhip_air_mask(air, cols.data(), offs.data(), n, &n) != 0) return 4;
    for (uint32_t i = 0; i < n; i++) if (cols[i] >= shape[0] || offs[i] < (int32_t)shape[6] || offs[i] > (int32_t)shape[7]) return 5;
    std::vector<uint32_t> mask(4 * n + 4), params(4 * shape[1] + 4), coeffs(4 * shape[2] + 4);
    for (auto* v : {&mask, &params, &coeffs}) for (auto& w : *v) w = below(4) == 0 ? P - 1 : below(P);
    const uint32_t point[8] = {1, 2, 3, 4, 5, 6, 7, 8};      // no point of the circle: the evaluator only needs x, and a non-zero denominator
    uint32_t out[4];
    if (bfhip_air_eval_at_point(air, 1 + below(30), point, mask.data(), n, params.data(), shape[1], coeffs.data(), shape[2], out) != 0) return 6;
    for (uint32_t w : out) if (w >= P) return 7;
    // the counts are checked, and so are the words
    if (bfhip_air_eval_at_point(air, 5, point, mask.data(), n + 1, params.data(), shape[1], coeffs.data(), shape[2], out) != -1) return 8;
    if (bfhip_air_eval_at_point(air, 5, point, mask.data(), n, params.data(), shape[1], coeffs.data(), shape[2] + 1, out) != -1) return 9;
    coeffs[0] = P;
    if (bfhip_air_eval_at_point(air, 5, point, mask.data(), n, params.data(), shape[1], coeffs.data(), shape[2], out) != -1) return 10;
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: air_host_sanitize <programs.txt>\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    int accepted = 0, refused = 0, unexpected = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        uint64_t expect, n_cols, n_params, w;
        ss >> expect >> n_cols >> n_params;
        std::vector<uint32_t> code;
        while (ss >> w) code.push_back((uint32_t)w);
        bfhip_air* air = nullptr;
        const int32_t rc = bfhip_air_create(code.data(), code.size(), (uint32_t)n_cols, (uint32_t)n_params, &air);
        if (rc == 0) {
            accepted++;
            if (!expect) unexpected++;
            if (const int e = exercise(air)) { printf("internal: exercise step %d: %s\n", e, g_error.c_str()); return 2; }
            if (bfhip_air_destroy(air) != 0) return 2;
        } else {
            refused++;
            if (expect || rc != -1 || g_error.find("bfhip_air_create: instruction ") != 0) { unexpected++; printf("unexpected: %s\n", g_error.c_str()); }
        }
    }
    printf("listed: %d accepted, %d refused, %d unexpected\n", accepted, refused, unexpected);
    // random word arrays: a third fully random, the rest with small fields so that whole prefixes validate
    int r_acc = 0, r_ref = 0;
    for (int t = 0; t < 10000; t++) {
        const uint32_t n_words = t % 7 == 0 ? below(70) : 4 * (1 + below(16));
        const bool wild = t % 3 == 0;
        std::vector<uint32_t> code(n_words + 1);
        for (uint32_t i = 0; i < n_words; i++) {
            const uint32_t field = i % 4;
            if (wild) code[i] = below(5) == 0 ? (uint32_t)next64() : below(20);
            else if (field == 0) code[i] = below(i + 8 >= n_words ? 17 : 14);
            else if (field == 3) code[i] = below(9) == 0 ? (uint32_t)(-(int32_t)below(20)) : below(4);
            else code[i] = below(6);
        }
        const uint32_t n_cols = below(12), n_params = below(5);
        bfhip_air* air = nullptr;
        const int32_t rc = bfhip_air_create(n_words ? code.data() : nullptr, n_words, n_cols, n_params, &air);
        if (rc == 0) {
            r_acc++;
            if (const int e = exercise(air)) { printf("internal: random program %d, exercise step %d: %s\n", t, e, g_error.c_str()); return 2; }
            bfhip_air_destroy(air);
        } else if (rc == -1) r_ref++;
        else { printf("internal: random program %d returned %d\n", t, rc); return 2; }
    }
    printf("random: %d accepted, %d refused of 10000\n", r_acc, r_ref);
    // edge calls: every one must be refused, none may read through a null pointer
    int edge_refused = 0, tried = 0;
    auto expect = [&](int32_t r) { tried++; if (r == -1) edge_refused++; };
    const uint32_t ok[8] = {1, 0, 1, 0, 13, 0, 0, 0};
    uint32_t out8[8], n = 0;
    bfhip_air* air = nullptr;
    expect(bfhip_air_create(nullptr, 8, 1, 0, &air));
    expect(bfhip_air_create(ok, 8, 1, 0, nullptr));
    expect(bfhip_air_create(ok, 0, 1, 0, &air));
    expect(bfhip_air_shape(nullptr, out8));
    expect(bfhip_air_mask(nullptr, nullptr, nullptr, 0, &n));
    expect(bfhip_air_eval_at_point(nullptr, 5, out8, nullptr, 0, nullptr, 0, ok, 1, out8));
    if (bfhip_air_create(ok, 8, 1, 0, &air) != 0) return 2;
    expect(bfhip_air_shape(air, nullptr));
    expect(bfhip_air_mask(air, nullptr, nullptr, 0, nullptr));
    expect(bfhip_air_eval_at_point(air, 5, nullptr, nullptr, 0, nullptr, 0, ok, 1, out8));
    expect(bfhip_air_eval_at_point(air, 5, ok, nullptr, 0, nullptr, 0, nullptr, 1, out8));
    expect(bfhip_air_eval_at_point(air, 0, ok, nullptr, 0, nullptr, 0, ok, 1, out8));
    bfhip_air_destroy(air);
    if (bfhip_air_destroy(nullptr) != 0) return 2;
    printf("edges refused %d of %d\n", edge_refused, tried);
    return unexpected == 0 && edge_refused == tried ? 0 : 3;
}
