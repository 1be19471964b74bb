// CPU sanitizer harness for the host-only half of the fraction programs (stwo-brainfuck_amd/csrc/logup_program_host.hip: bfhip_logup_create,
// bfhip_logup_shape, bfhip_logup_destroy). tests/test_logup_program_cpu.py compiles this file TOGETHER with logup_program_host.hip (as C++:
// the file makes no HIP call) under g++ -fsanitize=address,undefined and runs the program directly:
//   logup_host_sanitize <programs.txt>
// programs.txt: one program per line, "<expected: 1 accepted / 0 refused> <n_cols> <n_params> <word> <word> ...". After the listed programs
// come 10 000 seeded random word arrays, mostly invalid: none may crash the validator, and the shape of whatever it accepts must be consistent
// with a recount of the words. Prints three summary lines.
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

// an accepted program: the shape against a recount of the code
static int exercise(bfhip_logup* lp, const std::vector<uint32_t>& code, size_t n_words, uint32_t n_cols, uint32_t n_params) {
    uint32_t s[8];
    if (bfhip_logup_shape(lp, s) != 0) return 1;
    uint32_t fracs = 0, ends = 0;
    for (size_t i = 0; i < n_words; i += 4) { fracs += code[i] == BFHIP_LOGUP_FRAC; ends += code[i] == BFHIP_LOGUP_END_COL; if (code[i] > BFHIP_LOGUP_END_COL) return 2; }
    if (s[0] != n_cols || s[1] != n_params || s[2] != ends || s[3] != fracs || s[4] != n_words / 4 || s[7] != 0) return 3;
    if (ends == 0 || ends > BFHIP_LOGUP_MAX_COLUMNS || fracs < ends || fracs > BFHIP_LOGUP_MAX_FRACTIONS) return 4;
    if (s[5] > BFHIP_AIR_MAX_M_REGS || s[6] == 0 || s[6] > BFHIP_AIR_MAX_Q_REGS) return 5;
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: logup_host_sanitize <programs.txt>\n"); return 2; }
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
        bfhip_logup* lp = nullptr;
        const int32_t rc = bfhip_logup_create(code.data(), code.size(), (uint32_t)n_cols, (uint32_t)n_params, &lp);
        if (rc == 0) {
            accepted++;
            if (!expect) unexpected++;
            const int e = exercise(lp, code, code.size(), (uint32_t)n_cols, (uint32_t)n_params);
            if (e) { printf("internal: exercise step %d: %s\n", e, g_error.c_str()); return 2; }
            if (bfhip_logup_destroy(lp) != 0) return 2;
        } else {
            refused++;
            if (expect || rc != -1 || g_error.find("bfhip_logup_create: instruction ") != 0) { unexpected++; printf("unexpected: %s\n", g_error.c_str()); }
        }
    }
    printf("listed: %d accepted, %d refused, %d unexpected\n", accepted, refused, unexpected);
    // random word arrays: a third fully random, the rest with small fields so that whole prefixes validate; towards the end of an array the
    // two logUp opcodes become likely, so that some arrays close their columns
    int r_acc = 0, r_ref = 0;
    for (int t = 0; t < 10000; t++) {
        const uint32_t n_words = t % 7 == 0 ? below(70) : 4 * (1 + below(16));
        const bool wild = t % 3 == 0;
        std::vector<uint32_t> code(n_words + 1);
        for (uint32_t i = 0; i < n_words; i++) {
            const uint32_t field = i % 4;
            if (wild) code[i] = below(5) == 0 ? (uint32_t)next64() : below(20);
            else if (field == 0) code[i] = i + 4 >= n_words ? 16 : below(3) == 0 ? 15 + below(2) : (i < 8 ? 7 : below(13));
            else if (field == 3) code[i] = below(9) == 0 ? (uint32_t)(-(int32_t)below(20)) : below(3);
            else code[i] = below(4);
        }
        const uint32_t n_cols = below(12), n_params = below(5);
        bfhip_logup* lp = nullptr;
        const int32_t rc = bfhip_logup_create(n_words ? code.data() : nullptr, n_words, n_cols, n_params, &lp);
        if (rc == 0) {
            r_acc++;
            const int e = exercise(lp, code, n_words, n_cols, n_params);
            if (e) { printf("internal: random program %d, exercise step %d\n", t, e); return 2; }
            bfhip_logup_destroy(lp);
        } else if (rc == -1) r_ref++;
        else { printf("internal: random program %d returned %d\n", t, rc); return 2; }
    }
    printf("random: %d accepted, %d refused of 10000\n", r_acc, r_ref);
    // edge calls: every one must be refused, none may read through a null pointer
    int edge_refused = 0, tried = 0;
    auto expect = [&](int32_t r) { tried++; if (r == -1) edge_refused++; };
    const uint32_t ok[12] = {7, 0, 0, 0, 15, 0, 0, 0, 16, 0, 0, 0};
    uint32_t out8[8];
    bfhip_logup* lp = nullptr;
    expect(bfhip_logup_create(nullptr, 12, 1, 1, &lp));
    expect(bfhip_logup_create(ok, 12, 1, 1, nullptr));
    expect(bfhip_logup_create(ok, 0, 1, 1, &lp));
    expect(bfhip_logup_create(ok, 11, 1, 1, &lp));
    expect(bfhip_logup_create(ok, 12, 1, 0, &lp));
    expect(bfhip_logup_shape(nullptr, out8));
    if (bfhip_logup_create(ok, 12, 1, 1, &lp) != 0) return 2;
    expect(bfhip_logup_shape(lp, nullptr));
    bfhip_logup_destroy(lp);
    if (bfhip_logup_destroy(nullptr) != 0) return 2;
    printf("edges refused %d of %d\n", edge_refused, tried);
    return unexpected == 0 && edge_refused == tried ? 0 : 3;
}
