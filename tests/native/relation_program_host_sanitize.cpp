// CPU sanitizer harness for the host-only half of the relation programs (stwo-brainfuck_amd/csrc/relation_program_host.hip:
// bfhip_relation_program_create, _shape, _eval_row, _destroy). tests/test_relation_program_cpu.py compiles this file TOGETHER with
// relation_program_host.hip (as C++: the file makes no HIP call) under g++ -fsanitize=address,undefined and runs the program directly:
//   relation_program_host_sanitize <programs.txt>
// programs.txt: one program per line, "<expected: 1 accepted / 0 refused> <n_cols> <n_relations> <width> ... <word> <word> ...". After the
// listed programs come 10 000 seeded random word arrays, mostly invalid: none may crash the validator, whatever it accepts is evaluated on
// a row (bfhip_relation_program_eval_row) and its shape must be consistent with a recount of the words. Prints three summary lines.
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

// an accepted program: the shape against a recount of the code, then one row through the evaluator with exactly fitting buffers
static int exercise(bfhip_relation_program* rp, const std::vector<uint32_t>& code, size_t n_words, uint32_t n_cols, const std::vector<uint32_t>& widths) {
    uint32_t s[8];
    if (bfhip_relation_program_shape(rp, s) != 0) return 1;
    uint32_t entries = 0, words = 0;
    for (size_t i = 0; i < n_words; i += 4) { entries += code[i] == BFHIP_REL_ENTRY; words += code[i] == BFHIP_REL_WORD; if (code[i] > BFHIP_REL_ENTRY) return 2; }
    if (s[0] != n_cols || s[1] != widths.size() || s[2] != entries || s[3] != n_words / 4 || s[5] || s[6] || s[7]) return 3;
    if (entries == 0 || entries > BFHIP_RELATION_PROGRAM_MAX_ENTRIES || s[4] == 0 || s[4] > BFHIP_AIR_MAX_M_REGS) return 4;
    std::vector<uint32_t> row(n_cols);
    for (auto& v : row) v = below(3) == 0 ? 0x7ffffffeu : below(5);
    uint32_t n = 0;
    if (bfhip_relation_program_eval_row(rp, row.data(), nullptr, nullptr, nullptr, 0, &n) != 0 || n != entries) return 5;
    std::vector<uint32_t> rel(n), mult(n), tup(7 * (size_t)n);
    if (n > 1 && bfhip_relation_program_eval_row(rp, row.data(), rel.data(), mult.data(), tup.data(), n - 1, &n) != -2) return 6;
    if (bfhip_relation_program_eval_row(rp, row.data(), rel.data(), mult.data(), tup.data(), n, &n) != 0) return 7;
    uint32_t width_sum = 0;
    for (uint32_t e = 0; e < n; e++) {
        if (rel[e] >= widths.size() || mult[e] >= 0x7fffffffu) return 8;
        for (uint32_t k = 0; k < 7; k++) if (tup[7 * e + k] >= 0x7fffffffu || (k >= widths[rel[e]] && tup[7 * e + k] != 0)) return 9;
        width_sum += widths[rel[e]];
    }
    if (width_sum != words) return 10;
    row.assign(n_cols, 0x7fffffffu);      // not canonical: refused, nothing written past the buffers
    if (n_cols && bfhip_relation_program_eval_row(rp, row.data(), rel.data(), mult.data(), tup.data(), n, &n) != -1) return 11;
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: relation_program_host_sanitize <programs.txt>\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    int accepted = 0, refused = 0, unexpected = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        uint64_t expect, n_cols, n_rel, w;
        ss >> expect >> n_cols >> n_rel;
        std::vector<uint32_t> widths, code;
        for (uint64_t r = 0; r < n_rel && (ss >> w); r++) widths.push_back((uint32_t)w);
        while (ss >> w) code.push_back((uint32_t)w);
        std::vector<uint32_t> widths_arg = widths;
        widths_arg.resize(widths.size() + 1);      // a readable array even for n_relations 0
        bfhip_relation_program* rp = nullptr;
        const int32_t rc = bfhip_relation_program_create(code.data(), code.size(), (uint32_t)n_cols, widths_arg.data(), (uint32_t)n_rel, &rp);
        if (rc == 0) {
            accepted++;
            if (!expect) unexpected++;
            const int e = exercise(rp, code, code.size(), (uint32_t)n_cols, widths);
            if (e) { printf("internal: exercise step %d: %s\n", e, g_error.c_str()); return 2; }
            if (bfhip_relation_program_destroy(rp) != 0) return 2;
        } else {
            refused++;
            if (expect || rc != -1 || g_error.find("bfhip_relation_program_create: instruction ") != 0) { unexpected++; printf("unexpected: %s\n", g_error.c_str()); }
        }
    }
    printf("listed: %d accepted, %d refused, %d unexpected\n", accepted, refused, unexpected);
    // random word arrays: a third fully random, the rest with small fields so that whole prefixes validate; the two relation opcodes are
    // likely, and the last instruction is an ENTRY, so that some arrays close their tuples at the right width
    int r_acc = 0, r_ref = 0;
    for (int t = 0; t < 10000; t++) {
        const uint32_t n_words = t % 7 == 0 ? below(70) : 4 * (1 + below(16));
        const bool wild = t % 3 == 0;
        std::vector<uint32_t> code(n_words + 1);
        for (uint32_t i = 0; i < n_words; i++) {
            const uint32_t field = i % 4;
            if (wild) code[i] = below(5) == 0 ? (uint32_t)next64() : below(20);
            else if (field == 0) code[i] = i + 4 >= n_words ? 18 : below(3) == 0 ? 17 + below(2) : (i < 8 ? 1 : below(6));
            else if (field == 3) code[i] = below(9) == 0 ? (uint32_t)(-(int32_t)below(20)) : below(3);
            else code[i] = below(4);
        }
        const uint32_t n_cols = below(12), n_rel = 1 + below(3);
        std::vector<uint32_t> widths(n_rel);
        for (auto& v : widths) v = 1 + below(2);
        bfhip_relation_program* rp = nullptr;
        const int32_t rc = bfhip_relation_program_create(n_words ? code.data() : nullptr, n_words, n_cols, widths.data(), n_rel, &rp);
        if (rc == 0) {
            r_acc++;
            const int e = exercise(rp, code, n_words, n_cols, widths);
            if (e) { printf("internal: random program %d, exercise step %d\n", t, e); return 2; }
            bfhip_relation_program_destroy(rp);
        } else if (rc == -1) r_ref++;
        else { printf("internal: random program %d returned %d\n", t, rc); return 2; }
    }
    printf("random: %d accepted, %d refused of 10000\n", r_acc, r_ref);
    // edge calls: every one must be refused, none may read through a null pointer
    int edge_refused = 0, tried = 0;
    auto expect = [&](int32_t r) { tried++; if (r == -1) edge_refused++; };
    const uint32_t ok[12] = {1, 0, 5, 0, 17, 0, 0, 0, 18, 0, 0, 0}, one[1] = {1}, col[1] = {3};
    uint32_t out8[8], n = 0, rel[1], mult[1], tup[7];
    bfhip_relation_program* rp = nullptr;
    expect(bfhip_relation_program_create(nullptr, 12, 1, one, 1, &rp));
    expect(bfhip_relation_program_create(ok, 12, 1, nullptr, 1, &rp));
    expect(bfhip_relation_program_create(ok, 12, 1, one, 1, nullptr));
    expect(bfhip_relation_program_create(ok, 0, 1, one, 1, &rp));
    expect(bfhip_relation_program_create(ok, 11, 1, one, 1, &rp));
    expect(bfhip_relation_program_create(ok, 12, 1, one, 0, &rp));
    expect(bfhip_relation_program_create(ok, 12, 1, one, 17, &rp));
    expect(bfhip_relation_program_shape(nullptr, out8));
    expect(bfhip_relation_program_eval_row(nullptr, col, rel, mult, tup, 1, &n));
    if (bfhip_relation_program_create(ok, 12, 1, one, 1, &rp) != 0) return 2;
    expect(bfhip_relation_program_shape(rp, nullptr));
    expect(bfhip_relation_program_eval_row(rp, nullptr, rel, mult, tup, 1, &n));
    expect(bfhip_relation_program_eval_row(rp, col, rel, mult, tup, 1, nullptr));
    expect(bfhip_relation_program_eval_row(rp, col, nullptr, mult, tup, 1, &n));
    expect(bfhip_relation_program_eval_row(rp, col, rel, nullptr, tup, 1, &n));
    expect(bfhip_relation_program_eval_row(rp, col, rel, mult, nullptr, 1, &n));
    if (bfhip_relation_program_eval_row(rp, col, rel, mult, tup, 1, &n) != 0 || n != 1 || rel[0] != 0 || mult[0] != 5 || tup[0] != 5 || tup[6] != 0) return 2;
    bfhip_relation_program_destroy(rp);
    if (bfhip_relation_program_destroy(nullptr) != 0) return 2;
    printf("edges refused %d of %d\n", edge_refused, tried);
    return unexpected == 0 && edge_refused == tried ? 0 : 3;
}
