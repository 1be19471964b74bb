// CPU sanitizer harness for the host-only half of the witness programs (stwo-brainfuck_amd/csrc/witness_program_host.hip:
// bfhip_witness_program_create, _shape, _eval_table, _destroy). tests/test_witness_program_cpu.py compiles this file TOGETHER with
// witness_program_host.hip (as C++: the file makes no HIP call) under g++ -fsanitize=address,undefined and runs the program directly:
//   witness_host_sanitize <programs.txt>
// programs.txt: one program per line, "<expected: 1 accepted / 0 refused> <n_cols> <n_out> <n_args> <word> <word> ...". After the listed
// programs come 10 000 seeded random word arrays, many invalid: none may crash the validator, whatever it accepts is evaluated over whole
// tables with exactly fitting buffers (bfhip_witness_program_eval_table at log_size 1 and 3: offsets up to 16 wrap both) and its shape must
// be consistent with a recount of the words. Prints three summary lines.
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

// an accepted program: the shape against a recount of the code, then whole tables through the evaluator with exactly fitting buffers
static int exercise(bfhip_witness_program* wp, const std::vector<uint32_t>& code, size_t n_words, uint32_t n_cols, uint32_t n_out, uint32_t n_args) {
    uint32_t s[8];
    if (bfhip_witness_program_shape(wp, s) != 0) return 1;
    uint32_t stores = 0;
    int32_t lo = 0, hi = 0;
    for (size_t i = 0; i < n_words; i += 4) {
        stores += code[i] == BFHIP_WIT_STORE;
        if (code[i] > BFHIP_WIT_STORE || (code[i] >= 6 && code[i] < BFHIP_WIT_ARG)) return 2;
        if (code[i] == 0) { const int32_t off = (int32_t)code[i + 3]; if (off < lo) lo = off; if (off > hi) hi = off; }
    }
    if (s[0] != n_cols || s[1] != n_out || s[2] != n_args || s[3] != n_words / 4 || (int32_t)s[5] != lo || (int32_t)s[6] != hi || s[7]) return 3;
    if (stores != n_out || s[4] == 0 || s[4] > BFHIP_AIR_MAX_M_REGS || lo < -BFHIP_AIR_MAX_OFFSET || hi > BFHIP_AIR_MAX_OFFSET) return 4;
    std::vector<uint32_t> args(n_args);
    for (auto& v : args) v = below(3) == 0 ? 0x7ffffffeu : below(9);
    for (uint32_t log_size : {1u, 3u}) {
        const size_t n = (size_t)1 << log_size;
        std::vector<uint32_t> table(n * n_cols), out(n * n_out, 0xffffffffu);
        for (auto& v : table) v = below(3) == 0 ? 0x7ffffffeu : below(5);
        if (bfhip_witness_program_eval_table(wp, log_size, table.data(), args.data(), n_args, out.data()) != 0) return 5;
        for (uint32_t v : out) if (v >= 0x7fffffffu) return 6;      // every output stored, every value canonical
        if (n_args && bfhip_witness_program_eval_table(wp, log_size, table.data(), args.data(), n_args - 1, out.data()) != -1) return 7;
        if (n_cols) {
            table[n * n_cols - 1] = 0x7fffffffu;      // not canonical: refused, nothing read or written past the buffers
            if (bfhip_witness_program_eval_table(wp, log_size, table.data(), args.data(), n_args, out.data()) != -1) return 8;
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: witness_host_sanitize <programs.txt>\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    int accepted = 0, refused = 0, unexpected = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        uint64_t expect, n_cols, n_out, n_args, w;
        ss >> expect >> n_cols >> n_out >> n_args;
        std::vector<uint32_t> code;
        while (ss >> w) code.push_back((uint32_t)w);
        const size_t n_words = code.size();
        code.resize(n_words + 1);      // a readable array even for an empty program
        bfhip_witness_program* wp = nullptr;
        const int32_t rc = bfhip_witness_program_create(code.data(), n_words, (uint32_t)n_cols, (uint32_t)n_out, (uint32_t)n_args, &wp);
        if (rc == 0) {
            accepted++;
            if (!expect) unexpected++;
            const int e = exercise(wp, code, n_words, (uint32_t)n_cols, (uint32_t)n_out, (uint32_t)n_args);
            if (e) { printf("internal: exercise step %d: %s\n", e, g_error.c_str()); return 2; }
            if (bfhip_witness_program_destroy(wp) != 0) return 2;
        } else {
            refused++;
            if (expect || rc != -1 || g_error.find("bfhip_witness_program_create: instruction ") != 0) { unexpected++; printf("unexpected: %s\n", g_error.c_str()); }
        }
    }
    printf("listed: %d accepted, %d refused, %d unexpected\n", accepted, refused, unexpected);
    // random word arrays: a third fully random, the rest with small fields so that whole prefixes validate; the own opcodes are likely, the
    // first instruction writes register 0 and the last instructions store the outputs in order, so that many arrays are whole programs
    int r_acc = 0, r_ref = 0;
    for (int t = 0; t < 10000; t++) {
        const uint32_t n_out = 1 + below(3);
        const uint32_t n_words = t % 7 == 0 ? below(70) : 4 * (1 + n_out + below(14));
        const bool wild = t % 3 == 0;
        std::vector<uint32_t> code(n_words + 1);
        for (uint32_t i = 0; i < n_words; i++) {
            const uint32_t field = i % 4, instr = i / 4, n_instr = n_words / 4;
            const bool tail = instr + n_out >= n_instr;      // the last n_out instructions
            if (wild) code[i] = below(5) == 0 ? (uint32_t)next64() : below(28);
            else if (field == 0) code[i] = tail ? 26 : instr == 0 ? 1 : below(2) == 0 ? 19 + below(7) : below(6);
            else if (field == 1) code[i] = tail ? instr + n_out - n_instr : instr == 0 ? 0 : below(4);
            else if (field == 3) code[i] = below(9) == 0 ? (uint32_t)(-(int32_t)below(20)) : below(3);
            else code[i] = tail || below(3) ? 0 : below(4);
        }
        const uint32_t n_cols = below(12), n_args = below(4);
        bfhip_witness_program* wp = nullptr;
        const int32_t rc = bfhip_witness_program_create(n_words ? code.data() : nullptr, n_words, n_cols, n_out, n_args, &wp);
        if (rc == 0) {
            r_acc++;
            const int e = exercise(wp, code, n_words, n_cols, n_out, n_args);
            if (e) { printf("internal: random program %d, exercise step %d: %s\n", t, e, g_error.c_str()); return 2; }
            bfhip_witness_program_destroy(wp);
        } else if (rc == -1) r_ref++;
        else { printf("internal: random program %d returned %d\n", t, rc); return 2; }
    }
    printf("random: %d accepted, %d refused of 10000\n", r_acc, r_ref);
    // edge calls: every one must be refused, none may read through a null pointer
    int edge_refused = 0, tried = 0;
    auto expect = [&](int32_t r) { tried++; if (r == -1) edge_refused++; };
    const uint32_t ok[8] = {1, 0, 5, 0, 26, 0, 0, 0}, table[2] = {3, 4}, arg[1] = {1};
    uint32_t out8[8], out[2] = {9, 9};
    bfhip_witness_program* wp = nullptr;
    expect(bfhip_witness_program_create(nullptr, 8, 1, 1, 0, &wp));
    expect(bfhip_witness_program_create(ok, 8, 1, 1, 0, nullptr));
    expect(bfhip_witness_program_create(ok, 0, 1, 1, 0, &wp));
    expect(bfhip_witness_program_create(ok, 7, 1, 1, 0, &wp));
    expect(bfhip_witness_program_create(ok, 8, 1, 0, 0, &wp));
    expect(bfhip_witness_program_create(ok, 8, 1, 257, 0, &wp));
    expect(bfhip_witness_program_create(ok, 8, 1, 1, 65, &wp));
    expect(bfhip_witness_program_shape(nullptr, out8));
    expect(bfhip_witness_program_eval_table(nullptr, 1, table, nullptr, 0, out));
    if (bfhip_witness_program_create(ok, 8, 1, 1, 0, &wp) != 0) return 2;
    expect(bfhip_witness_program_shape(wp, nullptr));
    expect(bfhip_witness_program_eval_table(wp, 1, nullptr, nullptr, 0, out));
    expect(bfhip_witness_program_eval_table(wp, 1, table, nullptr, 0, nullptr));
    expect(bfhip_witness_program_eval_table(wp, 1, table, nullptr, 1, out));
    expect(bfhip_witness_program_eval_table(wp, 1, table, arg, 1, out));
    expect(bfhip_witness_program_eval_table(wp, 0, table, nullptr, 0, out));
    expect(bfhip_witness_program_eval_table(wp, 31, table, nullptr, 0, out));
    if (out[0] != 9 || out[1] != 9) return 2;
    if (bfhip_witness_program_eval_table(wp, 1, table, nullptr, 0, out) != 0 || out[0] != 5 || out[1] != 5) return 2;
    bfhip_witness_program_destroy(wp);
    if (bfhip_witness_program_destroy(nullptr) != 0) return 2;
    printf("edges refused %d of %d\n", edge_refused, tried);
    return unexpected == 0 && edge_refused == tried ? 0 : 3;
}
