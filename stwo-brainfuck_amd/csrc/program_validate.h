// The rules that bfhip_air_create, bfhip_logup_create and bfhip_relation_program_create share (include/bfhip.h states them), in one wording:
// the caps on a program's length, columns and parameters, and the M_* / Q_* opcodes with the registers they read and write. Each
// *_program_host.hip adds its family's own opcodes and its end-of-program rules. Host only, plain C++: no HIP type or call, so the sanitizer
// harnesses of tests/native compile it with the file that includes it.
#pragma once
#include "air_program.h"
#include <functional>
#include <stdexcept>

namespace bf {

struct ProgramRefusal : std::runtime_error { using std::runtime_error::runtime_error; };

// What a family allows beside the shared rules
struct ProgramFamily {
    const char* creator;          // the function that refuses: every message opens with its name
    const char* offset_refusal;   // null: offsets up to AIR_MAX_OFFSET; otherwise why the family reads offset 0 only
    const char* q_refusal;        // null: q registers and parameters; otherwise why the family has none
};

struct ProgramValidator {
    const ProgramFamily& family;
    const u32 n_cols, n_params;
    u32 n_m = 0, n_q = 0;                                    // registers in use: highest written + 1
    std::function<void(size_t, u32)> on_m_write;             // run on every write of an m register, after its range check
    bool m_written[AIR_MAX_M_REGS] = {}, q_written[AIR_MAX_Q_REGS] = {};

    [[noreturn]] void refuse(size_t instr, const std::string& rule) const {
        throw ProgramRefusal(std::string(family.creator) + ": instruction " + std::to_string(instr) + ": " + rule);
    }

    // The head of every *_create: what is refused before the first instruction is read
    ProgramValidator(const ProgramFamily& family_, size_t n_words, u32 n_cols_, u32 n_params_) : family(family_), n_cols(n_cols_), n_params(n_params_) {
        if (n_words == 0 || n_words % 4 != 0) refuse(n_words / 4, "the program is " + std::to_string(n_words) + " words, not a positive multiple of 4");
        if (n_words / 4 > AIR_MAX_INSTRUCTIONS) refuse(AIR_MAX_INSTRUCTIONS, "more than BFHIP_AIR_MAX_INSTRUCTIONS (4096) instructions");
        if (n_cols > AIR_MAX_COLUMNS) refuse(0, "more than BFHIP_AIR_MAX_COLUMNS (256) columns");
        if (n_params > AIR_MAX_PARAMS) refuse(0, "more than BFHIP_AIR_MAX_PARAMS (64) parameters");
    }

    void m_range(size_t i, u32 r) const { if (r >= AIR_MAX_M_REGS) refuse(i, "m register " + std::to_string(r) + " out of range (BFHIP_AIR_MAX_M_REGS = 96)"); }
    void q_range(size_t i, u32 r) const { if (r >= AIR_MAX_Q_REGS) refuse(i, "q register " + std::to_string(r) + " out of range (BFHIP_AIR_MAX_Q_REGS = 24)"); }
    void m_dst(size_t i, u32 r) { m_range(i, r); if (on_m_write) on_m_write(i, r); m_written[r] = true; if (r + 1 > n_m) n_m = r + 1; }
    void q_dst(size_t i, u32 r) { q_range(i, r); q_written[r] = true; if (r + 1 > n_q) n_q = r + 1; }
    void m_src(size_t i, u32 r) const { m_range(i, r); if (!m_written[r]) refuse(i, "m register " + std::to_string(r) + " is read before it is written"); }
    void q_src(size_t i, u32 r) const { q_range(i, r); if (!q_written[r]) refuse(i, "q register " + std::to_string(r) + " is read before it is written"); }
    void column(size_t i, u32 col, u32 width, u32 off_word) const {
        if (col >= n_cols || width > n_cols - col) refuse(i, "column " + std::to_string(col) + (width > 1 ? ".." + std::to_string((uint64_t)col + width - 1) : std::string()) + " out of range (the program has " + std::to_string(n_cols) + " columns)");
        const int32_t off = (int32_t)off_word;
        if (family.offset_refusal) { if (off) refuse(i, "offset " + std::to_string(off) + ": " + family.offset_refusal); }
        else if (off < -AIR_MAX_OFFSET || off > AIR_MAX_OFFSET) refuse(i, "offset " + std::to_string(off) + " out of range (|offset| <= 16)");
    }

    // One M_* / Q_* instruction. False: the opcode is not one of them, and the family's own switch decides.
    bool shared(size_t i, u32 op, u32 dst, u32 a, u32 b) {
        static const char* const Q_NAMES[] = {"Q_COL", "Q_PARAM", "Q_FROM_M", "Q_ADD", "Q_SUB", "Q_MUL", "Q_MULM"};
        if (op >= AIR_Q_COL && op <= AIR_Q_MULM && family.q_refusal) refuse(i, std::string(Q_NAMES[op - AIR_Q_COL]) + ": " + family.q_refusal);
        switch (op) {
            case AIR_M_COL: column(i, a, 1, b); m_dst(i, dst); return true;
            case AIR_M_CONST: if (a >= P31) refuse(i, "constant " + std::to_string(a) + " is not a canonical M31 (v < 2^31 - 1)"); m_dst(i, dst); return true;
            case AIR_M_ADD: case AIR_M_SUB: case AIR_M_MUL: m_src(i, a); m_src(i, b); m_dst(i, dst); return true;
            case AIR_M_NEG: m_src(i, a); m_dst(i, dst); return true;
            case AIR_Q_COL: column(i, a, 4, b); q_dst(i, dst); return true;
            case AIR_Q_PARAM: if (a >= n_params) refuse(i, "parameter " + std::to_string(a) + " out of range (the program has " + std::to_string(n_params) + " parameters)"); q_dst(i, dst); return true;
            case AIR_Q_FROM_M: m_src(i, a); q_dst(i, dst); return true;
            case AIR_Q_ADD: case AIR_Q_SUB: case AIR_Q_MUL: q_src(i, a); q_src(i, b); q_dst(i, dst); return true;
            case AIR_Q_MULM: q_src(i, a); m_src(i, b); q_dst(i, dst); return true;
            default: return false;
        }
    }
};

}  // namespace bf
