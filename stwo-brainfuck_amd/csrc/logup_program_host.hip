// The host-only half of the fraction program (include/bfhip.h "Fraction programs"): the validator behind bfhip_logup_create and the shape.
// No GPU, no HIP call: this file also compiles with a plain C++ compiler, which is how tests/native/logup_host_sanitize.cpp puts it under the
// sanitizers. The kernels that run a program on the trace domain are in logup_program.hip.
#include "api_guard.h"
#include "logup_program.h"

using namespace bf;

namespace {

struct Refusal : HipError { using HipError::HipError; };
[[noreturn]] void refuse(size_t instr, const std::string& rule) { throw Refusal("bfhip_logup_create: instruction " + std::to_string(instr) + ": " + rule); }

// One pass over the code: the rules of bfhip_air_create (in its words) without constraints and offsets, plus the column structure.
void validate(bfhip_logup& lp) {
    const size_t n = lp.n_instr;
    bool m_written[AIR_MAX_M_REGS] = {}, q_written[AIR_MAX_Q_REGS] = {};
    auto m_dst = [&](size_t i, u32 r) { if (r >= AIR_MAX_M_REGS) refuse(i, "m register " + std::to_string(r) + " out of range (BFHIP_AIR_MAX_M_REGS = 96)"); m_written[r] = true; if (r + 1 > lp.n_m) lp.n_m = r + 1; };
    auto q_dst = [&](size_t i, u32 r) { if (r >= AIR_MAX_Q_REGS) refuse(i, "q register " + std::to_string(r) + " out of range (BFHIP_AIR_MAX_Q_REGS = 24)"); q_written[r] = true; if (r + 1 > lp.n_q) lp.n_q = r + 1; };
    auto m_src = [&](size_t i, u32 r) {
        if (r >= AIR_MAX_M_REGS) refuse(i, "m register " + std::to_string(r) + " out of range (BFHIP_AIR_MAX_M_REGS = 96)");
        if (!m_written[r]) refuse(i, "m register " + std::to_string(r) + " is read before it is written");
    };
    auto q_src = [&](size_t i, u32 r) {
        if (r >= AIR_MAX_Q_REGS) refuse(i, "q register " + std::to_string(r) + " out of range (BFHIP_AIR_MAX_Q_REGS = 24)");
        if (!q_written[r]) refuse(i, "q register " + std::to_string(r) + " is read before it is written");
    };
    auto column = [&](size_t i, u32 col, u32 width, u32 off_word) {
        if (col >= lp.n_cols || width > lp.n_cols - col) refuse(i, "column " + std::to_string(col) + (width > 1 ? ".." + std::to_string((uint64_t)col + width - 1) : std::string()) + " out of range (the program has " + std::to_string(lp.n_cols) + " columns)");
        if (off_word) refuse(i, "offset " + std::to_string((int32_t)off_word) + ": a fraction program reads a row's own cells (offset 0 only)");
    };
    u32 open_fracs = 0;      // fractions of the open logUp column
    for (size_t i = 0; i < n; i++) {
        const u32 op = lp.code[4 * i], dst = lp.code[4 * i + 1], a = lp.code[4 * i + 2], b = lp.code[4 * i + 3];
        switch (op) {
            case AIR_M_COL: column(i, a, 1, b); m_dst(i, dst); break;
            case AIR_M_CONST: if (a >= P31) refuse(i, "constant " + std::to_string(a) + " is not a canonical M31 (v < 2^31 - 1)"); m_dst(i, dst); break;
            case AIR_M_ADD: case AIR_M_SUB: case AIR_M_MUL: m_src(i, a); m_src(i, b); m_dst(i, dst); break;
            case AIR_M_NEG: m_src(i, a); m_dst(i, dst); break;
            case AIR_Q_COL: column(i, a, 4, b); q_dst(i, dst); break;
            case AIR_Q_PARAM: if (a >= lp.n_params) refuse(i, "parameter " + std::to_string(a) + " out of range (the program has " + std::to_string(lp.n_params) + " parameters)"); q_dst(i, dst); break;
            case AIR_Q_FROM_M: m_src(i, a); q_dst(i, dst); break;
            case AIR_Q_ADD: case AIR_Q_SUB: case AIR_Q_MUL: q_src(i, a); q_src(i, b); q_dst(i, dst); break;
            case AIR_Q_MULM: q_src(i, a); m_src(i, b); q_dst(i, dst); break;
            case AIR_C_BASE: refuse(i, "C_BASE: a fraction program has no constraints");
            case AIR_C_EXT: refuse(i, "C_EXT: a fraction program has no constraints");
            case LOGUP_FRAC:
                q_src(i, a); q_src(i, b);
                if (lp.n_fractions == LOGUP_MAX_FRACTIONS) refuse(i, "FRAC: more than BFHIP_LOGUP_MAX_FRACTIONS (32) fractions");
                if (open_fracs == 0 && lp.n_logup_cols == LOGUP_MAX_COLUMNS) refuse(i, "FRAC: more than BFHIP_LOGUP_MAX_COLUMNS (8) logUp columns");
                lp.n_fractions++; open_fracs++;
                break;
            case LOGUP_END_COL:
                if (open_fracs == 0) refuse(i, "END_COL: no fraction since the previous END_COL (a logUp column has at least one FRAC)");
                lp.n_logup_cols++; open_fracs = 0;
                break;
            default: refuse(i, "unknown opcode " + std::to_string(op));
        }
    }
    if (open_fracs) refuse(n, "the program ends inside a logUp column (a FRAC that no END_COL follows)");
    if (lp.n_logup_cols == 0) refuse(n, "the program ends without a logUp column (at least one FRAC and its END_COL)");
}

}  // namespace

extern "C" {

int32_t bfhip_logup_create(const uint32_t* code, size_t n_words, uint32_t n_cols, uint32_t n_params, bfhip_logup** out) {
    API_TRY
    if (!code || !out) throw HipError("null argument");
    if (n_words == 0 || n_words % 4 != 0) refuse(n_words / 4, "the program is " + std::to_string(n_words) + " words, not a positive multiple of 4");
    if (n_words / 4 > AIR_MAX_INSTRUCTIONS) refuse(AIR_MAX_INSTRUCTIONS, "more than BFHIP_AIR_MAX_INSTRUCTIONS (4096) instructions");
    if (n_cols > AIR_MAX_COLUMNS) refuse(0, "more than BFHIP_AIR_MAX_COLUMNS (256) columns");
    if (n_params > AIR_MAX_PARAMS) refuse(0, "more than BFHIP_AIR_MAX_PARAMS (64) parameters");
    auto* lp = new bfhip_logup();
    try {
        lp->code.assign(code, code + n_words);
        lp->n_instr = (u32)(n_words / 4); lp->n_cols = n_cols; lp->n_params = n_params;
        validate(*lp);
    } catch (...) { delete lp; throw; }
    *out = lp;
    return 0;
    API_CATCH
}
int32_t bfhip_logup_destroy(bfhip_logup* lp) { API_TRY delete lp; return 0; API_CATCH }

int32_t bfhip_logup_shape(const bfhip_logup* lp, uint32_t out[8]) {
    API_TRY
    if (!lp || !out) throw HipError("null argument");
    const u32 v[8] = {lp->n_cols, lp->n_params, lp->n_logup_cols, lp->n_fractions, lp->n_instr, lp->n_m, lp->n_q, 0};
    memcpy(out, v, sizeof v);
    return 0;
    API_CATCH
}

}  // extern "C"
