// The host-only half of the constraint program (include/bfhip.h "Constraint programs"): the validator behind bfhip_air_create, the mask,
// and the out-of-domain evaluator — stwo's PointEvaluator run over a program instead of over a compiled `FrameworkEval::evaluate`. No GPU,
// no HIP call: this file also compiles with a plain C++ compiler, which is how tests/native/air_host_sanitize.cpp puts it under the
// sanitizers. The domain evaluator (the gfx950 kernel) is air_program.hip.
#include "api_guard.h"
#include "pcs_types.h"
#include "air_program.h"

using namespace bf;

namespace {

struct Refusal : HipError { using HipError::HipError; };
[[noreturn]] void refuse(size_t instr, const std::string& rule) { throw Refusal("bfhip_air_create: instruction " + std::to_string(instr) + ": " + rule); }

const char* op_name(u32 op) {
    static const char* names[AIR_N_OPS] = {"M_COL", "M_CONST", "M_ADD", "M_SUB", "M_MUL", "M_NEG", "Q_COL", "Q_PARAM", "Q_FROM_M", "Q_ADD", "Q_SUB", "Q_MUL", "Q_MULM",
                                           "C_BASE", "C_EXT"};
    return op < AIR_N_OPS ? names[op] : "?";
}

// One pass over the code: every rule of include/bfhip.h, the register counts, the offsets and the mask.
void validate(bfhip_air& air) {
    const size_t n = air.n_instr;
    bool m_written[AIR_MAX_M_REGS] = {}, q_written[AIR_MAX_Q_REGS] = {};
    std::vector<std::vector<int32_t>> offs(air.n_cols);      // per column: its offsets in order of first use
    air.col_read_shifted.assign(air.n_cols, 0);
    auto m_dst = [&](size_t i, u32 r) { if (r >= AIR_MAX_M_REGS) refuse(i, "m register " + std::to_string(r) + " out of range (BFHIP_AIR_MAX_M_REGS = 96)"); m_written[r] = true; if (r + 1 > air.n_m) air.n_m = r + 1; };
    auto q_dst = [&](size_t i, u32 r) { if (r >= AIR_MAX_Q_REGS) refuse(i, "q register " + std::to_string(r) + " out of range (BFHIP_AIR_MAX_Q_REGS = 24)"); q_written[r] = true; if (r + 1 > air.n_q) air.n_q = r + 1; };
    auto m_src = [&](size_t i, u32 r) {
        if (r >= AIR_MAX_M_REGS) refuse(i, "m register " + std::to_string(r) + " out of range (BFHIP_AIR_MAX_M_REGS = 96)");
        if (!m_written[r]) refuse(i, "m register " + std::to_string(r) + " is read before it is written");
    };
    auto q_src = [&](size_t i, u32 r) {
        if (r >= AIR_MAX_Q_REGS) refuse(i, "q register " + std::to_string(r) + " out of range (BFHIP_AIR_MAX_Q_REGS = 24)");
        if (!q_written[r]) refuse(i, "q register " + std::to_string(r) + " is read before it is written");
    };
    auto column = [&](size_t i, u32 col, u32 width, u32 off_word) {
        if (col >= air.n_cols || width > air.n_cols - col) refuse(i, "column " + std::to_string(col) + (width > 1 ? ".." + std::to_string((uint64_t)col + width - 1) : std::string()) + " out of range (the program has " + std::to_string(air.n_cols) + " columns)");
        const int32_t off = (int32_t)off_word;
        if (off < -AIR_MAX_OFFSET || off > AIR_MAX_OFFSET) refuse(i, "offset " + std::to_string(off) + " out of range (|offset| <= 16)");
        if (off < air.min_off) air.min_off = off;
        if (off > air.max_off) air.max_off = off;
        for (u32 c = col; c < col + width; c++) {
            if (off) air.col_read_shifted[c] = 1;
            bool seen = false;
            for (int32_t o : offs[c]) seen = seen || o == off;
            if (!seen) offs[c].push_back(off);
        }
    };
    for (size_t i = 0; i < n; i++) {
        const u32 op = air.code[4 * i], dst = air.code[4 * i + 1], a = air.code[4 * i + 2], b = air.code[4 * i + 3];
        switch (op) {
            case AIR_M_COL: column(i, a, 1, b); m_dst(i, dst); break;
            case AIR_M_CONST: if (a >= P31) refuse(i, "constant " + std::to_string(a) + " is not a canonical M31 (v < 2^31 - 1)"); m_dst(i, dst); break;
            case AIR_M_ADD: case AIR_M_SUB: case AIR_M_MUL: m_src(i, a); m_src(i, b); m_dst(i, dst); break;
            case AIR_M_NEG: m_src(i, a); m_dst(i, dst); break;
            case AIR_Q_COL: column(i, a, 4, b); q_dst(i, dst); break;
            case AIR_Q_PARAM: if (a >= air.n_params) refuse(i, "parameter " + std::to_string(a) + " out of range (the program has " + std::to_string(air.n_params) + " parameters)"); q_dst(i, dst); break;
            case AIR_Q_FROM_M: m_src(i, a); q_dst(i, dst); break;
            case AIR_Q_ADD: case AIR_Q_SUB: case AIR_Q_MUL: q_src(i, a); q_src(i, b); q_dst(i, dst); break;
            case AIR_Q_MULM: q_src(i, a); m_src(i, b); q_dst(i, dst); break;
            case AIR_C_BASE: m_src(i, a); break;
            case AIR_C_EXT: q_src(i, a); break;
            default: refuse(i, "unknown opcode " + std::to_string(op));
        }
        if (op == AIR_C_BASE || op == AIR_C_EXT) {
            if (air.n_constraints == AIR_MAX_CONSTRAINTS) refuse(i, std::string(op_name(op)) + ": more than BFHIP_AIR_MAX_CONSTRAINTS (64) constraints");
            air.n_constraints++;
        }
    }
    if (air.n_constraints == 0) refuse(n, "the program ends without a constraint (at least one C_BASE or C_EXT)");
    air.mask_first.assign(air.n_cols + 1, 0);
    for (u32 c = 0; c < air.n_cols; c++) {
        air.mask_first[c] = (u32)air.mask_cols.size();
        for (int32_t o : offs[c]) { air.mask_cols.push_back(c); air.mask_offs.push_back(o); }
    }
    air.mask_first[air.n_cols] = (u32)air.mask_cols.size();
}

}  // namespace

extern "C" {

int32_t bfhip_air_create(const uint32_t* code, size_t n_words, uint32_t n_cols, uint32_t n_params, bfhip_air** out) {
    API_TRY
    if (!code || !out) throw HipError("null argument");
    if (n_words == 0 || n_words % 4 != 0) refuse(n_words / 4, "the program is " + std::to_string(n_words) + " words, not a positive multiple of 4");
    if (n_words / 4 > AIR_MAX_INSTRUCTIONS) refuse(AIR_MAX_INSTRUCTIONS, "more than BFHIP_AIR_MAX_INSTRUCTIONS (4096) instructions");
    if (n_cols > AIR_MAX_COLUMNS) refuse(0, "more than BFHIP_AIR_MAX_COLUMNS (256) columns");
    if (n_params > AIR_MAX_PARAMS) refuse(0, "more than BFHIP_AIR_MAX_PARAMS (64) parameters");
    auto* air = new bfhip_air();
    try {
        air->code.assign(code, code + n_words);
        air->n_instr = (u32)(n_words / 4); air->n_cols = n_cols; air->n_params = n_params;
        validate(*air);
    } catch (...) { delete air; throw; }
    *out = air;
    return 0;
    API_CATCH
}
int32_t bfhip_air_destroy(bfhip_air* air) { API_TRY delete air; return 0; API_CATCH }

int32_t bfhip_air_shape(const bfhip_air* air, uint32_t out[8]) {
    API_TRY
    if (!air || !out) throw HipError("null argument");
    const u32 v[8] = {air->n_cols, air->n_params, air->n_constraints, air->n_instr, air->n_m, air->n_q, (u32)air->min_off, (u32)air->max_off};
    memcpy(out, v, sizeof v);
    return 0;
    API_CATCH
}

int32_t bfhip_air_mask(const bfhip_air* air, uint32_t* cols_out, int32_t* offs_out, uint32_t cap, uint32_t* n) {
    API_TRY
    if (!air || !n) throw HipError("null argument");
    *n = (u32)air->mask_cols.size();
    if (!cols_out && !offs_out && cap == 0) return 0;      // size query
    if (cap < *n) { bfhip_set_error("bfhip_air_mask: capacity"); return -2; }
    if (!cols_out || !offs_out) throw HipError("null argument");
    for (u32 i = 0; i < *n; i++) { cols_out[i] = air->mask_cols[i]; offs_out[i] = air->mask_offs[i]; }
    return 0;
    API_CATCH
}

// stwo's PointEvaluator over the program: both register files hold QM31 values, a mask entry is the column's sampled value at
// point + off * CanonicCoset(log_size).step(), a Q_COL combines its four coordinates' samples (SecureField::from_partial_evals, what
// `combine_ef` does at a point), and the weighted sum is divided by coset_vanishing(CanonicCoset(log_size).coset, point).
int32_t bfhip_air_eval_at_point(const bfhip_air* air, uint32_t log_size, const uint32_t point_h[8], const uint32_t* mask_values_h, uint32_t n_mask,
                                const uint32_t* params_h, uint32_t n_params, const uint32_t* coeffs_h, uint32_t n_coeffs, uint32_t out_h[4]) {
    API_TRY
    const char* me = "bfhip_air_eval_at_point";
    if (!air || !point_h || !coeffs_h || !out_h || (!mask_values_h && n_mask) || (!params_h && n_params)) throw HipError("null argument");
    if (log_size < 1 || log_size > 30) throw HipError(std::string(me) + ": log_size must be in [1, 30]");
    if (n_mask != air->mask_cols.size()) throw HipError(std::string(me) + ": the program's mask has " + std::to_string(air->mask_cols.size()) + " entries, got " + std::to_string(n_mask) + " values");
    if (n_params != air->n_params) throw HipError(std::string(me) + ": the program takes " + std::to_string(air->n_params) + " parameters, got " + std::to_string(n_params));
    if (n_coeffs != air->n_constraints) throw HipError(std::string(me) + ": the program has " + std::to_string(air->n_constraints) + " constraints, got " + std::to_string(n_coeffs) + " coefficients");
    const PtQ point = canonical_point(point_h, me);
    std::vector<Q31> mask(n_mask), params(n_params), coeffs(n_coeffs);
    for (u32 i = 0; i < n_mask; i++) mask[i] = canonical_q31(mask_values_h + 4 * i, me);
    for (u32 i = 0; i < n_params; i++) params[i] = canonical_q31(params_h + 4 * i, me);
    for (u32 i = 0; i < n_coeffs; i++) coeffs[i] = canonical_q31(coeffs_h + 4 * i, me);
    const Q31 denom = coset_vanishing_q(log_size, point);
    if (q_is_zero(denom)) throw HipError(std::string(me) + ": the point lies on the trace domain");
    std::vector<Q31> m(air->n_m ? air->n_m : 1, q_zero()), q(air->n_q ? air->n_q : 1, q_zero());
    Q31 acc = q_zero();
    u32 ci = 0;
    for (u32 i = 0; i < air->n_instr; i++) {
        const u32 op = air->code[4 * i], dst = air->code[4 * i + 1], a = air->code[4 * i + 2], b = air->code[4 * i + 3];
        switch (op) {
            case AIR_M_COL: m[dst] = mask[air->mask_index(a, (int32_t)b)]; break;
            case AIR_M_CONST: m[dst] = q_from_m(a); break;
            case AIR_M_ADD: m[dst] = q_add(m[a], m[b]); break;
            case AIR_M_SUB: m[dst] = q_sub(m[a], m[b]); break;
            case AIR_M_MUL: m[dst] = q_mul(m[a], m[b]); break;
            case AIR_M_NEG: m[dst] = q_neg(m[a]); break;
            case AIR_Q_COL: {
                Q31 r = mask[air->mask_index(a, (int32_t)b)];
                r = q_add(r, q_mul(mask[air->mask_index(a + 1, (int32_t)b)], q_make(0, 1, 0, 0)));
                r = q_add(r, q_mul(mask[air->mask_index(a + 2, (int32_t)b)], q_make(0, 0, 1, 0)));
                r = q_add(r, q_mul(mask[air->mask_index(a + 3, (int32_t)b)], q_make(0, 0, 0, 1)));
                q[dst] = r;
                break;
            }
            case AIR_Q_PARAM: q[dst] = params[a]; break;
            case AIR_Q_FROM_M: q[dst] = m[a]; break;
            case AIR_Q_ADD: q[dst] = q_add(q[a], q[b]); break;
            case AIR_Q_SUB: q[dst] = q_sub(q[a], q[b]); break;
            case AIR_Q_MUL: q[dst] = q_mul(q[a], q[b]); break;
            case AIR_Q_MULM: q[dst] = q_mul(q[a], m[b]); break;
            case AIR_C_BASE: acc = q_add(acc, q_mul(coeffs[ci++], m[a])); break;
            default: acc = q_add(acc, q_mul(coeffs[ci++], q[a])); break;      // AIR_C_EXT: the validator admits nothing else
        }
    }
    q31_words(q_mul(acc, q_inv(denom)), out_h);
    return 0;
    API_CATCH
}

}  // extern "C"
