// The host-only half of the witness program (include/bfhip.h "Witness programs"): the validator behind bfhip_witness_program_create, the
// shape, and the evaluator of a whole row-order table — the definition k_witness_program (witness_program.hip) is held to. No GPU, no HIP
// call: this file also compiles with a plain C++ compiler, which is how tests/native/witness_host_sanitize.cpp puts it under the sanitizers.
#include "api_guard.h"
#include "witness_program.h"
#include "program_validate.h"
#include "rows_index.h"

using namespace bf;

namespace {

const ProgramFamily FAMILY = {"bfhip_witness_program_create", nullptr, "a witness program is base field only (no q registers, no parameters)"};

// One pass over the code: the shared rules (program_validate.h) for the base-field opcodes, plus the own opcodes and the outputs.
void validate(bfhip_witness_program& wp, ProgramValidator& v) {
    const size_t n = wp.n_instr;
    std::vector<uint8_t> stored(wp.n_out, 0);
    for (size_t i = 0; i < n; i++) {
        const u32 op = wp.code[4 * i], dst = wp.code[4 * i + 1], a = wp.code[4 * i + 2], b = wp.code[4 * i + 3];
        if (v.shared(i, op, dst, a, b)) {
            if (op == AIR_M_COL) {
                const int32_t off = (int32_t)b;
                if (off < wp.min_off) wp.min_off = off;
                if (off > wp.max_off) wp.max_off = off;
            }
            continue;
        }
        switch (op) {
            case AIR_C_BASE: v.refuse(i, "C_BASE: a witness program has no constraints");
            case AIR_C_EXT: v.refuse(i, "C_EXT: a witness program has no constraints");
            case LOGUP_FRAC: v.refuse(i, "FRAC: a witness program has no fractions");
            case LOGUP_END_COL: v.refuse(i, "END_COL: a witness program has no logUp columns");
            case REL_WORD: v.refuse(i, "REL_WORD: a witness program has no relation entries");
            case REL_ENTRY: v.refuse(i, "REL_ENTRY: a witness program has no relation entries");
            case WIT_ARG:
                if (a >= wp.n_args) v.refuse(i, "ARG: arg " + std::to_string(a) + " out of range (the program has " + std::to_string(wp.n_args) + " args)");
                v.m_dst(i, dst);
                break;
            case WIT_ROW: v.m_dst(i, dst); break;
            case WIT_INV0: case WIT_IS_ZERO: v.m_src(i, a); v.m_dst(i, dst); break;
            case WIT_LT: v.m_src(i, a); v.m_src(i, b); v.m_dst(i, dst); break;
            case WIT_AND:
                v.m_src(i, a);
                if (b >> 31) v.refuse(i, "AND: immediate " + std::to_string(b) + " out of range (imm < 2^31)");
                v.m_dst(i, dst);
                break;
            case WIT_SHR:
                v.m_src(i, a);
                if (b > WIT_MAX_SHIFT) v.refuse(i, "SHR: immediate " + std::to_string(b) + " out of range (imm <= 30)");
                v.m_dst(i, dst);
                break;
            case WIT_STORE:
                if (dst >= wp.n_out) v.refuse(i, "STORE: output " + std::to_string(dst) + " out of range (the program has " + std::to_string(wp.n_out) + " outputs)");
                v.m_src(i, a);
                if (stored[dst]) v.refuse(i, "STORE: output " + std::to_string(dst) + " is stored a second time");
                stored[dst] = 1;
                break;
            default: v.refuse(i, "unknown opcode " + std::to_string(op));
        }
    }
    for (u32 k = 0; k < wp.n_out; k++) if (!stored[k]) v.refuse(n, "the program ends with output " + std::to_string(k) + " never stored");
    wp.n_m = v.n_m;
}

}  // namespace

extern "C" {

int32_t bfhip_witness_program_create(const uint32_t* code, size_t n_words, uint32_t n_cols, uint32_t n_out, uint32_t n_args, bfhip_witness_program** out) {
    API_TRY
    if (!code || !out) throw HipError("null argument");
    ProgramValidator v(FAMILY, n_words, n_cols, 0);
    if (n_args > AIR_MAX_PARAMS) v.refuse(0, "more than BFHIP_AIR_MAX_PARAMS (64) args");
    if (n_out < 1 || n_out > AIR_MAX_COLUMNS) v.refuse(0, std::to_string(n_out) + " outputs, not 1 to BFHIP_AIR_MAX_COLUMNS (256)");
    auto* wp = new bfhip_witness_program();
    try {
        wp->code.assign(code, code + n_words);
        wp->n_instr = (u32)(n_words / 4); wp->n_cols = n_cols; wp->n_out = n_out; wp->n_args = n_args;
        validate(*wp, v);
    } catch (...) { delete wp; throw; }
    *out = wp;
    return 0;
    API_CATCH
}
int32_t bfhip_witness_program_destroy(bfhip_witness_program* wp) { API_TRY delete wp; return 0; API_CATCH }

int32_t bfhip_witness_program_shape(const bfhip_witness_program* wp, uint32_t out[8]) {
    API_TRY
    if (!wp || !out) throw HipError("null argument");
    const u32 v[8] = {wp->n_cols, wp->n_out, wp->n_args, wp->n_instr, wp->n_m, (u32)wp->min_off, (u32)wp->max_off, 0};
    memcpy(out, v, sizeof v);
    return 0;
    API_CATCH
}

// The interpreter of witness_program.hip over a row-major table in ROW order: row r reads column c at offset `off` in row (r + off) mod n.
int32_t bfhip_witness_program_eval_table(const bfhip_witness_program* wp, uint32_t log_size, const uint32_t* table_h, const uint32_t* args_h, uint32_t n_args,
                                         uint32_t* out_h) {
    API_TRY
    const std::string who = "bfhip_witness_program_eval_table: ";
    if (!wp || !out_h || (!table_h && wp->n_cols) || (!args_h && n_args)) throw HipError(who + "null argument");
    if (log_size < 1 || log_size > ROWS_MAX_LOG) throw HipError(who + "log_size " + std::to_string(log_size) + " is outside 1..30");
    if (n_args != wp->n_args) throw HipError(who + std::to_string(n_args) + " args, the program has " + std::to_string(wp->n_args));
    for (u32 k = 0; k < n_args; k++)
        if (args_h[k] >= P31) throw HipError(who + "arg " + std::to_string(k) + ": " + std::to_string(args_h[k]) + " is not a canonical M31 value");
    const u64 n = u64(1) << log_size, nc = wp->n_cols, no = wp->n_out;
    for (u64 r = 0; r < n; r++)
        for (u64 c = 0; c < nc; c++)
            if (table_h[r * nc + c] >= P31)
                throw HipError(who + "row " + std::to_string(r) + ", column " + std::to_string(c) + ": " + std::to_string(table_h[r * nc + c]) + " is not a canonical M31 value");
    u32 m[AIR_MAX_M_REGS] = {};
    for (u64 r = 0; r < n; r++) {
        for (u32 i = 0; i < wp->n_instr; i++) {
            const u32 op = wp->code[4 * i], dst = wp->code[4 * i + 1], a = wp->code[4 * i + 2], b = wp->code[4 * i + 3];
            switch (op) {
                case AIR_M_COL: m[dst] = table_h[((r + (u64)(int64_t)(int32_t)b) & (n - 1)) * nc + a]; break;
                case AIR_M_CONST: m[dst] = a; break;
                case AIR_M_ADD: m[dst] = m_add(m[a], m[b]); break;
                case AIR_M_SUB: m[dst] = m_sub(m[a], m[b]); break;
                case AIR_M_MUL: m[dst] = m_mul(m[a], m[b]); break;
                case AIR_M_NEG: m[dst] = m_neg(m[a]); break;
                case WIT_STORE: out_h[r * no + dst] = m[a]; break;
                case WIT_ARG: m[dst] = wit_value(op, 0, 0, args_h[a], 0); break;
                case WIT_ROW: m[dst] = wit_value(op, 0, 0, 0, (u32)r); break;
                case WIT_LT: m[dst] = wit_value(op, m[a], m[b], 0, 0); break;
                default: m[dst] = wit_value(op, m[a], b, 0, 0); break;      // INV0, IS_ZERO, AND, SHR: the validator admits nothing else
            }
        }
    }
    return 0;
    API_CATCH
}

}  // extern "C"
