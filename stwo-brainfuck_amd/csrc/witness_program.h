// The witness program (include/bfhip.h "Witness programs"): the base-field half of a constraint program's bytecode (air_program.h) run once
// per row of CanonicCoset(log_size), reading input columns at trace offsets and STORING output columns — the columns an AIR's author can
// compute row by row from the ones they have: an inverse, a padding flag, the bits of a byte, a "next" value. witness_program_host.hip holds
// the validator and the whole-table evaluator (host only), witness_program.hip the gfx950 interpreter. Internal to the library.
#pragma once
#include "relation_program.h"

namespace bf {

// The numbering continues that of RelOp. {op, dst, a, b}:
//   WIT_ARG dst, k       m[dst] = args[k]                          WIT_ROW dst          m[dst] = the row's coset index
//   WIT_INV0 dst, a      m[dst] = 1 / m[a], and 0 for 0            WIT_IS_ZERO dst, a   m[dst] = m[a] == 0
//   WIT_LT dst, a, b     m[dst] = m[a] < m[b] as integers          WIT_AND dst, a, imm  m[dst] = m[a] & imm, imm < 2^31
//   WIT_SHR dst, a, imm  m[dst] = m[a] >> imm, imm <= 30           WIT_STORE out, a     output column `out` of this row = m[a]
enum WitOp : u32 { WIT_ARG = 19, WIT_ROW, WIT_INV0, WIT_IS_ZERO, WIT_LT, WIT_AND, WIT_SHR, WIT_STORE };
constexpr u32 WIT_MAX_SHIFT = 30;

// One own opcode that writes a register, on values: what the kernel and bfhip_witness_program_eval_table share (WIT_STORE is the caller's).
// `b` is m[b] for WIT_LT and the immediate for WIT_AND / WIT_SHR; `arg` and `row` are what WIT_ARG and WIT_ROW give.
BF_HD u32 wit_value(u32 op, u32 a, u32 b, u32 arg, u32 row) {
    switch (op) {
        case WIT_ARG: return arg;
        case WIT_ROW: return row;
        case WIT_INV0: return m_inv(a);      // x^(p - 2): 0 for 0
        case WIT_IS_ZERO: return a == 0 ? 1u : 0u;
        case WIT_LT: return a < b ? 1u : 0u;
        case WIT_AND: return a & b;
        default: return a >> b;              // WIT_SHR
    }
}

}  // namespace bf

// A validated program. Everything the interpreters index with was checked by bfhip_witness_program_create: they do no bounds checks of
// their own.
struct bfhip_witness_program {
    std::vector<uint32_t> code;              // 4 words per instruction
    uint32_t n_cols = 0, n_out = 0, n_args = 0, n_instr = 0, n_m = 0;
    int32_t min_off = 0, max_off = 0;
};
