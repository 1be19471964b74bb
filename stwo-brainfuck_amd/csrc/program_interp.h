// The instruction core of the four program kernels (device only): k_air_program (air_program.hip), air_check_cell (air_check.hip),
// k_logup_program (logup_program.hip) and k_relation_program (relation_program.hip) run the M_* / Q_* opcodes of air_program.h through the
// one loop below and differ in two small policy types.
//
// One lane per row, one wave per workgroup. The instruction stream, the column descriptors and the parameters are the same for every lane:
// they live in HBM and are fetched through scalar loads (address space 4), and the opcode dispatch is a scalar branch. The two register files
// would be runtime-indexed private arrays, which the compiler puts in scratch; they live in dynamic LDS instead, laid out [register][lane] so
// that the 64 lanes of an access hit 64 consecutive banks, and sized at launch from the registers the program uses (a small program keeps its
// occupancy). No barrier: a lane only ever touches its own slot of each register.
//
// Row policy — what a row is:
//   static constexpr bool OFFSETS              whether the family's validator admits a non-zero offset; without it the offset word is never tested
//   u32 or u64 at0(bf_u32x4 col) const         storage index of the row's own cell in a column, given the column's descriptor (what the type
//                                              decides: program_ld_cell)
//   u32 at(int off) const                      storage index of the row at trace offset `off` != 0 (a column read so is stored at full size)
// Sink policy — the family's own opcodes and the kernel's running state:
//   static constexpr bool HAS_Q                whether the family has q registers; without them the Q_* cases are unreachable and compile to nothing
//   static constexpr u32 OP                    the family's first own opcode, a case of the one switch like the shared ones: with both of a
//   void op(bf_u32x4 ins, u32* m, u32* q)      family's opcodes behind `default:` the switch compiles to another compare tree, and k_air_program and
//                                              k_air_check_cells took 8 % longer (profiles/program_interp_shared_ab.txt)
//   void other(bf_u32x4 ins, u32* m, u32* q)   the switch's `default:`: every other opcode; the validator admits only the family's own
#pragma once
#include "kernels.h"
#include "air_program.h"

namespace bf {

constexpr u32 PROGRAM_LANES = 64;

// One cell of a column from its descriptor {pointer low, pointer high, ...}. The byte offset is computed in the type the row policy gives its
// indices in. A domain has at most 2^29 cells (max_log_domain <= 29, and every entry point holds its log_size to it), so u32 is exact and
// compiles to a scalar base plus a 32-bit lane offset; u64 compiles to a 64-bit lane address. Each kernel keeps the form it was measured
// with before the interpreters were merged (profiles/program_interp_shared_ab.txt: k_relation_program's counting launches took 1 to 2 %
// longer with the 32-bit form).
template <class Index>
__device__ __forceinline__ u32 program_ld_cell(const bf_u32x4 col, Index idx) {
    const unsigned long long base = ((unsigned long long)col.y << 32) | col.x;
    return *(g_cu32p)((const BF_GLOBAL char*)base + (idx << 2));
}

// q points at the lane's slot of q register 0; `r` is a register number times PROGRAM_LANES: coordinate k of the register is q[4 r + k * PROGRAM_LANES]
__device__ __forceinline__ Q31 program_q_ld(const u32* q, u32 r) { return q_make(q[4 * r], q[4 * r + PROGRAM_LANES], q[4 * r + 2 * PROGRAM_LANES], q[4 * r + 3 * PROGRAM_LANES]); }
__device__ __forceinline__ void program_q_st(u32* q, u32 r, u32 v0, u32 v1, u32 v2, u32 v3) {
    q[4 * r] = v0; q[4 * r + PROGRAM_LANES] = v1; q[4 * r + 2 * PROGRAM_LANES] = v2; q[4 * r + 3 * PROGRAM_LANES] = v3;
}
__device__ __forceinline__ void program_q_st(u32* q, u32 r, Q31 v) { program_q_st(q, r, v.a.a, v.a.b, v.b.a, v.b.b); }

// m and q point at the lane's slot of register 0 of each file (m[r] = m[r * PROGRAM_LANES]); q is not touched when Sink::HAS_Q is false.
template <class Row, class Sink>
__device__ __forceinline__ void program_run(const BF_CONSTANT bf_u32x4* code, u32 n_instr, const BF_CONSTANT bf_u32x4* cols, const BF_CONSTANT bf_u32x4* params,
                                            u32* const m, u32* const q, const Row& row, Sink& sink) {
#pragma unroll 1
    for (u32 pc = 0; pc < n_instr; pc++) {
        const bf_u32x4 ins = code[pc];
        const u32 dst = ins.y * PROGRAM_LANES, ra = ins.z * PROGRAM_LANES, rb = ins.w * PROGRAM_LANES;
        switch (ins.x) {
            case AIR_M_COL: {
                const bf_u32x4 col = cols[ins.z];
                if constexpr (Row::OFFSETS) {
                    const int off = (int)ins.w;
                    m[dst] = program_ld_cell(col, off ? row.at(off) : row.at0(col));
                } else m[dst] = program_ld_cell(col, row.at0(col));
                break;
            }
            case AIR_M_CONST: m[dst] = ins.z; break;
            case AIR_M_ADD: m[dst] = m_add(m[ra], m[rb]); break;
            case AIR_M_SUB: m[dst] = m_sub(m[ra], m[rb]); break;
            case AIR_M_MUL: m[dst] = m_mul(m[ra], m[rb]); break;
            case AIR_M_NEG: m[dst] = m_neg(m[ra]); break;
            case AIR_Q_COL: {
                if constexpr (Sink::HAS_Q) {
                    int off = 0;
                    u32 orow = 0;
                    if constexpr (Row::OFFSETS) { off = (int)ins.w; if (off) orow = row.at(off); }
#pragma unroll
                    for (u32 k = 0; k < 4; k++) {
                        const bf_u32x4 col = cols[ins.z + k];
                        q[4 * dst + k * PROGRAM_LANES] = program_ld_cell(col, off ? orow : row.at0(col));
                    }
                } else __builtin_unreachable();
                break;
            }
            case AIR_Q_PARAM: {
                if constexpr (Sink::HAS_Q) {
                    const bf_u32x4 v = params[ins.z];
                    program_q_st(q, dst, v.x, v.y, v.z, v.w);
                } else __builtin_unreachable();
                break;
            }
            case AIR_Q_FROM_M:
                if constexpr (Sink::HAS_Q) program_q_st(q, dst, m[ra], 0, 0, 0); else __builtin_unreachable();
                break;
            case AIR_Q_ADD: case AIR_Q_SUB: case AIR_Q_MUL: {
                if constexpr (Sink::HAS_Q) {
                    const Q31 x = program_q_ld(q, ra), y = program_q_ld(q, rb);
                    program_q_st(q, dst, ins.x == AIR_Q_ADD ? q_add(x, y) : ins.x == AIR_Q_SUB ? q_sub(x, y) : q_mul(x, y));
                } else __builtin_unreachable();
                break;
            }
            case AIR_Q_MULM:
                if constexpr (Sink::HAS_Q) program_q_st(q, dst, q_mulm(program_q_ld(q, ra), m[rb])); else __builtin_unreachable();
                break;
            case Sink::OP: sink.op(ins, m, q); break;
            default: sink.other(ins, m, q); break;
        }
    }
}

}  // namespace bf
