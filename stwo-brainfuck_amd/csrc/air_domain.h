// What a row of the constraint domain is and what C_BASE / C_EXT do there (device only): the two policy types that the domain evaluators
// put on the interpreter core of program_interp.h. Shared by k_air_program (air_program.hip: one component, added into an accumulator) and
// k_air_compose (air_compose.hip: every component of a bucket, the sum written once).
#pragma once
#include "program_interp.h"

namespace bf {

// Storage index of the row at trace offset `off` from `row` on the 2^log_expand blowup (prev_lde_row of air.hip is off = -1, log_expand = 1):
// a trace step is 2^(log_expand - 1) steps of the half coset; in circle-domain order the first half moves with the offset, the conjugate
// half against it (-P + T = -(P - T)), each cyclically.
__device__ __forceinline__ u32 air_offset_row(u32 row, int off, u32 log_size, u32 log_expand) {
    const u32 el = log_size + log_expand, half = 1u << (el - 1);
    const u32 d = bit_rev(row, el);
    const u32 step = (u32)off * (1u << (log_expand - 1));      // modulo 2^32, of which half is a divisor
    const u32 pd = d < half ? ((d + step) & (half - 1)) : (((d - half - step) & (half - 1)) + half);
    return bit_rev(pd, el);
}

// A row of CanonicCoset(log_size + log_expand).circle_domain(); a column of shift s holds the row's own cell at row >> s
struct AirDomainRow {
    static constexpr bool OFFSETS = true;
    u32 self, log_size, log_expand;
    __device__ __forceinline__ u32 at0(const bf_u32x4 col) const { return self >> col.z; }
    __device__ __forceinline__ u32 at(int off) const { return air_offset_row(self, off, log_size, log_expand); }
};

// C_BASE / C_EXT: sum_j coeff_j * c_j as DomainEval::constraint(Fm) of air.hip keeps it: four 64-bit dot products with lazy reduction for
// the base-field constraints (four products of canonical values on top of a folded accumulator stay below 2^64), a QM31 sum for the others
struct AirDomainSink {
    static constexpr bool HAS_Q = true;
    const BF_CONSTANT bf_u32x4* coeffs;
    u64 acc[4] = {0, 0, 0, 0};
    u32 pending = 0, ci = 0;
    Q31 ext = q_zero();
    static constexpr u32 OP = AIR_C_BASE;
    __device__ __forceinline__ void op(const bf_u32x4 ins, const u32* m, const u32*) {
        const bf_u32x4 k = coeffs[ci++];
        const u32 v = m[ins.z * PROGRAM_LANES];
        if (pending == 4) {      // 4 (p - 1)^2 + 2^34 < 2^64
#pragma unroll
            for (int w = 0; w < 4; w++) acc[w] = m_fold(acc[w]);
            pending = 0;
        }
        acc[0] += (u64)k.x * v; acc[1] += (u64)k.y * v; acc[2] += (u64)k.z * v; acc[3] += (u64)k.w * v;
        pending++;
    }
    __device__ __forceinline__ void other(const bf_u32x4 ins, const u32*, const u32* q) {      // AIR_C_EXT: the validator admits nothing else
        const bf_u32x4 k = coeffs[ci++];
        ext = q_add(ext, q_mul(q_make(k.x, k.y, k.z, k.w), program_q_ld(q, ins.z * PROGRAM_LANES)));
    }
    __device__ __forceinline__ Q31 sum() const { return q_add(q_make(m_canon(acc[0]), m_canon(acc[1]), m_canon(acc[2]), m_canon(acc[3])), ext); }
};

}  // namespace bf
