// What a cell of the trace domain is and what FRAC / END_COL do there, plus the three bodies of the coset-order scan (device only): what the
// fraction-program kernels put on the interpreter core of program_interp.h. Shared by the single call (logup_program.hip: one component, four
// launches) and the batch (logup_batch.hip: every component of a list, the same four stages over tables), so that the sink's arithmetic and
// each scan body exist once.
//
// Row stage: FRAC folds q[a] / q[b] into the open column's running fraction fn / fd (three products; every denominator is tested for zero
// where it stands, so a vanishing one is named and not hidden in a product), END_COL adds fn / fd to the running value with the column's one
// q_inv; END_COL of a column before the last stores the running value to the column's four coordinate columns (lane = cell: 256-byte
// coalesced stores), END_COL of the last column stores it as one 16-byte word of v[cell], the input of the scan.
// Scan stage: the coset-order inclusive prefix sum of v over N = 2^log_size cells. With d = bit_rev(cell), coset position 2q is d = q and
// 2q + 1 is d = N - 1 - q: w[q] = v[d = q] + v[d = N - 1 - q] (q < N / 2) is scanned (1024-entry tiles, then the tile totals), and the prefix
// at 2q + 1 is W[q], at 2q it is W[q] - v[d = N - 1 - q]. Bit reversal commutes with the complement, so in cell indices d = N - 1 - q is cell
// N - 1 - bit_rev(q): the partner of cell c is always cell N - 1 - c.
#pragma once
#include "logup_program.h"
#include "program_interp.h"

namespace bf {

constexpr u32 LP_TILE = 1024, LP_CHUNK = 256;

// One component, staged in HBM. Addresses are kept as integers: read from address space 4 they arrive in SGPRs and are cast to global pointers.
struct LogupProgLaunch {
    u64 code;            // bf_u32x4[n_instr]
    u64 cols;            // bf_u32x4[n_cols]: {pointer low, pointer high, shift, 0}
    u64 params;          // bf_u32x4[n_params]
    u64 out[4 * LOGUP_MAX_COLUMNS];
    u64 v, wloc, totals; // uint4[N], uint4[N / 2], uint4[nb + 1]
    u64 tail;            // uint4[2]: the claimed sum; {zero-denominator key low, high, -, -}
    u32 n_instr, n_m, log_size, n_logup_cols, nb, pad;
};

__device__ __forceinline__ Q31 lp_ld(const uint4* p, u32 i) { const uint4 v = p[i]; return q_make(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ void lp_st(uint4* p, u32 i, Q31 q) { p[i] = make_uint4(q.a.a, q.a.b, q.b.a, q.b.b); }

// A cell of the trace domain, read at offset 0 only (bfhip_logup_create refuses offsets): a column of shift s holds it at cell >> s
struct LogupRow {
    static constexpr bool OFFSETS = false;
    u32 self;
    __device__ __forceinline__ u64 at0(const bf_u32x4 col) const { return self >> col.z; }
};

// FRAC / END_COL (the file header says what they do)
struct LogupSink {
    static constexpr bool HAS_Q = true;
    const BF_CONSTANT LogupProgLaunch* a;
    u32 cell, last_col;
    Q31 cur = q_zero();          // LogupTraceGenerator: column k starts from column k - 1 (finalize_col keeps the running sum)
    u32 col_i = 0, frac_i = 0, open = 0;
    Q31 fn = q_zero(), fd = q_one();      // the open column's fractions so far as one fraction fn / fd (`open` of them: wave-uniform)
    static constexpr u32 OP = LOGUP_FRAC;
    __device__ __forceinline__ void op(const bf_u32x4 ins, const u32*, const u32* q) {
        const Q31 num = program_q_ld(q, ins.z * PROGRAM_LANES), den = program_q_ld(q, ins.w * PROGRAM_LANES);
        // stwo panics on a zero denominator; q_inv(0) is 0 and would pass for a value. The lowest (cell, fraction) wins the key.
        if (q_is_zero(den)) atomicMin((unsigned long long*)(a->tail + 16), ((unsigned long long)cell << 8) | frac_i);
        // fn / fd + num / den = (fn den + num fd) / (fd den): three products per further fraction, one inversion per column
        if (open) { fn = q_add(q_mul(fn, den), q_mul(num, fd)); fd = q_mul(fd, den); } else { fn = num; fd = den; }
        open++; frac_i++;
    }
    __device__ __forceinline__ void other(const bf_u32x4, const u32*, const u32*) {      // LOGUP_END_COL: the validator admits nothing else
        cur = q_add(cur, q_mul(fn, q_inv(fd)));
        open = 0;
        if (col_i < last_col) {
#pragma unroll
            for (u32 k = 0; k < 4; k++) {
                g_u32p o = (g_u32p)a->out[4 * col_i + k];
                o[cell] = k == 0 ? cur.a.a : k == 1 ? cur.a.b : k == 2 ? cur.b.a : cur.b.b;
            }
        } else lp_st((uint4*)a->v, cell, cur);
        col_i++;
    }
};

// The row stage of one component on the 64 cells from cell - lane on (the caller has checked cell < 2^log_size); s_regs = the workgroup's
// dynamic LDS, at least (n_m + 4 n_q) * PROGRAM_LANES words
__device__ __forceinline__ void lp_rows(const BF_CONSTANT LogupProgLaunch* a, u32 cell, u32* s_regs) {
    LogupSink sink{a, cell, a->n_logup_cols - 1};
    program_run((const BF_CONSTANT bf_u32x4*)a->code, a->n_instr, (const BF_CONSTANT bf_u32x4*)a->cols, (const BF_CONSTANT bf_u32x4*)a->params,
                s_regs + threadIdx.x, s_regs + a->n_m * PROGRAM_LANES + threadIdx.x, LogupRow{cell}, sink);
}

// Tile-local inclusive scan of w[q] = v[cell bit_rev(q)] + v[cell N - 1 - bit_rev(q)], q < N / 2, for tile `tile` of one component: four
// consecutive entries per thread, the 256 thread sums scanned through LDS (s: uint4[256]). The tile's total goes to totals[tile].
__device__ __forceinline__ void lp_scan_tile(const LogupProgLaunch& a, u32 tile, uint4* s) {
    const uint4* __restrict__ v = (const uint4*)a.v;
    uint4* __restrict__ wloc = (uint4*)a.wloc;
    const u32 log_size = a.log_size, N = 1u << log_size, H = N >> 1;
    const u32 q0 = tile * LP_TILE + 4 * threadIdx.x;
    Q31 p[4];
    Q31 run = q_zero();
#pragma unroll
    for (u32 j = 0; j < 4; j++) {
        const u32 qi = q0 + j;
        if (qi < H) { const u32 c = bit_rev(qi, log_size); run = q_add(run, q_add(lp_ld(v, c), lp_ld(v, N - 1 - c))); }
        p[j] = run;
    }
    lp_st(s, threadIdx.x, run);
    __syncthreads();
    for (u32 off = 1; off < 256; off <<= 1) {
        const Q31 t = threadIdx.x >= off ? q_add(lp_ld(s, threadIdx.x), lp_ld(s, threadIdx.x - off)) : lp_ld(s, threadIdx.x);
        __syncthreads();
        lp_st(s, threadIdx.x, t);
        __syncthreads();
    }
    const Q31 before = threadIdx.x ? lp_ld(s, threadIdx.x - 1) : q_zero();
#pragma unroll
    for (u32 j = 0; j < 4; j++) if (q0 + j < H) lp_st(wloc, q0 + j, q_add(before, p[j]));
    if (threadIdx.x == 255) lp_st((uint4*)a.totals, tile, lp_ld(s, 255));
}

// Exclusive scan of one component's nb tile totals (one workgroup, serial over chunks of 256 with a carry; s: uint4[LP_CHUNK]); totals[nb]
// and tail[0] receive the grand total W[N / 2 - 1], which is the claimed sum: the last coset element of the prefix sum.
__device__ __forceinline__ void lp_scan_totals(const LogupProgLaunch& a, uint4* s) {
    uint4* __restrict__ totals = (uint4*)a.totals;
    const u32 nb = a.nb;
    Q31 carry = q_zero();
    for (u32 base = 0; base < nb; base += LP_CHUNK) {
        const u32 i = base + threadIdx.x;
        const Q31 v = i < nb ? lp_ld(totals, i) : q_zero();
        lp_st(s, threadIdx.x, v);
        __syncthreads();
        for (u32 off = 1; off < LP_CHUNK; off <<= 1) {
            const Q31 t = threadIdx.x >= off ? q_add(lp_ld(s, threadIdx.x), lp_ld(s, threadIdx.x - off)) : lp_ld(s, threadIdx.x);
            __syncthreads();
            lp_st(s, threadIdx.x, t);
            __syncthreads();
        }
        const Q31 incl = lp_ld(s, threadIdx.x), chunk_total = lp_ld(s, LP_CHUNK - 1);
        __syncthreads();
        if (i < nb) lp_st(totals, i, q_add(carry, q_sub(incl, v)));
        carry = q_add(carry, chunk_total);
    }
    if (threadIdx.x == 0) { lp_st(totals, nb, carry); lp_st((uint4*)a.tail, 0, carry); }
}

// The last logUp column at cell c < N of one component: cell c even is d = bit_rev(c) < N / 2, coset position 2q with q = d:
// W[q] - v[N - 1 - c]; cell c odd is coset position 2q + 1 with q = N - 1 - d = bit_rev(N - 1 - c): W[q].
__device__ __forceinline__ void lp_last_cell(const LogupProgLaunch& a, u32 c) {
    const uint4* __restrict__ v = (const uint4*)a.v;
    const uint4* __restrict__ wloc = (const uint4*)a.wloc;
    const uint4* __restrict__ totals = (const uint4*)a.totals;
    const u32 log_size = a.log_size, N = 1u << log_size;
    const bool even = (c & 1u) == 0;
    const u32 qi = bit_rev(even ? c : N - 1 - c, log_size);
    Q31 res = q_add(lp_ld(wloc, qi), lp_ld(totals, qi / LP_TILE));
    if (even) res = q_sub(res, lp_ld(v, N - 1 - c));
    const u64* out = a.out + 4 * (a.n_logup_cols - 1);
    ((u32*)out[0])[c] = res.a.a;
    ((u32*)out[1])[c] = res.a.b;
    ((u32*)out[2])[c] = res.b.a;
    ((u32*)out[3])[c] = res.b.b;
}

}  // namespace bf
