// Assertion of the 13 AIRs on the TRACE domain: which cells of CanonicCoset(log_size) violate which constraint.
//
// Replaces stwo's `assert_constraints` (constraint_framework/assert.rs: AssertEvaluator over every row of the trace), which the reference's
// component tests are built on — the positive cases at memory/component.rs:163-209 and brainfuck_air/mod.rs:252-396 (all 13 components),
// the ten negative cases at memory/component.rs:211-609, whose panic texts quote the failing row and value. The prover only says
// "ConstraintsNotSatisfied" after a whole proof (prover.hip: HipProver::prove, the out-of-domain check); this pass names the component, the constraint
// and the row: one streaming read of the columns, no transform, no hashing.
//
// A lane owns one domain cell (storage index, bit-reversed circle-domain order) and evaluates the component's AIR body of air.h with
// IsFirst = [cell == 0]; 16x-replicated columns are read row-granular (ColDesc shift 4), the last logUp column at the cell and at its
// trace-domain predecessor (air.h: prev_trace_cell). Constraint j sets bit j of the lane's mask when it is non-zero; nothing leaves
// early, so a wave stays uniform.
#include "kernels.h"
#include "air.h"

namespace bf {

// RECORD: also keep the lowest failing constraint of the cell and its value (k_check_first; a base-field value is reported as (v, 0, 0, 0))
template <bool RECORD>
struct CheckEval : LogupState<CheckEval<RECORD>, Fm> {
    typedef Fm F;
    const CheckLaunch& a; u32 cell; int ti = 0, ii = 0, ci = 0;
    u32 mask = 0; u32 first = 0xffffffffu; Q31 first_value;
    __device__ CheckEval(const CheckLaunch& a_, u32 cell_) : a(a_), cell(cell_) { first_value = q_zero(); this->total_sum = a_.total_sum; }
    __device__ __forceinline__ Fm is_first() { return {cell == 0 ? 1u : 0u}; }      // IsFirst(log_size) on its own domain: no column needed
    __device__ __forceinline__ Fm trace() { return {ld_col(a.trace[ti++], cell)}; }
    __device__ __forceinline__ Fm cst(u32 k) { return {k}; }
    __device__ __forceinline__ Q31 rd(int i0, u32 r) {
        return q_make(ld_col(a.inter[i0], r), ld_col(a.inter[i0 + 1], r), ld_col(a.inter[i0 + 2], r), ld_col(a.inter[i0 + 3], r));
    }
    __device__ __forceinline__ Fq inter_cur() { Fq v{rd(ii, cell)}; ii += 4; return v; }
    __device__ __forceinline__ void inter_cur_prev(Fq& cur, Fq& prev) {
        cur.v = rd(ii, cell);
        prev.v = rd(ii, prev_trace_cell(cell, a.log_size));
        ii += 4;
    }
    __device__ __forceinline__ void note(bool bad, Q31 v) {
        if (bad) {
            if (RECORD && first == 0xffffffffu) { first = (u32)ci; first_value = v; }
            mask |= 1u << ci;
        }
        ci++;
    }
    __device__ __forceinline__ void constraint(Fm c) { note(c.v != 0, q_from_m(c.v)); }
    __device__ __forceinline__ void constraint(Fq c) { note(!q_is_zero(c.v), c.v); }
};

// Slot 16 of a wave's / a workgroup's counters = cells with any violation; slots 0..15 = cells violating constraint j.
static constexpr u32 CHECK_SLOTS = 17;

// Reduction: the ballot of (mask != 0) decides everything — a wave without a violation issues no LDS traffic and no atomic (it only passes
// the two barriers), so a valid trace costs its loads. A wave with violations counts per constraint with popcounts of ballots; lanes are in
// cell order, so its first bad cell is the lowest set bit. Such waves first clear the four presence flags (all write the same zeros), then
// publish flag, counts and first cell; the lowest of them adds the workgroup's sums to the report: one 64-bit atomicAdd per non-zero
// counter and one 64-bit atomicMin. Integer atomics only: the report does not depend on the order in which workgroups arrive.
template <int COMP>
__global__ void __launch_bounds__(256) k_check_cells(const CheckLaunch* __restrict__ ap) {
    __shared__ u32 s_flag[4], s_first[4], s_cnt[4][CHECK_SLOTS];
    const CheckLaunch& a = *ap;
    const u32 n = 1u << a.log_size;
    const u32 cell = blockIdx.x * 256u + threadIdx.x;
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    u32 mask = 0;
    if (cell < n) {
        CheckEval<false> e(a, cell);
        air_eval<COMP>(e, a.el);
        mask = e.mask;
    }
    const u64 bad = __ballot(mask != 0);
    if (bad && lane < 4) s_flag[lane] = 0;
    __syncthreads();
    if (bad) {
        u32 mine = 0;
#pragma unroll
        for (u32 j = 0; j < 12; j++) {      // n_constraints(c) <= 12
            const u32 cnt = (u32)__popcll(__ballot((mask >> j) & 1u));
            if (lane == j) mine = cnt;
        }
        if (lane == 16) mine = (u32)__popcll(bad);
        if (lane < CHECK_SLOTS) s_cnt[wave][lane] = mine;
        if (lane == 0) { s_flag[wave] = 1; s_first[wave] = blockIdx.x * 256u + wave * 64u + (u32)(__ffsll((long long)bad) - 1); }
    }
    __syncthreads();
    if (!bad) return;
    u32 leader = 0;
    while (!s_flag[leader]) leader++;       // this wave's own flag is set: leader <= wave
    if (wave != leader) return;
    CheckReportDev* rep = a.report;
    if (lane < CHECK_SLOTS) {
        u32 sum = 0;
        for (u32 w = leader; w < 4; w++) if (s_flag[w]) sum += s_cnt[w][lane];
        if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(lane == 16 ? &rep->n_bad_cells : &rep->bad_per_constraint[lane]), (unsigned long long)sum);
    }
    if (lane == 0) atomicMin(reinterpret_cast<unsigned long long*>(&rep->first_bad_cell), (unsigned long long)s_first[leader]);   // waves are in cell order too
}

// One wave re-evaluates the AIR at the first bad cell (known once k_check_cells has completed: same stream) and writes the lowest failing
// constraint and its value; -1 and zeros for a trace without violations.
template <int COMP>
__global__ void __launch_bounds__(64) k_check_first(const CheckLaunch* __restrict__ ap) {
    const CheckLaunch& a = *ap;
    CheckReportDev* rep = a.report;
    const u64 cell = rep->first_bad_cell;
    u32 first = 0xffffffffu; Q31 v = q_zero();
    if (cell < ((u64)1 << a.log_size)) {
        CheckEval<true> e(a, (u32)cell);
        air_eval<COMP>(e, a.el);
        first = e.first; v = e.first_value;
    }
    if (threadIdx.x == 0) {
        rep->first_bad_constraint = first;
        rep->first_bad_value[0] = v.a.a; rep->first_bad_value[1] = v.a.b; rep->first_bad_value[2] = v.b.a; rep->first_bad_value[3] = v.b.b;
    }
}

template <int COMP>
static void launch_check(hipStream_t s, const CheckLaunch* a, u32 log_size) {
    const u32 n = 1u << log_size;
    hipLaunchKernelGGL(k_check_cells<COMP>, dim3((n + 255) / 256), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_check_first<COMP>, dim3(1), dim3(64), 0, s, a);
}

void check_constraints_launch(hipStream_t stream, int comp, const CheckLaunch* d_args, u32 log_size) {
    switch (comp) {
#define X(C) case C: launch_check<C>(stream, d_args, log_size); break;
        X(C_MEMORY) X(C_INSTRUCTION) X(C_PROGRAM) X(C_PROCESSOR) X(C_JNZ) X(C_JZ) X(C_INPUT) X(C_LEFT) X(C_MINUS) X(C_OUTPUT) X(C_PLUS) X(C_RIGHT)
        default: launch_check<C_EOE>(stream, d_args, log_size); break;
#undef X
    }
}

}  // namespace bf
