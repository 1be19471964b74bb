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
struct CheckShared { u32 flag[4], first[4], cnt[4][CHECK_SLOTS]; };

// The body shared by k_check_cells and k_check_batch: workgroup `block` of component COMP's cells, closing on `total_sum`.
template <int COMP>
__device__ __forceinline__ void check_cells_body(const CheckLaunch& a, CheckShared& sh, u32 block, Q31 total_sum) {
    const u32 n = 1u << a.log_size;
    const u32 cell = block * 256u + threadIdx.x;
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    u32 mask = 0;
    if (cell < n) {
        CheckEval<false> e(a, cell);
        e.total_sum = total_sum;
        air_eval<COMP>(e, a.el);
        mask = e.mask;
    }
    const u64 bad = __ballot(mask != 0);
    if (bad && lane < 4) sh.flag[lane] = 0;
    __syncthreads();
    if (bad) {
        u32 mine = 0;
#pragma unroll
        for (u32 j = 0; j < 12; j++) {      // n_constraints(c) <= 12
            const u32 cnt = (u32)__popcll(__ballot((mask >> j) & 1u));
            if (lane == j) mine = cnt;
        }
        if (lane == 16) mine = (u32)__popcll(bad);
        if (lane < CHECK_SLOTS) sh.cnt[wave][lane] = mine;
        if (lane == 0) { sh.flag[wave] = 1; sh.first[wave] = block * 256u + wave * 64u + (u32)(__ffsll((long long)bad) - 1); }
    }
    __syncthreads();
    if (!bad) return;
    u32 leader = 0;
    while (!sh.flag[leader]) leader++;       // this wave's own flag is set: leader <= wave
    if (wave != leader) return;
    CheckReportDev* rep = a.report;
    if (lane < CHECK_SLOTS) {
        u32 sum = 0;
        for (u32 w = leader; w < 4; w++) if (sh.flag[w]) sum += sh.cnt[w][lane];
        if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(lane == 16 ? &rep->n_bad_cells : &rep->bad_per_constraint[lane]), (unsigned long long)sum);
    }
    if (lane == 0) atomicMin(reinterpret_cast<unsigned long long*>(&rep->first_bad_cell), (unsigned long long)sh.first[leader]);   // waves are in cell order too
}

template <int COMP>
__global__ void __launch_bounds__(256) k_check_cells(const CheckLaunch* __restrict__ ap) {
    __shared__ CheckShared sh;
    check_cells_body<COMP>(*ap, sh, blockIdx.x, ap->total_sum);
}

// One wave re-evaluates the AIR at the first bad cell (known once the cells pass has completed: same stream) and writes the lowest failing
// constraint and its value; -1 and zeros for a trace without violations.
template <int COMP>
__device__ __forceinline__ void check_first_body(const CheckLaunch& a, Q31 total_sum) {
    CheckReportDev* rep = a.report;
    const u64 cell = rep->first_bad_cell;
    u32 first = 0xffffffffu; Q31 v = q_zero();
    if (cell < ((u64)1 << a.log_size)) {
        CheckEval<true> e(a, (u32)cell);
        e.total_sum = total_sum;
        air_eval<COMP>(e, a.el);
        first = e.first; v = e.first_value;
    }
    if (threadIdx.x == 0) {
        rep->first_bad_constraint = first;
        rep->first_bad_value[0] = v.a.a; rep->first_bad_value[1] = v.a.b; rep->first_bad_value[2] = v.b.a; rep->first_bad_value[3] = v.b.b;
    }
}

template <int COMP>
__global__ void __launch_bounds__(64) k_check_first(const CheckLaunch* __restrict__ ap) { check_first_body<COMP>(*ap, ap->total_sum); }

// ---- the 13 components in one launch pair (a proof's preflight) ---------------------------------------------------------------------------
// A workgroup finds its component from the workgroup offsets (uniform: scalar loads, as k_constraints_batch and k_rel_flags do) and branches
// on it once, so no wave mixes components; the component's total_sum is the claimed sum the logUp pass left in out->claimed[k].
#define CHECK_DISPATCH(k, CALL) \
    switch (k) { \
        case C_MEMORY: { constexpr int C = C_MEMORY; CALL; } break; case C_INSTRUCTION: { constexpr int C = C_INSTRUCTION; CALL; } break; \
        case C_PROGRAM: { constexpr int C = C_PROGRAM; CALL; } break; case C_PROCESSOR: { constexpr int C = C_PROCESSOR; CALL; } break; \
        case C_JNZ: { constexpr int C = C_JNZ; CALL; } break; case C_JZ: { constexpr int C = C_JZ; CALL; } break; \
        case C_INPUT: { constexpr int C = C_INPUT; CALL; } break; case C_LEFT: { constexpr int C = C_LEFT; CALL; } break; \
        case C_MINUS: { constexpr int C = C_MINUS; CALL; } break; case C_OUTPUT: { constexpr int C = C_OUTPUT; CALL; } break; \
        case C_PLUS: { constexpr int C = C_PLUS; CALL; } break; case C_RIGHT: { constexpr int C = C_RIGHT; CALL; } break; \
        default: { constexpr int C = C_EOE; CALL; } break; \
    }
__device__ __forceinline__ Q31 claimed_of(const CheckReadback* out, u32 k) { const uint4 v = out->claimed[k]; return q_make(v.x, v.y, v.z, v.w); }

__global__ void __launch_bounds__(256) k_check_batch(const CheckBatch* __restrict__ bp, const CheckLaunch* __restrict__ launches) {
    __shared__ CheckShared sh;
    const CheckBatch& b = *bp;
    u32 k = 0;
    while (k + 1 < (u32)N_COMPONENTS && b.blk0[k + 1] <= blockIdx.x) k++;
    const CheckLaunch& a = launches[k];
    const u32 block = blockIdx.x - b.blk0[k];
    const Q31 total_sum = claimed_of(b.out, k);
    CHECK_DISPATCH(k, check_cells_body<C>(a, sh, block, total_sum))
}

// Workgroup k < 13 (one wave): k_check_first of component k. Workgroup 13: the QM31 sum of the 13 claimed sums -> out->total.
__global__ void __launch_bounds__(64) k_check_first_batch(const CheckBatch* __restrict__ bp, const CheckLaunch* __restrict__ launches) {
    const CheckBatch& b = *bp;
    const u32 k = blockIdx.x;
    if (k >= (u32)N_COMPONENTS) {
        if (threadIdx.x != 0) return;
        Q31 t = q_zero();
        for (u32 j = 0; j < (u32)N_COMPONENTS; j++) t = q_add(t, claimed_of(b.out, j));
        b.out->total = make_uint4(t.a.a, t.a.b, t.b.a, t.b.b);
        return;
    }
    const CheckLaunch& a = launches[k];
    const Q31 total_sum = claimed_of(b.out, k);
    CHECK_DISPATCH(k, check_first_body<C>(a, total_sum))
}
#undef CHECK_DISPATCH

void check_batch_init(CheckBatch& b, const u32 log_sizes[N_COMPONENTS], CheckReadback* d_out) {
    b = CheckBatch{};
    u32 blocks = 0;
    for (int k = 0; k < N_COMPONENTS; k++) { b.blk0[k] = blocks; blocks += ((1u << log_sizes[k]) + 255u) / 256u; }      // log_size <= 29: at most 13 * 2^21 workgroups
    b.blk0[N_COMPONENTS] = blocks;
    b.out = d_out;
}
void check_batch_run(hipStream_t stream, const CheckBatch* d_batch, const CheckBatch& h_batch, const CheckLaunch* d_launches) {
    hipLaunchKernelGGL(k_check_batch, dim3(h_batch.blk0[N_COMPONENTS]), dim3(256), 0, stream, d_batch, d_launches);
    hipLaunchKernelGGL(k_check_first_batch, dim3(N_COMPONENTS + 1), dim3(64), 0, stream, d_batch, d_launches);
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
