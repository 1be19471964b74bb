// The constraint program asserted on the TRACE domain (include/bfhip.h "Constraint programs asserted on the trace domain": bfhip_air_check) —
// stwo's `assert_constraints` (constraint_framework/assert.rs: AssertEvaluator over every row of the trace) for any `FrameworkEval`, as ONE
// gfx950 kernel that interprets the program: the generic counterpart of check.hip, which compiles the 13 Brainfuck AIRs in. The prover's sweep
// (air_program.hip) cannot say where a trace is wrong: it folds every constraint into one accumulator under random coefficients, on a domain
// that does not contain the trace's points. This pass has no coefficients, no vanishing polynomial and no accumulator: per constraint, which
// cells of CanonicCoset(log_size) are non-zero.
//
// The interpreter is the core of program_interp.h, which k_air_program runs too: one lane per cell, one wave per workgroup (at the caps the
// register file is 48 KiB per wave: four waves would not fit a workgroup's LDS). A cell of the trace domain is AirTraceRow (trace_row.h,
// shared with witness_program.hip); this file adds what C_BASE / C_EXT do here (AirCheckSink).
#include "api_guard.h"
#include "program_interp.h"
#include "trace_row.h"
#include "../../include/bfhip.h"
#include <cstddef>
#include <cstring>

namespace bf {

static_assert(AIR_MAX_CONSTRAINTS <= 64 && AIR_MAX_CONSTRAINTS <= PROGRAM_LANES, "a lane's mask has one bit per constraint, and lane j reduces constraint j");

// What the kernels write; bfhip_air_check copies it field by field into bfhip_air_check_report.
struct AirCheckReportDev {
    u64 n_bad_cells, first_bad_cell;
    u64 bad_per_constraint[AIR_MAX_CONSTRAINTS], first_cell_per_constraint[AIR_MAX_CONSTRAINTS];
    u32 first_bad_constraint, first_bad_value[4], pad_[3];
};

// Staged in HBM. Addresses are kept as integers: read from address space 4 they arrive in SGPRs and are cast to global pointers.
struct AirCheckLaunch {
    u64 code;            // bf_u32x4[n_instr]
    u64 cols;            // bf_u32x4[n_cols]: {pointer low, pointer high, shift, 0}
    u64 params;          // bf_u32x4[n_params]
    u64 report;          // AirCheckReportDev*
    u32 n_instr, n_m, log_size, n_constraints;
};

// C_BASE / C_EXT set bit j of the lane's 64-bit mask when constraint j is non-zero; nothing leaves early, so the wave stays uniform.
// RECORD: also the lowest failing constraint and its value (a C_BASE constraint as (v, 0, 0, 0)).
template <bool RECORD>
struct AirCheckSink {
    static constexpr bool HAS_Q = true;
    u64 mask = 0;
    u32 ci = 0, first = 0xffffffffu;
    Q31 first_value = q_zero();
    static constexpr u32 OP = AIR_C_BASE;
    __device__ __forceinline__ void op(const bf_u32x4 ins, const u32* m, const u32*) {
        const u32 v = m[ins.z * PROGRAM_LANES];
        if (v != 0) {
            if (RECORD && first == 0xffffffffu) { first = ci; first_value = q_from_m(v); }
            mask |= (u64)1 << ci;
        }
        ci++;
    }
    __device__ __forceinline__ void other(const bf_u32x4 ins, const u32*, const u32* q) {      // AIR_C_EXT: the validator admits nothing else
        const Q31 x = program_q_ld(q, ins.z * PROGRAM_LANES);
        if (!q_is_zero(x)) {
            if (RECORD && first == 0xffffffffu) { first = ci; first_value = x; }
            mask |= (u64)1 << ci;
        }
        ci++;
    }
};

// The program at one cell. `cell` < 2^log_size; every column read is inside its column (a column of shift s is read at cell >> s, and only at
// offset 0).
template <bool RECORD>
__device__ __forceinline__ AirCheckSink<RECORD> air_check_cell(const BF_CONSTANT AirCheckLaunch* a, u32* s_regs, u32 cell) {
    AirCheckSink<RECORD> sink;
    program_run((const BF_CONSTANT bf_u32x4*)a->code, a->n_instr, (const BF_CONSTANT bf_u32x4*)a->cols, (const BF_CONSTANT bf_u32x4*)a->params,
                s_regs + threadIdx.x, s_regs + a->n_m * PROGRAM_LANES + threadIdx.x, AirTraceRow{cell, a->log_size}, sink);
    return sink;
}

// Reduction, after check.hip: the ballot of (mask != 0) decides everything — a wave without a violation issues no atomic, so a valid trace
// costs its loads. A wave with violations takes, per constraint with a bit set anywhere in the wave, a popcount of a ballot and the lowest set
// lane (lanes are in cell order); lane j keeps constraint j's pair. Then one vector atomicAdd and one vector atomicMin over the lanes whose
// constraint was touched (consecutive 8-byte slots of the report), and lane 0 adds the wave's bad cells and lowers first_bad_cell: at most
// 2 * 64 + 2 atomics for a wave in which every constraint fails. Integer atomics only: the report does not depend on the order of arrival.
__global__ void __launch_bounds__(PROGRAM_LANES) k_air_check_cells(const AirCheckLaunch* __restrict__ ap) {
    extern __shared__ u32 s_regs[];
    const BF_CONSTANT AirCheckLaunch* a = (const BF_CONSTANT AirCheckLaunch*)(unsigned long long)ap;
    const u32 n = 1u << a->log_size;
    const u32 base = blockIdx.x * PROGRAM_LANES, lane = threadIdx.x;
    // a domain below one wave (log_size < 6): the lanes past its end evaluate cell 0 and report nothing, so every lane runs the whole program
    const bool live = base + lane < n;
    u64 mask = air_check_cell<false>(a, s_regs, live ? base + lane : 0u).mask;
    if (!live) mask = 0;
    const u64 bad = __ballot(mask != 0);
    if (!bad) return;
    AirCheckReportDev* rep = (AirCheckReportDev*)a->report;
    u32 cnt = 0, lowest = 0;
    const u32 n_constraints = a->n_constraints;
    for (u32 j = 0; j < n_constraints; j++) {
        const u64 b = __ballot(((mask >> j) & 1u) != 0);
        if (b && lane == j) { cnt = (u32)__popcll(b); lowest = (u32)(__ffsll((long long)b) - 1); }
    }
    if (cnt) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&rep->bad_per_constraint[lane]), (unsigned long long)cnt);
        atomicMin(reinterpret_cast<unsigned long long*>(&rep->first_cell_per_constraint[lane]), (unsigned long long)(base + lowest));
    }
    if (lane == 0) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&rep->n_bad_cells), (unsigned long long)__popcll(bad));
        atomicMin(reinterpret_cast<unsigned long long*>(&rep->first_bad_cell), (unsigned long long)(base + (u32)(__ffsll((long long)bad) - 1)));
    }
}

// One wave re-interprets the program at the first bad cell (known once the cells pass has completed: same stream) and writes the lowest
// failing constraint and its value; the report keeps -1 and zeros for a trace without violations. Every lane evaluates the same cell.
__global__ void __launch_bounds__(PROGRAM_LANES) k_air_check_first(const AirCheckLaunch* __restrict__ ap) {
    extern __shared__ u32 s_regs[];
    const BF_CONSTANT AirCheckLaunch* a = (const BF_CONSTANT AirCheckLaunch*)(unsigned long long)ap;
    AirCheckReportDev* rep = (AirCheckReportDev*)a->report;
    const u64 cell = rep->first_bad_cell;
    if (cell >= ((u64)1 << a->log_size)) return;
    const AirCheckSink<true> found = air_check_cell<true>(a, s_regs, (u32)cell);
    const Q31 v = found.first_value;
    if (threadIdx.x == 0) {
        rep->first_bad_constraint = found.first;
        rep->first_bad_value[0] = v.a.a; rep->first_bad_value[1] = v.a.b; rep->first_bad_value[2] = v.b.a; rep->first_bad_value[3] = v.b.b;
    }
}

// "air check: ok", or the headline and one line per failing constraint (include/bfhip.h: bfhip_format_air_check)
static std::string air_check_text(const bfhip_air_check_report& r) {
    if (r.n_bad_cells == 0) return "air check: ok";
    const u32 K = r.n_constraints < AIR_MAX_CONSTRAINTS ? r.n_constraints : AIR_MAX_CONSTRAINTS;
    u32 k = 0;
    for (u32 j = 0; j < K; j++) k += r.bad_per_constraint[j] != 0;
    std::string s = "air check: " + std::to_string(r.n_bad_cells) + " of " + std::to_string((unsigned long long)1 << (r.log_size & 63u)) + " cells violate " +
                    std::to_string(k) + " of " + std::to_string(r.n_constraints) + " constraints";
    for (u32 j = 0; j < K; j++) {
        if (!r.bad_per_constraint[j]) continue;
        s += "\nconstraint " + std::to_string(j) + ": " + std::to_string(r.bad_per_constraint[j]) + " cells, first at cell " + std::to_string(r.first_cell_per_constraint[j]);
        if ((int32_t)j == r.first_bad_constraint)
            s += ", value (" + std::to_string(r.first_bad_value[0]) + ", " + std::to_string(r.first_bad_value[1]) + ", " + std::to_string(r.first_bad_value[2]) + ", " +
                 std::to_string(r.first_bad_value[3]) + ")";
    }
    return s;
}

}  // namespace bf

using namespace bf;

extern "C" int32_t bfhip_air_check(bfhip_ctx* ctx, const bfhip_air* air, uint32_t log_size, const uint32_t* const* cols_h, const uint32_t* col_shifts_h,
                                   const uint32_t* params_h, uint32_t n_params, bfhip_air_check_report* out) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    const std::string me = "bfhip_air_check";
    if (!air || !out || (!cols_h && air->n_cols) || (!params_h && n_params)) throw HipError(me + ": null argument");
    if (c.shard.count > 1) throw HipError(me + ": a context in a shard group is not supported (bfhip_ctx_leave_group first)");
    if (log_size < 1 || log_size > c.tw_root_log + 1) throw HipError(me + ": log_size must be in [1, max_log_domain = " + std::to_string(c.tw_root_log + 1) + "], got " + std::to_string(log_size));
    const ProgramInputs in(me, air->n_cols, cols_h, col_shifts_h, log_size, "log_size", air->col_read_shifted.data(), air->n_params, params_h, n_params);
    AirCheckReportDev init{};
    init.first_bad_cell = ~u64(0);
    init.first_bad_constraint = 0xffffffffu;
    for (u32 j = 0; j < AIR_MAX_CONSTRAINTS; j++) init.first_cell_per_constraint[j] = ~u64(0);
    AirCheckLaunch L{};
    L.n_instr = air->n_instr; L.n_m = air->n_m; L.log_size = log_size; L.n_constraints = air->n_constraints;
    c.stage_checkpoint();
    AirCheckReportDev* d_report = nullptr;
    {
        StageBatch sb(c);
        d_report = c.stage(&init, 1);
        L.report = (u64)d_report;
        L.code = (u64)c.stage(air->code.data(), air->code.size());
        in.stage(c, L.cols, L.params);
        const AirCheckLaunch* d_launch = c.stage(&L, 1);
        sb.end();
        const u32 n = 1u << log_size;
        const size_t lds = sizeof(u32) * PROGRAM_LANES * (air->n_m + 4 * air->n_q);
        ProfScope ps(c.stream, "k_air_check", 0);
        hipLaunchKernelGGL(k_air_check_cells, dim3((n + PROGRAM_LANES - 1) / PROGRAM_LANES), dim3(PROGRAM_LANES), lds, c.stream, d_launch);
        hipLaunchKernelGGL(k_air_check_first, dim3(1), dim3(PROGRAM_LANES), lds, c.stream, d_launch);
    }
    BF_HIP(hipGetLastError());
    AirCheckReportDev r;
    c.read_back(&r, d_report, sizeof r);      // the one host synchronisation of the call
    bfhip_air_check_report o{};
    o.log_size = log_size; o.n_constraints = air->n_constraints;
    o.n_bad_cells = r.n_bad_cells; o.first_bad_cell = r.first_bad_cell;
    o.first_bad_constraint = (int32_t)r.first_bad_constraint;
    for (int w = 0; w < 4; w++) o.first_bad_value[w] = r.first_bad_value[w];
    for (u32 j = 0; j < AIR_MAX_CONSTRAINTS; j++) { o.bad_per_constraint[j] = r.bad_per_constraint[j]; o.first_cell_per_constraint[j] = r.first_cell_per_constraint[j]; }
    *out = o;
    return 0;
    API_CATCH
}

extern "C" int32_t bfhip_format_air_check(const bfhip_air_check_report* rep, char* buf, size_t cap, size_t* need) {
    API_TRY
    if (!rep || (!buf && cap)) throw HipError("bfhip_format_air_check: null argument");
    const std::string s = air_check_text(*rep);
    if (need) *need = s.size() + 1;
    if (cap) {
        const size_t n = s.size() < cap - 1 ? s.size() : cap - 1;
        memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    if (cap < s.size() + 1) { bfhip_set_error("capacity"); return -2; }
    return 0;
    API_CATCH
}
