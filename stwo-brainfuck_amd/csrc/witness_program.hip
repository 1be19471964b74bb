// The witness program on the TRACE domain (include/bfhip.h "Witness programs": bfhip_witness_program_generate) — the columns an AIR's author
// computes row by row from the ones they have, derived where the inputs already are: ONE gfx950 kernel that interprets the program at every
// cell of CanonicCoset(log_size) and stores the output columns. The Brainfuck tables have hand-written builders for this (tables.hip); an AIR
// the library has never seen has this.
//
// The interpreter is the core of program_interp.h, on the row of k_air_check_cells (trace_row.h): one lane per cell, one wave per workgroup,
// the register file in dynamic LDS sized from the registers the program uses. This file adds what the own opcodes do (WitnessSink). Every
// value a program can produce is a canonical M31 word when its inputs are, so there is no failure, no report and no read-back: a lane never
// leaves early and the wave stays uniform.
#include "api_guard.h"
#include "api_args.h"
#include "program_interp.h"
#include "trace_row.h"
#include "witness_program.h"
#include "rows_index.h"
#include "../../include/bfhip.h"

namespace bf {

// Staged in HBM. Addresses are kept as integers: read from address space 4 they arrive in SGPRs and are cast to global pointers.
struct WitnessLaunch {
    u64 code;            // bf_u32x4[n_instr]
    u64 cols;            // bf_u32x4[n_cols]: {pointer low, pointer high, 0, 0} — every input is a full-size column
    u64 args;            // u32[n_args]
    u64 outs;            // u64[n_out]: the output columns
    u32 n_instr, n_m, log_size, pad_;
};

// WIT_STORE is the family's case of the one switch; the seven opcodes that write a register share `other`. The opcode, the operands' register
// numbers, the arg and the output pointer are the same for every lane (scalar loads, scalar branches); a STORE is one store of the lane's own
// cell, 64 consecutive words per wave.
struct WitnessSink {
    static constexpr bool HAS_Q = false;
    static constexpr u32 OP = WIT_STORE;
    const BF_CONSTANT u32* args;
    const BF_CONSTANT u64* outs;
    u32 cell, row;
    bool live;
    __device__ __forceinline__ void op(const bf_u32x4 ins, const u32* m, const u32*) {
        if (live) ((g_u32p)outs[ins.y])[cell] = m[ins.z * PROGRAM_LANES];
    }
    __device__ __forceinline__ void other(const bf_u32x4 ins, u32* m, const u32*) {
        const u32 op = ins.x;
        u32 a = 0, b = ins.w, arg = 0;
        if (op == WIT_ARG) arg = args[ins.z];
        else if (op != WIT_ROW) a = m[ins.z * PROGRAM_LANES];
        if (op == WIT_LT) b = m[ins.w * PROGRAM_LANES];
        m[ins.y * PROGRAM_LANES] = wit_value(op, a, b, arg, row);
    }
};

__global__ void __launch_bounds__(PROGRAM_LANES) k_witness_program(const WitnessLaunch* __restrict__ ap) {
    extern __shared__ u32 s_regs[];
    const BF_CONSTANT WitnessLaunch* a = (const BF_CONSTANT WitnessLaunch*)(unsigned long long)ap;
    const u32 log_size = a->log_size, n = 1u << log_size;
    // a domain below one wave (log_size < 6): the lanes past its end evaluate cell 0 and store nothing, so every lane runs the whole program
    const bool live = blockIdx.x * PROGRAM_LANES + threadIdx.x < n;
    const u32 cell = live ? blockIdx.x * PROGRAM_LANES + threadIdx.x : 0u;
    WitnessSink sink{(const BF_CONSTANT u32*)a->args, (const BF_CONSTANT u64*)a->outs, cell, rows_row_of_cell(log_size, cell), live};
    program_run((const BF_CONSTANT bf_u32x4*)a->code, a->n_instr, (const BF_CONSTANT bf_u32x4*)a->cols, (const BF_CONSTANT bf_u32x4*)nullptr,
                s_regs + threadIdx.x, (u32*)nullptr, AirTraceRow{cell, log_size}, sink);
}

}  // namespace bf

using namespace bf;

extern "C" int32_t bfhip_witness_program_generate(bfhip_ctx* ctx, const bfhip_witness_program* wp, uint32_t log_size, const uint32_t* const* cols_h,
                                                  const uint32_t* args_h, uint32_t n_args, uint32_t* const* out_cols_h, uint32_t n_out) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    const std::string who = "bfhip_witness_program_generate: ";
    if (!wp || !out_cols_h || (!cols_h && wp->n_cols) || (!args_h && n_args)) throw HipError(who + "null argument");
    if (c.shard.count > 1) throw HipError(who + "a context in a shard group is not supported (bfhip_ctx_leave_group first)");
    if (log_size < 1 || log_size > c.tw_root_log + 1)
        throw HipError(who + "log_size must be in [1, max_log_domain = " + std::to_string(c.tw_root_log + 1) + "], got " + std::to_string(log_size));
    if (n_out != wp->n_out) throw HipError(who + std::to_string(n_out) + " output columns, the program has " + std::to_string(wp->n_out));
    if (n_args != wp->n_args) throw HipError(who + std::to_string(n_args) + " args, the program has " + std::to_string(wp->n_args));
    for (u32 k = 0; k < n_args; k++)
        if (args_h[k] >= P31) throw HipError(who + "arg " + std::to_string(k) + ": " + std::to_string(args_h[k]) + " is not a canonical M31 value");
    const u64 col_bytes = sizeof(u32) << log_size;
    std::vector<ByteRange> used;      // the inputs first, then the output columns accepted so far
    std::vector<u32> cols(4 * (size_t)(wp->n_cols ? wp->n_cols : 1), 0u);      // one zero descriptor where there is no column
    for (u32 j = 0; j < wp->n_cols; j++) {
        if (!cols_h[j]) throw HipError(who + "input column " + std::to_string(j) + " is a null pointer");
        const u64 p = (u64)(uintptr_t)cols_h[j];
        cols[4 * j] = (u32)p; cols[4 * j + 1] = (u32)(p >> 32);
        used.push_back({p, col_bytes, "input column " + std::to_string(j)});
    }
    std::vector<u64> outs(n_out);
    for (u32 k = 0; k < n_out; k++) {
        if (!out_cols_h[k]) throw HipError(who + "output column " + std::to_string(k) + " is a null pointer");
        const ByteRange out{(u64)(uintptr_t)out_cols_h[k], col_bytes, "output column " + std::to_string(k)};
        for (const ByteRange& u : used) if (out.overlaps(u)) throw HipError(who + out.name + " overlaps " + u.name);
        used.push_back(out);
        outs[k] = out.base;
    }
    const u32 zero_arg = 0;
    c.stage_checkpoint(Ctx::stage_round(sizeof(u32) * wp->code.size()) + Ctx::stage_round(sizeof(u32) * cols.size()) + Ctx::stage_round(sizeof(u64) * n_out) +
                       Ctx::stage_round(sizeof(u32) * (n_args + 1)) + Ctx::stage_round(sizeof(WitnessLaunch)));
    WitnessLaunch L{};
    L.n_instr = wp->n_instr; L.n_m = wp->n_m; L.log_size = log_size;
    {
        StageBatch sb(c);
        L.code = (u64)c.stage(wp->code.data(), wp->code.size());
        L.cols = (u64)c.stage(cols.data(), cols.size());
        L.args = (u64)(n_args ? c.stage(args_h, n_args) : c.stage(&zero_arg, 1));
        L.outs = (u64)c.stage(outs.data(), outs.size());
        const WitnessLaunch* d_launch = c.stage(&L, 1);
        sb.end();
        const u32 n = 1u << log_size;
        ProfScope ps(c.stream, "k_witness_program", (u64)(wp->n_cols + n_out) * col_bytes);
        hipLaunchKernelGGL(k_witness_program, dim3((n + PROGRAM_LANES - 1) / PROGRAM_LANES), dim3(PROGRAM_LANES), sizeof(u32) * PROGRAM_LANES * wp->n_m, c.stream, d_launch);
    }
    BF_HIP(hipGetLastError());
    return 0;
    API_CATCH
}
