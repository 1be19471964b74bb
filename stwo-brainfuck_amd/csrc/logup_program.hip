// The fraction program on the trace domain (include/bfhip.h "Fraction programs": bfhip_logup_program_generate) — what a component's
// `interaction_trace_evaluation` does with LogupTraceGenerator::{new_col, write_frac, finalize_col, finalize_last} for any AIR, as four gfx950
// launches that interpret the program instead of one compiled branch per component (air.hip: k_logup_rows). Every cell is distinct: nothing
// here knows of the 16-fold replication the compiled path is built on.
//
// The policy types of the row stage (LogupRow, LogupSink) and the three scan bodies are in logup_domain.h, which says what they do; the batch
// (logup_batch.hip: bfhip_logup_program_generate_batch) runs the same bodies for a whole list of components. This call keeps its own four
// launches over one LogupProgLaunch.
#include "api_guard.h"
#include "logup_domain.h"
#include "../../include/bfhip.h"

namespace bf {

__global__ void __launch_bounds__(PROGRAM_LANES) k_logup_program(const LogupProgLaunch* __restrict__ ap) {
    extern __shared__ u32 s_regs[];
    const BF_CONSTANT LogupProgLaunch* a = (const BF_CONSTANT LogupProgLaunch*)(unsigned long long)ap;
    const u32 cell = blockIdx.x * PROGRAM_LANES + threadIdx.x;
    if (cell >= (1u << a->log_size)) return;
    lp_rows(a, cell, s_regs);
}

__global__ void __launch_bounds__(256) k_logup_program_scan(const LogupProgLaunch* __restrict__ ap) {
    __shared__ uint4 s[256];
    lp_scan_tile(*ap, blockIdx.x, s);
}

__global__ void __launch_bounds__(LP_CHUNK) k_logup_program_totals(const LogupProgLaunch* __restrict__ ap) {
    __shared__ uint4 s[LP_CHUNK];
    lp_scan_totals(*ap, s);
}

__global__ void __launch_bounds__(256) k_logup_program_last(const LogupProgLaunch* __restrict__ ap) {
    const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (1u << ap->log_size)) return;
    lp_last_cell(*ap, c);
}

}  // namespace bf

using namespace bf;

extern "C" int32_t bfhip_logup_program_generate(bfhip_ctx* ctx, const bfhip_logup* lp, uint32_t log_size, const uint32_t* const* cols_h, const uint32_t* col_shifts_h,
                                                const uint32_t* params_h, uint32_t n_params, uint32_t* const* out_cols_h, uint32_t claimed_sum_h[4]) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    const std::string me = "bfhip_logup_program_generate";
    if (!lp || !out_cols_h || !claimed_sum_h || (!cols_h && lp->n_cols) || (!params_h && n_params)) throw HipError("null argument");
    if (c.shard.count > 1) throw HipError(me + ": a context in a shard group is not supported (bfhip_ctx_leave_group first)");
    if (log_size < 1 || log_size > c.tw_root_log + 1 || log_size > 29) throw HipError(me + ": log_size must be in [1, max_log_domain = " + std::to_string(c.tw_root_log + 1) + "], got " + std::to_string(log_size));
    const ProgramInputs in(me, lp->n_cols, cols_h, col_shifts_h, log_size, "log_size", nullptr, lp->n_params, params_h, n_params);
    LogupProgLaunch L{};
    for (u32 k = 0; k < 4 * lp->n_logup_cols; k++) {
        if (!out_cols_h[k]) throw HipError(me + ": null output column pointer (coordinate column " + std::to_string(k) + ")");
        L.out[k] = (u64)out_cols_h[k];
    }
    // scratch, never from the arena (an open session owns it): v[N], wloc[N / 2], totals[nb + 1], tail[2] of 16 bytes each =
    // 24 N + 16 (nb + 3) bytes with nb = ceil(N / 2048) tiles: at most 24 * 2^log_size + 2^log_size / 128 + 64
    const size_t N = size_t(1) << log_size, H = N / 2, nb = (H + LP_TILE - 1) / LP_TILE;
    const size_t bytes = sizeof(uint4) * (N + H + nb + 1 + 2);
    uint4 tail[2];
    DeviceScratch owner(c);
    uint4* scratch = nullptr;
    if (hipError_t e = owner.try_alloc(&scratch, bytes); e != hipSuccess)
        throw HipError(me + ": cannot allocate " + std::to_string(bytes) + " bytes of scratch (" + hipGetErrorString(e) + ")");
    L.v = (u64)scratch; L.wloc = (u64)(scratch + N); L.totals = (u64)(scratch + N + H); L.tail = (u64)(scratch + N + H + nb + 1);
    L.n_instr = lp->n_instr; L.n_m = lp->n_m; L.log_size = log_size; L.n_logup_cols = lp->n_logup_cols; L.nb = (u32)nb;
    c.stage_checkpoint();
    BF_HIP(hipMemsetAsync((void*)L.tail, 0xFF, 2 * sizeof(uint4), c.stream));
    {
        StageBatch sb(c);
        L.code = (u64)c.stage(lp->code.data(), lp->code.size());
        in.stage(c, L.cols, L.params);
        const LogupProgLaunch* d_launch = c.stage(&L, 1);
        sb.end();
        const size_t lds = sizeof(u32) * PROGRAM_LANES * (lp->n_m + 4 * lp->n_q);
        { ProfScope ps(c.stream, "k_logup_program", 0); hipLaunchKernelGGL(k_logup_program, dim3((u32)((N + PROGRAM_LANES - 1) / PROGRAM_LANES)), dim3(PROGRAM_LANES), lds, c.stream, d_launch); }
        ProfScope ps(c.stream, "k_logup_program_scan", 0);
        hipLaunchKernelGGL(k_logup_program_scan, dim3((u32)nb), dim3(256), 0, c.stream, d_launch);
        hipLaunchKernelGGL(k_logup_program_totals, dim3(1), dim3(LP_CHUNK), 0, c.stream, d_launch);
        hipLaunchKernelGGL(k_logup_program_last, dim3((u32)((N + 255) / 256)), dim3(256), 0, c.stream, d_launch);
    }
    BF_HIP(hipGetLastError());
    c.read_back(tail, (const void*)L.tail, sizeof tail);
    const u64 key = ((u64)tail[1].y << 32) | tail[1].x;
    if (key != ~u64(0)) throw HipError(me + ": fraction " + std::to_string(key & 0xFF) + " has a zero denominator at cell " + std::to_string(key >> 8));
    claimed_sum_h[0] = tail[0].x; claimed_sum_h[1] = tail[0].y; claimed_sum_h[2] = tail[0].z; claimed_sum_h[3] = tail[0].w;
    return 0;
    API_CATCH
}
