// The fraction programs of ALL components of an AIR on their trace domains, in one call (include/bfhip.h "Fraction programs, batched":
// bfhip_logup_program_generate_batch) — the calls prove makes to every component's `interaction_trace_evaluation`, as the frozen Brainfuck
// path batches its 13 (air.hip: LogupBatch), on the interpreter of program_interp.h and the bodies of logup_domain.h.
//
// One LogupProgLaunch per component, as the single call stages it, in one array. Row stage (k_logup_program_batch): a workgroup is one wave
// and owns 64 consecutive cells of one component, which it finds from blockIdx.x in a segment table (uniform addresses: scalar loads, as
// k_air_compose finds its bucket); ONE launch for all components, sized for the largest program of the list, unless that LDS would lower the
// occupancy of a component of 2^16 cells and more, which then gets a launch sized for its own program (logup_batch_plan.h has the rule,
// DESIGN.md section 9o the measurement). Scan stage, three launches for the whole list:
// tiles (k_logup_batch_scan: a workgroup finds its component and tile in a prefix table), totals (k_logup_batch_totals: workgroup k scans
// component k's tile totals), last column (k_logup_batch_last: a workgroup finds its component and 256-cell block in a prefix table).
// Scratch: one hipMalloc that lives for the call — the arena may belong to an open session — laid out by the plan; one read-back of
// {claimed sum, zero-denominator key} per component.
#include "api_guard.h"
#include "logup_domain.h"
#include "logup_batch_plan.h"
#include "../../include/bfhip.h"
#include <cstring>
#include <map>

namespace bf {

// The entry k of a non-decreasing table with table[k] <= b < table[k + 1] (the last entry if none follows), through scalar loads
__device__ __forceinline__ u32 lp_find(const BF_CONSTANT u32* table, u32 n, u32 b) {
    u32 k = 0;
    while (k + 1 < n && b >= table[k + 1]) k++;
    return k;
}

__global__ void __launch_bounds__(PROGRAM_LANES) k_logup_program_batch(const LogupProgLaunch* __restrict__ lp, const LogupBatchSeg* __restrict__ sp, u32 n_segs) {
    extern __shared__ u32 s_regs[];
    const BF_CONSTANT LogupBatchSeg* segs = (const BF_CONSTANT LogupBatchSeg*)(unsigned long long)sp;
    u32 k = 0;
    while (k + 1 < n_segs && blockIdx.x >= segs[k + 1].block0) k++;
    const BF_CONSTANT LogupProgLaunch* a = (const BF_CONSTANT LogupProgLaunch*)(unsigned long long)(lp + segs[k].comp);
    const u32 cell = (blockIdx.x - segs[k].block0) * PROGRAM_LANES + threadIdx.x;
    if (cell >= (1u << a->log_size)) return;      // the last wave of a component of fewer than 64 cells
    lp_rows(a, cell, s_regs);
}

__global__ void __launch_bounds__(256) k_logup_batch_scan(const LogupProgLaunch* __restrict__ lp, const u32* __restrict__ tile0, u32 n) {
    __shared__ uint4 s[256];
    const BF_CONSTANT u32* t = (const BF_CONSTANT u32*)(unsigned long long)tile0;
    const u32 k = lp_find(t, n, blockIdx.x);
    lp_scan_tile(lp[k], blockIdx.x - t[k], s);
}

__global__ void __launch_bounds__(LP_CHUNK) k_logup_batch_totals(const LogupProgLaunch* __restrict__ lp) {
    __shared__ uint4 s[LP_CHUNK];
    lp_scan_totals(lp[blockIdx.x], s);
}

__global__ void __launch_bounds__(256) k_logup_batch_last(const LogupProgLaunch* __restrict__ lp, const u32* __restrict__ block0, u32 n) {
    const BF_CONSTANT u32* t = (const BF_CONSTANT u32*)(unsigned long long)block0;
    const u32 k = lp_find(t, n, blockIdx.x);
    const u32 c = (blockIdx.x - t[k]) * 256 + threadIdx.x;
    if (c >= (1u << lp[k].log_size)) return;
    lp_last_cell(lp[k], c);
}

}  // namespace bf

using namespace bf;

extern "C" int32_t bfhip_logup_program_generate_batch(bfhip_ctx* ctx, const bfhip_logup_component* comps, uint32_t n, uint32_t* claimed_sums_h, uint32_t total_h[4]) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    const std::string me = "bfhip_logup_program_generate_batch";
    if (!comps || !claimed_sums_h) throw HipError(me + ": null argument");
    if (n < 1 || n > BFHIP_LOGUP_BATCH_MAX_COMPONENTS) throw HipError(me + ": 1 to BFHIP_LOGUP_BATCH_MAX_COMPONENTS (64) components, got " + std::to_string(n));
    if (c.shard.count > 1) throw HipError(me + ": a context in a shard group is not supported (bfhip_ctx_leave_group first)");

    // ---- every rule about every component, before anything is staged or enqueued -------------------------------------------------------
    std::vector<ProgramInputs> inputs;
    inputs.reserve(n);
    std::vector<u32> log_sizes(n);
    std::vector<size_t> lds(n);
    std::vector<LogupBatchRange> ranges;
    u64 cells = 0;
    for (u32 k = 0; k < n; k++) {
        const bfhip_logup_component& p = comps[k];
        const std::string mk = me + ": component " + std::to_string(k);
        if (p.reserved != 0) throw HipError(mk + ": reserved must be 0");
        const bfhip_logup* lp = p.program;
        if (!lp || !p.out_cols_h || (!p.cols_h && lp->n_cols) || (!p.params_h && p.n_params)) throw HipError(mk + ": null argument");
        if (p.log_size < 1 || p.log_size > c.tw_root_log + 1 || p.log_size > 29) throw HipError(mk + ": log_size must be in [1, max_log_domain = " + std::to_string(c.tw_root_log + 1) + "], got " + std::to_string(p.log_size));
        inputs.emplace_back(mk, lp->n_cols, p.cols_h, p.col_shifts_h, p.log_size, "log_size", nullptr, lp->n_params, p.params_h, p.n_params);
        for (u32 j = 0; j < 4 * lp->n_logup_cols; j++) {
            if (!p.out_cols_h[j]) throw HipError(mk + ": null output column pointer (coordinate column " + std::to_string(j) + ")");
            ranges.push_back(LogupBatchRange{(u64)p.out_cols_h[j], (u64)p.out_cols_h[j] + (u64(4) << p.log_size), k, true});
        }
        for (u32 j = 0; j < lp->n_cols; j++) {
            const u32 s = p.col_shifts_h ? p.col_shifts_h[j] : 0u;
            ranges.push_back(LogupBatchRange{(u64)p.cols_h[j], (u64)p.cols_h[j] + (u64(4) << (p.log_size - s)), k, false});
        }
        log_sizes[k] = p.log_size;
        cells += u64(1) << p.log_size;
        lds[k] = sizeof(u32) * PROGRAM_LANES * (lp->n_m + 4 * lp->n_q);
    }
    {
        LogupBatchRange a{}, b{};
        if (logup_batch_overlap(ranges, a, b)) {
            const auto what = [](const LogupBatchRange& r) { return std::string(r.output ? "an output column" : "an input column") + " of component " + std::to_string(r.comp); };
            throw HipError(me + ": " + what(a) + " overlaps " + what(b) + " (every output column is written while other components still read and write theirs)");
        }
    }

    // a launch has fewer than 2^32 threads; the last-column launch has one per cell of the list, rounded up to 256 per component
    if (cells > (u64(1) << 31)) throw HipError(me + ": the list has " + std::to_string(cells) + " cells, a call takes at most 2^31 = 2147483648");

    // BFHIP_LOGUP_BATCH_LAUNCH=one / each / size: A/B knob of tools/logup_batch_rate.py — one row-stage launch for all / one per component /
    // every component of 2^16 cells and more alone (the same words)
    static const int launch_mode = [] {
        const char* v = getenv("BFHIP_LOGUP_BATCH_LAUNCH");
        return !v ? 0 : !strcmp(v, "one") ? 1 : !strcmp(v, "each") ? 2 : !strcmp(v, "size") ? 3 : 0;
    }();
    const LogupBatchPlan plan = logup_batch_plan(log_sizes.data(), lds.data(), n, launch_mode);

    // ---- what the call stages, every block rounded as Ctx::stage does ------------------------------------------------------------------
    size_t need = 0;
    {
        std::map<const bfhip_logup*, int> seen;
        for (u32 k = 0; k < n; k++) {
            if (seen.emplace(comps[k].program, 0).second) need += Ctx::stage_round(sizeof(u32) * comps[k].program->code.size());
            need += Ctx::stage_round(sizeof(u32) * inputs[k].cols.size()) + Ctx::stage_round(16 * (size_t)std::max(comps[k].n_params, 1u));
        }
        need += Ctx::stage_round(sizeof(LogupProgLaunch) * n) + Ctx::stage_round(sizeof(LogupBatchSeg) * plan.segs.size()) + 2 * Ctx::stage_round(sizeof(u32) * (n + 1));
    }
    if (need > c.stage_bytes) throw HipError(me + ": the list stages " + std::to_string(need) + " bytes, the context's staging ring holds " + std::to_string(c.stage_bytes));

    // scratch, never from the arena (an open session owns it): every component's v, wloc and totals as the single call has them, then the
    // 2 n tail words: exactly the sum of the single calls' allocations, each of which is within its stated bound
    std::vector<uint4> tails(2 * (size_t)n);
    DeviceScratch owner(c);
    char* scratch = nullptr;
    if (hipError_t e = owner.try_alloc(&scratch, plan.bytes); e != hipSuccess)
        throw HipError(me + ": cannot allocate " + std::to_string(plan.bytes) + " bytes of scratch (" + hipGetErrorString(e) + ")");
    c.stage_checkpoint(need);
    BF_HIP(hipMemsetAsync(scratch + plan.tails, 0xFF, 32 * (size_t)n, c.stream));
    {
        StageBatch sb(c);
        std::map<const bfhip_logup*, u64> code_d;      // equal programs are staged once
        std::vector<LogupProgLaunch> L(n);
        for (u32 k = 0; k < n; k++) {
            const bfhip_logup* lp = comps[k].program;
            auto it = code_d.find(lp);
            if (it == code_d.end()) it = code_d.emplace(lp, (u64)c.stage(lp->code.data(), lp->code.size())).first;
            L[k].code = it->second;
            inputs[k].stage(c, L[k].cols, L[k].params);
            for (u32 j = 0; j < 4 * lp->n_logup_cols; j++) L[k].out[j] = (u64)comps[k].out_cols_h[j];
            const LogupBatchScratch& s = plan.scratch[k];
            L[k].v = (u64)(scratch + s.v); L[k].wloc = (u64)(scratch + s.wloc); L[k].totals = (u64)(scratch + s.totals);
            L[k].tail = (u64)(scratch + plan.tails + 32 * (size_t)k);
            L[k].n_instr = lp->n_instr; L[k].n_m = lp->n_m; L[k].log_size = log_sizes[k]; L[k].n_logup_cols = lp->n_logup_cols; L[k].nb = s.nb;
        }
        const LogupProgLaunch* d_launch = c.stage(L.data(), L.size());
        const LogupBatchSeg* d_segs = c.stage(plan.segs.data(), plan.segs.size());
        const u32* d_tile0 = c.stage(plan.tile0.data(), plan.tile0.size());
        const u32* d_block0 = c.stage(plan.block0.data(), plan.block0.size());
        sb.end();
        for (const LogupBatchGroup& g : plan.groups) {
            ProfScope ps(c.stream, "k_logup_program_batch", 0);
            hipLaunchKernelGGL(k_logup_program_batch, dim3(g.blocks), dim3(PROGRAM_LANES), g.lds, c.stream, d_launch, d_segs + g.first, (u32)g.count);
        }
        ProfScope ps(c.stream, "k_logup_batch_scan", 0);
        hipLaunchKernelGGL(k_logup_batch_scan, dim3(plan.tile0[n]), dim3(256), 0, c.stream, d_launch, d_tile0, n);
        hipLaunchKernelGGL(k_logup_batch_totals, dim3(n), dim3(LP_CHUNK), 0, c.stream, d_launch);
        hipLaunchKernelGGL(k_logup_batch_last, dim3(plan.block0[n]), dim3(256), 0, c.stream, d_launch, d_block0, n);
    }
    BF_HIP(hipGetLastError());
    c.read_back(tails.data(), scratch + plan.tails, 32 * (size_t)n);
    u32 total[4] = {0, 0, 0, 0};
    for (u32 k = 0; k < n; k++) {
        const u64 key = ((u64)tails[2 * k + 1].y << 32) | tails[2 * k + 1].x;
        if (key != ~u64(0)) throw HipError(me + ": component " + std::to_string(k) + ": fraction " + std::to_string(key & 0xFF) + " has a zero denominator at cell " + std::to_string(key >> 8));
    }
    for (u32 k = 0; k < n; k++) {
        const u32 w[4] = {tails[2 * k].x, tails[2 * k].y, tails[2 * k].z, tails[2 * k].w};
        for (int j = 0; j < 4; j++) { claimed_sums_h[4 * k + j] = w[j]; total[j] = m_add(total[j], w[j]); }
    }
    if (total_h) memcpy(total_h, total, sizeof total);
    return 0;
    API_CATCH
}
