// C ABI (include/bfhip.h): the 13 built-in components — their shapes, the logUp generation and the constraint evaluation of one component,
// and the AIRs asserted on the trace domain (check.hip) for one component or a whole resident trace.
#include "../../include/bfhip.h"
#include "api_guard.h"
#include "api_args.h"
#include "pcs_types.h"
#include "prover.h"
#include <vector>

using namespace bf;

static Lookups lookups_from_h(const uint32_t v[24]) {
    Lookups el;
    el.memory = make_lookup(q_make(v[0], v[1], v[2], v[3]), q_make(v[4], v[5], v[6], v[7]));
    el.instruction = make_lookup(q_make(v[8], v[9], v[10], v[11]), q_make(v[12], v[13], v[14], v[15]));
    el.processor = make_lookup(q_make(v[16], v[17], v[18], v[19]), q_make(v[20], v[21], v[22], v[23]));
    return el;
}
// check_report_init / check_report_fill / check_launch_of / check_logup_launches / default_check_lookups: prover.h (shared with a proof's preflight)
static void check_not_sharded(const Ctx& c) {
    if (c.shard.count > 1) throw HipError("constraint check: a context in a shard group is not supported (bfhip_ctx_leave_group first)");
}

extern "C" {

int32_t bfhip_component_shape(int32_t component, uint32_t* n_main, uint32_t* n_logup, uint32_t* n_cons) {
    API_TRY
    if (component < 0 || component >= N_COMPONENTS) throw HipError("unknown component");
    if (n_main) *n_main = n_main_cols(component);
    if (n_logup) *n_logup = n_logup_cols(component);
    if (n_cons) *n_cons = n_constraints(component);
    return 0;
    API_CATCH
}
int32_t bfhip_logup_generate(bfhip_ctx* ctx, int32_t component, uint32_t log_size, const uint32_t* const* main_rows_h, const uint32_t lookup_h[24],
                             uint32_t* const* out_cols_h, uint32_t claimed_sum_h[4]) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    check_component(component, log_size, &c);
    u32 log_rows = log_size - LOG_N_LANES;
    size_t M = size_t(1) << log_rows;
    LogupLaunch L{};
    for (u32 j = 0; j < n_main_cols(component); j++) L.cols[j] = main_rows_h[j];
    u32 nl = n_logup_cols(component);
    for (u32 q = 0; q + 1 < nl; q++) for (int w = 0; w < 4; w++) L.out_rep[4 * q + w] = out_cols_h[4 * q + w];
    for (int w = 0; w < 4; w++) L.out_last[w] = out_cols_h[4 * (nl - 1) + w];
    // scratch: vrow[M], wloc[M], totals[M / 1024 + 2], claimed[1]
    size_t n_tot = M / 1024 + 2;
    uint4 r;      // declared before the guard: the copy into it has completed when it goes
    DeviceScratch owner(c);
    uint4* scratch = nullptr;
    owner.alloc(&scratch, sizeof(uint4) * (2 * M + n_tot + 1));
    L.vrow = scratch; L.wloc = scratch + M; L.totals = scratch + 2 * M; L.claimed = scratch + 2 * M + n_tot;
    L.el = lookups_from_h(lookup_h); L.log_rows = log_rows; L.comp = component;
    {
        LogupBatch lb;
        logup_batch_init(lb, L.el, &L, 1);
        c.stage_checkpoint();
        logup_batch_run(c.stream, c.stage(&lb, 1), lb);
    }
    BF_HIP(hipGetLastError());
    read_q31(c, (const uint4*)L.claimed, r, claimed_sum_h);
    return 0;
    API_CATCH
}
int32_t bfhip_eval_constraints(bfhip_ctx* ctx, int32_t component, uint32_t log_size, const uint32_t* is_first_d, const uint32_t* const* main_lde_h,
                               const uint32_t* main_shifts_h, const uint32_t* const* inter_lde_h, const uint32_t* inter_shifts_h, const uint32_t lookup_h[24],
                               const uint32_t claimed_sum_h[4], const uint32_t* coeffs_h, uint32_t* const acc_d[4]) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    check_component(component, log_size, &c, 1);
    u32 eval_log = log_size + 1;
    ConstraintLaunch L{};
    L.is_first = is_first_d;
    for (u32 j = 0; j < n_main_cols(component); j++) L.trace[j] = ColDesc{main_lde_h[j], main_shifts_h ? main_shifts_h[j] : 0u, 0};
    for (u32 j = 0; j < 4 * n_logup_cols(component); j++) L.inter[j] = ColDesc{inter_lde_h[j], inter_shifts_h ? inter_shifts_h[j] : 0u, 0};
    for (int w = 0; w < 4; w++) L.acc[w] = acc_d[w];
    for (u32 j = 0; j < n_constraints(component); j++) L.coeff[j] = q_from_h(coeffs_h + 4 * j);
    L.el = lookups_from_h(lookup_h); L.total_sum = q_from_h(claimed_sum_h); L.log_size = log_size;
    // 1 / coset_vanishing(CanonicCoset(log_size).coset, eval_domain.at(i)) takes two values, by the parity of the (bit-reversed) cell index
    for (u32 i = 0; i < 2; i++) L.denom_inv[i] = m_inv(coset_vanishing_m(log_size, canonic_domain_at(eval_log, i)));
    c.stage_checkpoint();
    eval_constraints(c.stream, component, c.stage(&L, 1), log_size, 0, constraint_group_rows(L, component));
    BF_HIP(hipGetLastError());
    return 0;
    API_CATCH
}
int32_t bfhip_check_constraints(bfhip_ctx* ctx, int32_t component, uint32_t log_size, const uint32_t* const* main_rows_h, const uint32_t* const* logup_cols_h,
                                const uint32_t lookup_h[24], const uint32_t claimed_sum_h[4], bfhip_check_report* out) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    check_component(component, log_size);
    if (!main_rows_h || !logup_cols_h || !lookup_h || !claimed_sum_h || !out) throw HipError("null argument");
    for (u32 j = 0; j < n_main_cols(component); j++) if (!main_rows_h[j]) throw HipError("null main column pointer");
    for (u32 j = 0; j < 4 * n_logup_cols(component); j++) if (!logup_cols_h[j]) throw HipError("null logUp column pointer");
    check_not_sharded(c);
    c.refuse_in_session("bfhip_check_constraints");
    const Q31 claimed = q_from_h(claimed_sum_h);
    const CheckReportDev init = check_report_init();
    c.stage_checkpoint();
    CheckReportDev* d_report = c.stage(&init, 1);
    const CheckLaunch L = check_launch_of(component, log_size, main_rows_h, logup_cols_h, lookups_from_h(lookup_h), claimed, d_report);
    {
        ProfScope ps(c.stream, "k_check_cells", 0);
        check_constraints_launch(c.stream, component, c.stage(&L, 1), log_size);
    }
    BF_HIP(hipGetLastError());
    CheckReportDev r;
    c.read_back(&r, d_report, sizeof r);
    check_report_fill(*out, r, component, log_size, claimed);
    return 0;
    API_CATCH
}
int32_t bfhip_trace_check(bfhip_ctx* ctx, const bfhip_trace* trace, const uint32_t* lookup_h, bfhip_check_report out[13], uint32_t logup_total_h[4],
                          int32_t* n_bad_components) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    if (!trace || !out || !logup_total_h) throw HipError("null argument");
    check_not_sharded(c);
    c.refuse_in_session("bfhip_trace_check");
    Lookups el;
    if (lookup_h) el = lookups_from_h(lookup_h);
    else {
        el = default_check_lookups();
    }
    const u32* rows[N_COMPONENTS][13] = {};
    u32 log_sizes[N_COMPONENTS];
    trace_columns(trace, rows, log_sizes);
    // like a proof: nothing of this context is in flight, and its per-proof memory starts empty
    c.sync();
    c.arena.reset();
    c.stage_checkpoint();
    uint4* d_claimed = (uint4*)c.arena.alloc(sizeof(uint4) * N_COMPONENTS);
    for (int k = 0; k < N_COMPONENTS; k++) if (log_sizes[k] < LOG_N_LANES || log_sizes[k] > 29) throw HipError("trace: component log_size out of range");
    const u32* inter[N_COMPONENTS][12] = {};
    const std::vector<LogupLaunch> logups = check_logup_launches(c, rows, log_sizes, d_claimed, inter);
    {
        LogupBatch lb;
        logup_batch_init(lb, el, logups.data(), N_COMPONENTS);
        const LogupBatch* d_lb = c.stage(&lb, 1);
        ProfScope ps(c.stream, "trace_check_logup", 0);      // bfhip_profile_enable mode 1: the two halves of a check, by HIP events (tools/trace_check_rate.py)
        logup_batch_run(c.stream, d_lb, lb);
    }
    BF_HIP(hipGetLastError());
    uint4 claimed_h[N_COMPONENTS];
    c.read_back(claimed_h, d_claimed, sizeof claimed_h);
    Q31 claimed[N_COMPONENTS], total = q_zero();
    CheckReportDev reports[N_COMPONENTS];
    for (int k = 0; k < N_COMPONENTS; k++) {
        claimed[k] = q_make(claimed_h[k].x, claimed_h[k].y, claimed_h[k].z, claimed_h[k].w);
        total = q_add(total, claimed[k]);
        reports[k] = check_report_init();
    }
    CheckLaunch launches[N_COMPONENTS];
    const CheckLaunch* d_launches = nullptr;
    CheckReportDev* d_reports = nullptr;
    {
        StageBatch sb(c);
        d_reports = c.stage(reports, N_COMPONENTS);
        for (int k = 0; k < N_COMPONENTS; k++) launches[k] = check_launch_of(k, log_sizes[k], rows[k], inter[k], el, claimed[k], d_reports + k);
        d_launches = c.stage(launches, N_COMPONENTS);
        sb.end();
    }
    {
        ProfScope ps(c.stream, "k_check_cells", 0);
        for (int k = 0; k < N_COMPONENTS; k++) check_constraints_launch(c.stream, k, d_launches + k, log_sizes[k]);
    }
    BF_HIP(hipGetLastError());
    c.read_back(reports, d_reports, sizeof reports);
    int32_t n_bad = 0;
    for (int k = 0; k < N_COMPONENTS; k++) { check_report_fill(out[k], reports[k], k, log_sizes[k], claimed[k]); n_bad += reports[k].n_bad_cells != 0; }
    q31_words(total, logup_total_h);
    if (n_bad_components) *n_bad_components = n_bad;
    return 0;
    API_CATCH
}

}  // extern "C"
