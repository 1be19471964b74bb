// A proof's preflight (include/bfhip.h: bfhip_ctx_set_preflight): bfhip_trace_check's assertion of the 13 AIRs and of the logUp total, run
// by HipProver::prove on its row-granular tables before anything of the main-trace phase is enqueued, so that a trace that cannot be proved
// is refused with the failing row and tuple instead of costing a proof that ends in "ConstraintsNotSatisfied" — or, for lookups that do not
// balance, in a proof that only a verifier rejects.
//
// A FILTER, NOT A SOUNDNESS GATE. The lookup elements are the fixed, public defaults of bfhip_trace_check(.., NULL, ..): a trace built to
// cancel under them passes, and then ends as it does without the preflight. Soundness is the verifier's.
//
// Passing path: logup_batch_run (4 launches) + check_batch_run (2 launches, check.hip) + ONE read-back of a CheckReadback: the 13 reports,
// the 13 claimed sums and their sum. The claimed sums never visit the host in between: the kernels read them from the slot the logUp pass
// wrote. Scratch (logUp columns, scans) is taken from the proof's arena above a mark and given back before the main-trace phase allocates,
// so the proof's own allocations land where they land without the preflight.
// This file also holds the report's text (bfhip_format_preflight, host only) and the C entry points of the switch.
#include "prover.h"
#include "api_guard.h"
#include <cstdio>

namespace bf {

static const char* const COMPONENT_NAME[N_COMPONENTS] = {"memory", "instruction", "program", "processor", "jnz", "jz", "input", "left", "minus", "output", "plus", "right",
                                                         "end_of_execution"};
static const char* const RELATION_NAME[3] = {"memory", "instruction", "processor"};

static std::string words_text(const uint32_t* w, u32 n) {
    std::string s;
    for (u32 i = 0; i < n; i++) { if (i) s += ", "; s += std::to_string(w[i]); }
    return s;
}

// The wording of the Python mirror's format_check_failure, CheckResult.failures(), format_relation_entry and RelationResult.lines()
// (tests/test_preflight_cpu.py compares the two on canned reports).
std::string preflight_text(const bfhip_preflight_report& r) {
    if (!r.ran) return "preflight: did not run";
    if (!r.rejected) return "preflight: ok";
    const bool total_bad = r.logup_total[0] || r.logup_total[1] || r.logup_total[2] || r.logup_total[3];
    std::string s = "TraceRejected: ";
    if (r.n_bad_components) s += std::to_string(r.n_bad_components) + " of 13 components violate their constraints";
    if (r.n_bad_components && total_bad) s += " and ";
    if (total_bad) s += "the logUp total is not zero";
    for (int k = 0; k < N_COMPONENTS; k++) {
        const bfhip_check_report& c = r.components[k];
        if (!c.n_bad_cells) continue;
        const int j = c.first_bad_constraint;
        s += std::string("\n") + COMPONENT_NAME[k] + ": constraint " + std::to_string(j) + " fails at table row " + std::to_string(c.first_bad_cell >> 4) + " (cell " +
             std::to_string(c.first_bad_cell) + "), value (" + words_text(c.first_bad_value, 4) + "); " +
             std::to_string(j >= 0 && j < 16 ? c.bad_per_constraint[j] : 0) + " cells violate it";
    }
    if (total_bad) s += "\nlogUp: the 13 claimed sums add up to (" + words_text(r.logup_total, 4) + "), not zero";
    auto where = [](int32_t table, uint64_t row) {
        if (table < 0) return std::string();
        return std::string(" (first: ") + (table < N_COMPONENTS ? COMPONENT_NAME[table] : "?") + " row " + std::to_string(row) + ")";
    };
    for (u32 q = 0; q < 3; q++) {
        for (u64 i = 0; i < r.relations[q].n_reported && i < 4; i++) {
            const bfhip_relation_entry& e = r.entries[4 * q + i];
            const long long net = e.net > P31 / 2 ? (long long)e.net - (long long)P31 : (long long)e.net;
            char sign[32]; snprintf(sign, sizeof sign, "%+lld", net);
            s += std::string("\n") + RELATION_NAME[e.relation < 3 ? e.relation : q] + " relation: (" + words_text(e.tuple, e.n_words <= 7 ? e.n_words : 7) + ") net " + sign +
                 ": yielded " + std::to_string(e.n_yield) + "x" + where(e.first_yield_table, e.first_yield_row) + ", used " + std::to_string(e.n_use) + "x" +
                 where(e.first_use_table, e.first_use_row);
            if (e.n_other) s += ", " + std::to_string(e.n_other) + " rows with another multiplicity";
        }
    }
    for (u32 q = 0; q < 3; q++) {
        const bfhip_relation_report& rr = r.relations[q];
        if (rr.n_unbalanced > rr.n_reported) s += std::string("\n") + RELATION_NAME[q] + " relation: " + std::to_string(rr.n_unbalanced - rr.n_reported) + " more unbalanced tuples not listed";
    }
    return s;
}

void HipProver::preflight(const TraceInput& in) {
    const double t_begin = now();
    // sizes the proof itself refuses keep their own message (prove: "a component exceeds LOG_MAX_ROWS")
    for (int k = 0; k < N_COMPONENTS; k++) if (in.log_sizes[k] > log_max_rows || in.log_sizes[k] < LOG_N_LANES || in.log_sizes[k] > 29) return;
    if (!c.preflight_last) c.preflight_last = std::make_shared<bfhip_preflight_report>();
    bfhip_preflight_report& rep = *c.preflight_last;
    rep = bfhip_preflight_report{};
    const Lookups el = default_check_lookups();
    const u32* rows[N_COMPONENTS][13] = {};
    const u32* const* tables[N_COMPONENTS];
    for (int k = 0; k < N_COMPONENTS; k++) { tables[k] = rows[k]; for (u32 j = 0; j < n_main_cols(k); j++) rows[k][j] = in.rows[k][j].ptr; }

    ArenaBorrow borrow(c);      // the logUp columns and scans: given back behind the read-back, or by a throw before it
    CheckReadback h_out{};
    for (int k = 0; k < N_COMPONENTS; k++) h_out.report[k] = check_report_init();
    const u32* inter[N_COMPONENTS][12] = {};
    CheckReadback* d_out = nullptr;
    {
        StageBatch sb(c);
        d_out = c.stage(&h_out, 1);
        const std::vector<LogupLaunch> logups = check_logup_launches(c, rows, in.log_sizes, d_out->claimed, inter);
        LogupBatch lb;
        logup_batch_init(lb, el, logups.data(), N_COMPONENTS);
        const LogupBatch* d_lb = c.stage(&lb, 1);
        CheckLaunch launches[N_COMPONENTS];
        for (int k = 0; k < N_COMPONENTS; k++) launches[k] = check_launch_of(k, in.log_sizes[k], rows[k], inter[k], el, q_zero(), &d_out->report[k]);
        const CheckLaunch* d_launches = c.stage(launches, N_COMPONENTS);
        CheckBatch cb;
        check_batch_init(cb, in.log_sizes, d_out);
        const CheckBatch* d_cb = c.stage(&cb, 1);
        sb.end();
        {
            ProfScope ps(c.stream, "preflight_logup", 0);      // bfhip_profile_enable mode 1: the two halves by HIP events (tools/preflight_rate.py)
            logup_batch_run(c.stream, d_lb, lb);
        }
        {
            ProfScope ps(c.stream, "preflight_check", 0);
            check_batch_run(c.stream, d_cb, cb, d_launches);
        }
    }
    BF_HIP(hipGetLastError());
    c.read_back(&h_out, d_out, sizeof h_out);      // the one host synchronisation of a passing preflight
    borrow.end();      // relations_in_proof, below, borrows from the same mark on its own
    mark("preflight read back");

    int32_t n_bad = 0;
    for (int k = 0; k < N_COMPONENTS; k++) {
        const uint4 cl = h_out.claimed[k];
        check_report_fill(rep.components[k], h_out.report[k], k, in.log_sizes[k], q_make(cl.x, cl.y, cl.z, cl.w));
        n_bad += h_out.report[k].n_bad_cells != 0;
    }
    rep.ran = 1;
    rep.n_bad_components = n_bad;
    rep.logup_total[0] = h_out.total.x; rep.logup_total[1] = h_out.total.y; rep.logup_total[2] = h_out.total.z; rep.logup_total[3] = h_out.total.w;
    const bool total_bad = h_out.total.x || h_out.total.y || h_out.total.z || h_out.total.w;
    if (!n_bad && !total_bad) { rep.seconds = now() - t_begin; return; }
    rep.rejected = 1;
    // the failure path: its read-backs do not matter. Which tuples do not cancel (relations.hip), at most 4 per relation
    if (total_bad) {
        try {
            relations_in_proof(c, tables, in.log_sizes, rep.relations, rep.entries, 4);
            for (u32 q = 0; q < 3; q++) rep.n_entries += (uint32_t)rep.relations[q].n_reported;
        } catch (...) {
            for (auto& rr : rep.relations) rr = bfhip_relation_report{};
            rep.n_entries = 0;
            rep.seconds = now() - t_begin;
            throw;
        }
    }
    rep.seconds = now() - t_begin;
    throw TraceRejected(preflight_text(rep));
}

}  // namespace bf

using namespace bf;

extern "C" {

int32_t bfhip_ctx_set_preflight(bfhip_ctx* ctx, int32_t on) {
    API_TRY
    if (!ctx) throw HipError("null context");
    if (on && ctx->c.shard.count > 1) throw HipError("bfhip_ctx_set_preflight: a context in a shard group is not supported (bfhip_ctx_leave_group first)");
    ctx->c.preflight = on != 0;
    return 0;
    API_CATCH
}
int32_t bfhip_ctx_get_preflight(bfhip_ctx* ctx, int32_t* on) {
    API_TRY
    if (!ctx || !on) throw HipError("null argument");
    *on = ctx->c.preflight ? 1 : 0;
    return 0;
    API_CATCH
}
int32_t bfhip_ctx_last_preflight(bfhip_ctx* ctx, bfhip_preflight_report* out) {
    API_TRY
    if (!ctx || !out) throw HipError("null argument");
    if (ctx->c.preflight_last) *out = *ctx->c.preflight_last; else *out = bfhip_preflight_report{};
    return 0;
    API_CATCH
}
int32_t bfhip_format_preflight(const bfhip_preflight_report* rep, char* buf, size_t cap, size_t* need) {
    API_TRY
    if (!rep || (!buf && cap)) throw HipError("null argument");
    const std::string s = preflight_text(*rep);
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

}  // extern "C"
