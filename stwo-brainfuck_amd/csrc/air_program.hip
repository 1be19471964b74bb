// The constraint program on the constraint domain (include/bfhip.h "Constraint programs": bfhip_air_eval_domain) — what
// `ComponentProver::evaluate_constraint_quotients_on_domain` does for any `FrameworkEval` (reached from prover::prove, mod.rs:732), as ONE
// gfx950 kernel that interprets the program instead of one compiled kernel per AIR (air.hip: k_constraints<COMP>).
//
// One lane per row of CanonicCoset(log_size + log_expand).circle_domain(), one wave per workgroup, on the interpreter core of
// program_interp.h (scalar loads of the program, scalar dispatch, register files in LDS: see there). This file adds what a row of the blown-up
// domain is (AirDomainRow) and what C_BASE / C_EXT do (AirDomainSink), both in air_domain.h; the coefficients come through scalar loads like
// the program.
#include "api_guard.h"
#include "air_domain.h"
#include "host/circle.h"
#include "../../include/bfhip.h"
#include <cstddef>

namespace bf {

__global__ void __launch_bounds__(PROGRAM_LANES) k_air_program(const AirLaunch* __restrict__ ap) {
    extern __shared__ u32 s_regs[];
    const BF_CONSTANT AirLaunch* a = (const BF_CONSTANT AirLaunch*)(unsigned long long)ap;
    const u32 log_size = a->log_size, log_expand = a->log_expand;
    const u32 row = blockIdx.x * PROGRAM_LANES + threadIdx.x;
    if (row >= (1u << (log_size + log_expand))) return;
    AirDomainSink sink{(const BF_CONSTANT bf_u32x4*)a->coeffs};
    program_run((const BF_CONSTANT bf_u32x4*)a->code, a->n_instr, (const BF_CONSTANT bf_u32x4*)a->cols, (const BF_CONSTANT bf_u32x4*)a->params,
                s_regs + threadIdx.x, s_regs + a->n_m * PROGRAM_LANES + threadIdx.x, AirDomainRow{row, log_size, log_expand}, sink);
    const u32 dinv = ((g_cu32p)(unsigned long long)ap)[offsetof(AirLaunch, denom_inv) / 4 + (row >> log_size)];
    const Q31 r = q_mulm(sink.sum(), dinv);
    g_u32p acc0 = (g_u32p)a->acc[0], acc1 = (g_u32p)a->acc[1], acc2 = (g_u32p)a->acc[2], acc3 = (g_u32p)a->acc[3];
    acc0[row] = m_add(acc0[row], r.a.a);
    acc1[row] = m_add(acc1[row], r.a.b);
    acc2[row] = m_add(acc2[row], r.b.a);
    acc3[row] = m_add(acc3[row], r.b.b);
}

}  // namespace bf

using namespace bf;

bf::ProgramInputs::ProgramInputs(const std::string& me, uint32_t n_cols, const uint32_t* const* cols_h, const uint32_t* col_shifts_h, uint32_t max_shift,
                                 const char* max_shift_text, const uint8_t* col_read_shifted, uint32_t program_params, const uint32_t* params_h_, uint32_t n_params_)
    : cols(4 * size_t(n_cols ? n_cols : 1), 0u), params_h(params_h_), n_params(n_params_) {
    if (n_params != program_params) throw HipError(me + ": the program takes " + std::to_string(program_params) + " parameters, got " + std::to_string(n_params));
    for (u32 i = 0; i < 4 * n_params; i++) if (params_h[i] >= P31) throw HipError(me + ": a parameter word is not a canonical M31");
    for (u32 k = 0; k < n_cols; k++) {
        const u32 s = col_shifts_h ? col_shifts_h[k] : 0u;
        if (!cols_h[k]) throw HipError(me + ": null column pointer (column " + std::to_string(k) + ")");
        if (s == 1 || s > max_shift) throw HipError(me + ": column " + std::to_string(k) + " has shift " + std::to_string(s) + " (0, or 2 .. " + max_shift_text + ")");
        if (s && col_read_shifted && col_read_shifted[k]) throw HipError(me + ": column " + std::to_string(k) + " is stored with shift " + std::to_string(s) + " and read at a non-zero offset");
        const unsigned long long p = (unsigned long long)cols_h[k];
        cols[4 * k] = (u32)p; cols[4 * k + 1] = (u32)(p >> 32); cols[4 * k + 2] = s;
    }
}

void bf::ProgramInputs::stage(Ctx& c, u64& cols_d, u64& params_d) const {
    static const u32 zero4[4] = {0, 0, 0, 0};
    cols_d = (u64)c.stage(cols.data(), cols.size());
    params_d = (u64)c.stage(n_params ? params_h : zero4, n_params ? 4 * (size_t)n_params : 4);
}

// The rules about one component's domain, in the caller's name `me` (bfhip_air_eval_domain; bfhip_air_compose names the component too)
void bf::air_domain_checks(const Ctx& c, const std::string& me, uint32_t log_size, uint32_t log_expand) {
    if (log_expand < 1 || log_expand > 3) throw HipError(me + ": log_expand must be in [1, 3], got " + std::to_string(log_expand));
    if (log_size < 1 || log_size > 29) throw HipError(me + ": log_size must be at least 1 and log_size + log_expand at most max_log_domain");
    const u32 el = log_size + log_expand;
    if (el > c.tw_root_log + 1) throw HipError(me + ": log_size + log_expand = " + std::to_string(el) + " exceeds the context's max_log_domain " + std::to_string(c.tw_root_log + 1));
}

// 1 / coset_vanishing(CanonicCoset(log_size).coset, domain.at(d)) depends on d mod 2^log_expand only; in bit-reversed storage those are the
// top bits of the row: entry i = row >> log_size belongs to d = bit_rev(i)
void bf::air_denominators(uint32_t log_size, uint32_t log_expand, uint32_t denom_inv[8]) {
    const u32 el = log_size + log_expand;
    for (u32 i = 0; i < (1u << log_expand); i++) denom_inv[i] = m_inv(coset_vanishing_m(log_size, canonic_domain_at(el, bit_rev(i, log_expand))));
}

// The checks and the staging of bfhip_air_eval_domain, shared with the compiled kernels' entry point (air_compile.hip): the two answer a bad
// argument with the same words.
const AirLaunch* bf::air_eval_stage(Ctx& c, const bfhip_air* air, bool with_code, uint32_t log_size, uint32_t log_expand, const uint32_t* const* cols_h,
                                    const uint32_t* col_shifts_h, const uint32_t* params_h, uint32_t n_params, const uint32_t* coeffs_h, uint32_t n_coeffs,
                                    uint32_t* const acc_d[4]) {
    const std::string me = "bfhip_air_eval_domain";
    if (!air || !coeffs_h || !acc_d || (!cols_h && air->n_cols) || (!params_h && n_params)) throw HipError("null argument");
    if (c.shard.count > 1) throw HipError(me + ": a context in a shard group is not supported (bfhip_ctx_leave_group first)");
    air_domain_checks(c, me, log_size, log_expand);
    const u32 el = log_size + log_expand;
    if (n_coeffs != air->n_constraints) throw HipError(me + ": the program has " + std::to_string(air->n_constraints) + " constraints, got " + std::to_string(n_coeffs) + " coefficients");
    for (u32 i = 0; i < 4 * n_coeffs; i++) if (coeffs_h[i] >= P31) throw HipError(me + ": a coefficient word is not a canonical M31");
    for (int w = 0; w < 4; w++) if (!acc_d[w]) throw HipError(me + ": null accumulator pointer");
    const ProgramInputs in(me, air->n_cols, cols_h, col_shifts_h, el, "log_size + log_expand", air->col_read_shifted.data(), air->n_params, params_h, n_params);
    AirLaunch L{};
    L.n_instr = air->n_instr; L.n_m = air->n_m; L.log_size = log_size; L.log_expand = log_expand;
    for (int w = 0; w < 4; w++) L.acc[w] = (u64)acc_d[w];
    air_denominators(log_size, log_expand, L.denom_inv);
    c.stage_checkpoint();
    {
        StageBatch sb(c);
        L.code = with_code ? (u64)c.stage(air->code.data(), air->code.size()) : 0;
        in.stage(c, L.cols, L.params);
        L.coeffs = (u64)c.stage(coeffs_h, 4 * (size_t)n_coeffs);
        const AirLaunch* d_launch = c.stage(&L, 1);
        sb.end();
        return d_launch;
    }
}

extern "C" int32_t bfhip_air_eval_domain(bfhip_ctx* ctx, const bfhip_air* air, uint32_t log_size, uint32_t log_expand, const uint32_t* const* cols_h,
                                         const uint32_t* col_shifts_h, const uint32_t* params_h, uint32_t n_params, const uint32_t* coeffs_h, uint32_t n_coeffs,
                                         uint32_t* const acc_d[4]) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    const AirLaunch* d_launch = air_eval_stage(c, air, true, log_size, log_expand, cols_h, col_shifts_h, params_h, n_params, coeffs_h, n_coeffs, acc_d);
    {
        const u32 n = 1u << (log_size + log_expand);
        const size_t lds = sizeof(u32) * PROGRAM_LANES * (air->n_m + 4 * air->n_q);
        ProfScope ps(c.stream, "k_air_program", 0);
        hipLaunchKernelGGL(k_air_program, dim3((n + PROGRAM_LANES - 1) / PROGRAM_LANES), dim3(PROGRAM_LANES), lds, c.stream, d_launch);
    }
    BF_HIP(hipGetLastError());
    return 0;
    API_CATCH
}
