// The composition polynomial of an AIR given as programs (include/bfhip.h "Composition": bfhip_air_compose) — what
// `ComponentProvers::compute_composition_polynomial` and `DomainEvaluationAccumulator::finalize` do for all components of a proof, as the
// frozen Brainfuck path does it for its 13 (prover_oods.hip: compute_composition), on the interpreter of program_interp.h.
//
// A bucket = the components of equal el = log_size + log_expand: they share an accumulator. k_air_compose takes every interpreted component
// of the call: the buckets below 2^16 rows in ONE launch, each larger bucket in a launch of its own (launch groups, below, say why). A workgroup is one wave and owns 64 consecutive rows of one bucket, which it finds from blockIdx.x in
// the bucket table (uniform addresses: scalar loads, as k_constraints_batch finds its class). It walks the bucket's components in list
// order, each with its own code, descriptors, parameters, coefficient slice, log_size, log_expand and denominator table, keeps the
// running QM31 sum in registers and writes it once: no read of the accumulator, no zero fill, and no two workgroups on one row. The register
// files are dynamic LDS as in k_air_program, sized for the largest program of the launch group.
// Components given as compiled kernels follow, one launch each (air_compile.hip), and add into their bucket. Finalize: one batched inverse
// transform over every bucket's four coordinate columns (the path of bfhip_interpolate), then accumulate_sizes adds the smaller buckets'
// coefficients onto the prefix of the largest: zero extension of coefficients is evaluation on a larger domain, and interpolation is linear
// (the comment in compute_composition has the argument). The largest bucket accumulates in the caller's destination; the smaller ones in
// one hipMalloc that lives for the call — the arena may belong to an open session.
#include "api_guard.h"
#include "air_domain.h"
#include "../../include/bfhip.h"
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <map>

namespace bf {

// One interpreted component of the launch: AirLaunch without the accumulator (the bucket has it)
struct AirComposeComp {
    u64 code, cols, params, coeffs;      // bf_u32x4 arrays, as in AirLaunch
    u32 n_instr, n_m, log_size, log_expand;
    u32 denom_inv[8];                    // 1 / coset_vanishing, indexed by row >> log_size
};
// The workgroups [block0, next bucket's block0) own the bucket's n_rows rows; its components are comp[comp0 .. comp0 + n_comps) in list order
struct AirComposeBucket { u64 acc[4]; u32 block0, n_rows, comp0, n_comps; };

__global__ void __launch_bounds__(PROGRAM_LANES) k_air_compose(const AirComposeBucket* __restrict__ bp, u32 n_buckets, const AirComposeComp* __restrict__ cp) {
    extern __shared__ u32 s_regs[];
    const BF_CONSTANT AirComposeBucket* buckets = (const BF_CONSTANT AirComposeBucket*)(unsigned long long)bp;
    u32 k = 0;
    while (k + 1 < n_buckets && blockIdx.x >= buckets[k + 1].block0) k++;
    const BF_CONSTANT AirComposeBucket* b = buckets + k;
    const u32 row = (blockIdx.x - b->block0) * PROGRAM_LANES + threadIdx.x;
    if (row >= b->n_rows) return;      // the last wave of a bucket of fewer than 64 rows
    const u32 comp0 = b->comp0, n_comps = b->n_comps;
    Q31 total = q_zero();
#pragma unroll 1
    for (u32 i = 0; i < n_comps; i++) {
        const AirComposeComp* cg = cp + comp0 + i;
        const BF_CONSTANT AirComposeComp* a = (const BF_CONSTANT AirComposeComp*)(unsigned long long)cg;
        const u32 log_size = a->log_size, log_expand = a->log_expand;
        AirDomainSink sink{(const BF_CONSTANT bf_u32x4*)a->coeffs};
        program_run((const BF_CONSTANT bf_u32x4*)a->code, a->n_instr, (const BF_CONSTANT bf_u32x4*)a->cols, (const BF_CONSTANT bf_u32x4*)a->params,
                    s_regs + threadIdx.x, s_regs + a->n_m * PROGRAM_LANES + threadIdx.x, AirDomainRow{row, log_size, log_expand}, sink);
        const u32 dinv = ((g_cu32p)(unsigned long long)cg)[offsetof(AirComposeComp, denom_inv) / 4 + (row >> log_size)];
        total = q_add(total, q_mulm(sink.sum(), dinv));
    }
    ((g_u32p)b->acc[0])[row] = total.a.a;
    ((g_u32p)b->acc[1])[row] = total.a.b;
    ((g_u32p)b->acc[2])[row] = total.b.a;
    ((g_u32p)b->acc[3])[row] = total.b.b;
}

// The inverse transform of a 4-cell domain, which the batched transform does not have (its circle layer reads twiddles in groups of four
// pairs: bfhip_interpolate starts at 8 cells). CanonicCoset(2).circle_domain() in bit-reversed order is (x, y), (x, -y), (-x, -y), (-x, y)
// with x = 2^15, y = -2^15, and the polynomial is c0 + c1 y + c2 x + c3 x y: two circle butterflies (twiddles 1 / y, -1 / y), two line
// butterflies (twiddle 1 / x), the scale 1 / 4. Lane w takes coordinate column w, in place.
__global__ void __launch_bounds__(64) k_air_compose_interp4(AirComposeBucket b) {
    if (threadIdx.x >= 4) return;
    g_u32p v = (g_u32p)b.acc[threadIdx.x];
    const u32 inv_x = 1u << 16, inv_y = P31 - (1u << 16), quarter = 1u << 29;      // 2^31 = 1
    const u32 s0 = v[0], s1 = v[1], s2 = v[2], s3 = v[3];
    const u32 a0 = m_add(s0, s1), a1 = m_mul(m_sub(s0, s1), inv_y), b0 = m_add(s2, s3), b1 = m_mul(m_sub(s3, s2), inv_y);
    v[0] = m_mul(m_add(a0, b0), quarter);
    v[1] = m_mul(m_add(a1, b1), quarter);
    v[2] = m_mul(m_mul(m_sub(a0, b0), inv_x), quarter);
    v[3] = m_mul(m_mul(m_sub(a1, b1), inv_x), quarter);
}

}  // namespace bf

using namespace bf;

namespace {

struct Bucket {
    u32 el = 0;
    u32* acc[4] = {};
    std::vector<u32> interpreted, compiled;      // indices into the caller's list, in list order
};

}  // namespace

extern "C" int32_t bfhip_air_compose(bfhip_ctx* ctx, const bfhip_air_component* comps, uint32_t n, const uint32_t random_coeff_h[4], uint32_t dst_log,
                                     uint32_t* const dst_d[4]) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    const std::string me = "bfhip_air_compose";
    if (!comps || !random_coeff_h || !dst_d) throw HipError(me + ": null argument");
    air_compose_count(me, n);
    if (c.shard.count > 1) throw HipError(me + ": a context in a shard group is not supported (bfhip_ctx_leave_group first)");
    for (int w = 0; w < 4; w++) if (!dst_d[w]) throw HipError(me + ": null destination pointer");

    // ---- every rule about every component, before anything is staged or enqueued -------------------------------------------------------
    std::vector<const bfhip_air*> airs(n);
    std::vector<ProgramInputs> inputs;
    std::vector<u32> counts(n), first(n);
    inputs.reserve(n);
    u32 max_el = 0, total = 0;
    for (u32 k = 0; k < n; k++) {
        const bfhip_air_component& p = comps[k];
        const std::string mk = me + ": component " + std::to_string(k);
        if (p.reserved != 0) throw HipError(mk + ": reserved must be 0");
        if (!p.program && !p.kernel) throw HipError(mk + ": neither program nor kernel is set");
        const bfhip_air* air = p.kernel ? &air_kernel_program(ctx, p.kernel, mk) : p.program;
        if ((!p.cols_h && air->n_cols) || (!p.params_h && p.n_params)) throw HipError(mk + ": null argument");
        air_domain_checks(c, mk, p.log_size, p.log_expand);
        const u32 el = p.log_size + p.log_expand;
        inputs.emplace_back(mk, air->n_cols, p.cols_h, p.col_shifts_h, el, "log_size + log_expand", air->col_read_shifted.data(), air->n_params, p.params_h, p.n_params);
        airs[k] = air; counts[k] = air->n_constraints; first[k] = total; total += counts[k];
        max_el = std::max(max_el, el);
    }
    std::vector<u32> coeffs(4 * (size_t)total);
    air_compose_coeffs(me, counts.data(), n, random_coeff_h, coeffs.data());
    if (dst_log != max_el) throw HipError(me + ": dst_log must be the largest log_size + log_expand of the list, " + std::to_string(max_el) + ", got " + std::to_string(dst_log));

    // ---- buckets, by descending size: the largest accumulates in dst_d ------------------------------------------------------------------
    std::vector<Bucket> buckets;
    for (u32 k = 0; k < n; k++) {
        const u32 el = comps[k].log_size + comps[k].log_expand;
        auto it = std::find_if(buckets.begin(), buckets.end(), [&](const Bucket& b) { return b.el == el; });
        if (it == buckets.end()) { buckets.emplace_back(); it = buckets.end() - 1; it->el = el; }
        (comps[k].kernel ? it->compiled : it->interpreted).push_back(k);
    }
    std::sort(buckets.begin(), buckets.end(), [](const Bucket& x, const Bucket& y) { return x.el > y.el; });
    size_t scratch_words = 0;
    for (size_t b = 1; b < buckets.size(); b++) scratch_words += size_t(4) << buckets[b].el;      // < 4 * 2^dst_log: distinct smaller powers of two

    // ---- the transforms: one job per bucket of 8 cells and more (planned here for its size, again below with the staged pointers) --------
    std::vector<FftJob> jobs;
    for (const Bucket& b : buckets) if (b.el >= 3) jobs.push_back(FftJob{nullptr, nullptr, 4, b.el, b.el, true});
    FftPlan plan;
    fft_plan(plan, true, jobs.data(), jobs.size(), c.d_tw, c.d_itw, c.tw_root_log);

    // ---- what the call stages, every block rounded as Ctx::stage does ------------------------------------------------------------------
    size_t need = 0, n_interpreted = 0;
    {
        std::map<const bfhip_air*, int> seen;
        for (u32 k = 0; k < n; k++) {
            if (!comps[k].kernel) {
                n_interpreted++;
                if (seen.emplace(airs[k], 0).second) need += Ctx::stage_round(sizeof(u32) * airs[k]->code.size());
            } else need += Ctx::stage_round(sizeof(AirLaunch));
            need += Ctx::stage_round(sizeof(u32) * inputs[k].cols.size()) + Ctx::stage_round(16 * (size_t)std::max(comps[k].n_params, 1u));
        }
        need += Ctx::stage_round(sizeof(u32) * coeffs.size()) + Ctx::stage_round(sizeof(AirComposeComp) * std::max<size_t>(n_interpreted, 1)) +
                Ctx::stage_round(sizeof(AirComposeBucket) * buckets.size()) + Ctx::stage_round(sizeof(u32*) * 4 * buckets.size()) +
                Ctx::stage_round(sizeof(PassArgs) * std::max<size_t>(plan.groups.size(), 1));
    }
    if (need > c.stage_bytes) throw HipError(me + ": the list stages " + std::to_string(need) + " bytes, the context's staging ring holds " + std::to_string(c.stage_bytes));

    // the smaller buckets' accumulators: no launch that uses them is in flight when the guard frees them
    DeviceScratch scratch(c);
    u32* small_acc = nullptr;
    if (scratch_words) scratch.alloc(&small_acc, scratch_words * sizeof(u32));
    {
        u32* at = small_acc;
        for (size_t b = 0; b < buckets.size(); b++)
            for (int w = 0; w < 4; w++) {
                if (b == 0) buckets[b].acc[w] = dst_d[w];
                else { buckets[b].acc[w] = at; at += size_t(1) << buckets[b].el; }
            }
    }

    // ---- one staged copy -----------------------------------------------------------------------------------------------------------------
    // Launch groups of the interpreter. A bucket of 2^16 rows and more gets a launch of its own, sized for its own largest program: with one
    // launch for all, every wave asked for the LDS of the largest program of the LIST, and on the sizes of a fib19 trace that cost 7 % of the
    // sweep (DESIGN.md section 9n has the figures). Below 2^16 rows (1024 waves: fewer than the chip holds at any program size) LDS does not
    // bound the occupancy and a launch costs more than it could save: those buckets share ONE launch and find themselves in the table.
    // BFHIP_AIR_COMPOSE_LAUNCH=one / bucket: A/B knob of tools/air_compose_rate.py — one launch for all / one per bucket (the same words).
    static const int launch_mode = [] { const char* v = getenv("BFHIP_AIR_COMPOSE_LAUNCH"); return !v ? 0 : !strcmp(v, "one") ? 1 : !strcmp(v, "bucket") ? 2 : 0; }();
    struct Group { size_t first, count; u32 blocks; size_t lds; };
    std::vector<Group> groups;
    std::vector<AirComposeBucket> h_buckets;      // the buckets of the interpreter launch
    std::vector<AirComposeComp> h_comps;
    std::vector<std::pair<u32, const AirLaunch*>> kernel_launches;      // (component, its staged launch block)
    const AirComposeBucket* d_buckets = nullptr;
    const AirComposeComp* d_comps = nullptr;
    c.stage_checkpoint(need);
    {
        StageBatch sb(c);
        const u32* d_coeffs = c.stage(coeffs.data(), coeffs.size());
        std::map<const bfhip_air*, u64> code_d;
        for (const Bucket& b : buckets) {
            if (!b.interpreted.empty()) {
                AirComposeBucket hb{};
                for (int w = 0; w < 4; w++) hb.acc[w] = (u64)b.acc[w];
                hb.n_rows = 1u << b.el; hb.comp0 = (u32)h_comps.size(); hb.n_comps = (u32)b.interpreted.size();
                size_t bl = 0;
                for (u32 k : b.interpreted) bl = std::max(bl, sizeof(u32) * PROGRAM_LANES * (airs[k]->n_m + 4 * airs[k]->n_q));
                // the buckets come by descending size: the small ones are the tail of the table and join the group the first of them opened
                const bool alone = launch_mode == 2 || (launch_mode == 0 && b.el >= 16);
                if (groups.empty() || alone || groups.back().count == 0) groups.push_back(Group{h_buckets.size(), 0, 0, 0});
                Group& g = groups.back();
                hb.block0 = g.blocks;
                g.count++; g.blocks += (hb.n_rows + PROGRAM_LANES - 1) / PROGRAM_LANES; g.lds = std::max(g.lds, bl);
                if (alone) groups.push_back(Group{h_buckets.size() + 1, 0, 0, 0});      // closed: the next bucket opens another
                h_buckets.push_back(hb);
            }
            for (u32 k : b.interpreted) {
                const bfhip_air* air = airs[k];
                AirComposeComp hc{};
                auto it = code_d.find(air);
                if (it == code_d.end()) it = code_d.emplace(air, (u64)c.stage(air->code.data(), air->code.size())).first;
                hc.code = it->second;
                inputs[k].stage(c, hc.cols, hc.params);
                hc.coeffs = (u64)(d_coeffs + 4 * (size_t)first[k]);
                hc.n_instr = air->n_instr; hc.n_m = air->n_m; hc.log_size = comps[k].log_size; hc.log_expand = comps[k].log_expand;
                air_denominators(hc.log_size, hc.log_expand, hc.denom_inv);
                h_comps.push_back(hc);
            }
            for (u32 k : b.compiled) {
                const bfhip_air* air = airs[k];
                AirLaunch L{};
                inputs[k].stage(c, L.cols, L.params);
                L.coeffs = (u64)(d_coeffs + 4 * (size_t)first[k]);
                for (int w = 0; w < 4; w++) L.acc[w] = (u64)b.acc[w];
                L.n_instr = air->n_instr; L.n_m = air->n_m; L.log_size = comps[k].log_size; L.log_expand = comps[k].log_expand;
                air_denominators(L.log_size, L.log_expand, L.denom_inv);
                kernel_launches.emplace_back(k, c.stage(&L, 1));
            }
        }
        if (!h_comps.empty()) {
            d_buckets = c.stage(h_buckets.data(), h_buckets.size());
            d_comps = c.stage(h_comps.data(), h_comps.size());
        }
        if (!jobs.empty()) {
            std::vector<u32*> ptrs;
            for (const Bucket& b : buckets) if (b.el >= 3) for (int w = 0; w < 4; w++) ptrs.push_back(b.acc[w]);
            u32* const* d_ptrs = c.stage(ptrs.data(), ptrs.size());
            for (size_t j = 0; j < jobs.size(); j++) { jobs[j].d_src = (const u32* const*)(d_ptrs + 4 * j); jobs[j].d_dst = d_ptrs + 4 * j; }
            fft_plan(plan, true, jobs.data(), jobs.size(), c.d_tw, c.d_itw, c.tw_root_log);
            plan.d_groups = c.stage(plan.groups.data(), plan.groups.size());
        }
        sb.end();
    }

    // ---- the sweep: the interpreted components by launch group, then the compiled ones into their buckets --------------------------------
    for (size_t b = 0; b < buckets.size(); b++) {
        if (!buckets[b].interpreted.empty()) continue;      // compiled kernels only: they add, so the accumulator starts at zero
        if (b == 0) for (int w = 0; w < 4; w++) BF_HIP(hipMemsetAsync(buckets[b].acc[w], 0, sizeof(u32) << buckets[b].el, c.stream));
        else BF_HIP(hipMemsetAsync(buckets[b].acc[0], 0, sizeof(u32) * 4 << buckets[b].el, c.stream));
    }
    for (const Group& g : groups) {
        if (!g.count) continue;
        ProfScope ps(c.stream, "k_air_compose", 0);
        hipLaunchKernelGGL(k_air_compose, dim3(g.blocks), dim3(PROGRAM_LANES), g.lds, c.stream, d_buckets + g.first, (u32)g.count, d_comps);
    }
    BF_HIP(hipGetLastError());
    for (const auto& kl : kernel_launches) air_kernel_launch(c, comps[kl.first].kernel, kl.second, 1u << (comps[kl.first].log_size + comps[kl.first].log_expand));

    // ---- finalize ------------------------------------------------------------------------------------------------------------------------
    for (const Bucket& b : buckets) {
        if (b.el >= 3) continue;
        AirComposeBucket hb{};
        for (int w = 0; w < 4; w++) hb.acc[w] = (u64)b.acc[w];
        hipLaunchKernelGGL(k_air_compose_interp4, dim3(1), dim3(64), 0, c.stream, hb);
    }
    if (!jobs.empty()) fft_run(c.stream, plan);
    BF_HIP(hipGetLastError());
    for (size_t b = 1; b < buckets.size();) {      // 12 sources per launch; the additions are exact, so their grouping does not matter
        AccumulateSizes as{};
        for (int w = 0; w < 4; w++) as.dst[w] = dst_d[w];
        for (; b < buckets.size() && as.n < 12; b++, as.n++) {
            for (int w = 0; w < 4; w++) as.src[as.n][w] = buckets[b].acc[w];
            as.log[as.n] = buckets[b].el;
        }
        accumulate_sizes(c.stream, as);
    }
    BF_HIP(hipGetLastError());
    if (small_acc) c.sync();      // the scratch is freed on return
    return 0;
    API_CATCH
}
