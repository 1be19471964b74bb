// C ABI (include/bfhip.h): the backend-trait operations, one stwo `*Ops` call each over the gfx950 kernels. Plain pointers and sizes.
#include "../../include/bfhip.h"
#include "api_guard.h"
#include "api_args.h"
#include "pcs_types.h"
#include "host/quotients.h"
#include "host/hash.h"
#include "rows.h"
#include "rows_index.h"
#include "rows_select.h"
#include "rows_fill.h"
#include <string>
#include <algorithm>
#include <vector>

using namespace bf;

// What bfhip_interpolate and bfhip_evaluate share behind their argument checks: the job's column lists staged, one plan, its launches
static void fft_columns(Ctx& c, bool inverse, FftJob job, uint32_t* const* src_cols_h, uint32_t* const* dst_cols_h) {
    c.stage_checkpoint();
    StageBatch sb(c);
    job.d_src = (const u32* const*)c.stage(src_cols_h, job.ncols);
    job.d_dst = (u32* const*)c.stage(dst_cols_h, job.ncols);
    FftPlan plan;
    fft_plan(plan, inverse, &job, 1, c.d_tw, c.d_itw, c.tw_root_log);
    plan.d_groups = c.stage(plan.groups.data(), plan.groups.size());
    sb.end();
    fft_run(c.stream, plan);
    BF_HIP(hipGetLastError());
}
// The destination columns of bfhip_is_first_coeffs / bfhip_is_first_lde behind the checks the two share
static IsFirstCols is_first_cols(const char* who, uint32_t log_min, uint32_t log_max, uint32_t* const* dst_cols_h) {
    if (!dst_cols_h) throw HipError("null argument");
    if (log_min < 4 || log_max < log_min || log_max - log_min >= 28) throw HipError(std::string(who) + ": need 4 <= log_min <= log_max < log_min + 28");
    IsFirstCols a{}; a.log_min = log_min; a.log_max = log_max;
    for (u32 n = log_min; n <= log_max; n++) a.ptr[n - log_min] = dst_cols_h[n - log_min];
    return a;
}
// The 32 factors of a fold-by-halves evaluation at point_h = (x, y), staged: y, then x and its images under the doubling map x -> 2 x^2 - 1
static const uint4* stage_point_factors(Ctx& c, const uint32_t point_h[8]) {
    uint4 factors[32];
    Q31 x = q_make(point_h[0], point_h[1], point_h[2], point_h[3]);
    factors[0] = make_uint4(point_h[4], point_h[5], point_h[6], point_h[7]);
    for (u32 b = 1; b < 32; b++) { factors[b] = make_uint4(x.a.a, x.a.b, x.b.a, x.b.b); Q31 s = q_mul(x, x); x = q_subm(q_add(s, s), 1); }
    return c.stage(factors, 32);
}
// Column descriptors of (pointer, shift) lists; no shifts = every column at full size
static std::vector<ColDesc> col_descs(const uint32_t* const* cols_h, const uint32_t* col_shifts_h, uint32_t n_cols) {
    std::vector<ColDesc> d(n_cols);
    for (u32 k = 0; k < n_cols; k++) d[k] = ColDesc{cols_h[k], col_shifts_h ? col_shifts_h[k] : 0u, 0};
    return d;
}
// One Merkle layer over the previous layer and this size's columns, by the context's Blake2s convention or by Poseidon252
static void merkle_commit_layer(Ctx& c, bool poseidon, uint32_t log_size, const void* prev_layer_d, const uint32_t* const* cols_h, const uint32_t* col_shifts_h, uint32_t n_cols,
                                void* out_hashes_d) {
    c.stage_checkpoint();
    const std::vector<ColDesc> d = col_descs(cols_h, col_shifts_h, n_cols);
    const ColDesc* dd = n_cols ? c.stage(d.data(), n_cols) : nullptr;
    if (poseidon) merkle_layer_poseidon(c.stream, out_hashes_d, prev_layer_d, dd, n_cols, log_size);
    else merkle_layer(c.stream, out_hashes_d, prev_layer_d, dd, n_cols, log_size, 0.0, 0, 0, c.conv.merkle_node_hash);
    BF_HIP(hipGetLastError());
}
static const u32* stage_alpha(Ctx& c, const uint32_t alpha_h[4]) {
    const Q31 a = q_from_h(alpha_h);
    u32 w[8];
    q31_words(a, w); q31_words(q_mul(a, a), w + 4);
    c.stage_checkpoint();
    return c.stage(w, 8);
}
// ---- what the two row-order entry points share (rows.hip); ByteRange is api_args.h's ----
static void rows_check_index(const char* who, uint32_t log_size, uint64_t index, const uint64_t* out) {
    if (!out) throw HipError(std::string(who) + ": null argument");
    if (log_size < 1 || log_size > ROWS_MAX_LOG) throw HipError(std::string(who) + ": log_size " + std::to_string(log_size) + " is outside 1..30");
    if (index >> log_size) throw HipError(std::string(who) + ": index " + std::to_string(index) + " is not below 2^" + std::to_string(log_size));
}
static void rows_check_shape(const std::string& who, uint32_t log_size, uint64_t n_rows, uint32_t n_cols, const char* n_cols_name) {
    if (log_size < 1 || log_size > ROWS_MAX_LOG) throw HipError(who + "log_size " + std::to_string(log_size) + " is outside 1..30");
    if (n_rows > (u64(1) << log_size)) throw HipError(who + "n_rows " + std::to_string(n_rows) + " exceeds 2^" + std::to_string(log_size));
    if (n_cols == 0 || n_cols > BFHIP_AIR_MAX_COLUMNS)
        throw HipError(who + n_cols_name + " " + std::to_string(n_cols) + " is outside 1.." + std::to_string((int)BFHIP_AIR_MAX_COLUMNS) + " (BFHIP_AIR_MAX_COLUMNS)");
}
static void rows_not_sharded(const Ctx& c, const std::string& who) {
    if (c.shard.count > 1) throw HipError(who + "a context in a shard group is not supported (bfhip_ctx_leave_group first)");
}

extern "C" {

int32_t bfhip_interpolate(bfhip_ctx* ctx, uint32_t* const* src_cols_h, uint32_t* const* dst_cols_h, uint32_t n_cols, uint32_t log_size, int32_t replicated) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    if (replicated && log_size < 4) throw HipError("replicated columns need log_size >= 4");
    if (!replicated && log_size < 3) throw HipError("circle transforms need log_size >= 3");
    if (log_size > c.tw_root_log + 1) throw HipError("log_size exceeds the context's twiddle tree");
    u32 log = replicated ? log_size - 4 : log_size;
    fft_columns(c, true, FftJob{nullptr, nullptr, n_cols, log, log, !replicated}, src_cols_h, dst_cols_h);
    return 0;
    API_CATCH
}

int32_t bfhip_evaluate(bfhip_ctx* ctx, uint32_t* const* coeff_cols_h, uint32_t* const* dst_cols_h, uint32_t n_cols, uint32_t log_size, uint32_t log_eval, int32_t replicated) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    if (log_eval < log_size) throw HipError("log_eval < log_size");
    if (replicated && log_size < 4) throw HipError("replicated columns need log_size >= 4");
    if (!replicated && log_eval < 3) throw HipError("circle transforms need log_eval >= 3");
    if (log_eval > c.tw_root_log + 1) throw HipError("log_eval exceeds the context's twiddle tree");
    u32 sh = replicated ? 4 : 0;
    fft_columns(c, false, FftJob{nullptr, nullptr, n_cols, log_eval - sh, log_size - sh, !replicated}, coeff_cols_h, dst_cols_h);
    return 0;
    API_CATCH
}

int32_t bfhip_is_first_coeffs(bfhip_ctx* ctx, uint32_t log_min, uint32_t log_max, uint32_t* const* dst_cols_h) {
    API_CTX(ctx)
    const IsFirstCols a = is_first_cols("is_first_coeffs", log_min, log_max, dst_cols_h);
    if (log_max > ctx->c.tw_root_log + 1) throw HipError("log_max exceeds the context's twiddle tree");
    is_first_coeffs(ctx->c.stream, a, ctx->c.d_itw, ctx->c.tw_root_log);
    BF_HIP(hipGetLastError());
    return 0;
    API_CATCH
}
int32_t bfhip_is_first_lde(bfhip_ctx* ctx, uint32_t log_min, uint32_t log_max, uint32_t log_blowup, uint32_t* const* dst_cols_h) {
    API_CTX(ctx)
    const IsFirstCols a = is_first_cols("is_first_lde", log_min, log_max, dst_cols_h);
    if (log_blowup > 31 || log_max + log_blowup > ctx->c.tw_root_log + 1 || log_max + log_blowup > 31) throw HipError("log_max + log_blowup exceeds the context's twiddle tree");
    is_first_lde(ctx->c.stream, a, log_blowup, ctx->c.d_tw, ctx->c.d_itw, ctx->c.tw_root_log);
    BF_HIP(hipGetLastError());
    return 0;
    API_CATCH
}
int32_t bfhip_is_first_eval_at_point(bfhip_ctx* ctx, uint32_t log_size, const uint32_t point_h[8], uint32_t out_h[4]) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    if (!point_h || !out_h) throw HipError("null argument");
    if (log_size < 4 || log_size > 31 || log_size > c.tw_root_log + 1) throw HipError("is_first_eval_at_point: need 4 <= log_size within the context's twiddle tree");
    c.stage_checkpoint();
    IsFirstSample job{log_size, 0, 0};
    const IsFirstSample* dj = c.stage(&job, 1);
    const uint4* df = stage_point_factors(c, point_h);
    uint4 r;      // declared before the guard: the copy into it has completed when it goes
    DeviceScratch scratch(c);
    uint4* dout = nullptr;
    scratch.alloc(&dout, sizeof(uint4));
    is_first_samples(c.stream, dj, 1, df, dout, c.d_itw, c.tw_root_log);
    read_q31(c, dout, r, out_h);
    return 0;
    API_CATCH
}
int32_t bfhip_broadcast16(bfhip_ctx* ctx, const uint32_t* rows_d, uint32_t* dst_d, size_t n_rows) {
    API_CTX(ctx) broadcast16(ctx->c.stream, rows_d, dst_d, (u32)(n_rows * 16)); BF_HIP(hipGetLastError()); return 0; API_CATCH
}
int32_t bfhip_bit_reverse(bfhip_ctx* ctx, const uint32_t* src_d, uint32_t* dst_d, uint32_t log_size) {
    API_CTX(ctx) if (src_d == dst_d) throw HipError("bit_reverse is out of place"); bit_reverse(ctx->c.stream, src_d, dst_d, log_size); BF_HIP(hipGetLastError()); return 0; API_CATCH
}
int32_t bfhip_batch_inverse_m31(bfhip_ctx* ctx, const uint32_t* src_d, uint32_t* dst_d, size_t n) {
    API_CTX(ctx) batch_inverse_m31(ctx->c.stream, src_d, dst_d, (u32)n); BF_HIP(hipGetLastError()); return 0; API_CATCH
}
int32_t bfhip_batch_inverse_qm31(bfhip_ctx* ctx, const uint32_t* const src_d[4], uint32_t* const dst_d[4], size_t n) {
    API_CTX(ctx) batch_inverse_qm31(ctx->c.stream, src_d, dst_d, (u32)n); BF_HIP(hipGetLastError()); return 0; API_CATCH
}
int32_t bfhip_accumulate(bfhip_ctx* ctx, uint32_t* dst_d, const uint32_t* src_d, size_t n) {
    API_CTX(ctx) accumulate(ctx->c.stream, dst_d, src_d, (u32)n); BF_HIP(hipGetLastError()); return 0; API_CATCH
}
int32_t bfhip_eval_at_point(bfhip_ctx* ctx, const uint32_t* coeffs_d, uint32_t log_size, int32_t replicated, const uint32_t point_h[8], uint32_t out_h[4]) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    if (replicated && log_size < 4) throw HipError("replicated columns need log_size >= 4");
    c.stage_checkpoint();
    EvalJob job{coeffs_d, replicated ? log_size - 4 : log_size, 0, replicated ? 4u : 0u, 0};
    const EvalJob* dj = c.stage(&job, 1);
    const uint4* df = stage_point_factors(c, point_h);
    u32 nchunks = job.log_n > 12 ? 1u << (job.log_n - 12) : 1u;
    uint4 r;      // declared before the guard: the copy into it has completed when it goes
    DeviceScratch scratch(c);
    uint4* partials = nullptr;
    scratch.alloc(&partials, sizeof(uint4) * (nchunks + 1));
    uint4* dout = partials + nchunks;
    eval_at_points(c.stream, dj, 1, nchunks, df, partials, dout);
    read_q31(c, dout, r, out_h);
    return 0;
    API_CATCH
}
int32_t bfhip_merkle_commit_layer(bfhip_ctx* ctx, uint32_t log_size, const void* prev_layer_d, const uint32_t* const* cols_h, const uint32_t* col_shifts_h,
                                  uint32_t n_cols, void* out_hashes_d) {
    API_CTX(ctx) merkle_commit_layer(ctx->c, false, log_size, prev_layer_d, cols_h, col_shifts_h, n_cols, out_hashes_d); return 0; API_CATCH
}
int32_t bfhip_merkle_commit_layer_poseidon252(bfhip_ctx* ctx, uint32_t log_size, const void* prev_layer_d, const uint32_t* const* cols_h, const uint32_t* col_shifts_h,
                                             uint32_t n_cols, void* out_hashes_d) {
    API_CTX(ctx) merkle_commit_layer(ctx->c, true, log_size, prev_layer_d, cols_h, col_shifts_h, n_cols, out_hashes_d); return 0; API_CATCH
}
int32_t bfhip_hades_permutation(bfhip_ctx* ctx, const uint32_t in_h[24], uint32_t out_h[24]) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    c.stage_checkpoint();
    u32* din = (u32*)c.stage(in_h, 24);
    u32* dout = (u32*)c.stage(in_h, 24);
    hades_once(c.stream, din, dout);
    BF_HIP(hipMemcpyAsync(out_h, dout, 24 * sizeof(u32), hipMemcpyDeviceToHost, c.stream));
    c.sync();
    return 0;
    API_CATCH
}
int32_t bfhip_fold_line(bfhip_ctx* ctx, const uint32_t* const src_d[4], uint32_t* const dst_d[4], uint32_t log_size, const uint32_t alpha_h[4]) {
    API_CTX(ctx)
    if (log_size < 1 || log_size > ctx->c.tw_root_log) throw HipError("fold_line: log_size outside the twiddle tree");
    fold_line(ctx->c.stream, dst_d, src_d, stage_alpha(ctx->c, alpha_h), ctx->c.d_itw, ctx->c.tw_root_log, log_size); BF_HIP(hipGetLastError()); return 0;
    API_CATCH
}
int32_t bfhip_fold_circle_into_line(bfhip_ctx* ctx, uint32_t* const dst_d[4], const uint32_t* const src_d[4], uint32_t log_size, const uint32_t alpha_h[4]) {
    API_CTX(ctx)
    if (log_size < 3 || log_size > ctx->c.tw_root_log + 1) throw HipError("fold_circle_into_line: log_size outside the twiddle tree");
    fold_circle_into_line(ctx->c.stream, dst_d, src_d, stage_alpha(ctx->c, alpha_h), ctx->c.d_itw, ctx->c.tw_root_log, log_size); BF_HIP(hipGetLastError()); return 0;
    API_CATCH
}
int32_t bfhip_fri_fold_leaf(bfhip_ctx* ctx, const uint32_t* const src_d[4], const uint32_t* const quot_d[4], uint32_t* const dst_d[4], uint32_t log_size,
                            const uint32_t alpha_h[4], void* out_hashes_d) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    if (!src_d && !quot_d) throw HipError("fri_fold_leaf: neither a line source nor a circle evaluation");
    if (!dst_d || !alpha_h || !out_hashes_d) throw HipError("fri_fold_leaf: null argument");
    if (log_size < 2 || log_size + 1 > c.tw_root_log + (src_d ? 0u : 1u)) throw HipError("fri_fold_leaf: log_size outside the twiddle tree");
    FriFoldLeafArgs fa{};
    for (int w = 0; w < 4; w++) { fa.src[w] = src_d ? src_d[w] : nullptr; fa.quot[w] = quot_d ? quot_d[w] : nullptr; fa.dst[w] = dst_d[w]; }
    fa.alpha8 = stage_alpha(c, alpha_h); fa.itw = c.d_itw; fa.tw_total = 1u << c.tw_root_log; fa.log = log_size;
    fri_fold_leaf(c.stream, out_hashes_d, fa, !src_d ? FF_CIRCLE : quot_d ? FF_LINE_CIRCLE : FF_LINE, c.conv.merkle_node_hash);
    BF_HIP(hipGetLastError());
    return 0;
    API_CATCH
}
int32_t bfhip_grind(bfhip_ctx* ctx, const uint8_t digest_h[32], uint32_t pow_bits, uint64_t* nonce) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    c.stage_checkpoint();
    u32* d_digest = (u32*)c.stage(digest_h, 32);
    unsigned long long init = ~0ull, best = ~0ull;
    unsigned long long* d_best = c.stage(&init, 1);
    const u32 span = 1u << 20;
    for (u64 base = 0; best == ~0ull; base += span) {
        grind_span(c.stream, d_digest, base, span, pow_bits, d_best, c.conv.mix_u64);
        BF_HIP(hipMemcpyAsync(&best, d_best, 8, hipMemcpyDeviceToHost, c.stream));
        c.sync();
        if (base > (u64(1) << 40)) throw HipError("grind: no nonce found below 2^40");
    }
    *nonce = best;
    return 0;
    API_CATCH
}
// Spans start at start_nonce and are scanned in order, so the first span with a hit holds the smallest nonce. Span per launch: 2^clamp(pow_bits - 4, 12, 20)
// — twice the expected 2^(pow_bits - 5) tries, at least 64 waves, at most ~1.4 ms of the GPU per launch.
int32_t bfhip_grind_poseidon252(bfhip_ctx* ctx, const uint8_t digest_h[32], uint32_t pow_bits, uint64_t start_nonce, uint64_t* nonce, uint64_t* tried) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    if (!digest_h || !nonce) throw HipError("grind_poseidon252: null argument");
    if (pow_bits > BFHIP_MAX_POW_BITS) throw HipError("grind_poseidon252: pow_bits must be at most 32, got " + std::to_string(pow_bits));
    if (!fe252::canonical_bytes_in_range(digest_h)) throw HipError("grind_poseidon252: digest is not a canonical felt252");
    c.stage_checkpoint();
    u32* d_digest = (u32*)c.stage(digest_h, 32);
    unsigned long long init = ~0ull, best = ~0ull;
    unsigned long long* d_best = c.stage(&init, 1);
    const u32 log_span = std::min(std::max(pow_bits, 16u) - 4u, 20u);
    const u64 span = u64(1) << log_span, limit = u64(64) << (std::max(pow_bits, 8u) - 5u);      // a legitimate miss of `limit` nonces: e^-64
    u64 scanned = 0;
    while (best == ~0ull) {
        if (scanned >= limit) throw HipError("grind_poseidon252: no nonce found");
        const u64 base = start_nonce + scanned;
        if (base < start_nonce || base + (span - 1) < base) throw HipError("grind_poseidon252: the scan would wrap past 2^64");
        grind_poseidon_span(c.stream, d_digest, base, (u32)span, pow_bits, d_best);
        BF_HIP(hipGetLastError());
        BF_HIP(hipMemcpyAsync(&best, d_best, 8, hipMemcpyDeviceToHost, c.stream));
        c.sync();
        scanned += span;
    }
    *nonce = best;
    if (tried) *tried = scanned;
    return 0;
    API_CATCH
}
int32_t bfhip_gather(bfhip_ctx* ctx, const uint32_t* col_d, const uint64_t* idx_h, size_t n, uint32_t* out_h) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    std::vector<GatherReq> req(n);
    for (size_t i = 0; i < n; i++) req[i] = GatherReq{col_d, idx_h[i], (u32)i, 1u};
    DeviceScratch scratch(c);      // behind req: the copy from it has completed when the guard goes
    GatherReq* dreq = nullptr; u32* dout = nullptr;
    scratch.alloc(&dreq, sizeof(GatherReq) * (n + 1));
    scratch.alloc(&dout, sizeof(u32) * (n + 1));
    BF_HIP(hipMemcpyAsync(dreq, req.data(), sizeof(GatherReq) * n, hipMemcpyHostToDevice, c.stream));
    gather_u32(c.stream, dreq, (u32)n, dout);
    BF_HIP(hipMemcpyAsync(out_h, dout, sizeof(u32) * n, hipMemcpyDeviceToHost, c.stream));
    BF_HIP(hipStreamSynchronize(c.stream));
    return 0;
    API_CATCH
}
int32_t bfhip_accumulate_quotients(bfhip_ctx* ctx, uint32_t log_size, const uint32_t* const* cols_h, const uint32_t* col_shifts_h, uint32_t n_cols,
                                   const uint32_t* n_samples_h, const uint32_t* sample_points_h, const uint32_t* sample_values_h,
                                   const uint32_t random_coeff_h[4], uint32_t* const out_d[4]) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    if (log_size < 3 || log_size > c.tw_root_log + 1) throw HipError("accumulate_quotients: log_size outside the twiddle tree");
    const std::vector<ColDesc> descs = col_descs(cols_h, col_shifts_h, n_cols);
    std::vector<std::vector<ColumnSample>> samples(n_cols);
    size_t si = 0;
    for (u32 k = 0; k < n_cols; k++) {
        if (descs[k].shift == 1) throw HipError("accumulate_quotients: column shift must be 0 or >= 2");
        for (u32 s = 0; s < n_samples_h[k]; s++, si++) {
            const uint32_t* p = sample_points_h + 8 * si;
            samples[k].push_back({PtQ{q_from_h(p), q_from_h(p + 4)}, q_from_h(sample_values_h + 4 * si)});
        }
    }
    std::vector<QuotientBatch> batches; std::vector<QuotientEntry> entries;
    build_quotient_batches(samples, q_from_h(random_coeff_h), batches, entries);
    quotient_entries_finish(batches.data(), batches.size(), entries.data(), descs.data());
    c.stage_checkpoint();
    QuotientArgs a{};
    a.batches = batches.empty() ? nullptr : c.stage(batches.data(), batches.size());
    a.entries = entries.empty() ? nullptr : c.stage(entries.data(), entries.size());
    a.n_batches = (u32)batches.size(); a.log = log_size; a.tw = c.d_tw; a.tw_total = 1u << c.tw_root_log;
    for (int w = 0; w < 4; w++) a.out[w] = out_d[w];
    const u32 blocks = quotient_groups_layout(&a, 1);
    accumulate_quotients(c.stream, c.stage(&a, 1), 1, blocks);
    BF_HIP(hipGetLastError());
    return 0;
    API_CATCH
}

// ---- row order <-> storage order (include/bfhip.h "Row order"; rows.hip) ----
int32_t bfhip_cell_of_row(uint32_t log_size, uint64_t row, uint64_t* cell) {
    API_TRY
    rows_check_index("bfhip_cell_of_row", log_size, row, cell);
    *cell = rows_cell_of_row(log_size, (u32)row);
    return 0;
    API_CATCH
}
int32_t bfhip_row_of_cell(uint32_t log_size, uint64_t cell, uint64_t* row) {
    API_TRY
    rows_check_index("bfhip_row_of_cell", log_size, cell, row);
    *row = rows_row_of_cell(log_size, (u32)cell);
    return 0;
    API_CATCH
}
int32_t bfhip_columns_from_rows(bfhip_ctx* ctx, const bfhip_rows_table* table, uint32_t log_size, const uint32_t* src_cols_h, const uint32_t* pad_h,
                                uint32_t* const* out_cols_h, uint32_t n_out) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    const std::string who = "bfhip_columns_from_rows: ";
    if (!table || !out_cols_h) throw HipError(who + "null argument");
    if (table->reserved != 0) throw HipError(who + "reserved must be 0");
    if (table->layout != BFHIP_ROWS_ROW_MAJOR && table->layout != BFHIP_ROWS_COLUMN_MAJOR) throw HipError(who + "unknown layout " + std::to_string(table->layout));
    if (table->flags & ~uint32_t(BFHIP_ROWS_REPEAT_LAST)) throw HipError(who + "unknown flag bits " + std::to_string(table->flags));
    const bool col_major = table->layout == BFHIP_ROWS_COLUMN_MAJOR, repeat = (table->flags & BFHIP_ROWS_REPEAT_LAST) != 0;
    const u64 n_rows = table->n_rows, stride = col_major ? 1 : table->row_stride;
    rows_check_shape(who, log_size, n_rows, n_out, "n_out");
    if (table->n_cols == 0) throw HipError(who + "the table has no columns");
    if (!col_major && table->row_stride < table->n_cols) throw HipError(who + "row_stride " + std::to_string(table->row_stride) + " is below n_cols " + std::to_string(table->n_cols));
    if (repeat && n_rows == 0) throw HipError(who + "BFHIP_ROWS_REPEAT_LAST needs at least one row");
    if (col_major ? !table->cols_h : (n_rows && !table->rows_d)) throw HipError(who + "null table pointer");
    rows_not_sharded(c, who);
    const u64 col_bytes = sizeof(u32) << log_size;
    std::vector<RowsCol> cols(n_out);
    std::vector<ByteRange> used;      // the source first, then the output columns accepted so far
    if (col_major) {
        for (u32 j = 0; j < table->n_cols; j++) {
            if (n_rows && !table->cols_h[j]) throw HipError(who + "source column " + std::to_string(j) + " is a null pointer");
            used.push_back({(u64)(uintptr_t)table->cols_h[j], n_rows * sizeof(u32), "source column " + std::to_string(j)});
        }
    } else if (n_rows) {
        used.push_back({(u64)(uintptr_t)table->rows_d, (rows_src_offset(n_rows - 1, stride, table->n_cols - 1) + 1) * sizeof(u32), "the source table"});
    }
    for (u32 k = 0; k < n_out; k++) {
        const u32 j = src_cols_h ? src_cols_h[k] : k;
        if (j >= table->n_cols) throw HipError(who + "column index " + std::to_string(j) + " is not below n_cols " + std::to_string(table->n_cols));
        if (!out_cols_h[k]) throw HipError(who + "output column " + std::to_string(k) + " is a null pointer");
        if (!repeat && pad_h && pad_h[k] >= P31) throw HipError(who + "pad value " + std::to_string(pad_h[k]) + " of output column " + std::to_string(k) + " is not a canonical M31 value");
        const ByteRange out{(u64)(uintptr_t)out_cols_h[k], col_bytes, "output column " + std::to_string(k)};
        for (const ByteRange& u : used) if (out.overlaps(u)) throw HipError(who + out.name + " overlaps " + u.name);
        used.push_back(out);
        const u64 table_word = col_major ? (u64)(uintptr_t)table->cols_h[j] : (u64)(uintptr_t)(table->rows_d + j);
        cols[k] = RowsCol{table_word, out.base, pad_h && !repeat ? pad_h[k] : 0u, 0};
    }
    c.stage_checkpoint(Ctx::stage_round(sizeof(RowsCol) * n_out) + 256);
    const unsigned long long none = ~0ull;
    RowsArgs a{};
    {
        StageBatch sb(c);
        a.cols = c.stage(cols.data(), n_out);
        a.first_bad = c.stage(&none, 1);
        sb.end();
    }
    a.n_rows = n_rows; a.row_stride = stride; a.log_size = log_size; a.n_cols = n_out; a.repeat_last = repeat;
    rows_launch(c.stream, a, false, col_major);
    BF_HIP(hipGetLastError());
    unsigned long long bad = ~0ull;
    c.read_back(&bad, a.first_bad, sizeof bad);
    if (bad != ~0ull) {
        const u64 row = bad >> 8; const u32 k = (u32)(bad & 255u);
        u32 v = 0;
        c.read_back(&v, (const u32*)(uintptr_t)cols[k].table + row * stride, sizeof v);
        throw HipError(who + "row " + std::to_string(row) + ", column " + std::to_string(k) + ": " + std::to_string(v) + " is not a canonical M31 value");
    }
    return 0;
    API_CATCH
}
int32_t bfhip_rows_from_columns(bfhip_ctx* ctx, const uint32_t* const* cols_h, uint32_t n_cols, uint32_t log_size, uint32_t* rows_d, uint64_t n_rows,
                                uint64_t row_stride, uint32_t reserved) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    const std::string who = "bfhip_rows_from_columns: ";
    if (!cols_h || (n_rows && !rows_d)) throw HipError(who + "null argument");
    if (reserved != 0) throw HipError(who + "reserved must be 0");
    rows_check_shape(who, log_size, n_rows, n_cols, "n_cols");
    if (row_stride < n_cols) throw HipError(who + "row_stride " + std::to_string(row_stride) + " is below n_cols " + std::to_string(n_cols));
    rows_not_sharded(c, who);
    const ByteRange dst{(u64)(uintptr_t)rows_d, n_rows ? (rows_src_offset(n_rows - 1, row_stride, n_cols - 1) + 1) * sizeof(u32) : 0, "the table"};
    std::vector<RowsCol> cols(n_cols);
    for (u32 k = 0; k < n_cols; k++) {
        if (!cols_h[k]) throw HipError(who + "column " + std::to_string(k) + " is a null pointer");
        const ByteRange col{(u64)(uintptr_t)cols_h[k], sizeof(u32) << log_size, "column " + std::to_string(k)};
        if (col.overlaps(dst)) throw HipError(who + col.name + " overlaps " + dst.name);
        cols[k] = RowsCol{(u64)(uintptr_t)(rows_d + k), col.base, 0, 0};
    }
    if (n_rows == 0) return 0;
    c.stage_checkpoint(Ctx::stage_round(sizeof(RowsCol) * n_cols));
    RowsArgs a{};
    a.cols = c.stage(cols.data(), n_cols);
    a.n_rows = n_rows; a.row_stride = row_stride; a.log_size = log_size; a.n_cols = n_cols;
    rows_launch(c.stream, a, true, false);
    BF_HIP(hipGetLastError());
    return 0;
    API_CATCH
}

// ---- filter and sort a row-order table (include/bfhip.h "Row selection"; rows_select.hip, the rules in rows_select.h) ----
int32_t bfhip_rows_select(bfhip_ctx* ctx, const bfhip_rows_table* table, const bfhip_rows_select_desc* sel, uint32_t log_size, const bfhip_select_out* outs_h,
                          uint32_t* const* out_cols_h, uint32_t n_out, uint32_t* order_d, uint64_t* n_selected) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    hipStream_t s = c.stream;
    const std::string who = "bfhip_rows_select: ";
    if (!table || !sel || !n_selected) throw HipError(who + "null argument");
    if (table->reserved != 0) throw HipError(who + "reserved must be 0");
    if (table->layout != BFHIP_ROWS_ROW_MAJOR && table->layout != BFHIP_ROWS_COLUMN_MAJOR) throw HipError(who + "unknown layout " + std::to_string(table->layout));
    if (table->flags & ~uint32_t(BFHIP_ROWS_REPEAT_LAST)) throw HipError(who + "unknown flag bits " + std::to_string(table->flags));
    const bool col_major = table->layout == BFHIP_ROWS_COLUMN_MAJOR, repeat = (table->flags & BFHIP_ROWS_REPEAT_LAST) != 0;
    const u64 n_rows = table->n_rows, stride = col_major ? 1 : table->row_stride;
    if (!col_major && table->row_stride < table->n_cols) throw HipError(who + "row_stride " + std::to_string(table->row_stride) + " is below n_cols " + std::to_string(table->n_cols));
    const SelectPlan plan = select_validate(who, SelectShape{n_rows, table->n_cols, repeat}, sel, log_size, outs_h, n_out, out_cols_h != nullptr, order_d != nullptr);
    if (col_major ? !table->cols_h : (n_rows && !table->rows_d)) throw HipError(who + "null table pointer");
    rows_not_sharded(c, who);
    const u32 n_cand = (u32)plan.n_candidates;
    std::vector<ByteRange> used;      // the source first, then the outputs accepted so far
    if (col_major) {
        for (u32 j = 0; j < table->n_cols; j++) {
            if (n_rows && !table->cols_h[j]) throw HipError(who + "source column " + std::to_string(j) + " is a null pointer");
            used.push_back({(u64)(uintptr_t)table->cols_h[j], n_rows * sizeof(u32), "source column " + std::to_string(j)});
        }
    } else if (n_rows) {
        used.push_back({(u64)(uintptr_t)table->rows_d, (rows_src_offset(n_rows - 1, stride, table->n_cols - 1) + 1) * sizeof(u32), "the source table"});
    }
    auto table_word = [&](u32 j) { return col_major ? (u64)(uintptr_t)table->cols_h[j] : (u64)(uintptr_t)(table->rows_d + j); };
    auto accept = [&](const ByteRange& out) {
        for (const ByteRange& u : used) if (out.overlaps(u)) throw HipError(who + out.name + " overlaps " + u.name);
        used.push_back(out);
    };
    if (order_d) accept({(u64)(uintptr_t)order_d, u64(n_cand) * sizeof(u32), "the order"});
    std::vector<SelectOutDev> outs(n_out);
    for (u32 k = 0; k < n_out; k++) {
        if (!out_cols_h[k]) throw HipError(who + "output column " + std::to_string(k) + " is a null pointer");
        accept({(u64)(uintptr_t)out_cols_h[k], sizeof(u32) << log_size, "output column " + std::to_string(k)});
        outs[k] = SelectOutDev{table_word(outs_h[k].col), (u64)(uintptr_t)out_cols_h[k], outs_h[k].offset, repeat ? 0u : outs_h[k].pad, outs_h[k].col, 0};
    }
    // ---- enqueued from here on ----
    c.stage_checkpoint(Ctx::stage_round(sizeof(SelectOutDev) * n_out) + 256);
    const unsigned long long none = ~0ull;
    SelectSource src{sel->row_begin, stride, nullptr};
    const SelectOutDev* d_outs = nullptr;
    {
        StageBatch sb(c);
        if (n_out) d_outs = c.stage(outs.data(), n_out);
        src.first_bad = c.stage(&none, 1);
        sb.end();
    }
    DeviceScratch scratch(c);
    // (1) flags, positions, the count
    u32 S = 0;
    u32 *flags = nullptr, *pos = nullptr, *tot = nullptr;
    if (n_cand) {
        scratch.alloc(&flags, sizeof(u32) * n_cand); scratch.alloc(&pos, sizeof(u32) * n_cand); scratch.alloc(&tot, sizeof(u32) * (n_cand / 2048 + 3));
        SelectFlagsArgs fa{};
        for (u32 i = 0; i < sel->n_terms; i++) fa.t[i] = SelectTermDev{table_word(sel->terms[i].col), sel->terms[i].op, sel->terms[i].value, sel->terms[i].col, 0};
        fa.src = src; fa.n_terms = sel->n_terms; fa.n = n_cand; fa.flags = flags;
        const u32* d_total;
        {
            ProfScope ps(s, "k_select_flags", 4.0 * double(n_cand) * double(sel->n_terms + 1));
            select_flags_launch(s, fa);
            d_total = exclusive_scan_u32(s, flags, pos, tot, n_cand);
        }
        BF_HIP(hipGetLastError());
        c.read_back(&S, d_total, sizeof S);
    }
    *n_selected = S;
    select_check_count(who, plan, repeat, S, log_size);
    // (2) the permutation: source order, then the key passes
    u32* perm[2] = {nullptr, nullptr};
    int cur = 0;
    const bool want_perm = !plan.count_only || order_d;
    if (S && want_perm) {
        const bool sorted = plan.n_passes != 0;
        scratch.alloc(&perm[0], sizeof(u32) * S);
        select_compact_launch(s, flags, pos, n_cand, perm[0]);
        if (sorted) {
            u64 *keys = nullptr, *keys_sorted = nullptr; void* tmp = nullptr;
            const size_t tmp_bytes = select_sort_tmp_bytes(S);
            scratch.alloc(&perm[1], sizeof(u32) * S);
            scratch.alloc(&keys, sizeof(u64) * S); scratch.alloc(&keys_sorted, sizeof(u64) * S);
            scratch.alloc(&tmp, tmp_bytes + 256);
            ProfScope ps(s, "rows_select_sort", 0);
            for (u32 p = 0; p < plan.n_passes; p++) {
                const bfhip_select_key& lo = sel->keys[plan.lo[p]];
                SelectKeyDev hi_d{0, 0, 0};
                if (plan.hi[p] >= 0) { const bfhip_select_key& hi = sel->keys[plan.hi[p]]; hi_d = SelectKeyDev{table_word(hi.col), hi.col, hi.flags}; }
                select_sort_pass(s, hi_d, SelectKeyDev{table_word(lo.col), lo.col, lo.flags}, src, perm[cur], perm[cur ^ 1], keys, keys_sorted, tmp, tmp_bytes, S);
                cur ^= 1;
            }
        }
        if (order_d) select_order_launch(s, perm[cur], sel->row_begin, S, order_d);
        BF_HIP(hipGetLastError());
    }
    // (3) the columns
    if (!plan.count_only) {
        SelectGatherArgs ga{};
        ga.outs = d_outs; ga.perm = perm[cur]; ga.src = src; ga.n_selected = S; ga.log_size = log_size; ga.n_out = n_out; ga.repeat_last = repeat;
        select_gather_launch(s, ga, col_major);
        BF_HIP(hipGetLastError());
    }
    unsigned long long bad = ~0ull;
    c.read_back(&bad, src.first_bad, sizeof bad);
    if (bad != ~0ull) {
        const u64 row = bad >> SELECT_BAD_COL_BITS; const u32 j = (u32)(bad & ((1u << SELECT_BAD_COL_BITS) - 1));
        u32 v = 0;
        c.read_back(&v, (const u32*)(uintptr_t)table_word(j) + row * stride, sizeof v);
        throw HipError(select_bad_word_message(who, bad, v));
    }
    return 0;
    API_CATCH
}

// ---- insert the missing rows of a row-order table (include/bfhip.h "Row filling"; rows_fill.hip, the rules in rows_fill.h) ----
int32_t bfhip_rows_fill(bfhip_ctx* ctx, const bfhip_rows_table* table, const bfhip_rows_fill_desc* fill, uint32_t log_size, const bfhip_fill_out* outs_h,
                        uint32_t* const* out_cols_h, uint32_t n_out, uint64_t* n_filled) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    hipStream_t s = c.stream;
    const std::string who = "bfhip_rows_fill: ";
    if (!table || !fill || !n_filled) throw HipError(who + "null argument");
    if (table->reserved != 0) throw HipError(who + "reserved must be 0");
    if (table->layout != BFHIP_ROWS_ROW_MAJOR && table->layout != BFHIP_ROWS_COLUMN_MAJOR) throw HipError(who + "unknown layout " + std::to_string(table->layout));
    if (table->flags & ~uint32_t(BFHIP_ROWS_REPEAT_LAST)) throw HipError(who + "unknown flag bits " + std::to_string(table->flags));
    const bool col_major = table->layout == BFHIP_ROWS_COLUMN_MAJOR;
    const u64 n_rows = table->n_rows, stride = col_major ? 1 : table->row_stride;
    if (!col_major && table->row_stride < table->n_cols) throw HipError(who + "row_stride " + std::to_string(table->row_stride) + " is below n_cols " + std::to_string(table->n_cols));
    const FillPlan plan = fill_validate(who, SelectShape{n_rows, table->n_cols, (table->flags & BFHIP_ROWS_REPEAT_LAST) != 0}, fill, log_size, outs_h, n_out, out_cols_h != nullptr);
    if (col_major ? !table->cols_h : !table->rows_d) throw HipError(who + "null table pointer");
    rows_not_sharded(c, who);
    const u32 n = (u32)fill->n_entries;
    std::vector<ByteRange> used;      // the source first, then the order and the outputs accepted so far
    if (col_major) {
        for (u32 j = 0; j < table->n_cols; j++) {
            if (!table->cols_h[j]) throw HipError(who + "source column " + std::to_string(j) + " is a null pointer");
            used.push_back({(u64)(uintptr_t)table->cols_h[j], n_rows * sizeof(u32), "source column " + std::to_string(j)});
        }
    } else {
        used.push_back({(u64)(uintptr_t)table->rows_d, (rows_src_offset(n_rows - 1, stride, table->n_cols - 1) + 1) * sizeof(u32), "the source table"});
    }
    auto table_word = [&](u32 j) { return col_major ? (u64)(uintptr_t)table->cols_h[j] : (u64)(uintptr_t)(table->rows_d + j); };
    if (fill->order_d) used.push_back({(u64)(uintptr_t)fill->order_d, u64(n) * sizeof(u32), "the order"});
    std::vector<FillOutDev> outs(n_out);
    for (u32 k = 0; k < n_out; k++) {
        if (!out_cols_h[k]) throw HipError(who + "output column " + std::to_string(k) + " is a null pointer");
        const ByteRange out{(u64)(uintptr_t)out_cols_h[k], sizeof(u32) << log_size, "output column " + std::to_string(k)};
        for (const ByteRange& u : used) if (out.overlaps(u)) throw HipError(who + out.name + " overlaps " + u.name);
        used.push_back(out);
        const bfhip_fill_out& o = outs_h[k];
        const bool mark = o.kind == BFHIP_FILL_MARK;
        outs[k] = FillOutDev{mark ? 0 : table_word(o.col), out.base, o.kind, o.kind == BFHIP_FILL_KEEP ? 0u : o.value, o.offset, mark ? 0u : o.col,
                             !mark && o.col == fill->step_col ? 1u : 0u, {0, 0, 0}};
    }
    // ---- enqueued from here on ----
    c.stage_checkpoint(Ctx::stage_round(sizeof(FillOutDev) * n_out) + 256);
    const unsigned long long records[3] = {~0ull, ~0ull, 0};      // the bad word, the bad order word, the total
    unsigned long long* d_records;
    const FillOutDev* d_outs = nullptr;
    {
        StageBatch sb(c);
        if (n_out) d_outs = c.stage(outs.data(), n_out);
        d_records = c.stage(records, 3);
        sb.end();
    }
    const FillSource src{fill->order_d, fill->row_begin, stride, d_records, d_records + 1};
    DeviceScratch scratch(c);
    // (0), (1): the order, the counts, the total
    u32 *counts = nullptr, *pos = nullptr, *tot = nullptr;
    u64 T = n;
    if (fill->order_d) fill_order_check_launch(s, fill->order_d, n, n_rows, src.order_bad);
    if (plan.gaps) {
        scratch.alloc(&counts, sizeof(u32) * n);
        FillCountsArgs ca{};
        for (u32 j = 0; j < fill->n_group; j++) { ca.group[j] = table_word(fill->group_cols[j]); ca.group_col[j] = fill->group_cols[j]; }
        ca.step = table_word(fill->step_col); ca.step_col = fill->step_col; ca.n_group = fill->n_group; ca.n = n; ca.src = src; ca.counts = counts; ca.total = d_records + 2;
        ProfScope ps(s, "k_fill_counts", 4.0 * double(n) * double(2 * (fill->n_group + 1) + 1));
        fill_counts_launch(s, ca);
    }
    if (fill->order_d || plan.gaps) {
        BF_HIP(hipGetLastError());
        unsigned long long got[2] = {~0ull, 0};
        c.read_back(got, d_records + 1, sizeof got);
        if (got[0] != ~0ull) throw HipError(fill_bad_order_message(who, got[0] >> 32, (u32)got[0], n_rows));
        if (plan.gaps) T = got[1];
    }
    *n_filled = T;
    fill_check_count(who, plan, T, log_size);
    // (2) the positions and the columns
    if (!plan.count_only) {
        if (plan.gaps) {
            scratch.alloc(&pos, sizeof(u32) * n); scratch.alloc(&tot, sizeof(u32) * (n / 2048 + 3));
            ProfScope ps(s, "rows_fill_scan", 12.0 * double(n));
            exclusive_scan_u32(s, counts, pos, tot, n);
        }
        FillGatherArgs ga{};
        ga.outs = d_outs; ga.pos = pos; ga.src = src; ga.n_entries = n; ga.n_filled = (u32)T; ga.log_size = log_size; ga.n_out = n_out;
        fill_gather_launch(s, ga, col_major);
        BF_HIP(hipGetLastError());
    }
    unsigned long long bad = ~0ull;
    if (!plan.count_only || plan.gaps) c.read_back(&bad, src.first_bad, sizeof bad);
    if (bad != ~0ull) {
        const u64 row = bad >> SELECT_BAD_COL_BITS; const u32 j = (u32)(bad & ((1u << SELECT_BAD_COL_BITS) - 1));
        u32 v = 0;
        c.read_back(&v, (const u32*)(uintptr_t)table_word(j) + row * stride, sizeof v);
        throw HipError(select_bad_word_message(who, bad, v));
    }
    return 0;
    API_CATCH
}

}  // extern "C"
