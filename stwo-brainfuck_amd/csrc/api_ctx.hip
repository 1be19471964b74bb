// C ABI (include/bfhip.h): the thread's error string, the devices, a context's creation, settings and getters, and plain device memory.
#include "../../include/bfhip.h"
#include "api_guard.h"

using namespace bf;

static thread_local std::string g_err;
void bfhip_set_error(const std::string& s) { g_err = s; }

extern "C" {

const char* bfhip_last_error(void) { return g_err.c_str(); }

int32_t bfhip_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }

int32_t bfhip_device_memory(int32_t device_id, uint64_t* free_bytes, uint64_t* total_bytes) {
    API_TRY
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) throw HipError("no HIP device: the bfhip backend has no CPU fallback");
    if (device_id < 0 || device_id >= n) throw HipError("bad device id");
    BF_HIP(hipSetDevice(device_id));
    size_t f = 0, t = 0;
    BF_HIP(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return 0;
    API_CATCH
}

int32_t bfhip_ctx_create(int32_t device_id, uint32_t max_log_domain, bfhip_ctx** out) {
    API_TRY
    if (!out) throw HipError("null argument");
    auto* c = new bfhip_ctx();
    try { c->c.init(device_id, max_log_domain); } catch (...) { delete c; throw; }     // ~Ctx releases whatever init() had created
    *out = c;
    return 0;
    API_CATCH
}
int32_t bfhip_ctx_destroy(bfhip_ctx* ctx) { API_TRY if (ctx) ctx->c.refuse_in_session("bfhip_ctx_destroy"); delete ctx; return 0; API_CATCH }
int32_t bfhip_ctx_set_conventions(bfhip_ctx* ctx, const bfhip_conventions* conv) {
    API_CTX(ctx)
    Conventions cv;
    if (conv) {
        if (conv->merkle_node_hash > 1 || conv->mix_u64 > 1 || conv->logup_mask_order > 1 || conv->merkle_channel > 1) throw HipError("unknown convention value");
        cv.merkle_node_hash = conv->merkle_node_hash; cv.mix_u64 = conv->mix_u64; cv.logup_mask_order = conv->logup_mask_order; cv.merkle_channel = conv->merkle_channel;
    }
    ctx->c.refuse_in_session("bfhip_ctx_set_conventions");
    ctx->c.sync();
    // a kept preprocessed tree is keyed on the hasher it was built with (prover.h: PreprocessedCache::matches) and dropped here as well
    if (cv.merkle_node_hash != ctx->c.conv.merkle_node_hash || cv.merkle_channel != ctx->c.conv.merkle_channel) preprocessed_cache_invalidate(&ctx->c);
    ctx->c.conv = cv;
    return 0;
    API_CATCH
}
// pcs_config_from (ctx.h): pcs_host.hip, with the other host-only checks of the commitment scheme's settings
int32_t bfhip_ctx_set_pcs_config(bfhip_ctx* ctx, const bfhip_pcs_config* pcs) {
    API_CTX(ctx)
    PcsConfig cfg = pcs_config_from(pcs);
    if (ctx->c.shard.count > 1 && !cfg.is_default()) throw HipError("bfhip_ctx_set_pcs_config: a context in a shard group keeps the default config");
    ctx->c.refuse_in_session("bfhip_ctx_set_pcs_config");
    ctx->c.sync();
    // a kept preprocessed tree is keyed on the blowup it was built with (prover.h: PreprocessedCache::matches)
    ctx->c.pcs = cfg;
    return 0;
    API_CATCH
}
int32_t bfhip_ctx_get_pcs_config(bfhip_ctx* ctx, bfhip_pcs_config* out) {
    API_CTX(ctx)
    if (!out) throw HipError("null argument");
    bfhip_pcs_config r{};
    r.pow_bits = ctx->c.pcs.pow_bits; r.log_blowup_factor = ctx->c.pcs.log_blowup; r.log_last_layer_degree_bound = ctx->c.pcs.log_last_layer_degree_bound;
    r.n_queries = ctx->c.pcs.n_queries;
    *out = r;
    return 0;
    API_CATCH
}
int32_t bfhip_ctx_set_sync_policy(bfhip_ctx* ctx, int32_t blocking) { API_CTX(ctx) ctx->c.sync_blocking = blocking != 0; return 0; API_CATCH }
int32_t bfhip_ctx_set_mailbox(bfhip_ctx* ctx, int32_t mode, uint32_t timeout_ms, int32_t test_delay_ms) {
    API_CTX(ctx)
    if (mode < -2 || mode > 1) throw HipError("bfhip_ctx_set_mailbox: mode must be -2 (keep), -1, 0 or 1");
    if (mode != -2) ctx->c.mailbox_mode = mode;
    if (timeout_ms) ctx->c.mailbox_timeout = timeout_ms * 1e-3;
#ifdef BFHIP_TEST_HOOKS
    if (test_delay_ms >= 0) ctx->c.mailbox_test_delay_ms = test_delay_ms;
#else
    if (test_delay_ms > 0) throw HipError("bfhip_ctx_set_mailbox: test_delay_ms needs the test-hooks build of the library (libbfhip_testhooks.so)");
#endif
    return 0;
    API_CATCH
}
int32_t bfhip_ctx_set_overlap(bfhip_ctx* ctx, uint32_t mask) {
    API_CTX(ctx)
    if (mask > 7) throw HipError("overlap mask: bit 0 = tree commitment, bit 1 = quotients / FRI first layer, bit 2 = shard-group exchanges");
    ctx->c.sync();
    if (mask) ctx->c.ensure_aux();
    ctx->c.overlap = mask;
    ctx->c.overlap_user_set = true;      // also switches OFF the default exchange overlap of a multi-GPU shard group when bit 2 is clear
    return 0;
    API_CATCH
}
int32_t bfhip_ctx_memory(bfhip_ctx* ctx, uint64_t out[4]) {
    API_CTX(ctx)
    if (!out) throw HipError("null argument");
    uint64_t reserved = 0;
    for (auto& ch : ctx->c.arena.chunks) reserved += ch.size;
    out[0] = reserved; out[1] = ctx->c.arena.peak; out[2] = ctx->c.owns_tables ? (uint64_t)(2 * sizeof(u32)) << ctx->c.tw_root_log : 0;      // a pool's sub-contexts borrow the first one's
    out[3] = ctx->c.arena.total_used;
    return 0;
    API_CATCH
}
int32_t bfhip_ctx_set_scratch_reserve(bfhip_ctx* ctx, uint64_t bytes) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    c.refuse_in_session("bfhip_ctx_set_scratch_reserve");
    c.sync();
    if (!c.reserve.idle()) throw HipError("bfhip_ctx_set_scratch_reserve: a call of this context is using the reserve");
    if (bytes > (uint64_t)SIZE_MAX) throw HipError("bfhip_ctx_set_scratch_reserve: cannot allocate " + std::to_string(bytes) + " bytes");
    if (c.d_reserve) { BF_HIP(hipFree(c.d_reserve)); c.d_reserve = nullptr; }
    c.reserve.set(0);
    if (bytes == 0) return 0;
    if (hipMalloc((void**)&c.d_reserve, (size_t)bytes) != hipSuccess) {
        (void)hipGetLastError();
        c.d_reserve = nullptr;
        throw HipError("bfhip_ctx_set_scratch_reserve: cannot allocate " + std::to_string(bytes) + " bytes (the context now has no reserve)");
    }
    c.reserve.set((size_t)bytes);
    return 0;
    API_CATCH
}
int32_t bfhip_ctx_scratch_stats(bfhip_ctx* ctx, uint64_t out[4]) {
    API_CTX(ctx)
    if (!out) throw HipError("null argument");
    const ScratchReserve& r = ctx->c.reserve;
    out[0] = r.bytes; out[1] = r.high_water; out[2] = r.device_allocs; out[3] = r.served;
    return 0;
    API_CATCH
}
int32_t bfhip_ctx_get_conventions(bfhip_ctx* ctx, bfhip_conventions* out) {
    API_CTX(ctx)
    if (!out) throw HipError("null argument");
    bfhip_conventions r{};
    r.merkle_node_hash = ctx->c.conv.merkle_node_hash; r.mix_u64 = ctx->c.conv.mix_u64; r.logup_mask_order = ctx->c.conv.logup_mask_order; r.merkle_channel = ctx->c.conv.merkle_channel;
    *out = r;
    return 0;
    API_CATCH
}
int32_t bfhip_ctx_sync(bfhip_ctx* ctx) { API_CTX(ctx) ctx->c.sync(); return 0; API_CATCH }

int32_t bfhip_malloc(bfhip_ctx* ctx, size_t bytes, void** out_d) { API_CTX(ctx) BF_HIP(hipSetDevice(ctx->c.device)); BF_HIP(hipMalloc(out_d, bytes ? bytes : 4)); return 0; API_CATCH }
int32_t bfhip_free(bfhip_ctx* ctx, void* p) { API_CTX(ctx) (void)ctx; BF_HIP(hipFree(p)); return 0; API_CATCH }
int32_t bfhip_upload(bfhip_ctx* ctx, void* dst_d, const void* src_h, size_t bytes) {
    API_CTX(ctx) BF_HIP(hipMemcpyAsync(dst_d, src_h, bytes, hipMemcpyHostToDevice, ctx->c.stream)); ctx->c.sync(); return 0; API_CATCH
}
int32_t bfhip_download(bfhip_ctx* ctx, void* dst_h, const void* src_d, size_t bytes) {
    API_CTX(ctx) BF_HIP(hipMemcpyAsync(dst_h, src_d, bytes, hipMemcpyDeviceToHost, ctx->c.stream)); ctx->c.sync(); return 0; API_CATCH
}
int32_t bfhip_memset_zero(bfhip_ctx* ctx, void* dst_d, size_t bytes) { API_CTX(ctx) BF_HIP(hipMemsetAsync(dst_d, 0, bytes, ctx->c.stream)); return 0; API_CATCH }

int32_t bfhip_twiddles(bfhip_ctx* ctx, const uint32_t** tw_d, const uint32_t** itw_d, uint32_t* root_log) {
    API_CTX(ctx) if (!tw_d || !itw_d || !root_log) throw HipError("null argument"); *tw_d = ctx->c.d_tw; *itw_d = ctx->c.d_itw; *root_log = ctx->c.tw_root_log; return 0; API_CATCH
}

}  // extern "C"
