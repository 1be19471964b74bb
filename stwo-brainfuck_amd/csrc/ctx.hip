// The context's lifecycle (ctx.h: Ctx::init / destroy / ensure_aux / ensure_side). Not ABI: bfhip_ctx_create (api_ctx.hip) and the pool
// (pool.hip) call these.
#include "ctx.h"
#include <algorithm>
#include <vector>

namespace bf {

void Ctx::ensure_aux() { for (auto& a : aux) if (!a) BF_HIP(hipStreamCreateWithFlags(&a, hipStreamNonBlocking)); }
void Ctx::ensure_side() { if (!stream2) BF_HIP(hipStreamCreateWithFlags(&stream2, hipStreamNonBlocking)); }

// A throw anywhere in here leaves a partially built context: the caller (bfhip_ctx_create, pool.hip) lets the destructor run destroy(), which
// releases exactly what exists (r06; before, a failed creation — e.g. out of memory at the twiddle tree — leaked its streams, events, pinned
// buffers and device allocations).
void Ctx::init(int dev, u32 max_log_domain, const Ctx* tables_from) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) throw HipError("no HIP device: the bfhip backend has no CPU fallback");
    if (dev < 0 || dev >= n) throw HipError("bad device id");
    // columns are addressed with 32-bit byte offsets (kernels.h: ld_col): at most 2^29 cells per column
    if (max_log_domain < 6 || max_log_domain > 29) throw HipError("max_log_domain out of range [6, 29]");
    device = dev;
    BF_HIP(hipSetDevice(dev));
    BF_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    id_main = stream;
    if (const char* v = getenv("BFHIP_SYNC")) sync_blocking = v[0] == 'b';
    if (const char* v = getenv("BFHIP_SINGLE_STREAM")) single_stream = atoi(v) != 0;
    if (const char* v = getenv("BFHIP_OVERLAP")) { overlap = (u32)atoi(v) & 7u; overlap_user_set = true; }
    if (const char* v = getenv("BFHIP_MAILBOX")) mailbox_mode = atoi(v) != 0 ? 1 : 0;
    if (const char* v = getenv("BFHIP_MAILBOX_TIMEOUT_MS")) mailbox_timeout = std::max(1, atoi(v)) * 1e-3;
#ifdef BFHIP_TEST_HOOKS      // libbfhip_testhooks.so only (Makefile): the late-host path of the mailboxes needs a host that is late on purpose
    if (const char* v = getenv("BFHIP_MAILBOX_TEST_DELAY_MS")) mailbox_test_delay_ms = std::max(0, atoi(v));
#endif
    if (overlap) ensure_aux();      // the partner streams exist only for contexts that use them (ctx.h: ensure_aux)
    for (auto& e : evp) BF_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto& e : reap_ev) BF_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto& e : ev) BF_HIP(hipEventCreate(&e));
    BF_HIP(hipEventCreateWithFlags(&sync_ev, hipEventDisableTiming));
    BF_HIP(hipEventCreateWithFlags(&block_ev, hipEventDisableTiming | hipEventBlockingSync));
    BF_HIP(hipHostMalloc((void**)&h_stage, stage_bytes));
    BF_HIP(hipHostMalloc((void**)&h_small, h_small_bytes));
    memset(h_small, 0, 4096);       // flags, stamps and the mailbox error word start at zero; proof numbers start at one
    BF_HIP(hipHostGetDevicePointer((void**)&d_small_alias, h_small, 0));
    BF_HIP(hipHostGetDevicePointer((void**)&d_hstage_alias, h_stage, 0));
    BF_HIP(hipMalloc((void**)&d_stage, stage_bytes));
    BF_HIP(hipMalloc((void**)&d_counters, 4 * 64 * sizeof(u32)));
    BF_HIP(hipMemset(d_counters, 0, 4 * 64 * sizeof(u32)));
    tw_root_log = max_log_domain - 1;
    if (tables_from) {
        // sub-context of a pool: the twiddle tree and the point tables are read-only after creation and the same for every context of a device
        if (tables_from->device != dev) throw HipError("shared tables live on another device");
        if (tables_from->tw_root_log < tw_root_log || !tables_from->d_tw) throw HipError("shared twiddle tree is too small");
        owns_tables = false;
        tw_root_log = tables_from->tw_root_log;      // a tree rooted higher serves every smaller domain (the layers nest: SURVEY.md B.2 item 9)
        d_tw = tables_from->d_tw; d_itw = tables_from->d_itw; d_tlo = tables_from->d_tlo; d_thi = tables_from->d_thi;
        return;
    }
    // point tables: G^a and G^(b << 16) for the M31 circle generator G = (2, 1268011823)
    std::vector<uint2> tlo(1 << 16), thi(1 << 15);
    auto mulp = [](uint2 p, uint2 q) { return uint2{m_sub(m_mul(p.x, q.x), m_mul(p.y, q.y)), m_add(m_mul(p.x, q.y), m_mul(p.y, q.x))}; };
    uint2 g{2u, 1268011823u}, cur{1u, 0u};
    for (u32 i = 0; i < (1u << 16); i++) { tlo[i] = cur; cur = mulp(cur, g); }
    uint2 g16 = cur;  // G^(2^16)
    cur = uint2{1u, 0u};
    for (u32 i = 0; i < (1u << 15); i++) { thi[i] = cur; cur = mulp(cur, g16); }
    BF_HIP(hipMalloc((void**)&d_tlo, tlo.size() * sizeof(uint2)));
    BF_HIP(hipMalloc((void**)&d_thi, thi.size() * sizeof(uint2)));
    BF_HIP(hipMemcpy(d_tlo, tlo.data(), tlo.size() * sizeof(uint2), hipMemcpyHostToDevice));
    BF_HIP(hipMemcpy(d_thi, thi.data(), thi.size() * sizeof(uint2), hipMemcpyHostToDevice));
    BF_HIP(hipMalloc((void**)&d_tw, sizeof(u32) << tw_root_log));
    BF_HIP(hipMalloc((void**)&d_itw, sizeof(u32) << tw_root_log));
    gen_twiddles(stream, d_tw, d_itw, tw_root_log, d_tlo, d_thi);
    BF_HIP(hipGetLastError());
    sync();
}

void Ctx::destroy() {
    if (stream || stream2 || h_stage || h_small || d_stage) (void)hipSetDevice(device);      // may run on any thread (a destructor)
    if (stream) (void)hipStreamSynchronize(stream);
    if (stream2) (void)hipStreamSynchronize(stream2);
    preprocessed_cache_drop(*this);      // the kept preprocessed tree: nothing reads it any more, and its memory goes before the streams do
    air_kernels_drop(*this);             // the modules of the constraint kernels compiled at run time; kernel objects still alive are orphaned
    for (auto& a : aux) if (a) { (void)hipStreamSynchronize(a); prof_forget(a); (void)hipStreamDestroy(a); a = nullptr; }
    for (auto& e : evp) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    for (auto& e : reap_ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    shard = ShardGroup();
    shared_pre = nullptr;
    if (stream) prof_forget(stream);
    if (stream2) prof_forget(stream2);
    arena.release();
    auto dfree = [](auto*& p) { if (p) (void)hipFree(p); p = nullptr; };
    dfree(d_counters); dfree(d_stage);
    dfree(d_reserve); reserve.set(0);
    if (owns_tables) { dfree(d_tw); dfree(d_itw); dfree(d_tlo); dfree(d_thi); }
    else d_tw = d_itw = nullptr, d_tlo = d_thi = nullptr;
    if (h_stage) { (void)hipHostFree(h_stage); h_stage = nullptr; }
    if (h_small) { (void)hipHostFree(h_small); h_small = nullptr; }
    d_small_alias = d_hstage_alias = nullptr;
    for (auto& e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    if (sync_ev) { (void)hipEventDestroy(sync_ev); sync_ev = nullptr; }
    if (block_ev) { (void)hipEventDestroy(block_ev); block_ev = nullptr; }
    if (stream2) { (void)hipStreamDestroy(stream2); stream2 = nullptr; }
    if (stream) { (void)hipStreamDestroy(stream); stream = nullptr; }
    id_main = nullptr;
}

}  // namespace bf
